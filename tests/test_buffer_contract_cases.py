"""The inputs of tests/test_gpu_buffer_contract.py, checked with the oracle
alone (no GPU): every case of the table has enough matches for its cut set
to mean something, the Arena leaves the haystack bytes alone whatever
surrounds them, and the expected values depend on those bytes only."""
import numpy as np
import pytest

import regex_amd as R
import buffer_contract as BC
from oracle_py import OracleRegex
import replace_ref as RR


@pytest.mark.parametrize("case", BC.CASES, ids=[c.name for c in BC.CASES])
def test_case_has_enough_matches(case):
    """T >= 4200 for the lexer (kGrpWin = 4096 records per window), >= 600
    for the run engine (kRunWin = 256), >= 40 otherwise; a unit with more
    than 4 records (the emit pass copies up to 4 per lane, larger units by
    the wave) and one with none.  anchored_rev has at most one record per
    haystack by construction: its units hold 0 or 1."""
    hays, counts, rows = BC.expected(case)
    T = int(counts.sum())
    assert len(rows) == T
    assert T >= {"lex": 4200, "run": 600}.get(case.kind, 40), T
    uc = BC.unit_counts(case, hays, counts, rows)
    assert sum(uc) == T
    assert min(uc) == 0, "no empty unit"
    if case.dense:
        assert max(uc) > 4, max(uc)
    else:
        assert max(uc) == 1
    if case.kind == "run":
        assert max(uc) > 257  # a unit that spans more than one record window
    pts = BC.cut_points(case, hays, counts, rows)
    assert {0, 1, T - 1, T, T + 1} <= set(pts) and len(pts) >= 10
    if not case.ragged:
        assert len(hays) == case.count and all(len(h) == case.L for h in hays)
        assert case.L <= 512 * 1024


def test_multi_case_has_enough_matches():
    text = BC.multi_text()
    assert len(text) <= 512 * 1024
    for p in BC.MULTI_PATS:
        assert len(OracleRegex(R.Regex(p)).find_iter(text)) >= 40, p


def _some_hays():
    rng = np.random.default_rng(1)
    return [bytes(rng.integers(0, 256, size=n, dtype=np.uint8)) for n in (37,) * 5], \
           [bytes(rng.integers(0, 256, size=n, dtype=np.uint8)) for n in (48,) * 4]


@pytest.mark.parametrize("fill", BC.FILLS)
@pytest.mark.parametrize("k", BC.KS)
def test_arena_layout(fill, k):
    """The haystack bytes read back are the same under every fill and base
    misalignment; every other byte is the fill's; the pads are as large as
    promised and every aligned block of a haystack lies inside the buffer."""
    for hays in _some_hays():
        L = len(hays[0])
        for S in (L, L + 5):
            a = BC.Arena(hays, k=k, stride=S, fill=fill)
            t = a.tensor()
            assert t.numel() % 16 == 0 and a.hay().data_ptr() - t.data_ptr() == BC.FRONT + k
            assert [a.read(i) for i in range(len(hays))] == hays
            assert a.begin >= 64 and t.numel() - a.end >= 64
            assert (a.begin & ~15) >= 16 and ((a.end + 15) & ~15) <= t.numel()
            host = a.host.copy()
            own = np.zeros(len(host), dtype=bool)
            for i in range(len(hays)):
                own[a.begin + i * S:a.begin + i * S + L] = True
            if fill != "self":
                assert (host[~own] == BC._FILL_BYTE[fill]).all()
            else:
                for i, h in enumerate(hays):  # what follows haystack i is its own beginning
                    g0 = a.begin + i * S + L
                    g1 = a.begin + (i + 1) * S if i + 1 < len(hays) else len(host)
                    assert bytes(host[g0:g1]) == (h * (1 + (g1 - g0) // L))[:g1 - g0]
                assert bytes(host[:a.begin]) == (hays[0] * (2 + a.begin // L))[-a.begin:]


def test_arena_offsets():
    hays = _some_hays()[1]
    a = BC.Arena(hays, k=3)
    assert a.offsets().tolist() == [0, 48, 96, 144, 192]


def test_expected_ignores_the_surroundings():
    """The expected value of a haystack is the oracle's answer on the bytes
    read back from the arena: the same under every fill (trivially: the
    oracle never sees the surroundings)."""
    case = BC.CASE_BY_NAME["looks"]
    hays, counts, rows = BC.expected(case)
    o = OracleRegex(R.Regex(case.pat))
    for fill in BC.FILLS:
        a = BC.Arena(hays, k=15, stride=case.L + 5, fill=fill)
        c, r = BC.oracle_rows(o, [a.read(i) for i in range(a.n)])
        assert np.array_equal(c, counts) and np.array_equal(r, rows), fill


@pytest.mark.parametrize("pat", [r"[ \t]+", r"a*", r"", r"x|yz"])
def test_reference_helpers(pat):
    """split_spans and replace_marked are replace_ref's split / splitn /
    replacen, as offsets and with the replacement bytes marked."""
    from test_gpu_replace import _texts
    o = OracleRegex(R.Regex(pat))
    for t in _texts(7, 60, 40):
        ms = o.find_iter(t)
        for limit in (None, 0, 1, 2, 3, 50):
            exp = RR.split(o, t) if limit is None else RR.splitn(o, t, limit)
            assert [t[a:b] for a, b in BC.split_spans(ms, len(t), limit)] == exp, (pat, t, limit)
        for limit in (0, 1, 2):
            out, mark = BC.replace_marked(t, ms, [b"<->"] * len(ms), limit)
            assert out == RR.replacen(o, None, t, limit, b"<->", True)
            assert len(mark) == len(out) and mark.count(b"\1") == 3 * (min(len(ms), limit) if limit else len(ms))


def test_byte_cut_points():
    mark = b"\0" * 40 + b"\1" * 3 + b"\0" * 30
    pts = BC.byte_cut_points(len(mark), mark)
    assert {0, 1, 15, 16, 17, 72, 73, 74} <= set(pts)
    assert any(40 < p < 43 for p in pts) and 55 in pts  # inside "\1\1\1"; inside the text-only block at 48
