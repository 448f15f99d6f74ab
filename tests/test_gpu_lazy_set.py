"""RegexSet matches on the set's on-demand DFA (host LazyDfa over the set
program, big_dfa.hip lazy_set_kernel): a set whose automaton is past the
eager state budget used to run on the Pike VM; now its batches walk the rows
the host builds as lanes park on them.  Every mask against the oracle's
many_matches_at; last_path() == Path.LAZY_DFA asserts the kernel answered.
Shapes are the smallest that reach each branch: less than a wave, one lane
past a wave, a second 1024-thread block, rows read from global memory past
the LDS-resident ones, forced parking rounds, offset batches, the budget's
Pike VM fallback, the words form of a larger set, and the batches and sets
that keep their paths."""
import ctypes
import functools

import numpy as np
import pytest

import regex_amd as R
from golden_data import corpus
from lazy_set_sim import FLAGS, NO_DFA
from oracle_py import OracleRegex
from regex_amd import Path
from regex_amd import _native as N
from regex_amd.workloads import log_lines_host
from set_long_data import CASES, MIXED

pytestmark = pytest.mark.gpu

ORDINARY = {"flags": FLAGS, "mixed": MIXED, "literals": CASES["literals"][0],
            "c4_ascii_wb": CASES["c4_ascii_wb"][0], "set130_group2": CASES["set130_group2"][0]}


@functools.lru_cache(maxsize=None)
def _sources():
    return corpus("sherlock"), bytes(log_lines_host(400, seed=0x5E7, lo=100, hi=100)[0])


def _mixed(nbytes, seed, which=0, runs=40):
    """Pieces of sherlock text (which=0) or log lines (1) with runs of a/b of
    1 to `runs` bytes for a third of the pieces."""
    rng = np.random.default_rng(seed)
    base = _sources()[which]
    out = bytearray()
    while len(out) < nbytes:
        if rng.integers(0, 3) == 0:
            out += bytes(rng.choice(np.frombuffer(b"ab", dtype=np.uint8), size=int(rng.integers(1, runs + 1))))
        else:
            a = int(rng.integers(0, len(base) - 100))
            out += base[a:a + int(rng.integers(1, 100))]
    return bytes(out[:nbytes])


def _mask(o, t, start=0):
    return sum(1 << j for j in o.matches(t, start)) if start <= len(t) else 0


def _u64(x):
    return int(x) & ((1 << 64) - 1)


def _dev(cuda, raw, pad=16):
    import torch
    return torch.from_numpy(np.frombuffer(raw + b"\0" * pad, dtype=np.uint8).copy()).to(cuda)


def _info(rs):
    return rs.lazy_tables()[0]


@pytest.mark.parametrize("start", [0, 3])
def test_past_the_budget(cuda, knobs, start):
    """The set without a DFA under big=2 (any batch size), fixed stride."""
    L = 200
    rs = R.RegexSet(NO_DFA)
    assert not rs.uses_dfa()
    o = OracleRegex(rs)
    raw = _mixed(1100 * L, 21 + start)
    dev = _dev(cuda, raw)
    knobs(big=2)
    for count in (1, 3, 65, 1100):
        got = rs.matches_batch(dev, stride=L, length=L, count=count, start=start).cpu().numpy()
        assert N.last_path() == Path.LAZY_DFA, count
        assert R.RegexSet.last_long_units() == (0, 0, 0)
        exp = [_mask(o, raw[i * L:(i + 1) * L], start) for i in range(count)]
        assert [_u64(g) for g in got] == exp, count
        if count >= 65:
            assert 0 < sum(e & 1 for e in exp) < count
    info = _info(rs)
    assert info["fell_back"] == 0 and info["rounds"] >= 1
    # rows past the LDS-resident ones are read from global memory (a/b runs
    # of up to 40 bytes suffice: thousands of distinct 18-byte windows)
    assert info["states"] > info["hot_rows"] and info["rows_built"] > info["hot_rows"]
    assert not rs.uses_dfa()


@pytest.mark.parametrize("name", sorted(ORDINARY))
def test_forced_rounds(cuda, knobs, name):
    """lazy=1, lazy_rows=1 over sets that have an eager DFA: one row built
    ahead per round, so every lane parks and resumes with its mask."""
    n, L = 300, 150
    rs = R.RegexSet(ORDINARY[name])
    o = OracleRegex(rs)
    raw = _mixed(n * L, len(name), which=1)
    knobs(lazy=1, lazy_rows=1)
    got = rs.matches_batch(_dev(cuda, raw), stride=L, length=L, count=n).cpu().numpy()
    assert N.last_path() == Path.LAZY_DFA
    info = _info(rs)
    assert info["rounds"] > 1 and info["fell_back"] == 0
    exp = [_mask(o, raw[i * L:(i + 1) * L]) for i in range(n)]
    assert [_u64(g) for g in got] == exp
    assert len(set(exp)) > 1


def test_offsets(cuda, knobs):
    """About 500 haystacks cut at random from 60000 bytes, empty ones among
    them, the last ending in the buffer's last 16-byte block; the bytes before
    the first and after the last haystack would match."""
    import torch
    rs = R.RegexSet(NO_DFA)
    o = OracleRegex(rs)
    rng = np.random.default_rng(11)
    total, lo, hi = 60000, 37, 60000 - 5
    assert total % 16 == 0 and total - hi < 16
    run = b"a" * 19 + b"bb"
    text = bytearray(_mixed(total, 3))
    text[:lo] = (run * 3)[:lo]
    text[lo - 1:lo] = b"a"  # an `a` before the first haystack: `^a` must not see it
    text[hi:] = b"bbbbb"
    text = bytes(text)
    cuts = np.sort(rng.integers(lo, hi, size=498))
    cuts[100] = cuts[101]  # (empty haystacks whatever the draw)
    offs = np.concatenate([[lo], cuts, [hi]]).astype(np.int64)
    assert (np.diff(offs) == 0).any()
    dev = _dev(cuda, text, pad=0)
    assert dev.numel() == total
    knobs(big=2)
    got = rs.matches_batch(dev, offsets=torch.from_numpy(offs).to(cuda)).cpu().numpy()
    assert N.last_path() == Path.LAZY_DFA
    exp = [_mask(o, text[offs[i]:offs[i + 1]]) for i in range(len(offs) - 1)]
    assert [_u64(g) for g in got] == exp
    assert len(set(exp)) > 2
    # the surroundings would have changed the answers
    assert _mask(o, text[lo - 1:offs[1]]) != exp[0] or _mask(o, text[offs[-2]:]) != exp[-1]


def test_second_call_reuses_the_table(cuda, knobs):
    n, L = 300, 200
    rs = R.RegexSet(NO_DFA)
    dev = _dev(cuda, _mixed(n * L, 7))
    knobs(big=2)
    first = rs.matches_batch(dev, stride=L, length=L, count=n).cpu().numpy()
    a = _info(rs)
    second = rs.matches_batch(dev, stride=L, length=L, count=n).cpu().numpy()
    b = _info(rs)
    assert N.last_path() == Path.LAZY_DFA
    assert a["rounds"] > 1 and b["rounds"] == 1
    assert b["rows_built"] == a["rows_built"] and b["states"] == a["states"]
    assert np.array_equal(first, second)


def test_budget_falls_back(cuda, knobs):
    """A few KiB of budget: the Pike VM answers the whole batch."""
    n, L = 300, 200
    raw = _mixed(n * L, 9)
    knobs(big=2, big_bytes=4096)
    rs = R.RegexSet(NO_DFA)
    o = OracleRegex(rs)
    got = rs.matches_batch(_dev(cuda, raw), stride=L, length=L, count=n).cpu().numpy()
    assert N.last_path() == Path.PIKE_ONLY
    info = _info(rs)
    assert info["fell_back"] == 1 and info["rows_built"] < info["states"]
    assert [_u64(g) for g in got] == [_mask(o, raw[i * L:(i + 1) * L]) for i in range(n)]


def test_words_form(cuda, knobs):
    """67 patterns: a group of 64 words with a DFA, and the three patterns
    without one as the second group, through
    rure_amd_set_matches_batch_words on a small batch."""
    import torch
    words = sorted(set(w for w in corpus("sherlock")[:40000].decode("ascii", "ignore").split()
                       if w.isalpha() and w.islower() and len(w) >= 4))[:64]
    assert len(words) == 64
    pats = words + NO_DFA
    rs = R.RegexSet(pats)
    assert len(rs) == 67 and not rs.uses_dfa()
    n, L = 70, 200
    raw = _mixed(n * L, 13)
    out = torch.full((n, 3), -5, dtype=torch.int64, device=cuda)
    dev = _dev(cuda, raw)
    b = R._batch(dev, stride=L, length=L, count=n)
    knobs(big=2)
    assert N.rure_amd_set_matches_batch_words(rs._set, ctypes.byref(b), ctypes.c_void_p(out.data_ptr()), 3,
                                              R._stream_ptr(None)) == N.OK
    assert N.last_path() == Path.LAZY_DFA  # (the last group's)
    got = out.cpu().numpy().view(np.uint64)
    o0, o1 = OracleRegex(R.RegexSet(words)), OracleRegex(R.RegexSet(NO_DFA))
    seen = [0, 0]
    for i in range(n):
        t = raw[i * L:(i + 1) * L]
        e = (_mask(o0, t), _mask(o1, t))
        assert (int(got[i, 0]), int(got[i, 1]), int(got[i, 2])) == (e[0], e[1], 0), i
        seen = [seen[0] | e[0], seen[1] | e[1]]
    assert seen[0] and seen[1] == 7


def test_kept_paths(cuda, knobs):
    """A set with a Unicode `\\b` member under lazy=1, the set without a DFA
    under lazy=0 and on a small batch with no knob: none takes the on-demand
    DFA, all answer right."""
    n, L = 64, 200
    raw = _mixed(n * L, 17)
    dev = _dev(cuda, raw)
    # (the `\b` set last: its DFA kernel notes no path, so what the check
    # reads there is that the on-demand DFA did not overwrite the one before)
    for pats, kn, path in ((NO_DFA, dict(lazy=0, big=2), Path.PIKE_ONLY),
                           (NO_DFA, dict(big=0), Path.PIKE_ONLY),
                           (NO_DFA, {}, Path.PIKE_ONLY),
                           ([r"\bthe\b", r"bb", r"^a"], dict(lazy=1), None)):
        rs = R.RegexSet(pats)
        o = OracleRegex(rs)
        knobs(**kn)
        got = rs.matches_batch(dev, stride=L, length=L, count=n).cpu().numpy()
        assert N.last_path() != Path.LAZY_DFA and (path is None or N.last_path() == path), (pats, kn)
        exp = [_mask(o, raw[i * L:(i + 1) * L]) for i in range(n)]
        assert [_u64(g) for g in got] == exp, (pats, kn)
        assert len(set(exp)) > 1
