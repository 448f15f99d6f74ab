"""find_iter on the on-demand forward DFA (host LazyDfa, big_dfa.hip
lazy_iter_kernel): one lane per haystack runs the whole iteration of
re_trait.rs:197-221, parks on rows not built yet and resumes inside the
search it left; the count form runs in rounds, the write form once.
`(?:a|b)*a(?:a|b){20}` has ~2^21 states, past the eager budgets, and used to
iterate on the Pike VM (Path.ITER_WAVE); knobs lazy=1, lazy_rows=1 force
ordinary regexes through many parking rounds.  Counts, records in haystack
order and the total are the oracle's, bit for bit; last_path() ==
Path.LAZY_DFA asserts the kernel answered.  split, replace, captures_iter
(the match list) and captures (its bounds) ride on it."""
import ctypes
import functools

import numpy as np
import pytest

import regex_amd as R
from regex_amd import Path
from regex_amd import _native as N
from oracle_py import OracleRegex
import replace_ref as RR
from lazy_iter_sim import HUGE, LOOKS, PLAIN
from test_gpu_lazy import _mixed

pytestmark = pytest.mark.gpu

N1, L1 = 400, 200
GROUPED = r"((?:a|b)*a)((?:a|b){20})"


def _dev(cuda, raw, pad=16):
    import torch
    return torch.from_numpy(np.frombuffer(raw + b"\0" * pad, dtype=np.uint8).copy()).to(cuda)


def _pairs(t):
    return [tuple(x) for x in t.cpu().numpy().tolist()]


def _per_haystack(counts, rows):
    out, at = [], 0
    for c in counts.cpu().numpy().tolist():
        out.append(rows[at:at + c])
        at += c
    assert at == len(rows)
    return out


def _texts(raw, n, L):
    return [raw[i * L:(i + 1) * L] for i in range(n)]


@functools.lru_cache(maxsize=None)
def _case1(start):
    """The haystacks of the huge-regex case and the oracle's matches of each."""
    raw = _mixed(N1, L1, 5)
    o = OracleRegex(R.Regex(HUGE))
    return raw, [o.find_iter(t, start) for t in _texts(raw, N1, L1)]


def _iter_equals(re, dev, exp, **where):
    """One call (the capacity holds the expected matches and one more, so the
    wrapper does not run a second pass over rows the first one built)."""
    counts, ms = re.find_iter_batch(dev, capacity=sum(len(e) for e in exp) + 1, **where)
    path = N.last_path()
    assert counts.cpu().numpy().tolist() == [len(e) for e in exp]
    assert _per_haystack(counts, _pairs(ms)) == exp
    return path


@pytest.mark.parametrize("start", [0, 3])
def test_huge(cuda, knobs, start):
    """past the eager budgets: the on-demand DFA, not the Pike VM"""
    raw, exp = _case1(start)
    hit = sum(1 for e in exp if e)
    assert 0 < hit < N1 and any(len(e) >= 2 for e in exp)
    knobs(big=2)
    re = R.Regex(HUGE)
    assert _iter_equals(re, _dev(cuda, raw), exp, stride=L1, length=L1, count=N1, start=start) == Path.LAZY_DFA
    info = re.lazy_tables()[0]
    assert info["rounds"] >= 1 and info["fell_back"] == 0 and 0 < info["rows_built"] < info["states"]


@pytest.mark.parametrize("pat", [HUGE] + PLAIN + LOOKS)
def test_forced_rounds(cuda, knobs, pat):
    """one row built ahead per round: every lane parks many times, inside
    searches that are not the haystack's first"""
    n, L = 300, 150
    raw = _mixed(n, L, len(pat))
    re = R.Regex(pat)
    o = OracleRegex(re)
    exp = [o.find_iter(t) for t in _texts(raw, n, L)]
    knobs(lazy=1, lazy_rows=1)
    path = _iter_equals(re, _dev(cuda, raw), exp, stride=L, length=L, count=n)
    if re.match_info()["match_type"] == "Dfa":  # (literal / suffix match types run their own engines)
        assert path == Path.LAZY_DFA, pat
        info = re.lazy_tables()[0]
        assert info["rounds"] > 1 and info["fell_back"] == 0, pat


def test_offsets(cuda, knobs):
    """60000 bytes cut at 500 random places, empty haystacks among them, from
    a base that is not 16-byte aligned"""
    import torch
    rng = np.random.default_rng(11)
    text = _mixed(1, 60000, 3)
    cuts = np.sort(rng.integers(0, len(text), size=500))
    cuts[100] = cuts[101]  # (empty haystacks whatever the draw)
    offs = np.concatenate([[0], cuts, [len(text)]]).astype(np.int64)
    assert len(offs) == 502 and (np.diff(offs) == 0).any()
    dev = _dev(cuda, b"a" + text)[1:]
    assert dev.data_ptr() % 16 == 1
    re = R.Regex(HUGE)
    o = OracleRegex(re)
    exp = [o.find_iter(text[offs[i]:offs[i + 1]]) for i in range(len(offs) - 1)]
    assert sum(len(e) for e in exp) > 10
    knobs(big=2)
    assert _iter_equals(re, dev, exp, offsets=torch.from_numpy(offs).to(cuda)) == Path.LAZY_DFA


def test_capacity(cuda, knobs):
    """counts and total stay exact, min(total, capacity) records are written
    and nothing at or past the capacity"""
    import torch
    raw, exp = _case1(0)
    flat = [m for e in exp for m in e]
    total = len(flat)
    assert total > 2
    dev = _dev(cuda, raw)
    b = R._batch(dev, stride=L1, length=L1, count=N1)
    re = R.Regex(HUGE)
    knobs(big=2)
    for cap in (0, 1, total - 1):
        counts = torch.full((N1,), -7, dtype=torch.int64, device=cuda)
        out = torch.full((total + 2, 2), -7, dtype=torch.int64, device=cuda)
        tot = torch.full((1,), -7, dtype=torch.int64, device=cuda)
        rc = N.rure_amd_find_iter_batch(re._re, ctypes.byref(b), ctypes.c_void_p(counts.data_ptr()),
                                        ctypes.c_void_p(out.data_ptr()), cap, ctypes.c_void_p(tot.data_ptr()),
                                        R._stream_ptr(None))
        torch.cuda.synchronize()
        assert rc == N.OK and N.last_path() == Path.LAZY_DFA
        assert int(tot.item()) == total and counts.cpu().numpy().tolist() == [len(e) for e in exp], cap
        rows = _pairs(out)
        assert rows[:cap] == flat[:cap], cap
        assert all(r == (-7, -7) for r in rows[cap:]), cap


def test_budget_falls_back(cuda, knobs):
    """A few KiB of budget: the Pike VM iterates the whole batch."""
    raw, exp = _case1(0)
    knobs(big=2, big_bytes=4096)
    re = R.Regex(HUGE)
    assert _iter_equals(re, _dev(cuda, raw), exp, stride=L1, length=L1, count=N1) == Path.ITER_WAVE
    info = re.lazy_tables()[0]
    assert info["fell_back"] == 1 and info["rows_built"] < info["states"]


def test_kept_paths(cuda, knobs):
    """lazy=0 keeps the Pike VM; a regex with an eager DFA keeps its chunked
    engine with no knob set; a Unicode word boundary keeps its engine under
    lazy=1."""
    raw, exp = _case1(0)
    dev = _dev(cuda, raw)
    where = dict(stride=L1, length=L1, count=N1)
    knobs(lazy=0, big=2)
    assert _iter_equals(R.Regex(HUGE), dev, exp, **where) == Path.ITER_WAVE
    for pat, kn in ((r"\d{4}-\d{2}-\d{2}|[a-z]+ing", {}), (r"\bthe\b", dict(lazy=1))):
        re = R.Regex(pat)
        assert re.uses_dfa()
        o = OracleRegex(re)
        e = [o.find_iter(t) for t in _texts(raw, N1, L1)]
        assert sum(len(x) for x in e) > 0
        knobs(lazy=0)
        before = _iter_equals(re, dev, e, **where)
        knobs(**kn)
        assert _iter_equals(re, dev, e, **where) == before, pat
        assert before != Path.LAZY_DFA and (kn or before != Path.ITER_WAVE), pat


def test_consumers(cuda, knobs):
    """captures (its bounds), captures_iter, split and replace (their match
    list) of the huge regex with groups; no scratch block outlives a call"""
    import torch
    raw, _ = _case1(0)
    n = 200
    texts = _texts(raw, n, L1)
    dev = _dev(cuda, raw)
    where = dict(stride=L1, length=L1, count=n)
    re = R.Regex(GROUPED)
    assert not re.uses_dfa() and re.captures_len() == 3
    o = OracleRegex(re)
    names = re.capture_names()
    knobs(big=2)

    def settled():
        torch.cuda.synchronize()
        return R.scratch_stats()["live"]

    def groups(row):
        g = [None if a < 0 or b < 0 else (a, b) for a, b in row]
        return None if g[0] is None else g

    def outputs(out, ooff):
        ob, oo = bytes(out.cpu().numpy()), ooff.cpu().numpy().tolist()
        return [ob[oo[i]:oo[i + 1]] for i in range(n)]

    assert settled() == 0
    got = re.captures_batch(dev, **where).cpu().numpy().tolist()
    assert settled() == 0
    exp = [o.captures(t) for t in texts]
    assert [groups(r) for r in got] == exp
    assert 0 < sum(1 for e in exp if e) < n
    counts, ms = re.find_iter_batch(dev, **where)
    assert N.last_path() == Path.LAZY_DFA and settled() == 0
    assert _per_haystack(counts, _pairs(ms)) == [o.find_iter(t) for t in texts]
    counts, rows, _ = re.captures_iter_batch(dev, **where)
    assert settled() == 0
    assert _per_haystack(counts, [groups(r) for r in rows.cpu().numpy().tolist()]) == \
        [RR.captures_iter(o, t) for t in texts]
    counts, pieces = re.split_batch(dev, **where)
    assert settled() == 0
    assert [[t[a:b] for a, b in p] for t, p in zip(texts, _per_haystack(counts, _pairs(pieces)))] == \
        [RR.split(o, t) for t in texts]
    out, ooff = re.replace_batch(dev, b"<$2>", **where)
    assert settled() == 0
    assert outputs(out, ooff) == [RR.replacen(o, names, t, 0, b"<$2>", True) for t in texts]
    out, ooff = re.replace_batch(dev, b"<$2>", expand=True, **where)
    assert settled() == 0
    assert outputs(out, ooff) == [RR.replacen(o, names, t, 0, b"<$2>", False) for t in texts]
    assert re.lazy_tables()[0]["fell_back"] == 0
