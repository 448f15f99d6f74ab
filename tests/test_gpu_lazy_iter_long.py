"""find_iter over few long haystacks on the on-demand forward DFA (big_dfa.hip
lazy_iter_long_kernel and the resolve kernels, dispatch.cpp
run_lazy_iter_long): a regex past the eager state budgets,
`(?:a|b)*a(?:a|b){20}`, used to iterate one long haystack on the Pike VM, a
wave per haystack (Path.ITER_WAVE).  Now the iteration is cut into units:
every unit iterates from its own start, the units a match reaches into
iterate again from where it ends, and a resolve step settles each unit's
true entry.  Forced onto 5000-byte haystacks with 16-, 48- and 4096-byte units
(knobs lazy_iter_long=2, lazy_chunk; ordinary regexes under lazy=1,
lazy_rows=1 park on nearly every row and link), by the production rule on
1 MiB, through split / replace / captures_iter, and the batches that keep
their paths.  Counts, records in haystack order and the total are the
oracle's; last_path() == Path.LAZY_DFA, units > haystacks and fell_back == 0
assert that the chunked kernels gave them.  The repaired units and the resume
passes are those of the CPU simulation (tests/lazy_iter_long_sim.py), which
also shows (tests/test_lazy_iter_long_host.py) that these inputs stay below
the 256 rounds and 64 resume passes at which a batch is given up."""
import ctypes
import functools

import numpy as np
import pytest

import regex_amd as R
from regex_amd import Path
from regex_amd import _native as N
from oracle_py import OracleRegex
import replace_ref as RR
import lazy_iter_long_sim as S
from lazy_long_sim import LongTables
from test_gpu_lazy_iter import _pairs, _per_haystack
from test_gpu_lazy_long import COUNT, HUGE, L, MIB, STRIDE, _dev, _mib, _small, _unit_bytes
from test_lazy_iter_long_host import EMPTY, FIXED, HUGE_LAZY, PLAIN, run_text

pytestmark = pytest.mark.gpu

GROUPED = r"((?:a|b)*)a((?:a|b){20})"
ZERO = dict(units=0, haystacks=0, chunk=0, rounds=0, repaired=0, resume_passes=0, fell_back=0)


def _iter(re, dev, exp, **where):
    """One call (the capacity holds the expected matches and one more, so the
    wrapper does not run a second pass); the path that answered."""
    counts, ms = re.find_iter_batch(dev, capacity=sum(len(e) for e in exp) + 1, **where)
    path = N.last_path()
    assert counts.cpu().numpy().tolist() == [len(e) for e in exp]
    assert _per_haystack(counts, _pairs(ms)) == exp
    return path


def _chunked(haystacks, chunk=None):
    """The last call ran the chunked kernels to the end."""
    info = R.Regex.last_lazy_iter_long()
    assert N.last_path() == Path.LAZY_DFA
    assert info["haystacks"] == haystacks and info["units"] > haystacks and info["fell_back"] == 0
    assert chunk is None or info["chunk"] == chunk
    return info


@functools.lru_cache(maxsize=None)
def _sim(pat, chunk, start):
    """What the CPU simulation needs for the small haystacks (no row built
    ahead: an upper bound of the rounds a pass takes on the device)."""
    got, info = S.lazy_iter_long(LongTables(R.Regex(pat)), _small()[1], start, chunk)
    assert got is not None, (pat, chunk, start, info)
    return info


@pytest.mark.parametrize("pat", [HUGE] + PLAIN + EMPTY)
def test_forced_units(cuda, knobs, pat):
    """3 haystacks of 5000 bytes, stride 5003, one byte past an aligned base,
    in units of 16, 48 and 4096 bytes from starts 0 and 3"""
    raw, texts = _small()
    dev = _dev(cuda, raw, 1)
    re = R.Regex(pat)
    o = OracleRegex(re)
    dfa_type = re.match_info()["match_type"] == "Dfa"  # (literal / suffix match types run their own engines)
    forced = {} if pat == HUGE else dict(lazy=1, lazy_rows=1)
    hits = 0
    for chunk in (16, 48, 4096):
        for start in (0, 3):
            exp = [o.find_iter(t, start) for t in texts]
            knobs(lazy_iter_long=2, lazy_chunk=chunk, **forced)
            path = _iter(re, dev, exp, stride=STRIDE, length=L, count=COUNT, start=start)
            if dfa_type:
                assert path == Path.LAZY_DFA
                info = _chunked(COUNT, chunk)
                want = _sim(pat, chunk, start)
                assert info["units"] == COUNT * -(-(L - start) // chunk) == want["units"]
                assert (info["repaired"], info["resume_passes"]) == (want["repaired"], want["resume_passes"])
                assert 0 < info["rounds"] < 256 * (2 + info["resume_passes"])
                if pat == HUGE and chunk == 16:
                    assert info["repaired"] > 0  # 39-byte runs cross 16-byte cuts
            hits += sum(len(e) for e in exp)
    assert hits > 0


def test_resume_passes(cuda, knobs):
    """a fixed-length match through a 200-byte run: the walker asks for unit
    after unit"""
    text = run_text(200)
    dev = _dev(cuda, text, 1)
    for pat, forced in ((FIXED, dict(lazy=1, lazy_rows=1)), (HUGE_LAZY, {})):
        re = R.Regex(pat)
        exp = [OracleRegex(re).find_iter(text)]
        assert len(exp[0]) > 5
        knobs(lazy_iter_long=2, lazy_chunk=16, **forced)
        assert _iter(re, dev, exp, stride=len(text), length=len(text), count=1) == Path.LAZY_DFA
        info = _chunked(1, 16)
        assert 1 <= info["resume_passes"] <= 64 and info["repaired"] > info["resume_passes"]


def _settled():
    import torch
    torch.cuda.synchronize()
    return R.scratch_stats()["live"]


def test_falls_back(cuda, knobs):
    """through a 5000-byte run the resolve step would need more than 64
    passes: the batch is given up and the engines below answer, the Pike VM
    for the regex without an eager DFA"""
    text = run_text(5000)
    dev = _dev(cuda, text, 1)
    where = dict(stride=len(text), length=len(text), count=1)
    assert _settled() == 0
    re = R.Regex(HUGE_LAZY)
    assert not re.uses_dfa()
    exp = [OracleRegex(re).find_iter(text)]
    assert len(exp[0]) > 100
    knobs(lazy_iter_long=2, lazy_chunk=16)
    assert _iter(re, dev, exp, **where) == Path.ITER_WAVE
    info = R.Regex.last_lazy_iter_long()
    assert info["fell_back"] == 1 and info["resume_passes"] == 65 and info["units"] > 1
    assert _settled() == 0


def test_falls_back_to_the_eager_dfa(cuda, knobs):
    """... and the chunked engine for the fixed-length regex, which has one"""
    text = run_text(5000)
    dev = _dev(cuda, text, 1)
    where = dict(stride=len(text), length=len(text), count=1)
    re = R.Regex(FIXED)
    exp = [OracleRegex(re).find_iter(text)]
    knobs(lazy_iter_long=2, lazy_chunk=16, lazy=1)
    assert _iter(re, dev, exp, **where) != Path.LAZY_DFA
    assert R.Regex.last_lazy_iter_long()["fell_back"] == 1 and _settled() == 0


def test_budget_falls_back(cuda, knobs):
    """A few KiB of budget: the Pike VM iterates the whole batch."""
    raw, texts = _small()
    knobs(lazy_iter_long=2, lazy_chunk=48, big_bytes=4096)
    re = R.Regex(HUGE)  # (the budget is read when the automaton is created)
    o = OracleRegex(re)
    exp = [o.find_iter(t) for t in texts]
    assert _iter(re, _dev(cuda, raw, 1), exp, stride=STRIDE, length=L, count=COUNT) == Path.ITER_WAVE
    info = R.Regex.last_lazy_iter_long()
    assert info["fell_back"] == 1 and info["units"] > info["haystacks"] == COUNT and info["chunk"] == 48
    assert _settled() == 0


def test_capacity(cuda, knobs):
    """counts and total stay exact, min(total, capacity) records are written
    and nothing at or past the capacity"""
    import torch
    raw, texts = _small()
    o = OracleRegex(R.Regex(HUGE))
    exp = [o.find_iter(t) for t in texts]
    flat = [m for e in exp for m in e]
    total = len(flat)
    assert total > 4
    dev = _dev(cuda, raw, 1)
    b = R._batch(dev, stride=STRIDE, length=L, count=COUNT)
    re = R.Regex(HUGE)
    knobs(lazy_iter_long=2, lazy_chunk=16)
    for cap in (0, 1, total - 1):
        counts = torch.full((COUNT,), -7, dtype=torch.int64, device=cuda)
        out = torch.full((total + 2, 2), -7, dtype=torch.int64, device=cuda)
        tot = torch.full((1,), -7, dtype=torch.int64, device=cuda)
        rc = N.rure_amd_find_iter_batch(re._re, ctypes.byref(b), ctypes.c_void_p(counts.data_ptr()),
                                        ctypes.c_void_p(out.data_ptr()), cap, ctypes.c_void_p(tot.data_ptr()),
                                        R._stream_ptr(None))
        torch.cuda.synchronize()
        assert rc == N.OK
        _chunked(COUNT, 16)
        assert int(tot.item()) == total and counts.cpu().numpy().tolist() == [len(e) for e in exp], cap
        rows = _pairs(out)
        assert rows[:cap] == flat[:cap], cap
        assert all(r == (-7, -7) for r in rows[cap:]), cap


def test_production_rule(cuda, knobs):
    """No knob, one haystack of 1 MiB: the rule takes the chunked iteration by
    itself, in units of the long scan's size.  The same text cut to 256 KiB,
    the shortest the rule takes: equal to the path it had (lazy_iter_long=0)."""
    import torch
    text = _mib(True)
    dev = _dev(cuda, text)
    re = R.Regex(HUGE)
    o = OracleRegex(re)
    assert not re.uses_dfa()
    exp = [o.find_iter(text)]
    assert len(exp[0]) > 100
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    assert _iter(re, dev, exp, stride=MIB, length=MIB, count=1) == Path.LAZY_DFA
    chunk = _unit_bytes(MIB, 1, cus)
    info = _chunked(1, chunk)
    assert info["units"] == -(-MIB // chunk) and info["units"] > 1
    q = MIB // 4
    knobs(lazy_iter_long=0)
    counts0, ms0 = re.find_iter_batch(dev, stride=q, length=q, count=1)
    assert N.last_path() == Path.ITER_WAVE and R.Regex.last_lazy_iter_long() == ZERO
    knobs()
    counts1, ms1 = re.find_iter_batch(dev, stride=q, length=q, count=1)
    _chunked(1, _unit_bytes(q, 1, cus))
    assert int(counts0[0]) > 20 and torch.equal(counts0, counts1) and torch.equal(ms0, ms1)
    assert _pairs(ms1) == o.find_iter(text[:q])


def test_kept_paths(cuda, knobs):
    """lazy_iter_long=0, lazy=0, an offset batch, a regex anchored at the
    start, a look-around regex, a regex with an eager DFA and a batch of many
    short haystacks keep the paths they had, and report no units."""
    import torch
    q = MIB // 4
    text = _mib(True)[:q]
    dev = _dev(cuda, text)
    re = R.Regex(HUGE)
    exp = [OracleRegex(re).find_iter(text)]
    where = dict(stride=q, length=q, count=1)
    for kn in (dict(lazy_iter_long=0), dict(lazy=0)):
        knobs(**kn)
        assert _iter(re, dev, exp, **where) == Path.ITER_WAVE, kn
        assert R.Regex.last_lazy_iter_long() == ZERO
    knobs()
    offs = torch.tensor([0, q], dtype=torch.int64, device=cuda)
    assert _iter(re, dev, exp, offsets=offs) == Path.ITER_WAVE
    assert R.Regex.last_lazy_iter_long() == ZERO
    # anchored at the start: no `.*?` prefix, no links
    ra = R.Regex("^" + HUGE)
    _iter(ra, dev, [OracleRegex(ra).find_iter(text)], **where)
    assert N.last_path() != Path.LAZY_DFA and R.Regex.last_lazy_iter_long() == ZERO
    # look-around: not under the knob either
    raw, texts = _small()
    small = _dev(cuda, raw, 1)
    swhere = dict(stride=STRIDE, length=L, count=COUNT)
    rl = R.Regex(r"(?-u)\bthe\b")
    el = [OracleRegex(rl).find_iter(t) for t in texts]
    knobs(lazy=1, lazy_rows=1)
    before = _iter(rl, small, el, **swhere)
    knobs(lazy=1, lazy_rows=1, lazy_iter_long=2, lazy_chunk=16)
    assert _iter(rl, small, el, **swhere) == before and R.Regex.last_lazy_iter_long() == ZERO
    # an eager DFA and no knob
    knobs()
    rd = R.Regex(r"\d{4}-\d{2}-\d{2}|[a-z]+ing")
    assert rd.uses_dfa()
    path = _iter(rd, dev, [OracleRegex(rd).find_iter(text)], **where)
    assert path not in (Path.LAZY_DFA, Path.ITER_WAVE) and R.Regex.last_lazy_iter_long() == ZERO
    # 400 haystacks of 200 bytes
    n, ln = 400, 200
    o = OracleRegex(re)
    assert _iter(re, dev, [o.find_iter(text[h * ln:(h + 1) * ln]) for h in range(n)],
                 stride=ln, length=ln, count=n) == Path.ITER_WAVE
    assert R.Regex.last_lazy_iter_long() == ZERO
    # and the chunked path after them, on the same regex object
    assert _iter(re, dev, exp, **where) == Path.LAZY_DFA
    _chunked(1)


def test_table_reuse(cuda, knobs):
    """A second call over the same text finds every row and link built: one
    round per pass, no row made (so nothing uploaded)."""
    raw, texts = _small()
    dev = _dev(cuda, raw, 1)
    re = R.Regex(HUGE)
    o = OracleRegex(re)
    exp = [o.find_iter(t) for t in texts]
    knobs(lazy_iter_long=2, lazy_chunk=16)
    where = dict(stride=STRIDE, length=L, count=COUNT)
    assert _iter(re, dev, exp, **where) == Path.LAZY_DFA
    first = _chunked(COUNT, 16)
    built = re.lazy_tables()[0]
    assert _iter(re, dev, exp, **where) == Path.LAZY_DFA
    second = _chunked(COUNT, 16)
    after = re.lazy_tables()[0]
    assert second["rounds"] == 2 + second["resume_passes"] <= first["rounds"]
    assert (after["states"], after["rows_built"]) == (built["states"], built["rows_built"])
    assert (second["repaired"], second["resume_passes"]) == (first["repaired"], first["resume_passes"])


def test_consumers(cuda, knobs):
    """split, replace (a literal and a $group template) and captures_iter of
    the grouped huge regex take their match list from the chunked iteration:
    one 5000-byte haystack in 16-byte units"""
    raw, texts = _small()
    t = texts[0]
    dev = _dev(cuda, raw, 1)
    where = dict(stride=STRIDE, length=L, count=1)
    re = R.Regex(GROUPED)
    assert not re.uses_dfa() and re.captures_len() == 3
    o = OracleRegex(re)
    names = re.capture_names()
    knobs(lazy_iter_long=2, lazy_chunk=16)

    def groups(row):
        g = [None if a < 0 or b < 0 else (a, b) for a, b in row]
        return None if g[0] is None else g

    def output(out, ooff):
        ob, oo = bytes(out.cpu().numpy()), ooff.cpu().numpy().tolist()
        return ob[oo[0]:oo[1]]

    assert _settled() == 0
    counts, pieces = re.split_batch(dev, **where)
    _chunked(1, 16)
    assert [t[a:b] for a, b in _pairs(pieces)] == RR.split(o, t) and len(RR.split(o, t)) > 3
    assert _settled() == 0
    out, ooff = re.replace_batch(dev, b"<->", **where)
    _chunked(1, 16)
    assert output(out, ooff) == RR.replacen(o, names, t, 0, b"<->", True)
    assert _settled() == 0
    out, ooff = re.replace_batch(dev, b"<$2>", expand=True, **where)
    assert R.Regex.last_lazy_iter_long()["fell_back"] == 0 and R.Regex.last_lazy_iter_long()["units"] > 1
    assert output(out, ooff) == RR.replacen(o, names, t, 0, b"<$2>", False)
    assert _settled() == 0
    counts, rows, _ = re.captures_iter_batch(dev, **where)
    assert R.Regex.last_lazy_iter_long()["fell_back"] == 0 and R.Regex.last_lazy_iter_long()["units"] > 1
    assert [groups(r) for r in rows.cpu().numpy().tolist()] == RR.captures_iter(o, t)
    assert _settled() == 0
