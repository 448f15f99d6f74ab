"""Few long haystacks on the on-demand forward DFA (big_dfa.hip
lazy_long_kernel, dispatch.cpp run_lazy_long): a regex past the eager state
budgets, `(?:a|b)*a(?:a|b){20}`, used to search one long haystack on the Pike
VM, a wave per haystack.  Now the search is cut into units; unit [c0, c1)
steps into its state's twin without the `.*?` prefix at c1 - 1 (a link made
on demand, as rows are) and walks on until the automaton dies.  Forced onto
5000-byte haystacks with 16-, 48- and 4096-byte units (knobs lazy_long=2,
lazy_chunk; ordinary regexes under lazy=1, lazy_rows=1 park on nearly every
row and link), by the production rule on 1 MiB, through the host calls, and
the batches that keep their paths.  Every answer is the oracle's;
last_path() == Path.LAZY_DFA, units > haystacks and fell_back == 0 assert
that the chunked kernel gave it and not the Pike VM fallback.

Rounds: a batch that needs 256 rounds or more goes to the Pike VM, so the
texts plant a/b runs (of at most 39 bytes) from a pool of six, whose states
the units share; _rounds() checks on the CPU simulation (no rows built ahead:
an upper bound of what the device needs, which builds more per round) that
every input here stays below that."""
import functools

import numpy as np
import pytest

import regex_amd as R
from regex_amd import Path
from regex_amd import _native as N
from golden_data import corpus
from oracle_py import OracleRegex
from lazy_long_sim import LongTables, crossing, lazy_long

pytestmark = pytest.mark.gpu

HUGE = r"(?:a|b)*a(?:a|b){20}"
GROUPED = r"((?:a|b)*)a((?:a|b){20})"
PLAIN = [r"\d{4}-\d{2}-\d{2}", r"[a-z]+ing", r"Sherlock|Holmes", r"(?i)holmes\w*", r"(?-u)\bthe\b", r"x*",
         r"(?s).{3}$|^Th"]
L, STRIDE, COUNT = 5000, 5003, 3
MIB = 1 << 20
MODES = ("find", "is_match", "shortest")


def _planted(n, seed, gap, extras=()):
    """n bytes of sherlock pieces of up to `gap` bytes with, between them,
    a/b runs from a pool of six (3 to 39 bytes) and, after one piece in four,
    one of `extras`"""
    rng = np.random.default_rng(seed)
    base = corpus("sherlock")
    pool = [bytes(rng.choice(np.frombuffer(b"ab", dtype=np.uint8), size=k)) for k in (3, 11, 22, 27, 33, 39)]
    out = bytearray()
    while len(out) < n:
        a = int(rng.integers(0, len(base) - gap))
        out += base[a:a + int(rng.integers(gap // 2, gap + 1))]
        if extras and rng.integers(0, 4) == 0:
            out += extras[int(rng.integers(0, len(extras)))]
        out += pool[int(rng.integers(0, len(pool)))]
    return bytes(out[:n])


@functools.lru_cache(maxsize=None)
def _small():
    """3 haystacks of 5000 bytes at stride 5003, a run about every 70 bytes;
    dates and names among them, so that every regex here has matches"""
    raw = _planted(COUNT * STRIDE, 7, 90, (b" on 2024-01-15, ", b" Mr. Sherlock Holmes's ", b" xx "))
    return raw, [raw[h * STRIDE:h * STRIDE + L] for h in range(COUNT)]


@functools.lru_cache(maxsize=None)
def _mib(planted):
    """1 MiB of sherlock text, with a run about every 3 KiB or none at all"""
    if planted:
        return _planted(MIB, 11, 4096)
    base = corpus("sherlock")
    return (base * (MIB // len(base) + 1))[:MIB]


def _dev(cuda, raw, lead=0):
    """raw on the device, `lead` bytes past a 16-byte aligned address"""
    import torch
    d = torch.from_numpy(np.frombuffer(b"a" * lead + raw + b"\0" * 16, dtype=np.uint8).copy()).to(cuda)[lead:]
    assert d.data_ptr() % 16 == lead
    return d


def _expected(o, t, start, mode):
    return {"find": o.find, "is_match": o.is_match, "shortest": o.shortest_match}[mode](t, start)


def _call(re, dev, mode, **where):
    """One batched call as the oracle's answers, and the path that gave them."""
    if mode == "find":
        got = [None if a < 0 else (a, b) for a, b in re.find_batch(dev, **where).cpu().numpy().tolist()]
    elif mode == "is_match":
        got = [bool(x) for x in re.is_match_batch(dev, **where).cpu().numpy().tolist()]
    else:
        got = [None if x < 0 else x for x in re.shortest_match_batch(dev, **where).cpu().numpy().tolist()]
    return got, N.last_path()


def _chunked(haystacks, chunk=None):
    """The last call ran the chunked kernel to the end."""
    units, hays, c, rounds, fell_back = R.Regex.last_lazy_long()
    assert N.last_path() == Path.LAZY_DFA
    assert hays == haystacks and units > hays and fell_back == 0 and 0 < rounds < 256
    assert chunk is None or c == chunk
    return units, c


@functools.lru_cache(maxsize=None)
def _rounds(pat, which, chunk, start):
    """The rounds the CPU simulation needs with no row built ahead."""
    texts = _small()[1] if which == "small" else [_mib(True)]
    got, rounds = lazy_long(LongTables(R.Regex(pat)), texts, start, chunk, "find", 0, 256)
    assert got is not None, (pat, which, chunk, rounds)
    return rounds


@pytest.mark.parametrize("pat", [HUGE] + PLAIN)
def test_forced_units(cuda, knobs, pat):
    """3 haystacks of 5000 bytes, stride 5003, one byte past an aligned base,
    in units of 16, 48 and 4096 bytes from starts 0 and 3"""
    raw, texts = _small()
    dev = _dev(cuda, raw, 1)
    re = R.Regex(pat)
    o = OracleRegex(re)
    dfa_type = re.match_info()["match_type"] == "Dfa"  # (literal / suffix match types run their own engines)
    forced = dict(big=2) if pat == HUGE else dict(lazy=1, lazy_rows=1)
    hits = 0
    for chunk in (16, 48, 4096):
        for start in (0, 3):
            assert _rounds(pat, "small", chunk, start) < 256
            exp = [o.find(t, start) for t in texts]
            if chunk == 16 and pat == HUGE:
                assert any(crossing(e, start, chunk) for e in exp)
            for mode in MODES:
                knobs(lazy_long=2, lazy_chunk=chunk, **forced)
                got, path = _call(re, dev, mode, stride=STRIDE, length=L, count=COUNT, start=start)
                assert got == [_expected(o, t, start, mode) for t in texts], (pat, chunk, start, mode)
                if dfa_type:
                    units, _ = _chunked(COUNT, chunk)
                    assert units == COUNT * -(-(L - start) // chunk)
            hits += sum(e is not None for e in exp)
    assert 0 < hits


def _unit_bytes(span, count, cus):
    """host/chunk_plan.hpp unit_bytes for the long scan: 1024 lanes per CU
    shared out over the haystacks, at least 16 KiB, an odd number of 128-byte
    lines"""
    per_h = -(-cus * 1024 // count)
    lines = -(-max(-(-span // per_h), 16 << 10) // 128)
    return (lines | 1) * 128


def test_production_rule(cuda):
    """No knob, one haystack of 1 MiB: the rule takes the chunked scan by
    itself, in units of the long scan's size; the batched calls and the host
    calls on the same bytes give the oracle's answers."""
    import torch
    text = _mib(True)
    dev = _dev(cuda, text)
    re = R.Regex(HUGE)
    o = OracleRegex(re)
    assert not re.uses_dfa() and o.find(text) is not None
    chunk = _unit_bytes(MIB, 1, torch.cuda.get_device_properties(cuda).multi_processor_count)
    assert _rounds(HUGE, "mib", chunk, 0) < 256
    for mode in MODES:
        got, _ = _call(re, dev, mode, stride=MIB, length=MIB, count=1)
        assert got == [_expected(o, text, 0, mode)], mode
        units, _ = _chunked(1, chunk)
        assert units == -(-MIB // chunk) and units > 1
    for mode, fn in (("find", re.find), ("is_match", re.is_match), ("shortest", re.shortest_match)):
        assert fn(text) == _expected(o, text, 0, mode), mode
        _chunked(1, chunk)
    assert re.find(text, 3) == o.find(text, 3)
    _chunked(1)


def test_no_match_anywhere(cuda):
    """A megabyte without a match answers "none" on all three calls."""
    text = _mib(False)
    dev = _dev(cuda, text)
    re = R.Regex(HUGE)
    assert OracleRegex(re).find(text) is None
    for mode in MODES:
        got, _ = _call(re, dev, mode, stride=MIB, length=MIB, count=1)
        assert got == [False if mode == "is_match" else None], mode
        _chunked(1)


def test_budget_falls_back(cuda, knobs):
    """A few KiB of budget: the Pike VM answers the whole batch."""
    raw, texts = _small()
    dev = _dev(cuda, raw, 1)
    knobs(lazy_long=2, lazy_chunk=48, big_bytes=4096)
    re = R.Regex(HUGE)  # (the budget is read when the automaton is created)
    o = OracleRegex(re)
    for mode in MODES:
        got, path = _call(re, dev, mode, stride=STRIDE, length=L, count=COUNT)
        assert got == [_expected(o, t, 0, mode) for t in texts], mode
        units, hays, chunk, rounds, fell_back = R.Regex.last_lazy_long()
        assert path == Path.PIKE_ONLY and fell_back == 1 and units > hays == COUNT and chunk == 48


def test_kept_paths(cuda, knobs):
    """lazy_long=0, a batch that fills the device, an offset batch and a
    regex anchored at the start keep the paths they had, and report no
    units."""
    import torch
    text = _mib(True)
    dev = _dev(cuda, text)
    re = R.Regex(HUGE)
    o = OracleRegex(re)
    exp = o.find(text)
    assert exp is not None and exp[1] < 8192  # (the Pike VM stops soon after the leftmost match)
    none = (0, 0, 0, 0, 0)
    knobs(lazy_long=0)
    assert _call(re, dev, "find", stride=MIB, length=MIB, count=1) == ([exp], Path.PIKE_ONLY)
    assert R.Regex.last_lazy_long() == none
    assert re.find(text) == exp and R.Regex.last_lazy_long() == none
    knobs()
    # an offset batch with the long haystack
    offs = torch.tensor([0, MIB], dtype=torch.int64, device=cuda)
    assert _call(re, dev, "find", offsets=offs) == ([exp], Path.PIKE_ONLY)
    assert R.Regex.last_lazy_long() == none
    # 64 haystacks per CU: one lane per haystack on the on-demand DFA
    n = torch.cuda.get_device_properties(cuda).multi_processor_count * 64
    ln = MIB // n
    got, path = _call(re, dev, "find", stride=ln, length=ln, count=n)
    assert path == Path.LAZY_DFA and R.Regex.last_lazy_long() == none
    assert got == [o.find(text[h * ln:(h + 1) * ln]) for h in range(n)]
    assert sum(g is not None for g in got) > 0
    # anchored at the start: no `.*?` prefix, no links
    ra = R.Regex("^" + HUGE)
    assert _call(ra, dev, "find", stride=MIB, length=MIB, count=1)[0] == [OracleRegex(ra).find(text)]
    assert R.Regex.last_lazy_long() == none
    # and the chunked path after them, on the same regex object
    assert _call(re, dev, "find", stride=MIB, length=MIB, count=1)[0] == [exp]
    _chunked(1)


def test_captures(cuda, knobs):
    """captures_batch takes its bounds from the chunked scan: one 5000-byte
    haystack in 16-byte units"""
    raw, texts = _small()
    dev = _dev(cuda, raw, 1)
    re = R.Regex(GROUPED)
    assert not re.uses_dfa() and re.captures_len() == 3
    o = OracleRegex(re)
    knobs(big=2, lazy_long=2, lazy_chunk=16)
    got = re.captures_batch(dev, stride=STRIDE, length=L, count=1).cpu().numpy().tolist()
    units, hays, chunk, rounds, fell_back = R.Regex.last_lazy_long()
    assert (units, hays, chunk, fell_back) == (-(-L // 16), 1, 16, 0)
    exp = o.captures(texts[0])
    assert exp is not None and [None if a < 0 or b < 0 else (a, b) for a, b in got[0]] == exp
