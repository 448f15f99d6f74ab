"""CPU check of find_iter over few long haystacks on a regex's on-demand
forward DFA (kernels: lazy_iter_long_kernel and the resolve kernels,
big_dfa.hip; host: run_lazy_iter_long): the passes of lazy_iter_long_sim.py
over the exported tables and strip links, parking on every row and link not
made yet, equal the oracle's find_iter -- for the regex past the eager state
budget, ordinary ones, regexes that match the empty string and a fixed-length
one, with units of 1, 16 and 48 bytes from starts 0 and 3.  After every
resolve step the unit records go through rure_amd_lazy_iter_resolve, the rule
the device runs compiled for the host: its final records and its to-do list
equal the simulation's, pass by pass.  The texts of tests/
test_gpu_lazy_iter_long.py run here too, which shows that they stay below the
256 rounds and 64 resume passes at which the device gives a batch up."""
import functools

import pytest

import regex_amd as R
from regex_amd import _native as N
from oracle_py import OracleRegex
from lazy_iter_sim import HUGE
from lazy_long_sim import LongTables
import lazy_iter_long_sim as S
from test_gpu_lazy_long import PLAIN as LONG_PLAIN
from test_gpu_lazy_long import _small

# test_gpu_lazy_long.py's regexes without look-around
PLAIN = [p for p in LONG_PLAIN if p not in (r"(?-u)\bthe\b", r"(?s).{3}$|^Th", r"x*")]
# (`a|x{0}`: "a or nothing"; the parser takes no empty alternate, `a|`)
EMPTY = [r"x*", r"a*", r"(?:ab)*", r"a|x{0}"]
FIXED = r"(?-u)[ab]{3}"
# never rejoins its speculation either, and has no eager DFA (the GPU fallback case)
HUGE_LAZY = r"(?:a|b)*?a(?:a|b){20}"


def run_text(n, seed=3):
    """n bytes of a and b, between two words"""
    import numpy as np
    rng = np.random.default_rng(seed)
    return b"The end " + bytes(rng.choice(np.frombuffer(b"ab", dtype=np.uint8), size=n)) + b" of it."


def _recs(rs):
    arr = (N.LilRec * max(len(rs), 1))()
    for i, r in enumerate(rs):
        arr[i] = N.LilRec(r["ep"], r["elm"], r["xp"], r["xlm"], r["count"], r["flags"] & (S.HAS | S.CLEAN | 0xF0))
    return arr


def _as_dict(r):
    return {"ep": r.entry_p, "elm": r.entry_lm, "xp": r.exit_p, "xlm": r.exit_lm, "count": r.count, "flags": r.flags}


class Mirror(object):
    """The shipped resolve rule beside the simulation's: check() after every
    resolve step of the simulation."""

    def __init__(self):
        self.steps = self.asked = 0
        self.last = None

    def __call__(self, sim, first, todo):
        import ctypes
        n, nh = len(sim.units), len(sim.texts)
        if first:
            self.spec, self.fix = _recs(sim.spec), _recs(sim.fix)
            self.fin = (N.LilRec * n)()
            self.changed = (ctypes.c_uint8 * n)()
            self.walk = (N.LilWalk * nh)()
        else:
            for u, p, lm in self.last:  # the runs asked for
                r = sim.fin[u]
                assert S.source(r) == S.RUN and (r["ep"], r["elm"]) == (p, lm)
                self.fin[u] = N.LilRec(r["ep"], r["elm"], r["xp"], r["xlm"], r["count"], r["flags"])
        got = R.Regex.lazy_iter_resolve(nh, sim.nk, sim.start, sim.chunk, first, self.spec, self.fix, self.fin,
                                        self.changed, self.walk)
        assert got == todo
        if first:
            assert [bool(c) for c in self.changed] == sim.changed
        asked = {u for u, _, _ in todo}
        for u in range(n):
            if u not in asked:  # (a unit asked for gets its record from the run)
                assert _as_dict(self.fin[u]) == sim.fin[u], (u, first)
        self.last = todo
        self.steps += 1
        self.asked += len(todo)


def _check(pat, texts, chunks=(16, 48), starts=(0, 3), capped=True):
    """capped=False: the algorithm without the cap on the resume passes (the
    device gives such a batch up; the answers it would reach are right)"""
    re = R.Regex(pat)
    o = OracleRegex(re)
    tb = LongTables(re)
    stats = []
    for chunk in chunks:
        for start in starts:
            mirror = Mirror()
            got, info = S.lazy_iter_long(tb, texts, start, chunk, check=mirror,
                                         max_passes=S.MAX_PASSES if capped else None)
            exp = [o.find_iter(t, start) for t in texts]
            assert got == exp, (pat, chunk, start)
            assert info["total"] == sum(len(e) for e in exp)
            assert info["rounds"] < S.MAX_ROUNDS and (info["resume_passes"] <= S.MAX_PASSES) == capped
            assert mirror.steps == info["resume_passes"] + 1
            stats.append(info)
    assert tb.builds > 0  # lanes did park and resume
    return stats


@functools.lru_cache(maxsize=None)
def _short():
    """1500 bytes of the GPU tests' text, for one-byte units"""
    return [_small()[1][0][:1500]]


@pytest.mark.parametrize("pat", [HUGE] + PLAIN + EMPTY + [FIXED])
def test_equals_oracle(pat):
    """the GPU tests' haystacks in 16- and 48-byte units, 1500 bytes in
    one-byte units"""
    stats = _check(pat, _small()[1])
    if pat == HUGE:
        assert all(s["repaired"] > 0 for s in stats)  # 39-byte runs cross 16-byte cuts
    # (three-byte matches through the runs in one-byte units: a resume pass per match, past the cap)
    _check(pat, _short(), chunks=(1,), capped=pat != FIXED)
    _check(pat, _small()[1], chunks=(4096,), starts=(0,))


@pytest.mark.parametrize("pat", [HUGE, r"x*", r"a|x{0}", FIXED])
def test_degenerate_shapes(pat):
    """the empty haystack, start == len, start > len, a haystack shorter than
    one unit"""
    re = R.Regex(pat)
    o = OracleRegex(re)
    tb = LongTables(re)
    for t in (b"", b"abc", b"ab" * 12):
        for start in (0, len(t), len(t) + 1):
            for chunk in (1, 16):
                got, _ = S.lazy_iter_long(tb, [t], start, chunk, check=Mirror())
                assert got == [o.find_iter(t, start) if start <= len(t) else []], (pat, t, start, chunk)


def test_resume_passes():
    """A fixed-length match through a 200-byte run never rejoins the units'
    speculation: the walker asks for unit after unit."""
    stats = _check(FIXED, [run_text(200)], chunks=(16,))
    assert all(1 <= s["resume_passes"] < S.MAX_PASSES for s in stats)
    stats = _check(HUGE_LAZY, [run_text(200)], chunks=(16,))
    assert all(1 <= s["resume_passes"] < S.MAX_PASSES for s in stats)


@pytest.mark.parametrize("pat", [FIXED, HUGE_LAZY])
def test_gives_up_past_the_cap(pat):
    """... and through a 5000-byte run it needs more passes than the cap"""
    re = R.Regex(pat)
    mirror = Mirror()
    got, info = S.lazy_iter_long(LongTables(re), [run_text(5000)], 0, 16, check=mirror)
    assert got is None and info["resume_passes"] == S.MAX_PASSES + 1
    assert mirror.asked == S.MAX_PASSES + 1


def test_capacity():
    re = R.Regex(HUGE)
    texts = _small()[1]
    flat = [m for t in texts for m in OracleRegex(re).find_iter(t)]
    assert len(flat) > 4
    for cap in (0, 1, len(flat) - 1):
        got, info = S.lazy_iter_long(LongTables(re), texts, 0, 16, cap=cap)
        assert [m for g in got for m in g] == flat[:cap] and info["total"] == len(flat)


def test_budget_spent(knobs):
    knobs(big_bytes=150)
    re = R.Regex(HUGE)
    tb = LongTables(re)  # (the budget is read when the automaton is created)
    knobs()
    assert S.lazy_iter_long(tb, _small()[1], 0, 16)[0] is None


def test_resolve_rejects_null():
    assert N.rure_amd_lazy_iter_resolve(1, 1, 0, 16, 1, None, None, None, None, None, None) == N.ERR_ARG
