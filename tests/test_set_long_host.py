"""CPU check of the chunked RegexSet scan (regex_amd/csrc/kernels/set_long.hip)
over the exported strip-built set automaton: the kernel's unit algorithm
(set_long_sim.py: start state at the unit's first byte, strip at the cut,
now_mask / eof_mask / reach) ORed over the units equals the oracle's
many_matches_at, at unit sizes 1, 7, 16 and 64, and the reach array is what
the kernel's early exit needs."""
import functools
import random
import zlib

import numpy as np
import pytest

import regex_amd as R
from oracle_py import OracleRegex
from regex_amd import _native as N
from regex_amd.workloads import log_lines_host
from set_long_data import CASES
from set_long_sim import set_long_matches, tables

CHUNKED = sorted(k for k, (_, chunked) in CASES.items() if chunked)
LANES = sorted(k for k, (_, chunked) in CASES.items() if not chunked)


@functools.lru_cache(maxsize=None)
def _log():
    return log_lines_host(6, seed=0x5E7, lo=100, hi=100)[0]


def _texts(name):
    rng = random.Random(zlib.crc32(name.encode()))
    log = _log()
    out = [b"", b"a", b"abc", b"xabc", b"12\n34 foo\nabc", b"xx foo z\nabc",
           b"a" * 250 + b" foo",                               # many a and no z
           b"qq a" + b"q" * 150 + b"z" + b"q" * 40,            # one match over several units
           b"." * 60 + b"status=404" + b"." * 100 + b"kernel",
           b"INFO x" + b" " * 120 + b"ERROR WARNING oom",      # INFO.*ERROR over several units
           bytes(log[:300]), bytes(log[300:597])]
    for _ in range(6):
        out.append(bytes(rng.choice(b"abcxz fo\n0123=.") for _ in range(rng.randint(0, 300))))
    return out


@pytest.fixture(scope="module")
def built():
    """name -> (tables, oracle), built once."""
    cache = {}

    def get(name):
        if name not in cache:
            rs = R.RegexSet(CASES[name][0])
            cache[name] = (tables(rs), OracleRegex(rs))
        return cache[name]
    return get


@pytest.mark.parametrize("name", CHUNKED)
def test_units_equal_oracle(built, name):
    tb, o = built(name)
    assert tb is not None
    n = tb[0]["n"]
    for t in _texts(name):
        for start in (0, 3, len(t), len(t) + 1):
            exp = sum(1 << j for j in o.matches(t, start)) if start <= len(t) else 0
            for chunk in (1, 7, 16, 64):
                for kw in ({}, {"reverse": True}, {"share": False}):
                    got = set_long_matches(tb, t, start, chunk, **kw)
                    assert got == exp, (name, t, start, chunk, kw, [j for j in range(n) if (got ^ exp) >> j & 1])


def test_units_stop_after_the_cut(built):
    """What the stripped states are for: past its cut a unit only finishes
    the matches it began, so the units together step little more than the
    text (a literal set: at most the longest literal past each cut), and a
    lingering `.*` thread of a pattern already reported stops at the next
    look at the mask word instead of running to the end of the text."""
    import set_long_sim as S
    tb, _ = built("literals")
    t = (b"status=40 ERROR kernel oo " * 12)[:300]
    S.STEPS[0] = 0
    set_long_matches(tb, t, 0, 16)
    assert S.STEPS[0] <= len(t) + len(S.units_of(len(t), 0, 16)) * len("status=404")
    tb, _ = built("mixed")
    t = b"a" * 299 + b"z"  # `(?s)a.*z`: every unit's thread lingers to the end
    S.STEPS[0] = 0
    set_long_matches(tb, t, 0, 16, reverse=True)  # the last unit reports it first
    assert S.STEPS[0] <= len(t) + len(S.units_of(len(t), 0, 16)) * 8  # (the simulation polls every 8 bytes)
    S.STEPS[0] = 0
    set_long_matches(tb, t, 0, 16, share=False)
    assert S.STEPS[0] > 4 * len(t)


@pytest.mark.parametrize("name", CHUNKED)
def test_reach(built, name):
    """reach[s] holds what s reports itself, is closed under transitions, and
    the dead state reaches nothing; strip stays inside the automaton."""
    info, tr, eof, now, st, strip, reach = built(name)[0]
    assert np.all(reach & now == now) and np.all(reach & eof == eof)
    assert reach[info["dead"]] == 0 and info["quit"] == -1
    succ = reach[tr]  # (states, 256)
    assert np.all(succ & ~reach[:, None] == 0)
    # the least such set: nothing in reach[s] that neither s nor a successor has
    assert np.array_equal(reach, now | eof | np.bitwise_or.reduce(succ, axis=1))
    assert strip.max() < info["states"] and strip[info["dead"]] == info["dead"]
    assert any(int(strip[s]) != s for s in set(int(x) for x in st))


@pytest.mark.parametrize("pats", [[r"\bfoo", "bar"], ["^a", "^b"]] + [CASES[k][0] for k in LANES],
                         ids=["unicode_wb", "anchored_start"] + LANES)
def test_no_automaton(pats):
    """A set whose DFA can quit (a Unicode `\\b` member: C4_PATTERNS too), that
    is anchored at the start in every pattern, or that has no DFA: no
    strip-built automaton, the set keeps one lane per haystack."""
    rs = R.RegexSet(pats)
    assert N.rure_amd_set_long_dfa_export(rs._set, None, None, None, None, None, None, None) == N.ERR_DFA
    assert rs.long_dfa_tables() is None


def test_export_argument_errors():
    assert N.rure_amd_set_long_dfa_export(None, None, None, None, None, None, None, None) == N.ERR_ARG
    one = R.RegexSet(["abc"])
    assert N.rure_amd_set_long_dfa_export(one._set, None, None, None, None, None, None, None) == N.ERR_ARG
    units, haystacks, chunk = R.RegexSet.last_long_units()  # (host only: no GPU needed)
    assert (units == 0) == (haystacks == 0) == (chunk == 0)
