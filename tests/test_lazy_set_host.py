"""CPU check of RegexSet matches on the set's on-demand DFA (host LazyDfa over
a set program; kernel: lazy_set_kernel, big_dfa.hip): the kernel's walk over
the exported tables (lazy_set_sim.py), parking on every row not built yet and
resuming with the mask carried, equals the oracle's many_matches_at; the
automaton is built on demand for a set past the eager state budget, gives up
within its memory budget, and is refused to the sets that keep the Pike VM."""
import functools
import random

import pytest

import regex_amd as R
from oracle_py import OracleRegex
from regex_amd.workloads import log_lines_host
from set_long_data import CASES, MIXED
from lazy_set_sim import FLAGS, NO_DFA, Tables, lazy_set_matches

SETS = {"no_dfa": NO_DFA, "flags": FLAGS}
for _k, (_p, _) in CASES.items():
    SETS[_k] = _p
assert SETS["mixed"] is MIXED


def _can_quit(rs):
    return bool(rs.program(0)[0].has_unicode_word_boundary)


@functools.lru_cache(maxsize=None)
def _built(name):
    rs = R.RegexSet(SETS[name])
    return rs, OracleRegex(rs)


@functools.lru_cache(maxsize=None)
def _texts():
    """About 50 texts of 0 to 200 bytes: log lines, a/b runs, empty, one byte."""
    rng = random.Random(0x1A27)
    buf, offs = log_lines_host(20, seed=0x5E7, lo=1, hi=200)
    out = [bytes(buf[offs[i]:offs[i + 1]]) for i in range(20)]
    out += [bytes(rng.choice(b"ab") for _ in range(rng.randint(2, 200))) for _ in range(14)]
    out += [bytes(rng.choice(b"ab\n 1fo") for _ in range(rng.randint(2, 60))) for _ in range(6)]
    out += [b"", b"a", b"b", b"\n", b"7", b"foo", b"a foo\n12\nabc", b"aaaa", b"12", b"xabc z"]
    return out


CANNOT_QUIT = sorted(k for k in SETS if not _can_quit(_built(k)[0]))


def test_the_sets_under_test():
    assert {"no_dfa", "flags", "mixed", "literals", "c4_ascii_wb"} <= set(CANNOT_QUIT)
    assert "c4" not in CANNOT_QUIT
    assert 45 <= len(_texts()) <= 55 and max(len(t) for t in _texts()) <= 200


@pytest.mark.parametrize("name", CANNOT_QUIT)
def test_walk_equals_oracle(name):
    rs, o = _built(name)
    tb = Tables(rs)
    ahead = 0 if name in ("no_dfa", "flags", "mixed") else 16  # (0: every new state parks the lane)
    for t in _texts():
        for start in (0, 3, len(t), len(t) + 1):
            exp = sum(1 << j for j in o.matches(t, start)) if start <= len(t) else 0
            got = lazy_set_matches(tb, t, start, ahead)
            assert got == exp, (name, t, start, [j for j in range(len(rs)) if (got ^ exp) >> j & 1])
    assert tb.builds > 0  # lanes did park and resume
    info = tb.info
    assert info["rows_built"] == int(tb.built.sum()) - 2  # (dead and the unused quit state count as built)
    assert info["hot_rows"] == min(info["states"], (64 << 10) // 4 // info["columns"])


def test_past_the_eager_budget_on_demand():
    """The set without a DFA: its texts visit a small part of the automaton,
    and only that part is built."""
    rs, _ = _built("no_dfa")
    assert not rs.uses_dfa()
    tb = Tables(rs)
    for t in _texts():
        lazy_set_matches(tb, t, 0, 0)
    assert 0 < tb.info["rows_built"] < tb.info["states"]
    assert not rs.uses_dfa()  # (the eager automaton's answer is not the on-demand one's)


def test_budget_spent(knobs):
    """A few KiB of budget: lazy_build reports it spent, and the simulation
    gives the batch up."""
    knobs(big_bytes=4096)
    rs = R.RegexSet(NO_DFA)
    tb = Tables(rs)  # (the budget is read when the automaton is created)
    knobs()
    rng = random.Random(5)
    got = [lazy_set_matches(tb, bytes(rng.choice(b"ab") for _ in range(200)), 0, 0) for _ in range(20)]
    assert None in got
    todo = [s for s in range(tb.info["states"]) if not tb.built[s]]
    assert todo and rs.lazy_build(todo[:1]) is False
    assert rs.lazy_build([], ahead=1) is False


@pytest.mark.parametrize("pats", [[r"\bfoo", "bar"], CASES["c4"][0], ["p%d" % i for i in range(65)]],
                         ids=["unicode_wb", "c4", "65_patterns"])
def test_no_automaton(pats):
    rs = R.RegexSet(pats)
    with pytest.raises(RuntimeError):
        rs.lazy_tables()
    with pytest.raises(RuntimeError):
        rs.lazy_build([2])
