"""CPU check of the chunked scan of long haystacks on a regex's on-demand
forward DFA (host LazyDfa::strip_of; kernel: lazy_long_kernel, big_dfa.hip):
the kernel's walk over the exported tables and strip links
(lazy_long_sim.py), unit by unit, parking on every row and link not made yet,
equals the oracle's find / is_match / shortest_match -- for the regex past
the eager state budget and for ordinary ones, with units of 1 to 64 bytes so
that matches cross cuts, reverse NoMatches included.  Links are made on
demand and leave the automaton there was as it is."""
import functools

import numpy as np
import pytest

import regex_amd as R
from oracle_py import OracleRegex
from lazy_iter_sim import HUGE, LOOKS
from lazy_long_sim import UNKNOWN, LongTables, crossing, lazy_long
from test_gpu_iter_looks import _text
from test_lazy_iter_host import _mixed

PLAIN = [r"\d{4}-\d{2}-\d{2}", r"[a-z]+ing", r"Sherlock|Holmes", r"(?i)holmes\w*", r"(?-u)\bthe\b", r"x*",
         r"(?s).{3}$|^Th"]
CHUNKS = (1, 7, 16, 64)
MODES = ("find", "is_match", "shortest")


@functools.lru_cache(maxsize=None)
def _hays():
    """200 to 2000 bytes of sherlock pieces and a/b runs of 1 to 39 bytes"""
    raw = _mixed(1, 4000, 5)
    return [raw[:200], raw[200:717], raw[717:2000], raw[2000:4000]]


def _expected(o, t, start, mode):
    if start > len(t):
        return False if mode == "is_match" else None
    return {"find": o.find, "is_match": o.is_match, "shortest": o.shortest_match}[mode](t, start)


def _check(pat, hays, chunks=CHUNKS, starts=(0, 3)):
    re = R.Regex(pat)
    o = OracleRegex(re)
    tb = LongTables(re)
    hits = cross = 0
    for chunk in chunks:
        for start in starts:
            for mode in MODES:
                got, rounds = lazy_long(tb, hays, start, chunk, mode)
                exp = [_expected(o, t, start, mode) for t in hays]
                assert got == exp, (pat, chunk, start, mode)
                if mode == "find":
                    hits += sum(e is not None for e in exp)
                    cross += sum(crossing(e, start, chunk) for e in exp)
    assert tb.builds > 0  # lanes did park and resume
    return tb, hits, cross


def test_huge_equals_oracle():
    """past the eager budgets; with 16-byte units every match crosses a cut"""
    re = R.Regex(HUGE)
    assert not re.uses_dfa()
    tb, hits, cross = _check(HUGE, _hays())
    assert hits > 0 and cross > 0
    o = OracleRegex(re)
    assert all(crossing(o.find(t), 0, 16) for t in _hays() if o.find(t))
    known = tb.strip != UNKNOWN
    assert 2 < int(known.sum()) < tb.info["states"]  # only the links the cuts asked for
    assert 0 < tb.info["rows_built"] < tb.info["states"]


@pytest.mark.parametrize("pat", PLAIN)
def test_plain_equals_oracle(pat):
    extra = [b"on 2024-01-15 and 1999-12-31x", b"The thing\nthe", b"sing a ringing thing"]
    _, hits, _ = _check(pat, _hays() + extra)
    assert hits > 0


@pytest.mark.parametrize("pat", LOOKS)
def test_looks_equal_oracle(pat):
    _check(pat, [_text(seed, 256, False) for seed in range(4)] + [b"ab ab", b"xxxaxab"])


@pytest.mark.parametrize("pat", [HUGE, r"x*", r"(?s).{3}$|^Th", r"(?-u)\B"])
def test_degenerate_shapes(pat):
    """the empty haystack, start == len, start > len, a haystack shorter than
    one unit"""
    re = R.Regex(pat)
    o = OracleRegex(re)
    tb = LongTables(re)
    for t in (b"", b"abc", b"Tha", b"ab" * 12):
        for start in (0, len(t), len(t) + 1, len(t) + 70):
            for chunk in (1, 16, 64):
                for mode in MODES:
                    got, _ = lazy_long(tb, [t], start, chunk, mode)
                    assert got == [_expected(o, t, start, mode)], (pat, t, start, chunk, mode)


def test_reverse_nomatch():
    r"""(?-u)\B[ab]+ searched from inside a word: the unit that holds the
    forward end claims the search, and the reverse scan over text[start..end]
    finds no start: no match, though a later unit holds one."""
    re = R.Regex(r"(?-u)\B[ab]+")
    o = OracleRegex(re)
    t = b"xxxaxab"
    assert o.find(t, 3) is None and o.find(t, 0) == (3, 4) and o.is_match(t, 3)
    tb = LongTables(re)
    for chunk in (1, 2, 16):
        assert lazy_long(tb, [t], 3, chunk, "find")[0] == [None]
        assert lazy_long(tb, [t], 0, chunk, "find")[0] == [(3, 4)]
        assert lazy_long(tb, [t], 3, chunk, "is_match")[0] == [True]


def test_twins_and_the_automaton_there_was():
    """The twin of a twin is itself, a new twin comes after every state there
    was with its row not built, and the states that existed keep their ids,
    rows, eof and built flags."""
    re = R.Regex(HUGE)
    tb = LongTables(re)
    for t in _hays():
        lazy_long(tb, [t], 0, 1 << 20, "find")  # one unit: rows, no link
    assert (tb.strip[2:] == UNKNOWN).all() and tb.strip[0] == 0
    before = (dict(tb.info), tb.trans.copy(), tb.eof.copy(), tb.built.copy(), tb.start.copy())
    n = before[0]["states"]
    asked = [s for s in range(2, n) if tb.built[s]][:50]
    assert asked and re.lazy_strip_build(asked)
    tb.load()
    assert tb.info["states"] > n and tb.info["rows_built"] == before[0]["rows_built"]
    assert np.array_equal(tb.trans[:n], before[1]) and np.array_equal(tb.eof[:n], before[2])
    assert np.array_equal(tb.built[:n], before[3]) and np.array_equal(tb.start, before[4])
    assert not tb.built[n:].any() and (tb.trans[n:] == UNKNOWN).all()
    twins = {int(tb.strip[s]) for s in asked}
    assert all(x == 0 or x < tb.info["states"] for x in twins) and any(x >= n for x in twins)
    for x in twins:
        assert tb.strip[x] == x
    others = [s for s in range(2, tb.info["states"]) if s not in asked and s not in twins]
    assert others and (tb.strip[others] == UNKNOWN).all()
    again = tb.strip.copy()
    assert re.lazy_strip_build(asked + sorted(twins)) and np.array_equal(re.lazy_strip(), again)
    # the walks still answer as before on the grown automaton
    o = OracleRegex(re)
    for t in _hays():
        assert lazy_long(tb, [t], 0, 16, "find")[0] == [o.find(t)]


def test_budget_spent(knobs):
    """A budget below what the start state alone takes (its key and the
    first rows: about 190 bytes): lazy_strip_build reports it spent, and the
    simulation gives the batch up."""
    knobs(big_bytes=150)
    re = R.Regex(HUGE)
    tb = LongTables(re)  # (the budget is read when the automaton is created)
    knobs()
    assert re.lazy_strip_build([2]) is False
    assert (re.lazy_strip()[2:] == UNKNOWN).all()
    assert lazy_long(tb, _hays(), 0, 16, "find")[0] is None


@pytest.mark.parametrize("pat", [r"^(?:a|b)*a(?:a|b){20}", r"^Th"])
def test_anchored_start_has_no_links(pat):
    re = R.Regex(pat)
    re.lazy_tables()  # (the automaton itself exists)
    with pytest.raises(RuntimeError):
        re.lazy_strip()
    with pytest.raises(RuntimeError):
        re.lazy_strip_build([2])


def test_no_automaton():
    re = R.Regex(r"\bthe\b")
    with pytest.raises(RuntimeError):
        re.lazy_strip()
