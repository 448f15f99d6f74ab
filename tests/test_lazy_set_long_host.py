"""CPU check of RegexSet matches over few long haystacks on the set's
on-demand DFA (host LazyDfa::strip_of and reach; kernel: lazy_set_long_kernel,
big_dfa.hip): the kernel's walk over the exported tables, links and reach
(lazy_set_long_sim.py), unit by unit, parking on every row and link not made
yet, ORed into one word per haystack, equals the oracle's many_matches_at --
for every set of test_lazy_set_host that cannot quit, with units of 16, 48
and 4096 bytes.  reach bounds what a walk reports, links leave the automaton
there was as it is, and the reach exit keeps a lingering `.*` thread from
dragging every unit to the end of the text."""
import functools
import random

import numpy as np
import pytest

import regex_amd as R
from oracle_py import OracleRegex
from lazy_set_long_sim import SetLongTables, Stats, check_reach, lazy_set_long
from lazy_set_sim import NO_DFA, UNKNOWN
from set_long_data import CASES
from test_lazy_set_host import CANNOT_QUIT, SETS, _texts

CHUNKS = (16, 48, 4096)
LINGER = [r"(?s)GET.*", NO_DFA[0], "bb"]


def ab_pool(rng, n=4, lo=19, hi=40):
    """a/b runs the texts plant again and again, so that units share states"""
    return [bytes(rng.choice(b"ab") for _ in range(rng.randint(lo, hi))) for _ in range(n)]


@functools.lru_cache(maxsize=None)
def long_texts():
    """Three texts of 5000 bytes: log-like lines (words of the sets under
    test among them) with a/b runs from a small pool planted between them;
    the last one ends inside a run."""
    rng = random.Random(0x5E71)
    pool = ab_pool(rng)
    words = [b"ERROR", b"INFO", b"status=404", b"foo", b"abc", b"oom", b"kernel", b"12", b"x", b"GET /a.js", b"z",
             b"the", b"null", b"warning", b"2024-01-15"]
    out = []
    for k in range(3):
        t = b"a " if k == 1 else b""  # (`^a` of the set without a DFA: another mask)
        while len(t) < 5000:
            t += b" ".join(rng.choice(words) for _ in range(rng.randint(1, 8)))
            t += rng.choice([b"\n", b" ", b"\n\n"])
            if rng.random() < 0.3:
                t += rng.choice(pool) + rng.choice([b"\n", b" "])
        if k == 2:
            t = t[:4960] + pool[0] + pool[1]
        out.append(t[:5000])
    return out


def _built(name):
    """A set of its own (test_lazy_set_host's shared ones must stay as its
    tests expect to find them: rows and links made here would stay in them)."""
    rs = R.RegexSet(SETS[name])
    return rs, OracleRegex(rs)


def _mask(o, t, start):
    return sum(1 << j for j in o.matches(t, start)) if start <= len(t) else 0


@pytest.mark.parametrize("name", CANNOT_QUIT)
def test_units_equal_oracle(name):
    rs, o = _built(name)
    tb = SetLongTables(rs)
    st = Stats(trace=True)
    for texts in (_texts(), long_texts()):
        for start in (0, 3, "len", "len+1"):
            for t in texts:  # (one haystack per call: starts len and len + 1 are per text)
                at = {"len": len(t), "len+1": len(t) + 1}.get(start, start)
                exp = _mask(o, t, at)
                for chunk in CHUNKS:
                    got, _ = lazy_set_long(tb, [t], at, chunk, ahead=0, stats=st)
                    assert got == [exp], (name, len(t), at, chunk, [j for j in range(len(rs)) if (got[0] ^ exp) >> j & 1])
                    check_reach(tb, st)
                    st.trace.clear()
    assert tb.builds > 0 and st.polls > 0  # lanes did park and resume, and units polled
    known = [s for s in range(tb.info["states"]) if tb.strip[s] != UNKNOWN]
    assert len(known) > 2  # (dead, quit and the links the cuts asked for)
    assert tb.reach[0] == 0
    for s in known:
        assert int(tb.reach[tb.strip[s]]) & ~int(tb.reach[s]) == 0, s
    assert 0 < tb.info["rows_built"] < tb.info["states"]


def test_batch_shares_rounds_and_words():
    """Three haystacks in one call: units of all of them park and resume in
    the same rounds, each ORs into its own word."""
    rs, o = _built("no_dfa")
    tb = SetLongTables(R.RegexSet(NO_DFA))
    texts = long_texts()
    for start in (0, 3, 4096):
        got, rounds = lazy_set_long(tb, texts, start, 48, bases=[1 + 5003 * h for h in range(3)])
        assert got == [_mask(o, t, start) for t in texts] and rounds >= 1
    assert len({_mask(o, t, 0) for t in texts}) > 1


def test_reach_bounds_every_walk():
    """For every state a unit passes, every pattern the unit reports later is
    in reach[state] (checked along the whole trace of every unit)."""
    pairs = 0
    for name in ("no_dfa", "mixed", "literals"):
        rs, _ = _built(name)
        tb = SetLongTables(rs)
        st = Stats(trace=True)
        lazy_set_long(tb, long_texts(), 0, 48, stats=st, use_reach=False)
        pairs += check_reach(tb, st)
    assert pairs > 1000


def test_mask_needs_two_units():
    """No single unit's mask is the haystack's: the OR across units is what
    answers."""
    rs, o = _built("no_dfa")
    tb = SetLongTables(rs)
    t = b"x " * 500 + b"a" + b"ab" * 9 + b" y" * 500 + b"bb" + b" z" * 300  # (no `bb` in the run)
    st = Stats()
    got, _ = lazy_set_long(tb, [t], 0, 48, stats=st)
    exp = _mask(o, t, 0)
    assert got == [exp] and exp == 3
    assert all(m != exp for m in st.unit_masks.values())
    assert {m for m in st.unit_masks.values() if m} == {1, 2}


def test_state_without_threads():
    """`bb` across the first cut: past the cut the unit's last thread reaches
    its Match, and the step that reports it enters a state that holds no
    thread at all, only what its entry reported.  That is a live id (not 0)
    whose row is all dead, whose reach is what it reported and which is its
    own twin; the walk enters it and dies on the next byte."""
    rs = R.RegexSet(NO_DFA)
    tb = SetLongTables(rs)
    t = b"." * 14 + b"bb" + b"." * 50
    st = Stats(trace=True)
    assert lazy_set_long(tb, [t], 0, 16, stats=st)[0] == [2]
    passed = {v for kind, v in st.trace[0] if kind == "state"}
    bare = [x for x in passed if tb.built[x] and not tb.trans[x].any()]
    assert bare and 0 not in bare
    assert rs.lazy_strip_build(bare)
    tb.load()
    for x in bare:
        assert tb.reach[x] == tb.now[x] == 2 and tb.eof[x] == 0 and tb.strip[x] == x


def test_links_leave_the_automaton_there_was():
    """A new twin comes after every state there was with its row not built;
    the states that existed keep their ids, rows, masks, flags and reach."""
    rs = R.RegexSet(NO_DFA)
    tb = SetLongTables(rs)
    for t in long_texts():
        lazy_set_long(tb, [t], 0, 1 << 20)  # one unit: rows, no link
    assert (tb.strip[2:] == UNKNOWN).all() and tb.strip[0] == 0
    info, trans, now, eof, built, start, colmap = rs.lazy_tables()
    reach = rs.lazy_reach()
    n = info["states"]
    asked = [s for s in range(2, n) if built[s]][:50]
    assert asked and rs.lazy_strip_build(asked)
    info2, trans2, now2, eof2, built2, start2, colmap2 = rs.lazy_tables()
    assert info2["states"] > n and info2["rows_built"] == info["rows_built"]
    for a, b in ((trans, trans2[:n]), (now, now2[:n]), (eof, eof2[:n]), (built, built2[:n]), (start, start2),
                 (colmap, colmap2), (reach, rs.lazy_reach()[:n])):
        assert a.tobytes() == b.tobytes()
    assert not built2[n:].any() and (trans2[n:] == UNKNOWN).all()
    strip = rs.lazy_strip()
    twins = {int(strip[s]) for s in asked}
    assert any(x >= n for x in twins) and all(strip[x] == x for x in twins)
    again = strip.copy()
    assert rs.lazy_strip_build(asked + sorted(twins)) and np.array_equal(rs.lazy_strip(), again)
    # the walks still answer as before on the grown automaton
    tb.load()
    o = OracleRegex(rs)
    for t in long_texts():
        assert lazy_set_long(tb, [t], 0, 48)[0] == [_mask(o, t, 0)]


def test_budget_spent(knobs):
    knobs(big_bytes=4096)
    rs = R.RegexSet(NO_DFA)
    tb = SetLongTables(rs)  # (the budget is read when the automaton is created)
    knobs()
    assert lazy_set_long(tb, long_texts(), 0, 48)[0] is None
    todo = [s for s in range(2, tb.info["states"]) if tb.strip[s] == UNKNOWN]
    assert todo and rs.lazy_strip_build(todo[:1]) is False


@pytest.mark.parametrize("pats", [[r"^abc", r"^\d+ x"], [r"\bfoo", "bar"], CASES["c4"][0],
                                  ["p%d" % i for i in range(65)]],
                         ids=["anchored_start", "unicode_wb", "c4", "65_patterns"])
def test_no_links(pats):
    rs = R.RegexSet(pats)
    with pytest.raises(RuntimeError):
        rs.lazy_strip()
    with pytest.raises(RuntimeError):
        rs.lazy_reach()
    with pytest.raises(RuntimeError):
        rs.lazy_strip_build([2])


def test_anchored_start_has_the_automaton():
    R.RegexSet([r"^abc", r"^\d+ x"]).lazy_tables()  # (it is the links it lacks)


def linger_text():
    """64 KiB of request lines, a GET in every one (so in the first KiB and in
    every unit), no `bb` and no a/b run: pattern 0 matches from the first
    line on and its `.*` thread never dies, the other two never match."""
    line = b"GET /index/%04d HTTP/1.1 200 1532\n"
    t = b"".join(line % (i % 10000) for i in range((64 << 10) // 33 + 1))
    return t[:64 << 10]


def test_reach_exit_ends_lingering_threads():
    """Every unit's `.*` thread survives its cut.  Without the exit unit k of
    the 16 walks from its start to the end of the text, (16 + 1) / 2 = 8.5
    text lengths in all; with it a unit walks its 4096 bytes and leaves at the
    first poll after its cut that sees pattern 0 in the word (at most 512
    bytes on), fewer than 4096 + 512 + 16 bytes a unit, 1.13 text lengths."""
    rs = R.RegexSet(LINGER)
    assert not rs.uses_dfa()
    t = linger_text()
    assert len(t) == 64 << 10 and b"GET" in t[:1024] and b"bb" not in t
    exp = _mask(OracleRegex(rs), t, 0)
    assert exp == 1
    tb = SetLongTables(rs)
    with_exit, without = Stats(), Stats()
    assert lazy_set_long(tb, [t], 0, 4096, ahead=16, stats=with_exit)[0] == [exp]
    assert lazy_set_long(tb, [t], 0, 4096, ahead=16, stats=without, use_reach=False)[0] == [exp]
    print("steps with the reach exit %d, without %d, text %d" % (with_exit.steps, without.steps, len(t)))
    assert with_exit.steps < 2 * len(t)
    assert without.steps >= 4 * with_exit.steps
    assert with_exit.left >= 15 and without.left == 0
