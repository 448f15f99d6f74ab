"""CPU check of find_iter on a regex's on-demand forward DFA (host LazyDfa;
kernel: lazy_iter_kernel, big_dfa.hip): the kernel's iteration over the
exported tables (lazy_iter_sim.py), parking on every row not built yet and
resuming inside the search it left, equals the oracle's find_iter
(re_trait.rs:197-221 over exec.rs:632-662) -- for the regex past the eager
state budget and for ordinary ones, reverse NoMatches and skipped empty
matches included; the automaton gives up within its memory budget and is
refused to the regexes that keep their engines."""
import functools

import numpy as np
import pytest

import regex_amd as R
from golden_data import corpus
from oracle_py import OracleRegex
from lazy_iter_sim import HUGE, LOOKS, PLAIN, Tables, lazy_find_iter
from test_gpu_iter_looks import _text


def _mixed(n, L, seed):
    """tests/test_gpu_lazy.py's text: sherlock lines with runs of a/b of
    random lengths (some past 21)"""
    rng = np.random.default_rng(seed)
    base = corpus("sherlock")
    out = bytearray()
    while len(out) < n * L:
        if rng.integers(0, 3) == 0:
            out += bytes(rng.choice(np.frombuffer(b"ab", dtype=np.uint8), size=int(rng.integers(1, 40))))
        else:
            a = int(rng.integers(0, len(base) - 100))
            out += base[a:a + int(rng.integers(1, 100))]
    return bytes(out[:n * L])


@functools.lru_cache(maxsize=None)
def _hays():
    raw = _mixed(40, 200, 5)
    return [raw[i * 200:(i + 1) * 200] for i in range(40)]


def _check(pat, hays):
    re = R.Regex(pat)
    o = OracleRegex(re)
    tb = Tables(re)
    matches = 0
    for start in (0, 3):
        for i, t in enumerate(hays):
            exp = o.find_iter(t, start)
            got = lazy_find_iter(tb, t, start, 0)  # (0 ahead: every new state parks the lane)
            assert got == exp, (pat, start, i)
            matches += len(exp)
    assert tb.builds > 0  # lanes did park and resume
    info = tb.info
    assert info["rows_built"] == int(tb.built.sum()) - 2  # (dead and the unused quit state count as built)
    assert info["hot_rows"] == min(info["states"], (64 << 10) // 4 // info["columns"])
    assert info["rounds"] == 0 and info["fell_back"] == 0  # (no batched call ran)
    return tb, matches


def test_huge_equals_oracle():
    """past the eager budgets: no forward DFA, the reverse one alone"""
    re = R.Regex(HUGE)
    assert not re.uses_dfa() and re.dfa_tables(0) is None and re.dfa_tables(1) is not None
    tb, matches = _check(HUGE, _hays())
    assert matches > 40  # (some haystack holds two matches or more)
    assert 0 < tb.info["rows_built"] < tb.info["states"]  # only what the texts visit is built


@pytest.mark.parametrize("pat", PLAIN)
def test_plain_equals_oracle(pat):
    extra = [b"", b"x", b"xxx", b"on 2024-01-15 and 1999-12-31x", b"The thing\nthe", b"sing a ringing thing"]
    _, matches = _check(pat, _hays() + extra)
    assert matches > 0


@pytest.mark.parametrize("pat", LOOKS)
def test_looks_equal_oracle(pat):
    _check(pat, [_text(seed, 256, False) for seed in range(6)] + [b"", b"a", b"\n", b"ab ab"])


def test_reverse_nomatch_ends_the_iteration():
    r"""(?-u)\B[ab]+ searched from inside a word: the forward DFA finds an end
    (it reads the byte before the start), the reverse scan over
    text[start..end] finds no start (it reads `start` as the text's start),
    and the reference's iteration stops there though matches follow."""
    re = R.Regex(r"(?-u)\B[ab]+")
    o = OracleRegex(re)
    t = b"xxxaxab"
    assert o.find_iter(t, 0) == [(3, 4), (5, 7)]
    assert o.find_iter(t, 3) == []
    tb = Tables(re)
    assert lazy_find_iter(tb, t, 3, 0) == [] and lazy_find_iter(tb, t, 0, 0) == [(3, 4), (5, 7)]


def test_budget_spent(knobs):
    """A few KiB of budget: lazy_build reports it spent, and the simulation
    gives the batch up."""
    knobs(big_bytes=4096)
    re = R.Regex(HUGE)
    tb = Tables(re)  # (the budget is read when the automaton is created)
    knobs()
    got = [lazy_find_iter(tb, t, 0, 0) for t in _hays()]
    assert None in got
    todo = [s for s in range(tb.info["states"]) if not tb.built[s]]
    assert todo and re.lazy_build(todo[:1]) is False
    assert re.lazy_build([], ahead=1) is False


@pytest.mark.parametrize("pat", [r"\bthe\b", r"Watson$"], ids=["unicode_wb", "anchored_reverse"])
def test_no_automaton(pat):
    re = R.Regex(pat)
    with pytest.raises(RuntimeError):
        re.lazy_tables()
    with pytest.raises(RuntimeError):
        re.lazy_build([2])
