"""The deferred long scan of find / is_match / shortest_match over an offset
batch: the one-lane-per-haystack kernel leaves the long haystacks on a device
list and a chunked scan of the listed ones follows, nothing read back
(dispatch.cpp run_ragged_long, long_scan.hip).

Knobs long_ragged=2, long_chunk=16 defer every haystack of more than 16 bytes
to search and cut it into 16-byte units, so that matches cross unit cuts
everywhere and deferred and undeferred haystacks mix in one batch.  Expected
values come from the CPU oracle, one haystack at a time; N.last_long_units()
tells what was deferred.  Every batch buffer is exactly its text plus 16
bytes."""
import numpy as np
import pytest

import regex_amd as R
from regex_amd import _native as N
from golden_data import corpus
from oracle_py import OracleRegex

pytestmark = pytest.mark.gpu

UNIT = 16
PLAIN = r"[A-Z][a-z]+ (Holmes|Watson)"
MODES = ("find", "is_match", "shortest_match")
KNOBS = dict(long_ragged=2, long_chunk=UNIT)


@pytest.fixture(scope="module")
def sherlock():
    return corpus("sherlock")[:200000]


@pytest.fixture(scope="module")
def lanes(cuda):
    """The lanes in flight the chunk rule divides the deferred bytes by."""
    import torch
    return torch.cuda.get_device_properties(cuda).multi_processor_count * 1024


def _dev(texts, cuda, pad=b"\0" * 16):
    """(buffer, offsets) on the device: the texts back to back and 16 bytes."""
    import torch
    assert len(pad) == 16
    offs = np.zeros(len(texts) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(t) for t in texts])
    buf = np.frombuffer(b"".join(texts) + pad, dtype=np.uint8).copy()
    assert buf.size == int(offs[-1]) + 16
    return torch.from_numpy(buf).to(cuda), torch.from_numpy(offs).to(cuda)


def _expected(o, texts, start=0, modes=MODES):
    """Per mode the oracle's answers in the batched calls' output form."""
    exp = {}
    if "find" in modes:
        exp["find"] = [list(o.find(t, start) or (-1, -1)) for t in texts]
    if "is_match" in modes:
        exp["is_match"] = [int(o.is_match(t, start)) for t in texts]
    if "shortest_match" in modes:
        exp["shortest_match"] = [(lambda e: -1 if e is None else e)(o.shortest_match(t, start)) for t in texts]
    return exp


def _call(re, mode, hay, offs, start=0):
    out = getattr(re, mode + "_batch")(hay, offsets=offs, start=start)
    return out.cpu().numpy().tolist()


def _geometry(texts, lanes, start=0, floor=UNIT, least=None, cap=None, rounded=False):
    """(units, haystacks, chunk) as the device makes them from the lengths:
    the spans of `least` bytes or more are deferred, the chunk is their sum
    over the lanes in flight, at least the floor."""
    least = floor + 1 if least is None else least
    spans = [max(0, len(t) - start) for t in texts]
    spans = [s for s in spans if s >= least]
    if cap is not None:
        assert len(spans) <= cap
    if not spans:
        return (0, 0, 0)
    c = max(floor, -(-sum(spans) // lanes))
    if rounded:  # odd_lines
        lines = -(-c // 128)
        c = 128 * (lines + (lines % 2 == 0))
    return (sum(max(1, -(-s // c)) for s in spans), len(spans), c)


def _check(re, texts, cuda, lanes, start=0, modes=MODES, knobs=KNOBS, deferred=True, what=None):
    """All modes against the oracle; the diagnostic against the lengths
    (deferred=False: a regex that keeps one lane per haystack)."""
    exp = _expected(OracleRegex(re), texts, start, modes)
    hay, offs = _dev(texts, cuda)
    paths = {}
    for mode in modes:
        with R.debug(**knobs):
            got = _call(re, mode, hay, offs, start)
            units = N.last_long_units()
            paths[mode] = N.last_path()
        assert got == exp[mode], (what, mode, [(i, g, e) for i, (g, e) in enumerate(zip(got, exp[mode])) if g != e][:4])
        if deferred:
            assert units == _geometry(texts, lanes, start, floor=knobs.get("long_chunk", UNIT)), (what, mode, units)
        else:
            assert units == (0, 0, 0), (what, mode, units)
    return exp, paths


# ---------------------------------------------------------------- 1. geometry

LENS = [0, 1, 15, 16, 17, 31, 32, 33, 0, 0, 160, 5, 161, 1000, 0, 48]


def _orderings():
    first = [1000] + [x for x in LENS if x != 1000]
    last = [x for x in LENS if x != 1000] + [1000]
    return {"as_listed": LENS, "longest_first": first, "longest_last": last}


def _geometry_texts(o, sherlock, lens):
    """Haystacks of the given lengths cut from the text so that one of the
    regex's matches lies in each that has room for it, some way in."""
    ms = o.find_iter(sherlock)
    assert len(ms) >= len(lens)
    texts = []
    for i, n in enumerate(lens):
        s, e = ms[(7 * i) % len(ms)]
        at = max(0, s - (n - (e - s)) * 2 // 3) if n >= e - s else s
        texts.append(sherlock[at:at + n])
    return texts


@pytest.mark.parametrize("order", sorted(_orderings()))
def test_geometry_edges(cuda, sherlock, lanes, order):
    """Empty haystacks between deferred ones, exact multiples of the unit, a
    one-byte last unit; haystacks of at most one chunk stay with their lane."""
    lens = _orderings()[order]
    re = R.Regex(PLAIN)
    texts = _geometry_texts(OracleRegex(re), sherlock, lens)
    exp, paths = _check(re, texts, cuda, lanes, what=order)
    assert sum(exp["is_match"]) >= 4
    geo = _geometry(texts, lanes)
    assert geo == (sum(-(-n // UNIT) for n in lens if n > UNIT), sum(n > UNIT for n in lens), UNIT)
    assert set(paths.values()) == {N.Path.LINES}


# ------------------------------------------- 2. the winning unit, the match end

def _filler(n):
    return (b"the quick brown fox jumps over a lazy dog, " * (n // 43 + 1))[:n]


def _unit_cases():
    nl_free = _filler(1500).replace(b"a", b"e").replace(b"z", b"s").replace(b"b", b"d")
    return {
        "no_match": (PLAIN, _filler(3000)),
        "last_unit_only": (PLAIN, _filler(1600) + b"Dr Watson."),            # starts at 1600 = 100 units in
        "ends_at_the_end": (PLAIN, _filler(1603) + b"Dr Watson"),            # the end-of-text step reports it
        "first_unit_to_far_end": (r"a[^\n]*z", b"a" + nl_free + b"z" + nl_free[:300] + b"z" + nl_free[:50]),
        "later_unit_ends_earlier": (r"a.*z|b", b"a" + nl_free[:500] + b"b" + nl_free[:500] + b"z" + nl_free[:100]),
        "empty_at_start": (r"a*", b"b" + _filler(700)),
        "empty_after_run": (r"a*", b"aaa" + _filler(700)),
        "never_dies": (r"[^\n]*", nl_free + nl_free),
    }


@pytest.mark.parametrize("case", sorted(_unit_cases()))
def test_winning_unit(cuda, lanes, case):
    pat, text = _unit_cases()[case]
    assert b"\n" not in text and len(text) > 40 * UNIT
    texts = [b"", text, text[:UNIT], text[:40], text]
    exp, _ = _check(R.Regex(pat), texts, cuda, lanes, what=case)
    if case == "no_match":
        assert exp["find"][1] == [-1, -1]
    if case == "last_unit_only":
        assert exp["find"][1] == [1600, 1609]
    if case == "ends_at_the_end":
        assert exp["find"][1][1] == len(text)
    if case == "first_unit_to_far_end":
        assert exp["find"][1][0] == 0 and exp["find"][1][1] > 100 * UNIT
    if case == "later_unit_ends_earlier":  # the `b` ends a match first, the unit of the `a` wins
        assert exp["find"][1] == [0, 1003] and exp["shortest_match"][1] < 1003
    if case == "empty_at_start":
        assert exp["find"][1] == [0, 0]
    if case == "never_dies":
        assert exp["find"][1] == [0, len(text)]


# ----------------------------------------------------------------- 3. start

START = 7


@pytest.mark.parametrize("pat,chunked", [
    (PLAIN, True),
    (r"(?m)^[A-Z]\w+", True),          # look-behind at `start`
    (r"(?-u:\b)Holmes", False),        # DfaSuffix: the lane search keeps it
    (r"(?-u:\B)(olmes|atson)", True),  # Dfa: a forward end, no start from inside the slice
])
def test_start_offset(cuda, sherlock, lanes, pat, chunked):
    """start = 7 with haystacks shorter than, equal to and just longer than
    it; the reverse scan sees text[start..] only (a match the
    forward scan ends may have no start, and then is no match)."""
    re = R.Regex(pat)
    o = OracleRegex(re)
    at = sherlock.index(b"Sherlock Holmes", 5000)
    body = sherlock[at - 500:at + 700]
    texts = [
        b"", b"abc", sherlock[100:100 + START - 1], sherlock[200:200 + START], sherlock[300:300 + START + 1],
        b"abcdef\nHolmes went out. " + body,   # a line starts at `start`
        b"abcdefgHolmes went out. " + body,    # `start` inside a word
        b"xxxxx Holmes and Watson  " * 30,     # `start` on the `o`: \B holds there, the slice hides the `H`
        b"Sherlock Holmes, " + body, body[:START + UNIT], body[:START + UNIT + 1],
    ]
    exp, _ = _check(re, texts, cuda, lanes, start=START, deferred=chunked, what=pat)
    assert any(e != [-1, -1] for e in exp["find"])
    if pat == r"(?-u:\B)(olmes|atson)":  # the quirk is in the inputs
        assert exp["find"][7] == [-1, -1] and exp["is_match"][7] == 1
    if chunked:
        assert _geometry(texts, lanes, START)[1] == sum(len(t) - START > UNIT for t in texts) >= 5


# ------------------------------------------------------ 4. both lane kernels

@pytest.mark.parametrize("order", sorted(_orderings()))
def test_lane_stream_defers(cuda, sherlock, lanes, order):
    """lines=0: the offsets form of the one-lane-per-haystack stream kernel."""
    re = R.Regex(PLAIN)
    texts = _geometry_texts(OracleRegex(re), sherlock, _orderings()[order])
    _, paths = _check(re, texts, cuda, lanes, knobs=dict(KNOBS, lines=0), what=order)
    assert set(paths.values()) == {N.Path.LANE_STREAM}


# ------------------------------------------------------------ 5. literal engine

def test_literal_engine_defers(cuda, sherlock, lanes):
    re = R.Regex(r"Sherlock|Holmes")
    texts = _geometry_texts(OracleRegex(re), sherlock, LENS + [3000, 700])
    modes = ("find", "is_match")  # what the literal engine answers
    exp_lit, paths = _check(re, texts, cuda, lanes, modes=modes, knobs=dict(KNOBS, lit=1), what="lit=1")
    assert set(paths.values()) == {N.Path.LITERAL}
    exp_dfa, paths = _check(re, texts, cuda, lanes, modes=modes, knobs=dict(KNOBS, lit=0), what="lit=0")
    assert N.Path.LITERAL not in paths.values()
    assert exp_lit == exp_dfa and sum(exp_lit["is_match"]) >= 3
    assert _geometry(texts, lanes)[1] > 0


# ------------------------------------------------- 6. exclusions keep their path

@pytest.mark.parametrize("pat", [
    r"\w+$",         # DfaAnchoredReverse: reads the match from the end
    r"\bHolmes\b",   # a Unicode word boundary: the DFA can quit
    r"[a-z]+ing",    # DfaSuffix: its search is not the forward DFA's
    r"^[A-Za-z ]+",  # anchored at the start: no `.*?` states to strip
])
def test_exclusions_keep_their_path(cuda, sherlock, lanes, pat):
    re = R.Regex(pat)
    texts = [sherlock[1500 * i:1500 * i + n] for i, n in enumerate(LENS + [2500])]
    texts[3] = "é Holmes é".encode() + texts[3]  # (the Unicode \b quits here)
    hay, offs = _dev(texts, cuda)
    with R.debug(long_ragged=0):
        parent = {mode: (_call(re, mode, hay, offs), N.last_path()) for mode in MODES}
    _, paths = _check(re, texts, cuda, lanes, deferred=False, what=pat)
    assert paths == {mode: parent[mode][1] for mode in MODES}
    if pat == r"\w+$":
        assert set(paths.values()) == {N.Path.ANCHORED_REVERSE}


# ------------------------------------------------------ 7. the production rule

DATE = r"\d{4}-\d{2}-\d{2}"


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_production_rule(cuda, sherlock, lanes, where):
    """No knobs: one document of 300 KiB among 200 lines is deferred and cut
    by the rule of long_batch over its bytes; its only match is in its last
    KiB.  Without the document nothing is deferred."""
    rng = np.random.default_rng(7)
    re = R.Regex(DATE)
    o = OracleRegex(re)
    lines = [sherlock[700 * i:700 * i + int(rng.integers(40, 161))] for i in range(200)]
    doc = (sherlock * 2)[:300 * 1024 - 500] + b" on 1887-03-14 it was. " + sherlock[:477]
    assert len(doc) == 300 * 1024 and o.find(doc) == (len(doc) - 496, len(doc) - 486)
    assert not any(o.is_match(t) for t in lines)
    at = {"first": 0, "middle": 100, "last": 200}[where]
    texts = lines[:at] + [doc] + lines[at:]
    exp = _expected(o, texts)
    hay, offs = _dev(texts, cuda)
    chunk = 128 * 129  # odd_lines(max(16 KiB, 300 KiB / lanes))
    assert _geometry(texts, lanes, floor=16 << 10, least=256 << 10, rounded=True) == (-(-len(doc) // chunk), 1, chunk)
    for mode in MODES:
        assert _call(re, mode, hay, offs) == exp[mode], mode
        assert N.last_long_units() == (-(-len(doc) // chunk), 1, chunk), mode
        assert N.last_path() == N.Path.LINES
    assert exp["is_match"] == [int(i == at) for i in range(201)]

    hay, offs = _dev(lines, cuda)
    for mode in MODES:
        got = _call(re, mode, hay, offs)
        assert N.last_long_units() == (0, 0, 0)
        with R.debug(long_ragged=0):
            assert _call(re, mode, hay, offs) == got, mode


# ---------------------------------------------------------- 8. the scratch bound

def test_scratch_bound(cuda, sherlock, lanes):
    """8 MiB under a chunk floor of 16 bytes: the device raises the chunk so
    that the units stay within count + lanes, what the scratch is sized for."""
    rng = np.random.default_rng(8)
    tail = b" on 1887-03-14 it was, Dr Watson said. "
    big = (sherlock * 42)[:(8 << 20) - len(tail)] + tail
    assert len(big) == 8 << 20
    texts = [sherlock[900 * i:900 * i + int(rng.integers(0, 200))] for i in range(50)]
    texts.insert(17, big)
    hay, offs = _dev(texts, cuda)
    for pat in (DATE, PLAIN):
        re = R.Regex(pat)
        exp = _expected(OracleRegex(re), texts, modes=("find", "is_match"))
        for mode in ("is_match", "find"):
            with R.debug(**KNOBS):
                got = _call(re, mode, hay, offs)
                units, n, chunk = N.last_long_units()
            assert got == exp[mode], (pat, mode)
            assert (units, n, chunk) == _geometry(texts, lanes)
            assert chunk > UNIT and n > 1 and units <= len(texts) + lanes
    assert exp["is_match"][17] == 1


# ------------------------------------------------------------ 9. list overflow

def test_list_overflow(cuda, sherlock, lanes):
    """A list of two entries and five haystacks that qualify: two are
    deferred, the other three are scanned by their lanes."""
    re = R.Regex(PLAIN)
    texts = _geometry_texts(OracleRegex(re), sherlock, [900, 10, 1200, 0, 700, 16, 2000, 1500])
    exp = _expected(OracleRegex(re), texts)
    assert sum(exp["is_match"]) >= 3
    hay, offs = _dev(texts, cuda)
    for mode in MODES:
        with R.debug(long_list=2, **KNOBS):
            got = _call(re, mode, hay, offs)
            units, n, chunk = N.last_long_units()
        assert got == exp[mode], mode
        assert n == 2 and chunk == UNIT
        # whichever two the lanes listed first
        assert units in {-(-a // UNIT) + -(-b // UNIT) for a in (900, 1200, 700, 2000, 1500)
                         for b in (900, 1200, 700, 2000, 1500) if a != b}
