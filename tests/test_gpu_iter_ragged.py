"""The ragged unit geometry of the batched find_iter: an offset batch whose
haystacks are cut into units by their own lengths (iter_device.hpp Geo::uoff).

Knobs iter_ragged=2, iter_chunk=16 cut every haystack into 16-byte units, so
that matches cross unit cuts everywhere, and unit cuts, haystack ends and
empty haystacks meet in every combination.  Expected values come from the CPU
oracle, one haystack at a time; N.last_iter_units() tells that the batch
really was cut.  Every batch buffer is exactly its text plus 16 bytes."""
import numpy as np
import pytest

import regex_amd as R
from regex_amd import _native as N
from golden_data import corpus
from oracle_py import OracleRegex

pytestmark = pytest.mark.gpu

UNIT = 16
PLAIN = r"[A-Z][a-z]+ (Holmes|Watson)"  # match type Dfa: the chunked iteration answers it
SUFFIX = r"[A-Z][a-z]+ Holmes"          # match type DfaSuffix, iterated like the forward DFA: see _chunked


def _chunked(re):
    """Whether the chunked iteration answers this regex's find_iter over an
    offset batch that the knobs or a long haystack make ragged.  The
    reference's DfaSuffix and anchored-start Literal searches are not the
    forward DFA's in general (`xa*ingb*ing|a+ing` over
    `xaaingbing`): those regexes keep one haystack per wavefront, except a
    DfaSuffix regex no match of which holds its suffix but at its end
    (rure_amd_suffix_forward), like SUFFIX."""
    mt = re.match_info()["match_type"]
    return mt in ("Dfa", "Literal(Unanchored)", "Literal(AnchoredEnd)") or N.rure_amd_suffix_forward(re._re) == 1


@pytest.fixture(scope="module")
def sherlock():
    return corpus("sherlock")[:200000]


@pytest.fixture(scope="module")
def dna():
    return corpus("regexdna")[:200000]


def _dev(texts, cuda, pad=b"\0" * 16):
    """(buffer, offsets) on the device: the texts back to back and 16 bytes."""
    import torch
    assert len(pad) == 16
    offs = np.zeros(len(texts) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(t) for t in texts])
    buf = np.frombuffer(b"".join(texts) + pad, dtype=np.uint8).copy()
    assert buf.size == int(offs[-1]) + 16
    return torch.from_numpy(buf).to(cuda), torch.from_numpy(offs).to(cuda)


def _units(texts, unit=UNIT, start=0):
    return sum(max(1, -(-max(0, len(t) - start) // unit)) for t in texts)


def _expected(o, texts, start=0):
    return [o.find_iter(t, start) for t in texts]


def _run(re, hay, offs, start=0):
    counts, m = re.find_iter_batch(hay, offsets=offs, start=start)
    return counts.cpu().numpy().tolist(), [(int(a), int(b)) for a, b in m.cpu().numpy()]


def _compare(counts, got, exp, what):
    k = 0
    for i, e in enumerate(exp):
        assert counts[i] == len(e), (what, i, counts[i], len(e))
        assert got[k:k + len(e)] == e, (what, i, got[k:k + len(e)][:4], e[:4])
        k += len(e)
    assert k == len(got), (what, k, len(got))


# ---------------------------------------------------------------- 1. geometry

LENS = [0, 1, 15, 16, 17, 31, 32, 33, 0, 0, 160, 5, 161, 1000, 0, 48]


def _orderings():
    first = [1000] + [x for x in LENS if x != 1000]
    last = [x for x in LENS if x != 1000] + [1000]
    return {"as_listed": LENS, "longest_first": first, "longest_last": last}


@pytest.mark.parametrize("order", sorted(_orderings()))
@pytest.mark.parametrize("pat", [r"[A-Za-z]+ [a-z]+", r"a*", r"(?-u)\b\w+\b"])
def test_geometry_edges(cuda, sherlock, pat, order):
    """Empty haystacks between long ones, exact multiples of the unit, a
    one-byte last unit, consecutive multi-unit haystacks."""
    lens = _orderings()[order]
    texts = [sherlock[5000 + 1500 * i:5000 + 1500 * i + n] for i, n in enumerate(lens)]
    re = R.Regex(pat)
    exp = _expected(OracleRegex(re), texts)
    hay, offs = _dev(texts, cuda)
    with R.debug(iter_ragged=2, iter_chunk=UNIT):
        counts, got = _run(re, hay, offs)
        units = N.last_iter_units()
    _compare(counts, got, exp, (pat, order))
    assert units == (_units(texts), len(texts))
    assert units[0] == sum(max(1, -(-n // UNIT)) for n in lens) > len(lens)


# ----------------------------------------------------- 2. engines and quirks

def _dense_text(o, text, size, rng):
    """About `size` bytes of `text` made of windows around the regex's
    non-empty matches (repeated if they are few), so that matches are dense."""
    ms = [(s, e) for s, e in o.find_iter(text) if e > s]
    assert ms, "the pattern has no non-empty match in the text"
    parts, n, i = [], 0, 0
    while n < size:
        s, e = ms[i % len(ms)]
        w = text[max(0, s - int(rng.integers(0, 40))):min(len(text), e + int(rng.integers(0, 40)))]
        parts.append(w)
        n += len(w)
        i += 1
    return b"".join(parts)


def _slices(o, text, n, rng, forced=25):
    """`text` cut into n consecutive haystacks of 0..600 bytes; `forced` of
    the cuts fall inside a match of the uncut text (after its first byte:
    haystack h ends with a match's prefix, h + 1 begins with the rest), or,
    for a regex whose matches are single bytes or empty, right at a match end.
    Returns the haystacks and the number of forced cuts."""
    ms = o.find_iter(text)
    inside = [int(rng.integers(s + 1, e)) for s, e in ms if e - s >= 2]
    ends = [e for s, e in ms if 0 < e < len(text)]
    pool = inside if len(inside) >= forced else ends
    pick = sorted(set(int(x) for x in rng.choice(pool, size=min(forced, len(pool)), replace=False)))
    cuts = set(pick)
    while len(cuts) < n - 1:
        cuts.add(int(rng.integers(1, len(text))))
    cuts = sorted(cuts)
    # not inside a UTF-8 sequence (planted letters): move to its first byte
    cuts = sorted(set(c - 1 if 0x80 <= text[c] < 0xC0 else c for c in cuts))
    texts, last = [], 0
    for c in cuts:
        texts.append(text[last:c][:600])
        last = c
    texts.append(text[last:][:600])
    # a few empty haystacks between the others
    for k in range(5, len(texts), 37):
        texts.insert(k, b"")
    return texts, len(pick)


def _plant_nonascii(text, rng):
    out, last = [], 0
    for p in range(30, len(text) - 1, 50):
        q = p + int(rng.integers(0, 10))
        if q < len(text) and 97 <= text[q] <= 122:
            out.append(text[last:q])
            out.append("é".encode())
            last = q + 1
    out.append(text[last:])
    return b"".join(out)


def _engine_case(cuda, pat, text, seed, dense=True, planted=False, at=False, words=()):
    rng = np.random.default_rng(seed)
    if words:  # the text has none of them: written over it every ~40 bytes
        t = bytearray(text[:60000].lower())
        for p in range(20, len(t) - 50, 40):
            w = words[int(rng.integers(0, len(words)))]
            q = p + int(rng.integers(0, 20))
            t[q:q + len(w)] = w
        text = bytes(t)
    if at:  # e-mail-like words for \w+@\w+
        text = bytes(64 if (c == 32 and i % 7 == 0) else c for i, c in enumerate(text))
    re = R.Regex(pat)
    o = OracleRegex(re)
    body = _dense_text(o, text[:60000], 60000, rng)
    if planted:
        body = _plant_nonascii(body, rng)
    texts, forced = _slices(o, body, 200, rng)
    assert forced >= 20 and len(texts) >= 200
    exp = _expected(o, texts)
    crossing = sum(1 for e in exp for s, t in e if t > s and s // UNIT != (t - 1) // UNIT)
    if dense:  # the inputs do put matches across unit cuts
        assert crossing >= 50, (pat, crossing)
    hay, offs = _dev(texts, cuda)
    with R.debug(iter_ragged=2, iter_chunk=UNIT):
        counts, got = _run(re, hay, offs)
        units = N.last_iter_units()
    _compare(counts, got, exp, pat)
    if _chunked(re):  # in its ragged form
        assert units == (_units(texts), len(texts)), (pat, units)


@pytest.mark.parametrize("pat", [
    PLAIN,                   # plain DFA, matches crossing unit cuts
    SUFFIX,                  # DfaSuffix, its suffix only at a match's end
    r"[a-z]+ing",            # DfaSuffix, not so (`singing`): one haystack per wavefront, results only
    r"Holmes|Watson|the",    # string set: the literal kernel
    r"(?-u)\b\w+n\b",        # look-around, U_UNSURE
    r"(?m)^\w+",             # multi-line start anchor
])
def test_engines_sherlock(cuda, sherlock, pat):
    _engine_case(cuda, pat, sherlock, seed=len(pat))


def test_engine_empty_matches(cuda, sherlock):
    """a*: the e + 1 rule at unit and haystack ends (its matches are single
    bytes or empty: forced cuts fall at match ends, nothing crosses a cut)."""
    _engine_case(cuda, r"a*", sherlock, seed=3, dense=False)


@pytest.mark.parametrize("planted", [False, True])
def test_engine_ascii_shadow(cuda, sherlock, planted):
    """\\w+@\\w+: a Unicode class with an ASCII shadow, over ASCII text and
    over text with a non-ASCII letter every ~50 bytes (the shadow quits)."""
    _engine_case(cuda, r"\w+@\w+", sherlock, seed=5 + planted, planted=planted, at=True)


def test_engine_unicode_word_boundary(cuda, sherlock):
    """\\b\\w+n\\b over planted non-ASCII letters: units served by waves."""
    _engine_case(cuda, r"\b\w+n\b", sherlock, seed=9, planted=True)


def test_engine_shift_and(cuda, dna):
    """agggtaaa|tttaccct over DNA: the per-lane Shift-And kernel (the fixture
    holds neither string, so they are planted)."""
    _engine_case(cuda, r"agggtaaa|tttaccct", dna, seed=11, words=(b"agggtaaa", b"tttaccct"))


@pytest.mark.parametrize("pat", [r"^abc", r"abc$"])
def test_engine_anchors(cuda, pat):
    rng = np.random.default_rng(len(pat) * 7)
    texts = []
    for i in range(200):
        n = int(rng.integers(0, 600))
        t = bytes(rng.choice(np.frombuffer(b"abcx \n", dtype=np.uint8), size=n).tobytes())
        if i % 3 == 0:
            t = b"abc" + t
        if i % 4 == 0:
            t = t + b"abc"
        texts.append(t)
    re = R.Regex(pat)
    exp = _expected(OracleRegex(re), texts)
    assert sum(len(e) for e in exp) >= 40
    hay, offs = _dev(texts, cuda)
    with R.debug(iter_ragged=2, iter_chunk=UNIT):
        counts, got = _run(re, hay, offs)
    _compare(counts, got, exp, pat)


# ----------------------------------------------------------------- 3. start

@pytest.mark.parametrize("start", [3, 20])
@pytest.mark.parametrize("pat", [PLAIN, r"a*", r"(?-u)\b\w+n\b"])
def test_start_offset(cuda, sherlock, pat, start):
    """Against the one-unit-per-haystack form (iter_ragged=0), with haystacks
    shorter than `start` among the others."""
    rng = np.random.default_rng(start)
    re = R.Regex(pat)
    o = OracleRegex(re)
    texts, _ = _slices(o, _dense_text(o, sherlock[:60000], 30000, rng), 120, rng)
    texts[3:3] = [b"", b"ab", sherlock[100:100 + start - 1], sherlock[200:200 + start], sherlock[300:300 + start + 1]]
    hay, offs = _dev(texts, cuda)
    with R.debug(iter_ragged=0):
        ref = _run(re, hay, offs, start)
        assert N.last_iter_units()[0] == N.last_iter_units()[1]
    with R.debug(iter_ragged=2, iter_chunk=UNIT):
        got = _run(re, hay, offs, start)
        units = N.last_iter_units()
    assert got == ref
    _compare(got[0], got[1], _expected(o, texts, start), (pat, start))
    assert units == (_units(texts, start=start), len(texts))


# ---------------------------------------------------------------- 4. riders

def test_riders_agree(cuda, sherlock):
    """replace, `$`-expanding replace, split and captures_iter sit on the
    batched find_iter: the same outputs in either geometry."""
    rng = np.random.default_rng(4)
    re = R.Regex(r"([A-Z][a-z]+) (Holmes|Watson)")
    o = OracleRegex(re)
    texts, _ = _slices(o, _dense_text(o, sherlock, 30000, rng), 100, rng)
    hay, offs = _dev(texts, cuda)

    def riders():
        out = []
        for t in re.replace_batch(hay, b"<X>", offsets=offs):
            out.append(t.cpu().numpy().tolist())
        for t in re.replace_batch(hay, b"[$2, $1]", offsets=offs, expand=True):
            out.append(t.cpu().numpy().tolist())
        for t in re.split_batch(hay, offsets=offs):
            out.append(t.cpu().numpy().tolist())
        for t in re.captures_iter_batch(hay, offsets=offs):
            out.append(t.cpu().numpy().tolist())
        return out

    with R.debug(iter_ragged=0):
        ref = riders()
        assert N.last_iter_units()[0] == len(texts)
    with R.debug(iter_ragged=2, iter_chunk=UNIT):
        got = riders()
        assert N.last_iter_units() == (_units(texts), len(texts))
    assert got == ref
    assert sum(ref[6]) >= 100  # captures_iter's counts: there were matches to ride on


# ----------------------------------------------------- 5. production geometry

@pytest.mark.parametrize("pat", [PLAIN, SUFFIX])
def test_production_geometry(cuda, sherlock, pat):
    """No knobs: a batch with a haystack of 256 KiB or more is cut, a batch of
    short haystacks keeps one unit per haystack.

    SUFFIX is of the DfaSuffix match type: it is cut because its iteration
    is the forward DFA's (rure_amd_suffix_forward); PLAIN is the same search
    of match type Dfa."""
    def rep(n, at):
        piece = sherlock[at:at + 50000]
        return (piece * (n // len(piece) + 1))[:n]

    rng = np.random.default_rng(5)
    short = [sherlock[1000 * i:1000 * i + int(rng.integers(0, 201))] for i in range(50)]
    texts = [rep(300 * 1024 + 7, 0), sherlock[777:782], rep((1 << 20) + 1, 60000)] + short
    re = R.Regex(pat)
    o = OracleRegex(re)
    hay, offs = _dev(texts, cuda)
    counts, got = _run(re, hay, offs)
    units = N.last_iter_units()
    _compare(counts, got, _expected(o, texts), "long among short")
    assert sum(counts) > 100
    assert units[0] > 53 and units[1] == 53

    texts = [texts[1]] + short
    hay, offs = _dev(texts, cuda)
    counts, got = _run(re, hay, offs)
    assert N.last_iter_units() == (51, 51)
    _compare(counts, got, _expected(o, texts), "short only")


# ---------------------------------------------------------------- 6. buffer end

@pytest.mark.parametrize("tail", [1, 14, 16, 17, 40])
def test_buffer_end(cuda, sherlock, tail):
    """The buffer is exactly the text plus 16 bytes, the last haystack ends
    inside a would-be match and the bytes after it would complete it: nothing
    past a haystack's end is read as text."""
    re = R.Regex(PLAIN)
    o = OracleRegex(re)
    last = (b"x" * 64 + b"Mr. Sherlock Holmes and Sherlock Hol")[-tail:]
    texts = [sherlock[3000:3000 + 333], b"", b"Sherlock Holmes. Sherlock Hol", last]
    hay, offs = _dev(texts, cuda, pad=b"mes and Watson. ")
    assert hay.numel() == sum(len(t) for t in texts) + 16
    with R.debug(iter_ragged=2, iter_chunk=UNIT):
        counts, got = _run(re, hay, offs)
        assert N.last_iter_units() == (_units(texts), len(texts))
    _compare(counts, got, _expected(o, texts), tail)
    assert counts[2] == 1 and counts[3] == (1 if tail == 40 else 0)
