"""The ownership rule of the record scan (regex_amd/csrc/kernels/
records_device.hpp) on the CPU: rure_amd_records_units runs the device's own
walk over a host text and is compared with a plain restatement -- a record
starts at 0 and at p + 1 for each delimiter at p with p + 1 < n, and belongs
to unit start // chunk."""
import ctypes

import numpy as np
import pytest

from regex_amd import _native as N

NONE = (1 << 64) - 1
CHUNKS = (16, 17, 48, 4096)


def restated(text, delim, chunk):
    n = len(text)
    starts = ([0] if n else []) + [p + 1 for p in range(n) if text[p] == delim and p + 1 < n]
    units = -(-n // chunk)
    first, count = [NONE] * units, [0] * units
    for s in starts:
        u = s // chunk
        if count[u] == 0:
            first[u] = s
        count[u] += 1
    return units, first, count, len(starts)


def native(text, delim, chunk, misalign=0):
    """The export over `text` placed `misalign` bytes past a 16-byte boundary."""
    n = len(text)
    raw = np.zeros(n + 64, dtype=np.uint8)
    off = (-raw.ctypes.data) % 16 + misalign
    raw[off:off + n] = np.frombuffer(bytes(text), dtype=np.uint8)
    units = -(-n // chunk)
    first = (ctypes.c_uint64 * max(units, 1))()
    count = (ctypes.c_uint64 * max(units, 1))()
    got = N.rure_amd_records_units(ctypes.c_void_p(raw.ctypes.data + off), n, delim, chunk, first, count, units)
    return got, list(first)[:units], list(count)[:units]


def check(text, delim, chunk, misalign=0):
    units, first, count, nrec = restated(text, delim, chunk)
    got, gfirst, gcount = native(text, delim, chunk, misalign)
    assert got == units
    assert gfirst == first, (bytes(text), chunk, misalign)
    assert gcount == count, (bytes(text), chunk, misalign)
    assert sum(gcount) == nrec


@pytest.mark.parametrize("chunk", CHUNKS)
def test_random_texts(chunk):
    """Random texts of up to 600 bytes over {a, b, delim}, delimiter densities
    from none to every byte, ending with and without a delimiter, at every
    placement class within a 16-byte block."""
    rng = np.random.default_rng(0xD311 + chunk)
    delim = 10
    for density in (0.0, 0.01, 0.05, 0.2, 0.5, 0.9, 1.0):
        for i in range(12):
            n = int(rng.integers(0, 601))
            t = np.where(rng.random(n) < density, delim, rng.choice([97, 98], size=n)).astype(np.uint8)
            for end in (97, delim):
                if n:
                    t[-1] = end
                check(bytearray(t.tobytes()), delim, chunk, misalign=(i * 5 + 1) % 16)


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("delim", [10, 0, ord(";"), 255])
def test_lengths_around_a_chunk(chunk, delim):
    fill = 97 if delim != 97 else 98
    for n in (0, 1, chunk - 1, chunk, chunk + 1):
        if n > 600 + 4096:
            continue
        for pattern in ("none", "all", "last", "first"):
            t = bytearray([fill]) * n
            if pattern == "all":
                t = bytearray([delim]) * n
            elif pattern == "last" and n:
                t[-1] = delim
            elif pattern == "first" and n:
                t[0] = delim
            check(t, delim, chunk)
            check(t, delim, chunk, misalign=1)


@pytest.mark.parametrize("chunk", (16, 17, 48))
def test_delimiter_at_the_cuts(chunk):
    """A single delimiter exactly at c0 - 1, c0 and c1 - 1 of unit 1 (and of
    the last unit), alone and together, with the text ending there or later."""
    delim = 10
    c0, c1 = chunk, 2 * chunk
    for n in (c1 - 1, c1, c1 + 1, 3 * chunk + 5):
        for spots in ([c0 - 1], [c0], [c1 - 1], [c0 - 1, c0], [c0 - 1, c0, c1 - 1], [c0 - 2, c1 - 2], [n - 1]):
            t = bytearray(b"a") * n
            for p in spots:
                if p < n:
                    t[p] = delim
            for mis in (0, 1, 15):
                check(t, delim, chunk, misalign=mis)


def test_surroundings_do_not_count():
    """The search loads whole 16-byte blocks: delimiters right before and
    after the text change nothing."""
    body = bytearray(b"ab\nabb\n\nb")
    n = len(body)
    raw = np.full(n + 64, 10, dtype=np.uint8)
    for mis in range(16):
        off = (-raw.ctypes.data) % 16 + 16 + mis
        raw[:] = 10
        raw[off:off + n] = np.frombuffer(bytes(body), dtype=np.uint8)
        units, first, count, nrec = restated(body, 10, 16)
        gf = (ctypes.c_uint64 * units)()
        gc = (ctypes.c_uint64 * units)()
        assert N.rure_amd_records_units(ctypes.c_void_p(raw.ctypes.data + off), n, 10, 16, gf, gc, units) == units
        assert list(gf) == first and list(gc) == count and sum(gc) == nrec == 4


def test_bad_arguments():
    assert N.rure_amd_records_units(None, 5, 10, 16, None, None, 0) == N.ERR_ARG
    buf = (ctypes.c_uint8 * 4)(97, 10, 97, 10)
    assert N.rure_amd_records_units(buf, 4, 10, 0, None, None, 0) == N.ERR_ARG
    assert N.rure_amd_records_units(None, 0, 10, 16, None, None, 0) == 0
    assert N.rure_amd_records_units(buf, 4, 10, 3, None, None, 0) == 2
