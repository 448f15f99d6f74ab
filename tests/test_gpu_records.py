"""Device grep on the GPU (regex_amd/csrc/kernels/records.hip,
Regex.match_records): the records of a raw delimited buffer that match, checked
record by record against the CPU oracle's is_match over a Python split.
Forced onto a few KiB with many cuts (knob records_chunk), by the production
rule on 1 MiB, with other delimiters, inverted, under small capacities, through
the Pike VM, and at the edges."""
import ctypes
import functools

import numpy as np
import pytest

import regex_amd as R
from golden_data import corpus
from oracle_py import OracleRegex
from regex_amd import _native as N

pytestmark = pytest.mark.gpu

MIB = 1 << 20
SENT = -0x5A5A5A5A5A5A5A5B  # what an untouched output entry holds

PATTERNS = [
    r"\d{4}-\d{2}-\d{2}",
    r"Sherlock|Holmes",
    r"[a-z]+ing",       # DfaSuffix
    r"^\s*$",
    r"^Th",
    r"es$",
    r"(?-u)\bthe\b",
    r"x*",
    r"(?s).",           # must select the non-empty records only
    r"\n",              # must select nothing: the delimiter is outside every record
]


def split(text, delim):
    """(start, end) of every record: a start at 0 and after every delimiter,
    provided it is below the length."""
    out, s, n = [], 0, len(text)
    while s < n:
        e = text.find(delim, s)
        if e < 0:
            e = n
        out.append((s, e))
        s = e + 1
    return out


@functools.lru_cache(maxsize=None)
def _prose():
    """Sherlock text as one line of prose, from the first 'Sherlock Holmes'."""
    t = corpus("sherlock").replace(b"\r\n", b" ").replace(b"\n", b" ")
    return t[t.index(b"Sherlock Holmes"):]


@functools.lru_cache(maxsize=None)
def _text(seed, size=5000):
    """About `size` bytes: sherlock pieces cut into lines of 0 to 300 bytes
    with runs of empty lines, dates planted in some lines, some lines made
    to begin with "Th" or to end with "es", and a few ';' and NUL bytes (the other delimiters of these tests).  No final newline."""
    rng = np.random.default_rng(seed)
    prose, at, lines, total = _prose(), 0, [], 0
    while total < size:
        kind = rng.random()
        if kind < 0.12:
            lines += [b""] * int(rng.integers(1, 5))  # a run of empty lines
            total += 4
            continue
        n = int(rng.integers(1, 40)) if kind < 0.5 else int(rng.integers(40, 301))
        line = bytearray(prose[at:at + n])
        at += n
        if rng.random() < 0.25 and n >= 10:
            p = int(rng.integers(0, n - 9))
            line[p:p + 10] = b"%04d-%02d-%02d" % (rng.integers(1900, 2100), rng.integers(1, 13), rng.integers(1, 29))
        if rng.random() < 0.2 and n >= 2:
            line[:2] = b"Th"
        if rng.random() < 0.2 and n >= 2:
            line[-2:] = b"es"
        for b in (b";", b"\0"):
            if rng.random() < 0.2:
                line[int(rng.integers(0, n))] = b[0]
        lines.append(bytes(line))
        total += n + 1
    return b"\n".join(lines).rstrip(b"\n")


def _device(cuda, text):
    """The text on the device, one byte past a 16-byte boundary."""
    import torch
    raw = torch.zeros(len(text) + 33, dtype=torch.uint8, device=cuda)
    view = raw[1:1 + len(text)]
    if text:
        assert view.data_ptr() % 16 == 1
        view.copy_(torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()))
    return raw, view


@functools.lru_cache(maxsize=None)
def _regex(pattern):
    re = R.Regex(pattern)
    return re, OracleRegex(re)


def _expected(o, text, delim, invert=False):
    recs = split(text, delim)
    pick = [(i, r) for i, r in enumerate(recs) if bool(o.is_match(text[r[0]:r[1]])) != invert]
    return [r for _, r in pick], [i for i, _ in pick], len(recs)


def _check(re, o, cuda, text, delim=b"\n", invert=False):
    _, view = _device(cuda, text)
    info = {}
    rec, num, nrec = re.match_records(view, delim=delim, invert=invert, info=info)
    erec, enum, enrec = _expected(o, text, delim, invert)
    assert nrec == enrec
    assert info["total"] == len(erec)
    assert [tuple(x) for x in rec.cpu().tolist()] == erec
    assert num.cpu().tolist() == enum
    return info, nrec, erec


@pytest.mark.parametrize("pattern", PATTERNS)
def test_forced_units(cuda, knobs, pattern):
    """Texts of about 5000 bytes cut into 16-, 48- and 4096-byte units: some
    units own nothing, some records span many units; ending with and without
    a newline."""
    re, o = _regex(pattern)
    for seed in (1, 2):
        body = _text(seed)
        for text in (body, body + b"\n"):
            for c in (16, 48, 4096):
                knobs(records_chunk=c)
                _, nrec, erec = _check(re, o, cuda, text)
                assert R.Regex.last_records() == (-(-len(text) // c), c)
                assert R.Regex.last_records()[0] > 1
                if pattern == r"\n":
                    assert erec == []
                if pattern == r"(?s).":
                    assert erec == [r for r in split(text, b"\n") if r[1] > r[0]] and 0 < len(erec) < nrec


@pytest.mark.parametrize("delim", [b";", b"\0"])
def test_other_delimiters(cuda, knobs, delim):
    """The same texts cut at ';' and at NUL: a newline is now a record byte."""
    text = _text(1)
    assert text.count(delim) >= 3
    for pattern in PATTERNS:
        re, o = _regex(pattern)
        for c in (16, 4096):
            knobs(records_chunk=c)
            _, _, erec = _check(re, o, cuda, text, delim=delim)
            if pattern == r"\n":
                assert len(erec) > 0


@pytest.mark.parametrize("pattern", [r"\d{4}-\d{2}-\d{2}", r"^\s*$", r"x*", r"\n"])
def test_invert(cuda, knobs, pattern):
    re, o = _regex(pattern)
    text = _text(2) + b"\n"
    for c in (16, 48, 4096):
        knobs(records_chunk=c)
        a, nrec, sel = _check(re, o, cuda, text)
        b, nrec2, unsel = _check(re, o, cuda, text, invert=True)
        assert nrec == nrec2 and a["total"] + b["total"] == nrec
        assert sorted(sel + unsel) == split(text, b"\n")


def _raw_call(re, view, n, cap, delim=10, flags=0, want_numbers=True):
    """The C call into sentinel-filled buffers of cap + 3 entries; returns
    (nrecords, total, served, records, numbers) on the host."""
    import torch
    head = torch.full((3,), SENT, dtype=torch.int64, device=view.device)
    rec = torch.full((cap + 3, 2), SENT, dtype=torch.int64, device=view.device)
    num = torch.full((cap + 3,), SENT, dtype=torch.int64, device=view.device)
    rc = N.rure_amd_match_records(re._re, ctypes.c_void_p(view.data_ptr()), n, delim, flags,
                                  ctypes.c_void_p(head.data_ptr()), ctypes.c_void_p(head.data_ptr() + 8),
                                  ctypes.c_void_p(rec.data_ptr()) if cap else None,
                                  ctypes.c_void_p(num.data_ptr()) if cap and want_numbers else None, cap,
                                  ctypes.c_void_p(head.data_ptr() + 16),
                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == N.OK
    torch.cuda.synchronize()
    h = head.cpu().tolist()
    return h[0], h[1], h[2], rec.cpu().tolist(), num.cpu().tolist()


def test_capacity(cuda, knobs):
    """Capacities 0, 1 and total - 1: the counts stay exact, the first
    `capacity` entries are right and nothing at or past it is written."""
    re, o = _regex(r"Sherlock|Holmes|\d{4}-\d{2}-\d{2}")
    text = _text(1) + b"\n"
    erec, enum, enrec = _expected(o, text, b"\n")
    assert len(erec) >= 4
    _, view = _device(cuda, text)
    for c in (16, 4096):
        knobs(records_chunk=c)
        for flags, (xrec, xnum, _) in ((0, (erec, enum, enrec)), (N.RECORDS_INVERT, _expected(o, text, b"\n", True))):
            for cap in (0, 1, len(xrec) - 1):
                nrec, total, served, rec, num = _raw_call(re, view, len(text), cap, flags=flags)
                assert (nrec, total, served) == (enrec, len(xrec), 0)
                assert [tuple(x) for x in rec[:cap]] == xrec[:cap]
                assert num[:cap] == xnum[:cap]
                assert all(x == [SENT, SENT] for x in rec[cap:]) and all(x == SENT for x in num[cap:])
        # numbers may be NULL
        nrec, total, _, rec, num = _raw_call(re, view, len(text), 2, want_numbers=False)
        assert [tuple(x) for x in rec[:2]] == erec[:2] and all(x == SENT for x in num)


def test_bad_arguments(cuda):
    import torch
    re, _ = _regex(r"x*")
    _, view = _device(cuda, b"a\nb")
    out = torch.zeros((8,), dtype=torch.int64, device=cuda)
    p, q, st = ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(out.data_ptr() + 8), None
    text = ctypes.c_void_p(view.data_ptr())
    f = N.rure_amd_match_records
    assert f(None, text, 3, 10, 0, p, q, None, None, 0, None, st) == N.ERR_ARG
    assert f(re._re, None, 3, 10, 0, p, q, None, None, 0, None, st) == N.ERR_ARG
    assert f(re._re, text, 3, 10, 0, None, q, None, None, 0, None, st) == N.ERR_ARG
    assert f(re._re, text, 3, 10, 0, p, None, None, None, 0, None, st) == N.ERR_ARG
    assert f(re._re, text, 3, 10, 0, p, q, None, None, 4, None, st) == N.ERR_ARG
    assert f(re._re, text, 3, 10, 2, p, q, None, None, 0, None, st) == N.ERR_ARG


def test_pike_unicode_word_boundary(cuda, knobs):
    """A Unicode \\b: the DFA quits on the records that hold a non-ASCII
    letter before any match, and the Pike VM answers exactly those."""
    re, o = _regex(r"\bthe\b")
    lines = _text(2).split(b"\n")
    for i in range(0, len(lines), 3):
        if len(lines[i]) > 4:
            lines[i] = lines[i][:2] + "thé éthe the".encode() + lines[i][2:]
    text = b"\n".join(lines)
    for c in (16, 48, 4096):
        knobs(records_chunk=c)
        info, nrec, erec = _check(re, o, cuda, text)
        assert 0 < info["pike_served"] < nrec
        assert 0 < len(erec) < nrec


def test_pike_only(cuda, knobs):
    """A regex without an eager DFA: every record goes to the Pike VM."""
    re, o = _regex(r"(?:a|b)*a(?:a|b){20}")
    assert not re.uses_dfa()
    rng = np.random.default_rng(7)
    text = bytes(rng.choice(np.frombuffer(b"aabb\n", dtype=np.uint8), size=3000, p=[0.24, 0.24, 0.24, 0.24, 0.04]))
    for c in (48, 4096):
        knobs(records_chunk=c)
        info, nrec, erec = _check(re, o, cuda, text)
        assert info["pike_served"] == nrec
        assert 0 < len(erec) < nrec


def test_cannot_quit_serves_nothing(cuda, knobs):
    re, o = _regex(r"(?-u)\bthe\b")
    knobs(records_chunk=48)
    info, _, _ = _check(re, o, cuda, _text(1))
    assert info["pike_served"] == 0


@functools.lru_cache(maxsize=None)
def _mib():
    """1 MiB of sherlock prose in lines of 20 to 120 bytes."""
    rng = np.random.default_rng(0xC4)
    prose, at, parts, total = _prose(), 0, [], 0
    while total < MIB:
        n = int(rng.integers(20, 121))
        if at + n > len(prose):
            at = 0
        parts.append(prose[at:at + n])
        at += n
        total += n + 1
    return b"\n".join(parts)[:MIB]


@pytest.mark.parametrize("pattern", [r"\d{4}-\d{2}-\d{2}", r"Sherlock|Holmes", r"es$"])
def test_production_rule(cuda, pattern):
    """No knob, 1 MiB of lines: the long scan's unit size, the engine path
    diagnostic untouched, no scratch left live."""
    import torch
    re, o = _regex(pattern)
    text = _mib()
    small = torch.from_numpy(np.frombuffer(b"a 2024-01-02 b", dtype=np.uint8).copy()).to(cuda)
    re.is_match_batch(small, stride=14, length=14, count=1)
    before = N.last_path()
    _check(re, o, cuda, text)
    units, chunk = R.Regex.last_records()
    assert chunk >= 16 << 10 and chunk % 128 == 0 and (chunk // 128) % 2 == 1  # the long scan's rule
    assert units == -(-MIB // chunk) and units > 1
    assert N.last_path() == before
    torch.cuda.synchronize()
    assert R.scratch_stats()["live"] == 0


def test_edges(cuda, knobs):
    re, o = _regex(r"x*")
    none, _ = _regex(r"y")
    for c in (16, 4096):
        knobs(records_chunk=c)
        for text in (b"", b"a", b"\n", b"\n\n\n", b"\n" * 100, b"a\nb", b"a\nb\n", b"y"):
            info, nrec, erec = _check(re, o, cuda, text)
            assert nrec == len(text.split(b"\n")) - (1 if text.endswith(b"\n") or not text else 0)
            assert len(erec) == nrec
            _check(none, OracleRegex(none), cuda, text)
    _check(re, o, cuda, b"")
    assert R.Regex.last_records() == (0, 0)
