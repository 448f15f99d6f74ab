"""The chunked RegexSet scan on the GPU (regex_amd/csrc/kernels/set_long.hip):
few long fixed-stride haystacks cut into units whose patterns are ORed into
the mask word, bit-exact against the oracle's many_matches_at; forced onto a
few KiB with many cuts (knobs set_long=2, set_chunk), by the production rule
on 1 MiB, through the host entry points and the words form, and the sets and
batches that keep one lane per haystack.  The sets are set_long_data.CASES:
C4_PATTERNS itself has Unicode word boundaries (a DFA that can quit), so it is
among those that keep their lanes; C4_ASCII_WB is the large set that chunks."""
import ctypes
import functools

import numpy as np
import pytest

import regex_amd as R
from oracle_py import OracleRegex
from regex_amd import _native as N
from regex_amd.workloads import log_lines_host
from set_long_data import CASES, MIXED
from bigset_data import SETS

pytestmark = pytest.mark.gpu

L, STRIDE = 5003, 5021  # about 5000 bytes; neither a multiple of 16
MIB = 1 << 20


@functools.lru_cache(maxsize=None)
def _log():
    """1 MiB (and 16 bytes) of log text, generated once."""
    buf, _ = log_lines_host((MIB + 16) // 100 + 1, seed=0x5E7, lo=100, hi=100)
    return buf[:MIB + 16].copy()


@functools.lru_cache(maxsize=None)
def _set(name):
    rs = R.RegexSet(CASES[name][0])
    return rs, OracleRegex(rs)


def _mask(o, t, start=0):
    return sum(1 << j for j in o.matches(t, start)) if start <= len(t) else 0


def _u64(x):
    return int(x) & ((1 << 64) - 1)


@pytest.mark.parametrize("name", sorted(CASES))
def test_forced_chunks(cuda, knobs, name):
    """1 and 3 haystacks of 5003 bytes cut into 16-, 48- and 4096-byte units,
    from five starts; the sets without the automaton answer on their lanes."""
    import torch
    rs, o = _set(name)
    chunked = CASES[name][1]
    host = _log()[:3 * STRIDE + 16].copy()
    dev = torch.from_numpy(host).to(cuda)
    for c in (16, 48, 4096):
        knobs(set_long=2, set_chunk=c)
        for count in (1, 3):
            for start in (0, 41, c, L, L + 1):  # (c: a start on what is a cut from 0)
                got = rs.matches_batch(dev, stride=STRIDE, length=L, count=count, start=start).cpu().numpy()
                units = R.RegexSet.last_long_units()
                for h in range(count):
                    exp = _mask(o, bytes(host[h * STRIDE:h * STRIDE + L]), start)
                    assert _u64(got[h]) == exp, (name, c, count, start, h)
                if not chunked:
                    assert units == (0, 0, 0)
                    continue
                span = max(L - start, 0)
                nk = 1 if span <= c else -(-span // c)
                assert units == (count * nk, count, c), (name, c, count, start)
                assert start > 41 or nk > 1
                assert N.last_path() == N.Path.LONG_SCAN


@pytest.mark.parametrize("name", ["c4", "c4_ascii_wb", "mixed"])
def test_production_rule(cuda, name):
    """No knobs, one haystack of 1 MiB: the dispatch rule takes the chunked
    scan by itself (C4_PATTERNS, which can quit, keeps its lane), and the host
    entry points on the same megabyte agree."""
    import torch
    rs, o = _set(name)
    host = _log()
    t = bytes(host[:MIB])
    exp = _mask(o, t)
    got = rs.matches_batch(torch.from_numpy(host).to(cuda), stride=MIB, length=MIB, count=1).cpu().numpy()
    units, hays, chunk = R.RegexSet.last_long_units()
    assert _u64(got[0]) == exp
    if CASES[name][1]:
        assert units > 1 and hays == 1 and chunk >= 16 << 10 and units == -(-MIB // chunk)
        assert N.last_path() == N.Path.LONG_SCAN
    else:
        assert (units, hays, chunk) == (0, 0, 0)
    assert sum(1 << j for j in rs.matches(t)) == exp
    assert (R.RegexSet.last_long_units()[0] > 1) == CASES[name][1]
    assert rs.is_match(t) == bool(exp)
    assert (R.RegexSet.last_long_units()[0] > 1) == CASES[name][1]


def test_unchanged_paths(cuda, knobs):
    """What keeps one lane per haystack still answers, and reports no units:
    a set with a Unicode `\\b` member (over text with a few non-ASCII bytes:
    the quit fallback), a set anchored at the start, set_long=0, an offset
    batch."""
    import torch
    host = _log()
    nonascii = host.copy()
    for p in (1000, MIB // 2, MIB - 7):
        nonascii[p:p + 2] = np.frombuffer("é".encode(), dtype=np.uint8)
    offs = torch.tensor([0, MIB], dtype=torch.int64, device=cuda)
    for pats, buf, kn, kw in (
            ([r"\bkernel\b", r"ERROR", r"\bnil$"], nonascii, {}, dict(stride=MIB, length=MIB, count=1)),
            ([r"^GET ", r"^POST ", r"^\d+"], host, {}, dict(stride=MIB, length=MIB, count=1)),
            (MIXED, host, {"set_long": 0}, dict(stride=MIB, length=MIB, count=1)),
            (MIXED, host, {}, dict(offsets=offs))):
        rs = R.RegexSet(pats)
        knobs(**kn)
        got = rs.matches_batch(torch.from_numpy(buf).to(cuda), **kw).cpu().numpy()
        assert _u64(got[0]) == _mask(OracleRegex(rs), bytes(buf[:MIB])), pats
        assert R.RegexSet.last_long_units() == (0, 0, 0), pats


def _group_oracle(pats, t):
    """The patterns of one 64-pattern group matching t, by the oracle over
    the group's set; by the oracle pattern by pattern where the group has no
    DFA (a pattern's membership does not depend on the rest of the set,
    test_set_groups.py; that group's set oracle gives up its lazy DFA and
    spends half a minute in its Pike VM over a megabyte)."""
    rs = R.RegexSet(pats)
    if rs.uses_dfa():
        return OracleRegex(rs).matches(t)
    return [j for j, p in enumerate(pats) if OracleRegex(R.Regex(p)).is_match(t)]


def test_words_form(cuda):
    """130 patterns through rure_amd_set_matches_batch_words on one 1 MiB
    haystack: every group's word equals the oracle's, each group having taken
    its own decision; unused bits and words are zero."""
    import torch
    k = 130
    rs = R.RegexSet(SETS[k])
    host = _log()
    t = bytes(host[:MIB])
    dev = torch.from_numpy(host).to(cuda)
    out = torch.full((1, 4), -5, dtype=torch.int64, device=cuda)
    b = R._batch(dev, stride=MIB, length=MIB, count=1)
    assert N.rure_amd_set_matches_batch_words(rs._set, ctypes.byref(b), ctypes.c_void_p(out.data_ptr()), 4,
                                              R._stream_ptr(None)) == N.OK
    got = out.cpu().numpy()[0].view(np.uint64)
    for g in range(3):
        assert int(got[g]) == sum(1 << j for j in _group_oracle(SETS[k][64 * g:64 * g + 64], t)), g
    assert int(got[2]) >> (k - 128) == 0 and int(got[3]) == 0
    # the last group (two patterns, a DFA that cannot quit) was chunked
    assert R.RegexSet.last_long_units()[0] > 1


@pytest.mark.parametrize("name", ["mixed", "literals"])
def test_buffer_contract(cuda, knobs, name):
    """The last haystack ends in the last 16-byte block of its tensor, and
    the bytes between and after the haystacks hold text that would match:
    the masks are those of the haystacks alone."""
    import torch
    rs, o = _set(name)
    count, base = 3, 5  # (an odd base: no haystack starts on a 16-byte boundary)
    total = (base + (count - 1) * STRIDE + L + 15) & ~15
    assert 0 < total - (base + (count - 1) * STRIDE + L) < 16
    filler = np.frombuffer((b"abc\n12 foo z ERROR status=404 oom kernel x" * (total // 40 + 1))[:total], dtype=np.uint8)
    host = filler.copy()
    text = _log()[100000:100000 + count * L]
    for h in range(count):
        host[base + h * STRIDE:base + h * STRIDE + L] = text[h * L:(h + 1) * L]
    dev = torch.from_numpy(host).to(cuda)
    assert dev.numel() == total
    for c in (16, 4096):
        knobs(set_long=2, set_chunk=c)
        got = rs.matches_batch(dev[base:], stride=STRIDE, length=L, count=count).cpu().numpy()
        assert R.RegexSet.last_long_units()[0] > count
        for h in range(count):
            assert _u64(got[h]) == _mask(o, bytes(text[h * L:(h + 1) * L])), (name, c, h)
