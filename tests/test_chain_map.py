"""The byte map rure_amd_replace_all_chain composes on the host
(regex_amd/csrc/host/chain_map.hpp through rure_amd_chain_map_export, no
GPU) against a plain-Python restatement: each byte's image is the byte with
every step's (byte set, replacement) applied to it in turn (tests/
chain_ref.py).  For every mappable chain: the images in the pool, their
lengths after every step, the changed-byte indices the count kernel's
histogram is built on; and the edges of "mappable": 255 / 256 changed byte
values (index 255 is legal, 256 changed bytes would give byte 0xFF the
"unchanged" mark 0xFF), a pool of 4096 / 4160 bytes, an image of 64 / 66."""
import ctypes

import numpy as np
import pytest

import regex_amd as R
from regex_amd import _native as N
from chain_ref import CHAINS, LIMITS, apply_chain

ALL_CHAINS = {"chain%d" % i: c for i, c in enumerate(CHAINS)}
ALL_CHAINS.update({k: v[0] for k, v in LIMITS.items()})
MAPPABLE = sorted(k for k in ALL_CHAINS if k not in LIMITS or LIMITS[k][1])


def export(steps):
    """(mappable, nact, pool_len, flen, soff, aidx, pool, dlen)"""
    n = len(steps)
    regs = [R.Regex(p) for p, _, _ in steps]
    res = (ctypes.c_void_p * n)(*[r._re for r in regs])
    bufs = [ctypes.create_string_buffer(rep, len(rep)) for _, _, rep in steps]
    reps = (ctypes.c_void_p * n)(*[ctypes.addressof(b) for b in bufs])
    lens = (ctypes.c_size_t * n)(*[len(rep) for _, _, rep in steps])
    flen, aidx = np.full(256, 0xEE, np.uint8), np.full(256, 0xEE, np.uint8)
    soff, pool = np.full(256, 0xEEEE, np.uint16), np.full(4096, 0xEE, np.uint8)
    dlen = np.full((n, 256), 0xEEEEEEEE, np.uint32)
    nact, plen = ctypes.c_uint32(12345), ctypes.c_size_t(12345)
    rc = N.rure_amd_chain_map_export(res, reps, lens, n, flen.ctypes.data, soff.ctypes.data, aidx.ctypes.data,
                                     ctypes.addressof(nact), pool.ctypes.data, pool.size, ctypes.addressof(plen),
                                     dlen.ctypes.data)
    assert rc in (0, 1), rc
    return rc == 1, nact.value, plen.value, flen, soff, aidx, pool, dlen


def images(steps):
    """per byte value: its image after no step, step 0, step 1, ..."""
    return [apply_chain(steps, bytes((x,))) for x in range(256)]


def test_byte_sets_are_the_regexes_classes():
    """The literal byte sets of chain_ref are what the product reads off each
    pattern (the reference rule itself never asks the product)."""
    seen = {}
    for steps in ALL_CHAINS.values():
        for pat, cset, _ in steps:
            assert seen.setdefault(pat, cset) == cset, pat
    for pat, cset in seen.items():
        cls = np.zeros(256, np.uint8)
        re = R.Regex(pat)
        assert N.rure_amd_class_one_export(re._re, cls.ctypes.data) == 1, pat
        assert frozenset(np.flatnonzero(cls).tolist()) == cset, pat


@pytest.mark.parametrize("name", MAPPABLE)
def test_map_is_the_composition(name):
    steps = ALL_CHAINS[name]
    ok, nact, plen, flen, soff, aidx, pool, dlen = export(steps)
    assert ok
    img = images(steps)
    changed = [x for x in range(256) if img[x][-1] != bytes((x,))]
    assert nact == len(changed)
    assert plen == sum(len(img[x][-1]) for x in range(256)) <= 4096
    for x in range(256):
        assert bytes(pool[int(soff[x]):int(soff[x]) + int(flen[x])]) == img[x][-1], (name, x)
        assert int(soff[x]) + int(flen[x]) <= plen
        for i in range(len(steps)):
            assert int(dlen[i][x]) == len(img[x][i + 1]) - 1, (name, i, x)
    # the changed bytes are numbered 0 .. nact - 1 in byte order, every other byte is 0xFF
    assert [int(aidx[x]) for x in changed] == list(range(nact))
    assert all(int(aidx[x]) == 0xFF for x in range(256) if x not in set(changed))
    assert all(int(aidx[x]) != 0xFF for x in changed)


@pytest.mark.parametrize("name", sorted(LIMITS))
def test_mappable_edges(name):
    """nact 255 is mappable and 256 is not; a pool of 4096 is and 4160 is not;
    an image of 64 bytes is and 66 is not.  The expected figures are
    chain_ref's literals, checked against the restatement where an image can
    be composed at all."""
    steps, mappable, want_nact, want_pool = LIMITS[name]
    ok, nact, plen = export(steps)[:3]
    img = images(steps)
    longest = max(len(img[x][-1]) for x in range(256))
    if want_pool is None:
        assert longest > 64 and (ok, nact, plen) == (False, 0, 0)
        return
    assert longest <= 64
    assert want_nact == sum(img[x][-1] != bytes((x,)) for x in range(256))
    assert want_pool == sum(len(img[x][-1]) for x in range(256))
    assert (ok, nact, plen) == (mappable, want_nact, want_pool)
    assert mappable == (want_nact <= 255 and want_pool <= 4096)


def test_the_edges_are_the_edges():
    assert [LIMITS[k][2] for k in ("c255", "all256")] == [255, 256]
    assert [LIMITS[k][3] for k in ("pool4096", "pool4160")] == [4096, 4160]
    assert [max(len(i[-1]) for i in images(LIMITS[k][0])) for k in ("img64", "img66")] == [64, 66]


def test_export_rejects():
    x = R.Regex(r"x")
    res = (ctypes.c_void_p * 1)(x._re)
    buf = ctypes.create_string_buffer(b"y" * 65, 65)
    reps = (ctypes.c_void_p * 1)(ctypes.addressof(buf))

    def rc(res_, rep_len, n=1):
        lens = (ctypes.c_size_t * 1)(rep_len)
        return N.rure_amd_chain_map_export(res_, reps, lens, n, None, None, None, None, None, 0, None, None)

    assert rc(res, 1) == 1 and rc(res, 64) == 1
    assert rc(res, 0) == N.ERR_ARG and rc(res, 65) == N.ERR_ARG
    assert rc(res, 1, n=0) == N.ERR_ARG and rc(None, 1) == N.ERR_ARG
    ab = R.Regex(r"ab")  # matches are not single bytes of a class
    assert rc((ctypes.c_void_p * 1)(ab._re), 1) == N.ERR_ARG
