"""The tile kernel's skip rule on the device (dfa_fwd_tile_kernel<.., SKIP>):
for each eligible pattern, find / is_match / shortest_match over batches above
the byte table's threshold (131,072 haystacks) are bit-equal to the oracle and
to the same call with the rule off (tileskip=0), on the TILE1 path.

The batch is a block of haystacks repeated (tile_skip_cases.block): whole
64-haystack wave groups, one per adversarial row (near-misses, matches
straddling the tile cut, anchor-byte floods, a match on a tile's last byte)
among match-free ASCII filler, so that the wave skips and the row's answer
comes from the skip rule alone; groups of their own for the rows with
non-ASCII bytes; random printable text and unicode_mix text.  The host
simulation must find at least half of the block's wave-tiles clean, so the
clean branch is what is compared.  The oracle answers the block once; the
device answers every copy.  (The kernel uses the rule for the patterns of
tile_skip_cases.USED; for the other eligible ones, whose anchors are too
frequent, it must leave everything as it is.)"""
import numpy as np
import pytest

import regex_amd as R
from regex_amd import Path
from regex_amd import _native as N
from oracle_py import OracleRegex
from regex_amd.workloads import date_haystacks_host
from tile_skip_cases import ELIGIBLE, USED, block, clean_share

pytestmark = pytest.mark.gpu

N_BASE = 140_000   # above the byte table's threshold of 131,072 haystacks
_blocks = {}


def _block(pat, L):
    """(block bytes [k, stride], oracle find / is_match / shortest of its rows,
    the share of its wave-tiles the skip rule finds clean)."""
    key = (pat, L)
    if key not in _blocks:
        stride = (L + 15) & ~15
        rows = block(pat, L, seed=L)
        k = len(rows)
        assert k % 64 == 0
        blk = np.full((k, stride), ord("-"), dtype=np.uint8)   # anchor bytes in the stride padding
        blk[:, :L] = rows
        re = R.Regex(pat)
        o = OracleRegex(re)
        flat = np.ascontiguousarray(blk).reshape(-1)
        f, _ = o.find_batch(flat, stride, L, k, nthreads=8)
        i = o.is_match_batch(flat, stride, L, k, nthreads=8)
        s = o.shortest_batch(flat, stride, L, k, nthreads=8)
        _blocks[key] = (blk, f.astype(np.int64), i.astype(bool), s.astype(np.int64), clean_share(re, rows))
    return _blocks[key]


def _tiled(a, n):
    reps = (n + len(a) - 1) // len(a)
    return np.concatenate([a] * reps)[:n]


def _run(re, dev, stride, L, n):
    f = re.find_batch(dev, stride=stride, length=L, count=n).cpu().numpy()
    p = [N.last_path()]
    i = re.is_match_batch(dev, stride=stride, length=L, count=n).cpu().numpy()
    p.append(N.last_path())
    s = re.shortest_match_batch(dev, stride=stride, length=L, count=n).cpu().numpy()
    p.append(N.last_path())
    return f, i.astype(bool), s.astype(np.int64), p


@pytest.mark.parametrize("n", [N_BASE, N_BASE + 37])
@pytest.mark.parametrize("L", [128, 144, 261])
@pytest.mark.parametrize("pat", sorted(ELIGIBLE))
def test_skip_parity(cuda, knobs, pat, L, n):
    import torch
    blk, ef, ei, es, share = _block(pat, L)
    assert share >= 0.5, share   # the waves skip: the clean branch is what is compared
    stride = blk.shape[1]
    re = R.Regex(pat)
    info = re.tile_skip_info()
    assert info["eligible"] == 1 and info["used"] == (1 if pat in USED else 0)
    dev = torch.from_numpy(_tiled(blk, n).reshape(-1)).to(cuda)
    knobs()
    f, i, s, p = _run(re, dev, stride, L, n)
    assert p == [Path.TILE1] * 3, p
    knobs(tileskip=0)
    f0, i0, s0, p0 = _run(re, dev, stride, L, n)
    knobs()
    assert p0 == [Path.TILE1] * 3, p0
    for got, off, exp, what in ((f, f0, ef, "find"), (i, i0, ei, "is_match"), (s, s0, es, "shortest_match")):
        exp = _tiled(exp, n)
        bad = np.nonzero((got != exp).reshape(n, -1).any(axis=1))[0]
        assert bad.size == 0, (what, pat, L, int(bad[0]), got[bad[0]].tolist(), exp[bad[0]].tolist(),
                               blk[bad[0] % len(blk)].tobytes())
        assert np.array_equal(got, off), what
    assert (f[:, 0] >= 0).sum() > 0


def test_ineligible_control(cuda, knobs):
    """A regex the rule does not apply to: nothing changes for it."""
    import torch
    pat, L = r"\d{2,5}-x", 144
    re = R.Regex(pat)
    assert re.tile_skip_info()["eligible"] == 0
    buf, _ = date_haystacks_host(N_BASE, L, seed=0x7C01, frac=0.3)
    buf[5 * L + 20:5 * L + 26] = np.frombuffer(b"1234-x", dtype=np.uint8)
    o = OracleRegex(re)
    exp, _ = o.find_batch(buf, L, L, N_BASE, nthreads=8)
    dev = torch.from_numpy(buf).to(cuda)
    knobs()
    got = re.find_batch(dev, stride=L, length=L, count=N_BASE).cpu().numpy()
    assert N.last_path() == Path.TILE1
    knobs(tileskip=0)
    off = re.find_batch(dev, stride=L, length=L, count=N_BASE).cpu().numpy()
    knobs()
    assert np.array_equal(got, exp.astype(np.int64))
    assert np.array_equal(got, off)
    assert got[5, 0] >= 0
