"""Host checks of the tile kernel's skip rule (kernels/tile_skip_device.hpp,
host/tile_skip.cpp): which regexes are eligible, and that a lane walked under
the rule (rure_amd_tile_skip_simulate, the kernel's own rule compiled for the
host) is in the exact walk's state at every tile boundary."""
import numpy as np
import pytest

import regex_amd as R
from regex_amd.workloads import date_haystacks_host
from tile_skip_cases import ELIGIBLE, INELIGIBLE, USED, block, clean_share, rows

DATE = r"\d{4}-\d{2}-\d{2}"


@pytest.mark.parametrize("pat", sorted(ELIGIBLE))
def test_eligible(pat):
    info = R.Regex(pat).tile_skip_info()
    assert info["eligible"] == 1, info
    assert info["m"] == ELIGIBLE[pat][2]
    assert 0 <= info["anchor_a"] <= info["anchor_b"] < info["m"]
    if pat == DATE:
        assert (info["anchor_a"], info["anchor_b"]) == (4, 7)
    assert info["used"] == (1 if pat in USED else 0)


@pytest.mark.parametrize("pat", INELIGIBLE)
def test_ineligible(pat):
    re = R.Regex(pat)
    info = re.tile_skip_info()
    assert info is not None and info["eligible"] == 0, info
    assert re.tile_skip_simulate(b"x" * 256) is None


@pytest.mark.parametrize("pat", sorted(ELIGIBLE))
def test_simulation_is_exact(pat):
    re = R.Regex(pat)
    skipped = 0
    for L in (256, 384, 261):
        for i, hay in enumerate(rows(pat, L)):
            ss, se, d = re.tile_skip_simulate(hay)
            assert len(ss) == L // 128
            assert np.array_equal(ss, se), (pat, L, i, hay, ss.tolist(), se.tolist(), d.tolist())
            skipped += int((d == 0).sum())
    assert skipped > 0


def test_simulation_random_text():
    """Random printable text with planted dates, tile by tile."""
    re = R.Regex(DATE)
    buf, _ = date_haystacks_host(512, 1024, seed=0x51C1, frac=0.5)
    for h in range(512):
        ss, se, d = re.tile_skip_simulate(buf[h * 1024:(h + 1) * 1024].tobytes())
        assert np.array_equal(ss, se), h


def test_the_skip_fires():
    """1 % of the haystacks carry one date, and a date dirties at most 3 of a
    haystack's 32 tiles: at least 99 % of the lane-tiles are clean."""
    re = R.Regex(DATE)
    n, L = 4096, 4096
    buf, planted = date_haystacks_host(n, L, seed=0x5EED0002, frac=0.01)
    dirty = 0
    for h in range(n):
        ss, se, d = re.tile_skip_simulate(buf[h * L:(h + 1) * L].tobytes())
        assert np.array_equal(ss, se), h
        dirty += int(d.sum())
    assert dirty <= 0.01 * n * (L // 128), dirty
    assert dirty >= len(planted)


def test_dirt_does_not_stick():
    """A lone 0xFF dirties its own tile and the one after, no more."""
    re = R.Regex(DATE)
    hay = bytearray(b"x" * 1024)
    hay[77] = 0xFF
    ss, se, d = re.tile_skip_simulate(bytes(hay))
    assert d.tolist() == [1, 1, 0, 0, 0, 0, 0, 0]
    assert np.array_equal(ss, se)
    hay[640:650] = b"1234-56-78"   # and a later match is still found: its tile is dirty again
    ss, se, d = re.tile_skip_simulate(bytes(hay))
    assert d.tolist()[:6] == [1, 1, 0, 0, 0, 1]
    assert np.array_equal(ss, se)


@pytest.mark.parametrize("pat", sorted(ELIGIBLE))
def test_simulation_random_mixes(pat):
    """Matches, near-misses, Unicode digits and stray bytes at random offsets
    of 1 KiB haystacks: clean and dirty tiles alternate many ways."""
    match, miss, m = ELIGIBLE[pat]
    d0 = next(i for i, c in enumerate(match) if chr(c).isdigit())
    near = bytearray(match)
    near[m - 1:m] = miss
    items = [match, bytes(near), match[:d0] + "\u0663".encode() + match[d0 + 1:], b"\xff", "\u00e9".encode(),
             match[:m // 2]]
    rng = np.random.default_rng(len(pat))
    re = R.Regex(pat)
    cleans = 0
    for h in range(300):
        hay = bytearray(bytes(rng.choice(np.frombuffer(b"abcxyz 0123456789ABC_.", dtype=np.uint8), size=1024)))
        for _ in range(int(rng.integers(0, 5))):
            it = items[int(rng.integers(len(items)))]
            at = int(rng.integers(0, 1024 - len(it)))
            if rng.integers(0, 2):   # at a tile cut
                at = max(0, min(1024 - len(it), 128 * int(rng.integers(1, 8)) - int(rng.integers(0, len(it) + 1))))
            hay[at:at + len(it)] = it
        ss, se, d = re.tile_skip_simulate(bytes(hay))
        assert np.array_equal(ss, se), (pat, h, bytes(hay), ss.tolist(), se.tolist(), d.tolist())
        cleans += int((d == 0).sum())
    assert cleans > 300


@pytest.mark.parametrize("pat", sorted(ELIGIBLE))
def test_gpu_block_is_not_vacuous(pat):
    """The GPU parity test's batch: most of its wave-tiles are clean."""
    re = R.Regex(pat)
    for L in (128, 144, 261):
        assert clean_share(re, block(pat, L, seed=L)) >= 0.5
