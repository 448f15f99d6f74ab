"""Host side of the ragged find_iter geometry (offset batches cut into
units by each haystack's own length): the rure_amd_last_iter_units diagnostic
and the iter_ragged knob.  The GPU side is tests/test_gpu_iter_ragged.py."""
import ctypes

import numpy as np
import pytest

import regex_amd as R
from regex_amd import Path
from regex_amd import _native as N
from golden_data import corpus
from oracle_py import OracleRegex


def test_last_iter_units_exported():
    n = ctypes.c_uint64(12345)
    units = N.rure_amd_last_iter_units(ctypes.byref(n))
    assert N.rure_amd_last_iter_units(None) == units  # the haystack count is optional
    if N.last_path() == Path.NONE:  # nothing launched in this process yet
        assert (units, n.value) == (0, 0)
        assert N.last_iter_units() == (0, 0)
    else:  # at least one unit per haystack
        assert units >= n.value
        assert N.last_iter_units() == (units, n.value)


def test_iter_ragged_knob_accepted():
    try:
        assert N.rure_amd_debug_set(b"iter_ragged=2,iter_chunk=16") == N.OK
        with R.debug(iter_ragged=0) as d:
            assert d.spec == "iter_ragged=0"
    finally:
        R._debug_set(None)


# A DfaSuffix regex is iterated by the reference's suffix walk, which is not
# the forward DFA's search in general.  rure_amd_suffix_forward
# tells when it is: no match holds the longest common suffix but at its end.
SUFFIX_FORWARD = [
    (r"[A-Z][a-z]+ Holmes", 1),
    (r"[a-z]+ Holmes", 1),
    (r"[a-z ]+ Holmes", 1),      # the class has no `H`: ` Holmes` only at the end
    (r"[a-c]+xyz", 1),
    (r"xa*ingb*ing|a+ing", 0),   # (0, 10) of `xaaingbing` holds an earlier `ing`; the walk gives (1, 6)
    (r"[a-z]+ing", 0),           # `singing`
    (r"\w+\s+Holmes", 0),        # `\w+` may read `Holmes`
    (r"(?-u)\b\w+ Holmes", 0),   # look-around
    (r"[A-Z][a-z]+ (Holmes|Watson)", 0),  # not DfaSuffix at all
]


@pytest.mark.parametrize("pat,want", SUFFIX_FORWARD)
def test_suffix_forward_analysis(pat, want):
    re = R.Regex(pat)
    assert N.rure_amd_suffix_forward(re._re) == want
    if want:
        assert re.match_info()["match_type"] == "DfaSuffix"


@pytest.mark.parametrize("pat,alphabet", [(r"[A-Z][a-z]+ Holmes", None), (r"[a-z]+ Holmes", None),
                                          (r"[a-c]+xyz", (b"a", b"b", b"c", b"xyz", b"xy", b" ", b"z")),
                                          (r"[a-z ]+ Holmes", (b"a", b" ", b" Holmes", b"Hol", b"mes", b"b"))])
def test_suffix_forward_agrees_with_the_walk(pat, alphabet):
    """Where the analysis says so, the oracle's suffix walk and its forward
    DFA arm iterate alike (and on the counter-example they do not)."""
    re = R.Regex(pat)
    assert N.rure_amd_suffix_forward(re._re) == 1
    walk, fwd = OracleRegex(re), OracleRegex(re, dispatch=False)
    rng = np.random.default_rng(len(pat))
    text = corpus("sherlock")[:300000]
    some = 0
    for _ in range(200):
        if alphabet:
            t = b"".join(alphabet[int(i)] for i in rng.integers(0, len(alphabet), size=int(rng.integers(0, 60))))
        else:
            a = int(rng.integers(0, len(text) - 3000))
            t = text[a:a + int(rng.integers(0, 3000))]
        m = walk.find_iter(t)
        assert m == fwd.find_iter(t), (pat, t)
        some += len(m)
    assert some >= 20
    q = R.Regex(r"xa*ingb*ing|a+ing")
    assert OracleRegex(q).find_iter(b"xaaingbing") != OracleRegex(q, dispatch=False).find_iter(b"xaaingbing")
