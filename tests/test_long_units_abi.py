"""rure_amd_last_long_units (the deferred long scan's diagnostic): declared in
include/rure_amd.h, exported, bound in _native, and 0 / 0 / 0 in a process
that has made no such call (no device needed)."""
import ctypes
import os
import re

import regex_amd as R
from regex_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_declared_and_exported():
    src = open(os.path.join(ROOT, "include", "rure_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"uint64_t\s+rure_amd_last_long_units\s*\(\s*uint64_t\s*\*\s*haystacks\s*,\s*uint64_t\s*\*\s*chunk\s*\)\s*;",
                     src)
    assert hasattr(N.lib, "rure_amd_last_long_units")


def test_zero_without_a_call():
    n, c = ctypes.c_uint64(5), ctypes.c_uint64(5)
    assert N.rure_amd_last_long_units(ctypes.byref(n), ctypes.byref(c)) == 0
    assert (n.value, c.value) == (0, 0)
    assert N.rure_amd_last_long_units(None, None) == 0
    assert N.last_long_units() == (0, 0, 0)


def test_knobs_accepted():
    with R.debug(long_ragged=2, long_chunk=16, long_list=2) as d:
        assert d.spec == "long_ragged=2,long_chunk=16,long_list=2"
