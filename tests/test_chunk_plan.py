"""The unit-size rule of the chunked scans (regex_amd/csrc/host/chunk_plan.hpp)
from a plain C++ program: tests/ctest/chunk_plan_ctest.cpp compiled with g++
(no HIP), one unit size per input row.

The expected values are the formulas the dispatch held before the header
existed, one per former site and named after the function it stood in,
written out here in 64-bit unsigned arithmetic: the header must give what
each of them gave, the round-down division of ragged_plan and the fixed 1024
lanes per CU of the suffix paths included."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = (1 << 64) - 1
KiB, MiB = 1 << 10, 1 << 20


def odd_lines(b):
    lines = ((b + 127) & M) // 128
    if lines & 1 == 0:
        lines += 1
    return (lines * 128) & M


def _share(span, count, lanes, floor):
    per_h = ((lanes + count - 1) & M) // count
    return odd_lines(max(floor, ((span + per_h - 1) & M) // per_h))


def long_batch_long(cus, count, span, per_cu=1024):
    return _share(span, count, cus * per_cu, 16 << 10)


def long_batch_split(cus, count, span):
    c = _share(span, count, cus * 64, 128)
    return 0 if c >= span else c  # `if (c >= span) return false`


def suffix_long_ok(cus, count, span, forced=False):
    return _share(span, count, cus * 1024, 128 if forced else 16 << 10)


run_find_iter_suffix = suffix_long_ok  # the same lines, a second time


def run_find_iter_fixed(cus, count, span, per_cu=1024):
    return _share(span, count, cus * per_cu, 4096)


def ragged_plan(cus, total, per_cu=1024):
    return odd_lines(max(4096, total // (cus * per_cu)))


def find_iter_span_multi(cus, span, per_cu=1024):
    lanes = cus * per_cu
    return odd_lines(max(4096, ((span + lanes - 1) & M) // lanes))


def long_geometry_kernel(lanes, total, floor, rnd):
    c = max(((total + lanes - 1) & M) // lanes, floor)
    return odd_lines(c) if rnd else c


def cases():
    """(input row of the program, expected unit size)"""
    rows = []

    def add(rule, cus, count, nbytes, want, per_cu=1024, floor=0, odd=1):
        rows.append(("%s %d %d %d %d %d %d" % (rule, cus, count, nbytes, per_cu, floor, odd), want))

    spans = (0, 1, 511, 512, 4 * KiB, 256 * KiB, 64 * MiB, 1 << 63)
    for cus in (1, 256, 304):
        for count in (1, 3, 64, 1024):
            for span in spans:
                add("long", cus, count, span, long_batch_long(cus, count, span))
                add("long", cus, count, span, long_batch_long(cus, count, span, 64), per_cu=64)
                add("split", cus, count, span, long_batch_split(cus, count, span))
                add("suffix", cus, count, span, suffix_long_ok(cus, count, span))
                add("suffix_forced", cus, count, span, run_find_iter_suffix(cus, count, span, True))
                add("iter", cus, count, span, run_find_iter_fixed(cus, count, span))
                add("iter", cus, count, span, run_find_iter_fixed(cus, count, span, 2048), per_cu=2048)
        for total in spans + (262144 * 4224 + 1, cus * 1024 * 4224 + 1, cus * 1024 * 4352 - 1):
            add("ragged", cus, 1, total, ragged_plan(cus, total))
            add("iter", cus, 1, total, find_iter_span_multi(cus, total))
        lanes = cus * 1024
        for floor in (16, 100, 16 << 10):
            for total in spans + (floor * lanes - 1, floor * lanes, floor * lanes + 1, (floor + 1) * lanes + 1):
                for rnd in (0, 1):
                    add("device", cus, 1, total, long_geometry_kernel(lanes, total, floor, rnd), floor=floor, odd=rnd)
    for b in (0, 1, 127, 128, 129, 256, 16 << 10, 1 << 63):
        add("odd_lines", 1, 1, b, odd_lines(b))
    return rows


def test_the_issue_table():
    """The cases with fixed figures, against the formulas above."""
    assert long_batch_long(256, 1, 64 * MiB) == 16512
    assert run_find_iter_fixed(256, 1, 64 * MiB) == 4224
    assert long_batch_split(256, 1024, 1 * KiB) == 128
    assert long_batch_split(256, 64, 512) == 128 and long_batch_split(256, 64, 128) == 0
    assert ragged_plan(256, 262144 * 4224 + 1) == 4224
    assert find_iter_span_multi(256, 262144 * 4224 + 1) == 4480  # what rounding up would give


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("chunk_plan") / "chunk_plan_ctest")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-o", path,
                           os.path.join(ROOT, "tests", "ctest", "chunk_plan_ctest.cpp"),
                           "-I", os.path.join(ROOT, "regex_amd", "csrc")])
    return path


def test_header_gives_the_former_formulas(exe):
    rows = cases()
    r = subprocess.run([exe], input="\n".join(row for row, _ in rows) + "\n", capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 0, r.stderr
    out = r.stdout.split("\n")
    assert out[len(rows)] == "long_span %d lanes_per_cu 1024" % (256 * KiB)
    bad = [(row, want, int(got)) for (row, want), got in zip(rows, out) if int(got) != want]
    assert not bad, bad[:10]
