"""The engine paths (rure_amd_path, include/rure_amd.h) are named once: the
Python mirror follows the header, the values are frozen (recorded profiles
and the bench hold them), and the library notes a path only by name."""
import glob
import os
import re

from regex_amd import Path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FROZEN = {
    "NONE": -1, "LANE_STREAM": 0, "TILE1": 1, "TILE2": 2, "TILE4": 4, "ANCHORED_REVERSE": -2, "LITERAL": -3,
    "LONG_SCAN": -4, "LANE_SEARCH": -5, "BIG_DFA": -6, "LINES": -8, "SUFFIX_LONG": -9, "LAZY_DFA": -10,
    "SUFFIX_ITER": -11, "ITER_LOOKS": -12, "ITER_LOOKS_QUIT": -13, "ITER_SHADOW": -14, "ITER_SHADOW_QUIT": -15,
    "PIKE_ONLY": -16, "SET_CORE_OFFSETS": -17, "ITER_RUNS": -19, "ITER_RUNS_ASCII": -20, "ITER_CHUNKED": -21,
    "ITER_WAVE": -22, "REPLACE_CLASS": -23, "REPLACE_HMAP": -24, "ITER_SHADOW_GATED": -25,
    "ITER_WAVE_SERVED": -27, "CAPTURES_ITER": -28, "REPLACE_EXPAND": -29,
}


def _header_enum():
    text = open(os.path.join(ROOT, "include", "rure_amd.h")).read()
    body = re.search(r"typedef enum rure_amd_path \{(.*?)\} rure_amd_path;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    items = [x.strip() for x in body.split(",") if x.strip()]
    out = {}
    for item in items:
        m = re.fullmatch(r"RURE_AMD_PATH_(\w+) = (-?\d+)", item)
        assert m, item
        assert m.group(1) not in out, item
        out[m.group(1)] = int(m.group(2))
    return out


def test_python_mirrors_header():
    # __members__ lists aliases too: two names for one value would show here
    assert {k: int(v) for k, v in Path.__members__.items()} == _header_enum()


def test_values_frozen():
    assert {k: int(v) for k, v in Path.__members__.items()} == FROZEN
    assert len(set(FROZEN.values())) == len(FROZEN)


def test_library_notes_paths_by_name():
    srcs = [p for p in glob.glob(os.path.join(ROOT, "regex_amd", "csrc", "**", "*"), recursive=True)
            if p.endswith((".cpp", ".hip", ".hpp", ".h"))]
    assert len(srcs) > 10
    calls = 0
    for p in srcs:
        for n, line in enumerate(open(p, encoding="utf-8", errors="replace"), 1):
            for arg in re.findall(r"note_fwd_path\(\s*([^)]*)", line):
                calls += 1
                assert not re.search(r"(?<![\w.])[-+]?\d", arg), "%s:%d: %s" % (p, n, line.strip())
    assert calls > 20
