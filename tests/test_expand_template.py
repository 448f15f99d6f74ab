"""The compiled replacement template (rure_amd_expand_template_export: the
pieces the device expansion runs, host only) against regex_amd.expand, the
pinned Python statement of expand.rs:50-166: every expand! / replace!
template of the reference's vectors, its find_cap_ref cases and the edge
templates of the `$` syntax, evaluated over random group tuples with some
groups unset."""
import random
import zlib

import pytest

import regex_amd as R
from golden_data import vectors

V = vectors()

# expand.rs:195-207 (as in tests/test_replace_host.py)
FIND_CAP_REF = ["$foo", "${foo}", "$0", "$5", "$10", "$42a", "${42}a", "${42", "${42 ", " $0 ", "$", " ", ""]
EDGE = [b"$$1 $$foo ${1}x $", b"$1a", b"${1}a", b"$99", b"$nosuch", b"", b"$4294967295", b"$4294967296",
        b"${foo}${1}$$", b"a$1b$2c$0", b"$foo$", b"${", b"${}", b"$}", b"\xff$1\xff", b"$00001", b"$0$0$0"]
PATTERNS = [r"(?P<foo>\w+) (\w+)", r"a+", r"(a)(b)?(?P<x1>c)(?P<_y>d)", r"(?P<y>\d+)-(?P<m>\d+)"]


def run_pieces(pieces, lits, groups, text):
    out = bytearray()
    for kind, a, b in pieces:
        if kind == 0:
            out += lits[a:a + b]
        else:
            assert kind == 1 and b == 0 and a < len(groups)
            if groups[a] is not None:
                out += text[groups[a][0]:groups[a][1]]
    return bytes(out)


def check(re, rep):
    names = re.capture_names()
    ng = re.captures_len()
    pieces, lits = re.expand_template(rep)
    assert len(lits) <= len(rep)
    for i in range(len(pieces) - 1):
        assert not (pieces[i][0] == 0 and pieces[i + 1][0] == 0), "adjacent literals are merged"
    assert all(b > 0 for k, a, b in pieces if k == 0)
    rng = random.Random(zlib.crc32(rep) + ng)
    text = bytes(rng.randrange(256) for _ in range(48))
    for _ in range(20):
        groups = []
        for g in range(ng):
            s = rng.randint(0, len(text))
            groups.append(None if g and rng.random() < 0.3 else (s, rng.randint(s, len(text))))
        assert run_pieces(pieces, lits, groups, text) == R.expand(groups, names, rep, text), (rep, groups)


@pytest.mark.parametrize("pat", PATTERNS)
def test_edge_templates(pat):
    re = R.Regex(pat)
    for rep in EDGE + [t.encode() for t in FIND_CAP_REF]:
        check(re, rep)


def test_vector_templates():
    seen = 0
    for v in V["expand"]:
        check(R.Regex(v["re"]), bytes.fromhex(v["template"]))
        seen += 1
    for v in V["replace"]:
        check(R.Regex(v["re"]), bytes.fromhex(v["rep"]))
        seen += 1
    assert seen >= 10


def test_dropped_and_merged():
    re = R.Regex(r"(?P<foo>a)(b)")
    assert re.expand_template(b"$$1 $$foo ${1}x $") == ([(0, 0, 8), (1, 1, 0), (0, 8, 3)], b"$1 $foo x $")
    assert re.expand_template(b"$1a") == ([], b"")                      # the name "1a": unknown
    assert re.expand_template(b"${1}a") == ([(1, 1, 0), (0, 0, 1)], b"a")
    assert re.expand_template(b"x$99 y$nosuch-z") == ([(0, 0, 5)], b"x y-z")  # dropped, literals merged
    assert re.expand_template(b"") == ([], b"")
    assert re.expand_template(b"${42") == ([(0, 0, 4)], b"${42")
    assert re.expand_template(b"$foo$2$0") == ([(1, 1, 0), (1, 2, 0), (1, 0, 0)], b"")


def test_size_query():
    import ctypes
    import regex_amd._native as N
    re = R.Regex(r"(a)(b)")
    rep = b"<$1|$2>"
    n = N.rure_amd_expand_template_export(re._re, rep, len(rep), None, 0, None, 0)
    assert n == 5
    pieces = (ctypes.c_uint32 * 6)()
    assert N.rure_amd_expand_template_export(re._re, rep, len(rep), pieces, 2, None, 0) == 5
    assert list(pieces) == [0, 0, 1, 1, 1, 0]
    assert N.rure_amd_expand_template_export(None, rep, len(rep), None, 0, None, 0) == N.ERR_ARG
