"""No scratch block outlives a batched call: after each entry point has run
once and the stream is synchronised, scratch_stats()["live"] is 0, on the
smallest shapes that reach each branch of the host dispatch that allocates
(the quit flag and its Pike VM fallback, the deferred long scan, the ragged
find_iter plan, the on-demand DFA's rounds, the match list of replace / split
/ captures_iter).  Every result is the CPU oracle's."""
import numpy as np
import pytest

import regex_amd as R
from oracle_py import OracleRegex
import replace_ref as RR

pytestmark = pytest.mark.gpu

L = 64
_LINE = (b"Mr Sherlock Holmes met Dr Watson. No one saw Mrs Hudson; Mary Watson said Mycroft Holmes goes "
         b"to see John Watson or Irene Adler, and Sherlock Holmes does too. ")
EIGHT = [(_LINE * 2)[11 * i:11 * i + L] for i in range(8)]
NON_ASCII = ["é Holmes goes home; café closes, she sees é".encode()]
GROUPS = r"([A-Z][a-z]+) (Holmes|Watson)"
WORDS = r"\b([a-z]+)(e)s\b"  # a Unicode word boundary: the DFA quits on a non-ASCII byte

# name: (regex, set patterns, texts, offset batch, knobs)
SHAPES = {
    "fixed_stride": (GROUPS, ["Holmes", "Watson$"], EIGHT, False, {}),
    "long_ragged": (GROUPS, ["Holmes", "Watson$"], EIGHT, True, dict(long_ragged=2, long_chunk=16)),
    "iter_ragged": (GROUPS, ["Holmes", "Watson$"], EIGHT, True, dict(iter_ragged=2, iter_chunk=16)),
    "quit_fallback": (WORDS, [r"\bgoes\b", "Watson"], NON_ASCII, False, {}),
    "lazy_rounds": (GROUPS, ["Holmes", "Watson$"], EIGHT, False, dict(lazy=1, lazy_rows=1)),
}


def _settled():
    import torch
    torch.cuda.synchronize()
    return R.scratch_stats()["live"]


def _pairs(t):
    return [tuple(x) for x in t.cpu().numpy().tolist()]


def _per_haystack(counts, rows):
    out, at = [], 0
    for c in counts.cpu().numpy().tolist():
        out.append(rows[at:at + c])
        at += c
    assert at == len(rows)
    return out


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_no_live_scratch_after_a_call(cuda, shape):
    import torch
    pat, set_pats, texts, ragged, knobs = SHAPES[shape]
    assert all(len(t) == len(texts[0]) for t in texts)
    re, rs = R.Regex(pat), R.RegexSet(set_pats)
    o, os_ = OracleRegex(re), OracleRegex(rs)
    names, ng = re.capture_names(), re.captures_len()
    hay = torch.from_numpy(np.frombuffer(b"".join(texts) + b"\0" * 16, dtype=np.uint8).copy()).to(cuda)
    n, w = len(texts), len(texts[0])
    if ragged:
        where = dict(offsets=torch.arange(0, (n + 1) * w, w, dtype=torch.int64).to(cuda))
    else:
        where = dict(stride=w, length=w, count=n)
    live = {}

    def call(what, fn, *args, **kw):
        with R.debug(**knobs):
            out = fn(hay, *args, **dict(where, **kw))
            live[what] = _settled()
        return out

    assert _settled() == 0
    got = call("find", re.find_batch)
    assert _pairs(got) == [o.find(t) or (-1, -1) for t in texts]
    got = call("is_match", re.is_match_batch)
    assert got.cpu().numpy().tolist() == [int(o.is_match(t)) for t in texts]
    got = call("shortest_match", re.shortest_match_batch)
    assert got.cpu().numpy().tolist() == [(lambda e: -1 if e is None else e)(o.shortest_match(t)) for t in texts]

    def groups(row):
        g = [None if a < 0 or b < 0 else (a, b) for a, b in row]
        return None if g[0] is None else g

    got = call("captures", re.captures_batch).cpu().numpy().tolist()
    assert [groups(r) for r in got] == [o.captures(t) for t in texts]
    counts, ms = call("find_iter", re.find_iter_batch)
    assert _per_haystack(counts, _pairs(ms)) == [o.find_iter(t) for t in texts]
    counts, rows, _ = call("captures_iter", re.captures_iter_batch)
    assert _per_haystack(counts, [groups(r) for r in rows.cpu().numpy().tolist()]) == \
        [RR.captures_iter(o, t) for t in texts]

    def outputs(out, ooff):
        ob, oo = bytes(out.cpu().numpy()), ooff.cpu().numpy().tolist()
        return [ob[oo[i]:oo[i + 1]] for i in range(n)]

    out, ooff = call("replace", re.replace_batch, b"<$2>")
    assert outputs(out, ooff) == [RR.replacen(o, names, t, 0, b"<$2>", True) for t in texts]
    out, ooff = call("replace_expand", re.replace_batch, b"<$2:$1>", expand=True)
    assert outputs(out, ooff) == [RR.replacen(o, names, t, 0, b"<$2:$1>", False) for t in texts]
    counts, pieces = call("split", re.split_batch)
    assert [[t[a:b] for a, b in p] for t, p in zip(texts, _per_haystack(counts, _pairs(pieces)))] == \
        [RR.split(o, t) for t in texts]
    got = call("set_matches", rs.matches_batch).cpu().numpy().tolist()
    assert [[j for j in range(len(set_pats)) if (m >> j) & 1] for m in got] == [os_.matches(t) for t in texts]

    assert len(live) == 10 and not any(live.values()), live
    if shape == "quit_fallback":  # the inputs do reach it
        assert ng == 3 and len(o.find_iter(texts[0])) == 3 and os_.matches(texts[0]) == [0]
