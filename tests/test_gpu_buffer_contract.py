"""The buffer contract of the batched calls (include/rure_amd.h, "Outputs"),
on the GPU, bit-exact against the CPU oracle over the haystack bytes alone:

 (a) a cut output: counts and total exact, the rows below the capacity the
     oracle's, nothing at or past the capacity (or in front) written;
 (b) the capacity never changes the rows (it sizes the dense slot geometry);
 (c) record outputs that are 8- but not 16-byte aligned;
 (d) haystacks at any base address and stride, surrounded by bytes that
     would change the result if an engine read them as text;
 (e) the other record producers (split, captures_iter, spans, compaction);
 (f) the byte outputs of replace.

One test function per property, over tests/buffer_contract.py's table of
find_iter engines (tests/test_buffer_contract_cases.py checks on the CPU that
every case's cut set means something)."""
import numpy as np
import pytest

import regex_amd as R
from regex_amd import Path
from regex_amd import _native as N
import buffer_contract as BC
from buffer_contract import Arena, RaggedArena
from oracle_py import OracleRegex
import replace_ref as RR

pytestmark = pytest.mark.gpu

IDS = [c.name for c in BC.CASES]


def _layout(case, cuda, L=None, k=0, stride=None, fill="zero"):
    """(hay, keyword arguments of the batch) of the case's haystacks."""
    hays = BC.expected(case, L)[0]
    if case.ragged:
        a = RaggedArena(hays, k=k, fill=fill)
        return a.hay(cuda), {"offsets": a.offsets(cuda), "start": case.start}
    a = Arena(hays, k=k, stride=stride, fill=fill)
    return a.hay(cuda), {"stride": a.S, "length": a.L, "count": a.n, "start": case.start}


def _check(res, counts, rows, cap, what):
    assert res.guard_ok, ("written outside the output", what)
    assert res.total == len(rows), (what, res.total, len(rows))
    assert np.array_equal(res.counts, counts), what
    k = min(len(rows), cap)
    assert res.rows.shape[0] == k
    bad = np.nonzero((res.rows != rows[:k]).any(axis=1))[0]
    assert bad.size == 0, (what, int(bad[0]), res.rows[bad[0]].tolist(), rows[bad[0]].tolist())


@pytest.mark.parametrize("case", BC.CASES, ids=IDS)
def test_cut_output(cuda, knobs, case):
    """(a)"""
    knobs(**case.knobs)
    re = R.Regex(case.pat)
    hays, counts, rows = BC.expected(case)
    hay, kw = _layout(case, cuda)
    for cap in BC.cut_points(case, hays, counts, rows):
        _check(BC.raw_find_iter(re, hay, cap, **kw), counts, rows, cap, (case.name, cap))
    _check(BC.raw_find_iter(re, hay, 0, null=True, **kw), counts, rows, 0, (case.name, "NULL"))


@pytest.mark.parametrize("case", BC.CASES, ids=IDS)
def test_capacity_invariance(cuda, knobs, case):
    """(b)"""
    knobs(**case.knobs)
    re = R.Regex(case.pat)
    hays, counts, rows = BC.expected(case)
    T = len(rows)
    hay, kw = _layout(case, cuda)
    got = [BC.raw_find_iter(re, hay, cap, **kw) for cap in (T, 2 * T + 7, 64 * T)]
    for cap, g in zip((T, 2 * T + 7, 64 * T), got):
        assert np.array_equal(g.rows, got[0].rows) and np.array_equal(g.counts, got[0].counts), (case.name, cap)
        _check(g, counts, rows, cap, (case.name, cap))


@pytest.mark.parametrize("case", BC.CASES, ids=IDS)
def test_output_alignment(cuda, knobs, case):
    """(c)"""
    knobs(**case.knobs)
    re = R.Regex(case.pat)
    hays, counts, rows = BC.expected(case)
    T = len(rows)
    hay, kw = _layout(case, cuda)
    for cap in (T // 2, T):
        _check(BC.raw_find_iter(re, hay, cap, off8=True, **kw), counts, rows, cap, (case.name, cap, "+8"))


@pytest.mark.parametrize("case", BC.CASES, ids=IDS)
def test_surroundings_and_placement(cuda, knobs, case):
    """(d): every fill x base misalignment x (16-byte stride, stride = length
    + 5, odd length); the engine is asserted for the aligned zero-fill layout
    only (elsewhere another kernel may answer, with the same results)."""
    knobs(**case.knobs)
    re = R.Regex(case.pat)
    shapes = [(None, None)] if case.ragged else [(case.L, case.L), (case.L, case.L + 5), (case.L - 3, case.L - 3)]
    for L, S in shapes:
        hays, counts, rows = BC.expected(case, L)
        cap = len(rows) + 1
        for fill in BC.FILLS:
            for k in BC.KS:
                hay, kw = _layout(case, cuda, L, k, S, fill)
                res = BC.raw_find_iter(re, hay, cap, **kw)
                _check(res, counts, rows, cap, (case.name, L, S, fill, k))
                if case.path is not None and fill == "zero" and k == 0 and S in (None, case.L):
                    assert res.path in case.path, (case.name, res.path)


# ------------------------------------------- (d) find / is_match / shortest / set / captures

def _small_hays(n, L, seed):
    from test_gpu_split import _buf
    buf = _buf(n, L, L, seed)
    return [bytes(buf[i * L:(i + 1) * L]) for i in range(n)], buf


FIND_PATS = [r"\d{4}-\d{2}-\d{2}", r"\w+@\w+\.\w+", r"(?m)^abc$", r"\bfoo\b", r"(a|ab)(c|bcd)", r"x*"]
# (a Unicode \b next to the planted non-ASCII bytes sends a haystack to the Pike VM: 112-byte haystacks only)
FIND_CASES = [(p, L) for L in (112, 1024) for p in FIND_PATS if not (p == r"\bfoo\b" and L == 1024)]
_small = {}


def _small_expected(pat, L):
    """find / is_match / shortest_match of 300 haystacks of L bytes, once."""
    if (pat, L) not in _small:
        hays, buf = _small_hays(300, L, 0x5151 + L)
        o = OracleRegex(R.Regex(pat))
        f, _ = o.find_batch(buf, L, L, 300, nthreads=4)
        _small[(pat, L)] = (hays, f.astype(np.int64), o.is_match_batch(buf, L, L, 300, 4).astype(bool),
                            o.shortest_batch(buf, L, L, 300, 4).astype(np.int64))
    return _small[(pat, L)]


def _guarded(dev, n, words, dtype):
    """n x words outputs with 64 sentinel elements behind them."""
    import torch
    t = torch.full((n * words + 64,), 0x5A, dtype=dtype, device=dev)
    return t, lambda: bool((t[n * words:] == 0x5A).all().item())


@pytest.mark.parametrize("pat,L", FIND_CASES)
def test_find_family_surroundings(cuda, pat, L):
    """(d) for find_batch, is_match_batch and shortest_match_batch: 300
    haystacks of 100 to 1024 bytes (the tile kernels, the lane stream, the
    split is_match units; as an offset batch the line kernel)."""
    import torch
    re = R.Regex(pat)
    seen = {}  # zero fill: (offset batch, aligned base, 16-byte stride) -> the paths of find and is_match
    for LL, S in ((L, L), (L, L + 5), (L - 3, L - 3)):
        hays, ef, em, es = _small_expected(pat, LL)
        for fill in BC.FILLS:
            for k in BC.KS:
                a = Arena(hays, k=k, stride=S, fill=fill)
                batches = [{"stride": S, "length": LL, "count": a.n}]
                if S == LL:
                    batches.append({"offsets": a.offsets(cuda)})
                for kw in batches:
                    what = (pat, LL, S, fill, k, sorted(kw))
                    f, fok = _guarded(cuda, a.n, 2, torch.int64)
                    m, mok = _guarded(cuda, a.n, 1, torch.uint8)
                    s, sok = _guarded(cuda, a.n, 1, torch.int64)
                    re.find_batch(a.hay(cuda), out=f, **kw)
                    pf = N.last_path()
                    re.is_match_batch(a.hay(cuda), out=m, **kw)
                    if fill == "zero":
                        seen[("offsets" in kw, k == 0, S % 16 == 0)] = (pf, N.last_path())
                    re.shortest_match_batch(a.hay(cuda), out=s, **kw)
                    assert fok() and mok() and sok(), what
                    assert np.array_equal(f[:2 * a.n].view(a.n, 2).cpu().numpy(), ef), what
                    assert np.array_equal(m[:a.n].cpu().numpy().astype(bool), em), what
                    assert np.array_equal(s[:a.n].cpu().numpy(), es), what
    if pat in FIND_PATS[:2]:
        # the kernels the placements reach (dfa_scan.hip launch_dfa_fwd, dispatch.cpp long_batch): the tile
        # kernel needs a 16-byte-aligned base and stride and 128 bytes, is_match over 300 x 1 KiB is split into
        # units, an offset batch takes the line kernel, everything else one streaming lane per haystack
        tiles = (Path.TILE1, Path.TILE2, Path.TILE4)
        assert seen[(False, True, True)][0] in (tiles if L >= 128 else (Path.LANE_STREAM,)), seen
        assert seen[(False, False, True)][0] == Path.LANE_STREAM and seen[(False, True, False)][0] == Path.LANE_STREAM
        assert seen[(True, True, True)][0] == Path.LINES and seen[(True, False, True)][0] == Path.LINES, seen
        if L >= 512:
            assert all(v[1] == Path.LONG_SCAN for key, v in seen.items() if not key[0]), seen


SET_PATS = [r"\d{4}-\d{2}-\d{2}", r"\w+@\w+\.\w+", r"(?m)^abc$", r"(?-u)\bfoo\b", r"x+y"]


@pytest.mark.parametrize("L", [112, 400])
def test_set_and_captures_surroundings(cuda, L):
    """(d) for set_matches_batch and captures_batch."""
    import torch
    rs = R.RegexSet(SET_PATS)
    rc = R.Regex(r"(\w+)@(\w+)\.(\w+)")
    oc = OracleRegex(rc)
    for LL, S in ((L, L), (L, L + 5), (L - 3, L - 3)):
        hays, buf = _small_hays(300, LL, 0x5151 + LL)
        emask = OracleRegex(rs).set_batch(buf, LL, LL, 300, 4).astype(np.int64)
        ecap = np.full((300, 4, 2), -1, dtype=np.int64)
        for i, h in enumerate(hays):
            g = oc.captures(h)
            if g is not None:
                ecap[i] = [(-1, -1) if x is None else x for x in g]
        assert (ecap[:, 0, 0] >= 0).sum() >= 10 and (emask != 0).sum() >= 30
        for fill in BC.FILLS:
            for k in BC.KS:
                a = Arena(hays, k=k, stride=S, fill=fill)
                kw = {"stride": S, "length": LL, "count": a.n}
                m, mok = _guarded(cuda, a.n, 1, torch.int64)
                c, cok = _guarded(cuda, a.n, 8, torch.int64)
                rs.matches_batch(a.hay(cuda), out=m, **kw)
                rc.captures_batch(a.hay(cuda), out=c, **kw)
                assert mok() and cok(), (LL, S, fill, k)
                assert np.array_equal(m[:a.n].cpu().numpy(), emask), (LL, S, fill, k)
                assert np.array_equal(c[:8 * a.n].view(a.n, 4, 2).cpu().numpy(), ecap), (LL, S, fill, k)


# ------------------------------------------------------- (e) the other producers

def _cuts(T):
    return sorted({0, 1, T // 2, T - 1, T, T + 1} - {-1})


def _stream_hays(texts, L, n):
    """n haystacks of L bytes cut from the texts joined."""
    t = b"".join(texts)
    assert len(t) >= n * L
    return [t[i * L:(i + 1) * L] for i in range(n)]


@pytest.mark.parametrize("limit", [None, 0, 1, 3])
def test_split_cut(cuda, limit):
    """(e) split_batch: test_gpu_replace's alphabet, 200 haystacks of 40
    bytes at stride 45 from a misaligned base."""
    from test_gpu_replace import _texts
    pat = r"[ \t]+"
    re = R.Regex(pat)
    o = OracleRegex(re)
    hays = _stream_hays(_texts(BC._seed(pat) + 7, 600, 60), 40, 200)
    per = [BC.split_spans(o.find_iter(h), len(h), limit) for h in hays]
    for h, p in zip(hays[:20], per[:20]):  # the offsets are replace_ref's fields
        assert [h[a:b] for a, b in p] == (RR.split(o, h) if limit is None else RR.splitn(o, h, limit))
    counts = np.array([len(p) for p in per], dtype=np.int64)
    rows = np.array([f for p in per for f in p], dtype=np.int64).reshape(-1, 2)
    T = len(rows)
    assert T >= (40 if limit != 0 else 0)
    for fill in BC.FILLS:
        a = Arena(hays, k=1, stride=45, fill=fill)
        kw = {"stride": 45, "length": 40, "count": 200}
        for cap in _cuts(T):
            _check(BC.raw_split(re, a.hay(cuda), limit, cap, **kw), counts, rows, cap, (limit, fill, cap))
    _check(BC.raw_split(re, a.hay(cuda), limit, T // 2, off8=True, **kw), counts, rows, T // 2, (limit, "+8"))


def test_captures_iter_cut(cuda):
    """(e) captures_iter_batch: test_gpu_captures' alphabet, a regex without
    look-around (its rows never diverge)."""
    from test_gpu_captures import _texts
    pat = r"(\w)(\d)?"
    re = R.Regex(pat)
    o = OracleRegex(re)
    hays = _stream_hays(_texts(BC._seed(pat), 600), 40, 200)
    per = [RR.captures_iter(o, h) for h in hays]
    counts = np.array([len(p) for p in per], dtype=np.int64)
    rows = np.array([[(-1, -1) if g is None else g for g in c] for p in per for c in p], dtype=np.int64)
    rows = rows.reshape(-1, 6)
    T = len(rows)
    assert T >= 40
    for fill in BC.FILLS:
        a = Arena(hays, k=1, stride=45, fill=fill)
        kw = {"stride": 45, "length": 40, "count": 200}
        for cap in _cuts(T):
            res = BC.raw_captures_iter(re, a.hay(cuda), cap, **kw)
            _check(res, counts, rows, cap, (fill, cap))
            assert not res.diverged.any()
    _check(BC.raw_captures_iter(re, a.hay(cuda), T // 2, off8=True, **kw), counts, rows, T // 2, "+8")


@pytest.mark.parametrize("pat", [r"\w+", r"[a-z]+ing", r"\b\w+\b"])
def test_span_cut(cuda, pat):
    """(e) find_iter_span: two spans, the second entered with the first's
    exit; each span's rows are the whole iteration's matches that start in
    it, whatever the capacity."""
    from golden_data import corpus
    text = corpus("sherlock")[:60000]
    re = R.Regex(pat)
    allm = OracleRegex(re).find_iter_array(text).astype(np.int64).reshape(-1, 2)
    n, mid = len(text), len(text) // 3 + 5
    first, second = allm[allm[:, 0] < mid], allm[allm[:, 0] >= mid]
    assert len(first) >= 40 and len(second) >= 40
    one = np.ones(1, dtype=np.int64)
    for fill in BC.FILLS:
        a = Arena([text], k=1, fill=fill)
        hay = a.hay(cuda)
        exit0 = None
        for cap in _cuts(len(first)):
            r0 = BC.raw_span(re, hay, n, 0, mid, cap)
            _check(BC.Result(counts=one, total=r0.total, rows=r0.rows, guard_ok=r0.guard_ok), one, first, cap,
                   (pat, fill, cap, "first"))
            assert exit0 is None or np.array_equal(exit0, r0.exit)
            exit0 = r0.exit
        for cap in _cuts(len(second)):
            r1 = BC.raw_span(re, hay, n, mid, n, cap, entry=exit0)
            _check(BC.Result(counts=one, total=r1.total, rows=r1.rows, guard_ok=r1.guard_ok), one, second, cap,
                   (pat, fill, cap, "second"))
    r1 = BC.raw_span(re, hay, n, mid, n, len(second) // 2, entry=exit0, off8=True)
    _check(BC.Result(counts=one, total=r1.total, rows=r1.rows, guard_ok=r1.guard_ok), one, second, len(second) // 2,
           (pat, "+8"))


@pytest.mark.parametrize("kmer", [1, 0])
def test_span_multi_cut(cuda, knobs, kmer):
    """(e) find_iter_span_multi (the k-mer probes; Shift-And words with
    kmer=0): a different capacity for every regex."""
    if not kmer:
        knobs(kmer=0)
    text = BC.multi_text()
    res = [R.Regex(p) for p in BC.MULTI_PATS]
    exp = [OracleRegex(r).find_iter_array(text).astype(np.int64).reshape(-1, 2) for r in res]
    cuts = [_cuts(len(e)) for e in exp]
    one = np.ones(1, dtype=np.int64)
    for fill in BC.FILLS:
        a = Arena([text], k=1, fill=fill)
        for j in range(len(cuts[0])):
            caps = [cuts[i][(j + 2 * i) % len(cuts[i])] for i in range(len(res))]
            got = BC.raw_span_multi(res, a.hay(cuda), len(text), 0, len(text), caps, off8=(j % 2 == 1))
            for i, g in enumerate(got):
                _check(BC.Result(counts=one, total=g.total, rows=g.rows, guard_ok=g.guard_ok), one, exp[i], caps[i],
                       (kmer, fill, i, caps))


def test_compact_cut(cuda):
    """(e) compact_matches over test_gpu_gather's synthetic find output."""
    import torch
    n = 5000
    rng = np.random.default_rng(n)
    f = np.full((n, 2), -1, dtype=np.int64)
    hit = np.sort(rng.choice(n, size=n * 3 // 10, replace=False))
    f[hit, 0] = rng.integers(0, 1 << 40, size=hit.size)
    f[hit, 1] = f[hit, 0] + rng.integers(0, 100, size=hit.size)
    found = torch.from_numpy(f).to(cuda)
    exp = np.stack([hit + 12345, f[hit, 0], f[hit, 1]], 1)
    T = len(exp)
    for off8 in (False, True):
        for cap in _cuts(T):
            r = BC.raw_compact(found, 12345, cap, off8)
            assert r.guard_ok and r.total == T, (cap, off8)
            assert np.array_equal(r.rows, exp[:min(T, cap)]), (cap, off8)


# -------------------------------------------------------------- (f) byte outputs

def _replace_expected(o, hays, rep, limit, names=None, expand=False):
    outs, marks = [], []
    for h in hays:
        if expand:
            caps = RR.captures_iter(o, h)
            spans = [c[0] for c in caps]
            reps = [R.expand(c, names, rep, h) for c in caps]
        else:
            spans = o.find_iter(h)
            reps = [rep] * len(spans)
        out, mark = BC.replace_marked(h, spans, reps, limit)
        assert out == RR.replacen(o, names, h, limit, rep, not expand)  # replace_ref's output
        outs.append(out)
        marks.append(mark)
    ooff = np.zeros(len(hays) + 1, dtype=np.int64)
    ooff[1:] = np.cumsum([len(x) for x in outs])
    return b"".join(outs), b"".join(marks), ooff


def _check_bytes(res, exp, ooff, cap, what):
    assert res.rc == N.OK, what
    assert res.guard_ok, ("written outside out_capacity", what)
    assert res.total == len(exp), (what, res.total, len(exp))
    assert np.array_equal(res.out_offsets, ooff), what
    assert res.out == exp[:cap], what


@pytest.mark.parametrize("limit", [0, 2])
def test_replace_generic_cut(cuda, limit):
    """(f) replace_batch, the generic copy: 200 haystacks, a replacement of
    three bytes."""
    from test_gpu_replace import _texts
    pat, rep = r"\d+", b"<->"
    re = R.Regex(pat)
    o = OracleRegex(re)
    hays = _stream_hays(_texts(BC._seed(pat) + limit, 600, 60), 40, 200)
    exp, mark, ooff = _replace_expected(o, hays, rep, limit)
    assert rep in exp
    for fill in BC.FILLS:
        a = Arena(hays, k=1, stride=45, fill=fill)
        for cap in BC.byte_cut_points(len(exp), mark):
            res = BC.raw_replace(re, a.hay(cuda), rep, limit, cap, stride=45, length=40, count=200)
            _check_bytes(res, exp, ooff, cap, (limit, fill, cap))


@pytest.mark.parametrize("generic", [0, 1])
def test_replace_one_haystack_cut(cuda, knobs, generic):
    """(f) replace_all over one haystack: the one-byte-class path
    (test_gpu_replace_class's [KM] text) and, with replace_generic=1, the
    generic per-block copy of the same call; without the knob and with a
    regex that is no byte class, the grouped copy."""
    from test_gpu_replace_class import text
    knobs(replace_generic=generic)
    t = text(5, 20000, b"acgtKM")
    for pat, rep in ((r"[KM]", b"(a|c)"), (r"[KM]+", b"(a|c)"), (r"g[KM]?", b"")):
        re = R.Regex(pat)
        exp, mark, ooff = _replace_expected(OracleRegex(re), [t], rep, 0)
        pts = BC.byte_cut_points(len(exp), mark) if rep else sorted({0, 1, 15, 16, 17, len(exp) - 1, len(exp),
                                                                     len(exp) + 1, len(exp) // 2 + 3})
        for fill in ("zero", "self"):
            a = Arena([t], k=0, fill=fill)
            for cap in pts:
                res = BC.raw_replace(re, a.hay(cuda), rep, 0, cap, stride=len(t), length=len(t), count=1)
                _check_bytes(res, exp, ooff, cap, (pat, generic, fill, cap))
                if pat == r"[KM]" and not generic:
                    assert res.path == Path.REPLACE_CLASS


def test_replace_expand_cut(cuda):
    """(f) replace_expand_batch: `$` groups; its byte stores take an output
    of any alignment (here 1 byte past a 16-byte boundary)."""
    from test_gpu_captures import _texts
    pat, rep = r"([0-9]+)(\.[0-9]+)?", b"<$2|$1>"
    re = R.Regex(pat)
    o = OracleRegex(re)
    hays = _stream_hays(_texts(BC._seed(pat), 600), 40, 200)
    for limit in (0, 2):
        exp, mark, ooff = _replace_expected(o, hays, rep, limit, re.capture_names(), True)
        for fill in BC.FILLS:
            a = Arena(hays, k=1, stride=45, fill=fill)
            for shift in (0, 1):
                for cap in BC.byte_cut_points(len(exp), mark):
                    res = BC.raw_replace(re, a.hay(cuda), rep, limit, cap, stride=45, length=40, count=200,
                                         expand=True, shift=shift)
                    _check_bytes(res, exp, ooff, cap, (limit, fill, shift, cap))
                    assert res.path == Path.REPLACE_EXPAND and not res.diverged.any()


@pytest.mark.parametrize("shift", [1, 8])
def test_replace_rejects_a_misaligned_out(cuda, shift):
    """rure_amd_replace_batch stores whole 16-byte blocks: an `out` that is
    not 16-byte aligned is RURE_AMD_ERR_ARG and nothing is launched (the
    buffer, the offsets and the total keep their sentinels)."""
    from test_gpu_replace_class import text
    t = text(5, 5000, b"acgtKM")
    a = Arena([t], k=0)
    for pat in (r"[KM]", r"[KM]+"):
        res = BC.raw_replace(R.Regex(pat), a.hay(cuda), b"(a|c)", 0, 8000, stride=len(t), length=len(t), count=1,
                             shift=shift)
        assert res.rc == N.ERR_ARG and res.untouched, (pat, shift)


def test_wrapper_needs_no_slack(cuda):
    """Regex.replace_batch allocates exactly the bytes it asks for."""
    from test_gpu_replace_class import text
    t = text(5, 5000, b"acgtKM")
    a = Arena([t], k=0)
    re = R.Regex(r"[KM]+")
    out, ooff = re.replace_batch(a.hay(cuda), b"(a|c)", stride=len(t), length=len(t), count=1)
    exp = RR.replacen(OracleRegex(re), None, t, 0, b"(a|c)", True)
    assert bytes(out.cpu().numpy()) == exp and ooff.cpu().numpy().tolist() == [0, len(exp)]
    assert out.untyped_storage().nbytes() == max(a.hay(cuda).numel() + 1024, len(exp))
