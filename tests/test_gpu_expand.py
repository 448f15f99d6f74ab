"""Batched captures_iter and `$`-expanding replace on the GPU
(rure_amd_captures_iter_batch: a wave per find_iter match through the
captures Pike VM; rure_amd_replace_expand_batch: compiled template, plan and
write over the rows) against the oracle's sequential captures_iter /
replacen (tests/replace_ref.py), including the haystacks where
captures_iter's matches differ from find_iter's (a look-ahead at the cut of
the captures window): flagged by the device, resolved by the sequential path."""
import ctypes
import zlib

import numpy as np
import pytest

import regex_amd as R
from regex_amd import Path
import regex_amd._native as N
from golden_data import vectors
from oracle_py import OracleRegex
import replace_ref as RR
from test_gpu_captures import CAP_PATTERNS, _texts, ragged

pytestmark = pytest.mark.gpu

V = vectors()

LOOKS = [r"(?m)^(\w+) (\w+)$", r"(a..$)|(a)", r"(ab|a)(bc|c)?$", r"(x)(?-u:\b)", r"^(a+)(b*)", r"(a+)(b*)$",
         r"\b(\w+)\b", r"(\w)\B(\w)", r"(?-u:\b)(a+)"]
LOOK_FREE = [p for p in CAP_PATTERNS if p not in LOOKS] + [r"(\w)(\d)?"]
QUIET_LOOKS = [r"\b(\w+)\b", r"(\w)\B(\w)", r"(?m)^(\w+) (\w+)$", r"^(a+)(b*)", r"(a+)(b*)$"]
# (oracle counts; the third has a Unicode \b and no literal prefix, the last two have other prefix searchers
# than one byte: 182, 77 and 51 by the same CPU check)
DIVERGING = [(r"(a..$)|(a)", 205), (r"(a..\b)|(a)", 42), (r"(\w..\b)|(\w)", 182), (r"([ab]..\b)|([ab])", 77),
             (r"(?:x|ab)(..\b)?", 51)]

_oracle_cache = {}


def oracle_rows(pat, texts_key, texts):
    """(captures_iter, find_iter) of the oracle per text, computed once."""
    key = (pat, texts_key)
    if key not in _oracle_cache:
        o = OracleRegex(R.Regex(pat))
        _oracle_cache[key] = ([RR.captures_iter(o, t) for t in texts], [o.find_iter(t) for t in texts])
    return _oracle_cache[key]


def run_batch(re, texts, cuda, **kw):
    import torch
    buf, offs = ragged(texts)
    counts, groups, div = re.captures_iter_batch(torch.from_numpy(buf).to(cuda),
                                                 offsets=torch.from_numpy(offs).to(cuda), **kw)
    return counts.cpu().numpy(), groups.cpu().numpy(), div.cpu().numpy()


def split_rows(counts, groups):
    out, k = [], 0
    for c in counts:
        out.append([[None if a < 0 or b < 0 else (a, b) for a, b in row] for row in groups[k:k + c].tolist()])
        k += int(c)
    assert k == len(groups)
    return out


def std_texts(pat):
    return _texts(zlib.crc32(pat.encode()), 400)


@pytest.mark.parametrize("pat", LOOK_FREE)
def test_look_free(cuda, pat):
    re = R.Regex(pat)
    assert re.nfa_tables()[0]["looks"] == 0
    texts = std_texts(pat)
    exp, _ = oracle_rows(pat, "std", texts)
    counts, groups, div = run_batch(re, texts, cuda, resolve=False)
    assert N.last_path() == Path.CAPTURES_ITER
    assert div.shape == (len(texts),) and div.sum() == 0
    assert groups.shape[1:] == (re.captures_len(), 2)
    got = split_rows(counts, groups)
    for i, t in enumerate(texts):
        assert got[i] == exp[i], (pat, t)


@pytest.mark.parametrize("pat", QUIET_LOOKS)
def test_looks_that_do_not_diverge(cuda, pat):
    re = R.Regex(pat)
    assert re.nfa_tables()[0]["looks"] != 0
    texts = std_texts(pat)
    exp, fi = oracle_rows(pat, "std", texts)
    assert all([c[0] for c in e] == f for e, f in zip(exp, fi)), "the oracle shows no diverging haystack"
    counts, groups, div = run_batch(re, texts, cuda, resolve=False)
    assert div.sum() == 0
    got = split_rows(counts, groups)
    for i, t in enumerate(texts):
        assert got[i] == exp[i], (pat, t)


@pytest.mark.parametrize("pat,ndiv", DIVERGING)
def test_diverging(cuda, pat, ndiv):
    """Regexes with a Unicode \\b and prefix literals (`a`; the bytes `a` `b`;
    `x` `ab`) depend on the reference's start-state prefix skip
    (dfa.rs:700-711): its DFA never reads, so never quits on, a non-ASCII byte
    that lies before a prefix candidate, and takes the captures from the cut
    window there, not from the whole text."""
    re = R.Regex(pat)
    texts = std_texts(pat)
    exp, fi = oracle_rows(pat, "std", texts)
    want = np.array([[c[0] for c in e] != f for e, f in zip(exp, fi)])
    assert want.sum() == ndiv
    counts, groups, div = run_batch(re, texts, cuda, resolve=False)
    assert np.array_equal(div != 0, want)
    got = split_rows(counts, groups)
    for i, t in enumerate(texts):
        if not want[i]:
            assert got[i] == exp[i], (pat, t)
    counts, groups, div = run_batch(re, texts, cuda)
    assert np.array_equal(div != 0, want)
    got = split_rows(counts, groups)
    for i, t in enumerate(texts):
        assert got[i] == exp[i], (pat, t)
    # a capacity below the total, with haystacks to splice: still a prefix
    cap = len(groups) // 2
    c2, g2, _ = run_batch(re, texts, cuda, capacity=cap)
    assert np.array_equal(c2, counts) and np.array_equal(g2, groups[:cap])


def test_scratch_path(cuda):
    """A program whose per-wave slot rows exceed LDS (global scratch rows)."""
    re = R.Regex(r"(\w+) (\w+) (\w+) (\w+) (\w+)")
    info = re.nfa_tables()[0]
    ns = 2 * re.captures_len()
    assert info["leaves"] * (16 * ns + 12) > 160 * 1024
    o = OracleRegex(re)
    texts = [("héllo wörld foo bar baz qux " * k).encode() for k in range(1, 6)] + _texts(77, 60, 80)
    counts, groups, div = run_batch(re, texts, cuda, resolve=False)
    assert div.sum() == 0
    got = split_rows(counts, groups)
    for i, t in enumerate(texts):
        assert got[i] == RR.captures_iter(o, t), t
    assert counts[4] >= 5


def test_capacity_and_empty_batch(cuda):
    import torch
    pat = r"(\w)(\d)?"
    re = R.Regex(pat)
    texts = std_texts(pat)
    counts, groups, _ = run_batch(re, texts, cuda)
    total = len(groups)
    assert total > 100 and counts.sum() == total
    for cap in (total - 1, total // 3, 1):
        c2, g2, _ = run_batch(re, texts, cuda, capacity=cap)
        assert np.array_equal(c2, counts) and c2.sum() == total   # the total is exact
        assert g2.shape == (cap, 3, 2) and np.array_equal(g2, groups[:cap])
    dev = torch.zeros(16, dtype=torch.uint8, device=cuda)
    c0, g0, d0 = re.captures_iter_batch(dev, stride=4, length=4, count=0)
    assert c0.shape == (0,) and g0.shape == (0, 3, 2) and d0.shape == (0,)
    c0, g0, d0 = R.Regex(r"a+").captures_iter_batch(dev, stride=4, length=4, count=0)
    assert c0.shape == (0,) and g0.shape == (0, 1, 2)
    # a start other than 0 is refused by the C entry
    b = R._batch(dev, None, 4, 4, 2, 1)
    tot = torch.zeros(1, dtype=torch.int64, device=cuda)
    cnt = torch.zeros(2, dtype=torch.int64, device=cuda)
    dv = torch.zeros(2, dtype=torch.uint8, device=cuda)
    assert N.rure_amd_captures_iter_batch(re._re, ctypes.byref(b), cnt.data_ptr(), None, 0, tot.data_ptr(),
                                          dv.data_ptr(), None) == N.ERR_ARG


def test_one_group_regex(cuda):
    """Two slots: the rows are the find_iter matches (no captures pass)."""
    pat = r"a+|\b"
    re = R.Regex(pat)
    texts = std_texts(pat)
    o = OracleRegex(re)
    counts, groups, div = run_batch(re, texts, cuda, resolve=False)
    assert div.sum() == 0
    got = split_rows(counts, groups)
    for i, t in enumerate(texts):
        assert got[i] == RR.captures_iter(o, t), t


REP_PATTERNS = [r"(\w)(\d)?", r"(a*)", r"(?P<y>\d+)-(?P<m>\d+)", r"\b", r"(a..$)|(a)"]
TEMPLATES = [b"<$1>", b"$2$1", b"${1}x$$", b"$0$0$0", b"", b"$nosuch", b"$y/$m"]
REP_ALPHA = [b"a", b"b", b"x", b"1", b"2", b"-", b" ", b"\n", "é".encode(), b"\xff"]


def rep_texts(pat):
    import random
    rng = random.Random(zlib.crc32(pat.encode()) ^ 0x5EED)
    return [b"".join(rng.choice(REP_ALPHA) for _ in range(rng.randint(0, 60))) for _ in range(300)]


@pytest.mark.parametrize("rep", TEMPLATES)
@pytest.mark.parametrize("pat", REP_PATTERNS)
def test_replace_expand_batch(cuda, pat, rep):
    import torch
    re = R.Regex(pat)
    names = re.capture_names()
    texts = rep_texts(pat)
    o = OracleRegex(re)
    buf, offs = ragged(texts)
    dbuf, doffs = torch.from_numpy(buf).to(cuda), torch.from_numpy(offs).to(cuda)
    for limit in (0, 1, 3):
        out, ooff = re.replace_batch(dbuf, rep, limit=limit, offsets=doffs, expand=True)
        if b"$" in rep and pat != r"(a..$)|(a)":   # (resolving runs the single-haystack path last)
            assert N.last_path() == Path.REPLACE_EXPAND
        out = out.cpu().numpy().tobytes()
        ooff = ooff.cpu().numpy()
        assert ooff[0] == 0 and ooff[-1] == len(out)
        for i, t in enumerate(texts):
            assert out[ooff[i]:ooff[i + 1]] == RR.replacen(o, names, t, limit, rep, False), (pat, t, rep, limit)


def test_expand_off_keeps_the_literal(cuda):
    import torch
    re = R.Regex(r"(\w)(\d)?")
    o = OracleRegex(re)
    texts = rep_texts(r"(\w)(\d)?")[:50]
    buf, offs = ragged(texts)
    dbuf, doffs = torch.from_numpy(buf).to(cuda), torch.from_numpy(offs).to(cuda)
    for kw, rep in (({}, b"$1"), ({"expand": False}, b"$1"), ({"expand": True}, R.NoExpand(b"$1")),
                    ({"expand": True}, b"no dollar")):
        out, ooff = re.replace_batch(dbuf, rep, offsets=doffs, **kw)
        assert N.last_path() != Path.REPLACE_EXPAND
        out, ooff = out.cpu().numpy().tobytes(), ooff.cpu().numpy()
        lit = rep.rep if isinstance(rep, R.NoExpand) else rep
        for i, t in enumerate(texts):
            assert out[ooff[i]:ooff[i + 1]] == RR.replacen(o, None, t, 0, lit, True), (t, rep)


def test_raw_result_flags(cuda):
    """resolve=False: the flags of a limited replace cover the first `limit`
    matches only, and unflagged haystacks are the reference's."""
    import torch
    pat = r"(a..$)|(a)"
    re = R.Regex(pat)
    names = re.capture_names()
    o = OracleRegex(re)
    texts = rep_texts(pat)
    caps, fi = oracle_rows(pat, "rep", texts)
    buf, offs = ragged(texts)
    dbuf, doffs = torch.from_numpy(buf).to(cuda), torch.from_numpy(offs).to(cuda)
    for limit in (0, 1):
        out, ooff, div = re.replace_batch(dbuf, b"[$1|$2]", limit=limit, offsets=doffs, expand=True, resolve=False)
        out, ooff, div = out.cpu().numpy().tobytes(), ooff.cpu().numpy(), div.cpu().numpy()
        k = limit or 1 << 30
        want = np.array([[c[0] for c in e][:k] != f[:k] for e, f in zip(caps, fi)])
        assert want.sum() > 10 and np.array_equal(div != 0, want)
        for i, t in enumerate(texts):
            if not want[i]:
                assert out[ooff[i]:ooff[i + 1]] == RR.replacen(o, names, t, limit, b"[$1|$2]", False), (t, limit)


def test_strided_long(cuda):
    """Fixed-stride long haystacks: the chunked find_iter feeds the captures
    pass, and the text between matches crosses the copy's unit edges."""
    import torch
    from regex_amd.workloads import date_haystacks_host
    n, L = 64, 1 << 16
    buf, _ = date_haystacks_host(n, L, seed=3, frac=0.5)
    re = R.Regex(r"(?P<y>\d{4})-(?P<m>\d{2})-(?P<d>\d{2})")
    o = OracleRegex(re)
    dbuf = torch.from_numpy(buf).to(cuda)
    re.find_iter_batch(dbuf, stride=L, length=L, count=n)
    assert N.last_path() in (Path.ITER_CHUNKED, Path.ITER_SHADOW_GATED, Path.ITER_SHADOW, Path.ITER_SHADOW_QUIT)   # chunked
    out, ooff = re.replace_batch(dbuf, b"$d/$m/$y", stride=L, length=L, count=n, expand=True)
    assert N.last_path() == Path.REPLACE_EXPAND
    out = out.cpu().numpy().tobytes()
    ooff = ooff.cpu().numpy()
    assert ooff[-1] == len(out) == n * L   # dd/mm/yyyy is as long as yyyy-mm-dd
    names = re.capture_names()
    for i in range(0, n, 7):
        t = bytes(buf[i * L:(i + 1) * L])
        assert out[ooff[i]:ooff[i + 1]] == RR.replacen(o, names, t, 0, b"$d/$m/$y", False), i


def test_one_long_haystack(cuda):
    """300 007 bytes (no multiple of the copy's unit) with a single match in
    the last 100 bytes, then without a match: the gap before the match and
    the tail are copied unit by unit."""
    import torch
    L = 300007
    text = bytearray(bytes(97 + (i * 7 + i // 251) % 26 for i in range(L)))
    p = L - 60
    text[p:p + 10] = b"2024-02-29"
    re = R.Regex(r"(\d{4})-(\d{2})-(\d{2})")
    for t, exp in ((bytes(text), bytes(text[:p]) + b"<29.02.2024>" + bytes(text[p + 10:])),
                   (bytes(text).replace(b"2024-02-29", b"2024x02y29"), None)):
        exp = t if exp is None else exp
        dbuf = torch.from_numpy(np.frombuffer(t + b"\0" * 16, dtype=np.uint8).copy()).to(cuda)
        out, ooff = re.replace_batch(dbuf, b"<$3.$2.$1>", stride=L, length=L, count=1, expand=True)
        assert ooff.cpu().tolist() == [0, len(exp)]
        assert out.cpu().numpy().tobytes() == exp
        # the same haystack in an offset batch, between two short ones
        offs = torch.tensor([0, 5, 5 + L - 5, L], dtype=torch.int64)
        out, ooff = re.replace_batch(dbuf, b"<$3.$2.$1>", offsets=offs.to(cuda), expand=True)
        assert ooff.cpu().tolist()[-1] == len(exp) and out.cpu().numpy().tobytes() == exp


def test_output_cut(cuda):
    """The C entry with a short output: the total is the need, the prefix is
    exact and nothing is written at or past out_capacity."""
    import torch
    pat = r"(\w)(\d)?"
    re = R.Regex(pat)
    texts = rep_texts(pat)
    buf, offs = ragged(texts)
    dbuf, doffs = torch.from_numpy(buf).to(cuda), torch.from_numpy(offs).to(cuda)
    rep = b"<$2$1>"
    full, foff = re.replace_batch(dbuf, rep, offsets=doffs, expand=True)
    full = full.cpu().numpy().tobytes()
    need = len(full)
    cap = need - 5
    out = torch.full((cap + 64,), 0xA5, dtype=torch.uint8, device=cuda)
    ooff = torch.zeros(len(texts) + 1, dtype=torch.int64, device=cuda)
    total = torch.zeros(1, dtype=torch.int64, device=cuda)
    div = torch.zeros(len(texts), dtype=torch.uint8, device=cuda)
    b = R._batch(dbuf, doffs)
    rc = N.rure_amd_replace_expand_batch(re._re, ctypes.byref(b), rep, len(rep), 0, out.data_ptr(), ooff.data_ptr(),
                                         cap, total.data_ptr(), div.data_ptr(),
                                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == N.OK
    assert int(total.item()) == need
    got = out.cpu().numpy().tobytes()
    assert got[:cap] == full[:cap]
    assert got[cap:] == b"\xa5" * 64
    assert np.array_equal(ooff.cpu().numpy(), foff.cpu().numpy())


@pytest.mark.parametrize("v", V["replace"], ids=[x["name"] for x in V["replace"]])
def test_golden_replace_vectors(cuda, v):
    import torch
    re = R.Regex(v["re"])
    text, rep = bytes.fromhex(v["text"]), bytes.fromhex(v["rep"])
    if v["mode"] == "literal":
        rep = R.NoExpand(rep)
    dbuf = torch.from_numpy(np.frombuffer(text + b"\0" * 16, dtype=np.uint8).copy()).to(cuda)
    out, ooff = re.replace_batch(dbuf, rep, limit=1 if v["which"] == "replace" else 0, stride=len(text),
                                 length=len(text), count=1, expand=True)
    assert out.cpu().numpy().tobytes() == bytes.fromhex(v["result"]), v["src"]
    assert ooff.cpu().tolist() == [0, len(out)]
