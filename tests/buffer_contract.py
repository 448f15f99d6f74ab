"""TEST INFRASTRUCTURE: the buffer contract of the batched calls
(include/rure_amd.h, "Outputs" and the haystack placement note at
rure_amd_batch), shared by tests/test_buffer_contract_cases.py (CPU: the
conditions on the inputs) and tests/test_gpu_buffer_contract.py (GPU).

  Arena       one uint8 buffer: front pad, the haystacks at any base
              misalignment and stride, back pad; every byte that is not a
              haystack byte holds a fill chosen to change the result of an
              engine that reads past a haystack's ends.
  raw_*       the ctypes entries called directly, with an output tensor that
              holds a sentinel in front of and behind the `capacity` rows the
              call may write, optionally 8- but not 16-byte aligned.
  CASES       one entry per find_iter engine: the pattern, knobs and text with
              which the existing test file of that engine reaches it.

Expected values come from the CPU oracle over the haystack bytes alone.

The recipes are imported from the engines' own test files; a rename there
has to be followed here (and in tests/test_gpu_buffer_contract.py):
  test_gpu_iter           _fb_text, _lex_text
  test_gpu_iter_looks     _text
  test_gpu_iter_wave      _text
  test_gpu_literals       texts
  test_gpu_shiftand       texts
  test_gpu_runs           sherlock
  test_gpu_suffix_iter    _text
  test_gpu_anchored       _texts
  test_gpu_iter_ragged    _dense_text, _slices
  test_gpu_split          _buf
  test_gpu_replace        _texts
  test_gpu_replace_class  text
  test_gpu_captures       _texts"""
import ctypes
import random
import zlib

import numpy as np

import regex_amd as R
from regex_amd import Path
from regex_amd import _native as N

FRONT = 64            # bytes in front of the first haystack's aligned slot
BACK = 64             # bytes behind the 16-byte-rounded end of the last haystack
GUARD = 64            # guard rows behind `capacity` rows; guard bytes behind `out_capacity`
SENT = 0xA5A5A5A5A5A5A5A5
SENT_I64 = SENT - (1 << 64)
FILLS = ("zero", "a", "c3", "nl", "self")
_FILL_BYTE = {"zero": 0x00, "a": 0x61, "c3": 0xC3, "nl": 0x0A}
KS = (0, 1, 8, 15)    # base misalignments


class Arena(object):
    """`hays` (equal lengths L) laid out at buf[FRONT + k + i * stride]; all
    other bytes hold `fill`:
      zero / a / c3 / nl   that byte everywhere (b"a" extends \\w+ runs and
                           literal matches, 0xC3 is a UTF-8 lead and a quit
                           byte of a Unicode \\b, b"\\n" ends a line);
      self                 the gap behind haystack i starts with haystack i's
                           first bytes again (a match cut by the haystack's
                           end would complete there) and the bytes in front of
                           the first haystack are the end of that haystack.
    The haystack bytes are written last: they are the same for every fill.
    Every aligned 16-byte block that overlaps a haystack lies inside the
    buffer (FRONT and BACK are multiples of 16 and the buffer's base is
    16-byte aligned: tensor() checks it)."""

    def __init__(self, hays, k=0, stride=None, fill="zero"):
        self.n, self.L = len(hays), len(hays[0])
        assert all(len(h) == self.L for h in hays) and self.L > 0
        self.S = self.L if stride is None else stride
        assert self.S >= self.L and 0 <= k < 16
        self.k, self.fill = k, fill
        self.begin = FRONT + k
        self.end = self.begin + (self.n - 1) * self.S + self.L
        size = ((self.end + 15) & ~15) + BACK
        hs = [np.frombuffer(h, dtype=np.uint8) for h in hays]
        if fill == "self":
            a = np.empty(size, dtype=np.uint8)
            a[:self.begin] = np.resize(hs[0], self.begin + self.L)[self.L - self.begin % self.L:][:self.begin] \
                if self.begin % self.L else np.resize(hs[0], self.begin)
            for i, h in enumerate(hs):
                g0 = self.begin + i * self.S + self.L
                g1 = self.begin + (i + 1) * self.S if i + 1 < self.n else size
                a[g0:g1] = np.resize(h, g1 - g0)
        else:
            a = np.full(size, _FILL_BYTE[fill], dtype=np.uint8)
        for i, h in enumerate(hs):
            a[self.begin + i * self.S:self.begin + i * self.S + self.L] = h
        self.host = a
        self._dev = {}

    def tensor(self, device="cpu"):
        import torch
        key = str(device)
        if key not in self._dev:
            t = torch.from_numpy(self.host.copy()).to(device)
            assert t.data_ptr() % 16 == 0
            self._dev[key] = t
        return self._dev[key]

    def hay(self, device="cpu"):
        """The view to pass as `haystack`: its byte 0 is haystack 0's."""
        return self.tensor(device)[self.begin:]

    def offsets(self, device="cpu"):
        """The same batch as an offset batch (needs stride == L)."""
        import torch
        assert self.S == self.L
        return torch.arange(0, (self.n + 1) * self.L, self.L, dtype=torch.int64).to(device)

    def read(self, i, device="cpu"):
        v = self.hay(device)[i * self.S:i * self.S + self.L]
        return bytes(v.cpu().numpy().tobytes())


# ------------------------------------------------------------- raw callers

class _Rows(object):
    """`capacity` rows of `words` int64 on the device between sentinels: one or
    two words in front (one: the rows start 8 bytes past a 16-byte boundary),
    GUARD rows behind.  null: the call gets NULL (capacity 0)."""

    def __init__(self, dev, capacity, words, off8=False, null=False):
        import torch
        assert not null or capacity == 0
        self.cap, self.w, self.front = capacity, words, 1 if off8 else 2
        self.t = torch.full((self.front + (capacity + GUARD) * words,), SENT_I64, dtype=torch.int64, device=dev)
        assert self.t.data_ptr() % 16 == 0
        self.ptr = None if null else ctypes.c_void_p(self.t.data_ptr() + 8 * self.front)
        assert null or (self.t.data_ptr() + 8 * self.front) % 16 == (8 if off8 else 0)

    def read(self, total):
        h = self.t.cpu().numpy()
        k = min(int(total), self.cap)
        body = h[self.front:self.front + k * self.w].reshape(k, self.w).copy()
        guard_ok = bool((h[:self.front] == SENT_I64).all() and (h[self.front + self.cap * self.w:] == SENT_I64).all())
        return body, guard_ok


class _Words(object):
    """n int64 words the call fills entirely (counts, total, exit), sentinels
    around them."""

    def __init__(self, dev, n):
        import torch
        self.n = n
        self.t = torch.full((2 + n + 8,), SENT_I64, dtype=torch.int64, device=dev)
        self.ptr = ctypes.c_void_p(self.t.data_ptr() + 16)

    def read(self):
        h = self.t.cpu().numpy()
        ok = bool((h[:2] == SENT_I64).all() and (h[2 + self.n:] == SENT_I64).all())
        return h[2:2 + self.n].copy(), ok


class Result(object):
    """counts, total, the first min(total, capacity) rows, and guard_ok: no
    word outside what the call may write was touched."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _sync():
    import torch
    torch.cuda.synchronize()


def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def raw_find_iter(re, hay, capacity, stride=None, length=None, count=None, offsets=None, start=0, off8=False,
                  null=False):
    b = R._batch(hay, offsets, stride, length, count, start)
    out = _Rows(hay.device, capacity, 2, off8, null)
    counts, total = _Words(hay.device, b.count), _Words(hay.device, 1)
    R._check(N.rure_amd_find_iter_batch(re._re, ctypes.byref(b), counts.ptr, out.ptr, capacity, total.ptr, None),
             "find_iter_batch")
    path = N.last_path()
    _sync()
    (c, ok1), (t, ok2) = counts.read(), total.read()
    rows, ok3 = out.read(t[0])
    return Result(counts=c, total=int(t[0]), rows=rows, guard_ok=ok1 and ok2 and ok3, path=path)


def raw_split(re, hay, limit, capacity, stride=None, length=None, count=None, offsets=None, off8=False):
    b = R._batch(hay, offsets, stride, length, count, 0)
    out = _Rows(hay.device, capacity, 2, off8)
    counts, total = _Words(hay.device, b.count), _Words(hay.device, 1)
    lim = (1 << 64) - 1 if limit is None else limit
    R._check(N.rure_amd_split_batch(re._re, ctypes.byref(b), lim, counts.ptr, out.ptr, capacity, total.ptr, None),
             "split_batch")
    _sync()
    (c, ok1), (t, ok2) = counts.read(), total.read()
    rows, ok3 = out.read(t[0])
    return Result(counts=c, total=int(t[0]), rows=rows, guard_ok=ok1 and ok2 and ok3)


def raw_captures_iter(re, hay, capacity, stride=None, length=None, count=None, offsets=None, off8=False):
    import torch
    b = R._batch(hay, offsets, stride, length, count, 0)
    out = _Rows(hay.device, capacity, 2 * re.captures_len(), off8)
    counts, total = _Words(hay.device, b.count), _Words(hay.device, 1)
    div = torch.full((b.count + 64,), 0xA5, dtype=torch.uint8, device=hay.device)
    R._check(N.rure_amd_captures_iter_batch(re._re, ctypes.byref(b), counts.ptr, out.ptr, capacity, total.ptr,
                                            _vp(div), None), "captures_iter_batch")
    _sync()
    (c, ok1), (t, ok2) = counts.read(), total.read()
    rows, ok3 = out.read(t[0])
    d = div.cpu().numpy()
    ok4 = bool((d[b.count:] == 0xA5).all())
    return Result(counts=c, total=int(t[0]), rows=rows, diverged=d[:b.count].copy(),
                  guard_ok=ok1 and ok2 and ok3 and ok4)


def raw_span(re, hay, length, lo, hi, capacity, entry=None, off8=False):
    """entry: None or the three int64 of a previous span's exit."""
    import torch
    out = _Rows(hay.device, capacity, 2, off8)
    count, exit_ = _Words(hay.device, 1), _Words(hay.device, 3)
    ent = None if entry is None else torch.tensor([int(x) for x in entry], dtype=torch.int64, device=hay.device)
    R._check(N.rure_amd_find_iter_span(re._re, _vp(hay), length, lo, hi, _vp(ent), count.ptr, out.ptr, capacity,
                                       exit_.ptr, None), "find_iter_span")
    _sync()
    (t, ok1), (x, ok2) = count.read(), exit_.read()
    rows, ok3 = out.read(t[0])
    return Result(total=int(t[0]), rows=rows, exit=x, guard_ok=ok1 and ok2 and ok3)


def raw_span_multi(res, hay, length, lo, hi, capacities, off8=False):
    k = len(res)
    outs = [_Rows(hay.device, c, 2, off8) for c in capacities]
    counts = [_Words(hay.device, 1) for _ in res]
    exits = [_Words(hay.device, 3) for _ in res]
    VP = ctypes.c_void_p
    R._check(N.rure_amd_find_iter_span_multi((VP * k)(*[r._re for r in res]), k, _vp(hay), length, lo, hi, None,
                                             (VP * k)(*[c.ptr for c in counts]), (VP * k)(*[o.ptr for o in outs]),
                                             (ctypes.c_size_t * k)(*capacities), (VP * k)(*[x.ptr for x in exits]),
                                             None), "find_iter_span_multi")
    _sync()
    rs = []
    for i in range(k):
        (t, ok1), (x, ok2) = counts[i].read(), exits[i].read()
        rows, ok3 = outs[i].read(t[0])
        rs.append(Result(total=int(t[0]), rows=rows, exit=x, guard_ok=ok1 and ok2 and ok3))
    return rs


def raw_compact(found, base, capacity, off8=False):
    out = _Rows(found.device, capacity, 3, off8)
    count = _Words(found.device, 1)
    rc = N.rure_amd_compact_matches(_vp(found), found.shape[0], base, out.ptr, capacity, count.ptr, None)
    assert rc == N.OK
    _sync()
    t, ok1 = count.read()
    rows, ok2 = out.read(t[0])
    return Result(total=int(t[0]), rows=rows, guard_ok=ok1 and ok2)


def raw_replace(re, hay, rep, limit, out_capacity, stride=None, length=None, count=None, offsets=None, expand=False,
                shift=0):
    """rure_amd_replace_batch / _replace_expand_batch into out_capacity bytes
    that start 16 + shift bytes into a tensor of sentinel bytes which ends
    GUARD bytes behind them (no slack).  Returns rc too: nothing is read
    back when the call refused its arguments."""
    import torch
    b = R._batch(hay, offsets, stride, length, count, 0)
    buf = torch.full((16 + shift + out_capacity + GUARD,), 0xA5, dtype=torch.uint8, device=hay.device)
    assert buf.data_ptr() % 16 == 0
    out = ctypes.c_void_p(buf.data_ptr() + 16 + shift)
    ooff, total = _Words(hay.device, b.count + 1), _Words(hay.device, 1)
    if expand:
        div = torch.zeros((b.count + 1,), dtype=torch.uint8, device=hay.device)
        rc = N.rure_amd_replace_expand_batch(re._re, ctypes.byref(b), rep, len(rep), limit, out, ooff.ptr,
                                             out_capacity, total.ptr, _vp(div), None)
    else:
        rc = N.rure_amd_replace_batch(re._re, ctypes.byref(b), rep, len(rep), limit, out, ooff.ptr, out_capacity,
                                      total.ptr, None)
        div = None
    path = N.last_path()
    _sync()
    h = buf.cpu().numpy()
    untouched = bool((h == 0xA5).all())
    if rc != N.OK:
        return Result(rc=rc, untouched=untouched)
    (oo, ok1), (t, ok2) = ooff.read(), total.read()
    k = min(int(t[0]), out_capacity)
    o0 = 16 + shift
    guard_ok = bool((h[:o0] == 0xA5).all() and (h[o0 + out_capacity:] == 0xA5).all())
    return Result(rc=rc, out_offsets=oo, total=int(t[0]), out=h[o0:o0 + k].tobytes(), guard_ok=ok1 and ok2 and guard_ok,
                  diverged=None if div is None else div.cpu().numpy()[:b.count], path=path, untouched=untouched)


# -------------------------------------------------------------- case table

class Case(object):
    """One find_iter engine.  text(): the flat text, cut into `count`
    haystacks of L bytes (L % 16 == 0) at i * L.  unit: the bytes per unit of
    the engine under these knobs (None: one unit per haystack).  kind: "lex"
    / "run" for the engines with a record window (kGrpWin, kRunWin).  path:
    the Paths the aligned zero-fill layout may report, None where Path does
    not tell the engine apart.  dense: a unit can hold more than 4 records."""

    def __init__(self, name, pat, text, L, count=1, knobs=None, unit=None, kind=None, path=None, start=0,
                 dense=True, ragged=False):
        self.name, self.pat, self.text, self.L, self.count = name, pat, text, L, count
        self.knobs, self.unit, self.kind, self.path, self.start = knobs or {}, unit, kind, path, start
        self.dense, self.ragged = dense, ragged
        assert L % 16 == 0

    def hays(self, L=None):
        L = self.L if L is None else L
        t = self.text()
        assert len(t) >= self.count * self.L, (self.name, len(t))
        return [t[i * self.L:i * self.L + L] for i in range(self.count)]


def _seed(pat):
    return zlib.crc32(pat.encode())


def _memo(f):
    box = []

    def g():
        if not box:
            box.append(f())
        return box[0]
    return g


# (the text recipes of the engines' own test files, imported where they are
# functions and restated where they are inline)
def _fb(pat, n):
    def f():
        from test_gpu_iter import _fb_text
        return _fb_text(_seed(pat), n, True)
    return _memo(f)


def _lex(pat, n):
    def f():
        from test_gpu_iter import _lex_text
        return _lex_text(_seed(pat), n, True)
    return _memo(f)


def _looks(pat, n, nonascii, salt=0):
    def f():
        from test_gpu_iter_looks import _text
        return _text(_seed(pat) + salt, n, nonascii)
    return _memo(f)


def _wave(pat, n, every):
    def f():
        from test_gpu_iter_wave import _text
        return _text(_seed(pat) + 7 + every, n, every)
    return _memo(f)


def _lit(pat, n):
    def f():
        from test_gpu_literals import texts
        return list(texts(pat))[3][:n]
    return _memo(f)


def _sa(pat, n):
    def f():
        from test_gpu_shiftand import texts
        return list(texts(pat))[3][:n]
    return _memo(f)


def _runs_text():
    """test_gpu_runs: sherlock made ASCII (a dozen KiB: units with hundreds
    of runs) around a run that covers two whole 4 KiB units."""
    from test_gpu_runs import sherlock
    t = bytes(b if b < 0x80 else 0x20 for b in sherlock()[:20480])
    return t[:12288] + b" " + b"a" * 9000 + b" " + t[12288:12288 + 4102]


def _runs_text_unicode():
    """test_gpu_runs.test_runs_non_ascii's alphabet (the Unicode class reads
    UTF-8) in front of the same long run."""
    rng = random.Random(3)
    alpha = [b"ab", b"Z9", b" ", b"\n", "é".encode(), "✓".encode(), b"\xff", "٣".encode(), b"x_y"]
    t = b"".join(rng.choices(alpha, k=9000))
    return t[:12288] + b" " + b"a" * 9000 + b" " + t[12288:12288 + 4102]


def _suffix_text():
    from test_gpu_suffix_iter import _text
    return b"".join(_text(9008, 50 + i) for i in range(3))


def _anchored_text():
    from test_gpu_anchored import _texts
    return b"".join(_texts(3000, 7))


def multi_text():
    """test_gpu_multi.test_multi_engines_mixed_bytes, a twentieth of it."""
    rng = np.random.default_rng(11)
    motifs = [b"agggtaaa", b"tttaccct", b"cgggtaaa", b"tttacccg", b"aggggtaa", b"ggtaaaTT", b"AGGGTAAA"]
    noise = np.frombuffer(b"acgtacgtACGTnNBDHKMRSVWY\n\x80\xff\xc3\xa9", dtype=np.uint8)
    parts = [motifs[int(i)] if rng.random() < 0.4 else bytes(rng.choice(noise, size=int(rng.integers(1, 12))))
             for i in rng.integers(0, len(motifs), size=7500)]
    return b"".join(parts)


MULTI_PATS = [r"agggtaaa|tttaccct", r"[cgt]gggtaaa|tttaccc[acg]", r"a[act]ggtaaa|tttacc[agt]t"]

_WAVE_PAT, _LOOKS_PAT, _LEX_A, _LEX_B = r"\b\w+n\b", r"(?-u)\b[a-c]+\b", r">[^\n]*\n|\n", r"a[^b]*b"
_SHADOW = r"\w+\s+\w+"
_CHUNKED = (Path.ITER_CHUNKED,)

CASES = [
    # the burst kernel over the full automaton (first-byte rule), cut into 16- and 128-byte units
    Case("burst", r"a(b|cd)*e?", _fb(r"a(b|cd)*e?", 16384), 4096, 4, {"iter_chunk": 16}, 16, path=_CHUNKED),
    Case("burst_dot", r"(?s)a.*b|c", _fb(r"(?s)a.*b|c", 16384), 16384, 1, {"iter_chunk": 128}, 128, path=_CHUNKED),
    # Unicode classes: the ASCII shadow gated on the device, and read back (answered / quit)
    Case("shadow_gated", _SHADOW, _looks(_SHADOW, 16384, False, 5), 8192, 2, {"iter_chunk": 30}, 30,
         path=(Path.ITER_SHADOW_GATED,)),
    Case("shadow_sync", _SHADOW, _looks(_SHADOW, 16384, False, 5), 8192, 2, {"iter_chunk": 30, "shadow_sync": 1}, 30,
         path=(Path.ITER_SHADOW,)),
    Case("shadow_quit", _SHADOW, _looks(_SHADOW, 16384, True, 5), 8192, 2, {"iter_chunk": 30, "shadow_sync": 1}, 30,
         path=(Path.ITER_SHADOW_QUIT,)),
    # the lexer: four bytes per step and byte per step, one haystack and several
    Case("lex4_one", _LEX_A, _lex(_LEX_A, 262144), 262144, 1, {"iter_chunk": 128}, 128, "lex", _CHUNKED),
    Case("lex4_many", _LEX_B, _lex(_LEX_B, 262144), 65536, 4, {"iter_chunk": 128}, 128, "lex", _CHUNKED),
    Case("lex1_one", _LEX_B, _lex(_LEX_B, 262144), 262144, 1, {"iter_chunk": 128, "lex4": 0}, 128, "lex", _CHUNKED),
    Case("lex1_many", _LEX_A, _lex(_LEX_A, 262144), 65536, 4, {"iter_chunk": 128, "lex4": 0}, 128, "lex", _CHUNKED),
    # string sets: the literal engine, Shift-And (tile kernel by default, per lane with sa=2)
    Case("literal", r"a|ab", _lit(r"a|ab", 16384), 4096, 4, {"lit": 1, "iter_chunk": 16}, 16,
         path=_CHUNKED),
    Case("shiftand_tile", r"agggtaaa|tttaccct", _sa(r"agggtaaa|tttaccct", 32768), 8192, 4, {"iter_chunk": 128}, 128,
         path=_CHUNKED),
    Case("shiftand_lane", r"agggtaaa|tttaccct", _sa(r"agggtaaa|tttaccct", 32768), 8192, 4,
         {"iter_chunk": 128, "sa": 2}, 128, path=_CHUNKED),
    # C+: the run engine, a byte class and a Unicode class read as UTF-8 (ITER_RUNS_ASCII, the run engine with
    # the ASCII shadow's class alone, is not listed: no regex of the suite has a run class in its shadow only)
    Case("runs", r"[a-z]+", _memo(_runs_text), 25392, 1, {}, 4096, "run", (Path.ITER_RUNS,)),
    Case("runs_unicode", r"\w+", _memo(_runs_text_unicode), 25392, 1, {}, 4096, "run", (Path.ITER_RUNS,)),
    # look-around: chunked; Unicode \b with non-ASCII text served by waves, or sent to the wave path
    Case("looks", _LOOKS_PAT, _looks(_LOOKS_PAT, 6000 * 3, False, 2), 5984, 3, {"iter_chunk": 61}, 61,
         path=(Path.ITER_LOOKS,)),
    Case("wave_served", _WAVE_PAT, _wave(_WAVE_PAT, 6000 * 3, 40), 5984, 3, {"iter_chunk": 61}, 61,
         path=(Path.ITER_WAVE_SERVED,)),
    Case("looks_quit", _WAVE_PAT, _wave(_WAVE_PAT, 6000 * 3, 40), 5984, 3, {"iter_chunk": 61, "iter_wave": 0}, 61,
         path=(Path.ITER_LOOKS_QUIT,)),
    # one wave per haystack: a look-around regex kept off the chunked path, and a Literal match type
    Case("wave", r"\bthe\b", _wave(r"\bthe\b", 192 * 96, 40), 192, 96, {"iter_looks": 0}, None, path=(Path.ITER_WAVE,)),
    Case("wave_literal", r"then|the", _wave(r"then|the", 192 * 96, 0), 192, 96, {}, None, path=None),
    # DfaSuffix in 128-byte units
    Case("suffix_iter", r"[a-z]+ing", _memo(_suffix_text), 9008, 3, {"suffix_iter": 2}, 128, path=(Path.SUFFIX_ITER,)),
    # end-anchored, searched from start > 0: at most the find result per haystack
    Case("anchored_rev", r"\d$", _memo(_anchored_text), 48, 512, {}, None, path=None, start=3, dense=False),
    # an offset batch cut into 64-byte units by the haystacks' own lengths
    Case("ragged", r"[A-Za-z]+ [a-z]+", None, 16, 0, {"iter_ragged": 2, "iter_chunk": 64}, 64,
         path=_CHUNKED, ragged=True),
]
CASE_BY_NAME = {c.name: c for c in CASES}
FIXED = [c for c in CASES if not c.ragged]


@_memo
def ragged_texts():
    """test_gpu_iter_ragged: windows around the matches of the ragged case's
    pattern (one of test_geometry_edges') in sherlock (_dense_text), cut into
    haystacks of 0..600 bytes, a few of them empty, with cuts forced inside
    matches (_slices)."""
    from golden_data import corpus
    from test_gpu_iter_ragged import _dense_text, _slices
    from oracle_py import OracleRegex
    o = OracleRegex(R.Regex(CASE_BY_NAME["ragged"].pat))
    rng = np.random.default_rng(41)
    text = _dense_text(o, corpus("sherlock")[:200000], 24000, rng)
    hs, _ = _slices(o, text, 80, rng)
    return hs


# ---------------------------------------------------------------- expected

_exp = {}


def oracle_rows(o, hays, start=0):
    """(counts int64 (n,), rows int64 (T, 2)) of find_iter per haystack."""
    per = [o.find_iter_array(h, start).astype(np.int64) for h in hays]
    counts = np.array([len(p) for p in per], dtype=np.int64)
    rows = np.concatenate(per) if per else np.zeros((0, 2), dtype=np.int64)
    return counts, rows.reshape(-1, 2)


def expected(case, L=None):
    """The oracle's find_iter of the case's haystacks cut to L bytes, from
    the haystack bytes alone; computed once."""
    from oracle_py import OracleRegex
    L = case.L if L is None else L
    key = (case.name, L)
    if key not in _exp:
        o = OracleRegex(R.Regex(case.pat))
        hays = ragged_texts() if case.ragged else case.hays(L)
        _exp[key] = (hays,) + oracle_rows(o, hays, case.start)
    return _exp[key]


def unit_counts(case, hays, counts, rows):
    """Records per unit, in output order (units of case.unit bytes from
    `start` within each haystack; one unit per haystack if unit is None)."""
    out, k = [], 0
    for h, c in zip(hays, counts):
        r = rows[k:k + c, 0]
        k += c
        if case.unit is None:
            out.append(int(c))
            continue
        span = max(0, len(h) - case.start)
        nu = max(1, -(-span // case.unit))
        idx = np.minimum((r - case.start) // case.unit, nu - 1)
        out += np.bincount(idx, minlength=nu).tolist()
    return out


def cut_points(case, hays, counts, rows):
    """Issue (a): the capacities at which a cut can go wrong."""
    T = int(counts.sum())
    pts = {0, 1, 4, 5, T // 2, T - 1, T, T + 1}
    uc = np.cumsum([0] + unit_counts(case, hays, counts, rows))
    for j in (len(uc) // 3, 2 * len(uc) // 3):  # records before two unit boundaries
        pts |= {int(uc[j]) - 1, int(uc[j]), int(uc[j]) + 1}
    if case.kind == "run":
        pts |= {255, 256, 257}
    if case.kind == "lex":
        pts |= {4095, 4096, 4097}
    return sorted(p for p in pts if p >= 0)


class RaggedArena(object):
    """An offset batch: the texts back to back behind FRONT + k bytes, BACK
    bytes behind the 16-byte-rounded end; the pads hold `fill` (self: the
    end of the first text in front, the beginning of the last one behind)."""

    def __init__(self, texts, k=0, fill="zero"):
        body = np.frombuffer(b"".join(texts), dtype=np.uint8)
        self.texts, self.k, self.begin = texts, k, FRONT + k
        self.end = self.begin + len(body)
        size = ((self.end + 15) & ~15) + BACK
        if fill == "self":
            a = np.empty(size, dtype=np.uint8)
            first = np.frombuffer(next(t for t in texts if t), dtype=np.uint8)
            last = np.frombuffer(next(t for t in reversed(texts) if t), dtype=np.uint8)
            a[:self.begin] = np.resize(first[::-1], self.begin)[::-1]
            a[self.end:] = np.resize(last, size - self.end)
        else:
            a = np.full(size, _FILL_BYTE[fill], dtype=np.uint8)
        a[self.begin:self.end] = body
        self.host = a
        self.offs = np.zeros(len(texts) + 1, dtype=np.int64)
        self.offs[1:] = np.cumsum([len(t) for t in texts])

    def hay(self, device):
        import torch
        t = torch.from_numpy(self.host.copy()).to(device)
        assert t.data_ptr() % 16 == 0
        return t[self.begin:]

    def offsets(self, device):
        import torch
        return torch.from_numpy(self.offs.copy()).to(device)


# ------------------------------------------- references of the other producers

def split_spans(ms, n, limit):
    """The fields of split (limit None) / splitn over a text of n bytes with
    find_iter matches ms, as (start, end): re_bytes.rs:699-749, the iterators
    of tests/replace_ref.py yielding offsets instead of bytes."""
    it, last, out = iter(ms), 0, []

    def nxt():
        nonlocal last
        m = next(it, None)
        if m is None:
            if last >= n:
                return None
            f, last = (last, n), n
            return f
        f, last = (last, m[0]), m[1]
        return f

    if limit is None:
        while True:
            f = nxt()
            if f is None:
                return out
            out.append(f)
    k = limit
    while k:
        k -= 1
        if k == 0:
            out.append((last, n))
            break
        f = nxt()
        if f is None:
            break
        out.append(f)
    return out


def replace_marked(text, spans, reps, limit):
    """replacen's output and, per output byte, whether it comes from a
    replacement: spans = the matches, reps[j] = match j's replacement."""
    if limit:
        spans = spans[:limit]
    out, mark, last = bytearray(), bytearray(), 0
    for (s, e), r in zip(spans, reps):
        out += text[last:s] + r
        mark += b"\0" * (s - last) + b"\1" * len(r)
        last = e
    out += text[last:]
    mark += b"\0" * (len(text) - last)
    return bytes(out), bytes(mark)


def byte_cut_points(total, mark):
    """Issue (f): out_capacity values, with one inside a replacement and one
    inside a 16-byte block that is copied text only."""
    pts = {0, 1, 15, 16, 17, total - 1, total, total + 1}
    m = np.frombuffer(mark, dtype=np.uint8)
    inside = np.nonzero(m[1:] & m[:-1])[0]
    assert inside.size, "no replacement of two bytes"
    pts.add(int(inside[len(inside) // 2]) + 1)
    blocks = [p for p in range(16, len(m) - 16, 16) if not m[p:p + 16].any()]
    assert blocks, "no block of copied text"
    pts.add(blocks[len(blocks) // 2] + 7)
    return sorted(p for p in pts if p >= 0)
