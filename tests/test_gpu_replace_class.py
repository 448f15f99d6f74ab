"""replace_all of a one-byte-class regex on the GPU without a match list
(replace_scan.hip launch_replace_class, Path.REPLACE_CLASS) against the
oracle's find_iter + the reference's replacen rule (re_bytes.rs:489-512):
sparse, dense and all-class text, replacements of 1 to 64 bytes, lengths
around the 64-byte lane and 4 KiB unit edges, an output buffer smaller than
the result (the call reports the length, the retry writes it), and the
regex-dna IUB substitutions chained (their known output length)."""
import ctypes
import functools
import random

import numpy as np
import pytest

import chain_ref
import regex_amd as R
from regex_amd import Path
from regex_amd import _native as N
from oracle_py import OracleRegex

pytestmark = pytest.mark.gpu


def dev(t, cuda):
    import torch
    return torch.from_numpy(np.frombuffer(t + b"\0" * 16, dtype=np.uint8).copy()).to(cuda)


def expect(re, t, rep):
    out, last = bytearray(), 0
    for s, e in OracleRegex(re).find_iter(t):
        out += t[last:s] + rep
        last = e
    return bytes(out + t[last:])


def text(seed, n, alpha):
    rng = random.Random(seed)
    return bytes(rng.choice(alpha) for _ in range(n))


CASES = [(r"B", b"acgtB"), (r"[KM]", b"acgtacgtacgtKM"), (r"x", b"x"), (r"[a-c]", b"abcdefgh \n"),
         (r"(?-u)\xff", b"a\xff\xfe"), (r"(?s-u:.)", b"ab\n")]


@pytest.mark.parametrize("pat,alpha", CASES)
@pytest.mark.parametrize("n", [0, 1, 15, 63, 64, 65, 4095, 4096, 4097, 70001])
@pytest.mark.parametrize("rep", [b"Z", b"(c|g|t)", b"<" + b"r" * 62 + b">"])
def test_replace_class(cuda, pat, alpha, n, rep):
    re = R.Regex(pat)
    t = text(n * 7 + len(rep), n, alpha)
    out, ooff = re.replace_batch(dev(t, cuda), rep, stride=max(n, 1), length=n, count=1)
    if n:
        assert N.last_path() == Path.REPLACE_CLASS
    assert bytes(out.cpu().numpy()) == expect(re, t, rep), (pat, n, rep)
    assert ooff.cpu().numpy().tolist() == [0, len(expect(re, t, rep))]


def test_replace_class_small_buffer(cuda):
    """An output buffer shorter than the result: *total is the length and no
    byte past the capacity is written."""
    import torch
    re = R.Regex(r"[KM]")
    t = text(5, 50000, b"acgtKM")
    exp = expect(re, t, b"(a|c)")
    d = dev(t, cuda)
    b = R._batch(d, None, len(t), len(t), 1, 0)
    cap = len(exp) // 3
    out = torch.full((cap + 64,), 0xAB, dtype=torch.uint8, device=cuda)
    ooff = torch.empty(2, dtype=torch.int64, device=cuda)
    total = torch.zeros(1, dtype=torch.int64, device=cuda)
    rc = N.rure_amd_replace_batch(re._re, ctypes.byref(b), b"(a|c)", 5, 0, ctypes.c_void_p(out.data_ptr()),
                                  ctypes.c_void_p(ooff.data_ptr()), cap, ctypes.c_void_p(total.data_ptr()),
                                  R._stream_ptr(None))
    assert rc == N.OK
    torch.cuda.synchronize()
    assert int(total.item()) == len(exp)
    got = out.cpu().numpy()
    assert bytes(got[:cap]) == exp[:cap]
    assert (got[cap:] == 0xAB).all()


def test_iub_chain_known_length(cuda):
    """The 11 IUB substitutions of the regex-dna shootout chained over the
    stripped input: the output length the reference prints."""
    from golden_data import corpus, known_counts
    from regex_amd import shootout
    kc = known_counts()["regexdna"]
    raw = corpus("regexdna")
    strip = R.Regex(shootout.STRIP.decode())
    seq = strip.replace_all(raw, b"")
    cur = dev(seq, cuda)
    n = len(seq)
    for p, rep in shootout.SUBSTS:
        re = R.Regex(p.decode())
        out, ooff = re.replace_batch(cur, rep, stride=n, length=n, count=1)
        assert N.last_path() == Path.REPLACE_CLASS
        n = int(ooff[1].item())
        import torch
        cur = torch.cat([out[:n], torch.zeros(16, dtype=torch.uint8, device=cuda)])
    assert n == kc["substituted_len"], (n, kc["substituted_len"])


def chain_expect(steps, t):
    for re, rep in steps:
        t = expect(re, t, rep)
    return t


# (pattern, replacement) per step; tests/chain_ref.py holds them with their byte sets
CHAINS = [[(p, rep) for p, _, rep in c] for c in chain_ref.CHAINS]


@pytest.mark.parametrize("seq", [0, 1])
@pytest.mark.parametrize("ci", range(len(CHAINS)))
@pytest.mark.parametrize("n", [0, 1, 63, 4096, 4097, 70001, 300007])
def test_replace_chain(cuda, knobs, seq, ci, n):
    """rure_amd_replace_all_chain against the host rule applied step by step:
    the same bytes and every intermediate length — as one composed byte map
    (default, REPLACE_HMAP) and step by step (knob chain_seq=1, REPLACE_CLASS)."""
    if seq:
        knobs(chain_seq=1)
    steps = [(R.Regex(p), rep) for p, rep in CHAINS[ci]]
    alpha = b"acgtBDNKMxy\xff\xfe<>Q\n"
    t = text(ci * 1000 + n, n, alpha)
    out, lengths = R.replace_all_chain([r for r, _ in steps], [rep for _, rep in steps], dev(t, cuda), length=n,
                                       capacity=16 * n + 4096)
    exp, lens = t, [n]
    for re, rep in steps:
        exp = expect(re, exp, rep)
        lens.append(len(exp))
    assert lengths.cpu().numpy().tolist() == lens
    assert bytes(out[:lens[-1]].cpu().numpy()) == exp
    if n:
        assert N.last_path() == (Path.REPLACE_CLASS if seq else Path.REPLACE_HMAP)


CUT_STEPS = [(r"x", chain_ref.lit(b"x"), b"x" * 40), (r"y", chain_ref.lit(b"y"), b"yy"),
             (r"z", chain_ref.lit(b"z"), b"zzz")]


@functools.lru_cache(maxsize=None)
def cut_texts():
    """The cut tests' text and its true text after every step."""
    return chain_ref.apply_chain(CUT_STEPS, text(5, 20000, b"xyz "))


def cut_lengths(steps, texts, cap, seq):
    """The lengths a chain reports with `cap` bytes per buffer.  As one byte
    map they come from the input's histogram: exact whatever is cut.  Step by
    step, a step reads at most the cap bytes its input buffer holds: the
    first step to overflow still reports its whole length, a step whose input
    was cut the length of what it makes of those cap bytes."""
    if not seq:
        return [len(x) for x in texts]
    return [len(texts[0])] + [len(chain_ref.apply_step(texts[i][:cap], cset, rep))
                              for i, (_, cset, rep) in enumerate(steps)]


@pytest.mark.parametrize("seq", [0, 1])
def test_replace_chain_cut(cuda, knobs, seq):
    """A capacity below an intermediate length: every length is what
    cut_lengths says (exact as one byte map; step by step the cut step's is
    exact and the later ones are those of the cut input), some length exceeds
    the capacity, and the caller retries with the largest until the chain
    fits."""
    if seq:
        knobs(chain_seq=1)
    steps = [(R.Regex(p), rep) for p, _, rep in CUT_STEPS]
    exps = cut_texts()
    t = exps[0]
    cap, tries = len(t) + 100, 0
    while True:
        out, lengths = R.replace_all_chain([r for r, _ in steps], [rep for _, rep in steps], dev(t, cuda),
                                           length=len(t), capacity=cap)
        ln = lengths.cpu().numpy().tolist()
        tries += 1
        assert ln[0] == len(t) and ln[1] == len(exps[1])
        assert ln == cut_lengths(CUT_STEPS, exps, cap, seq), (cap, ln)
        # after a cut input: more than the capacity, at most the true length
        assert all(cap < ln[i] <= len(exps[i]) for i in (2, 3) if len(exps[i - 1]) > cap)
        if max(ln) <= cap:
            break
        cap = max(ln)
    assert 2 <= tries <= 4
    assert ln == [len(x) for x in exps]
    assert bytes(out[:ln[3]].cpu().numpy()) == exps[3]


def test_replace_chain_rejects(cuda):
    """A regex whose matches are not single class bytes is refused."""
    with pytest.raises(Exception):
        R.replace_all_chain([R.Regex(r"ab")], [b"x"], dev(b"abab", cuda), length=4)


def test_replace_chain_long_images(cuda):
    """Images longer than 64 bytes after composition (x -> 40 x, then each x
    -> 2 x): the call runs the chain step by step (REPLACE_CLASS), same bytes."""
    steps = [(R.Regex(r"x"), b"x" * 40), (R.Regex(r"x"), b"xx")]
    t = text(9, 5000, b"xab")
    out, lengths = R.replace_all_chain([r for r, _ in steps], [rep for _, rep in steps], dev(t, cuda), length=len(t),
                                       capacity=100 * len(t))
    assert N.last_path() == Path.REPLACE_CLASS
    exp = chain_expect(steps, t)
    assert int(lengths[-1]) == len(exp)
    assert bytes(out[:len(exp)].cpu().numpy()) == exp


# ------------------------------------------------------------------
# The limits of the composed byte map (chain_ref.LIMITS), on both engines.

LIMIT_NS = [1, 63, 4096, 4097, 70001]


@functools.lru_cache(maxsize=None)
def limit_case(name, n):
    """(text, its true text after every step): random bytes over all 256
    values with 0xFF, 0x00 and each class's first and last byte planted (as
    many of them as n holds); computed once per (chain, n)."""
    steps = chain_ref.LIMITS[name][0]
    must = [0xFF, 0x00] + [b for _, cset, _ in steps for b in (min(cset), max(cset))]
    must = list(dict.fromkeys(must))[:n]
    rng = random.Random("%s/%d" % (name, n))
    t = bytearray(rng.randrange(256) for _ in range(n))
    for pos, b in zip(rng.sample(range(n), len(must)), must):
        t[pos] = b
    return bytes(t), chain_ref.apply_chain(steps, bytes(t))


def run_chain(steps, t, cuda, capacity):
    """(the result buffer as bytes, lengths) of R.replace_all_chain."""
    out, lengths = R.replace_all_chain([R.Regex(p) for p, _, _ in steps], [rep for _, _, rep in steps], dev(t, cuda),
                                       length=len(t), capacity=capacity)
    return bytes(out.cpu().numpy()), lengths.cpu().numpy().tolist()


@pytest.mark.parametrize("seq", [0, 1])
@pytest.mark.parametrize("n", LIMIT_NS)
@pytest.mark.parametrize("name", sorted(chain_ref.LIMITS))
def test_chain_map_limits(cuda, knobs, name, n, seq):
    """Each chain at a limit of the byte map against the byte-set rule: the
    final bytes, every intermediate length, and the engine — REPLACE_HMAP
    where the chain is mappable (255 changed byte values, 16 / 17 / 154 of
    them for the count kernel's two histograms, a pool of exactly 4096, an
    image of exactly 64), the step-by-step fallback just past each limit (256
    changed values, a pool of 4160, an image of 66) and under chain_seq=1."""
    if seq:
        knobs(chain_seq=1)
    steps, mappable = chain_ref.LIMITS[name][:2]
    t, texts = limit_case(name, n)
    if name == "all256":
        assert texts[-1] == b"xx" * n
    got, lengths = run_chain(steps, t, cuda, len(texts[-1]) + 32)
    print("%s n=%d seq=%d lengths=%r want=%r path=%s bytes right=%s" % (
        name, n, seq, lengths, [len(x) for x in texts], N.last_path().name, got[:len(texts[-1])] == texts[-1]))
    assert lengths == [len(x) for x in texts], name
    assert got[:len(texts[-1])] == texts[-1], name
    assert N.last_path() == (Path.REPLACE_HMAP if mappable and not seq else Path.REPLACE_CLASS)


@pytest.mark.parametrize("seq", [0, 1])
@pytest.mark.parametrize("name", ["c154", "c17"])
def test_chain_tight_capacity(cuda, knobs, name, seq):
    """A capacity of exactly the result holds all of it; one byte less, and
    lengths[-1] == capacity + 1 says so, the bytes that fit are right and
    every length is still exact (only the last step's output is cut)."""
    if seq:
        knobs(chain_seq=1)
    steps = chain_ref.LIMITS[name][0]
    t, texts = limit_case(name, 4097)
    lens = [len(x) for x in texts]
    assert lens[-2] < lens[-1]
    got, lengths = run_chain(steps, t, cuda, lens[-1])
    assert lengths == lens and got[:lens[-1]] == texts[-1]
    cap = lens[-1] - 1
    got, lengths = run_chain(steps, t, cuda, cap)
    assert lengths == lens and lengths[-1] == cap + 1
    assert got[:cap] == texts[-1][:cap]
    assert got[cap:] == b"\0" * 16  # (the wrapper's zeroed tail)


# ------------------------------------------------------------------
# The entry point called directly, over buffers the test lays out itself.

def chain_args(steps):
    """(keep-alive, res, reps, rep_lens) for N.rure_amd_replace_all_chain"""
    n = len(steps)
    regs = [R.Regex(p) for p, _, _ in steps]
    bufs = [ctypes.create_string_buffer(rep, max(len(rep), 1)) for _, _, rep in steps]
    res = (ctypes.c_void_p * max(n, 1))(*[r._re for r in regs])
    reps = (ctypes.c_void_p * max(n, 1))(*[ctypes.addressof(b) for b in bufs])
    lens = (ctypes.c_size_t * max(n, 1))(*[len(rep) for _, _, rep in steps])
    return (regs, bufs), res, reps, lens


GUARD = 8192


def cut_capacities():
    """(capacity, the step whose output is the first to be cut): every
    residue of 4096 the unit rounding can meet (just past a unit edge, mid
    unit, just before the edge, on it), cut first in step 1 and in step 2."""
    lens = [len(x) for x in cut_texts()]
    caps = []
    for r in (1, 2049, 4095, 0):
        caps.append((lens[1] // 2 // 4096 * 4096 + r, 1))
        c2 = (lens[1] + 4095 - r) // 4096 * 4096 + r  # the first capacity >= lens[1] with this residue
        assert lens[1] <= c2 < lens[2]
        caps.append((c2, 2))
    assert all(lens[0] < c for c, _ in caps) and any(c % 16 for c, _ in caps)
    return caps


@pytest.mark.parametrize("seq", [0, 1])
@pytest.mark.parametrize("cap,first_cut", cut_capacities())
def test_chain_cut_guarded(cuda, knobs, seq, cap, first_cut):
    """A cut chain over buffers inside one larger tensor, each followed by
    guard bytes the tensor owns, run twice: with everything outside the
    result filled with the later steps' class bytes (y, z) and with spaces.
    Whatever lies at or past `capacity` changes nothing (the same lengths in
    both runs, those of cut_lengths) and is not changed (no byte outside
    [0, capacity) of either buffer is written); the bytes that fit are the
    true text's."""
    import torch
    if seq:
        knobs(chain_seq=1)
    texts = cut_texts()
    t, lens = texts[0], [len(x) for x in texts]
    assert lens[first_cut - 1] <= cap < lens[first_cut]
    keep, res, reps, rl = chain_args(CUT_STEPS)
    hay = dev(t, cuda)
    span = (cap + 16 + GUARD + 15) // 16 * 16  # a buffer, its 16 readable bytes, its guard
    arena = torch.empty(16 + 2 * span, dtype=torch.uint8, device=cuda)
    off0 = -arena.data_ptr() % 16
    off1 = off0 + span
    inside = np.zeros(arena.numel(), dtype=bool)
    inside[off0:off0 + cap] = inside[off1:off1 + cap] = True
    want = cut_lengths(CUT_STEPS, texts, cap, seq)
    runs, checks = [], []
    for fill in (b"yz", b" "):
        pat = np.frombuffer(fill * arena.numel(), dtype=np.uint8)[:arena.numel()].copy()
        arena.copy_(torch.from_numpy(pat))
        lengths = torch.full((4,), -1, dtype=torch.int64, device=cuda)
        rc = N.rure_amd_replace_all_chain(res, reps, rl, 3, ctypes.c_void_p(hay.data_ptr()), len(t),
                                          ctypes.c_void_p(arena.data_ptr() + off0),
                                          ctypes.c_void_p(arena.data_ptr() + off1), cap,
                                          ctypes.c_void_p(lengths.data_ptr()), R._stream_ptr(None))
        assert rc == N.OK
        torch.cuda.synchronize()
        assert N.last_path() == (Path.REPLACE_CLASS if seq else Path.REPLACE_HMAP)
        got = arena.cpu().numpy()
        runs.append(lengths.cpu().numpy().tolist())
        outside = int((got[~inside] != pat[~inside]).sum())
        prefix = bytes(got[off0:off0 + cap]) == texts[3][:cap]
        print("seq=%d cap=%d fill=%r lengths=%r want=%r bytes changed outside=%d prefix right=%s"
              % (seq, cap, fill, runs[-1], want, outside, prefix))
        checks.append((outside, prefix))
    assert runs[0] == runs[1], runs                                                                # (a)
    assert [o for o, _ in checks] == [0, 0], "a byte at or past the capacity was written"          # (b)
    assert all(p for _, p in checks)                                                               # (f)
    ln = runs[0]
    assert ln[0] == len(t)                                                                         # (c)
    assert ln[:first_cut + 1] == lens[:first_cut + 1]  # up to the step that overflows first: exact
    assert ln == want                                                                              # (d), (e)
    assert all(cap < ln[k] <= lens[k] for k in range(first_cut + 1, 4))
    del keep


def test_chain_cut_then_nothing_to_replace(cuda, knobs):
    """Step by step, a step that finds nothing to replace in its cut input
    reports exactly the capacity: whether a chain was cut is read off every
    length, not the last one alone."""
    knobs(chain_seq=1)
    steps = CUT_STEPS[:2]
    t = b"x" * 1000 + b"y" * 10
    texts = chain_ref.apply_chain(steps, t)
    cap = 5008
    got, lengths = run_chain(steps, t, cuda, cap)
    assert lengths == cut_lengths(steps, texts, cap, 1) == [1010, 40010, cap]
    assert got[:cap] == texts[2][:cap]
    knobs()
    got, lengths = run_chain(steps, t, cuda, cap)
    assert lengths == [1010, 40010, 40020] and got[:cap] == texts[2][:cap]


def test_chain_argument_checks(cuda):
    """What the entry point refuses it refuses before it enqueues anything:
    the buffers and the lengths keep their bytes.  No steps: lengths[0] is
    the input length."""
    import torch
    steps = CUT_STEPS[:2]
    keep, res, reps, rl = chain_args(steps)
    hay = dev(b"xyxy" * 8, cuda)
    o0 = torch.full((256,), 0xAB, dtype=torch.uint8, device=cuda)
    o1 = torch.full((256,), 0xAB, dtype=torch.uint8, device=cuda)
    lengths = torch.full((3,), -7, dtype=torch.int64, device=cuda)
    assert hay.data_ptr() % 16 == 0 and o0.data_ptr() % 16 == 0 and o1.data_ptr() % 16 == 0

    def call(n=2, h=0, a=0, b=0, null1=False, lens=rl, res_=res):
        return N.rure_amd_replace_all_chain(res_, reps, lens, n, ctypes.c_void_p(hay.data_ptr() + h), 32,
                                            ctypes.c_void_p(o0.data_ptr() + a),
                                            None if null1 else ctypes.c_void_p(o1.data_ptr() + b), 200,
                                            ctypes.c_void_p(lengths.data_ptr()), R._stream_ptr(None))

    def sizes(*v):
        return (ctypes.c_size_t * 2)(*v)

    assert call(h=1) == N.ERR_ARG and call(h=8) == N.ERR_ARG
    assert call(a=1) == N.ERR_ARG and call(a=8) == N.ERR_ARG
    assert call(b=1) == N.ERR_ARG and call(b=8) == N.ERR_ARG
    assert call(null1=True) == N.ERR_ARG
    for bad in (0, 65):
        assert call(lens=sizes(bad, 2)) == N.ERR_ARG
        assert call(lens=sizes(40, bad)) == N.ERR_ARG
    torch.cuda.synchronize()
    assert (o0.cpu().numpy() == 0xAB).all() and (o1.cpu().numpy() == 0xAB).all()
    assert lengths.cpu().numpy().tolist() == [-7, -7, -7]
    # one step needs no second buffer; no steps write the input length alone
    assert call(n=1, null1=True) == N.OK
    torch.cuda.synchronize()
    assert lengths.cpu().numpy().tolist()[:2] == [32, 32 + 16 * 39]
    assert (o1.cpu().numpy() == 0xAB).all()
    lengths.fill_(-7)
    o0.fill_(0xAB)
    assert call(n=0, null1=True) == N.OK
    torch.cuda.synchronize()
    assert lengths.cpu().numpy().tolist() == [32, -7, -7]
    assert (o0.cpu().numpy() == 0xAB).all()
    del keep
