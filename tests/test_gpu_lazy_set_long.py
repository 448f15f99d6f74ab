"""RegexSet matches over few long haystacks on the set's on-demand DFA
(big_dfa.hip lazy_set_long_kernel, dispatch.cpp run_lazy_set_long): a set
whose automaton is past the eager state budget used to search one long
haystack on the Pike VM, a wave per haystack.  Now the haystack is cut into
units; unit [c0, c1) steps into its state's twin without the `.*?` prefix at
c1 - 1 (a link made on demand, as rows are), walks on until the automaton
dies or can report nothing new, and ORs its patterns into the haystack's word.
Forced onto 5000-byte haystacks with 16-, 48- and 4096-byte units (knobs
lazy_long=2, lazy_chunk; sets with an eager DFA under lazy=1, lazy_rows=1 park
on nearly every row and link), by the production rule on 1 MiB, through the
host calls and the words form, and the batches and sets that keep their
paths.  Every mask is the oracle's; last_path() == Path.LAZY_DFA, the units
reported and fell_back == 0 assert that the chunked kernel gave it and not
the Pike VM fallback.

Rounds: a batch that needs 256 rounds or more goes to the Pike VM, so the
texts of the set without a DFA plant a/b runs from a pool of six, whose states
the units share; _sim_rounds() checks on the CPU simulation that every input
here stays below that.  The simulation builds no row ahead and lets no unit
leave early, and runs the calls in the order the test makes them on one
automaton: the device has at least its rows at every call, so it needs at most
its rounds."""
import ctypes
import functools

import numpy as np
import pytest

import regex_amd as R
from regex_amd import Path
from regex_amd import _native as N
from golden_data import corpus
from lazy_set_long_sim import SetLongTables, Stats, lazy_set_long
from lazy_set_sim import FLAGS, NO_DFA
from oracle_py import OracleRegex
from set_long_data import CASES, MIXED
from test_gpu_lazy_long import L, STRIDE, COUNT, MIB, _dev, _mib, _small, _unit_bytes
from test_gpu_set_long import _log

pytestmark = pytest.mark.gpu

SETS = {"no_dfa": NO_DFA, "flags": FLAGS, "mixed": MIXED, "literals": CASES["literals"][0],
        "c4_ascii_wb": CASES["c4_ascii_wb"][0]}
CHUNKS = (16, 48, 4096)


def _forced(name, chunk):
    kn = dict(lazy_long=2, lazy_chunk=chunk)
    if name != "no_dfa":
        kn.update(lazy=1, lazy_rows=1)
    return kn


@functools.lru_cache(maxsize=None)
def _texts(name):
    """3 haystacks of 5000 bytes at stride 5003: for the set without a DFA
    sherlock pieces with planted a/b runs (the first haystack made to begin
    with `a`, for `^a`), for the others log lines (the first haystack ends in
    `abc`, for `abc$` of MIXED; the second has no `ERROR`)."""
    if name == "no_dfa":
        raw = b"a" + _small()[0][1:]
    else:
        raw = bytearray(bytes(_log()[:COUNT * STRIDE]))
        raw[L - 3:L] = b"abc"
        raw[STRIDE:2 * STRIDE] = bytes(raw[STRIDE:2 * STRIDE]).replace(b"ERROR", b"ERR0R")
        raw = bytes(raw)
    return raw, [raw[h * STRIDE:h * STRIDE + L] for h in range(COUNT)]


def _mask(o, t, start=0):
    return sum(1 << j for j in o.matches(t, start)) if start <= len(t) else 0


def _by_pattern(pats, t):
    """The mask of a megabyte pattern by pattern (the set oracle spends half a
    minute per megabyte once its lazy DFA gives up; a pattern's membership
    does not depend on the rest of the set, test_set_groups.py)."""
    return sum(1 << j for j, p in enumerate(pats) if OracleRegex(R.Regex(p)).is_match(t))


def _u64(x):
    return int(x) & ((1 << 64) - 1)


def _nk(length, start, chunk):
    span = max(length - start, 0)
    return 1 if span <= chunk else -(-span // chunk)


def _chunked(rs, count, nk, chunk):
    """The last call ran the chunked kernel to the end."""
    assert N.last_path() == Path.LAZY_DFA
    assert R.RegexSet.last_long_units() == (count * nk, count, chunk)
    info = rs.lazy_tables()[0]
    assert info["fell_back"] == 0 and 0 < info["rounds"] < 256, info
    return info


def _sim_rounds(tb, texts, start, chunk, bases):
    got, rounds = lazy_set_long(tb, texts, start, chunk, 0, 256, use_reach=False, use_all=False, bases=bases)
    assert got is not None and rounds < 256, (start, chunk, rounds)
    return got


def _forced_calls():
    return [(chunk, count, start) for chunk in CHUNKS for count in (1, COUNT) for start in (0, 3, chunk, L, L + 1)]


@pytest.mark.parametrize("name", sorted(SETS))
def test_forced_units(cuda, knobs, name):
    """1 and 3 haystacks of 5000 bytes, stride 5003, one byte past an aligned
    base, in units of 16, 48 and 4096 bytes from starts 0, 3, the unit size
    (what is a cut from 0), L and L + 1.  More than one unit per haystack
    wherever the span exceeds the unit: from 0 and 3 always."""
    raw, texts = _texts(name)
    rs = R.RegexSet(SETS[name])
    assert rs.uses_dfa() == (name != "no_dfa")
    o = OracleRegex(rs)
    tb = SetLongTables(R.RegexSet(SETS[name]))
    exp = {}
    for chunk, count, start in _forced_calls():
        for h in range(count):
            if (h, start) not in exp:
                exp[h, start] = _mask(o, texts[h], start)
        want = [exp[h, start] for h in range(count)]
        assert _sim_rounds(tb, texts[:count], start, chunk, [1 + h * STRIDE for h in range(count)]) == want
    dev = _dev(cuda, raw, 1)
    for chunk, count, start in _forced_calls():
        knobs(**_forced(name, chunk))
        got = rs.matches_batch(dev, stride=STRIDE, length=L, count=count, start=start).cpu().numpy()
        assert [_u64(g) for g in got] == [exp[h, start] for h in range(count)], (name, chunk, count, start)
        nk = _nk(L, start, chunk)
        _chunked(rs, count, nk, chunk)
        assert nk > 1 or start >= chunk
    assert len(set(exp.values())) > 1 and len({exp[h, 0] for h in range(COUNT)}) > 1
    assert rs.lazy_tables()[0]["rows_built"] > 0


@functools.lru_cache(maxsize=None)
def _mib_case(planted):
    """1 MiB for the set without a DFA and its mask."""
    text = _mib(planted)
    exp = _by_pattern(NO_DFA, text)
    return text, exp


def _production_chunk(cuda):
    import torch
    return _unit_bytes(MIB, 1, torch.cuda.get_device_properties(cuda).multi_processor_count)


@functools.lru_cache(maxsize=None)
def _mib_rounds(planted, chunk):
    text, exp = _mib_case(planted)
    assert _sim_rounds(SetLongTables(R.RegexSet(NO_DFA)), [text], 0, chunk, [0]) == [exp]
    return True


def test_production_rule(cuda):
    """No knob, one haystack of 1 MiB: the rule takes the chunked scan by
    itself, in units of the long scan's size; the batched call and the host
    calls on the same bytes give the oracle's mask and report units."""
    text, exp = _mib_case(True)
    assert exp == 3  # the runs hold both the long pattern and `bb`; the text does not begin with `a`
    chunk = _production_chunk(cuda)
    assert _mib_rounds(True, chunk)
    rs = R.RegexSet(NO_DFA)
    assert not rs.uses_dfa()
    got = rs.matches_batch(_dev(cuda, text), stride=MIB, length=MIB, count=1).cpu().numpy()
    assert _u64(got[0]) == exp
    nk = -(-MIB // chunk)
    assert nk > 1
    _chunked(rs, 1, nk, chunk)
    assert sum(1 << j for j in rs.matches(text)) == exp
    _chunked(rs, 1, nk, chunk)
    assert rs.is_match(text) is True
    _chunked(rs, 1, nk, chunk)
    assert sum(1 << j for j in rs.matches(text, 3)) == exp
    _chunked(rs, 1, _nk(MIB, 3, chunk), chunk)


def test_nothing_new_matches(cuda):
    """A megabyte of plain sherlock text (no a/b run: only `bb`, inside
    words): exactly the oracle's mask, still chunked."""
    text, exp = _mib_case(False)
    assert exp & 1 == 0
    chunk = _production_chunk(cuda)
    assert _mib_rounds(False, chunk)
    rs = R.RegexSet(NO_DFA)
    got = rs.matches_batch(_dev(cuda, text), stride=MIB, length=MIB, count=1).cpu().numpy()
    assert _u64(got[0]) == exp
    _chunked(rs, 1, -(-MIB // chunk), chunk)
    # and a set of which nothing matches at all: mask 0
    quiet = [NO_DFA[0], r"qqq", r"^a"]
    assert _by_pattern(quiet, text) == 0
    rq = R.RegexSet(quiet)
    assert not rq.uses_dfa()
    got = rq.matches_batch(_dev(cuda, text), stride=MIB, length=MIB, count=1).cpu().numpy()
    assert _u64(got[0]) == 0
    _chunked(rq, 1, -(-MIB // chunk), chunk)


def test_second_call_reuses_the_table(cuda, knobs):
    """Whether a unit leaves at a poll depends on what the other units have
    published by then, and with it the rows a call reads.  This input has no
    such exit: no haystack matches every pattern, and the two bytes before
    every 16-byte block that polls and the block itself (a unit that resumes
    inside it polls again) are blanks, so a unit past its cut is dead before
    it polls (or polls in its cut's own state, which can still report every
    pattern).  The simulation with the exits on confirms that no unit leaves;
    the second call then reads exactly the rows the first one built."""
    import torch
    raw = bytearray(b" " + _small()[0][1:])  # (not `^a`)
    dev = _dev(cuda, bytes(raw), 1)
    bases = [(dev.data_ptr() + h * STRIDE) % 512 for h in range(COUNT)]
    for p in range(2, len(raw)):
        if (dev.data_ptr() + p) % 512 == 0:
            raw[p - 2:p + 16] = b" " * 18
    raw = bytes(raw)
    dev[:len(raw)].copy_(torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()))
    texts = [raw[h * STRIDE:h * STRIDE + L] for h in range(COUNT)]
    rs = R.RegexSet(NO_DFA)
    o = OracleRegex(rs)
    exp = [_mask(o, t) for t in texts]
    assert all(e not in (0, 7) for e in exp)
    st = Stats()
    assert lazy_set_long(SetLongTables(R.RegexSet(NO_DFA)), texts, 0, 48, 0, 256, bases=bases, stats=st)[0] == exp
    assert st.polls > 0 and st.left == 0
    knobs(lazy_long=2, lazy_chunk=48)
    first = rs.matches_batch(dev, stride=STRIDE, length=L, count=COUNT).cpu().numpy()
    a = _chunked(rs, COUNT, _nk(L, 0, 48), 48)
    second = rs.matches_batch(dev, stride=STRIDE, length=L, count=COUNT).cpu().numpy()
    b = _chunked(rs, COUNT, _nk(L, 0, 48), 48)
    assert a["rounds"] > 1 and b["rounds"] == 1
    assert b["rows_built"] == a["rows_built"] and b["states"] == a["states"]
    assert np.array_equal(first, second)
    assert [_u64(g) for g in first] == exp


def test_budget_falls_back(cuda, knobs):
    """A few KiB of budget: the Pike VM answers the whole batch, and the
    units are still reported."""
    raw, texts = _texts("no_dfa")
    knobs(lazy_long=2, lazy_chunk=48, big_bytes=4096)
    rs = R.RegexSet(NO_DFA)  # (the budget is read when the automaton is created)
    o = OracleRegex(rs)
    got = rs.matches_batch(_dev(cuda, raw, 1), stride=STRIDE, length=L, count=COUNT).cpu().numpy()
    assert N.last_path() == Path.PIKE_ONLY
    assert rs.lazy_tables()[0]["fell_back"] == 1
    assert R.RegexSet.last_long_units() == (COUNT * _nk(L, 0, 48), COUNT, 48)
    assert [_u64(g) for g in got] == [_mask(o, t) for t in texts]
    assert len({_u64(g) for g in got}) > 1


def test_words_form(cuda):
    """67 patterns: a group of 64 words with a DFA (chunked on set_long_kernel)
    and the three patterns without one as the second group, through
    rure_amd_set_matches_batch_words on one 1 MiB haystack."""
    import torch
    words = sorted(set(w for w in corpus("sherlock")[:40000].decode("ascii", "ignore").split()
                       if w.isalpha() and w.islower() and len(w) >= 4))[:64]
    assert len(words) == 64
    rs = R.RegexSet(words + NO_DFA)
    assert len(rs) == 67 and not rs.uses_dfa()
    text, exp1 = _mib_case(True)
    chunk = _production_chunk(cuda)
    assert _mib_rounds(True, chunk)
    out = torch.full((1, 3), -5, dtype=torch.int64, device=cuda)
    dev = _dev(cuda, text)
    b = R._batch(dev, stride=MIB, length=MIB, count=1)
    assert N.rure_amd_set_matches_batch_words(rs._set, ctypes.byref(b), ctypes.c_void_p(out.data_ptr()), 3,
                                              R._stream_ptr(None)) == N.OK
    # the last group ran this path
    assert N.last_path() == Path.LAZY_DFA
    assert R.RegexSet.last_long_units() == (-(-MIB // chunk), 1, chunk)
    got = out.cpu().numpy()[0].view(np.uint64)
    exp0 = _mask(OracleRegex(R.RegexSet(words)), text)
    assert (int(got[0]), int(got[1]), int(got[2])) == (exp0, exp1, 0)
    assert exp0 and exp1 == 3


@pytest.mark.parametrize("name", ["no_dfa", "mixed"])
def test_buffer_contract(cuda, knobs, name):
    """The last haystack ends in the last 16-byte block of its tensor, with
    no padding after it, and the bytes between and after the haystacks hold
    text that would match: the masks are those of the haystacks alone."""
    import torch
    rs = R.RegexSet(SETS[name])
    o = OracleRegex(rs)
    count, base, ln, stride = 3, 5, 5003, 5021  # (an odd base: no haystack starts on a 16-byte boundary)
    total = (base + (count - 1) * stride + ln + 15) & ~15
    assert 0 < total - (base + (count - 1) * stride + ln) < 16
    fill = b"abc\n12 foo z " + b"a" * 19 + b"bb x" + b"a"
    host = np.frombuffer((fill * (total // len(fill) + 1))[:total], dtype=np.uint8).copy()
    text = _mib(True)[1000:1000 + count * ln]
    text = text.replace(b"bb", b"ba") if name == "no_dfa" else text
    for h in range(count):
        host[base + h * stride:base + h * stride + ln] = np.frombuffer(text[h * ln:(h + 1) * ln], dtype=np.uint8)
    hays = [text[h * ln:(h + 1) * ln] for h in range(count)]
    exp = [_mask(o, t) for t in hays]
    # the surroundings would have changed an answer
    assert any(_mask(o, bytes(host[base + h * stride - 1:base + h * stride + ln + 13])) != exp[h] for h in range(count))
    tb = SetLongTables(R.RegexSet(SETS[name]))
    dev = torch.from_numpy(host).to(cuda)
    assert dev.numel() == total
    for c in (16, 4096):
        assert _sim_rounds(tb, hays, 0, c, [base + h * stride for h in range(count)]) == exp
        knobs(**_forced(name, c))
        got = rs.matches_batch(dev[base:], stride=stride, length=ln, count=count).cpu().numpy()
        assert [_u64(g) for g in got] == exp, (name, c)
        _chunked(rs, count, _nk(ln, 0, c), c)


KIB256 = 256 << 10  # the rule's span threshold: the smallest haystack it takes
ANCHORED = ["^" + NO_DFA[0], r"^bb", r"^(?s:.)"]
UNICODE_WB = [NO_DFA[0], r"\bbb", r"^a"]


@pytest.mark.parametrize("pats,kn,offsets,size", [
    (NO_DFA, dict(lazy_long=0), False, KIB256), (NO_DFA, dict(lazy=0), False, KIB256),
    (NO_DFA, dict(set_long=0), False, KIB256), (NO_DFA, {}, True, MIB), (ANCHORED, {}, False, KIB256),
    (UNICODE_WB, {}, False, KIB256)], ids=["lazy_long=0", "lazy=0", "set_long=0", "offsets", "anchored", "unicode_wb"])
def test_kept_on_the_pike_vm(cuda, knobs, pats, kn, offsets, size):
    """What does not take the chunked on-demand scan answers right on the
    Pike VM as before, and reports no units: the knobs that turn the path off,
    an offset batch holding the megabyte, a set anchored at the start and one
    with a Unicode `\\b` member (256 KiB, the rule's threshold, where the size
    is free: the Pike VM needs a second per megabyte)."""
    import torch
    text = _mib(True)[:size]
    want = _by_pattern(pats, text)
    assert want != 0
    rs = R.RegexSet(pats)
    assert not rs.uses_dfa()
    dev = _dev(cuda, text)
    knobs(**kn)
    if offsets:
        got = rs.matches_batch(dev, offsets=torch.tensor([0, size], dtype=torch.int64, device=cuda)).cpu().numpy()
    else:
        got = rs.matches_batch(dev, stride=size, length=size, count=1).cpu().numpy()
    assert _u64(got[0]) == want
    assert N.last_path() == Path.PIKE_ONLY and R.RegexSet.last_long_units() == (0, 0, 0)
    if not offsets and not kn:
        assert sum(1 << j for j in rs.matches(text)) == want and R.RegexSet.last_long_units() == (0, 0, 0)
    if kn and pats is NO_DFA:  # and the chunked path on the same set once the knob is gone
        knobs()
        got = rs.matches_batch(dev, stride=size, length=size, count=1).cpu().numpy()
        assert _u64(got[0]) == want
        chunk = _unit_bytes(size, 1, torch.cuda.get_device_properties(cuda).multi_processor_count)
        _chunked(rs, 1, -(-size // chunk), chunk)


def test_kept_kernels(cuda):
    """CUs x 64 haystacks run one lane each on lazy_set_kernel, a set with an
    eager DFA keeps set_long_kernel on its megabyte; the chunked on-demand scan
    after them on the same set."""
    import torch
    text, exp = _mib_case(True)
    dev = _dev(cuda, text)
    rs = R.RegexSet(NO_DFA)
    o = OracleRegex(rs)
    n = torch.cuda.get_device_properties(cuda).multi_processor_count * 64
    ln = MIB // n
    got = rs.matches_batch(dev, stride=ln, length=ln, count=n).cpu().numpy()
    assert N.last_path() == Path.LAZY_DFA and R.RegexSet.last_long_units() == (0, 0, 0)
    want = [_mask(o, text[h * ln:(h + 1) * ln]) for h in range(n)]
    assert [_u64(g) for g in got] == want and len(set(want)) > 1
    log = _log()
    rm = R.RegexSet(MIXED)
    got = rm.matches_batch(torch.from_numpy(log).to(cuda), stride=MIB, length=MIB, count=1).cpu().numpy()
    assert N.last_path() == Path.LONG_SCAN and R.RegexSet.last_long_units()[0] > 1
    assert _u64(got[0]) == _mask(OracleRegex(rm), bytes(log[:MIB]))
    got = rs.matches_batch(dev, stride=MIB, length=MIB, count=1).cpu().numpy()
    assert _u64(got[0]) == exp
    chunk = _production_chunk(cuda)
    _chunked(rs, 1, -(-MIB // chunk), chunk)
