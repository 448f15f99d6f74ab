"""find / is_match / shortest_match over offset batches (documents of their own
lengths) with and without the deferred long scan (dispatch.cpp
run_ragged_long): the one-lane-per-haystack kernel leaves the long haystacks
on a device list, a chunked scan of the listed ones follows, nothing is read
back.  Regexes: `[A-Z][a-z]+ (Holmes|Watson)` (match type Dfa),
`Sherlock|Holmes` (the literal engine), `\\d{4}-\\d{2}-\\d{2}`,
`\\w{1,10}@\\w{1,10}`.

  A  4096 haystacks of at most 200 bytes and one of 64 MiB (sherlock
     repeated), as an offset batch: find, is_match, shortest_match; is_match
     of the literal regex (both match early in the document, where one
     lane's search ends); find and is_match of the date regex, which matches
     nowhere in it; the units from rure_amd_last_long_units.
  B  the 64 MiB alone as one fixed-stride haystack, same calls: today's
     long_scan_kernel on the same bytes, the yardstick of A.
  C  100 000 log lines of 40-160 bytes (workloads.log_lines_device): find and
     is_match, nothing to defer; with knob long_ragged=0 where the library
     knows it.  Beside it the cost of launches that exit at once: k trivial
     kernels enqueued back to back and one synchronise, against one kernel
     and a synchronise.
  D  the sherlock text replicated to ~1 GiB and cut at its newlines
     (tools/ragged_bench.py's batch): is_match and find, bytes per second.
  E  the first offset-batch find of a fresh regex (host work included: the
     deferred scan needs the find_iter automaton, built on that call).

Whole-call times: a host clock around the C call and a stream synchronise,
outputs allocated once, the median of --reps calls after --warmup (a call
that takes more than 100 ms is repeated three times only).  The library under
test is whichever `regex_amd` imports first on sys.path: run the same script
with PYTHONPATH at a checkout of the parent commit for its figures.  One JSON
line per figure, appended to --out when given.

    python tools/ragged_long_bench.py [--what A,B,C,D,E] [--reps R] [--label L] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)  # after PYTHONPATH: another checkout's package may be measured
sys.path.append(os.path.join(ROOT, "tests"))
import regex_amd as R  # noqa: E402
from regex_amd import _native as N  # noqa: E402
from regex_amd.workloads import log_lines_device  # noqa: E402
from golden_data import corpus  # noqa: E402

PAT = r"[A-Z][a-z]+ (Holmes|Watson)"
LIT = r"Sherlock|Holmes"
DATE = r"\d{4}-\d{2}-\d{2}"
MAIL = r"\w{1,10}@\w{1,10}"
HAS_KNOB = hasattr(N, "rure_amd_last_long_units")  # this commit's library and package


def timed(fn, warmup, reps):
    t0 = time.perf_counter()
    fn()
    if time.perf_counter() - t0 > 0.1:
        warmup, reps = 0, 3
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return {"ms_median": round(ts[len(ts) // 2], 4), "ms_min": round(ts[0], 4), "ms_max": round(ts[-1], 4),
            "reps": reps}


def caller(re, mode, hay, offs=None, stride=None, length=None, count=None):
    """The raw call on a preallocated output, ending in a synchronise."""
    b = R._batch(hay, offs, stride, length, count, 0)
    shape, dt = {"find": ((b.count, 2), torch.int64), "is_match": ((b.count,), torch.uint8),
                 "shortest_match": ((b.count,), torch.int64)}[mode]
    out = torch.empty(shape, dtype=dt, device=hay.device)
    fn = getattr(N, "rure_amd_%s_batch" % mode)
    vp = ctypes.c_void_p

    def call():
        rc = fn(re._re, ctypes.byref(b), vp(out.data_ptr()), None)
        assert rc == 0, rc
        torch.cuda.synchronize()

    return call, out


def units():
    return list(N.last_long_units()) if HAS_KNOB else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="A,B,C,D,E")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--label", default="")
    ap.add_argument("--long-mib", type=int, default=64)
    ap.add_argument("--out")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def emit(**kw):
        kw = dict(label=a.label, knobs=R._debug_spec[0] or "", **kw)
        print(json.dumps(kw), flush=True)
        lines.append(kw)

    what = a.what.split(",")
    # (PAT and LIT match within the document's first KiB, where a lane's search
    # ends; DATE matches nowhere in it: the lane walks all of it)
    calls = [(PAT, "find"), (PAT, "is_match"), (PAT, "shortest_match"), (LIT, "is_match"), (DATE, "find"),
             (DATE, "is_match")]
    res = {p: R.Regex(p) for p in (PAT, LIT, DATE)}
    if "A" in what or "B" in what:
        text = np.frombuffer(corpus("sherlock"), dtype=np.uint8)
        nlong = a.long_mib << 20
        rng = np.random.default_rng(64)
        lens = rng.integers(0, 201, size=4096)
        at = rng.integers(0, len(text) - 200, size=4096)
        short = [text[p:p + n] for p, n in zip(at, lens)]
        long_ = np.tile(text, nlong // len(text) + 1)[:nlong]
        parts = short[:2048] + [long_] + short[2048:]  # the long document in the middle of the batch
        offs = np.zeros(len(parts) + 1, dtype=np.int64)
        offs[1:] = np.cumsum([len(p) for p in parts])
        hay = torch.from_numpy(np.concatenate(parts + [np.zeros(16, dtype=np.uint8)])).to(dev)
        od = torch.from_numpy(offs).to(dev)
        lh = torch.from_numpy(np.concatenate([long_, np.zeros(16, dtype=np.uint8)])).to(dev)
        for pat, mode in calls:
            call, out = caller(res[pat], mode, hay, offs=od)
            call1, out1 = caller(res[pat], mode, lh, stride=nlong, length=nlong, count=1)
            if "A" in what:
                emit(row="A", case="skew_offsets", pattern=pat, mode=mode, haystacks=len(parts), bytes=int(offs[-1]),
                     **timed(call, a.warmup, a.reps), units=units(), path=int(N.rure_amd_last_fwd_path()))
            if "B" in what:
                emit(row="B", case="long_alone_fixed_stride", pattern=pat, mode=mode, haystacks=1, bytes=nlong,
                     **timed(call1, a.warmup, a.reps), path=int(N.rure_amd_last_fwd_path()))
            if "A" in what and "B" in what:  # the same answer for the long document either way
                assert out[2048].cpu().tolist() == out1[0].cpu().tolist(), (pat, mode)
        del hay, lh
    if "C" in what:
        hay, od = log_lines_device(100000, dev)
        for pat in (PAT, DATE):
            for mode in ("find", "is_match"):
                call, out = caller(res[pat], mode, hay, offs=od)
                call()
                ref = out.clone()
                emit(row="C", case="short_lines", pattern=pat, mode=mode, haystacks=100000, bytes=int(od[-1].item()),
                     **timed(call, a.warmup, a.reps), units=units(), path=int(N.rure_amd_last_fwd_path()))
                if HAS_KNOB:
                    with R.debug(long_ragged=0):
                        emit(row="C", case="short_lines", pattern=pat, mode=mode, haystacks=100000,
                             **timed(call, a.warmup, a.reps), path=int(N.rure_amd_last_fwd_path()))
                        assert torch.equal(out, ref)
        # launches that exit at once: what the deferred scan adds to a batch
        # that defers nothing is three of them (the header's init kernel, the
        # geometry kernel, the ragged scan), an event record and a scratch
        # block; `added_ms` of 4 kernels is the cost of the three
        x = torch.zeros(1, device=dev)

        def trivial(k):
            def f():
                for _ in range(k):
                    x.add_(0)
                torch.cuda.synchronize()
            return f

        one = timed(trivial(1), a.warmup, a.reps)
        for k in (4, 5):
            t = timed(trivial(k), a.warmup, a.reps)
            emit(row="C", case="trivial_kernels_back_to_back", kernels=k, **t, one_kernel_ms_median=one["ms_median"],
                 added_ms=round(t["ms_median"] - one["ms_median"], 4))
        del hay
    if "D" in what:
        text = corpus("sherlock")
        big = text * ((1 << 30) // len(text))
        hay = torch.from_numpy(np.frombuffer(big + b"\0" * 16, dtype=np.uint8).copy()).to(dev)
        ends = np.nonzero(np.frombuffer(big, dtype=np.uint8) == 10)[0] + 1
        od = torch.from_numpy(np.concatenate([[0], ends]).astype(np.int64)).to(dev)
        for mode in ("is_match", "find"):
            call, _ = caller(res[PAT], mode, hay, offs=od)
            t = timed(call, a.warmup, a.reps)
            emit(row="D", case="sherlock_lines", pattern=PAT, mode=mode, haystacks=int(od.numel() - 1),
                 bytes=int(ends[-1]), **t, gb_per_s=round(int(ends[-1]) / t["ms_median"] / 1e6, 1), units=units(),
                 path=int(N.rure_amd_last_fwd_path()))
        del hay
    if "E" in what:
        hay, od = log_lines_device(100000, dev)
        for pat in (DATE, MAIL):
            t0 = time.perf_counter()
            re = R.Regex(pat)
            t1 = time.perf_counter()
            call, _ = caller(re, "find", hay, offs=od)
            call()
            t2 = time.perf_counter()
            call()
            t3 = time.perf_counter()
            emit(row="E", case="first_call", pattern=pat, mode="find", compile_ms=round((t1 - t0) * 1e3, 3),
                 first_call_ms=round((t2 - t1) * 1e3, 3), second_call_ms=round((t3 - t2) * 1e3, 3))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for kw in lines:
                f.write(json.dumps(kw) + "\n")


if __name__ == "__main__":
    main()
