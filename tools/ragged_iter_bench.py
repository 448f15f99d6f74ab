"""find_iter_batch over offset batches (documents of their own lengths) with
and without the ragged unit geometry (iter_device.hpp Geo::uoff).  Regex
(--pattern): `[A-Z][a-z]+ (Holmes|Watson)`, of match type Dfa; or
`[A-Z][a-z]+ Holmes`, of match type DfaSuffix, which ran one wave per
haystack of an offset batch before.

  skew   4096 haystacks of at most 200 bytes and one of 64 MiB (sherlock
         repeated), as an offset batch; and the 64 MiB text alone as one
         fixed-stride haystack (the same kernels in the uniform geometry:
         what the ragged form adds is the geometry pass, two read-backs and
         the owner search).
  short  100 000 log lines of 40-160 bytes (workloads.log_lines_device): one
         unit per haystack either way; the new cost is the span reduction and
         its read-back.  An empty kernel plus a stream synchronisation is
         timed beside it.

Whole-call times: a host clock around rure_amd_find_iter_batch and a stream
synchronise, outputs allocated once, the median of --reps calls after
--warmup.  The library under test is whichever `regex_amd` imports first on
sys.path (run the same script from a checkout of the parent commit for its
figures); knob iter_ragged=0 on this commit gives the parent's geometry.
One JSON line per figure, appended to --out when given.

    python tools/ragged_iter_bench.py [--what skew,short] [--pattern RE] [--reps R] [--label L] [--out FILE]
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


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return {"ms_median": round(ts[len(ts) // 2], 4), "ms_min": round(ts[0], 4), "ms_max": round(ts[-1], 4)}


def caller(re, hay, offs=None, stride=None, length=None, count=None, cap=1 << 20):
    """The raw call on preallocated outputs, ending in a synchronise; returns
    (call, read) where read() gives (total matches, sum of counts)."""
    b = R._batch(hay, offs, stride, length, count, 0)
    dev = hay.device
    counts = torch.empty(b.count, dtype=torch.int64, device=dev)
    out = torch.empty((cap, 2), dtype=torch.int64, device=dev)
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    vp = ctypes.c_void_p

    def call():
        rc = N.rure_amd_find_iter_batch(re._re, ctypes.byref(b), vp(counts.data_ptr()), vp(out.data_ptr()), cap,
                                        vp(total.data_ptr()), None)
        assert rc == 0, rc
        torch.cuda.synchronize()

    def read():
        t = int(total.item())
        assert t <= cap, (t, cap)
        return t, int(counts.sum().item()), out[:t].cpu().numpy().copy(), counts.cpu().numpy().copy()

    return call, read


def units():
    f = getattr(N, "last_iter_units", None)  # absent before the ragged geometry
    return list(f()) if f else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="skew,short")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--label", default="")
    ap.add_argument("--long-mib", type=int, default=64)
    ap.add_argument("--pattern", default=PAT)
    ap.add_argument("--out")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    re = R.Regex(a.pattern)
    lines = []

    def emit(**kw):
        kw = dict(label=a.label, pattern=a.pattern, knobs=R._debug_spec[0] or "", **kw)
        print(json.dumps(kw), flush=True)
        lines.append(kw)

    what = a.what.split(",")
    if "skew" in what:
        text = np.frombuffer(corpus("sherlock"), dtype=np.uint8)
        nlong = a.long_mib << 20
        rng = np.random.default_rng(64)
        lens = rng.integers(0, 201, size=4096)
        at = rng.integers(0, len(text) - 200, size=4096)
        short = [text[p:p + n] for p, n in zip(at, lens)]
        long_ = np.tile(text, nlong // len(text) + 1)[:nlong]
        # the long document in the middle of the batch
        parts = short[:2048] + [long_] + short[2048:]
        offs = np.zeros(len(parts) + 1, dtype=np.int64)
        offs[1:] = np.cumsum([len(p) for p in parts])
        hay = torch.from_numpy(np.concatenate(parts + [np.zeros(16, dtype=np.uint8)])).to(dev)
        od = torch.from_numpy(offs).to(dev)
        call, read = caller(re, hay, offs=od, cap=4 << 20)
        call()
        tot, csum, m_ragged, c_ragged = read()
        assert tot == csum
        emit(case="skew_offsets", haystacks=len(parts), bytes=int(offs[-1]), matches=tot, units=units(),
             **timed(call, a.warmup, a.reps))
        # the long text alone, fixed stride
        lh = torch.from_numpy(np.concatenate([long_, np.zeros(16, dtype=np.uint8)])).to(dev)
        call1, read1 = caller(re, lh, stride=nlong, length=nlong, count=1, cap=4 << 20)
        call1()
        tot1, _, m_fixed, _ = read1()
        # same matches in the long document either way
        k0 = int(c_ragged[:2048].sum())
        assert int(c_ragged[2048]) == tot1 and np.array_equal(m_ragged[k0:k0 + tot1], m_fixed)
        emit(case="skew_long_alone_fixed_stride", haystacks=1, bytes=nlong, matches=tot1, units=units(),
             **timed(call1, a.warmup, a.reps))
    if "short" in what:
        hay, od = log_lines_device(100000, dev)
        call, read = caller(re, hay, offs=od)
        call()
        tot, csum, _, _ = read()
        assert tot == csum
        emit(case="short_lines", haystacks=100000, bytes=int(od[-1].item()), matches=tot, units=units(),
             **timed(call, a.warmup, a.reps))
        x = torch.zeros(1, device=dev)

        def empty_sync():
            x.add_(0)  # one trivial kernel
            torch.cuda.synchronize()

        emit(case="empty_kernel_plus_sync", **timed(empty_sync, a.warmup, a.reps))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for kw in lines:
                f.write(json.dumps(kw) + "\n")


if __name__ == "__main__":
    main()
