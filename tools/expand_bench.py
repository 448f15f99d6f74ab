"""replace_all with a `$` template on the device (rure_amd_replace_expand_batch)
against the literal replace (rure_amd_replace_batch) on the same batch:
1 048 576 x 4096 B of date_haystacks, `(?P<y>\\d{4})-(?P<m>\\d{2})-(?P<d>\\d{2})`
-> `$d/$m/$y` and -> a 10-byte literal.  Both run the same find_iter and move
the same bytes; the difference is the captures pass and the variable-length
plan.  Whole-call times (host clock around calls that end in a synchronise,
one reused output buffer, the two calls alternating); the kernel split comes
from a run of its own under `rocprofv3 --kernel-trace --stats` with --only.

    python tools/expand_bench.py [--n N] [--len L] [--frac F] [--reps R] [--only expand|literal] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import regex_amd as R  # noqa: E402
from regex_amd import _native as N  # noqa: E402
from regex_amd.workloads import date_haystacks_device  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--len", type=int, default=4096)
    ap.add_argument("--frac", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", choices=["expand", "literal"])
    ap.add_argument("--out")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n, L = a.n, a.len
    hay, planted = date_haystacks_device(n, L, 0x5EED0002, dev, frac=a.frac)
    hay = torch.cat([hay, torch.zeros(16, dtype=torch.uint8, device=dev)])
    re = R.Regex(r"(?P<y>\d{4})-(?P<m>\d{2})-(?P<d>\d{2})")
    cap = n * L + 1024
    out = torch.empty(cap + 16, dtype=torch.uint8, device=dev)
    ooff = torch.empty(n + 1, dtype=torch.int64, device=dev)
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    div = torch.zeros(n, dtype=torch.uint8, device=dev)
    b = R._batch(hay, None, L, L, n, 0)
    vp = ctypes.c_void_p

    def expand():
        rc = N.rure_amd_replace_expand_batch(re._re, ctypes.byref(b), b"$d/$m/$y", 8, 0, vp(out.data_ptr()),
                                             vp(ooff.data_ptr()), cap, vp(total.data_ptr()), vp(div.data_ptr()), None)
        assert rc == 0
        torch.cuda.synchronize()

    def literal():
        rc = N.rure_amd_replace_batch(re._re, ctypes.byref(b), b"DD/MM/YYYY", 10, 0, vp(out.data_ptr()),
                                      vp(ooff.data_ptr()), cap, vp(total.data_ptr()), None)
        assert rc == 0
        torch.cuda.synchronize()

    fns = {"expand": expand, "literal": literal}
    if a.only:
        fns = {a.only: fns[a.only]}
    times = {k: [] for k in fns}
    for k, fn in fns.items():   # warm-up: tables, the match-buffer guess, code objects
        fn()
        fn()
        assert int(total.item()) == n * L and int(div.sum().item()) == 0
    for _ in range(a.reps):
        for k, fn in fns.items():
            t = time.perf_counter()
            fn()
            times[k].append((time.perf_counter() - t) * 1e3)
    counts, _ = re.find_iter_batch(hay, stride=L, length=L, count=n, capacity=1)
    res = {"bench": "expand_replace", "n": n, "len": L, "frac": a.frac, "matches": int(counts.sum().item()),
           "planted": int(len(planted)), "bytes": n * L, "reps": a.reps}
    for k, v in times.items():
        v = sorted(v)
        res[k + "_ms_median"] = round(v[len(v) // 2], 3)
        res[k + "_ms_min"] = round(v[0], 3)
        res[k + "_ms_max"] = round(v[-1], 3)
    if len(times) == 2:
        res["expand_over_literal"] = round(res["expand_ms_median"] / res["literal_ms_median"], 3)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
