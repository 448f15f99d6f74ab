"""Device grep (Regex.match_records, records.hip) over one raw buffer of
sherlock lines, against what a caller could do before it existed: a torch pass
that builds an offsets array from the newlines, is_match_batch(offsets=...)
and a nonzero over its output.  That two-step path keeps each line's newline
inside its haystack, so its answers may differ where a regex sees the
delimiter: only the timings are compared (the counts are printed).

The text is the sherlock corpus tiled to --bytes (default 1 GiB, past the
256 MiB cache).  Each variant: warm-up calls, then the median of event-timed
calls with the stream synchronised around each; the variants alternate.
`records` = one call with the capacity known, `records_sized` = the wrapper's
default (a capacity-0 call to size the buffers, then the call).  One JSON line
per (regex, variant); `frac_hbm` = bytes / time over 8 TB/s.
usage: python tools/records_bench.py [--bytes N] [--reps 7] [--out profiles/records_bench.jsonl]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import regex_amd as R  # noqa: E402
from golden_data import corpus  # noqa: E402

HBM = 8.0e12
PATTERNS = [r"\d{4}-\d{2}-\d{2}", r"Sherlock|Holmes"]


def timed(fn, warm, reps):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ms.append(s.elapsed_time(e))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    base = torch.from_numpy(np.frombuffer(corpus("sherlock"), dtype=np.uint8).copy()).to(dev)
    n = a.bytes
    text = base.repeat(n // base.numel() + 1)[:n + 16].contiguous()[:n]
    out_file = open(a.out, "w") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out_file:
            out_file.write(line + "\n")
            out_file.flush()

    for pattern in PATTERNS:
        re = R.Regex(pattern)
        info = {}
        rec0, _, nrecords = re.match_records(text, info=info)  # (uploads the tables; sizes the buffers)
        total = info["total"]
        units, chunk = R.Regex.last_records()
        kept = {}

        def records():
            kept["records"] = re.match_records(text, capacity=total)[0].shape[0]

        def records_sized():
            kept["records_sized"] = re.match_records(text)[0].shape[0]

        def two_step():
            nl = (text == 10).nonzero().flatten() + 1
            ends = torch.tensor([n], dtype=torch.int64, device=dev)
            offs = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), nl[nl < n], ends])
            hit = re.is_match_batch(text, offsets=offs)
            kept["two_step"] = hit.nonzero().shape[0]

        variants = [("records", records), ("records_sized", records_sized), ("two_step", two_step)]
        res = {}
        for _ in range(2):  # alternate the variants: two rounds each, the later one kept
            for name, fn in variants:
                res[name] = timed(fn, a.warm, a.reps)
        for name, _ in variants:
            med, lo, hi = res[name]
            emit({"tool": "tools/records_bench.py", "regex": pattern, "variant": name, "bytes": n,
                  "records": nrecords, "selected": kept[name], "units": units, "chunk": chunk, "reps": a.reps,
                  "ms": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4),
                  "GBps": round(n / med / 1e6, 2), "frac_hbm": round(n / (med * 1e-3) / HBM, 4),
                  "speedup_vs_two_step": round(res["two_step"][0] / med, 3)})


if __name__ == "__main__":
    main()
