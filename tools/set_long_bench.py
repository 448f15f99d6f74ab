"""RegexSet over one long haystack: the chunked scan (set_long.hip, the
default from 256 KiB) against one lane per haystack (debug knob set_long=0,
the path before the chunked scan existed), on log text of 256 KiB to 1 GiB.

Sets: the 64-pattern C4 set (its Unicode word boundaries make its DFA
quit-capable, so it keeps its lane under either setting), the same set with
ASCII word boundaries (the large set that chunks), and a 4-literal set.
The text is 16 MiB of the C4 log stream, tiled.  Each setting: warm-up calls,
then the median of event-timed calls, the stream synchronised around each;
the two settings alternate per size, and their masks are compared.  A lane
run that would exceed --lane-limit seconds (extrapolated from the size
before) is skipped and recorded as such.  One JSON line per (set, size,
setting); `frac_hbm` = bytes / time over 8 TB/s.
usage: python tools/set_long_bench.py [--lane-limit 60] [--sizes KiB,KiB,...] [--out file.jsonl]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import regex_amd as R  # noqa: E402
from regex_amd.workloads import C4_PATTERNS, log_lines_device  # noqa: E402

HBM = 8.0e12
SIZES = [256 << 10, 1 << 20, 16 << 20, 256 << 20, 1 << 30]
SETS = {
    "c4": C4_PATTERNS,
    "c4_ascii_wb": [p.replace(r"\b", r"(?-u:\b)") for p in C4_PATTERNS],
    "lit4": ["ERROR", "status=404", "oom", "kernel"],
}


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
    ap.add_argument("--lane-limit", type=float, default=60.0, help="skip a set_long=0 run predicted to take longer (s)")
    ap.add_argument("--sizes", default=None, help="haystack sizes in KiB, comma separated (default: 256 KiB .. 1 GiB)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sizes = [int(x) << 10 for x in a.sizes.split(",")] if a.sizes else SIZES
    dev = torch.device("cuda:0")
    base, _ = log_lines_device((16 << 20) // 160 + 1, dev, lo=160, hi=160)
    base = base[:16 << 20]
    text = base.repeat(max(sizes) // base.numel() + 1)[:max(sizes) + 16].contiguous()
    out_file = open(a.out, "w") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out_file:
            out_file.write(line + "\n")
            out_file.flush()

    for name, pats in SETS.items():
        rs = R.RegexSet(pats)
        lane_ms = None  # the last one-lane time, and its size
        chunks = True   # the default setting chunks this set (known after its first run)
        for size in sizes:
            res = {}
            for setting in ("default", "set_long=0"):
                rec = {"tool": "tools/set_long_bench.py", "set": name, "patterns": len(pats), "bytes": size,
                       "knobs": setting}
                R._debug_set(None if setting == "default" else setting)
                out = torch.empty(1, dtype=torch.int64, device=dev)
                call = lambda: rs.matches_batch(text, stride=size, length=size, count=1, out=out)  # noqa: E731
                lanes = setting != "default" or not chunks
                if lanes and lane_ms is not None and lane_ms[0] * size / lane_ms[1] > a.lane_limit * 1e3:
                    rec.update(skipped="one lane per haystack: %.0f s predicted from %.1f ms at %d bytes"
                               % (lane_ms[0] * size / lane_ms[1] / 1e3, lane_ms[0], lane_ms[1]))
                    emit(rec)
                    continue
                call()  # (the first call builds and uploads the automaton)
                torch.cuda.synchronize()
                units, _, chunk = R.RegexSet.last_long_units()
                if setting == "default":
                    chunks = units > 0
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                call()
                e.record()
                torch.cuda.synchronize()
                one = s.elapsed_time(e)
                reps = 20 if one < 50 else 5 if one < 1000 else 1
                med, lo, hi = (one, one, one) if reps == 1 else timed(call, 2, reps)
                if units == 0:
                    lane_ms = (med, size)
                res[setting] = int(out.item())
                rec.update(ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4), reps=reps, units=units,
                           chunk=chunk, GBps=round(size / med / 1e6, 2), frac_hbm=round(size / (med * 1e-3) / HBM, 4),
                           mask="%016x" % (res[setting] & (2 ** 64 - 1)))
                if len(res) == 2:
                    rec["masks_equal"] = res["default"] == res["set_long=0"]
                emit(rec)
    R._debug_set(None)


if __name__ == "__main__":
    main()
