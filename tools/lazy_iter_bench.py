"""Regex.find_iter_batch of a regex past the eager state budget,
`(?:a|b)*a(?:a|b){20}`, over sherlock lines with 1 % planted a/b runs
(tools/lazy_bench.py's "sparse" text): the first call (on the on-demand DFA:
the rounds that build the rows the text needs), then steady state, then the
same batch with lazy=0 (the Pike VM, one wavefront per haystack:
Path.ITER_WAVE) as a cross-check, then prefixes of the batch from 64 to 64
haystacks per CU under big=2, for the batch size from which the on-demand
DFA wins.  The base of the comparison is this script run on a build of the
commit before lazy_iter_kernel, where every line's path reads ITER_WAVE; the
`crc` fields of the two builds must agree.  Whole calls ending in a
synchronise; medians of 7.  Prints one JSON line per measurement.
usage: python tools/lazy_iter_bench.py [haystacks] [length] [label]"""
import json
import os
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import regex_amd as R
from regex_amd import _native as N
from golden_data import corpus

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 18
L = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
LABEL = sys.argv[3] if len(sys.argv) > 3 else "this build"
PAT = r"(?:a|b)*a(?:a|b){20}"
rng = np.random.default_rng(1)
base = corpus("sherlock")
parts, total = [], 0
while total < n * L:
    if rng.integers(0, 100) == 0:
        x = bytes(rng.choice(np.frombuffer(b"ab", dtype=np.uint8), size=int(rng.integers(22, 31))))
    else:
        a = int(rng.integers(0, len(base) - 100))
        x = base[a:a + int(rng.integers(1, 100))]
    parts.append(x)
    total += len(x)
raw = b"".join(parts)[:n * L]
dev = torch.device("cuda", 0)
d = torch.from_numpy(np.frombuffer(raw + b"\0" * 16, dtype=np.uint8).copy()).to(dev)
cus = torch.cuda.get_device_properties(0).multi_processor_count


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def median_ms(fn, reps=7):
    fn()  # warm: every shape the window uses
    return float(np.median([once(fn)[0] for _ in range(reps)]))


def line(**kw):
    print(json.dumps(dict({"build": LABEL, "pattern": PAT, "length": L, "cus": cus}, **kw)), flush=True)


def crc(out):
    counts, ms = out
    return zlib.crc32(ms.cpu().numpy().tobytes(), zlib.crc32(counts.cpu().numpy().tobytes()))


def lazy_info(re):
    """rounds and rows of the on-demand DFA (a build without it: none)"""
    if not hasattr(re, "lazy_tables"):
        return {}
    i = re.lazy_tables()[0]
    return dict(rounds=i["rounds"], states=i["states"], rows_built=i["rows_built"], hot_rows=i["hot_rows"],
                fell_back=i["fell_back"])


# the default dispatch (no knob) on the full batch: first call, steady state
R._debug_set(None)
re = R.Regex(PAT)
assert not re.uses_dfa()
first_ms, out = once(lambda: re.find_iter_batch(d, stride=L, length=L, count=n))
path = int(N.rure_amd_last_fwd_path())
info = lazy_info(re)
matches = int(out[1].shape[0])
cap = max(matches, 1)  # (the exact capacity: one pass per call)
full_crc = crc(out)
steady = median_ms(lambda: re.find_iter_batch(d, stride=L, length=L, count=n, capacity=cap))
line(what="default dispatch", haystacks=n, first_call_ms=round(first_ms, 1), first_call=info,
     steady_ms=round(steady, 3), steady_GBps=round(n * L / steady / 1e6, 1), steady=lazy_info(re), path=path,
     matches=matches, haystacks_matching=int((out[0] != 0).sum().item()), crc=full_crc)

# the cross-check: the same batch with lazy=0 (the Pike VM on any build)
R._debug_set("lazy=0")
rp = R.Regex(PAT)
pike_first, out = once(lambda: rp.find_iter_batch(d, stride=L, length=L, count=n, capacity=cap))
ppath = int(N.rure_amd_last_fwd_path())
pike = median_ms(lambda: rp.find_iter_batch(d, stride=L, length=L, count=n, capacity=cap), 3)
line(what="lazy=0", haystacks=n, first_call_ms=round(pike_first, 1), steady_ms=round(pike, 2),
     steady_GBps=round(n * L / pike / 1e6, 2), path=ppath, outputs_equal=bool(crc(out) == full_crc))

# prefixes of the batch under big=2 (the on-demand DFA at any count, its
# table as the full batch left it; the base build: the Pike VM)
R._debug_set("big=2")
for c in sorted({64, 256, 1024, 4096, cus * 16, cus * 64}):
    if c > n:
        continue
    out = re.find_iter_batch(d, stride=L, length=L, count=c)
    k = max(int(out[1].shape[0]), 1)
    ms = median_ms(lambda: re.find_iter_batch(d, stride=L, length=L, count=c, capacity=k))
    line(what="prefix, big=2", haystacks=c, ms=round(ms, 4), path=int(N.rure_amd_last_fwd_path()),
         matches=int(out[1].shape[0]), crc=crc(out), default_takes_lazy=bool(c >= cus * 64))
R._debug_set(None)
