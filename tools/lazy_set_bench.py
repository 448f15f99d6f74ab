"""RegexSet.matches_batch on the set's on-demand DFA (host LazyDfa over the
set program + lazy_set_kernel) for a set past the eager state budget, over
sherlock lines with 1 % planted a/b runs (tools/lazy_bench.py's "sparse"
text): the first call (the rounds that build the rows the text needs), then
steady state (one round), against the same batch with lazy=0, which is the
Pike VM (Path.PIKE_ONLY), the only engine such a set had before.  Then the
same comparison over smaller batches (prefixes of the text), for the batch
size from which the on-demand DFA wins.  Whole calls ending in a
synchronise; medians.  Prints one JSON line per measurement.
usage: python tools/lazy_set_bench.py [haystacks] [length]"""
import json
import os
import sys
import time

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
PATS = [r"(?:a|b)*a(?:a|b){20}", r"Sherlock|Holmes", r"^[A-Z][a-z]+ ", r"(?-u)\d+"]
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


def median_ms(fn, reps):
    fn()  # warm: every shape the window uses
    return float(np.median([once(fn)[0] for _ in range(reps)]))


def line(**kw):
    print(json.dumps(dict({"patterns": PATS, "length": L, "cus": cus}, **kw)), flush=True)


# the default dispatch (no knob) on the full batch: first call, steady state
R._debug_set(None)
rs = R.RegexSet(PATS)
assert not rs.uses_dfa()
first_ms, out = once(lambda: rs.matches_batch(d, stride=L, length=L, count=n))
path = int(N.rure_amd_last_fwd_path())
info = rs.lazy_tables()[0]
steady = median_ms(lambda: rs.matches_batch(d, stride=L, length=L, count=n), 7)
info2 = rs.lazy_tables()[0]
lazy_out = out.cpu().numpy()
line(what="on-demand DFA, default dispatch", haystacks=n, first_call_ms=round(first_ms, 1),
     first_call_rounds=info["rounds"], steady_ms=round(steady, 3), steady_GBps=round(n * L / steady / 1e6, 1),
     steady_rounds=info2["rounds"], path=path, states=info2["states"], rows_built=info2["rows_built"],
     hot_rows=info2["hot_rows"], fell_back=info2["fell_back"])

# the base: the same batch with lazy=0 (the Pike VM, the parent's path)
R._debug_set("lazy=0")
rp = R.RegexSet(PATS)
pike_first, out = once(lambda: rp.matches_batch(d, stride=L, length=L, count=n))
ppath = int(N.rure_amd_last_fwd_path())
pike = median_ms(lambda: rp.matches_batch(d, stride=L, length=L, count=n), 3)
same = bool((out.cpu().numpy() == lazy_out).all())
line(what="Pike VM (lazy=0), the base", haystacks=n, first_call_ms=round(pike_first, 1), steady_ms=round(pike, 2),
     steady_GBps=round(n * L / pike / 1e6, 2), path=ppath, outputs_equal=same,
     haystacks_matching=int((lazy_out != 0).sum()))

# the crossover: prefixes of the batch, the table as the full batch left it
# (big=2 takes the on-demand DFA at any count; lazy=0 the Pike VM)
for c in (64, 256, 1024, 4096, cus * 16, cus * 64, cus * 256):
    if c > n:
        continue
    R._debug_set("big=2")
    a = median_ms(lambda: rs.matches_batch(d, stride=L, length=L, count=c), 7)
    pa = int(N.rure_amd_last_fwd_path())
    R._debug_set("lazy=0")
    b = median_ms(lambda: rp.matches_batch(d, stride=L, length=L, count=c), 5)
    line(what="crossover", haystacks=c, lazy_ms=round(a, 4), pike_ms=round(b, 4), lazy_path=pa,
         default_takes_lazy=bool(c >= cus * 64))
R._debug_set(None)
