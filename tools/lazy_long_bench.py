"""One long haystack of a regex past the eager budgets,
`(?:a|b)*a(?:a|b){20}`: find / is_match / shortest_match over a single
fixed-stride haystack of 256 KiB to 1 GiB.  The chunked scan on the
on-demand DFA (run_lazy_long, lazy_long_kernel) answers it; before that
scan existed the Pike VM did, one wave for the whole haystack, so the same
script run on that commit gives the base (--label base --reps 1, each size
in a process of its own under a time limit: it needs about a second per
MiB it has to scan).

Texts: "sparse" = sherlock pieces with 1 % planted a/b runs of 22-30 bytes
(tools/lazy_bench.py's): the text holds matches, and every engine stops at
or soon after the first; "nomatch" = the same with runs of 1-15 bytes, which
cannot match, so the whole haystack is scanned.  A 4 MiB block is generated
and repeated up to the size asked for.

Per size and call: a fresh Regex; the first call (the automaton, the rounds
that build the rows and links the text needs, the table's upload) and the
steady state, the median of --reps whole calls each ending in a synchronise;
the path, and units, rounds and rows built where the library reports them.
One JSON line per measurement, appended to --out when given.
usage: python tools/lazy_long_bench.py [--sizes 256K,1M,4M,64M,1G] [--texts sparse,nomatch]
                                       [--modes find,is_match,shortest] [--reps 7] [--label new] [--out FILE]"""
import argparse
import json
import os
import statistics
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

PAT = r"(?:a|b)*a(?:a|b){20}"
BLOCK = 4 << 20


def parse_size(s):
    return int(s[:-1]) << {"K": 10, "M": 20, "G": 30}[s[-1].upper()]


def block(kind):
    rng = np.random.default_rng(1)
    base = corpus("sherlock")
    lo, hi = (22, 31) if kind == "sparse" else (1, 16)
    parts, total = [], 0
    while total < BLOCK:
        if rng.integers(0, 100) == 0:
            x = bytes(rng.choice(np.frombuffer(b"ab", dtype=np.uint8), size=int(rng.integers(lo, hi))))
        else:
            a = int(rng.integers(0, len(base) - 100))
            x = base[a:a + int(rng.integers(1, 100))]
        parts.append(x)
        total += len(x)
    return np.frombuffer(b"".join(parts)[:BLOCK], dtype=np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256K,1M,4M,64M,1G")
    ap.add_argument("--texts", default="sparse,nomatch")
    ap.add_argument("--modes", default="find,is_match,shortest")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--label", default="new")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    for kind in a.texts.split(","):
        blk = block(kind)
        for size in (parse_size(s) for s in a.sizes.split(",")):
            host = np.concatenate([np.resize(blk, size), np.zeros(16, dtype=np.uint8)])
            d = torch.from_numpy(host).to(dev)
            del host
            for mode in a.modes.split(","):
                re = R.Regex(PAT)
                call = {"find": re.find_batch, "is_match": re.is_match_batch,
                        "shortest": re.shortest_match_batch}[mode]

                def once():
                    t0 = time.perf_counter()
                    out = call(d, stride=size, length=size, count=1)
                    torch.cuda.synchronize()
                    return (time.perf_counter() - t0) * 1e3, out

                first, out = once()
                steady = statistics.median(once()[0] for _ in range(a.reps))
                rec = {"label": a.label, "pattern": PAT, "text": kind, "bytes": size, "mode": mode,
                       "first_call_ms": round(first, 3), "steady_ms": round(steady, 4), "reps": a.reps,
                       "steady_GBps": round(size / steady / 1e6, 3), "path": int(N.rure_amd_last_fwd_path()),
                       "result": [int(x) for x in out.cpu().numpy().reshape(-1)],
                       "rows_built": re.lazy_tables()[0]["rows_built"]}
                if hasattr(R.Regex, "last_lazy_long"):
                    units, _, chunk, rounds, fell_back = R.Regex.last_lazy_long()
                    rec.update(units=units, chunk=chunk, steady_rounds=rounds, fell_back=fell_back)
                line = json.dumps(rec)
                print(line, flush=True)
                if a.out:
                    with open(a.out, "a") as f:
                        f.write(line + "\n")
            del d


if __name__ == "__main__":
    main()
