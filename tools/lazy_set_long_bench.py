"""One long haystack of a RegexSet past the eager state budget (the set of
tools/lazy_set_bench.py): matches_batch over a single fixed-stride haystack of
256 KiB to 1 GiB.  The chunked scan on the set's on-demand DFA
(run_lazy_set_long, lazy_set_long_kernel) answers it; before that scan existed
the Pike VM did, one wave for the whole haystack, so the same script run on
that commit gives the base (--label base --reps 1 --package-root <its tree>,
each size in a process of its own under a time limit: a set's Pike VM scans
the whole haystack whatever it finds).

Texts as tools/lazy_long_bench.py: "sparse" = sherlock pieces with 1 %
planted a/b runs of 22-30 bytes (the long pattern matches); "nomatch" = the
same with runs of 1-15 bytes (it never does).  A 4 MiB block is generated and
repeated up to the size asked for.

Per size: a fresh RegexSet; the first call (the automaton, the rounds that
build the rows and links the text needs, the table's upload) and the steady
state, the median of --reps whole calls each ending in a synchronise; the
mask, the path, and units, rounds and rows built where the library reports
them.  One JSON line per measurement, appended to --out when given.
usage: python tools/lazy_set_long_bench.py [--sizes 256K,1M,4M,64M,1G] [--texts sparse,nomatch] [--reps 7]
                                           [--label new] [--out FILE] [--package-root DIR]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256K,1M,4M,64M,1G")
    ap.add_argument("--texts", default="sparse,nomatch")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--label", default="new")
    ap.add_argument("--out", default=None)
    ap.add_argument("--package-root", default=ROOT, help="the tree regex_amd is imported from (another build: the base)")
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.abspath(a.package_root))
    import numpy as np
    import torch

    import regex_amd as R
    from regex_amd import _native as N
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from lazy_long_bench import block, parse_size

    pats = [r"(?:a|b)*a(?:a|b){20}", r"Sherlock|Holmes", r"^[A-Z][a-z]+ ", r"(?-u)\d+"]
    dev = torch.device("cuda", 0)
    for kind in a.texts.split(","):
        blk = block(kind)
        for size in (parse_size(s) for s in a.sizes.split(",")):
            host = np.concatenate([np.resize(blk, size), np.zeros(16, dtype=np.uint8)])
            d = torch.from_numpy(host).to(dev)
            del host
            rs = R.RegexSet(pats)
            assert not rs.uses_dfa()

            def once():
                t0 = time.perf_counter()
                out = rs.matches_batch(d, stride=size, length=size, count=1)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3, out

            first, out = once()
            info1 = rs.lazy_tables()[0]
            steady = statistics.median(once()[0] for _ in range(a.reps))
            info = rs.lazy_tables()[0]
            units, _, chunk = R.RegexSet.last_long_units()
            rec = {"label": a.label, "patterns": pats, "text": kind, "bytes": size,
                   "first_call_ms": round(first, 3), "steady_ms": round(steady, 4), "reps": a.reps,
                   "steady_GBps": round(size / steady / 1e6, 3), "path": int(N.rure_amd_last_fwd_path()),
                   "mask": int(out.cpu().numpy().reshape(-1)[0]), "units": units, "chunk": chunk,
                   "first_call_rounds": info1["rounds"], "steady_rounds": info["rounds"],
                   "fell_back": info["fell_back"], "states": info["states"], "rows_built": info["rows_built"]}
            line = json.dumps(rec)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")
            del d


if __name__ == "__main__":
    main()
