"""find_iter over one long haystack of a regex past the eager budgets,
`(?:a|b)*a(?:a|b){20}`: a single fixed-stride haystack of 256 KiB to 1 GiB.
The chunked iteration on the on-demand DFA (run_lazy_iter_long,
lazy_iter_long_kernel) answers it; before it existed the Pike VM did, one
wave for the whole haystack (Path.ITER_WAVE), so the same script run on that
commit's build gives the base (--label base --reps 0 --root <that checkout>,
each size in a process of its own under a time limit: it needs about a
second per MiB).

Texts: tools/lazy_long_bench.py's "sparse" (1 % planted a/b runs of 22-30
bytes: about 200 matches per MiB) and "nomatch" (runs of 1-15 bytes: none).

Per size: a fresh Regex; the first call (the automaton, the rounds that build
the rows and links the text needs, the table's upload) and the steady state,
the median of --reps whole find_iter_batch calls each ending in a
synchronise (--reps 0: the first call only); the path, the match count and a
checksum of the records for comparing two builds, and units, rounds,
repaired units and resume passes where the library reports them.  One JSON
line per measurement, appended to --out when given.
usage: python tools/lazy_iter_long_bench.py [--sizes 256K,1M,4M,64M,1G] [--texts sparse,nomatch] [--reps 7]
                                            [--label new] [--root DIR] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAT = r"(?:a|b)*a(?:a|b){20}"
BLOCK = 4 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256K,1M,4M,64M,1G")
    ap.add_argument("--texts", default="sparse,nomatch")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--label", default="new")
    ap.add_argument("--root", default=ROOT, help="the checkout whose built regex_amd package is measured")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.abspath(a.root))
    import numpy as np
    import torch
    import regex_amd as R
    from regex_amd import _native as N
    from golden_data import corpus
    assert os.path.abspath(R.__file__).startswith(os.path.abspath(a.root))

    def parse_size(s):
        return int(s[:-1]) << {"K": 10, "M": 20, "G": 30}[s[-1].upper()]

    def block(kind):
        """tools/lazy_long_bench.py's 4 MiB block"""
        rng = np.random.default_rng(1)
        base = corpus("sherlock")
        lo, hi = (22, 31) if kind == "sparse" else (1, 16)
        parts, total = [], 0
        while total < BLOCK:
            if rng.integers(0, 100) == 0:
                x = bytes(rng.choice(np.frombuffer(b"ab", dtype=np.uint8), size=int(rng.integers(lo, hi))))
            else:
                i = int(rng.integers(0, len(base) - 100))
                x = base[i:i + int(rng.integers(1, 100))]
            parts.append(x)
            total += len(x)
        return np.frombuffer(b"".join(parts)[:BLOCK], dtype=np.uint8)

    dev = torch.device("cuda", 0)
    for kind in a.texts.split(","):
        blk = block(kind)
        for size in (parse_size(s) for s in a.sizes.split(",")):
            host = np.concatenate([np.resize(blk, size), np.zeros(16, dtype=np.uint8)])
            d = torch.from_numpy(host).to(dev)
            del host
            re = R.Regex(PAT)

            def once():
                t0 = time.perf_counter()
                counts, ms = re.find_iter_batch(d, stride=size, length=size, count=1)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3, counts, ms

            first, counts, ms = once()
            path = int(N.rure_amd_last_fwd_path())
            rec = {"label": a.label, "pattern": PAT, "text": kind, "bytes": size, "first_call_ms": round(first, 3),
                   "reps": a.reps, "path": path, "matches": int(counts[0]),
                   "checksum": int((ms.to(torch.int64) * torch.tensor([3, 5], device=dev)).sum() & ((1 << 62) - 1)),
                   "rows_built": re.lazy_tables()[0]["rows_built"]}
            if a.reps:
                steady = statistics.median(once()[0] for _ in range(a.reps))
                rec.update(steady_ms=round(steady, 4), steady_MBps=round(size / steady / 1e3, 2))
            if hasattr(R.Regex, "last_lazy_iter_long"):
                rec.update(R.Regex.last_lazy_iter_long())
            line = json.dumps(rec)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")
            del d, counts, ms


if __name__ == "__main__":
    main()
