"""The cooperative score path against the one-wave kernel: one global protein
pair N x N, seq2 a mutated copy of seq1 (tools/bench_band.py's pair and seeded random 24-symbol
table), gaps (12, 1).

For every N: the one-wave kernel (score_matrix_batch), then the cooperative path at forced W = 1, 2,
4, 8 and at the automatic W; one warm-up call and --steps timed calls each (one timed call, no
warm-up, for the one-wave kernel at N >= --single-from): the median, minimum and maximum device time
of the fill kernel (last_stats kernel_ms), W, the items, the edge bytes and the score, which must be
the one-wave kernel's.  One JSON line each; --out appends them to a file.

    python tools/bench_matrix_coop.py [--sizes 8192,16384,32768,65536] [--steps 10] [--mode global]
                                      [--out profiles/matrix_coop.jsonl]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import concurrentproject_amd as sw  # noqa: E402
from bench_band import SYMBOLS, make_pair, random_table  # noqa: E402


def run(call, steps, warm=True):
    if warm:
        call()
    ms, score = [], None
    for _ in range(steps):
        score = call()[0]
        ms.append(sw.last_stats()["kernel_ms"])
    return statistics.median(ms), min(ms), max(ms), score, sw.last_stats()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="8192,16384,32768,65536")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--single-from", type=int, default=65536)
    ap.add_argument("--mode", default="global")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    rng = np.random.default_rng(2024)
    table = random_table(rng)
    lines = []
    with sw.Matrix(SYMBOLS, table) as mx:
        for n in (int(x) for x in args.sizes.split(",") if x):
            pair = make_pair(rng, n)
            base = {"bench": "matrix_coop", "n": n, "m": n, "mode": args.mode, "gaps": [12, 1],
                    "lib": os.path.basename(sw.LIB_PATH), "source": sw.source_stamp()[:16]}
            once = n >= args.single_from
            med, lo, hi, want, st = run(lambda: sw.score_matrix_batch([pair], mx, 12, 1, mode=args.mode),
                                        1 if once else args.steps, warm=not once)
            one = dict(base, path="one_wave", kernel_ms=round(med, 4), kernel_ms_min=round(lo, 4), kernel_ms_max=round(hi, 4),
                       W=st["W"], score=want, gcups=round(st["cells"] / med / 1e6, 3), calls=1 if once else args.steps)
            print(json.dumps(one), flush=True)
            lines.append(one)
            for W in (1, 2, 4, 8, 0):
                sw.set_option("W", W)
                try:
                    med, lo, hi, got, st = run(lambda: sw.score_matrix_batch([pair], mx, 12, 1, mode=args.mode, coop=True),
                                               args.steps)
                    rec = dict(base, path="coop", forced_W=W, kernel_ms=round(med, 4), kernel_ms_min=round(lo, 4),
                               kernel_ms_max=round(hi, 4), W=st["W"], items=st["items"], edge_bytes=st["boundary_bytes"],
                               blocks=st["blocks"], waves_per_cu=st["waves_per_cu"], score=got, same_score=got == want,
                               gcups=round(st["cells"] / med / 1e6, 3), speedup=round(one["kernel_ms"] / med, 2),
                               calls=args.steps)
                except sw.SwError as e:
                    rec = dict(base, path="coop", forced_W=W, result="refused", error=str(e)[:200])
                finally:
                    sw.set_option("W", 0)
                print(json.dumps(rec), flush=True)
                lines.append(rec)
    if args.out:
        with open(args.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")
    return 0 if all(r.get("same_score", True) for r in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
