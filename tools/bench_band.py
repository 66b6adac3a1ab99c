"""Banded alignment against the whole matrix: one global protein pair N x N,
seq2 a mutated copy of seq1 (8 % substitutions, 1 % single-residue insertions and deletions), under
a seeded random 24-symbol table with gaps (12, 1).

For every N and every band B (and "none": the unbanded call) one warm-up call and ten timed calls,
score-only (score_matrix_batch) and traced (align_matrix_batch): the median device time of the fill
kernel (last_stats kernel_ms), the chosen W, the cells computed and GCUPS over them, the trace bytes
the launch held.  A traced call whose trace is refused (option trace_mb) is reported as "refused".
One JSON line each; --out appends them to a file.

    python tools/bench_band.py [--sizes 8192,16384,32768] [--bands 64,512,2048] [--big 262144 --big-band 1024]
                               [--steps 10] [--out profiles/band.jsonl]

With SWMI355_LIB naming an older build only the unbanded lines are produced (the yardstick)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import concurrentproject_amd as sw  # noqa: E402

SYMBOLS = b"ARNDCQEGHILKMFPSTWYVBZX*"


def random_table(rng):
    t = rng.integers(-4, 4, (24, 24))
    t = np.minimum(t, t.T)
    t[np.arange(24), np.arange(24)] = rng.integers(4, 12, 24)
    return t.astype(np.int32)


def make_pair(rng, n):
    a = np.frombuffer(SYMBOLS, np.uint8)[rng.integers(0, 20, n)]
    out, i = [], 0
    r = rng.random(n)
    sub = np.frombuffer(SYMBOLS, np.uint8)[rng.integers(0, 20, n)]
    for i in range(n):
        if r[i] < 0.005:
            continue                                   # a deletion
        out.append(sub[i] if r[i] < 0.085 else a[i])
        if r[i] > 0.995:
            out.append(sub[(i * 7 + 3) % n])           # an insertion
    b = np.array(out, np.uint8)
    b = np.concatenate([b, sub])[:n]                   # the same length: the band is B on either side
    return a, b


def run(call, steps):
    call()
    ms = []
    for _ in range(steps):
        call()
        ms.append(sw.last_stats()["kernel_ms"])
    return statistics.median(ms), min(ms), max(ms), sw.last_stats()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="8192,16384,32768")
    ap.add_argument("--bands", default="64,512,2048")
    ap.add_argument("--big", type=int, default=0)
    ap.add_argument("--big-band", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    has_band = hasattr(sw.lib(), "sw_align_matrix_batch_band")
    rng = np.random.default_rng(2024)
    table = random_table(rng)
    cases = [(int(n), [None] + [int(b) for b in args.bands.split(",")]) for n in args.sizes.split(",") if n]
    if args.big:
        cases.append((args.big, [args.big_band]))
    lines = []
    with sw.Matrix(SYMBOLS, table) as mx:
        for n, bands in cases:
            pair = make_pair(rng, n)
            for band in bands:
                if band is not None and not has_band:
                    continue
                kw = {} if band is None else {"band": band}
                for what in ("score", "align"):
                    f = sw.score_matrix_batch if what == "score" else sw.align_matrix_batch
                    rec = {"bench": "band", "what": what, "n": n, "m": n, "band": band, "mode": "global", "gaps": [12, 1],
                           "lib": os.path.basename(sw.LIB_PATH)}
                    try:
                        med, lo, hi, st = run(lambda: f([pair], mx, 12, 1, mode="global", **kw), args.steps)
                    except sw.SwError as e:
                        rec.update(result="refused", error=str(e)[:160])
                    else:
                        rec.update(kernel_ms=round(med, 4), kernel_ms_min=round(lo, 4), kernel_ms_max=round(hi, 4), W=st["W"],
                                   cells=st["cells"], gcups=round(st["cells"] / med / 1e6, 3), stats_mode=st["mode"])
                        if what == "align":
                            rec["trace_bytes"] = st["boundary_bytes"]
                            if band is not None:
                                rec["plan_trace_bytes"] = sw.band_plan(n, n, band)["trace_bytes"]
                            rec["walk_ms"] = round(sw.last_align_ms()[1], 4)
                    print(json.dumps(rec), flush=True)
                    lines.append(rec)
    if args.out:
        with open(args.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
