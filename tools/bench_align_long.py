"""Long pairs by checkpointed traceback (sw_align_matrix_long): what one pair costs.

One protein pair of N x N residues under a seeded random 24-symbol table, gaps (12, 1):

  --kind crossing   seq2 is a mutated copy of seq1 (6 % substitutions, a few short insertions and deletions
                    every 80 residues), so the alignment crosses every strip: the worst case, N / 512 rounds
  --kind random     seq2 is random: a short alignment, one or two rounds

One step (--n N --kind K) prints one JSON line: the locate, strip-fill and walk milliseconds, the rounds,
boundary_bytes, the plan (sw_align_long_plan), the time of sw_score_matrix on the same pair and, with --check
(N = 8192 in the default run), the time of sw_align_matrix_batch and whether the three aligners agree
(align_matrix_long == align_matrix_batch == the CPU aligner).

Without --n: the whole series, N = 8192, 16384, 32768, both kinds, every step a fresh child process under a
time limit of its own; the first step that fails or runs out of time ends the series (nothing more is started
on the GPU after it).  Lines are appended to --out (default profiles/align_long.jsonl).

--coop runs sw_align_matrix_long_coop instead (the locate pass on many waves, a window of strips a round;
DESIGN.md section 17), --window G with option long_window = G (0: automatic).  --reps R (default 1) times R
calls after the warm-up: the line then carries the median of every device time and, as *_min / *_max, their
range.  Every line carries a digest of the alignment, so that runs can be compared.

--series-coop: the series of DESIGN.md section 17: N = 8192, 16384, 32768, both kinds, each as the baseline
(align_matrix_long), --coop automatic and --coop --window 1, 4, 16, five timed calls each, a fresh child
process a step as above; the series fails when a digest differs from its baseline's.  Lines are appended to
--out (default then profiles/align_long_coop.jsonl).

--mode global|semiglobal (default local) runs the step through sw_align_matrix_long_mode /
sw_align_matrix_long_coop_mode; the score, the whole-trace alignment and the CPU
alignment it is compared with are then those of that mode.

--series-modes: the series of DESIGN.md section 18: the crossing pair at N = 8192, 16384, 32768 in every mode
(local first: the unchanged code, in the same session), each on one wave, --coop automatic and --coop
--window 16, three timed calls each, and at N = 8192 one --check step a mode (the whole-trace path and the CPU
aligner); a fresh child process a step as above.  Lines are appended to --out (default then
profiles/align_long_modes.jsonl).

    python tools/bench_align_long.py [--out FILE] [--limit SECONDS]
    python tools/bench_align_long.py --n 8192 --kind crossing [--check] [--coop [--window G]] [--reps R] [--mode M]
    python tools/bench_align_long.py --series-coop [--out FILE] [--limit SECONDS]
    python tools/bench_align_long.py --series-modes [--out FILE] [--limit SECONDS]
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SYMBOLS = b"ARNDCQEGHILKMFPSTWYVBZX*"


def make_pair(n, kind):
    rng = np.random.default_rng(n + (1 if kind == "crossing" else 2))
    sym = np.frombuffer(SYMBOLS, np.uint8)
    a = sym[rng.integers(0, 23, n)]
    if kind == "random":
        return a, sym[rng.integers(0, 23, n)]
    b = a.copy()
    sub = rng.random(n) < 0.06
    b[sub] = sym[rng.integers(0, 23, int(sub.sum()))]
    for at in sorted((int(x) for x in rng.integers(1, n - 1, n // 80)), reverse=True):
        k = int(rng.integers(1, 4))
        b = np.delete(b, slice(at, at + k)) if rng.random() < 0.5 else np.insert(b, at, sym[rng.integers(0, 23, k)])
    b = b[:n]
    return a, np.concatenate([b, sym[rng.integers(0, 23, n - len(b))]])


def table():
    rng = np.random.default_rng(24)
    t = rng.integers(-4, 4, (24, 24))
    t = np.minimum(t, t.T)
    t[np.arange(24), np.arange(24)] = rng.integers(4, 12, 24)
    return t.astype(np.int8)


def step(n, kind, check, coop=False, window=0, reps=1, mode="local"):
    import concurrentproject_amd as sw
    a, b = make_pair(n, kind)
    rec = {"what": "align_long_coop" if coop else "align_long", "n": n, "m": len(b), "kind": kind, "gaps": [12, 1],
           "stamp": sw.source_stamp()[:12], "align_mode": mode}
    with sw.Matrix(SYMBOLS, table()) as mx:
        if coop:
            sw.set_option("long_window", window)
            rec.update(long_window=window, plan=sw.align_long_coop_plan(n, len(b)))
        else:
            rec["plan"] = sw.align_long_plan(n, len(b))
        sw.align_matrix_long([(a[:600], b[:600])], mx, 12, 1, coop=coop, mode=mode)   # loads the kernels, allocates the context
        if reps > 1:
            sw.align_matrix_long([(a, b)], mx, 12, 1, coop=coop, mode=mode)           # the warm-up call of a timed series
        runs = []
        for _ in range(reps):
            t0 = time.perf_counter()
            x = sw.align_matrix_long([(a, b)], mx, 12, 1, coop=coop, mode=mode)[0]
            ms = dict(sw.last_align_long_ms(), call_ms=(time.perf_counter() - t0) * 1e3)
            ms["device_ms"] = ms["locate_ms"] + ms["strip_ms"] + ms["walk_ms"]
            runs.append(ms)
        st = sw.last_stats()
        for key in ("call_ms", "locate_ms", "strip_ms", "walk_ms", "device_ms"):
            v = sorted(r[key] for r in runs)
            rec[key] = round(float(np.median(v)), 3)
            if reps > 1:
                rec[key + "_min"], rec[key + "_max"] = round(v[0], 3), round(v[-1], 3)
        ms = runs[-1]
        rec.update(reps=reps, rounds=ms["rounds"], strip_launches=st["variant"] & 0xFFFFFFF, boundary_bytes=st["boundary_bytes"],
                   mode=st["mode"], items=st["items"],
                   score=x.score, beg1=x.beg1, end1=x.end1, beg2=x.beg2, end2=x.end2, cigar_entries=len(x.ops),
                   digest=hashlib.sha1(repr(x).encode()).hexdigest()[:16],
                   locate_gcups=round(n * len(b) / max(rec["locate_ms"], 1e-9) / 1e6, 3))
        if reps > 1:      # a timed series: the device times only
            print(json.dumps(rec), flush=True)
            return 0
        sw.score_matrix(a[:600], b[:600], mx, 12, 1, mode=mode)
        t0 = time.perf_counter()
        s = sw.score_matrix(a, b, mx, 12, 1, mode=mode)
        rec["score_call_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        st = sw.last_stats()
        rec.update(score_kernel_ms=round(st["kernel_ms"], 3), score_W=st["W"], score_same=bool(s == x.score))
        if check:
            sw.align_matrix_batch([(a[:600], b[:600])], mx, 12, 1, mode=mode)
            t0 = time.perf_counter()
            y = sw.align_matrix_batch([(a, b)], mx, 12, 1, mode=mode)[0]
            rec["batch_call_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
            fill, walk = sw.last_align_ms()
            rec.update(batch_fill_ms=round(fill, 3), batch_walk_ms=round(walk, 3),
                       batch_trace_bytes=sw.last_stats()["boundary_bytes"], equals_batch=bool(x == y))
            t0 = time.perf_counter()
            z = sw.align_matrix_batch([(a, b)], mx, 12, 1, cpu=True, mode=mode)[0]
            rec["cpu_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            rec["equals_cpu"] = bool(x == z)
    print(json.dumps(rec), flush=True)
    return 0 if rec["score_same"] and rec.get("equals_batch", True) and rec.get("equals_cpu", True) else 4


def series(out, limit):
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    for n in (8192, 16384, 32768):
        for kind in ("crossing", "random"):
            cmd = [sys.executable, os.path.abspath(__file__), "--n", str(n), "--kind", kind] + (["--check"] if n == 8192 else [])
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
            except subprocess.TimeoutExpired:
                print("bench_align_long: %d %s ran past %d s; stopping" % (n, kind, limit), file=sys.stderr)
                return 124
            sys.stderr.write(r.stderr[-2000:])
            if r.returncode != 0:
                print("bench_align_long: %d %s failed (%d); stopping" % (n, kind, r.returncode), file=sys.stderr)
                return r.returncode
            line = r.stdout.strip().split("\n")[-1]
            print(line, flush=True)
            with open(out, "a") as f:
                f.write(line + "\n")
    return 0


def series_coop(out, limit):
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    for n in (8192, 16384, 32768):
        for kind in ("crossing", "random"):
            base = None
            for extra in ([], ["--coop"], ["--coop", "--window", "1"], ["--coop", "--window", "4"], ["--coop", "--window", "16"]):
                cmd = [sys.executable, os.path.abspath(__file__), "--n", str(n), "--kind", kind, "--reps", "5"] + extra
                try:
                    r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
                except subprocess.TimeoutExpired:
                    print("bench_align_long: %d %s %s ran past %d s; stopping" % (n, kind, extra, limit), file=sys.stderr)
                    return 124
                sys.stderr.write(r.stderr[-2000:])
                if r.returncode != 0:
                    print("bench_align_long: %d %s %s failed (%d); stopping" % (n, kind, extra, r.returncode), file=sys.stderr)
                    return r.returncode
                line = r.stdout.strip().split("\n")[-1]
                print(line, flush=True)
                with open(out, "a") as f:
                    f.write(line + "\n")
                digest = json.loads(line)["digest"]
                base = base or digest
                if digest != base:
                    print("bench_align_long: %d %s %s: another alignment than the baseline's; stopping" % (n, kind, extra),
                          file=sys.stderr)
                    return 4
    return 0


def series_modes(out, limit):
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    for n in (8192, 16384, 32768):
        for mode in ("local", "global", "semiglobal"):
            base = None
            steps = [["--reps", "3"], ["--reps", "3", "--coop"], ["--reps", "3", "--coop", "--window", "16"]]
            for extra in steps + ([["--check"]] if n == 8192 else []):
                cmd = [sys.executable, os.path.abspath(__file__), "--n", str(n), "--kind", "crossing", "--mode", mode] + extra
                try:
                    r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
                except subprocess.TimeoutExpired:
                    print("bench_align_long: %d %s %s ran past %d s; stopping" % (n, mode, extra, limit), file=sys.stderr)
                    return 124
                sys.stderr.write(r.stderr[-2000:])
                if r.returncode != 0:
                    print("bench_align_long: %d %s %s failed (%d); stopping" % (n, mode, extra, r.returncode), file=sys.stderr)
                    return r.returncode
                line = r.stdout.strip().split("\n")[-1]
                print(line, flush=True)
                with open(out, "a") as f:
                    f.write(line + "\n")
                digest = json.loads(line)["digest"]
                base = base or digest
                if digest != base:
                    print("bench_align_long: %d %s %s: another alignment than the one-wave path's; stopping" % (n, mode, extra),
                          file=sys.stderr)
                    return 4
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=0)
    ap.add_argument("--kind", default="crossing", choices=("crossing", "random"))
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--coop", action="store_true", help="sw_align_matrix_long_coop")
    ap.add_argument("--window", type=int, default=0, help="with --coop: option long_window (0: automatic)")
    ap.add_argument("--reps", type=int, default=1, help="timed calls after a warm-up call: medians and ranges")
    ap.add_argument("--series-coop", action="store_true", help="baseline against --coop, DESIGN.md section 17")
    ap.add_argument("--mode", default="local", choices=("local", "global", "semiglobal"), help="the alignment mode of a step")
    ap.add_argument("--series-modes", action="store_true", help="every mode on both long paths, DESIGN.md section 18")
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=150, help="seconds a step of the series may take")
    a = ap.parse_args()
    if a.window and not a.coop:
        ap.error("--window goes with --coop")
    if a.n:
        return step(a.n, a.kind, a.check, a.coop, a.window, a.reps, a.mode)
    if a.series_modes:
        return series_modes(a.out or os.path.join(ROOT, "profiles", "align_long_modes.jsonl"), a.limit)
    if a.series_coop:
        return series_coop(a.out or os.path.join(ROOT, "profiles", "align_long_coop.jsonl"), a.limit)
    return series(a.out or os.path.join(ROOT, "profiles", "align_long.jsonl"), a.limit)


if __name__ == "__main__":
    sys.exit(main())
