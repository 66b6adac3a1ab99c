"""Database-search rate (f-4): one query against a synthetic FASTA of ragged DNA (or protein) records.

Times ``Database.search`` (sw_db_search, synchronous: query H2D + one batch launch over every record + score D2H),
so the figure is host-API GCUPS, not kernel-only.  Records are uniform ACGT with lengths drawn uniformly from
[lo, hi]; the arena is uploaded to HBM by the first (untimed) search.  --alphabet protein: uniform over
the 20 amino-acid letters (SwissProt-style; the engine's byte path, duo kernels with option duo_raw = 1).

--matrix random|FILE --gaps G_INIT,G_EXT: the same search under a substitution matrix (sw_db_search_matrix, the
wave-per-pair kernel of sw_matrix.hip): FILE in the NCBI text format, or "random": a seeded random table over the
alphabet's letters with diagonal entries in [4, 11] and off-diagonal entries in [-4, 3].

--alignments K (with --matrix): a second line: the search plus aligning its top K (Database.top(alignments=True):
sw_db_align_matrix, the traced kernel and the walk) next to the search alone, the traced kernel against the
score-only kernel at the same W on those K pairs, the walk's time and the trace bytes.  --plant P replaces P records
by mutated copies of the query, so that the top hits have real alignments (with neither, nothing changes).

--mode global|semiglobal (with --matrix): the same search, alignments and timings in that alignment mode
(Database.search(mode=...)); the lines then carry "align_mode".

--profile (with --matrix): a further line: the search with Profile.from_matrix(matrix, query) (sw_db_search_profile, the
PROFILE instantiations of sw_matrix.hip) against the matrix search of the same query, alternated three times, --steps
searches each after one warm-up: both times, their ratio, W and the resident waves per CU of each, and whether the scores
are equal (they must be).

--translated (with --matrix): instead of all the above, the translated search (Database.search_translated, the XLATE
instantiations of sw_matrix.hip) of a random protein query against R DNA records of 3 * lo to 3 * hi bases, and its
yardstick: the existing matrix search of the same query over a protein database that holds the six host-translated
frames of the same records -- the same items, cells and W.  Alternated three times, --steps searches each after one
warm-up; one line with both times, the kernel times, the ratios and whether the scores are equal (they must be).

    python tools/bench_db.py [--records R] [--qlen Q] [--lo L] [--hi H] [--steps K] [--alphabet dna|protein]
                             [--opt k=v ...] [--matrix random|FILE --gaps G_INIT,G_EXT] [--alignments K] [--plant P]
                             [--mode local|global|semiglobal] [--profile] [--translated]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from concurrentproject_amd.db import Database  # noqa: E402


def translated(a):
    import concurrentproject_amd as sw
    for kv in a.opt:
        k, v = kv.split("=")
        sw.set_option(k, int(v))
    rng = np.random.default_rng(4)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    aa = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
    lens = rng.integers(3 * a.lo, 3 * a.hi + 1, size=a.records)
    recs = [acgt[rng.integers(0, 4, size=n)] for n in lens]
    q = aa[rng.integers(0, 20, size=a.qlen)]
    if a.matrix == "random":   # over the amino acids and what else the code emits: 'X' and '*'
        trng = np.random.default_rng(62)
        sym = aa.tobytes() + b"X*"
        tab = trng.integers(-4, 4, (22, 22))
        tab[np.arange(22), np.arange(22)] = trng.integers(4, 12, 22)
        mx = sw.Matrix(sym, tab)
    else:
        mx = sw.Matrix.open(a.matrix)
    gi, ge = (int(x) for x in a.gaps.split(","))
    dna = Database.from_fasta(b"".join(b">r%d\n" % i + r.tobytes() + b"\n" for i, r in enumerate(recs)))
    frames = Database.from_fasta(b"".join(b">r%d%+d\n" % (i, f) + sw.translate(r, f) + b"\n"
                                          for i, r in enumerate(recs) for f in sw.FRAMES))
    runs = {"translated": lambda: dna.search_translated(q, mx, gi, ge, mode=a.mode).reshape(-1),
            "frames": lambda: frames.search(q, matrix=mx, gap_init=gi, gap_ext=ge, mode=a.mode)}
    ms = {k: [] for k in runs}
    kms = {k: [] for k in runs}
    stats, equal, ref = {}, True, None
    for _ in range(3):
        for which in ("frames", "translated"):
            got = runs[which]()   # warm
            ref = got if ref is None else ref
            equal = equal and got.tolist() == ref.tolist()
            k = []
            t0 = time.perf_counter()
            for _ in range(a.steps):
                runs[which]()
                k.append(sw.last_stats()["kernel_ms"])
            ms[which].append(round((time.perf_counter() - t0) / a.steps * 1e3, 3))
            kms[which].append(round(float(np.median(k)), 3))
            stats[which] = sw.last_stats()
    cells = stats["translated"]["cells"]
    launch = lambda st: {"mode": st["mode"], "W": st["W"], "waves_per_cu": st["waves_per_cu"], "blocks": st["blocks"],
                         "cells": st["cells"]}
    print(json.dumps({"metric": "db translated search against the matrix search of the six translated frames (host API, alternated)",
                      "matrix": a.matrix, "gaps": [gi, ge], "align_mode": a.mode, "records": a.records, "qlen": a.qlen,
                      "dna_len_range": [3 * a.lo, 3 * a.hi], "bases": int(lens.sum()), "steps": a.steps,
                      "frames_ms_per_search": ms["frames"], "translated_ms_per_search": ms["translated"],
                      "frames_kernel_ms": kms["frames"], "translated_kernel_ms": kms["translated"],
                      "ratio_translated_over_frames": round(float(np.median(ms["translated"])) / float(np.median(ms["frames"])), 3),
                      "kernel_ratio_translated_over_frames": round(float(np.median(kms["translated"])) / float(np.median(kms["frames"])), 3),
                      "frames_launch": launch(stats["frames"]), "translated_launch": launch(stats["translated"]),
                      "translated_GCUPS": round(cells / (float(np.median(ms["translated"])) / 1e3) / 1e9, 2),
                      "scores_equal": equal, "max_score": int(ref.max())}))
    dna.close()
    frames.close()
    mx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=65536)
    ap.add_argument("--qlen", type=int, default=1024)
    ap.add_argument("--lo", type=int, default=256)
    ap.add_argument("--hi", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--alphabet", default="dna", choices=("dna", "protein"))
    ap.add_argument("--queries", type=int, default=0,
                    help="also time search_db over this many queries of qlen (pipelined on the database's stream)")
    ap.add_argument("--opt", action="append", default=[], help="engine option k=v (sw_set_option), repeatable")
    ap.add_argument("--matrix", default=None, help="'random' or a matrix file: search under a substitution matrix")
    ap.add_argument("--gaps", default=None, help="G_INIT,G_EXT of a --matrix search")
    ap.add_argument("--alignments", type=int, default=0, help="also time the search plus aligning its top K (--matrix)")
    ap.add_argument("--plant", type=int, default=0, help="records replaced by mutated copies of the query")
    ap.add_argument("--mode", default="local", choices=("local", "global", "semiglobal"),
                    help="alignment mode of a --matrix search")
    ap.add_argument("--profile", action="store_true",
                    help="also search with Profile.from_matrix(matrix, query), alternated with the matrix search (--matrix)")
    ap.add_argument("--translated", action="store_true",
                    help="the translated search of a protein query against DNA records, and the matrix search over their "
                         "six host-translated frames (--matrix)")
    a = ap.parse_args()
    if a.translated and a.matrix is None:
        ap.error("--translated needs --matrix")
    if a.translated:
        return translated(a)
    if a.profile and a.matrix is None:
        ap.error("--profile needs --matrix")
    if a.mode != "local" and a.matrix is None:
        ap.error("--mode needs --matrix")
    if (a.matrix is None) != (a.gaps is None):
        ap.error("--matrix and --gaps go together")
    if a.alignments and a.matrix is None:
        ap.error("--alignments needs --matrix")
    import concurrentproject_amd as sw
    for kv in a.opt:
        k, v = kv.split("=")
        sw.set_option(k, int(v))
    rng = np.random.default_rng(4)
    acgt = np.frombuffer(b"ACGT" if a.alphabet == "dna" else b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
    lens = rng.integers(a.lo, a.hi + 1, size=a.records)
    parts = []
    for i, n in enumerate(lens):
        parts.append(b">r%d\n" % i + acgt[rng.integers(0, len(acgt), size=n)].tobytes() + b"\n")
    q = acgt[rng.integers(0, len(acgt), size=a.qlen)]
    if a.plant:   # (after every draw above, so that a run without --plant has the inputs it always had)
        prng = np.random.default_rng(5)
        for i in prng.choice(a.records, a.plant, replace=False):
            h = q.copy()
            sub = prng.random(len(h)) < 0.3
            h[sub] = acgt[prng.integers(0, len(acgt), int(sub.sum()))]
            for _ in range(4):
                at = int(prng.integers(1, len(h) - 8))
                h = np.delete(h, slice(at, at + int(prng.integers(1, 8))))
            n = int(lens[i])
            pad = acgt[prng.integers(0, len(acgt), size=max(n - len(h), 0))]
            cut = int(prng.integers(0, len(pad) + 1))
            rec = np.concatenate([pad[:cut], h, pad[cut:]])[:n]
            parts[i] = b">r%d\n" % i + rec.tobytes() + b"\n"
    db = Database.from_fasta(b"".join(parts))
    kw, extra = {}, {}
    if a.matrix is not None:
        if a.matrix == "random":
            trng = np.random.default_rng(62)
            k = len(acgt)
            tab = trng.integers(-4, 4, (k, k))
            tab[np.arange(k), np.arange(k)] = trng.integers(4, 12, k)
            mx = sw.Matrix(acgt.tobytes(), tab)
        else:
            mx = sw.Matrix.open(a.matrix)
        gi, ge = (int(x) for x in a.gaps.split(","))
        kw = {"matrix": mx, "gap_init": gi, "gap_ext": ge}
        extra = {"matrix": a.matrix, "gaps": [gi, ge]}
        if a.mode != "local":   # (a local run prints the lines it always printed)
            kw["mode"] = a.mode
            extra["align_mode"] = a.mode
    db.search(q, **kw)  # upload + warm
    t0 = time.perf_counter()
    for _ in range(a.steps):
        sc = db.search(q, **kw)
    dt = (time.perf_counter() - t0) / a.steps
    cells = int(lens.sum()) * a.qlen
    st = sw.last_stats()
    print(json.dumps({**extra, "metric": "db search GCUPS (host API, synchronous)", "alphabet": a.alphabet,
                      "kernel_ms": round(st.get("kernel_ms", -1), 3), "mode": st["mode"], "W": st["W"], "value": round(cells / dt / 1e9, 2),
                      "unit": "GCUPS", "ms_per_search": round(dt * 1e3, 3), "records": a.records,
                      "residues": int(lens.sum()), "qlen": a.qlen, "len_range": [a.lo, a.hi],
                      "max_score": int(sc.max())}))
    if a.profile:
        pf = sw.Profile.from_matrix(mx, q)
        t_mx, t_pf, k_mx, k_pf, st_mx, st_pf, equal = [], [], [], [], None, None, True
        for _ in range(3):
            for which in ("matrix", "profile"):
                run = (lambda: db.search(q, **kw)) if which == "matrix" else (lambda: db.search_profile(pf, gi, ge, mode=a.mode))
                got = run()   # warm
                equal = equal and got.tolist() == sc.tolist()
                kms = []
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    run()
                    kms.append(sw.last_stats()["kernel_ms"])
                dt = (time.perf_counter() - t0) / a.steps
                (t_mx if which == "matrix" else t_pf).append(round(dt * 1e3, 3))
                (k_mx if which == "matrix" else k_pf).append(round(float(np.median(kms)), 3))
                if which == "matrix":
                    st_mx = sw.last_stats()
                else:
                    st_pf = sw.last_stats()
        print(json.dumps({**extra, "metric": "db profile search against matrix search (host API, alternated)", "alphabet": a.alphabet,
                          "records": a.records, "qlen": a.qlen, "len_range": [a.lo, a.hi], "steps": a.steps,
                          "matrix_ms_per_search": t_mx, "profile_ms_per_search": t_pf,
                          "matrix_kernel_ms": k_mx, "profile_kernel_ms": k_pf,
                          "ratio_profile_over_matrix": round(float(np.median(t_pf)) / float(np.median(t_mx)), 3),
                          "kernel_ratio_profile_over_matrix": round(float(np.median(k_pf)) / float(np.median(k_mx)), 3),
                          "matrix_launch": {"mode": st_mx["mode"], "W": st_mx["W"], "waves_per_cu": st_mx["waves_per_cu"], "blocks": st_mx["blocks"]},
                          "profile_launch": {"mode": st_pf["mode"], "W": st_pf["W"], "waves_per_cu": st_pf["waves_per_cu"], "blocks": st_pf["blocks"]},
                          "profile_GCUPS": round(cells / (float(np.median(t_pf)) / 1e3) / 1e9, 2), "scores_equal": equal}))
        pf.close()
    if a.alignments:
        K = a.alignments
        top = db.top(q, k=K, **kw, alignments=True)   # warm: the trace buffers are allocated here
        t0 = time.perf_counter()
        for _ in range(a.steps):
            top = db.top(q, k=K, **kw, alignments=True)
        dta = (time.perf_counter() - t0) / a.steps
        t0 = time.perf_counter()
        for _ in range(a.steps):
            db.top(q, k=K, **kw)
        dts = (time.perf_counter() - t0) / a.steps
        idx = [t[1] for t in top]
        fills, walks = [], []
        for _ in range(a.steps):
            al = db.align(q, idx, mx, gi, ge, mode=a.mode)
            sta = sw.last_stats()
            f, w = sw.last_align_ms()
            fills.append(f)
            walks.append(w)
        pairs = [(q, np.frombuffer(db.record(i)[1], np.uint8)) for i in idx]
        sw.set_option("W", sta["W"])                     # the score-only kernel at the traced kernel's W, same pairs
        plain = []
        for _ in range(a.steps + 1):
            assert sw.score_matrix_batch(pairs, mx, gi, ge, mode=a.mode) == [x.score for x in al]
            plain.append(sw.last_stats()["kernel_ms"])
        sw.set_option("W", 0)
        kcells = sum(len(y) for _, y in pairs) * a.qlen
        fill, walk, score_ms = float(np.median(fills)), float(np.median(walks)), float(np.median(plain[1:]))
        print(json.dumps({**extra, "metric": "db search + alignments of the top K (host API)", "alphabet": a.alphabet, "K": K,
                          "planted": a.plant, "ms_search_top": round(dts * 1e3, 3), "ms_search_top_aligned": round(dta * 1e3, 3),
                          "W": sta["W"], "launches": sta["variant"] & 0xFFFFFFF, "trace_bytes": sta["boundary_bytes"], "cells": kcells,
                          "fill_kernel_ms": round(fill, 4), "fill_GCUPS": round(kcells / fill / 1e6, 2),
                          "score_kernel_ms_same_W": round(score_ms, 4), "score_GCUPS_same_W": round(kcells / score_ms / 1e6, 2),
                          "walk_kernel_ms": round(walk, 4), "cigar_ops_mean": round(float(np.mean([len(x.ops) for x in al])), 1),
                          "aligned_span_mean": round(float(np.mean([x.end1 - x.beg1 for x in al])), 1)}))
    if a.queries:
        from concurrentproject_amd.db import Database as D
        qrecs = [("q%d" % k, acgt[rng.integers(0, len(acgt), size=a.qlen)].tobytes()) for k in range(a.queries)]
        qdb = D.from_records(qrecs)
        db.search_db(qdb)   # warm
        t0 = time.perf_counter()
        many = db.search_db(qdb)
        dm = (time.perf_counter() - t0) / a.queries
        t0 = time.perf_counter()
        one = [db.search(q) for _, q in qrecs]
        ds = (time.perf_counter() - t0) / a.queries
        print(json.dumps({"metric": "db search_db GCUPS (host API, pipelined queries)", "alphabet": a.alphabet,
                          "queries": a.queries, "ms_per_query": round(dm * 1e3, 3),
                          "value": round(cells / dm / 1e9, 2), "unit": "GCUPS",
                          "ms_per_query_one_by_one": round(ds * 1e3, 3),
                          "equal": all(many[k].tolist() == one[k].tolist() for k in range(a.queries))}))
        qdb.close()
    db.close()


if __name__ == "__main__":
    main()
