"""``python -m concurrentproject_amd.align --query q.fa --db sp.swdb [--top K]``:
every query record scored against every database record on the GPU (the
``align`` step of the reference's timing.sh:7, CUDASW++4's tool there).

Prints, per query, its K best hits as tab-separated lines
``query_index  query_header  rank  score  db_index  db_header``; the search's
cells, time and GCUPS go to stderr.  Scores are the reference's byte-equality
affine scores (main.cpp:28-66) with --params MATCH,MISMATCH,G_INIT,G_EXT, or, with
--matrix FILE --gaps G_INIT,G_EXT, scores under the substitution matrix of FILE (NCBI
text format, e.g. BLOSUM62; none is built in).  A gap of L residues costs
G_INIT + (L-1)*G_EXT: BLAST's "open 11, extend 1" is --gaps 12,1.

With --alignments every hit line gains ``q_beg  q_end  d_beg  d_end  cigar``: the half-open
ranges of the query and of the record that the alignment covers and its operations (M an aligned
pair, I a query residue against a gap, D a record residue against a gap; ``*`` for a score of 0).
Only the top K of each query are aligned.  Without --matrix the alignments are made under the
equality table of --params over the bytes present (at most 32 distinct ones).  --long makes the
same alignments by checkpointed traceback (Database.align(long=True)): for hits so long that a
whole pair's trace does not fit option trace_mb; the lines are the same.  --coop (with --long) makes
them on many waves (Database.align(long=True, coop=True)); the lines are the same again.

--mode global|semiglobal (with --matrix; default local): the query and the record end to end, or
the whole query inside the record with the record's flanks free.  Scores may be negative, an
alignment may begin or end with a gap, and the queries are searched one after another
(Database.search(mode=...)).  Not with --long.

--translate (with --matrix and --gaps): the database is DNA and the queries are proteins; every query is scored
against the six reading frames (+1, +2, +3, -1, -2, -3) of every record, translated under the standard genetic
code by the kernel (Database.search_translated), one query after another.  A hit is a (record, frame): its line is
``query_index  query_header  rank  score  db_index  db_header  frame``, and with --alignments it gains
``q_beg  q_end  dna_beg  dna_end  cigar``, the DNA range on the forward strand.  Ties rank by record, then by frame
in the order above.  Not with --long or --coop (no long path against a translated frame)."""
import argparse
import sys
import time

import numpy as np

from . import Matrix, Params, set_params
from .db import Database


def translated(a, db, qs, matrix, gaps, lens) -> int:
    """--translate: every query through Database.top_translated, one after another."""
    t0 = time.perf_counter()
    out = sys.stdout
    for q in range(len(qs)):
        qh, query = qs.record(q)
        hits = db.top_translated(query, a.top, matrix, gaps[0], gaps[1], alignments=a.alignments, mode=a.mode)
        for r, h in enumerate(hits):
            line = "%d\t%s\t%d\t%d\t%d\t%s\t%+d" % (q, qh, r + 1, h[0], h[1], h[3], h[2])
            if a.alignments:
                x = h[4]
                line += "\t%d\t%d\t%d\t%d\t%s" % (x.beg1, x.end1, x.dna_beg, x.dna_end, x.cigar or "*")
            out.write(line + "\n")
    dt = time.perf_counter() - t0
    cells = int(qs.lengths().sum()) * int(sum(2 * ((L - o) // 3 if L >= o + 3 else 0) for L in lens for o in range(3)))
    print("%d queries x %d records x 6 frames: %.3e cells in %.3f s = %.2f GCUPS"
          % (len(qs), len(db), cells, dt, cells / max(dt, 1e-12) / 1e9), file=sys.stderr)
    return 0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="align", description=__doc__)
    ap.add_argument("--query", required=True, help="FASTA file (or a makedb file) of queries")
    ap.add_argument("--db", required=True, help="FASTA file or a makedb file")
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--params", default="1,-1,1,1", help="MATCH,MISMATCH,G_INIT,G_EXT")
    ap.add_argument("--matrix", default=None, help="substitution matrix file (NCBI text format); needs --gaps")
    ap.add_argument("--gaps", default=None, help="G_INIT,G_EXT of a --matrix search")
    ap.add_argument("--alignments", action="store_true", help="align the top K hits: ranges and cigar per line")
    ap.add_argument("--long", action="store_true",
                    help="with --alignments: checkpointed traceback, for hits whose whole trace does not fit (same lines)")
    ap.add_argument("--coop", action="store_true",
                    help="with --long: the locate pass on many waves and a window of strips a round (same lines)")
    ap.add_argument("--mode", choices=("local", "global", "semiglobal"), default="local",
                    help="alignment mode of a --matrix search: global = query and record end to end, semiglobal = the "
                         "whole query inside the record")
    ap.add_argument("--translate", action="store_true",
                    help="the database is DNA: protein queries against its six reading frames (needs --matrix and --gaps)")
    a = ap.parse_args(argv)
    if a.translate and (a.matrix is None or a.gaps is None):
        ap.error("--translate requires --matrix and --gaps")
    if a.translate and (a.long or a.coop):
        ap.error("--translate is not with --long or --coop: there is no long path against a translated frame")
    if a.long and not a.alignments:
        ap.error("--long goes with --alignments")
    if a.coop and not a.long:
        ap.error("--coop goes with --long")
    if a.mode != "local" and a.matrix is None:
        ap.error("--mode %s requires --matrix (and --gaps)" % a.mode)
    if a.mode != "local" and a.long:
        ap.error("--long is local only: not with --mode %s (Database.align_long(..., mode=...) aligns long records in a mode)"
                 % a.mode)
    if (a.matrix is None) != (a.gaps is None):
        ap.error("--matrix and --gaps go together")
    matrix, gaps = None, (None, None)
    if a.matrix is not None:
        gaps = tuple(int(x) for x in a.gaps.split(","))
        if len(gaps) != 2:
            ap.error("--gaps takes G_INIT,G_EXT")
        matrix = Matrix.open(a.matrix)
    else:
        prm = Params(*(int(x) for x in a.params.split(",")))
        set_params(prm)
    with Database.open(a.db) as db, Database.open(a.query) as qs:
        lens = db.lengths()
        if a.translate:
            return translated(a, db, qs, matrix, gaps, lens)
        t0 = time.perf_counter()
        if a.mode != "local":   # one query after another: search_db is local only
            scores = np.zeros((len(qs), len(db)), dtype=np.int32)
            for q in range(len(qs)):
                scores[q] = db.search(qs.record(q)[1], matrix=matrix, gap_init=gaps[0], gap_ext=gaps[1], mode=a.mode)
        else:
            scores = db.search_db(qs, matrix=matrix, gap_init=gaps[0], gap_ext=gaps[1])
        dt = time.perf_counter() - t0
        cells = int(qs.lengths().sum()) * int(lens.sum())
        out = sys.stdout
        amatrix, agaps = matrix, gaps
        if a.alignments and matrix is None:   # the equality table of --params over the bytes present
            present = set()
            for d in (db, qs):
                for r in range(len(d)):
                    present.update(d.record(r)[1])
            if len(present) > 32:
                print("align --alignments: %d distinct bytes in the query and the database; an equality matrix "
                      "holds at most 32 (pass --matrix)" % len(present), file=sys.stderr)
                return 2
            amatrix = Matrix.equality(bytes(sorted(present)) or b"A", prm.match, prm.mismatch)
            agaps = (prm.gap_init, prm.gap_ext)
        for q in range(len(qs)):
            qh = qs.header(q)
            sc = scores[q]
            order = np.lexsort((np.arange(len(sc)), -sc.astype(np.int64)))[:a.top]
            if a.alignments:
                al = db.align(qs.record(q)[1], [int(i) for i in order], amatrix, agaps[0], agaps[1], long=a.long, mode=a.mode,
                              coop=a.coop)
                for r, (i, x) in enumerate(zip(order, al)):
                    out.write("%d\t%s\t%d\t%d\t%d\t%s\t%d\t%d\t%d\t%d\t%s\n"
                              % (q, qh, r + 1, int(sc[i]), int(i), db.header(int(i)), x.beg1, x.end1, x.beg2, x.end2,
                                 x.cigar or "*"))
                continue
            for r, i in enumerate(order):
                out.write("%d\t%s\t%d\t%d\t%d\t%s\n" % (q, qh, r + 1, int(sc[i]), int(i), db.header(int(i))))
        print("%d queries x %d records: %.3e cells in %.3f s = %.2f GCUPS"
              % (len(qs), len(db), cells, dt, cells / max(dt, 1e-12) / 1e9), file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
