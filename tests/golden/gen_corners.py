#!/usr/bin/env python3
"""Generate tests/golden/params_corners.json: the oracle pinned to the reference's own code at every
corner of the scoring-constant domain (CORNERS, tests/test_param_corners.py).

Run in the build container.  For every constant set the reference's main.cpp + lazySmith.cpp are built
with the set substituted (``make -C oracle refvar MA= MI= GI= GE=``, into oracle/_ref, nothing of it
committed), and both entry points (SmithWatermanScore, LazySmith) score six small pairs shared by all
sets: random DNA, a mutated copy with indels, an identical pair, a protein pair, an ACGTN pair and
1 x k.  The restatement (oracle.score_full, oracle.score_linear) must equal SmithWatermanScore, the
recurrence of main.cpp:54-66 that include/algoGPU.h defines the score by, at every set, and LazySmith
wherever that computes the same recurrence (G_INIT <= 2 G_EXT, see main() below), or generation aborts.
The fixture is data only: the pairs, and per set the constants and the six scores of each entry point.

    python tests/golden/gen_corners.py
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle  # noqa: E402
from test_param_corners import ACGT, ACGTN, CORNERS, PROTEIN, rand_seq  # noqa: E402


def copy_with_indels(rng, alpha, a, m):
    """m residues from a: 5-10 % substitutions, a deletion and an insertion of 1-3 residues."""
    b = a.copy()
    sub = rng.random(len(b)) < rng.uniform(0.05, 0.10)
    b[sub] = rand_seq(rng, alpha, int(sub.sum()))
    d, i = sorted(int(x) for x in rng.choice(np.arange(10, len(b) - 10), 2, replace=False))
    b = np.insert(b, i, rand_seq(rng, alpha, int(rng.integers(1, 4))))
    b = np.delete(b, slice(d, d + int(rng.integers(1, 4))))
    return np.ascontiguousarray(np.resize(b, m))


def pairs():
    rng = np.random.default_rng(20261019)
    a = rand_seq(rng, ACGT, 200)
    s = rand_seq(rng, ACGT, 120)
    pr = rand_seq(rng, PROTEIN, 160)
    nn = rand_seq(rng, ACGTN, 180)
    one = rand_seq(rng, ACGT, 1)
    return [("random DNA", rand_seq(rng, ACGT, 150), rand_seq(rng, ACGT, 180)),
            ("mutated copy with indels", a, copy_with_indels(rng, ACGT, a, 190)),
            ("identical", s, s.copy()),
            ("protein", pr, copy_with_indels(rng, PROTEIN, pr, 140)),
            ("ACGTN", nn, copy_with_indels(rng, ACGTN, nn, 170)),
            ("1 x k", one, np.concatenate([rand_seq(rng, ACGT, 129), one]))]


def main():
    oracle.build()
    ps = pairs()
    sets = []
    for t in CORNERS:
        prm = oracle.Params(*t)
        if not oracle.build_refvar(prm) or oracle.ref_lib(prm) is None:
            sys.exit("no reference build for %r: run this in the build container" % (t,))
        scores, lazy = [], []
        for _, a, b in ps:
            lin = oracle.score_linear(a, b, prm)
            got = (oracle.score_full(a, b, prm), oracle.ref_score(a, b, prm, "full"))
            assert got == (lin, lin), (t, lin, got)
            scores.append(lin)
            lazy.append(oracle.ref_score(a, b, prm, "lazy"))
        # LazySmith's second pass (lazySmith.cpp:43-62) carries a gap along the row into F at G_EXT a
        # residue, so a gap that turns the corner pays G_INIT once where main.cpp:57-58 pays it twice:
        # the same recurrence exactly when G_INIT <= 2 G_EXT, and never a smaller score
        assert lazy == scores if t[2] <= 2 * t[3] else all(x >= y for x, y in zip(lazy, scores)), (t, scores, lazy)
        sets.append({"params": list(t), "scores": scores, "lazy_scores": lazy})
    out = {"source": "tests/golden/gen_corners.py: six pairs shared by every set",
           "pinned_by": ["reference SmithWatermanScore (main.cpp) and LazySmith (lazySmith.cpp) built with each set "
                         "(oracle/Makefile refvar): scores / lazy_scores", "oracle swo_full", "oracle swo_linear"],
           "note": "lazy_scores differ from scores only where G_INIT > 2 G_EXT: LazySmith's second pass "
                   "(lazySmith.cpp:43-62) lets a gap turn the corner at G_EXT; the score is main.cpp's",
           "pairs": [{"kind": k, "seq1": a.tobytes().decode("ascii"), "seq2": b.tobytes().decode("ascii")}
                     for k, a, b in ps],
           "sets": sets}
    with open(os.path.join(HERE, "params_corners.json"), "w") as f:
        json.dump(out, f, indent=1)
    print("wrote params_corners.json:", len(sets), "sets x", len(ps), "pairs")


if __name__ == "__main__":
    main()
