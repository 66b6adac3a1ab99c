"""GPU parity of the leaner half-chunk links of the staged flow3 loops (tools/gen_flow3.py LINK_*; DESIGN.md
section 8): the ring offset advanced once a loop body (the odd chunk through immediate offsets, slot of row 0 at
F3_HL_SLOT0), the inflow read landing in the next chunk's I/O register, the producer-word checks on the VALU and
the consumer word written every second chunk.  Bit-exact against oracle.score_linear at the smallest shapes where
a link can go wrong.

Columns 253 .. 1135: 2, 3, 4, 5, 8 and 9 strips (LDS links, a group edge, a second group, a third).  Rows: around
one and two chunk pairs (63 .. 129: the half-chunk boundary and the odd chunk), around the ring's wrap (479 .. 545:
the odd chunk's window one chunk before, at and after slot R), 1055, 1536 (three laps) and 4129 (wedges at nine
strips).  Plans: the whole pair, the column cut, the uniform wedge and the steep wedge, forced by option f3split
and SWMI_F3WEDGE / SWMI_F3WEDGE_DROPS wherever the plan admits the shape (the admission arithmetic: engine
split_bounds, tests/test_wedge_identity.py, tests/test_steep_identity.py).  Grids of 1, 2 and 3 workgroups.  Two
linear-gap constant sets, one with G > 1.  A seven-letter pair per shape.  Random pairs, and a mutated copy laid
corner to corner, so that H stays large across every link.  Every launch is followed by stream_status: a
time-out or a failed edge key raises.  The C2 golden and its lower-case relabeling once each."""
import os

import numpy as np
import pytest

from test_steep_identity import steep_plan
from test_wedge_identity import wedge_plan

pytestmark = pytest.mark.gpu

NS = [253, 254, 379, 504, 505, 631, 1009, 1135]
MS = [63, 64, 65, 95, 96, 97, 127, 128, 129, 479, 480, 481, 511, 512, 513, 543, 544, 545, 1055, 1536, 4129]
PARAMS = [(1, -1, 1, 1), (2, -3, 3, 3)]
GRIDS = (1, 2, 3)
UNIFORM, STEEP_D = (64, 64, 64, 64), (64, 128, 64, 128)
ACGT = np.frombuffer(b"ACGT", np.uint8)
SEVEN = np.frombuffer(b"ACGTNRY", np.uint8)
F3, HL, HEP, CUT, WEDGE, STEEP = 1 << 6, 1 << 9, 1 << 16, 1 << 17, 1 << 18, 1 << 19
ENVS = ("SWMI_F3WEDGE", "SWMI_F3WEDGE_DROPS")


@pytest.fixture(autouse=True)
def _defaults(engine, request):
    def reset():
        for e in ENVS:
            os.environ.pop(e, None)
        for k, v in (("f3split", -1), ("blocks", 0), ("orient", 0), ("mode", -1)):
            engine.set_option(k, v)
    request.addfinalizer(reset)
    reset()


def _force(engine):
    engine.set_option("orient", 1)   # seq1 across the lanes: n is its length
    engine.set_option("mode", 5)     # the staged kernels at every size


def _plans(engine, n, m):
    """(name, f3split, environment, variant bits expected) of every plan that admits n x m"""
    out = [("whole", 0, {"SWMI_F3WEDGE": "0"}, 0)]
    if engine.split_bounds(n) is not None:
        out.append(("cut", 1, {"SWMI_F3WEDGE": "0"}, CUT))
    if wedge_plan(n, m) is not None:
        out.append(("wedge", -1, {"SWMI_F3WEDGE": "1", "SWMI_F3WEDGE_DROPS": ",".join(map(str, UNIFORM))}, WEDGE))
    if steep_plan(n, m, STEEP_D) is not None:
        out.append(("steep", -1, {"SWMI_F3WEDGE": "1", "SWMI_F3WEDGE_DROPS": ",".join(map(str, STEEP_D))},
                    WEDGE | STEEP))
    return out


def _stretched(rng, alpha, a, m):
    """a laid over m rows corner to corner, 5 % of it substituted"""
    n = len(a)
    b = a[np.minimum((np.arange(m) * n) // m, n - 1)].copy()
    mut = rng.random(m) < 0.05
    b[mut] = alpha[rng.integers(0, len(alpha), int(mut.sum()))]
    return np.ascontiguousarray(b)


_CASES = {}


def _cases(oracle_mod, n, m):
    """The seeded pairs of a shape with their oracle scores, computed once:
    (tag, a, b, constants, score, every grid or one)"""
    if (n, m) not in _CASES:
        rng = np.random.default_rng([n, m])
        a = ACGT[rng.integers(0, 4, n)]
        rnd = ACGT[rng.integers(0, 4, m)]
        sim = _stretched(rng, ACGT, a, m)
        a7 = SEVEN[rng.integers(0, 7, n)]
        sim7 = _stretched(rng, SEVEN, a7, m)
        sc = lambda x, y, p: oracle_mod.score_linear(x, y, oracle_mod.Params(*p))
        _CASES[(n, m)] = [("random", a, rnd, PARAMS[0], sc(a, rnd, PARAMS[0]), True),
                          ("similar", a, sim, PARAMS[0], sc(a, sim, PARAMS[0]), False),
                          ("similar G=3", a, sim, PARAMS[1], sc(a, sim, PARAMS[1]), False),
                          ("random G=3", a, rnd, PARAMS[1], sc(a, rnd, PARAMS[1]), False),
                          ("seven letters", a7, sim7, PARAMS[0], sc(a7, sim7, PARAMS[0]), False)]
    return _CASES[(n, m)]


def _launch(engine, a, b, prm_t, exp, bits, tag):
    got = engine.score(a, b, engine.Params(*prm_t))
    engine.stream_status()            # ERR_TIMEOUT / ERR_EDGE raise
    st = engine.last_stats()
    assert got == exp, (tag, got, exp, st)
    assert st["mode"] == 5 and st["variant"] & F3 and st["variant"] & HL, (tag, st)
    assert st["variant"] & (CUT | WEDGE | STEEP) == bits, (tag, bits, st)
    return st


@pytest.mark.parametrize("n", NS)
def test_shapes_plans_and_grids(engine, oracle_mod, n):
    _force(engine)
    launches, seen = 0, set()
    for mi, m in enumerate(MS):
        for name, split, env, bits in _plans(engine, n, m):
            for e in ENVS:
                os.environ.pop(e, None)
            os.environ.update(env)
            engine.set_option("f3split", split)
            seen.add(name)
            for ci, (tag, a, b, prm_t, exp, every_grid) in enumerate(_cases(oracle_mod, n, m)):
                for blocks in (GRIDS if every_grid else (GRIDS[(mi + ci) % 3],)):
                    engine.set_option("blocks", blocks)
                    st = _launch(engine, a, b, prm_t, exp, bits, (n, m, name, tag, blocks))
                    assert bool(st["variant"] & HEP) == (tag == "seven letters"), (n, m, name, tag, st)
                    launches += 1
    # every plan occurs at every width but the cut below 379 columns and the steep plan where its frame refuses
    assert {"whole", "wedge"} <= seen and (("cut" in seen) == (n >= 379)), (n, seen)
    print(n, "launches", launches, "plans", sorted(seen))


def test_steep_plan_is_covered():
    """The shapes above reach the steep plan at the widths its frame admits, the tall ones among them."""
    got = {(n, m) for n in NS for m in MS if steep_plan(n, m, STEEP_D) is not None}
    assert {n for n, _ in got} == {253, 254, 379, 504, 631, 1135} and (1135, 4129) in got and (631, 1055) in got, got


def test_c2_golden_and_lower_case(engine, golden):
    """The flagship pair on the automatic plan, and relabeled a, c, g, t (the seven-letter kernels)."""
    c = golden("configs.json")["C2"]
    a, b = engine.gen_pair(c["seed"], c["N"])
    assert engine.SmithWatermanScoreCUDA(a, b) == c["score"] == 7458
    engine.stream_status()
    st = engine.last_stats()
    assert st["variant"] & F3 and st["variant"] & HL and st["variant"] & WEDGE and st["variant"] & STEEP, st
    lower = np.arange(256, dtype=np.uint8)
    lower[ACGT] = np.frombuffer(b"acgt", np.uint8)
    assert engine.SmithWatermanScoreCUDA(lower[a], lower[b]) == 7458
    engine.stream_status()
    st = engine.last_stats()
    assert st["dna"] == 2 and st["variant"] & HL and st["variant"] & WEDGE, st
