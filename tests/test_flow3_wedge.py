"""GPU parity of the wedge plan: one pair on flow3's staged two-column linear-gap kernel
as two chains over all columns, one forward and one on both sequences mirrored, each strip 64 rows shorter
than the one before, joined along the staircase by sw_flow3_wedge_combine_kernel.  Bit-exact against
oracle.score_linear, with environment SWMI_F3WEDGE = 1 forcing the plan wherever the geometry admits it
(m >= 64 S + 64 for S = ceil((n - 2) / 126) strips a chain).

Covered: 2, 3, 5 and 6 strips a chain (an in-workgroup and a cross-workgroup hop), lead pads of 0, 1, 58 and
125 columns, m at the admission edge, one chunk above it, off a multiple of 32 (every such m gives the
mirrored chain dead rows in front), about n and about 2 n; random pairs and mutated copies laid corner to
corner, whose best path crosses the staircase (counted with the CPU model of tests/test_wedge_identity.py);
three linear-gap constant sets; a seven-letter pair; grids of 1, 2 and 3 workgroups; launches back to back
on the same buffers; and the automatic plan's choice (variant bit 18 of sw_last_stats).
The corners of the scoring-constant domain over these launches: tests/test_wedge_corners.py."""
import os
import zlib

import numpy as np
import pytest

from test_wedge_identity import wedge_model, wedge_plan

pytestmark = pytest.mark.gpu

PARAMS = [(1, -1, 1, 1), (2, -3, 2, 2), (3, -1, 4, 4)]
NS = [253, 254, 255, 379, 380, 631, 700]
ACGT = np.frombuffer(b"ACGT", np.uint8)
WEDGE = 1 << 18
CUT = 1 << 17
ENV = "SWMI_F3WEDGE"


@pytest.fixture(autouse=True)
def _defaults(engine, request):
    def reset():
        os.environ.pop(ENV, None)
        engine.set_option("f3split", -1)
        engine.set_option("blocks", 0)
        engine.set_option("orient", 0)
        engine.set_option("trace", 0)
    request.addfinalizer(reset)
    engine.set_option("orient", 1)   # seq1 across the lanes: n is its length
    os.environ[ENV] = "1"


def _stretched(rng, alpha, a, m):
    """a stretched (or squeezed) over m rows, 5 % replaced and one short insertion: corner to corner"""
    n = len(a)
    b = a[np.minimum((np.arange(m) * n) // m, n - 1)].copy()
    mut = rng.random(m) < 0.05
    b[mut] = alpha[rng.integers(0, len(alpha), int(mut.sum()))]
    k = int(rng.integers(5, m - 5))
    return np.ascontiguousarray(np.concatenate([b[:k], alpha[rng.integers(0, len(alpha), 2)], b[k:]])[:m])


def _heights(n):
    lo = 64 * wedge_plan(n, 1 << 20)[0] + 64
    return [lo, lo + 32, lo + 13, max(lo, n + 1), 2 * n - 3]


def _check(engine, oracle_mod, a, b, prm_t, tag):
    exp = oracle_mod.score_linear(a, b, oracle_mod.Params(*prm_t))
    got = engine.score(a, b, engine.Params(*prm_t))
    st = engine.last_stats()
    assert got == exp, (tag, got, exp, st)
    return st


@pytest.mark.parametrize("prm_t", PARAMS)
def test_shapes_against_oracle(engine, oracle_mod, prm_t):
    rng = np.random.default_rng(zlib.crc32(repr(prm_t).encode()))
    crossing = 0
    for n in NS:
        S = wedge_plan(n, 1 << 20)[0]
        for m in _heights(n):
            a = ACGT[rng.integers(0, 4, n)]
            for kind, y in (("random", ACGT[rng.integers(0, 4, m)]), ("stretched", _stretched(rng, ACGT, a, m))):
                st = _check(engine, oracle_mod, a, y, prm_t, (kind, n, m))
                assert st["variant"] & WEDGE and st["variant"] & 64 and not st["variant"] & CUT, (kind, n, m, st)
                assert st["items"] == 2 * ((S + 3) // 4), (n, m, st)
            crossing += wedge_model(a, y, prm_t)[1]
    # the CPU model counts 33, 29 and 35 of the 35 stretched copies decided by the crossing term for the three
    # constant sets (a property of these seeded inputs, not of the kernel)
    assert crossing >= 25, crossing


def test_below_admission_stays_off(engine, oracle_mod):
    """One row short of 64 S + 64 the plan is not taken, forced or not."""
    rng = np.random.default_rng(3)
    for n in (253, 700):
        m = 64 * wedge_plan(n, 1 << 20)[0] + 63
        a = ACGT[rng.integers(0, 4, n)]
        st = _check(engine, oracle_mod, a, _stretched(rng, ACGT, a, m), (1, -1, 1, 1), ("short", n, m))
        assert not st["variant"] & WEDGE, st


@pytest.mark.parametrize("blocks", [1, 2, 3])
def test_small_grids(engine, oracle_mod, blocks):
    """Fewer workgroups than strip groups (1200 columns: 3 + 3 groups, claimed F0, B0, F1, ...): every
    group's producer has a lower item number, so it has been claimed before."""
    engine.set_option("blocks", blocks)
    rng = np.random.default_rng(100 + blocks)
    a = ACGT[rng.integers(0, 4, 1200)]
    for prm_t in PARAMS:
        b = _stretched(rng, ACGT, a, 64 * 10 + 64 + 17)
        st = _check(engine, oracle_mod, a, b, prm_t, ("grid", blocks, prm_t))
        assert st["variant"] & WEDGE and st["blocks"] == blocks and st["items"] == 6, st


def test_seven_letter_pair(engine, oracle_mod):
    """A pair over seven byte values on sw_flow3h_kernel (mirrored column words and row symbols)."""
    alpha = np.frombuffer(b"ACGTNRY", np.uint8)
    rng = np.random.default_rng(7)
    for n, m in ((700, 64 * 6 + 64 + 5), (380, 400)):
        a = alpha[rng.integers(0, 7, n)]
        b = _stretched(rng, alpha, a, m)
        for prm_t in PARAMS:
            st = _check(engine, oracle_mod, a, b, prm_t, ("hep", n, m, prm_t))
            assert st["variant"] & WEDGE and st["dna"] == 2, st


def test_back_to_back_launches(engine, oracle_mod):
    """Launches of one shape reuse the boundary buffers: the epoch-keyed entries of the last launch must
    not serve the next one (the combine kernel checks every key)."""
    rng = np.random.default_rng(23)
    n, m = 700, 777
    a1 = ACGT[rng.integers(0, 4, n)]
    a2 = ACGT[rng.integers(0, 4, n)]
    pairs = [(a1, _stretched(rng, ACGT, a1, m)), (a2, ACGT[rng.integers(0, 4, m)]), (a2, _stretched(rng, ACGT, a2, m))]
    exp = [oracle_mod.score_linear(x, y) for x, y in pairs]
    assert len(set(exp)) == 3
    for _ in range(2):
        for (x, y), e in zip(pairs, exp):
            assert engine.score(x, y) == e
            assert engine.last_stats()["variant"] & WEDGE


def test_switches(engine, oracle_mod):
    """SWMI_F3WEDGE = 0 and option f3split = 0 switch the plan off; f3split = 1 keeps forcing the column
    cut; a traced launch stays one chain."""
    import torch
    rng = np.random.default_rng(5)
    n, m = 700, 600
    a = ACGT[rng.integers(0, 4, n)]
    b = _stretched(rng, ACGT, a, m)
    st = _check(engine, oracle_mod, a, b, (1, -1, 1, 1), "forced")
    assert st["variant"] & WEDGE, st
    engine.set_option("f3split", 1)
    st = _check(engine, oracle_mod, a, b, (1, -1, 1, 1), "f3split = 1")
    assert st["variant"] & CUT and not st["variant"] & WEDGE, st
    engine.set_option("f3split", 0)
    st = _check(engine, oracle_mod, a, b, (1, -1, 1, 1), "f3split = 0")
    assert not st["variant"] & (CUT | WEDGE), st
    engine.set_option("f3split", -1)
    os.environ[ENV] = "0"
    st = _check(engine, oracle_mod, a, b, (1, -1, 1, 1), "env 0")
    assert not st["variant"] & WEDGE, st
    os.environ[ENV] = "1"
    st = _check(engine, oracle_mod, a, b, (2, -3, 5, 2), "affine constants")
    assert not st["variant"] & WEDGE, st
    strips = (n - 2 + 125) // 126
    trace = torch.zeros(16 * strips, dtype=torch.int64, device="cuda")
    engine.set_option("trace", trace.data_ptr())
    st = _check(engine, oracle_mod, a, b, (1, -1, 1, 1), "traced")
    engine.set_option("trace", 0)
    torch.cuda.synchronize()
    assert not st["variant"] & WEDGE, st


def test_automatic_choice(engine, oracle_mod):
    """SWMI_F3WEDGE unset, f3split = -1: the wedge from 4096 columns (sw_engine.hip F3_WEDGE_AUTO_N) wherever
    every strip keeps 64 rows, the column cut one row below that, whole below 4096 columns and when traced."""
    import torch
    os.environ.pop(ENV, None)
    rng = np.random.default_rng(9)
    n = 4096
    S = wedge_plan(n, 1 << 20)[0]
    edge = 64 * S + 64
    a = ACGT[rng.integers(0, 4, n)]
    for m in (edge, n):
        st = _check(engine, oracle_mod, a, _stretched(rng, ACGT, a, m), (1, -1, 1, 1), ("auto", m))
        assert st["variant"] & WEDGE and not st["variant"] & CUT and st["items"] == 2 * ((S + 3) // 4), (m, st)
    b = _stretched(rng, ACGT, a, edge - 1)
    st = _check(engine, oracle_mod, a, b, (1, -1, 1, 1), "one row short")
    assert st["variant"] & CUT and not st["variant"] & WEDGE, st
    b = _stretched(rng, ACGT, a, n)
    st = _check(engine, oracle_mod, a[:n - 1], b, (1, -1, 1, 1), "below 4096 columns")
    assert not st["variant"] & (CUT | WEDGE), st
    strips = (n - 2 + 125) // 126
    trace = torch.zeros(16 * strips, dtype=torch.int64, device="cuda")
    engine.set_option("trace", trace.data_ptr())
    st = _check(engine, oracle_mod, a, b, (1, -1, 1, 1), "traced")
    engine.set_option("trace", 0)
    torch.cuda.synchronize()
    assert not st["variant"] & (CUT | WEDGE), st
    engine.set_option("f3split", 0)
    st = _check(engine, oracle_mod, a, b, (1, -1, 1, 1), "off")
    assert not st["variant"] & (CUT | WEDGE), st
