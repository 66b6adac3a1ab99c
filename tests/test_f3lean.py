"""GPU parity of the staged flow3 kernel's row staging and of the trace of a wedge launch.
A mirrored chain reads row r from byte m + rlead - 1 - r; where that address is off a dword its 16-row blocks
come out of five aligned dwords shifted by the misalignment, and only the blocks at the two ends of the sequence
take byte loads.  With SWMI_F3WEDGE_TRACE = 1 beside option trace a traced launch keeps both chains, every strip
writing one 16-word row at chain * S + strip.

Bit-exact against oracle.score_linear.  Shapes: 4096 x 4096 (automatic steep plan), 4096 x 2176 (wedge admission
edge), 16384 x 12700 (just above the steep admission edge), the narrowest width the steep plan admits (from
tests/test_steep_identity.py steep_plan, at its lowest height and at a tall one), rows off a multiple of 64 (dead
rows in front of the mirrored chain) in every class of m mod 4 (every misalignment of the mirrored loads), widths
whose mirrored chain starts with three, one and no wholly dead strips and a partly dead one (no plan has a wholly
dead group: tests/test_f3lean_cpu.py), and tall pairs whose group 0 stages 17 KB of row codes.  Random pairs,
mutated copies laid corner to corner (long gap runs across the staircase) and a pair whose best cell lies in the
first staged rows.  Each under SWMI_F3WEDGE = 0, SWMI_F3JOIN = 0, a forced drop pattern and the lower-case
relabeling (seven-letter kernels).

The bounded waits: option stall_item acts in flow2's staged kernel only, and the issue behind this file allows no
new way to stall, so test_stalled_item_still_times_out repeats the existing flow2 pattern and then scores a wedge
launch; it does not enter a flow3 spin.  This change adds no spin to any kernel."""
import os
import time

import numpy as np
import pytest

from test_steep_identity import steep_min_m, steep_plan

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", np.uint8)
WEDGE, STEEP = 1 << 18, 1 << 19
AUTO = (64, 128, 64, 128)
ENVS = ("SWMI_F3WEDGE", "SWMI_F3WEDGE_DROPS", "SWMI_F3JOIN", "SWMI_F3WEDGE_TRACE")
LOWER = np.arange(256, dtype=np.uint8)
LOWER[ACGT] = np.frombuffer(b"acgt", np.uint8)


def narrowest_steep_n():
    n = 1
    while steep_plan(n, 1 << 20, AUTO) is None:
        n += 1
    return n


@pytest.fixture(autouse=True)
def _defaults(engine, request):
    def reset():
        for e in ENVS:
            os.environ.pop(e, None)
        engine.set_option("orient", 0)
        engine.set_option("trace", 0)
    request.addfinalizer(reset)
    reset()
    engine.set_option("orient", 1)   # seq1 across the lanes: n is its length


def _stretched(rng, a, m):
    """a stretched (or squeezed) over m rows, 5 % replaced and one short insertion: corner to corner"""
    n = len(a)
    b = a[np.minimum((np.arange(m) * n) // m, n - 1)].copy()
    mut = rng.random(m) < 0.05
    b[mut] = ACGT[rng.integers(0, 4, int(mut.sum()))]
    k = int(rng.integers(5, m - 5))
    return np.ascontiguousarray(np.concatenate([b[:k], ACGT[rng.integers(0, 4, 2)], b[k:]])[:m])


def _early(rng, a, m):
    """a random pair with 290 columns of a copied into rows 5 .. 294: the best cell is in the first staged rows"""
    b = ACGT[rng.integers(0, 4, m)]
    b[5:295] = a[10:300]
    return b


_PAIRS = {}


def _pair(oracle_mod, n, m, kind):
    """The seeded pair of a shape and its oracle score, computed once"""
    key = (n, m, kind)
    if key not in _PAIRS:
        rng = np.random.default_rng([n, m, len(kind)])
        a = ACGT[rng.integers(0, 4, n)]
        b = {"random": lambda: ACGT[rng.integers(0, 4, m)], "similar": lambda: _stretched(rng, a, m),
             "early": lambda: _early(rng, a, m)}[kind]()
        _PAIRS[key] = (a, b, oracle_mod.score_linear(a, b, oracle_mod.Params(1, -1, 1, 1)))
    return _PAIRS[key]


def _score(engine, a, b, env=None):
    for e in ENVS:
        os.environ.pop(e, None)
    os.environ.update(env or {})
    got = engine.score(a, b, engine.Params(1, -1, 1, 1))
    return got, engine.last_stats()


SWITCHES = [{}, {"SWMI_F3WEDGE": "0"}, {"SWMI_F3JOIN": "0"}, {"SWMI_F3WEDGE_DROPS": "64,64,64,128"}]
N0 = narrowest_steep_n()
# (n, m, kind, the automatic plan is steep, SWMI_F3WEDGE forced)
SHAPES = [
    (4096, 4096, "similar", True, False),            # lead 440: three dead strips and 62 dead columns
    (4096, 2176, "random", False, False),            # the wedge admission edge (uniform plan)
    (16384, 12700, "similar", True, False),          # lead 248: one dead strip
    (N0, steep_min_m(N0, AUTO), "similar", True, True),
    (N0, 23975, "similar", True, True),              # tall; m mod 4 = 3
    (4400, 4135, "random", True, False),             # lead 136, m mod 64 = 39
    (4158, 30038, "similar", True, False),           # lead 378: three dead strips exactly; m mod 64 = 22, mod 4 = 2
    (4096, 30037, "early", True, False),             # m mod 4 = 1
]


@pytest.mark.parametrize("n,m,kind,steep,forced", SHAPES)
def test_shapes_and_switches(engine, oracle_mod, n, m, kind, steep, forced):
    a, b, exp = _pair(oracle_mod, n, m, kind)
    base = {"SWMI_F3WEDGE": "1", "SWMI_F3WEDGE_DROPS": ",".join(map(str, AUTO))} if forced else {}
    for sw in SWITCHES:
        env = dict(base, **sw)
        got, st = _score(engine, a, b, env)
        assert got == exp, (n, m, kind, env, got, exp, st)
        if not sw:
            assert bool(st["variant"] & WEDGE) and bool(st["variant"] & STEEP) == steep, (n, m, env, st)
        if "SWMI_F3WEDGE" in sw:
            assert not st["variant"] & WEDGE, (n, m, env, st)
    got, st = _score(engine, LOWER[a], LOWER[b], base)
    assert got == exp and st["dna"] == 2, (n, m, kind, "acgt", got, exp, st)


def test_traced_wedge_launch(engine, oracle_mod):
    """Option trace with SWMI_F3WEDGE_TRACE = 1 keeps the two wedges: the same score as untraced, a row of
    timestamps per chain and strip with entry <= staged <= first step <= last step <= join start <= join end, the
    plan's steps in word 8, and nothing behind the 2 S rows, S = 2 x items as tools/trace_wedge.py sizes it."""
    import torch
    n, m = 4096, 30037
    a, b, exp = _pair(oracle_mod, n, m, "early")
    S = steep_plan(n, m, AUTO)[0]
    trace = torch.zeros(16 * (2 * S + 8), dtype=torch.int64, device="cuda")
    engine.set_option("trace", trace.data_ptr())
    got, st = _score(engine, a, b, {"SWMI_F3WEDGE_TRACE": "1"})
    engine.set_option("trace", 0)
    torch.cuda.synchronize()
    assert got == exp and st["variant"] & WEDGE and st["variant"] & STEEP and 2 * st["items"] == S, (got, exp, st)
    t = trace.cpu().numpy().reshape(-1, 16)
    assert not t[2 * S:].any()
    rows = t[:2 * S]
    assert (rows[:, 0] > 0).all()
    for k in range(5):
        assert (rows[:, k] <= rows[:, k + 1]).all(), (k, rows[(rows[:, k] > rows[:, k + 1])][:4])
    p = steep_plan(n, m, AUTO)
    steps = np.concatenate([p[3] - p[5], p[4] - p[5]])
    assert (rows[:, 8] == steps).all()
    got, st = _score(engine, a, b)
    assert got == exp and st["variant"] & WEDGE


def test_traced_launch_stays_one_chain_without_the_variable(engine, oracle_mod):
    import torch
    n, m = 4096, 4096
    a, b, exp = _pair(oracle_mod, n, m, "similar")
    strips = (n - 2 + 125) // 126
    trace = torch.zeros(16 * strips, dtype=torch.int64, device="cuda")
    engine.set_option("trace", trace.data_ptr())
    got, st = _score(engine, a, b)
    engine.set_option("trace", 0)
    torch.cuda.synchronize()
    assert got == exp and not st["variant"] & WEDGE, (got, exp, st)


def test_stalled_item_still_times_out(engine, oracle_mod):
    """The bounded waits still end a launch whose producer never publishes (option stall_item, the pattern of
    tests/test_gpu_parity.py test_flow2_loader_wave_timeout: flow2's staged kernel, the only one the option acts
    in): ERR_TIMEOUT within seconds, and the next launches, a wedge launch among them, score correctly."""
    rng = np.random.default_rng(77)
    a, b = ACGT[rng.integers(0, 4, 2000)], ACGT[rng.integers(0, 4, 500)]
    prm = engine.Params(2, -3, 5, 2)
    engine.set_option("mode", 5)
    engine.set_option("f3a", 0)
    engine.set_option("timeout", 1)
    try:
        engine.set_option("stall_item", 0)
        t0 = time.time()
        with pytest.raises(engine.SwError):
            engine.score(a, b, prm)
        assert time.time() - t0 < 60
        engine.set_option("stall_item", -1)
        assert engine.score(a, b, prm) == oracle_mod.score_linear(a, b, oracle_mod.Params(2, -3, 5, 2))
    finally:
        engine.set_option("stall_item", -1)
        engine.set_option("timeout", 5)
        engine.set_option("f3a", 1)
        engine.set_option("mode", -1)
    x, y, exp = _pair(oracle_mod, 4096, 30037, "early")
    assert _score(engine, x, y)[0] == exp
