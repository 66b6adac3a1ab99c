"""GPU parity of the wedge launches at the corners of the scoring-constant domain: test_param_corners.CORNERS over
the launches that score one long DNA pair on the staged two-column linear-gap kernel: the
uniform two-wedge plan, the steep staircase with its hand-off columns, the join inside the staged kernel
(sw_flow3.hip f3_join_strip) and, with SWMI_F3JOIN = 0, sw_flow3_wedge_combine_kernel and
sw_flow3_steep_combine_kernel.  tests/test_flow3_wedge.py, test_flow3_steep.py and test_flow3_join.py run these
launches at three constant sets with small MATCH, MISMATCH < 0 and G > 0; here come free gaps (the granules carry
H - G = H and 0 is a legitimate value), G = 100 (every granule holds a negative H - G that the join adds G back
to), MISMATCH = 0 (dead columns and rows must still contribute nothing), MATCH = 127 (the largest H_F + H_B; 127 000
in the score word) and MATCH <= 0 (the score slot reads 0 because the last strip wrote 0).

The plan is forced as in those files (option orient = 1, SWMI_F3WEDGE = 1, SWMI_F3WEDGE_DROPS, SWMI_F3JOIN), over
the three drop patterns and both join settings.  Whether a set is admissible is computed from the documented rules
restated in test_param_corners (flow_ok, linear), never by asking the engine:
  admissible      every score equals oracle.score_linear and sw_last_stats proves the launch (mode 5, variant bit
                  18, bit 19 exactly on a steep pattern, bit 6, bit 17 clear, two chains' groups of items);
  not admissible  a forced mode = 5 launch raises SwError where the score byte does not fit and runs an affine set
                  without bit 18; the automatic plan is exact without bit 18.
The inputs, and the proof on the CPU models that the crossing term and the hand-off columns decide them at these
sets, are in tests/test_wedge_corners_cpu.py."""
import os

import numpy as np
import pytest

from test_param_corners import ACGT, CORNERS, flow_ok, linear
from test_steep_identity import steep_plan
from test_wedge_corners_cpu import ADMITTED, IDENT, PATTERNS, STEEP_PATTERNS, UNIFORM, ZERO, expected, inputs, stretched
from test_wedge_identity import wedge_plan

pytestmark = pytest.mark.gpu

WEDGE = 1 << 18
STEEP = 1 << 19
CUT = 1 << 17
STAGED = 64
ENV = "SWMI_F3WEDGE"
ENV_DROPS = "SWMI_F3WEDGE_DROPS"
ENV_JOIN = "SWMI_F3JOIN"
JOINS = [True, False]

# counted by hand from the table: 10 sets are flow_ok with G_INIT == G_EXT (test_param_corners.N_FLOW_LIN); of
# the other 19, M + G_INIT = 128 twice and G_INIT >= 65408 four times leave the score byte, 13 are affine
N_ADMITTED, N_REFUSED, N_AFFINE = 10, 6, 13
HIGH = [(127, 0, 0, 0), (127, -127, 0, 0)]     # the identical pair scores 127 000 under both
FREE, STIFF = (127, 0, 0, 0), (27, -127, 100, 100)


@pytest.fixture(autouse=True)
def _defaults(engine, request):
    def reset():
        for k in (ENV, ENV_DROPS, ENV_JOIN):
            os.environ.pop(k, None)
        engine.set_params(engine.Params())
        engine.set_option("mode", -1)
        engine.set_option("orient", 0)
    request.addfinalizer(reset)
    engine.set_option("orient", 1)   # seq1 across the lanes: n is its length
    os.environ[ENV] = "1"


def _plan(d, join):
    os.environ[ENV_DROPS] = ",".join(str(x) for x in d)
    if join:
        os.environ.pop(ENV_JOIN, None)
    else:
        os.environ[ENV_JOIN] = "0"


def _proves(st, d, tag):
    """sw_last_stats of a wedge launch of pattern d over the input `tag`"""
    groups = (wedge_plan(tag[2], 1 << 20)[0] + 3) // 4
    v = st["variant"]
    return (st["mode"] == 5 and v & WEDGE and bool(v & STEEP) == (d != UNIFORM) and v & STAGED and not v & CUT and
            st["items"] == 2 * groups and st["dna"] == (2 if tag[0] == "acgtn" else 1))


def _score(engine, a, b, t):
    return engine.score(a, b, engine.Params(*t)), engine.last_stats()


@pytest.mark.parametrize("join", JOINS)
@pytest.mark.parametrize("d", PATTERNS)
def test_admitted_sets(engine, oracle_mod, d, join):
    """Every admitted set over every input, on one context and one score buffer.  Each MATCH <= 0 set follows
    the identical pair at 127 000 directly and starts with that pair: its 0 must be written, not left over."""
    _plan(d, join)
    ins = inputs(d)
    ident = ins[-1]
    count = 0
    for k, t in enumerate(t for t in CORNERS if flow_ok(t) and linear(t)):
        count += 1
        exp = expected(oracle_mod, d, t)
        order = list(range(len(ins)))
        if t[0] <= 0:
            got, st = _score(engine, ident[1], ident[2], HIGH[k % 2])
            assert got == 127 * IDENT and _proves(st, d, ident[0]), (d, join, HIGH[k % 2], got, st)
            order = order[-1:] + order[:-1]
            assert exp == [0] * len(ins)
        for i in order:
            tag, a, b = ins[i]
            got, st = _score(engine, a, b, t)
            assert got == exp[i], (d, join, t, tag, got, exp[i], st)
            assert _proves(st, d, tag), (d, join, t, tag, st)
    assert count == N_ADMITTED == len(ADMITTED) and len(ZERO) == 3


@pytest.mark.parametrize("join", JOINS)
@pytest.mark.parametrize("d", PATTERNS)
def test_gap_alternation(engine, oracle_mod, d, join):
    """G = 100 directly after G = 0 on the same shape and buffers, and the reverse: the segment and edge granules
    of the two launches differ by the epoch key alone."""
    _plan(d, join)
    for i, (tag, a, b) in enumerate(inputs(d)):
        for t in (FREE, STIFF, HIGH[1], STIFF, FREE):
            got, st = _score(engine, a, b, t)
            assert got == expected(oracle_mod, d, t)[i], (d, join, t, tag, got, st)
            assert _proves(st, d, tag), (d, join, t, tag, st)


@pytest.mark.parametrize("join", JOINS)
@pytest.mark.parametrize("d", PATTERNS)
def test_sets_not_admitted(engine, oracle_mod, d, join):
    """The other 19 sets on the 1000-column inputs at the admission edge + 17 and the identical pair: refused or
    run without the wedge when mode 5 is forced, exact without it on the automatic plan."""
    _plan(d, join)
    ins = inputs(d)
    pick = [i for i, (tag, _, _) in enumerate(ins) if tag[2] == 1000 and tag[3] < 1300]
    assert len(pick) == 5 and {ins[i][0][0] for i in pick} == {"acgt", "acgtn"}
    refused = affine = 0
    for t in CORNERS:
        if flow_ok(t) and linear(t):
            continue
        for i, want in zip(pick, expected(oracle_mod, d, t, pick)):
            tag, a, b = ins[i]
            engine.set_option("mode", 5)
            if not flow_ok(t):
                with pytest.raises(engine.SwError):
                    engine.score(a, b, engine.Params(*t))
            else:
                got, st = _score(engine, a, b, t)
                assert got == want and st["mode"] == 5 and not st["variant"] & WEDGE, (d, join, t, tag, got, want, st)
            engine.set_option("mode", -1)
            got, st = _score(engine, a, b, t)      # the automatic plan
            assert got == want and not st["variant"] & WEDGE, (d, join, t, tag, "automatic plan", got, want, st)
        refused += not flow_ok(t)
        affine += flow_ok(t)
    assert (refused, affine) == (N_REFUSED, N_AFFINE) and refused + affine + N_ADMITTED == len(CORNERS) == 29


@pytest.mark.parametrize("join", JOINS)
def test_device_entry_point(engine, oracle_mod, join):
    """sw_score_batch_device, the call the benchmark times: one pair, whose slot nothing clears before the kernel's
    last strip writes it, and the pair between two empty ones (prepare_device's nscores > 1 branch), whose slots
    must read 0.  Free gaps, G = 100 and MISMATCH = 0 with paid gaps."""
    import torch
    d = STEEP_PATTERNS[0]
    _plan(d, join)
    ins = inputs(d)
    i = next(i for i, (tag, _, _) in enumerate(ins) if tag[:3] == ("acgt", "stretched", 1000))
    tag, a, b = ins[i]
    boff = (len(a) + 63) // 64 * 64
    host = np.zeros(boff + (len(b) + 63) // 64 * 64 + 64, np.uint8)
    host[:len(a)] = a
    host[boff:boff + len(b)] = b
    arena = torch.from_numpy(host).cuda()
    for t in (FREE, STIFF, (5, 0, 3, 3)):
        exp = expected(oracle_mod, d, t)[i]
        assert exp > 0
        engine.set_params(engine.Params(*t))
        sc = torch.full((3,), 0x55555555, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        engine.score_batch_device(arena.data_ptr(), [0], [len(a)], [boff], [len(b)], sc.data_ptr(), flags=1)
        st = engine.last_stats()
        assert sc.tolist() == [exp, 0x55555555, 0x55555555] and _proves(st, d, tag), (join, t, sc.tolist(), exp, st)
        sc.fill_(0x55555555)
        torch.cuda.synchronize()
        engine.score_batch_device(arena.data_ptr(), [0, 0, 0], [0, len(a), 0], [0, boff, 0], [0, len(b), 0],
                                  sc.data_ptr(), flags=1)
        st = engine.last_stats()
        assert sc.tolist() == [0, exp, 0] and _proves(st, d, tag), (join, t, sc.tolist(), exp, st)


def _boundary_bytes(n, m, d):
    """sw_last_stats' boundary_bytes of a steep launch with the drops d (sw_engine.hip plan_wedge): both chains'
    group edges of max(e0) + 64 rows, two boundary buffers of 128 granules a strip and two segment buffers of
    max(d) - 62 eight-byte entries a strip, in 16-byte granules"""
    S, _, _, e0f, e0b, _ = steep_plan(n, m, d)
    return 16 * (2 * ((S + 3) // 4) * (max(e0f, e0b) + 64) + 256 * S + S * (max(d) - 62))


def test_automatic_plan(engine, oracle_mod):
    """All three variables unset, 4096 columns against a stretched copy of 4300 rows: the steep plan with
    (64,128,64,128), the pattern of a launch with no more groups than CUs (sw_engine.hip F3_STEEP_AUTO_DROPS; 18
    groups here), which the boundary arena's size tells from the queued pattern and from the uniform plan."""
    for k in (ENV, ENV_DROPS, ENV_JOIN):
        os.environ.pop(k, None)
    rng = np.random.default_rng(4096)
    n, m = 4096, 4300
    a = ACGT[rng.integers(0, 4, n)]
    b = stretched(rng, ACGT, a, m)
    want = _boundary_bytes(n, m, STEEP_PATTERNS[0])
    assert want != _boundary_bytes(n, m, STEEP_PATTERNS[1])
    for t in (HIGH[1], STIFF):
        got, st = _score(engine, a, b, t)
        assert got == oracle_mod.score_linear(a, b, oracle_mod.Params(*t)), (t, got, st)
        assert _proves(st, STEEP_PATTERNS[0], ("acgt", "stretched", n, m)), (t, st)
        assert st["boundary_bytes"] == want, (t, st, want)
