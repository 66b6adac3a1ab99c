"""CPU: the host side of the cooperative score path (include/algoGPU.h sw_score_matrix_batch_coop,
sw_matrix_coop_plan): the plan's arithmetic, the refusal above option coop_mb,
the argument errors of the Python layer and the ranges of the two options.  No GPU call is made."""
import numpy as np
import pytest

OPTS = ("W", "orient", "coop_mb", "coop_poison")


@pytest.fixture
def sw():
    import concurrentproject_amd as eng
    eng.lib()
    before = {k: eng.get_option(k) for k in OPTS}
    yield eng
    for k, v in before.items():
        eng.set_option(k, v)


def strips(n, W):
    return -(-n // (64 * W))


# (n, m, W, mode) -> (swap, columns, rows): by hand from the contract.  The estimate is
# (rows + strips * 64 * (W + 1)) * (the time of a step at that W), the same factor for both orientations of a
# pair, so the orientation with the smaller rows + strips * 64 * (W + 1) wins and a tie keeps seq1.
CASES = [
    # a square pair: both orientations cost the same, seq1 stays across the lanes
    ((4096, 4096, 1, "local"), (0, 4096, 4096)),
    ((4096, 4096, 8, "global"), (0, 4096, 4096)),
    # W = 1: a strip costs 128 steps for 64 columns, a row one: the longer sequence streams
    ((1000, 5000, 1, "local"), (0, 1000, 5000)),       # 5000 + 16 * 128 = 7048 < 1000 + 79 * 128 = 11112
    ((5000, 1000, 1, "local"), (1, 1000, 5000)),
    ((5000, 1000, 1, "global"), (1, 1000, 5000)),
    ((5000, 1000, 1, "semiglobal"), (0, 5000, 1000)),  # semi-global: seq1 always across the lanes
    # W = 8: a strip costs 576 steps for 512 columns: 1000 + 10 * 576 = 6760 > 5000 + 2 * 576 = 6152
    ((5000, 1000, 8, "local"), (1, 1000, 5000)),
    ((129, 64, 2, "local"), (1, 64, 129)),             # 64 + 2 * 192 = 448 > 129 + 1 * 192 = 321
    ((1, 1, 4, "global"), (0, 1, 1)),
]


@pytest.mark.parametrize("case,want", CASES)
def test_plan_arithmetic(sw, case, want):
    n, m, W, mode = case
    swap, cols, rows = want
    sw.set_option("W", W)
    p = sw.coop_plan(n, m, mode)
    s = strips(cols, W)
    assert p == {"W": W, "strips": s, "swap": swap, "edge_bytes": (s - 1) * rows * 8, "items": s}


def test_plan_of_an_empty_pair_and_the_automatic_w(sw):
    sw.set_option("W", 0)
    assert sw.coop_plan(0, 100) == {"W": 0, "strips": 0, "swap": 0, "edge_bytes": 0, "items": 0}
    assert sw.coop_plan(100, 0, "global")["items"] == 0
    # one long pair: 32768 + 256 * 192 = 81920 steps of 106 ns at W = 2 against 98304 of 93 ns at W = 1,
    # 73728 of 147 ns at W = 4 and 69632 of 263 ns at W = 8
    p = sw.coop_plan(32768, 32768, "global")
    assert p["W"] == 2 and p["strips"] == 256 and p["edge_bytes"] == 255 * 32768 * 8
    # a short pair of one strip at every W: no hand-off, and the shortest step wins
    p = sw.coop_plan(40, 40)
    assert p["W"] == 1 and p["strips"] == 1 and p["edge_bytes"] == 0 and p["items"] == 1


def test_memory_decides_the_w(sw):
    sw.set_option("W", 0)
    assert sw.coop_plan(8192, 8192)["W"] == 2
    sw.set_option("coop_mb", 1)
    # 8192 x 8192 under 1 MiB: 63 * 8192 * 8 = 4128768 B at W = 2 and 2031616 B at W = 4 do not fit,
    # 15 * 8192 * 8 = 983040 B at W = 8 do
    p = sw.coop_plan(8192, 8192)
    assert p["W"] == 8 and p["edge_bytes"] == 983040 and p["swap"] == 0
    # 4096 x 4096: W = 1 needs 63 * 4096 * 8 = 2064384 B; W = 2, the cheapest, 1015808 B, which fit
    p = sw.coop_plan(4096, 4096)
    assert p["W"] == 2 and p["edge_bytes"] == 31 * 4096 * 8


def test_refusal_above_coop_mb_gives_the_bytes(sw):
    sw.set_option("W", 0)
    sw.set_option("coop_mb", 1)
    # at W = 8 a 16384 x 16384 pair has 32 strips: 31 * 16384 * 8 = 4063232 bytes, more than 1 MiB
    with pytest.raises(sw.SwError, match=r"pair 0: a 16384 x 16384 pair needs 4063232 bytes of edge columns.*coop_mb = 1 MiB"):
        sw.coop_plan(16384, 16384, "global")
    # a forced W is the one the bytes are given for
    sw.set_option("W", 1)
    with pytest.raises(sw.SwError, match=r"needs %d bytes of edge columns.*W = 1" % (63 * 4096 * 8)):
        sw.coop_plan(4096, 4096)
    sw.set_option("coop_mb", 2)
    assert sw.coop_plan(4096, 4096)["edge_bytes"] == 63 * 4096 * 8
    # the batch call refuses such a pair before it touches a device, and names its input index
    sw.set_option("coop_mb", 1)
    a = np.full(4096, ord("A"), np.uint8)
    with sw.Matrix(b"AC", np.array([[2, -1], [-1, 2]], np.int8)) as mx:
        with pytest.raises(sw.SwError, match=r"pair 1: a 4096 x 4096 pair needs %d bytes" % (63 * 4096 * 8)):
            sw.score_matrix_batch([(a[:10], a[:10]), (a, a)], mx, 3, 1, coop=True)


def test_value_errors(sw):
    a = np.full(10, ord("A"), np.uint8)
    with sw.Matrix(b"AC", np.array([[2, -1], [-1, 2]], np.int8)) as mx:
        with pytest.raises(ValueError, match=r"band= is not built for coop=True"):
            sw.score_matrix(a, a, mx, 3, 1, band=4, coop=True)
        with pytest.raises(ValueError, match=r"band= is not built for coop=True"):
            sw.score_matrix_batch([(a, a)], mx, 3, 1, mode="global", band=0, coop=True)
        with pytest.raises(ValueError, match="unknown alignment mode"):
            sw.score_matrix_batch([(a, a)], mx, 3, 1, mode="overlap", coop=True)
        assert sw.score_matrix_batch([], mx, 3, 1, coop=True) == []
    with pytest.raises(ValueError, match="coop=True needs a substitution matrix"):
        sw.score_matrix_batch([(a, a)], None, 3, 1, coop=True)
    with pytest.raises(ValueError, match="unknown alignment mode"):
        sw.coop_plan(10, 10, "overlap")
    with pytest.raises(sw.SwError, match="sw_matrix_coop_plan: invalid arguments"):
        sw.coop_plan(-1, 10)
    assert "coop_plan" in sw.__all__


@pytest.mark.parametrize("key,default,good,bad", [
    ("coop_mb", 1024, (1, 1024, 3072), (0, -1, 3073)),
    ("coop_poison", 0, (0, 1), (-1, 2)),
])
def test_option_ranges(sw, key, default, good, bad):
    import subprocess
    import sys
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", "import concurrentproject_amd as sw; print(sw.get_option(%r))" % key],
                         cwd=root, check=True, capture_output=True, text=True).stdout
    assert int(out.strip().splitlines()[-1]) == default
    for v in good:
        sw.set_option(key, v)
        assert sw.get_option(key) == v
        for r in bad:
            with pytest.raises(sw.SwError):
                sw.set_option(key, r)
            assert sw.get_option(key) == v
