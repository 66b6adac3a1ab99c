"""GPU: the cooperative score path (include/algoGPU.h sw_score_matrix_batch_coop; csrc/sw_matrix.hip
sw_matrix_coop_kernel): the strips of one pair on as many waves, each handing
its right edge to the wave on its right inside one launch.

The reference is the CPU aligner's score (align_matrix_batch(cpu=True, mode=...)), and for the two
largest pairs the unchanged one-wave kernel (score_matrix_batch(mode=...)); the cooperative path is
never compared with itself.  Every test runs with option coop_poison = 1: the host fills the edge
columns with 0x3F bytes before each launch, so a row consumed before it was stored carries H of about
10^9 into the score."""
import threading

import numpy as np
import pytest

from test_matrix import SYMBOLS, mutated_copy, rand_seq, table  # noqa: F401  (table: a fixture)
from test_matrix_cpu import random_table

MODES = ("local", "global", "semiglobal")
OPTS = ("W", "blocks", "orient", "coop_mb", "coop_poison")


@pytest.fixture
def coop(engine, request):
    """The engine with coop_poison = 1; every option a test may touch is put back afterwards."""
    before = {k: engine.get_option(k) for k in OPTS}
    request.addfinalizer(lambda: [engine.set_option(k, v) for k, v in before.items()])
    engine.set_option("coop_poison", 1)
    return engine


def cpu_scores(engine, pairs, T, gaps, mode):
    with engine.Matrix(SYMBOLS, T) as mx:
        return [x.score for x in engine.align_matrix_batch(pairs, mx, *gaps, cpu=True, mode=mode)]


def coop_scores(engine, pairs, T, gaps, mode):
    with engine.Matrix(SYMBOLS, T) as mx:
        return engine.score_matrix_batch(pairs, mx, *gaps, mode=mode, coop=True)


def strips_of(engine, pairs, mode):
    """Sum of the plans' strips: what last_stats()["items"] must report."""
    return sum(engine.coop_plan(len(a), len(b), mode)["strips"] for a, b in pairs)


def edge_pairs(W):
    rng = np.random.default_rng(160 + W)
    SW = 64 * W
    pairs = []
    for i, n in enumerate((1, SW - 1, SW, SW + 1, 3 * SW + 5)):
        for j, m in enumerate((1, 63, 64, 65, SW + 1, 300)):
            a = rand_seq(rng, n)
            pairs.append((a, rand_seq(rng, m)))
            pairs.append((a, mutated_copy(rng, a, m)))
    return pairs


# 1. every strip boundary and chunk edge at every W, every mode; many pairs' items interleave
@pytest.mark.gpu
@pytest.mark.parametrize("gaps", [(12, 1), (0, 0), (1, 3)])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("W", [1, 2, 4, 8])
def test_edges(coop, table, W, mode, gaps):
    pairs = edge_pairs(W)
    want = cpu_scores(coop, pairs, table, gaps, mode)
    coop.set_option("W", W)
    got = coop_scores(coop, pairs, table, gaps, mode)
    st = coop.last_stats()
    assert got == want
    assert (st["mode"], st["W"], st["variant"]) == (11, W, MODES.index(mode))
    assert st["items"] == strips_of(coop, pairs, mode) > len(pairs)
    assert st["cells"] == sum(len(a) * len(b) for a, b in pairs)


# 2. more strips than waves: one workgroup's four waves work through 20 strips; the same call twice,
#    so the progress words must be zeroed again
@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("W", [1, 2])
def test_more_strips_than_waves(coop, table, W, mode):
    rng = np.random.default_rng(170 + W)
    a = rand_seq(rng, 20 * 64 * W)
    pairs = [(a, mutated_copy(rng, a, 1000))]
    want = cpu_scores(coop, pairs, table, (12, 1), mode)
    coop.set_option("W", W)
    coop.set_option("blocks", 1)
    coop.set_option("orient", 1)   # seq1, the 20 strips, across the lanes in local and global mode too
    for _ in range(2):
        assert coop_scores(coop, pairs, table, (12, 1), mode) == want
        st = coop.last_stats()
        assert st["blocks"] == 1 and st["items"] == 20


# 3. stale lines: two different pairs of one shape in one launch on one workgroup, then the same
#    shapes with the contents exchanged: a consumer served from a cached edge of the other pair,
#    or of the call before, gets the other pair's score
@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_stale_lines(coop, table, mode):
    rng = np.random.default_rng(180)
    a, c = rand_seq(rng, 6 * 64), rand_seq(rng, 6 * 64)
    p, q = (a, mutated_copy(rng, a, 500)), (c, mutated_copy(rng, c, 500))
    want = cpu_scores(coop, [p, q], table, (12, 1), mode)
    assert want[0] != want[1]
    coop.set_option("W", 1)
    coop.set_option("blocks", 1)
    coop.set_option("orient", 1)
    assert coop.coop_plan(384, 500, mode)["strips"] == 6
    assert coop_scores(coop, [p, q], table, (12, 1), mode) == want
    assert coop_scores(coop, [q, p], table, (12, 1), mode) == want[::-1]
    assert coop_scores(coop, [p, q], table, (12, 1), mode) == want


# 4. short rows: with m < 64 a strip's first publication is already its last; m = 1
@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("m", [1, 37])
def test_short_rows(coop, table, mode, m):
    rng = np.random.default_rng(190 + m)
    a = rand_seq(rng, 10 * 64 - 3)
    pairs = [(a, mutated_copy(rng, a[200:], m)), (a, rand_seq(rng, m))]
    want = cpu_scores(coop, pairs, table, (3, 1), mode)
    coop.set_option("W", 1)
    coop.set_option("orient", 1)
    assert coop_scores(coop, pairs, table, (3, 1), mode) == want
    assert coop.last_stats()["items"] == 20


# 5. a batch that does not fit option coop_mb runs as several launches
@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_several_launches(coop, table, mode):
    rng = np.random.default_rng(200)
    coop.set_option("W", 1)
    coop.set_option("coop_mb", 1)
    pairs = []
    for k in range(3):       # 1536 x 1200 at W = 1: 23 * 1200 * 8 = 220800 B, or 18 * 1536 * 8 swapped: four fit 1 MiB
        a = rand_seq(rng, 1536)
        pairs += [(a, mutated_copy(rng, a, 1200)) for _ in range(4)]
    plans = [coop.coop_plan(len(a), len(b), mode) for a, b in pairs]
    need = [p["edge_bytes"] for p in plans]
    # the launches the contract describes: pairs packed in input order under the budget
    launches, cur = [], 0
    for x in need:
        if cur and cur + x > (1 << 20):
            launches.append(cur)
            cur = 0
        cur += x
    launches.append(cur)
    assert len(launches) == 3
    want = cpu_scores(coop, pairs, table, (12, 1), mode)
    assert coop_scores(coop, pairs, table, (12, 1), mode) == want
    st = coop.last_stats()
    assert st["boundary_bytes"] == max(launches)
    assert st["items"] == sum(p["strips"] for p in plans)


# 6. a long gap across hand-offs: at W = 1 a 200-residue deletion spans three strips
@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("gaps", [(12, 1), (3, 1)])
def test_long_gaps_across_the_hand_offs(coop, table, gaps, mode):
    rng = np.random.default_rng(73)
    pairs = []
    for block in (40, 200):
        for at in (100, 450, 511, 512, 600):
            a = rand_seq(rng, 900, 20)
            b = np.concatenate([a[:at], a[at + block:]])
            pairs += [(a, b), (b, a)]
    want = cpu_scores(coop, pairs, table, gaps, mode)
    coop.set_option("W", 1)
    assert coop_scores(coop, pairs, table, gaps, mode) == want


# 7. two larger pairs at the automatic W, against the one-wave kernel
@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_two_larger_pairs(coop, table, mode):
    rng = np.random.default_rng(210)
    a, b = rand_seq(rng, 8192), rand_seq(rng, 4096)
    pairs = [(a, mutated_copy(rng, a[2000:], 4096)), (b, mutated_copy(rng, b, 8192))]
    with coop.Matrix(SYMBOLS, table) as mx:
        want = coop.score_matrix_batch(pairs, mx, 12, 1, mode=mode)
        assert coop.last_stats()["mode"] == 6
        got = coop.score_matrix_batch(pairs, mx, 12, 1, mode=mode, coop=True)
    st = coop.last_stats()
    assert got == want
    assert st["mode"] == 11 and st["items"] == strips_of(coop, pairs, mode) and st["items"] >= 16


# 8. two host threads at once
@pytest.mark.gpu
def test_two_host_threads(coop):
    rng = np.random.default_rng(220)
    jobs = []
    for t in range(2):
        T = random_table(rng, 24)
        pairs = []
        for _ in range(40):
            a = rand_seq(rng, int(rng.integers(1, 700)))
            pairs.append((a, mutated_copy(rng, a, int(rng.integers(1, 400)))))
        jobs.append((T, pairs, (12, 1) if t == 0 else (4, 2), "global" if t == 0 else "local"))
    got, errors = [None, None], []
    start = threading.Barrier(2)

    def run(t):
        try:
            T, pairs, gaps, mode = jobs[t]
            with coop.Matrix(SYMBOLS, T) as mx:
                start.wait(timeout=60)
                for _ in range(3):
                    got[t] = coop.score_matrix_batch(pairs, mx, *gaps, mode=mode, coop=True)
        except Exception as e:      # reported by the main thread
            errors.append(e)

    threads = [threading.Thread(target=run, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for t, (T, pairs, gaps, mode) in enumerate(jobs):
        assert got[t] == cpu_scores(coop, pairs, T, gaps, mode)
