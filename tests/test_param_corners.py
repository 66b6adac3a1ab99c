"""GPU parity at the corners of the scoring-constant domain (include/algoGPU.h sw_set_params, DESIGN.md
section 2), over every kernel family.

The documented domain is 0 <= G_INIT, G_EXT <= 2^20, -127 <= MISMATCH <= 0, MISMATCH <= MATCH <= 127, and
every family takes a sub-domain of it through a host predicate of its own (flow2_fits, pwg3_fits, duo_fits,
duo_f16_fits, duo_raw_ok in csrc/sw_engine.hip).  CORNERS sits on the edges of those predicates, the last five
sets on the same edges with G_INIT == G_EXT (the linear-gap step's kernels: M + G_INIT = 127 in and 128 out at
G = 100, MISMATCH = 0 with free and with paid gaps; tests/test_wedge_corners.py runs them, and the rest of the
table, over the wedge launches of one long pair).  Each test
forces one family with the options the family's own test file uses, proves from last_stats() that the
family ran, and compares every score bit for bit with oracle.score_linear (lazySmith.cpp:15-69 restated;
pinned to the reference's own code at every corner set by tests/test_corners_cpu.py).

Whether a set is admissible to a family is computed HERE, from the documented rules restated in Python
(flow_ok, duo_ok, f16_ok, raw_ok below) and never by asking the engine:
  admissible      the family's stats bits must be set and the scores exact;
  not admissible  a forced launch raises SwError where the engine refuses (mode 3, mode 5), and the
                  automatic plan is exact on another kernel.
Every family asserts how many sets it admitted, so a predicate that rejects everything cannot pass.

Shapes are the smallest that still cross every hand-off of a family: 1 x 1, 1 x 130, a random pair, a
mutated copy whose two indels lie at the family's strip and group boundaries, an identical pair, and widths
just past two strip groups.  tests/test_corners_cpu.py checks on the oracle alone that these inputs make the
constants matter."""
import numpy as np
import pytest

G20 = 1 << 20

# (MATCH, MISMATCH, G_INIT, G_EXT)   the predicate edge the set sits on
CORNERS = [
    (127, -127, 0, 0),         # M+GI = 127 in; MI+GI = -127; M-MI = 254: duo in, raw duo out; free gaps; linear step
    (127, -127, 0, 1),         # the same edges on the affine step: G_EXT > G_INIT = 0
    (126, -127, 1, 0),         # the same edges on the affine step: free extension
    (27, -127, 100, 1),        # M+GI = 127: the last set inside flow2 / flow3 / pwg3
    (28, -127, 100, 1),        # M+GI = 128: the first one outside
    (1, -127, 0, 5),           # MI+GI = -127; G_INIT = 0 with G_EXT > 0
    (64, -63, 5, 2),           # M-MI = 127: raw duo in
    (64, -64, 5, 2),           # M-MI = 128: raw duo out, the DNA duo unaffected
    (127, -1, 65408, 65535),   # GI+M = 65535 and GE = 65535: duo in
    (127, -1, 65409, 1),       # GI+M = 65536: duo out by one
    (1, -1, 1, 65536),         # GE = 65536: duo out by one
    (127, -1, G20, G20),       # the domain maximum: int32 kernels only
    (1, -1, G20, 0),           # G_INIT at the maximum, free extension: int32 kernels only
    (1, -1, 0, G20),           # G_EXT at the maximum, free opening: int32 kernels only
    (1, -1, 1, 3),             # G_EXT > G_INIT
    (3, -2, 2, 9),             # G_EXT > G_INIT
    (5, 0, 0, 3),              # MISMATCH = 0: raw duo out
    (1, 0, 0, 0),              # MISMATCH = 0, free gaps: raw duo out
    (0, 0, 0, 0),              # MATCH = 0: every score is 0
    (0, -5, 3, 1),             # MATCH = 0: every score is 0
    (-1, -2, 1, 1),            # MATCH < 0: every score is 0; duo out (A = H + MATCH is an unsigned half)
    (-127, -127, 0, 0),        # MATCH = MISMATCH = -127: every score is 0; duo out
    (1, -1, 1, 1),             # control: the reference's constants
    (2, -3, 5, 2),             # control: affine
    # the same edges on the linear-gap step (G_INIT == G_EXT: the two-column kernels, and the wedge launches of
    # tests/test_wedge_corners.py)
    (27, -127, 100, 100),      # M+GI = 127 on the linear step: the last set inside
    (28, -127, 100, 100),      # M+GI = 128 on the linear step: the first one outside
    (100, -1, 27, 27),         # M+GI = 127 from the MATCH side; M-MI = 101: raw duo in
    (127, 0, 0, 0),            # MATCH max, MISMATCH = 0, free gaps: 127 * LCS; raw duo out
    (5, 0, 3, 3),              # MISMATCH = 0 with paid linear gaps: raw duo out
]

ACGT = np.frombuffer(b"ACGT", np.uint8)
ACGTN = np.frombuffer(b"ACGTN", np.uint8)
PROTEIN = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)


# ---- the documented rules, restated (algoGPU.h option "mode") ------------------------

def flow_ok(t):
    """flow2 / flow3 / pwg3: the score byte s + G_INIT is a signed byte above the -128 sentinel."""
    ma, mi, gi, _ = t
    return ma + gi <= 127 and mi + gi >= -127


def raw_ok(t):
    """Raw-byte duos: the penalty MATCH - s comes from the bytes, capped at MATCH - MISMATCH <= 127."""
    ma, mi, _, _ = t
    return mi < 0 and ma - mi <= 127


def duo_ok(t, pairs, raw=False):
    """16-bit duos: A = H + MATCH in an unsigned half (so MATCH >= 0), every constant a u16."""
    ma, mi, gi, ge = t
    if ma < 0 or gi + ma > 65535 or ge > 65535 or ma - mi > 254 or (raw and not raw_ok(t)):
        return False
    return all(max(ma, 1) * min(len(a), len(b)) + ma <= 65535 for a, b in pairs)


def f16_ok(t, pairs):
    """The duo's f16 max3 variant: every value a finite f16 bit pattern."""
    return all(max(t[0], 1) * (min(len(a), len(b)) + 1) <= 0x7BFF for a, b in pairs)


def linear(t):
    return t[2] == t[3]


# How many of the 29 sets each rule admits, counted by hand from the table:
N_FLOW = 23       # out: M+GI = 128 twice (affine and linear), and the four sets with G_INIT of 65408 or more
N_FLOW_LIN = 10   # of those, G_INIT == G_EXT: (127,-127,0,0), (1,0,0,0), (0,0,0,0), (-1,-2,1,1), (-127,-127,0,0), (1,-1,1,1),
                  # (27,-127,100,100), (100,-1,27,27), (127,0,0,0), (5,0,3,3)
N_DUO = 22        # out: GI+M = 65536, GE = 65536, the three 2^20 sets, MATCH < 0 twice
N_DUO_RAW = 7     # (64,-63,5,2), (1,-1,1,3), (3,-2,2,9), (0,-5,3,1), the two controls and (100,-1,27,27)


# ---- inputs ---------------------------------------------------------------------------------------------

def rand_seq(rng, alpha, n):
    return alpha[rng.integers(0, len(alpha), n)]


def mutated(rng, alpha, a, lo, m, at):
    """m rows made from the columns a[lo:]: ~7 % substitutions, and a deletion and an insertion of 1-3
    residues at the columns `at` of a (a strip and a group boundary of the family)."""
    b = a[lo:lo + m + 4].copy()
    sub = rng.random(len(b)) < 0.07
    b[sub] = rand_seq(rng, alpha, int(sub.sum()))
    d, i = sorted(c - lo for c in at)
    assert 2 < d < i < len(b) - 4, (lo, m, at)
    b = np.insert(b, i, rand_seq(rng, alpha, int(rng.integers(1, 4))))
    b = np.delete(b, slice(d, d + int(rng.integers(1, 4))))
    if len(b) < m:
        b = np.concatenate([b, rand_seq(rng, alpha, m - len(b))])
    return np.ascontiguousarray(b[:m])


def family_pairs(seed, alpha, wide, ident, small=(300, 200)):
    """1 x 1, 1 x 130, a random pair, an identical pair of `ident` residues and, per entry (n, lo, m, at) of
    `wide`, n columns against a mutated copy of a[lo:lo + m] with indels at the columns `at`."""
    rng = np.random.default_rng(seed)
    one = rand_seq(rng, alpha, 1)
    s = rand_seq(rng, alpha, ident)
    pairs = [(one, one.copy()), (one, np.concatenate([rand_seq(rng, alpha, 129), one])),
             (rand_seq(rng, alpha, small[0]), rand_seq(rng, alpha, small[1])), (s, s.copy())]
    for n, lo, m, at in wide:
        a = rand_seq(rng, alpha, n)
        pairs.append((a, mutated(rng, alpha, a, lo, m, at)))
    return pairs


# name -> (pairs, indices of the mutated pairs, indices of the identical pairs).  Columns are seq1
# (option orient = 1).  The duo lists keep min(n, m) <= 240 so that MATCH = 127 stays inside the u16 and f16
# ranges (the score-range edges have cases of their own, RANGE_CASES).
def _lists():
    out = {}

    def add(name, pairs, ident=(3,)):
        out[name] = (pairs, tuple(range(4, len(pairs))), ident)
    # strips of 64 W columns, groups of four: W = 1 boundaries at 64 / 256, W = 8 at 512 / (2048)
    add("legacy", family_pairs(1, ACGT, [(1030, 400, 300, (512, 640)), (1030, 760, 270, (1024, 832))], 1030))
    add("duo", family_pairs(2, ACGT, [(1030, 400, 240, (512, 576)), (1030, 800, 230, (1024, 960))], 240))
    add("duo_protein", family_pairs(3, PROTEIN, [(1030, 400, 240, (512, 576)), (1030, 800, 230, (1024, 960))], 240))
    add("duo_acgtn", family_pairs(4, ACGTN, [(1030, 400, 240, (512, 576)), (1030, 800, 230, (1024, 960))], 240))
    # flow2: strips of 63 (126 at two columns) new columns, groups of 252 (504)
    add("flow", family_pairs(5, ACGT, [(505, 150, 250, (252, 315)), (1000, 380, 300, (504, 630))], 300))
    # seven-letter pairs: every one wider than a strip (one strip takes the byte path)
    rng = np.random.default_rng(6)
    s = rand_seq(rng, ACGTN, 300)
    a5, a10 = rand_seq(rng, ACGTN, 505), rand_seq(rng, ACGTN, 1000)
    out["hep"] = ([(rand_seq(rng, ACGTN, 300), rand_seq(rng, ACGTN, 200)), (s, s.copy()),
                   (a5, mutated(rng, ACGTN, a5, 150, 250, (252, 315))),
                   (a10, mutated(rng, ACGTN, a10, 380, 300, (504, 630)))], (2, 3), (1,))
    # ring mode: 700 rows wrap a 512-row ring; groups of 504 columns at two per lane, 756 at three
    rng = np.random.default_rng(7)
    s = rand_seq(rng, ACGT, 1000)
    a10, a16 = rand_seq(rng, ACGT, 1000), rand_seq(rng, ACGT, 1600)
    out["ring"] = ([(a10, mutated(rng, ACGT, a10, 200, 700, (504, 756))), (s, s.copy()),
                    (a16, mutated(rng, ACGT, a16, 450, 700, (1008, 756))),
                    (rand_seq(rng, ACGT, 1600), rand_seq(rng, ACGT, 700))], (0, 2), (1,))
    # four / five columns per lane: strips of 252 (315) columns
    s = rand_seq(rng, ACGT, 1100)
    a11 = rand_seq(rng, ACGT, 1100)
    out["ring45"] = ([(a11, mutated(rng, ACGT, a11, 200, 700, (252, 756))), (s, s.copy()),
                      (rand_seq(rng, ACGT, 1100), rand_seq(rng, ACGT, 700))], (0,), (1,))
    # a pair per workgroup: strips of 189 columns, groups of 756
    add("pwg", family_pairs(8, ACGT, [(1030, 600, 300, (756, 700)), (800, 60, 250, (189, 126))], 300))
    return out


LISTS = _lists()

_EXP = {}


def expected(oracle_mod, name, t):
    """oracle.score_linear of list `name` under the constants t, computed once."""
    if (name, t) not in _EXP:
        op = oracle_mod.Params(*t)
        _EXP[name, t] = [oracle_mod.score_linear(a, b, op) for a, b in LISTS[name][0]]
    return _EXP[name, t]


# ---- the sweep ------------------------------------------------------------------------------------------

DEFAULTS = (("W", 0), ("C", 0), ("bytes", 0), ("blocks", 0), ("orient", 0), ("f2w", 0), ("mode", -1), ("ring", -1),
            ("ring_rows", 4096), ("linear", -1), ("duo16", 1), ("duo_lds", 1), ("duo_tab", 1), ("duo_raw", 1), ("f3", 1),
            ("f3a", 1), ("f3split", -1), ("f3pwg", 1), ("f2pwg", -1), ("f2stream", 0))


def reset(engine):
    engine.set_params(engine.Params())
    for k, v in DEFAULTS:
        engine.set_option(k, v)


@pytest.fixture(autouse=True)
def _defaults(engine):
    reset(engine)
    yield
    reset(engine)


def run(engine, pairs, p, single):
    """(scores, [(stats, pair or None)]): one launch per pair, or one for the batch."""
    if not single:
        return engine.score_batch(pairs, p), [(engine.last_stats(), None)]
    got, stats = [], []
    for a, b in pairs:
        got.append(engine.score(a, b, p))
        stats.append((engine.last_stats(), (a, b)))
    return got, stats


def sweep(engine, oracle_mod, name, force, admit, ran, refuses, admitted, single=False):
    """Every corner set on list `name`.  force(t) sets the family's options; admit(t) says whether the
    documented rules admit the set; ran(t, stats, pair) whether the family's kernel ran; refuses(t) whether
    the engine refuses the forced launch of a set that is not admitted."""
    pairs = LISTS[name][0]
    count = 0
    for t in CORNERS:
        p = engine.Params(*t)
        exp = expected(oracle_mod, name, t)
        reset(engine)
        if admit(t):
            count += 1
            force(t)
            got, stats = run(engine, pairs, p, single)
            for st, pair in stats:
                assert ran(t, st, pair), (t, st, pair and (len(pair[0]), len(pair[1])))
            assert got == exp, (t, got, exp)
            continue
        if refuses(t):
            force(t)
            try:
                got, refused = run(engine, pairs, p, single)[0], False
            except engine.SwError:
                got, refused = None, True
            assert refused, (t, "the forced launch was not refused; it scored", got, "expected", exp)
            reset(engine)
        got, stats = run(engine, pairs, p, single)      # the automatic plan
        assert got == exp, (t, "automatic plan", got, exp)
        for st, pair in stats:
            assert not ran(t, st, pair), (t, "automatic plan", st)
    assert count == admitted, (count, admitted)


def bits(st, on=0, off=0):
    return st["variant"] & on == on and not st["variant"] & off


pytestmark = pytest.mark.gpu


# ---- legacy int32 kernels: strip, pairwg, chain (modes 0 / 1 / 2) and flow (mode 4) ----------------------

@pytest.mark.parametrize("mode,W,C,force_bytes", [(mode, W, C, fb) for mode in (0, 1, 2) for W, C in ((1, 16), (8, 64))
                                                  for fb in (0, 1)] + [(4, 1, 16, 0), (4, 8, 64, 0)])
def test_legacy_int32(engine, oracle_mod, mode, W, C, force_bytes):
    """The only kernels the 2^20 and 65409-class sets reach: every set of the domain is admitted."""
    def force(t):
        for k, v in (("orient", 1), ("mode", mode), ("W", W), ("C", C), ("bytes", force_bytes)):
            engine.set_option(k, v)

    def ran(t, st, pair):
        return st["mode"] == mode and st["W"] == W and st["dna"] == 1 - force_bytes

    sweep(engine, oracle_mod, "legacy", force, lambda t: True, ran, lambda t: False, len(CORNERS))


# ---- 16-bit duos (mode 3) ---------------------------------------------------------------------------------

DUO_VARIANTS = [(d16, lin, lds, tab) for d16 in (1, 0) for lin in (-1, 0) for lds in (1, 0) for tab in (0, 2)]


def duo_force(engine, d16, lin, lds, tab):
    for k, v in (("orient", 1), ("mode", 3), ("W", 8), ("C", 64), ("duo16", d16), ("linear", lin), ("duo_lds", lds),
                 ("duo_tab", tab)):
        engine.set_option(k, v)


def duo_ran(t, st, pairs, d16, lin, lds, tab, dna=1):
    """mode 3; bit 0: the f16 max3 variant; bit 3: the linear-gap step (f16 duos only); bit 7: strip
    hand-offs in LDS; bit 8: row codes from the LDS table."""
    f16 = bool(d16) and f16_ok(t, pairs)
    want = (1 if f16 else 0) | (8 if f16 and lin and linear(t) else 0) | (128 if lds else 0) | (256 if lds and tab else 0)
    return st["mode"] == 3 and st["dna"] == dna and st["W"] == 8 and st["variant"] & (1 | 8 | 128 | 256) == want


@pytest.mark.parametrize("d16,lin,lds,tab", DUO_VARIANTS)
def test_duo_dna(engine, oracle_mod, d16, lin, lds, tab):
    pairs = LISTS["duo"][0]
    sweep(engine, oracle_mod, "duo", lambda t: duo_force(engine, d16, lin, lds, tab), lambda t: duo_ok(t, pairs),
          lambda t, st, pair: duo_ran(t, st, pairs, d16, lin, lds, tab), lambda t: True, N_DUO)


@pytest.mark.parametrize("name", ["duo_protein", "duo_acgtn"])
@pytest.mark.parametrize("d16,lds", [(1, 1), (0, 1), (1, 0)])
def test_duo_raw_bytes(engine, oracle_mod, name, d16, lds):
    """Byte batches on the duo kernels (option duo_raw): MISMATCH < 0 and MATCH - MISMATCH <= 127 besides."""
    pairs = LISTS[name][0]
    sweep(engine, oracle_mod, name, lambda t: duo_force(engine, d16, -1, lds, 2), lambda t: duo_ok(t, pairs, raw=True),
          lambda t, st, pair: duo_ran(t, st, pairs, d16, -1, lds, 2, dna=0), lambda t: True, N_DUO_RAW)


# Score-range edges on identical pairs: (MATCH, length, inside the u16 range, inside the f16 range)
RANGE_CASES = [
    (127, 515, True, False),    # score 65405, A = 65532: the last exact duo case at MATCH = 127
    (127, 516, False, False),   # score 65532, A = 65659: needs int32
    (127, 248, True, True),     # A = 31623 <= 0x7BFF: f16 in
    (127, 249, True, False),    # A = 31750: f16 out, u16 max
    (9, 3526, True, True),      # A = 31743 = 0x7BFF exactly
    (9, 3527, True, False),     # A = 31752
]


@pytest.mark.parametrize("d16,lin,lds,tab", DUO_VARIANTS)
def test_duo_score_range_edges(engine, d16, lin, lds, tab):
    """Identical pairs put H, t and the running maximum on the edge itself; the expected score MATCH * length
    needs no oracle.  One past the u16 edge a forced duo refuses and the automatic plan is exact."""
    rng = np.random.default_rng(11)
    s = rand_seq(rng, ACGT, 3527)
    for ma, n, u16, f16 in RANGE_CASES:
        pairs = [(s[:n], s[:n].copy()), (s[:100], s[:100].copy())]
        for t in ((ma, -ma, 0, 0), (ma, -1, 65408 if ma == 127 else 7, 65535 if ma == 127 else 2)):
            assert duo_ok(t, pairs) == u16 and f16_ok(t, pairs) == f16
            p = engine.Params(*t)
            reset(engine)
            duo_force(engine, d16, lin, lds, tab)
            if u16:
                assert engine.score_batch(pairs, p) == [ma * n, ma * 100], (t, n)
                st = engine.last_stats()
                assert duo_ran(t, st, pairs, d16, lin, lds, tab), (t, n, st)
                continue
            with pytest.raises(engine.SwError):
                engine.score_batch(pairs, p)
            reset(engine)
            assert engine.score_batch(pairs, p) == [ma * n, ma * 100], (t, n)
            assert engine.last_stats()["mode"] != 3


# ---- flow2 (mode 5, the compiled kernel: f3 = 0, f3a = 0) -------------------------------------------------

@pytest.mark.parametrize("cols", [1, 2])
@pytest.mark.parametrize("stream", [0, 1])
@pytest.mark.parametrize("single", [True, False])
def test_flow2(engine, oracle_mod, cols, stream, single):
    """One and two columns per lane (two: the linear-gap step only), rows staged in LDS and streamed."""
    def force(t):
        for k, v in (("orient", 1), ("mode", 5), ("W", 1), ("f3", 0), ("f3a", 0), ("f2w", 1 if cols == 1 else 0),
                     ("f2stream", stream)):
            engine.set_option(k, v)

    def ran(t, st, pair):
        return st["mode"] == 5 and bits(st, (16 if cols == 2 else 0) | (8 if linear(t) else 0) | (2 if stream else 0),
                                        64 | 1024 | 32768 | 4 | (16 if cols == 1 else 0) | (0 if stream else 2) |
                                        (0 if linear(t) else 8))

    sweep(engine, oracle_mod, "flow", force, lambda t: flow_ok(t) and (cols == 1 or linear(t)), ran,
          lambda t: not flow_ok(t), N_FLOW if cols == 1 else N_FLOW_LIN, single)


# ---- flow3, staged rows ------------------------------------------------------------------------------------

CUT = 1 << 17


@pytest.mark.parametrize("split", [-1, 1])
def test_flow3_staged_linear(engine, oracle_mod, split):
    """sw_flow3_kernel (two columns per lane, the linear-gap step), uncut and cut at a column (f3split = 1:
    every pair of 379 columns or more)."""
    def force(t):
        for k, v in (("orient", 1), ("mode", 5), ("f3split", split)):
            engine.set_option(k, v)

    def ran(t, st, pair):
        cut = split == 1 and len(pair[0]) >= 379
        return st["mode"] == 5 and bits(st, 64 | 16 | 8 | (CUT if cut else 0), 4 | 2 | 1024 | (0 if cut else CUT))

    sweep(engine, oracle_mod, "flow", force, lambda t: flow_ok(t) and linear(t), ran, lambda t: not flow_ok(t),
          N_FLOW_LIN, True)


def test_flow3_staged_affine(engine, oracle_mod):
    """sw_flow3a_kernel (one column per lane, the general affine step): G_INIT != G_EXT, and G_INIT == G_EXT
    with option linear = 0."""
    def force(t):
        for k, v in (("orient", 1), ("mode", 5), ("linear", 0)):
            engine.set_option(k, v)

    def ran(t, st, pair):
        return st["mode"] == 5 and bits(st, 1024, 64 | 16 | 8 | 4 | 2)

    sweep(engine, oracle_mod, "flow", force, flow_ok, ran, lambda t: not flow_ok(t), N_FLOW, True)


HEP = 1 << 16


@pytest.mark.parametrize("lin", [-1, 0])
def test_flow3_seven_letter(engine, oracle_mod, lin):
    """ACGTN pairs on sw_flow3h_kernel (linear-gap step) and sw_flow3ah_kernel (affine): the automatic plan
    of a single pair over at most seven byte values (stats dna = 2)."""
    def force(t):
        engine.set_option("orient", 1)
        engine.set_option("linear", lin)

    def ran(t, st, pair):
        step = bits(st, 64 | 8, 1024) if lin and linear(t) else bits(st, 1024, 64 | 8)
        return st["mode"] == 5 and st["dna"] == 2 and bits(st, HEP) and step

    sweep(engine, oracle_mod, "hep", force, flow_ok, ran, lambda t: False, N_FLOW, True)


# ---- flow3, ring mode --------------------------------------------------------------------------------------

def w45_plan(n, blocks):
    """plan_w45 (sw_engine.hip): whether n columns run at four / five per lane on `blocks` blocks."""
    g5 = max(0, (n - 1008 * blocks + 251) // 252)
    return g5 <= blocks and n >= 1024


@pytest.mark.parametrize("f2w", [2, 3, 4])
@pytest.mark.parametrize("aff", [0, 1])
@pytest.mark.parametrize("blocks", [1, 3])
def test_flow3_ring(engine, oracle_mod, f2w, aff, blocks):
    """Ring edges (option ring = 1, 512-row rings that the 700 rows wrap) at two, three and four / five
    columns per lane, the linear-gap step (sw_flow3r / r3 / r45_kernel) and the affine one (sw_flow3ra / ra3)."""
    name = "ring45" if f2w == 4 else "ring"

    def force(t):
        for k, v in (("orient", 1), ("mode", 5), ("ring", 1), ("ring_rows", 512), ("blocks", blocks), ("f2w", f2w),
                     ("linear", 0 if aff else -1)):
            engine.set_option(k, v)

    def ran(t, st, pair):
        if aff:   # no affine kernel at four / five columns: three then
            return st["mode"] == 5 and bits(st, 4 | 2 | 1024 | 16 | (0 if f2w == 2 else 8192),
                                            64 | 8 | 16384 | (8192 if f2w == 2 else 0))
        assert f2w != 4 or w45_plan(len(pair[0]), blocks)
        w = {2: 0, 3: 8192, 4: 16384}[f2w]
        return st["mode"] == 5 and bits(st, 4 | 2 | 64 | 8 | 16 | w, 1024 | ((8192 | 16384) & ~w))

    sweep(engine, oracle_mod, name, force, lambda t: flow_ok(t) and (aff or linear(t)), ran, lambda t: not flow_ok(t),
          N_FLOW if aff else N_FLOW_LIN, True)


# ---- a pair per workgroup (mode 5, f2pwg = 1) --------------------------------------------------------------

@pytest.mark.parametrize("f3pwg", [1, 0])
@pytest.mark.parametrize("aff", [0, 1])
def test_pair_per_workgroup(engine, oracle_mod, f3pwg, aff):
    """flow3's three-column ring step with a pair per workgroup (sw_flow3r3p / ra3p_kernel) and flow2's PWG
    kernel (f3pwg = 0), on grids of one and three workgroups."""
    for blocks in (1, 3):
        def force(t):
            for k, v in (("orient", 1), ("mode", 5), ("f2pwg", 1), ("f3pwg", f3pwg), ("blocks", blocks),
                         ("linear", 0 if aff else -1)):
                engine.set_option(k, v)

        def ran(t, st, pair):
            if f3pwg:
                return st["mode"] == 5 and bits(st, 32768 | (1024 if aff else 8), 8 if aff else 1024)
            return st["mode"] == 5 and bits(st, 32 | (0 if aff else 8 | 16), 32768 | 64 | 1024 | (8 | 16 if aff else 0))

        sweep(engine, oracle_mod, "pwg", force, lambda t: flow_ok(t) and (aff or linear(t)), ran,
              lambda t: not flow_ok(t), N_FLOW if aff else N_FLOW_LIN)


# ---- substitution matrices (sw_matrix.hip) -------------------------------------------------------------------

MATRIX_GAPS = [(0, 5), (1, 3), (G20, 0), (0, G20)]   # G_INIT = 0 with G_EXT > 0; G_EXT > G_INIT; the maxima


def matrix_tables():
    from test_matrix_cpu import identity_table
    k = 24
    return {"diag": identity_table(k, 127, -127),          # the entry range's two ends
            "ties": np.full((k, k), 127, np.int32),        # every entry +127: every cell ties, the tie rule decides
            "zero": np.zeros((k, k), np.int32)}            # every entry 0: score 0, no alignment


@pytest.fixture(scope="module")
def matrix_pairs():
    from test_matrix import SYM
    rng = np.random.default_rng(12)
    a6, a10 = rand_seq(rng, SYM[:23], 640), rand_seq(rng, SYM[:23], 1030)
    return [(a6, mutated(rng, SYM[:23], a6, 440, 130, (512, 480))),             # across the strip boundary at 512
            (a10, mutated(rng, SYM[:23], a10, 760, 300, (1024, 900))),          # ... and at 1024
            (rand_seq(rng, SYM[:23], 513), rand_seq(rng, SYM[:23], 200))]


@pytest.mark.parametrize("gaps", MATRIX_GAPS)
@pytest.mark.parametrize("tname", ["diag", "ties", "zero"])
def test_matrix_scores(engine, matrix_pairs, tname, gaps):
    from test_matrix import SYMBOLS, check_many
    T = matrix_tables()[tname]
    want = check_many(matrix_pairs, T, *gaps)
    with engine.Matrix(SYMBOLS, T) as mx:
        assert engine.score_matrix_batch(matrix_pairs, mx, *gaps) == want
        assert engine.last_stats()["mode"] == 6
    if tname == "zero":
        assert want == [0, 0, 0]
    if tname == "ties":
        assert want == [127 * min(len(a), len(b)) for a, b in matrix_pairs]
    if tname == "diag":
        assert min(want) >= 127 and want[1] > 127 * 20


@pytest.mark.parametrize("gaps", MATRIX_GAPS)
@pytest.mark.parametrize("tname", ["diag", "ties", "zero"])
def test_matrix_alignments(engine, matrix_pairs, tname, gaps):
    """The traced kernel and the walk against the CPU aligner, every alignment re-scored (test_align.both).
    G_EXT > G_INIT: a gap run costs min(gap_ext, gap_init) per further residue (algoGPU.h)."""
    from test_align import both
    from test_matrix import check_many
    T = matrix_tables()[tname]
    got = both(engine, matrix_pairs, T, *gaps)
    assert engine.last_stats()["mode"] == 7
    assert [x.score for x in got] == check_many(matrix_pairs, T, *gaps)
    if tname == "zero":
        assert all(x.ops == () for x in got)
    if tname == "ties":     # the end cell: the smallest i + j, so the diagonal from the origin
        assert all(x.ops == ((min(len(a), len(b)), "M"),) and x.beg1 == x.beg2 == 0 for x, (a, b) in zip(got, matrix_pairs))
