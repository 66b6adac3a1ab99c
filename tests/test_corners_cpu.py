"""CPU: the checker at the corners of the scoring-constant domain, before any kernel is compared with it.

tests/golden/params_corners.json (tests/golden/gen_corners.py) holds, for every set of
test_param_corners.CORNERS, the scores of six small pairs from the reference's own main.cpp and
lazySmith.cpp built with that set.  The oracle must reproduce main.cpp's (the recurrence the engine is
defined by) at every set, and LazySmith's wherever G_INIT <= 2 G_EXT: with a cheaper extension LazySmith's
second pass lets a gap turn the corner without a second opening and scores higher, which the fixture
records.  Where oracle/_ref holds the reference builds (the build container) a fresh run equals both.  The
last test checks on the oracle alone that the inputs of tests/test_param_corners.py make the constants matter."""
import pytest

from test_param_corners import CORNERS, G20, LISTS


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("params_corners.json")


def test_fixture_covers_every_corner(fixture):
    assert [tuple(s["params"]) for s in fixture["sets"]] == CORNERS
    assert len(fixture["pairs"]) == 6 and all(len(c["seq1"]) <= 200 and len(c["seq2"]) <= 200 for c in fixture["pairs"])
    assert any("main.cpp" in s and "lazySmith.cpp" in s for s in fixture["pinned_by"]), fixture["pinned_by"]
    kinds = {c["kind"] for c in fixture["pairs"]}
    assert kinds == {"random DNA", "mutated copy with indels", "identical", "protein", "ACGTN", "1 x k"}


@pytest.mark.parametrize("k", range(len(CORNERS)))
def test_oracle_equals_reference_at_corner(oracle_mod, fixture, k):
    s = fixture["sets"][k]
    prm = oracle_mod.Params(*s["params"])
    have_ref = oracle_mod.build_refvar(prm) and oracle_mod.ref_lib(prm) is not None
    # LazySmith computes main.cpp's recurrence exactly when G_INIT <= 2 G_EXT (tests/golden/gen_corners.py)
    if prm.gap_init <= 2 * prm.gap_ext:
        assert s["lazy_scores"] == s["scores"]
    assert all(x >= y for x, y in zip(s["lazy_scores"], s["scores"]))
    for c, want, lazy in zip(fixture["pairs"], s["scores"], s["lazy_scores"]):
        a, b = c["seq1"], c["seq2"]
        assert oracle_mod.score_full(a, b, prm) == want, (prm, c["kind"])
        assert oracle_mod.score_linear(a, b, prm) == want, (prm, c["kind"])
        if have_ref:   # a fresh build of the reference with these constants
            assert oracle_mod.ref_score(a, b, prm, "full") == want, (prm, c["kind"])
            assert oracle_mod.ref_score(a, b, prm, "lazy") == lazy, (prm, c["kind"])


def test_corner_inputs_make_the_constants_matter(oracle_mod):
    """Every identical pair reaches MATCH * min(n, m); every MATCH <= 0 set scores 0 although matching
    residues are present; and gaps are taken: under at least half the sets with cheap gaps every mutated pair
    scores differently than with the same MATCH / MISMATCH at prohibitive gaps."""
    cheap = [t for t in CORNERS if t[0] > 0 and t[2] <= 9 and t[3] <= 9]
    assert len(cheap) >= 10
    for name, (pairs, mut, ident) in LISTS.items():
        for t in CORNERS:
            exp = [oracle_mod.score_linear(a, b, oracle_mod.Params(*t)) for a, b in pairs]
            for k in ident:
                a, b = pairs[k]
                assert (a == b).all() and exp[k] == max(t[0], 0) * len(a), (name, t, k)
            if t[0] <= 0:
                assert exp == [0] * len(pairs) and any((a[:, None] == b[None, :]).any() for a, b in pairs), (name, t)
        for k in mut:
            a, b = pairs[k]
            differ = 0
            for t in cheap:
                stiff = oracle_mod.Params(t[0], t[1], G20, G20)
                differ += oracle_mod.score_linear(a, b, oracle_mod.Params(*t)) != oracle_mod.score_linear(a, b, stiff)
            assert 2 * differ >= len(cheap), (name, k, differ, len(cheap))
