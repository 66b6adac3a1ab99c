"""CPU: what the steep plan's frame says about dead strips (sw_internal.h steep_bounds, restated by
tests/test_steep_identity.py steep_plan).  The forward chain has no lead: its dead columns are the last ones, in its
shortest strips.  The mirrored chain starts behind W - 2 - n dead columns: up to three wholly dead strips and one
partly dead, never a whole group, so every workgroup of a chain has a live strip."""
from test_steep_identity import steep_plan

AUTO = (64, 128, 64, 128)


def dead_strips(lead):
    """(wholly dead strips, dead columns of the next strip) in front of the mirrored chain: strip s holds the
    frame's columns 126 s .. 126 s + 127, of which 126 s + 126 and + 127 are the next strip's first two"""
    return lead // 126, lead % 126


def test_no_plan_has_a_dead_group():
    worst = 0
    for n in range(253, 70000, 1):
        p = steep_plan(n, 1 << 22, AUTO)
        if p is None:   # (the frame's 126 S columns hold no n = 504 k + 1 or + 2)
            assert n % 504 in (1, 2), n
            continue
        S, lead = p[0], p[1]
        assert S % 4 == 0 and 0 <= lead < 504, (n, S, lead)
        worst = max(worst, lead)
    assert worst == 501 and dead_strips(worst) == (3, 123)


def test_c2_frame():
    S, lead, rlead, e0f, e0b, cum = steep_plan(65536, 65536, (128, 64, 128, 128))
    assert (S, lead) == (524, 488) and dead_strips(lead) == (3, 110)
    # both chains' strip 0 run the same steps at C2 (within 128 of each other anywhere), and the forward one's
    # columns are all live: skipping the mirrored chain's dead strips cannot shorten the launch
    assert 0 <= e0b - e0f < 128 and e0f == e0b == 62080
