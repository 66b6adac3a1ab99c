"""CPU: the leaner half-chunk links of the staged flow3 loops (tools/gen_flow3.py LINK_*).

The generated file is in sync; the C = 32 half-chunk-link roles with a link carry fewer VALU + SALU + DS a chunk
than the parent's census (profiles/r04_flow3_census.txt, lines 32,1,*); the ring-mode, affine and pool files are
what their generators write; and the ring arithmetic holds: with the ring offset advanced once a loop body the odd
chunk's windows start 32 rows behind the even chunk's, and every window start the loops can form keeps every
lane's read and both copies of every write inside the ring's allocation, reads every row where its publish put
it, and lets no write-ahead lane touch a row that is published and not yet consumed."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "concurrentproject_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))

import flow3_census  # noqa: E402
import gen_flow3  # noqa: E402

R, C, H = 512, 32, 16


def test_generator_check_passes():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_flow3.py"), "--check"])
    assert r.returncode == 0, "run: python tools/gen_flow3.py"


def _parent_census():
    """role -> VALU beyond the body + SALU + DS per chunk, from the parent's census file"""
    out = {}
    for line in open(os.path.join(ROOT, "profiles", "r04_flow3_census.txt")):
        w = line.split()
        if len(w) == 9 and w[0] == "sw_flow3_loops.inc" and w[1].startswith("32,1,"):
            out[w[1]] = float(w[3]) + float(w[4]) + float(w[7])
    return out


def test_census_below_the_parent():
    parent = _parent_census()
    assert len(parent) == 6
    rows = {sig: flow3_census.census(sig, body)["per_chunk"]
            for sig, body in flow3_census.blocks(os.path.join(CSRC, "sw_flow3_loops.inc"))}
    assert len(rows) == 18
    linked = [sig for sig in parent if "F3_LDS" in sig]
    assert len(linked) == 4
    for sig in linked:
        p = rows[sig]
        now = p["extra_valu"] + p["salu"] + p["ds"]
        print(sig, "parent", parent[sig], "now", now, "s_nop", p["s_nop"], "waits", p["waitcnt"])
        assert now < parent[sig], (sig, now, parent[sig])
    # the roles without a link are what they were
    for sig in set(parent) - set(linked):
        p = rows[sig]
        assert p["extra_valu"] + p["salu"] + p["ds"] == parent[sig], sig


def test_other_generated_files_unchanged():
    """The ring-mode, affine and pool loops come out of their generators as committed."""
    for path, emit in ((gen_flow3.OUT_RING, gen_flow3.emit_ring), (gen_flow3.OUT_RING3, gen_flow3.emit_ring3),
                       (gen_flow3.OUT_RING45, gen_flow3.emit_ring45), (gen_flow3.OUT_AFF, gen_flow3.emit_aff),
                       (gen_flow3.OUT_RING_AFF, gen_flow3.emit_ring_aff), (gen_flow3.OUT_POOL, gen_flow3.emit_pool)):
        assert open(path).read() == emit(), os.path.basename(path)


def _f3_rs():
    src = open(os.path.join(CSRC, "sw_flow3.hip")).read()
    r = int(re.search(r"constexpr int F3_R = (\d+);", src).group(1))
    m = re.search(r"constexpr int F3_RS = 2 \* F3_R \+ (\d+);", src)
    assert r == R and m, "the ring's size is no longer 2 R + slack: restate this test"
    return 2 * r + int(m.group(1))


def _slot0():
    inc = open(os.path.join(CSRC, "sw_flow3_loops.inc")).read()
    s = int(re.search(r"constexpr int F3_HL_SLOT0 = (\d+);", inc).group(1))
    assert s == gen_flow3.hl_slot0()
    return s


def _reads(k0):
    """slot -> row of the chunk at k0: lanes 0..31 at the top, lanes 0..15 16 rows on at mid-chunk"""
    b = gen_flow3.hl_base(k0)
    top = {b + 64 + C + (lane & (C - 1)): k0 + (lane & (C - 1)) for lane in range(64)}
    mid = {b + 64 + C + H + (lane & (C - 1)): k0 + H + (lane & (C - 1)) for lane in range(64)}
    return top, mid


def _writes(k0):
    """(slot, row or None for a write-ahead lane) of the chunk top's and the mid-chunk publish, one copy"""
    b = gen_flow3.hl_base(k0)
    top = [(b + ((lane + C) & 63), k0 - 64 - C + (lane - 32) if lane >= 32 else None) for lane in range(64)]
    mid = [(b + ((lane + C) & 63) + H + (32 if 32 <= lane < 48 else 0), k0 - 64 + (lane - 48) if lane >= 48 else None)
           for lane in range(64)]
    return top, mid


def test_window_starts():
    """Every multiple of 32 below R is a window start, the odd chunk's through its offset (LINK_ADV: the even
    chunk's register value is a multiple of 64 and the odd chunk adds 32 rows without a wrap)."""
    starts = {gen_flow3.hl_base(k0) for k0 in range(0, 4 * R, C)}
    assert starts == set(range(0, R, C))
    if gen_flow3.LINK_ADV:
        assert {gen_flow3.hl_base(k0) for k0 in range(0, 4 * R, 2 * C)} == set(range(0, R, 2 * C))
        assert all(gen_flow3.hl_base(k0 + C) == gen_flow3.hl_base(k0) + C for k0 in range(0, 4 * R, 2 * C))


def test_windows_stay_inside_the_ring():
    rs, slot0 = _f3_rs(), _slot0()
    lo, hi = rs, 0
    for k0 in range(0, 4 * R, C):
        top, mid = _reads(k0)
        for slot in list(top) + list(mid):
            assert 0 <= slot < 2 * R, (k0, slot)           # a read never takes the slack
        for part in _writes(k0):
            for slot, _ in part:
                assert 0 <= slot and slot + R < rs, (k0, slot, rs)
                lo, hi = min(lo, slot), max(hi, slot + R)
    print("slot0", slot0, "writes span", lo, hi, "of", rs)


def test_rows_are_read_where_they_were_written():
    """Row r lives at slot (r + slot0) mod R; a publish writes slot s' and s' + R with s' = that slot or R more,
    and the consumer's lane must find the row in one of the two."""
    slot0 = _slot0()
    where = {}
    for k0 in range(0, 6 * R, C):
        for part in _writes(k0):
            for slot, row in part:
                if row is not None and row >= 0:
                    assert slot % R == (row + slot0) % R, (k0, slot, row)
                    where.setdefault(row, set()).update((slot, slot + R))
    checked = 0
    for k0 in range(0, 4 * R, C):
        for part in _reads(k0):
            for slot, row in part.items():
                assert slot in where[row], (k0, slot, row, sorted(where[row]))
                checked += 1
    assert checked == (4 * R // C) * (C + C)


def test_write_ahead_lanes_touch_no_live_row():
    """The lanes that hold no outflow write onto slots of rows not yet published, or of rows the back-pressure
    floor says are consumed: the even chunk's check admits its own and the odd chunk's publishes once the
    consumer's word has reached k0 + 16, that is rows < k0 + 16 - R taken (a word written every second chunk
    is older, never larger).  Live rows at a publish: from that floor up to the rows already available."""
    slot0 = _slot0()
    for k0 in range(2 * R, 5 * R, C):
        k0e = k0 - C * ((k0 // C) & 1)
        floor = k0e + H - R
        top, mid = _writes(k0)
        for part, avail in ((top, k0 - 64), (mid, k0 - 64 + H)):
            live = {(r + slot0) % R for r in range(floor, avail)}   # (this publish's own rows among them)
            for slot, row in part:
                if row is None:
                    assert slot % R not in live, (k0, slot, floor, avail)
