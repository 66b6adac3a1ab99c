// sw_internal.h -- structures shared by the gfx950 kernels (sw_kernels.hip) and
// the C++ host layer (sw_engine.hip).  Not part of the public C-ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

namespace swmi {

// One pair after orientation: the "column" sequence (length n) runs across the
// lanes of a wave, the "row" sequence (length m) streams through it.  The score
// is symmetric in (seq1, seq2), so the host picks the orientation.
struct PairDesc {
    uint64_t col_off;   // byte offset of the column sequence in the sequence arena
    uint64_t row_off;   // byte offset of the row sequence
    uint64_t bnd_off;   // granule offset of this pair's strip-boundary buffers
    int n;              // columns (> 0)
    int m;              // rows    (> 0)
    int strips;         // ceil(n / (64*W))
    int out_idx;        // slot in the score array
    // One half of a pair cut at a column (sw_engine.hip plan_split; flow3's staged linear-gap
    // kernel only, 0 elsewhere).  PAIR_HALF: the last strip publishes its outflow as granules
    // into edge (strips + 3) / 4 - 1 for the combine kernel.  PAIR_REV: columns and rows are
    // read mirrored (column j is byte col_off + n - 1 - j, row r byte row_off + m - 1 - r).
    // PAIR_WEDGE: one chain of a pair cut along an anti-diagonal staircase (plan_wedge; KParams::wedge_*):
    // strip s runs wedge_e0 - 64 s steps and every strip writes its lanes' last two rows of H into the
    // chain's boundary buffer for the wedge combine kernel.
    int flags;
    int lead;           // dead columns in front of column 0 (strip s, lane l: column 126 s + 2 l - lead)
};
enum : int { PAIR_HALF = 1, PAIR_REV = 2, PAIR_WEDGE = 4 };

// Two pairs scored in lock step by the packed-u16 "duo" kernel: lane values
// hold pair 0 in the low and pair 1 in the high 16 bits.  Both are padded to
// (n_pad, m_pad) with dead columns / sentinel rows.
struct DuoDesc {
    uint64_t col_off[2];
    uint64_t row_off[2];
    uint64_t bnd_off;   // granule offset of the duo's strip-boundary buffers (m_pad rows each)
    int n[2], m[2];
    int n_pad, m_pad;
    int strips;         // ceil(n_pad / (64*W))
    int out_idx[2];     // out_idx[1] == -1: no second pair
};

// Per-launch control block: next_item is zeroed by hipMemsetAsync before every launch, except a two-wedge launch
// that joins its chains itself, which counts on from KParams::item0.
struct Ctrl {
    unsigned int next_item;   // work-claim counter (items claimed strictly in order)
    unsigned int error;       // nonzero: a bounded spin gave up (see ERR_*)
    unsigned int err_item;
    unsigned int pad;
};

enum : unsigned { ERR_TIMEOUT = 1u, ERR_EDGE = 2u };   // EDGE: a cut pair's final edge held an unwritten row

// A strip boundary hand-off granule: written ONCE per launch with a single
// 16-byte write-through (sc1) store by the producer wave, read with sc1 loads
// by the consumer wave.  `tag` carries the launch epoch, `chk` detects a torn
// or stale read.  (MI355X_MICROARCH.md, Workgroup dispatch ... R2 granules.)
struct alignas(16) Granule {
    unsigned int tag;
    int hg;      // H - G_INIT of the strip's last column at this row
    int eh;      // E - G_EXT  of the strip's last column at this row
    unsigned int chk;
};

// Torn-read guard of a 16-B granule {tag, hg, eh, chk}: injective in each of
// tag, hg and eh for fixed others, so a granule mixing dwords of two writes
// (different epoch, or a stale value) fails the check.  Multiply-free: XORs
// and one rotate (v_xor3 / v_alignbit), on the consumer's critical path.
__host__ __device__ inline unsigned granule_chk(unsigned tag, int hg, int eh, int row) {
    const unsigned e = (unsigned)eh;
    return tag ^ (unsigned)hg ^ ((e << 13) | (e >> 19)) ^ ((unsigned)row << 7) ^ 0x5BD1E995u;
}

struct KParams {
    const unsigned char* seq;     // sequence arena (raw bytes)
    const PairDesc* pairs;
    const int* item_base;         // npairs+1 prefix sums of strips
    Granule* bnd;                 // strip-boundary granule arena
    Ctrl* ctrl;
    int* scores;
    int npairs;
    int total_items;
    unsigned epoch;               // != 0, unique per launch
    int match, mismatch, gap_init, gap_ext;
    unsigned prof[4];             // DNA mode: per column code, 4 biased score bytes (row code 0..3)
    unsigned prof2[4];            // flow2 mode: per column code, 4 signed score bytes s + G_INIT (row code 0..3)
    unsigned prof3[4];            // flow2 W2: per column code, 4 signed score bytes s (row code 0..3)
    unsigned pen[4];              // duo mode: per column code, 4 penalty bytes MATCH - s (row code 0..3)
    // a pair over an alphabet of up to seven byte values (flow3 staged, LaunchCfg::hep): the symbol
    // 0..6 of each byte value, and per column symbol the perm's high word (row symbols 0..3) and low
    // word (byte 0: the no-row 0x80; bytes 1..3: row symbols 4..6), as signed bytes s + G_INIT (hp2,
    // hq2) and s (hp3, hq3)
    unsigned char hsym[256];
    unsigned hp2[7], hq2[7], hp3[7], hq3[7];
    const unsigned char* hrows;   // ring mode (sw_flow3r3h / ra3h_kernel): the pair's rows as perm selectors
    const DuoDesc* duos;          // duo mode: nduos descriptors (npairs counts duos)
    long long timeout_ticks;      // s_memrealtime ticks (100 MHz) before a spin gives up
    unsigned long long* trace;    // optional (tools/trace_flow.py): per-strip timestamps, else null; a wedge launch
                                  // (tools/trace_wedge.py): 16 words at row chain * S + strip, sw_flow3.hip
    // Column slab of a pair split across GPUs (grouped modes, one pair per launch):
    // the first group's inflow comes from slab_in (the previous slab's last
    // column, written by the previous GPU over xGMI), the last group's outflow
    // goes to slab_out (the next GPU's slab_in, mapped here by IPC).  Both use
    // slab_epoch, agreed by all ranks; null = an ordinary pair edge.
    Granule* slab_in;
    Granule* slab_out;
    unsigned slab_epoch;
    // flow2 ring mode (one pair; sw_flow2.hip): 0 = linear edges (one m-row
    // granule buffer per group boundary, written once).  Else block j of the
    // G-block grid runs groups j, j+G, j+2G, ...; boundary k*G+j streams through
    // ring j (ring_rows rows, j < G-1) or the wrap ring (wrap_rows >= m rows,
    // j = G-1), so the boundary state is O(G*ring_rows + m), not O(groups*m).
    int ring_rows;
    int wrap_rows;
    unsigned* ring_cons;          // ring j's consumer progress (positions consumed), RING_CONS_STRIDE apart;
                                  // duo LDS kernel: DUO_CU_WORDS zeroed role words (or null)
    int duo_prio;                 // duo LDS kernel with roles: 0 = off, k in 6..20 = the CU's two workgroups
                                  // take turns at issue priority every 2^k ticks of s_memrealtime (s_setprio)
    int w45_s4;                   // flow3 ring at four / five columns per lane (sw_flow3r45_kernel): strips below
                                  // this index have 252 new columns, the rest 315 (a multiple of 4); -1 otherwise
    int stall_item;               // tests only (option stall_item): flow2's compute waves skip this item, so its
                                  // edges are never published and its consumers' bounded waits must expire; -1 = none
    // (the duo kernel with LDS hand-offs takes its wrap-buffer slots from wrap_rows)
    // One pair as two wedges (sw_engine.hip plan_wedge; flow3's staged linear-gap kernel): pair 0 is the
    // forward chain, pair 1 the mirrored one; item i is group i / 2 of pair i % 2.  Chain p's strip s runs
    // wedge_e0[p] - 64 s steps (multiples of 64); the mirrored chain has wedge_rlead dead rows in front of its
    // row 0; a chain's group edges are wedge_rows rows apart, and its boundary buffer (two 16-B entries
    // per strip and lane) starts wedge_bnd[p] granules into the arena.
    // The drop behind strip j (strip j + 1 ends that many steps before strip j) is wedge_drop[j % 4], 64 each in
    // the uniform plan.  A steep plan (steep_bounds; wedge_segr > 0) joins the chains along every strip's hand-off
    // column too: each strip but the last stores the outflow row no publish sends (row end - 64) as an 8-B
    // granule {H - G, key} at entry strip * wedge_segr of its chain's segment buffer, wedge_seg[p] granules into
    // the arena, and a producer on an in-workgroup link the drop - 63 rows above it (end - drop - 1 .. end - 65)
    // behind that.
    int wedge;                    // 0: no wedge launch
    int wedge_e0[2];
    int wedge_rlead;
    int wedge_rows;
    unsigned long long wedge_bnd[2];
    int wedge_drop[4];
    int wedge_segr;
    unsigned long long wedge_seg[2];
    // A wedge launch that joins its chains itself (sw_flow3.hip the join; environment SWMI_F3JOIN, default on): the
    // launch is this one kernel, with no copy, memset or combine kernel beside it.  wedge_join points at the
    // context's join words (JOIN_*; zero between launches): a counter per join unit, the 64-bit score word and
    // the counter of finished strips.  The two descriptors travel here (wedge_pair: item & 1 selects), and the
    // claim counter is not reset: a launch's workgroups make total_items + blocks claims, the host keeps the
    // sum, and item = claim - item0.
    unsigned* wedge_join;         // null: the copies, the memsets and the combine kernel of a launch without the join
    unsigned item0;
    PairDesc wedge_pair[2];
};
// the join words of a context: the score word (64 bits: epoch << 32 | score, atomicMax), the finished strips, and
// from JOIN_UNITS on a counter per join unit (forward strip)
enum : int { JOIN_SCORE = 0, JOIN_DONE = 2, JOIN_UNITS = 4 };
// Join unit s is what the combine kernels compute for forward strip s: its lanes' diagonal nodes against the mirrored
// lanes they meet and, in a steep plan, its hand-off column against the mirrored chain's.  It reads forward strip s
// and the mirrored strips S - s - 2 .. S - s - lo inside [0, S), lo = 1 in a steep plan (whose mirrored chain sits
// two dead columns further left) and 0 in the uniform one (tools/wedge_bounds_check.cpp checks both against the
// combine kernels' index sets).  A strip adds one to every unit that reads it; the add that brings a unit to
// join_unit_full runs it.
__host__ __device__ inline int join_unit_lo(int S, int s, bool steep) { return S - s - 2 < 0 ? 0 : S - s - 2; }
__host__ __device__ inline int join_unit_hi(int S, int s, bool steep) {
    const int hi = S - s - (steep ? 1 : 0);
    return hi > S - 1 ? S - 1 : hi;
}
__host__ __device__ inline int join_unit_full(int S, int s, bool steep) {
    return 1 + join_unit_hi(S, s, steep) - join_unit_lo(S, s, steep) + 1;
}

constexpr int RING_CONS_STRIDE = 32;   // dwords between consumer progress words (one 128-B line each)

// Grid organisations (sw_kernels.hip):
//   MODE_STRIP  independent waves claim (pair, strip) items in order
//   MODE_PAIRWG one workgroup per pair, its 4 waves interleave the strips
//   MODE_CHAIN  one workgroup per group of 4 consecutive strips, LDS hand-offs
//   MODE_DUO    one workgroup per two pairs, packed u16 (DNA, small scores)
//   MODE_FLOW   as MODE_CHAIN, free-running waves with LDS progress words
//   MODE_FLOW2  W=1 DNA single pairs: overlapping 64-column strips, DPP-add
//               hand-offs, 11 instructions per step (sw_flow2.hip)
enum : int { MODE_STRIP = 0, MODE_PAIRWG = 1, MODE_CHAIN = 2, MODE_DUO = 3, MODE_FLOW = 4, MODE_FLOW2 = 5 };
inline bool grouped_mode(int mode) { return mode == MODE_CHAIN || mode == MODE_FLOW || mode == MODE_FLOW2; }

#ifndef SW_DUO_WAVES
#define SW_DUO_WAVES 4
#endif
constexpr int DUO_WAVES = SW_DUO_WAVES;   // waves per workgroup of the duo kernel (one workgroup per duo)

// Host-side launch (sw_kernels.hip).  sw_engine.hip select_variant fills it; f2_wgs and blocks after the rest (size_grid).
struct LaunchCfg {
    int W;          // columns per lane
    int C;          // rows per hand-off chunk
    bool dna;       // 2-bit ACGT profile path (else raw-byte compare)
    int blocks;     // persistent workgroups (256 threads = 4 waves)
    int mode;       // MODE_*
    int max_m;      // longest row sequence (MODE_FLOW stages it in LDS)
    bool duo_f16 = false;   // MODE_DUO: max3 through v_pk_maximum3_f16 (every value < 0x7C00)
    bool f2_stream = false; // MODE_FLOW2: row codes streamed through per-wave LDS rings (rows too long to stage)
    int f2_wgs = 1;         // MODE_FLOW2 streamed: workgroups per CU (LDS pad sized to admit exactly this many)
    bool f2_lin = false;    // G_INIT == G_EXT, the exact linear-gap step: MODE_FLOW2 at C = 32 or 64 (sw_flow2.hip
                            // LIN) and MODE_DUO with duo_f16 (sw_kernels.hip StripDuo LIN)
    bool f2_w2 = false;     // MODE_FLOW2 with f2_lin: two columns per lane (126 new columns per strip)
    bool f2_pwg = false;    // MODE_FLOW2 batch: a pair per workgroup, all hand-offs in LDS (C = 64, streamed)
    bool f3 = false;        // MODE_FLOW2 staged two-column linear-gap launch on the flow3 kernel (sw_flow3.hip)
    bool f3_hl = false;     // flow3 staged at C = 32: in-workgroup links hand off every half chunk
    bool f3a = false;       // MODE_FLOW2 staged one-column launch with the affine step on flow3 (sw_flow3a_kernel)
    bool f3p = false;       // flow3 staged on the pool loops (sw_flow3p_kernel: C = 32, f3_hl, no I/O rotation)
    bool hep = false;       // flow3 staged launch of a pair over up to seven byte values (sw_flow3h / ah_kernel, KParams::hsym)
    bool f3_w3 = false;     // flow3 ring mode at three columns per lane (sw_flow3r3_kernel / sw_flow3r3s_kernel)
    bool f3_w45 = false;    // flow3 ring mode at four and five columns per lane (sw_flow3r45_kernel, KParams::w45_s4)
    bool f3_pwg = false;    // flow3 three-column ring step, a pair per workgroup (sw_flow3r3p_kernel; int32 batches)
    bool f3ra = false;      // MODE_FLOW2 ring-mode two-column launch with the affine step on flow3 (sw_flow3ra_kernel)
    bool f3_slab = false;   // flow3 ring launch of a column slab (sw_flow3rs_kernel / sw_flow3ras_kernel)
    int duo_wrap = 0;       // MODE_DUO at C = 64: > 0 = strip hand-offs in LDS (sw_duo_lds_kernel), this many
                            // wrap-buffer slots (a power of two >= every m_pad); 0 = HBM granules
    int duo_tab = 0;        // with duo_wrap, W % 4 == 0: > 0 = row codes from an LDS table of this many words
};
// the duo LDS kernel's wrap buffer: slots for rows of m_pad up to m, and its dynamic LDS
inline int duo_wrap_slots(int m) {
    int w = 64;
    while (w < m) w *= 2;
    return w;
}
// the duo LDS kernel's row-code table (sw_kernels.hip StripDuoT): rows -DUO_TAB_OFF .. m_pad + DUO_TAB_TAIL
constexpr int DUO_TAB_OFF = 528;     // rows below row 0: lane 63's W = 8 positions and a read group ahead
constexpr int DUO_TAB_TAIL = 768;    // rows past m_pad: the last chunk's steps, the build's two chunks ahead
// the duo LDS kernel's dynamic LDS: the wrap buffer, then the code table (words, 16-B rounded)
inline int duo_lds_dyn(const LaunchCfg& cfg) {
    return cfg.duo_wrap * (cfg.f2_lin ? 4 : 8) + ((cfg.duo_tab * 4 + 15) & ~15);
}
constexpr int DUO_LDS_DYN_MAX = 72 * 1024;   // attribute limit of the duo LDS kernel's dynamic LDS
constexpr int DUO_CU_WORDS = 8 * 256;         // duo strip roles: a word per (XCC, SE, SH, CU) of HW_ID
// the most dynamic LDS that still admits two workgroups per CU beside the static LDS (rings, sinks:
// ~5 KB at the linear-gap step's 4-B slots, ~9 KB affine)
inline int duo_lds_fit(bool lin) { return lin ? 72 * 1024 : 68 * 1024; }
constexpr int F2_WGS_MAX = 4;   // flow2 streamed kernel: most workgroups per CU (launch_c sizes the LDS pad)

// MODE_FLOW stages a pair's row codes in LDS: one byte per row plus the
// prefetch tail; pairs whose rows do not fit use MODE_CHAIN.
constexpr int LDS_PER_CU = 160 * 1024;
__host__ __device__ constexpr int flow_stage_rows(int m, int W, int C) { return ((m + 64 * W + 2 * C + 64) + 15) & ~15; }
__host__ __device__ constexpr int flow_ring_rows(int W, int C) {
    int r = 256;
    while (r < 2 * 64 * W + 4 * C) r *= 2;
    return r;
}
// static LDS of sw_flow_kernel<W,C> (rings + sinks + words), rounded up
__host__ __device__ constexpr int flow_static_lds(int W, int C) { return 3 * flow_ring_rows(W, C) * 8 + 4096; }
__host__ __device__ constexpr int flow_stage_max(int W, int C) { return LDS_PER_CU - flow_static_lds(W, C); }

// MODE_FLOW2 (sw_flow2.hip): strip s covers columns [63s, 63s + 64); the row
// codes of the pair are staged in LDS (one byte per row, 64 rows of border in
// front, a chunk of prefetch behind).
__host__ __device__ constexpr int flow2_strips(int n) { return n <= 64 ? 1 : (n - 1 + 62) / 63; }
// two columns per lane (LaunchCfg::f2_w2): strip s covers columns [126s, 126s + 128)
__host__ __device__ constexpr int flow2_strips_w2(int n) { return n <= 128 ? 1 : (n - 2 + 125) / 126; }
// three columns per lane (flow3 ring mode): strips of 189 new columns overlapping by three
__host__ __device__ constexpr int flow2_strips_w3(int n) { return n <= 192 ? 1 : (n - 3 + 188) / 189; }
__host__ __device__ constexpr int flow2_stage_bytes(int m, int C) {
    return (64 + ((m + 64 + C - 1) / C + 1) * C + 8 + 15) & ~15;
}
// (rings: 4, or 5 with the staged kernel's loader wave, whose static LDS bounds the staged rows)
__host__ __device__ constexpr int flow2_static_lds(int C, int rings = 5) { return rings * (256 * 8 + 64 * 8 + 64 * 4) + 64 + 0 * C; }
__host__ __device__ constexpr int flow2_stage_max(int C) { return LDS_PER_CU - flow2_static_lds(C) - 256; }
// the most dynamic LDS a streamed flow2 launch may take (sw_flow2.hip flow2_dyn_lds): the staged
// limit less the 4 per-wave code rings (F2_CR = 256 rows + a chunk + 64 sinks each)
__host__ __device__ constexpr int flow2_stream_dyn_max(int C) { return flow2_stage_max(C) - 4 * (256 + C + 64); }
// flow2 pair per workgroup (LaunchCfg::f2_pwg): the wave 3 -> wave 0 buffer holds a round's
// rows (int2 each) in the dynamic LDS; workgroups per CU that fit beside the static LDS
// (4 rings) and the 4 streamed code rings
// (4 B per row at the linear-gap step, whose edges carry H - G twice)
__host__ __device__ constexpr int flow2_pwg_rows(int m, int C) { return (m + 64 + C - 1) / C * C; }
__host__ __device__ constexpr int flow2_pwg_row_bytes(bool lin) { return lin ? 4 : 8; }
__host__ __device__ constexpr int flow2_pwg_wgs(int m, int C, bool lin) {
    return LDS_PER_CU /
           (flow2_pwg_row_bytes(lin) * flow2_pwg_rows(m, C) + flow2_static_lds(C, 4) + 4 * (256 + C + 64) + 1024);
}
// sets the calling thread's sw_last_error() text (sw_engine.hip)
void report_error(const char* msg);
// hipFuncSetAttribute(fn, MaxDynamicSharedMemorySize, bytes) once per (kernel, device) (sw_engine.hip)
hipError_t raise_dyn_lds(const void* fn, int bytes);

hipError_t launch_sw_flow2(const LaunchCfg& cfg, const KParams& kp, hipStream_t stream);
// flow3 (sw_flow3.hip): flow2's staged W2 linear-gap kernel with hand-scheduled chunk loops
hipError_t launch_sw_flow3(const LaunchCfg& cfg, const KParams& kp, hipStream_t stream);
bool flow3_fits(int max_m, int C, bool aff = false);
// the crossing term of a pair cut at a column (sw_flow3.hip): max over rows r of gl[r] + gr[m - 2 - r] + 2 G
// from the two halves' final edges (8-B granules keyed with the launch epoch), atomicMax into *score
hipError_t launch_sw_flow3_combine(const Granule* gl, const Granule* gr, int m, int gap, unsigned epoch, Ctrl* ctrl,
                                   int* score, hipStream_t stream);
// One pair as two wedges (sw_engine.hip plan_wedge): strips per chain, dead columns and rows in front of the
// mirrored chain, and the steps of each chain's strip 0.  False where a strip would keep less than 64 rows.
// A steep plan (steep_bounds) also has drops above 64.
struct WedgePlan {
    int strips, lead, rlead, e0[2];
    int drop[4] = {64, 64, 64, 64};
    bool steep = false;
};
// Both chains run S = ceil((n - 2) / 126) strips over 126 S + 2 padded columns, so the mirrored chain's strip
// S - 1 - s lies on the forward chain's strip s (lane 63 - l on lane l).  With T = m + rlead - 2 + 64 S a
// multiple of 64 and e0[0] + e0[1] = T, the two rows a forward lane exports are the two its mirror lane
// exports (tests/test_wedge_identity.py proves the join and that the shared nodes cover every crossing path).
inline bool wedge_bounds(int n, int m, WedgePlan* w) {
    if (n < 253 || m < 1) return false;
    const long long S = ((long long)n - 2 + 125) / 126;
    if ((long long)m < 64 * S + 64) return false;
    const long long rlead = ((2 - (long long)m) % 64 + 64) % 64;
    const long long T = (long long)m + rlead - 2 + 64 * S;
    w->strips = (int)S;
    w->lead = (int)(126 * S + 2 - n);
    w->rlead = (int)rlead;
    w->e0[0] = (int)(64 * (T / 128));
    w->e0[1] = (int)(T - w->e0[0]);
    return true;
}
// The steep plan: the drop behind strip j is d[j % 4], multiples of 64 from 64 to WEDGE_DROP_MAX with
// d[0] == d[2], so that the mirrored chain, whose drops are the forward chain's read from the far end, has the
// same pattern once S is a multiple of 4.  Both chains run S = roundup4(ceil((n - 2) / 126)) strips over
// W = 126 S + 2 padded columns, the mirrored chain behind W - 2 - n dead columns (two fewer than the uniform
// plan's, n <= 126 S).  A strip hands its lane 62's column B to the strip on its right (whose lane 0 repeats lane
// 63's columns), and those two dead columns less put the hand-off column of forward strip s and that of the
// mirrored strip S - 2 - s onto one node column, 126 s + 126.  The staircase runs down that column from the
// node of the right strip's lane 0 to those of the left strip's lane 62, drop - 60 nodes, and the join takes H
// of both chains along it from the rows handed off (published up to row end - 65), the one row still in the
// I/O register (end - 64) and lane 62's own two.  With D the sum of the S - 1 drops, rlead = (3 - m) mod 64 and
// e0[0] + e0[1] = m + rlead + 61 + D the rows line up lane to lane (tests/test_steep_identity.py).  False where
// W has no room or the last strip would keep less than 64 rows (m < D + 65).
constexpr int WEDGE_DROP_MAX = 256;   // a producer runs drop - 64 rows past its consumer's last: well inside the LDS ring
inline bool wedge_drops_ok(const int d[4]) {
    for (int j = 0; j < 4; ++j)
        if (d[j] < 64 || d[j] > WEDGE_DROP_MAX || d[j] % 64 != 0) return false;
    return d[0] == d[2];
}
inline long long steep_cum(const int d[4], long long s) {   // the drops behind strips 0 .. s - 1
    long long c = (s >> 2) * ((long long)d[0] + d[1] + d[2] + d[3]);
    for (int j = 0; j < (int)(s & 3); ++j) c += d[j];
    return c;
}
inline bool steep_bounds(int n, int m, const int d[4], WedgePlan* w) {
    if (n < 253 || m < 1 || !wedge_drops_ok(d)) return false;
    const long long S = (((long long)n - 2 + 125) / 126 + 3) / 4 * 4;
    if ((long long)n + 2 > 126 * S + 2) return false;
    const long long D = steep_cum(d, S - 1);
    const long long rlead = ((3 - (long long)m) % 64 + 64) % 64;
    const long long T = (long long)m + rlead + 61 + D;
    const long long e0f = 64 * (T / 128), e0b = T - e0f;
    if (std::min(e0f, e0b) - D < 64 || e0f > (long long)m - 1 || e0b > (long long)m + rlead - 1) return false;
    w->strips = (int)S;
    w->lead = (int)(126 * S - n);
    w->rlead = (int)rlead;
    w->e0[0] = (int)e0f;
    w->e0[1] = (int)e0b;
    for (int j = 0; j < 4; ++j) w->drop[j] = d[j];
    w->steep = true;
    return true;
}
// the crossing term of a wedge launch (sw_flow3.hip): max of H_F + H_B over the staircase's shared nodes from
// the two chains' boundary buffers (entries keyed with the launch epoch), atomicMax into *score
hipError_t launch_sw_flow3_wedge_combine(const Granule* bf, const Granule* bb, const WedgePlan& w, int m, unsigned epoch,
                                         Ctrl* ctrl, int* score, hipStream_t stream);
// ... of a steep plan: the diagonal part re-indexed, and the hand-off columns from the chains' group edges
// (ef, eb: edge b at b * edge_rows granules) and segment buffers (sf, sb: strip s at s * segr 8-B entries)
struct SteepJoin {
    const Granule *bf, *bb, *ef, *eb, *sf, *sb;
    int edge_rows, segr, m, gap;
};
hipError_t launch_sw_flow3_steep_combine(const SteepJoin& j, const WedgePlan& w, unsigned epoch, Ctrl* ctrl, int* score,
                                         hipStream_t stream);
// workgroups per CU resident for a flow3 ring-mode launch (its LDS pad of cfg.f2_wgs), -1 on error
int flow3_ring_resident(const LaunchCfg& cfg);
int flow2_waves_per_cu(int C);
// workgroups per CU resident for the streamed flow2 kernel cfg selects (ring / slab
// instantiation, LDS pad of cfg.f2_wgs); -1 on error (sw_flow2.hip)
int flow2_stream_resident(const LaunchCfg& cfg, bool ring, bool slab);
bool flow2_variant_exists(int C);

hipError_t launch_sw_strip(const LaunchCfg& cfg, const KParams& kp, hipStream_t stream);
int kernel_waves_per_cu(const LaunchCfg& cfg);     // residency of the chosen variant
bool variant_exists(int W, int C);

}  // namespace swmi
