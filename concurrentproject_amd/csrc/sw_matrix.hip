// sw_matrix.hip -- local-alignment scores under a substitution matrix (affine gaps): the gfx950
// kernel, its launch and the pair / batch entry points of include/algoGPU.h.
//
// The recurrence is the engine's (sw_kernels.hip header; main.cpp:54-66) with s(a, b) a table
// lookup instead of a byte compare, in the same clamped form: E and F kept as max(E, 0),
// max(F, 0), the running maximum over t = H[i-1][j-1] + s only.
//
// ONE WAVE OWNS ONE PAIR.  The wave sweeps the pair's strips of 64*W columns left to right with
// the int32 anti-diagonal strip step of Strip<W, false> (sw_kernels.hip): W columns per lane,
// wave_shr:1 DPP moves for the flowing H - G_INIT, E - G_EXT and row code, the rotating I/O
// registers, v_max3.  A strip's right-edge column (H - G_INIT, E - G_EXT: 8 B a row) goes to a
// scratch buffer private to the wave and comes back as the next strip's inflow.  The buffer is
// used in place: a chunk that starts at step k0 has read rows up to k0 + 127 and waited for rows
// up to k0 + 63 before it stores rows k0 - (64W - 1) .. k0 + 64 - 64W <= k0, so a row is always
// read (and its load complete) before the same wave overwrites it.  Strips are separated by a
// wave-level wait for the stores (an agent-scope fence; the loads and stores are sc1, past the
// per-CU cache).  No wave ever waits for another wave: no spins, no tags, no barriers after the
// table is staged, hence nothing that can hang and no use for the "timeout" option.
//
// The score lookup: the workgroup stages the 256-byte byte-to-code map and, per orientation, a
// (K + 1)-row table of MAT_STRIDE bytes a row in LDS.  Row c of a table holds the scores of column
// symbol c (the sequence spread across the lanes) against every row symbol (the sequence that
// streams), so a lane's W lookups fall in its columns' own rows: one ds_read_i8 at
// table[col_code[p] * MAT_STRIDE + row_code] per cell.  Row K is for dead (past-the-end) columns,
// which the -DEAD bias keeps out of the maximum; column K is the "no row" sentinel, -127, so a
// cell without a row contributes t <= H[i-1][j-1], nothing new.  Orientation is per pair: table 0
// has seq1 across the lanes, table 1 (the transpose) seq2.
//
// Waves claim pairs in order from Ctrl::next_item; the host orders them longest first.
//
// ALIGNMENTS.  Tracing is a template parameter of the strip step, the pair loop and the kernel; the
// score-only instantiations are the code they were.  The traced variant (W = 8, seq1 always across
// the lanes) stores 4 bits a cell, a dword a lane a step, to a per-pair trace buffer (WalkPair below)
// and reports the end cell with the maximum; sw_matrix_walk_kernel then follows the recorded
// decisions from the end cell, one lane a pair (matrix_walk, the one walk of this file), and the host
// reverses and run-length encodes (sw_align_host.cpp).  The end-cell rule and the walk priorities
// are in include/algoGPU.h.  A launch holds at most option "trace_mb" MiB of trace; a pair that does
// not fit alone is refused there.
// Such pairs go through sw_align_matrix_long: a locate pass that keeps every strip's right-edge
// column (a checkpoint), then the strips filled again one at a time, traced, from the checkpoint on
// their left, and walked right to left -- the same bits, so the same alignment (LONG PAIRS below).
//
// ALIGNMENT MODES.  Everything above is local alignment.  Global and semi-global alignment
// (include/algoGPU.h SW_MODE_*) are a third template parameter of the same
// step, pair loop and kernel (AM, below): no clamp, borders made by the set-up and the inflow, the
// end read from one column.  The long path takes them too (LONG PAIRS IN A MODE below).
//
// BANDED ALIGNMENT (include/algoGPU.h sw_*_band) is a fourth template parameter
// (BAND, below) of the step, the pair loop and the kernel: a strip runs only the chunks that hold
// cells of the band, a cell outside it is forced to the absent state, the inflow is absent outside
// the rows the strip on the left stored, and the trace holds the band only.
//
// Every fill kernel is the same claim loop (matrix_stage, matrix_claim, matrix_claimed_pair) around matrix_pair, and
// the host names each instantiation once (MatCtx::fill).
//
// THE COOPERATIVE SCORE PATH (include/algoGPU.h sw_score_matrix_batch_coop) is the one
// exception to "one wave owns one pair" and to "no wave waits for another": its kernels, sw_matrix_coop_kernel<W, AM>,
// claim one strip of a pair at a time, and the wave of strip s + 1 follows the wave of strip s through the pair's edge
// columns with a bounded poll (option "timeout").  Opt-in, score-only, no band (COOPERATIVE SCORE below).
//
// LONG PAIRS ON MANY WAVES (include/algoGPU.h sw_align_matrix_long_coop) puts the locate pass of
// the long path on that hand-off -- the edge columns are the checkpoint columns -- and lets a round fill a window of
// consecutive strips of a pair, which do not depend on one another.  Opt-in, every mode; the same alignments.
#include "sw_device.h"
#include "sw_matrix_host.h"
#include "../../include/algoGPU.h"

#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <map>
#include <numeric>
#include <vector>

namespace swmi {

void report_stats(const sw_stats& s);   // sw_engine.hip: the calling thread's sw_last_stats()

namespace {

constexpr int MAT_ROWS = SW_MATRIX_MAX_K + 1;
constexpr int MAT_STRIDE = 36;                       // bytes a table row: K + 1 <= 33 entries, dword aligned
constexpr int MAT_TAB_BYTES = MAT_ROWS * MAT_STRIDE; // one orientation
constexpr int MAT_SENT = -127;                       // s of a cell without a row
constexpr int MAT_C = 64;                            // rows per inflow / outflow chunk
constexpr int MODE_MATRIX = 6;
constexpr int MODE_MATRIX_TRACE = 7;                 // the traced launches (alignments)
constexpr int MODE_MATRIX_LONG = 8;                  // checkpointed traceback of long pairs (sw_align_matrix_long)
constexpr int MODE_MATRIX_BAND = 9;                  // the band launches, score-only (sw_score_matrix_batch_band)
constexpr int MODE_MATRIX_BAND_TRACE = 10;           // and traced (sw_align_matrix_batch_band)
constexpr int MODE_MATRIX_PROFILE = 13;              // the profile launches, score-only (sw_score_profile_batch)
constexpr int MODE_MATRIX_PROFILE_TRACE = 14;        // and traced (sw_align_profile_batch)
constexpr int MODE_MATRIX_XLATE = 15;                // the translated launches, score-only (sw_score_matrix_translated_batch)
constexpr int MODE_MATRIX_XLATE_TRACE = 16;          // and traced (sw_align_matrix_translated_batch)
constexpr int TRACE_W = 8;                           // the traced variant's columns per lane: a step is a dword a lane
static_assert(SW_PROFILE_STRIDE == MAT_STRIDE && SW_PROFILE_SENT == MAT_SENT, "the profile image is rows of the table");

struct MatPair {
    uint64_t col_off;   // the sequence across the lanes
    uint64_t row_off;   // the sequence that streams
    int n, m;           // columns, rows (> 0)
    int out_idx;
    int swap_or_band;   // 1: the columns are seq2 (table 1); a band launch, which never swaps: the pair's band B
};

// Traced launches.  A cell's 4 bits: bits 0-1 where H came from (0 none: H = 0, 1 the diagonal, 2 E,
// 3 F), bit 2 E extended a gap (clear: opened one), bit 3 the same for F.  A step's 8 cells of a lane
// (its columns p = 0..7 at nibble p) are one dword, and the pair's buffer is [strip][step][lane]
// dwords: a step's 64 lanes store 256 contiguous bytes.  A strip has `steps` = 64 * chunks steps, so
// cell (i, j) -- i in seq1, across the lanes -- is nibble i & 7 of dword
// ((i >> 9) * steps + j + (i & 511)) * 64 + ((i & 511) >> 3).
struct WalkPair {
    uint64_t trace_off;     // bytes, from MatArgs::trace
    uint64_t ops_off;       // bytes, from WalkArgs::ops: n + m bytes, the operations last first
    unsigned trace_bytes;   // strips * steps * 256
    int steps;              // per strip
};
struct TraceRes {
    int score, ei, ej, pad;    // the fill kernel: the maximum and its end cell (one 16-B store)
    int bi, bj, nops, err;     // the walk kernel: the begin cell, operations written, WALK_* error
};
constexpr int WALK_OVERRUN = 1;   // more than n + m operations
constexpr int WALK_RANGE = 2;     // a cell outside the pair or its trace buffer

// Band launches (BANDED ALIGNMENT below): the pair's diagonal range, dlo <= j - i <= dhi.  A band
// launch never swaps the sequences (j - i has one meaning), and its MatPair::swap_or_band is the pair's
// band B (clamped to max(n, m): band_range, sw_align_host.cpp); the kernels derive the range from it.
struct BandPair {
    int dlo, dhi;
};
__host__ __device__ inline BandPair band_of(int n, int m, int B) {
    return BandPair{(m < n ? m - n : 0) - B, (m > n ? m - n : 0) + B};
}

struct MatArgs {
    const unsigned char* seq;
    const MatPair* pairs;
    Ctrl* ctrl;
    int* scores;
    uint2* scratch;           // scratch_rows entries per wave
    long long scratch_rows;
    int npairs;
    int nscores;              // entries of scores
    int gap_init, gap_ext;
    int k;                    // symbols: code k is the sentinel / dead code
    unsigned code[64];        // the byte-to-code map, 256 bytes
    unsigned tab[2 * MAT_TAB_BYTES / 4];
    // traced launches only
    const WalkPair* walk;     // per item
    unsigned char* trace;
    TraceRes* res;            // nscores entries
    // profile launches only (PROFILE below): the device image, pd.n + 1 rows of MAT_STRIDE bytes
    // translated launches (XLATE below) instead: the two tables of the translation in a small device buffer, the
    // base-class map, 256 bytes, then the matrix code of every codon's amino acid, 68 bytes, entry 64 that of 'X'
    // (sw_translated_tables).  MatArgs does not grow for them: no existing kernel sees another argument layout.
    const unsigned char* prof;
};
static_assert(sizeof(MatArgs) <= 4096, "kernel arguments");
static_assert(MAT_TAB_BYTES % 4 == 0, "table words");

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// MODE: M_SCORE the maximum only; M_TRACE the traced step: the end-cell bookkeeping and a dword of
// decisions a lane a step; M_LOCATE the bookkeeping without the stores (long pairs, below).
constexpr int M_SCORE = 0, M_TRACE = 1, M_LOCATE = 2;

// AM: the alignment mode (include/algoGPU.h SW_MODE_*), a compile-time parameter as MODE is: the
// local instantiations are the code they were.  Global and semi-global have
// no clamp at 0, so nothing makes the borders for free:
//   * the top border H[i][-1] = -(G_INIT + i * gx), gx = min(G_EXT, G_INIT), is the E chain of row
//     -1, which the pre-border cells compute themselves: setup() puts H[i0][-1] (as H and as E) into
//     the strip's first column, whose state before step 0 is row -1, H[i0-1][-1] into its diagonal,
//     and MAT_NEG ("minus infinity") everywhere else.  Column c then meets row -1 at step c - 1 with
//     t and F from rows <= -2 (MAT_NEG and below) and E = max(E - G_EXT, H - G_INIT) from column
//     c - 1: exactly H[c][-1], one step before its first row arrives, at no cost in the step;
//   * the left border of strip 0 is the inflow: H[-1][j] (0, or -(G_INIT + j * gx)) and E = MAT_NEG;
//   * the end: one lane follows one column, n - 1 (`pstar` of the lane that holds it in the last
//     strip), over the row window [0, m) (semi-global) or [m - 1, m) (global): jrow is the row of
//     that column at this step minus the window's first row, MAT_NEG on every other lane, so
//     pre-border, drain and dead-column cells are never candidates; the strict update keeps the
//     smallest j.
// Pre-border, drain and dead-column cells hold unclamped garbage: mode_range_ok (sw_align_host.cpp)
// refuses the pairs on which any of it could wrap.
constexpr int AM_LOCAL = SW_MODE_LOCAL, AM_GLOBAL = SW_MODE_GLOBAL, AM_SEMI = SW_MODE_SEMIGLOBAL;
constexpr int MAT_NEG = -(1 << 30);

// BAND: the banded step (BANDED ALIGNMENT below), one more compile-time parameter: a cell outside
// the band is forced to the "absent" state every step -- the border state H = E = F = 0 (local),
// MAT_NEG for all three (global, semi-global) -- and never updates M.
//   * the mask: bu is the lane's diagonal counter, (j - i) - dlo of its column p = 0 at this step,
//     advanced once a step; column p is 2p diagonals behind, so the cell is in the band iff
//     (unsigned)(bu - 2p) <= dhi - dlo;
//   * row -1 (global, semi-global): H[i][-1] is a border, not a cell, and must reach every column
//     whose cell (i, 0) is in the band: i <= -dlo.  The raw test keeps the E chain of row -1 up to
//     i = -dlo - 1 only.  The one missing cell (-dlo, -1) is met by one lane at one step: bz counts
//     up to 0 there (and never reaches 0 anywhere else), and at that step that lane tests
//     (unsigned)(bu + 1 - 2p) <= dhi - dlo + 1 instead: the lower bound one diagonal lower, the upper
//     bound where it was.  The lane's other cells of that step are either in rows >= 0 on diagonals
//     >= dlo + 1 (columns before it: unaffected) or in rows <= -2 (columns after it: never read by a
//     cell of the matrix).
//
// PROFILE: position-specific scoring (include/algoGPU.h sw_*_profile_*), a fifth
// compile-time parameter: the columns are the positions of a profile, and column c reads its scores from a
// table row that is its own, P[c][.], instead of the row of its residue in a table the workgroup shares.  The
// step is the same step: cb[p] is still "the LDS offset of this column's table row".  The rows live in a slab
// that belongs to the wave, W * 64 slots of MAT_STRIDE bytes laid out [p][lane] (a lane's slots are 9 dwords from
// its neighbour's: odd, so a step's 64 byte reads at one row code fall in 64 different banks), and before each
// strip lane l copies the rows of its W columns there from the device image (stage_rows).  A lane reads only
// the slots it wrote itself, and a wave's LDS operations complete in order: no barrier, and nothing shared
// with the other waves of the workgroup.  LDS does not grow with the profile's length.  Row pd.n of the image is
// the dead row, for the columns past the end.  seq1 is always the profile: there is no swap, no band, no
// cooperative and no long instantiation.
template <int W, int MODE, int AM = AM_LOCAL, bool BAND = false, bool PROFILE = false>
struct MStrip {
    static_assert(MODE == M_SCORE || W == TRACE_W, "a traced step stores one dword a lane");
    static_assert(!BAND || MODE != M_LOCATE, "the long path has no band");
    static_assert(!PROFILE || (!BAND && MODE != M_LOCATE), "a profile has neither a band nor a long path");
    int cb[W], tb[W];                       // LDS offset of the column's table row / bias
    int hgA[W], hgB[W], eh[W], r[W], fh[W]; // DP state, as Strip (sw_kernels.hip)
    int L0, M, IOH, IOE, IOR;
    int Mkp, kp8;                           // M_TRACE, M_LOCATE: step * 8 + p at which M was reached; this step * 8
    int pstar, jrow, wl, Mj;                // AM != AM_LOCAL: the end bookkeeping (above); M is H - G_INIT there
    int bu, bz;                             // BAND: the diagonal counter and the row -1 exception (above)
    int bt, bts;                            // BAND, M_TRACE: the lane's trace step (band_trace_origin) and their number

    __device__ __forceinline__ void setup(const MatArgs& a, const MatPair& pd, int strip, int lane,
                                          const unsigned char* s_code) {
        constexpr int SW = 64 * W;
        const int go = a.gap_init, ge = a.gap_ext;
        if constexpr (PROFILE) {   // the lane's own slots of the wave's slab (stage_rows fills them)
#pragma unroll
            for (int p = 0; p < W; ++p) {
                cb[p] = (p * 64 + lane) * MAT_STRIDE;
                tb[p] = strip * SW + lane * W + p < pd.n ? go : -DEAD;
            }
        } else {
            const unsigned char* colseq = a.seq + pd.col_off;
            const int tbase = pd.swap_or_band ? MAT_TAB_BYTES : 0;   // (a band launch's claim loop has taken B out)
#pragma unroll
            for (int p = 0; p < W; ++p) {
                const int c = strip * SW + lane * W + p;
                if (c < pd.n) {
                    cb[p] = tbase + (int)s_code[colseq[c]] * MAT_STRIDE;
                    tb[p] = go;
                } else {
                    cb[p] = tbase + a.k * MAT_STRIDE;
                    tb[p] = -DEAD;
                }
            }
        }
#pragma unroll
        for (int p = 0; p < W; ++p) {   // everything starts at the border (H = E = F = 0)
            hgA[p] = -go; hgB[p] = -go; eh[p] = -ge; fh[p] = -ge; r[p] = a.k;
        }
        L0 = -go; IOH = -go; IOE = -ge; IOR = a.k;
        if constexpr (AM != AM_LOCAL) {
            const int gx = min(go, ge), i0 = strip * SW;
            const int b0 = -(go + i0 * gx);   // H[i0][-1]
#pragma unroll
            for (int p = 0; p < W; ++p) {
                hgA[p] = MAT_NEG; hgB[p] = MAT_NEG; eh[p] = MAT_NEG; fh[p] = MAT_NEG;
            }
            hgB[0] = lane == 0 ? b0 - go : MAT_NEG;   // the first step's hgPrev
            eh[0] = lane == 0 ? b0 - ge : MAT_NEG;
            L0 = lane == 0 ? (i0 > 0 ? b0 + gx : 0) - go : MAT_NEG;   // H[i0-1][-1]
            IOE = MAT_NEG;
            const int cl = pd.n - 1 - i0;   // column n - 1 in this strip (the last strip: 0 <= cl < SW)
            const int jlo = AM == AM_GLOBAL ? pd.m - 1 : 0;
            pstar = cl & (W - 1);
            jrow = cl >= 0 && cl < SW && cl / W == lane ? -cl - jlo : MAT_NEG;
            wl = pd.m - jlo;
        }
    }

    // PROFILE, before the strip's first step: rows min(c, pd.n) of the image, c the lane's W columns, into the
    // lane's slots of the wave's slab.  Every row read is inside the image (pd.n + 1 rows) and every slot written
    // inside the slab (W * 64 slots).  The strip's reads of these slots come after these writes in the wave's own
    // LDS order, and the previous strip's reads before them: only the compiler's wait for the writes is needed.
    __device__ __forceinline__ void stage_rows(const MatArgs& a, const MatPair& pd, int strip, int lane, unsigned* slab) {
        constexpr int SW = 64 * W, RW = MAT_STRIDE / 4;
        const unsigned* img = reinterpret_cast<const unsigned*>(a.prof);
#pragma unroll
        for (int p = 0; p < W; ++p) {
            const unsigned* src = img + (size_t)min(strip * SW + lane * W + p, pd.n) * RW;
            unsigned* dst = slab + (p * 64 + lane) * RW;
#pragma unroll
            for (int q = 0; q < RW; ++q) dst[q] = src[q];
        }
    }

    // BAND, after setup(): the strip starts at step kf (a multiple of 64), not at 0.
    __device__ __forceinline__ void band_setup(int strip, int lane, int kf, int dlo) {
        constexpr int SW = 64 * W;
        const int i0 = strip * SW;
        bu = kf - i0 - 2 * lane * W - dlo;
        bz = 1;
        if constexpr (AM != AM_LOCAL) {
            const int cs = -dlo - i0;   // column -dlo in this strip: its row -1 cell is the exception (kf is 0 then)
            bz = cs >= 1 && cs < SW && cs / W == lane ? 1 - cs : 1;
            if (i0 + dlo > 0) {   // no column of the strip has its row 0 in the band: no border to build
                hgB[0] = MAT_NEG;
                eh[0] = MAT_NEG;
                L0 = MAT_NEG;
            }
            jrow = jrow == MAT_NEG ? MAT_NEG : jrow + kf;
        }
    }

    // One anti-diagonal step (Strip::step with the score from the LDS table).
    // M_TRACE: the step's cells go to trc at byte toff (the lane's dword of this step).  M_TRACE and
    // M_LOCATE: M is updated strictly, so that a lane keeps the first step (anti-diagonal) that
    // reached its maximum and, within a step, the largest p: the smallest row.
    __device__ __forceinline__ void step(int (&hgCur)[W], const int (&hgPrev)[W], const bool l63, const int go,
                                         const int ge, const signed char* s_tab, const __amdgpu_buffer_rsrc_t trc,
                                         unsigned& toff, const int bw = 0) {
        const int ioh = dpp_rol1(IOH), ioe = dpp_rol1(IOE), ior = dpp_rol1(IOR);
        const int hgL0 = dpp_shr1(IOH, hgPrev[W - 1]);
        const int ehL0 = dpp_shr1(IOE, eh[W - 1]);
        const int rL0 = dpp_shr1(IOR, r[W - 1]);
        // the W lookups first (they need only the row codes): their LDS latencies overlap
        int sv[W];
#pragma unroll
        for (int p = 0; p < W; ++p) sv[p] = (int)s_tab[cb[p] + (p > 0 ? r[p - 1] : rL0)];   // ds_read_i8
        unsigned bits = 0;
        int bue = 0, bwe = 0;   // BAND: this step's test (the exception moves both by one)
        if constexpr (BAND) {
            bue = bu;
            bwe = bw;
            if constexpr (AM != AM_LOCAL) {
                const int e = bz == 0 ? 1 : 0;
                bue += e;
                bwe += e;
                bz += 1;
            }
            bu += 1;
        }
#pragma unroll
        for (int p = W - 1; p >= 0; --p) {
            const int q = p > 0 ? p - 1 : 0;
            const int hgL = p > 0 ? hgPrev[q] : hgL0;
            const int ehL = p > 0 ? eh[q] : ehL0;
            const int rL = p > 0 ? r[q] : rL0;
            const int hgD = p > 0 ? hgCur[q] : L0;
            const int t = hgD + sv[p] + tb[p];           // H[i-1][j-1] + s(q_j, d_i)
            const int E = AM == AM_LOCAL ? max3i(ehL, hgL, 0) : max(ehL, hgL);               // clamped E (local)
            const int F = AM == AM_LOCAL ? max3i(fh[p], hgPrev[p], 0) : max(fh[p], hgPrev[p]);   // clamped F (local)
            const int H = vmax3(t, E, F);
            bool inb = true;
            if constexpr (BAND) inb = (unsigned)(bue - 2 * p) <= (unsigned)bwe;
            if constexpr (AM != AM_LOCAL) {
                if constexpr (MODE == M_TRACE) {   // source 0 is unused: there is no H = 0 stop
                    const unsigned src = t == H ? 1u : (E == H ? 2u : 3u);
                    bits |= (src | (ehL > hgL ? 4u : 0u) | (fh[p] > hgPrev[p] ? 8u : 0u)) << (4 * p);
                }
            } else if constexpr (MODE != M_SCORE) {
                const bool up = BAND ? inb && t > M : t > M;
                M = up ? t : M;
                Mkp = up ? kp8 + p : Mkp;
                if constexpr (MODE == M_TRACE) {
                    const unsigned src = H == 0 ? 0u : (t == H ? 1u : (E == H ? 2u : 3u));
                    bits |= (src | (ehL > hgL ? 4u : 0u) | (fh[p] > hgPrev[p] ? 8u : 0u)) << (4 * p);
                }
            } else {
                if constexpr (BAND) M = inb ? max(M, t) : M;
                else M = max(M, t);
            }
            if constexpr (BAND) {   // absent: the border state (local: H - go, E - ge of 0), minus infinity (else)
                hgCur[p] = inb ? H - go : (AM == AM_LOCAL ? -go : MAT_NEG);
                eh[p] = inb ? E - ge : (AM == AM_LOCAL ? -ge : MAT_NEG);
                fh[p] = inb ? F - ge : (AM == AM_LOCAL ? -ge : MAT_NEG);
            } else {
                hgCur[p] = H - go;
                eh[p] = E - ge;
                fh[p] = F - ge;
            }
            r[p] = rL;
        }
        L0 = hgL0;
        IOH = l63 ? hgCur[W - 1] : ioh;   // lane 63 <- this step's right-edge output
        IOE = l63 ? eh[W - 1] : ioe;
        IOR = ior;
        if constexpr (MODE == M_TRACE && BAND) {   // the lane's own run of dwords; a step outside it is dropped
            __builtin_amdgcn_raw_buffer_store_b32(bits, trc, (unsigned)bt < (unsigned)bts ? toff : OOR, 0, 0);
            toff += 4u;
            bt += 1;
        } else if constexpr (MODE == M_TRACE) {
            __builtin_amdgcn_raw_buffer_store_b32(bits, trc, toff, 0, 0);
            toff += 256u;
        }
        if constexpr (MODE != M_SCORE) kp8 += 8;
        if constexpr (AM != AM_LOCAL) {   // the lane's cell of column n - 1, if its row is in the window
            int cand = hgCur[0];
#pragma unroll
            for (int p = 1; p < W; ++p) cand = pstar == p ? hgCur[p] : cand;
            const bool in = (unsigned)jrow < (unsigned)wl;
            if constexpr (MODE != M_SCORE) {
                const bool up = in && cand > M;
                M = up ? cand : M;
                Mj = up ? jrow : Mj;
            } else {
                M = in ? max(M, cand) : M;
            }
            jrow += 1;
        }
    }

    __device__ __forceinline__ void run(const bool l63, const int go, const int ge, const signed char* s_tab,
                                        const __amdgpu_buffer_rsrc_t trc, unsigned& toff, const int bw = 0) {
#pragma unroll 2
        for (int s = 0; s < MAT_C; s += 2) {
            step(hgA, hgB, l63, go, ge, s_tab, trc, toff, bw);
            step(hgB, hgA, l63, go, ge, s_tab, trc, toff, bw);
        }
    }
};

__device__ __forceinline__ unsigned mat_fetch_raw(const __amdgpu_buffer_rsrc_t row_rsrc, int k0, int lane, int m) {
    const int row = k0 + lane;
    return __builtin_amdgcn_raw_buffer_load_b8(row_rsrc, row < m ? (unsigned)row : OOR, 0, 0);
}
// XLATE: translated search (include/algoGPU.h sw_*_matrix_translated*), a sixth compile-time
// parameter of the pair loop and the kernel, not of the step: the rows are the residues of one reading frame of a
// DNA, and only where a chunk's row code comes from changes.  The item's rows are the 3 * m bases the frame covers
// (row_rsrc holds exactly those, so the resource drops any stray read), pd.swap_or_band says the frame is a minus
// frame, and seq1 is always across the lanes (table 0).  A lane loads the three bytes of its row's codon, one
// chunk ahead as the byte of a plain row is: row r of a plus frame at 3r, 3r + 1, 3r + 2; of a minus frame at
// 3(m - 1 - r) + 2, + 1, + 0, to be complemented.  The three travel as one dword.
__device__ __forceinline__ unsigned xl_fetch_raw(const __amdgpu_buffer_rsrc_t row_rsrc, int k0, int lane, int m, int minus) {
    const int row = k0 + lane;
    const bool live = row < m;
    const unsigned o0 = minus ? 3u * (unsigned)(m - 1 - row) + 2u : 3u * (unsigned)row;
    const unsigned o1 = minus ? o0 - 1u : o0 + 1u, o2 = minus ? o0 - 2u : o0 + 2u;
    const unsigned b0 = __builtin_amdgcn_raw_buffer_load_b8(row_rsrc, live ? o0 : OOR, 0, 0);
    const unsigned b1 = __builtin_amdgcn_raw_buffer_load_b8(row_rsrc, live ? o1 : OOR, 0, 0);
    const unsigned b2 = __builtin_amdgcn_raw_buffer_load_b8(row_rsrc, live ? o2 : OOR, 0, 0);
    return (b0 & 0xFFu) | (b1 & 0xFFu) << 8 | (b2 & 0xFFu) << 16;
}
// the row code of a fetched codon: the bytes' classes through the base map in LDS (a minus frame complements a
// class, x ^ 2; an ambiguous byte stays above 3 either way), then the composed codon table at 16a + 4b + c, or
// its entry 64 when a base is ambiguous
__device__ __forceinline__ int xl_row_code(unsigned raw, int minus, const unsigned char* s_base, const unsigned char* s_codon) {
    const int cx = minus ? 2 : 0;
    const int c0 = (int)s_base[raw & 0xFFu] ^ cx, c1 = (int)s_base[(raw >> 8) & 0xFFu] ^ cx, c2 = (int)s_base[(raw >> 16) & 0xFFu] ^ cx;
    return (int)s_codon[(c0 | c1 | c2) > 3 ? 64 : 16 * c0 + 4 * c1 + c2];
}
__device__ __forceinline__ u32x2 mat_fetch_edge(const __amdgpu_buffer_rsrc_t scr_rsrc, int k0, int lane, int m) {
    const int row = k0 + lane;
    return __builtin_amdgcn_raw_buffer_load_b64(scr_rsrc, row < m ? (unsigned)row * 8u : OOR, 0, AUX_SC1);
}
// BAND: only the rows [olo, ohi] that the strip on the left stored (band_rows below)
__device__ __forceinline__ u32x2 mat_fetch_edge_band(const __amdgpu_buffer_rsrc_t scr_rsrc, int k0, int lane, int olo, int ohi) {
    const int row = k0 + lane;
    return __builtin_amdgcn_raw_buffer_load_b64(scr_rsrc, row >= olo && row <= ohi ? (unsigned)row * 8u : OOR, 0, AUX_SC1);
}

// BANDED ALIGNMENT (include/algoGPU.h sw_*_band).  Only the cells with
// dlo <= j - i <= dhi exist.  A strip of columns [i0, i0 + SW) meets cells of the band at the steps
// k = j + c in [max(0, i0 + dlo), min(m - 1, i0 + SW - 1 + dhi) + SW - 1] and runs the chunks of 64
// that hold them, from one step earlier: the first cell of column i0, (i0, i0 + dlo), takes its diagonal
// input H[i0 - 1][i0 + dlo - 1] from the inflow of the step before.  kf is the first step, nch the chunks.  (The corner (n - 1, m - 1) is in the band and
// i0 <= n - 1, so i0 + dlo <= m - 1: every strip has rows.)  Rows below kf never enter the strip: every
// cell that would need them lies below diagonal dlo.  The same two functions on the host: band_first,
// band_chunks (sw_align_host.cpp).
__device__ __forceinline__ int band_kf(int i0, int dlo) { return max(0, i0 + dlo - 1) & ~63; }
// THE BAND'S TRACE.  A dense [step][lane] strip would hold width + 2 * 512 steps: the skew of the
// wavefront, not the band.  Instead every lane keeps its own run of dwords: lane l's eight columns
// i0 + 8l + p meet cells of the band at the steps from max(0, i0 + 8l + dlo) + 8l (column p = 0 enters
// the band; the others enter later) to min(m - 1, i0 + 8l + 7 + dhi) + 8l + 7: at most
// min(dhi - dlo, m - 1) + 15 steps, the pair's wp.steps.  The trace is [strip][lane][step - origin]
// dwords, n / 8 * steps * 4 bytes: n * width / 2, and a lane fills a cache line in 16 steps of its own.
__device__ __forceinline__ int band_trace_origin(int i0, int lane, int dlo) {
    return max(0, i0 + TRACE_W * lane + dlo) + TRACE_W * lane;
}
__device__ __forceinline__ int band_nch(int i0, int SW, int m, int dlo, int dhi) {
    return (min(m - 1, i0 + SW - 1 + dhi) + SW - 1 - band_kf(i0, dlo)) / 64 + 1;
}

// All strips of one pair on this wave; scr: the wave's scratch (at least m entries when the pair has
// more than one strip).  TRACE: wp is the pair's trace buffer; the result is the maximum with its end
// cell -- among the cells whose t equals the maximum, the smallest i + j, then the smallest row j
// (include/algoGPU.h) -- so each strip starts its own M and the strips are merged by that rule.
// M_LOCATE: the same result without a trace; strip s reads its inflow from checkpoint column s - 1
// of the pair and stores its right edge to column s (ckpt: column 0, ckpt_stride bytes a column,
// m * 8 of them used), every column a buffer of its own, and the scratch is not touched.
// BAND: bp is the pair's diagonal range.  Strip s runs the steps [kf, kf + 64 * nch) of its own, the
// trace is [strip][lane][step - band_trace_origin] with wp.steps dwords a lane (below), and
// the inflow is what the strip on the left stored -- its rows [olo, ohi] -- and "absent" outside them:
// the scratch column there holds rows of the strip before last or of an earlier pair.  The column is
// still used in place: a chunk at k0 stores rows <= k0 + 64 - SW <= k0, a row r is read by the chunk
// that holds it, k0' <= r, and that read is complete before chunk k0' runs, so before any store of
// chunk k0 >= k0'; which rows a strip skips changes nothing in that.
// PROFILE: the columns are the positions of a profile; s_tab is the wave's slab (MStrip above), filled again
// before every strip.
// XLATE: the rows are the residues of a reading frame (xl_fetch_raw above); minus: the frame is a minus frame;
// s_base and s_codon: the two tables of the translation in LDS.
template <int W, int MODE, int AM = AM_LOCAL, bool BAND = false, bool PROFILE = false, bool XLATE = false>
__device__ void matrix_pair(const MatArgs& a, const MatPair& pd, const WalkPair& wp, const int lane, uint2* scr,
                            const signed char* s_tab, const unsigned char* s_code, unsigned char* ckpt = nullptr,
                            unsigned ckpt_stride = 0, const BandPair bp = BandPair{0, 0}, const int minus = 0,
                            const unsigned char* s_base = nullptr, const unsigned char* s_codon = nullptr) {
    static_assert(!XLATE || (!BAND && !PROFILE && MODE != M_LOCATE), "a translated frame has no band, profile or long path");
    constexpr bool TRACE = MODE != M_SCORE;   // the end cell is kept
    constexpr int SW = 64 * W, C = MAT_C;
    const int m = pd.m;
    const int go = a.gap_init, ge = a.gap_ext;
    const bool l63 = lane == 63;
    const int strips = (pd.n + SW - 1) / SW;
    const __amdgpu_buffer_rsrc_t row_rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(a.seq + pd.row_off), 0, XLATE ? 3 * m : m, RSRC_FLAGS);
    // a single strip never touches the scratch: a resource of no bytes drops every access
    const __amdgpu_buffer_rsrc_t scr_rsrc =
        __builtin_amdgcn_make_buffer_rsrc(scr, 0, MODE != M_LOCATE && strips > 1 ? (int)((unsigned)m * 8u) : 0, RSRC_FLAGS);
    const int nchunks = (m + SW - 1 + C - 1) / C;
    // every store of a step is inside the buffer by construction (strips * steps * 256 bytes); the
    // resource drops whatever is not
    const __amdgpu_buffer_rsrc_t trc =
        MODE == M_TRACE ? __builtin_amdgcn_make_buffer_rsrc(a.trace + wp.trace_off, 0, (int)wp.trace_bytes, RSRC_FLAGS)
                        : scr_rsrc;
    unsigned toff = (unsigned)lane * 4u;
    int bM = 0, bD = 0, bJ = 0;   // TRACE: the best of the strips so far: t, i + j, j
    MStrip<W, MODE, AM, BAND, PROFILE> S;
    S.M = AM == AM_LOCAL ? 0 : MAT_NEG;
    if constexpr (AM != AM_LOCAL) S.Mj = 0;
    for (int strip = 0; strip < strips; ++strip) {
        S.setup(a, pd, strip, lane, s_code);
        if constexpr (PROFILE) S.stage_rows(a, pd, strip, lane, reinterpret_cast<unsigned*>(const_cast<signed char*>(s_tab)));
        if constexpr (TRACE && AM == AM_LOCAL) {
            S.M = 0;
            S.Mkp = 0;
            S.kp8 = 0;
        }
        const bool has_in = strip > 0;
        const bool has_out = strip < strips - 1;
        if constexpr (BAND) {
            const int i0 = strip * SW, kf = band_kf(i0, bp.dlo), nch = band_nch(i0, SW, m, bp.dlo, bp.dhi);
            const int bw = bp.dhi - bp.dlo;
            S.band_setup(strip, lane, kf, bp.dlo);
            // the rows the strip on the left stored: its lane l of chunk k0 stores row k0 + l - (SW - 1)
            const int kfl = band_kf(i0 - SW, bp.dlo);
            const int olo = max(0, kfl - (SW - 1)), ohi = min(m - 1, kfl + 64 * band_nch(i0 - SW, SW, m, bp.dlo, bp.dhi) - SW);
            if constexpr (MODE == M_TRACE) {
                S.bt = kf - band_trace_origin(i0, lane, bp.dlo);
                S.bts = wp.steps;
                toff = (((unsigned)strip * 64u + (unsigned)lane) * (unsigned)wp.steps + (unsigned)S.bt) * 4u;
            }
            unsigned raw_nxt = mat_fetch_raw(row_rsrc, kf, lane, m);
            u32x2 g_nxt = has_in ? mat_fetch_edge_band(scr_rsrc, kf, lane, olo, ohi) : u32x2{0u, 0u};
            for (int c = 0; c < nch; ++c) {
                const int k0 = kf + c * C;
                const unsigned raw = raw_nxt;
                const u32x2 g = g_nxt;
                raw_nxt = mat_fetch_raw(row_rsrc, k0 + C, lane, m);
                if (has_in) g_nxt = mat_fetch_edge_band(scr_rsrc, k0 + C, lane, olo, ohi);
                const int row = k0 + lane;
                const bool inr = row >= olo && row <= ohi;
                S.IOR = row < m ? (int)s_code[raw & 0xFFu] : a.k;
                if constexpr (AM == AM_LOCAL) {
                    S.IOH = has_in && inr ? (int)g.x : -go;
                    S.IOE = has_in && inr ? (int)g.y : -ge;
                } else {   // strip 0: the left border, which is not masked; else absent outside the stored rows
                    const int lb = AM == AM_GLOBAL ? -(go + row * min(go, ge)) - go : -go;
                    S.IOH = has_in ? (inr ? (int)g.x : MAT_NEG) : lb;
                    S.IOE = has_in && inr ? (int)g.y : MAT_NEG;
                }
                S.run(l63, go, ge, s_tab, trc, toff, bw);
                if (has_out) {
                    const int row_out = k0 + lane - (SW - 1);
                    const bool st = row_out >= 0 && row_out < m;
                    __builtin_amdgcn_raw_buffer_store_b64(u32x2{(unsigned)S.IOH, (unsigned)S.IOE}, scr_rsrc,
                                                          st ? (unsigned)row_out * 8u : OOR, 0, AUX_SC1);
                }
            }
            if (has_out) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
            if constexpr (TRACE && AM == AM_LOCAL) {
                const int k = kf + (S.Mkp >> 3), cl = lane * W + (S.Mkp & 7);
                const int j = k - cl, d = strip * SW + k;
                const bool better = S.M > bM || (S.M == bM && (d < bD || (d == bD && j < bJ)));
                bM = better ? S.M : bM;
                bD = better ? d : bD;
                bJ = better ? j : bJ;
            }
            continue;
        }
        __amdgpu_buffer_rsrc_t in_rsrc = scr_rsrc, out_rsrc = scr_rsrc;
        if constexpr (MODE == M_LOCATE) {   // a column that is not there (strip 0's left, the last strip's right) has no bytes
            in_rsrc = __builtin_amdgcn_make_buffer_rsrc(ckpt + (uint64_t)(has_in ? strip - 1 : 0) * ckpt_stride, 0,
                                                        has_in ? (int)((unsigned)m * 8u) : 0, RSRC_FLAGS);
            out_rsrc = __builtin_amdgcn_make_buffer_rsrc(ckpt + (uint64_t)(has_out ? strip : 0) * ckpt_stride, 0,
                                                         has_out ? (int)((unsigned)m * 8u) : 0, RSRC_FLAGS);
        }
        unsigned raw_nxt = XLATE ? xl_fetch_raw(row_rsrc, 0, lane, m, minus) : mat_fetch_raw(row_rsrc, 0, lane, m);
        u32x2 g_nxt = has_in ? mat_fetch_edge(in_rsrc, 0, lane, m) : u32x2{0u, 0u};
        for (int c = 0; c < nchunks; ++c) {
            const int k0 = c * C;
            const unsigned raw = raw_nxt;
            const u32x2 g = g_nxt;
            // the next chunk's rows in flight while this chunk computes
            raw_nxt = XLATE ? xl_fetch_raw(row_rsrc, k0 + C, lane, m, minus) : mat_fetch_raw(row_rsrc, k0 + C, lane, m);
            if (has_in) g_nxt = mat_fetch_edge(in_rsrc, k0 + C, lane, m);
            const bool live = k0 + lane < m;
            if constexpr (XLATE) S.IOR = live ? xl_row_code(raw, minus, s_base, s_codon) : a.k;
            else S.IOR = live ? (int)s_code[raw & 0xFFu] : a.k;
            if constexpr (AM == AM_LOCAL) {
                S.IOH = has_in && live ? (int)g.x : -go;
                S.IOE = has_in && live ? (int)g.y : -ge;
            } else {   // strip 0: the left border H[-1][j], and no E to extend out of it
                const int lb = AM == AM_GLOBAL ? -(go + (k0 + lane) * min(go, ge)) - go : -go;
                S.IOH = has_in && live ? (int)g.x : lb;
                S.IOE = has_in && live ? (int)g.y : MAT_NEG;
            }
            S.run(l63, go, ge, s_tab, trc, toff);
            if (has_out) {   // lane l holds the right edge of row k0 + l - (SW - 1)
                const int row_out = k0 + lane - (SW - 1);
                const bool st = row_out >= 0 && row_out < m;
                __builtin_amdgcn_raw_buffer_store_b64(u32x2{(unsigned)S.IOH, (unsigned)S.IOE}, out_rsrc,
                                                      st ? (unsigned)row_out * 8u : OOR, 0, AUX_SC1);
            }
        }
        // the next strip (or the next pair's) reads what this one stored
        if (has_out) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
        if constexpr (TRACE && AM == AM_LOCAL) {   // the lane's cell of this strip: column lane * W + p, reached at step k
            const int k = S.Mkp >> 3, cl = lane * W + (S.Mkp & 7);
            const int j = k - cl, d = strip * SW + k;
            const bool better = S.M > bM || (S.M == bM && (d < bD || (d == bD && j < bJ)));
            bM = better ? S.M : bM;
            bD = better ? d : bD;
            bJ = better ? j : bJ;
        }
    }
    if constexpr (AM != AM_LOCAL) {   // one lane holds the end; M is H - G_INIT
        int M = S.M, J = S.Mj;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const int oM = __shfl_xor(M, off), oJ = __shfl_xor(J, off);
            J = oM > M ? oJ : J;
            M = max(M, oM);
        }
        // lane 0's store without a branch on the lane (below)
        if constexpr (TRACE) {
            const int jlo = AM == AM_GLOBAL ? m - 1 : 0;
            const __amdgpu_buffer_rsrc_t res_rsrc = __builtin_amdgcn_make_buffer_rsrc(
                a.res, 0, (int)((unsigned)a.nscores * (unsigned)sizeof(TraceRes)), RSRC_FLAGS);
            __builtin_amdgcn_raw_buffer_store_b128(u32x4{(unsigned)(M + go), (unsigned)(pd.n - 1), (unsigned)(J + jlo), 0u},
                                                   res_rsrc, lane == 0 ? (unsigned)pd.out_idx * (unsigned)sizeof(TraceRes) : OOR,
                                                   0, 0);
        } else {
            const __amdgpu_buffer_rsrc_t sc_rsrc =
                __builtin_amdgcn_make_buffer_rsrc(a.scores, 0, (int)((unsigned)a.nscores * 4u), RSRC_FLAGS);
            __builtin_amdgcn_raw_buffer_store_b32(M + go, sc_rsrc, lane == 0 ? (unsigned)pd.out_idx * 4u : OOR, 0, 0);
        }
        return;
    }
    if constexpr (TRACE) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const int oM = __shfl_xor(bM, off), oD = __shfl_xor(bD, off), oJ = __shfl_xor(bJ, off);
            const bool better = oM > bM || (oM == bM && (oD < bD || (oD == bD && oJ < bJ)));
            bM = better ? oM : bM;
            bD = better ? oD : bD;
            bJ = better ? oJ : bJ;
        }
        // lane 0's store without a branch on the lane (below)
        const __amdgpu_buffer_rsrc_t res_rsrc =
            __builtin_amdgcn_make_buffer_rsrc(a.res, 0, (int)((unsigned)a.nscores * (unsigned)sizeof(TraceRes)), RSRC_FLAGS);
        __builtin_amdgcn_raw_buffer_store_b128(u32x4{(unsigned)bM, (unsigned)(bD - bJ), (unsigned)bJ, 0u}, res_rsrc,
                                               lane == 0 ? (unsigned)pd.out_idx * (unsigned)sizeof(TraceRes) : OOR, 0, 0);
        return;
    }
    int M = S.M;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) M = max(M, __shfl_xor(M, off));
    // Lane 0's store, without a branch on the lane: after `if (lane == 0) store` the compiler threads
    // the claim loop's `if (lane == 0) atomicAdd` onto it, and lanes 1..63 then reach the next
    // iteration's readfirstlane on their own, with lane 0 masked off, read item 0 and never leave.
    const __amdgpu_buffer_rsrc_t sc_rsrc =
        __builtin_amdgcn_make_buffer_rsrc(a.scores, 0, (int)((unsigned)a.nscores * 4u), RSRC_FLAGS);
    __builtin_amdgcn_raw_buffer_store_b32(M, sc_rsrc, lane == 0 ? (unsigned)pd.out_idx * 4u : OOR, 0, 0);
}

// THE CLAIM LOOP of every fill kernel: the workgroup stages the byte-to-code map and both tables in
// LDS, then each wave claims items from Ctrl::next_item until none is left.
struct MatLds {
    const signed char* tab;
    const unsigned char* code;
};
__device__ __forceinline__ MatLds matrix_stage(const MatArgs& a) {
    __shared__ unsigned s_tabw[2 * MAT_TAB_BYTES / 4];
    __shared__ unsigned s_codew[64];
    for (int i = threadIdx.x; i < 2 * MAT_TAB_BYTES / 4; i += 256) s_tabw[i] = a.tab[i];
    if (threadIdx.x < 64) s_codew[threadIdx.x] = a.code[threadIdx.x];
    __syncthreads();
    return MatLds{reinterpret_cast<const signed char*>(s_tabw), reinterpret_cast<const unsigned char*>(s_codew)};
}
// PROFILE: the byte-to-code map alone is staged; the table is the wave's slab in the dynamic LDS, W * 64 slots
// of MAT_STRIDE bytes a wave (MStrip above), which the launch sizes (profile_slab_bytes)
constexpr int profile_slab_bytes(int W) { return 4 * W * 64 * MAT_STRIDE; }
template <int W>
__device__ __forceinline__ MatLds profile_stage(const MatArgs& a) {
    __shared__ unsigned s_codew[64];
    extern __shared__ unsigned s_slabw[];
    if (threadIdx.x < 64) s_codew[threadIdx.x] = a.code[threadIdx.x];
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    return MatLds{reinterpret_cast<const signed char*>(s_slabw + wave * (W * 64 * MAT_STRIDE / 4)),
                  reinterpret_cast<const unsigned char*>(s_codew)};
}
// XLATE: the map, the table of seq1 across the lanes (a frame is never swapped onto them) and the two tables of
// the translation, 256 + 68 bytes more
struct XlLds {
    MatLds m;
    const unsigned char* base;
    const unsigned char* codon;
};
__device__ __forceinline__ XlLds xlate_stage(const MatArgs& a) {
    __shared__ unsigned s_tabw[MAT_TAB_BYTES / 4];
    __shared__ unsigned s_codew[64];
    __shared__ unsigned s_basew[64];
    __shared__ unsigned s_codonw[17];
    for (int i = threadIdx.x; i < MAT_TAB_BYTES / 4; i += 256) s_tabw[i] = a.tab[i];
    if (threadIdx.x < 64) s_codew[threadIdx.x] = a.code[threadIdx.x];
    const unsigned* xl = reinterpret_cast<const unsigned*>(a.prof);   // 64 + 17 dwords (fill_args)
    if (threadIdx.x >= 64 && threadIdx.x < 128) s_basew[threadIdx.x - 64] = xl[threadIdx.x - 64];
    if (threadIdx.x >= 128 && threadIdx.x < 128 + 17) s_codonw[threadIdx.x - 128] = xl[threadIdx.x - 64];
    __syncthreads();
    return XlLds{MatLds{reinterpret_cast<const signed char*>(s_tabw), reinterpret_cast<const unsigned char*>(s_codew)},
                 reinterpret_cast<const unsigned char*>(s_basew), reinterpret_cast<const unsigned char*>(s_codonw)};
}
// the wave's next item; false: none is left
__device__ __forceinline__ bool matrix_claim(const MatArgs& a, const int lane, unsigned& item) {
    item = 0;
    if (lane == 0) item = atomicAdd(&a.ctrl->next_item, 1u);
    item = __builtin_amdgcn_readfirstlane(item);
    return (int)item < a.npairs;
}
// the claimed item's pair, every field provably wave-uniform (buffer descriptors live in SGPRs);
// TRACE: its trace buffer too
template <bool TRACE>
__device__ __forceinline__ void matrix_claimed_pair(const MatArgs& a, const unsigned item, MatPair& pd, WalkPair& wp) {
    const MatPair raw = a.pairs[item];
    pd.col_off = uniform64(raw.col_off);
    pd.row_off = uniform64(raw.row_off);
    pd.n = __builtin_amdgcn_readfirstlane(raw.n);
    pd.m = __builtin_amdgcn_readfirstlane(raw.m);
    pd.out_idx = __builtin_amdgcn_readfirstlane(raw.out_idx);
    pd.swap_or_band = __builtin_amdgcn_readfirstlane(raw.swap_or_band);
    wp = WalkPair{};
    if constexpr (TRACE) {
        const WalkPair wraw = a.walk[item];
        wp.trace_off = uniform64(wraw.trace_off);
        wp.trace_bytes = __builtin_amdgcn_readfirstlane(wraw.trace_bytes);
        wp.steps = __builtin_amdgcn_readfirstlane(wraw.steps);
    }
}

// BAND: the pair's diagonal range beside it; seq1 is across the lanes (table 0) in local mode too.
// PROFILE: seq1 is the profile of the launch (MatArgs::prof), pd.n its length for every item.
// XLATE: seq2 is a reading frame of a DNA, translated by the fetch; the item's swap_or_band is 1 for a minus frame.
template <int W, bool TRACE = false, int AM = AM_LOCAL, bool BAND = false, bool PROFILE = false, bool XLATE = false>
__global__ void __launch_bounds__(256) sw_matrix_kernel(MatArgs a) {
    MatLds s;
    XlLds x{};
    if constexpr (XLATE) {
        x = xlate_stage(a);
        s = x.m;
    } else if constexpr (PROFILE) s = profile_stage<W>(a);
    else s = matrix_stage(a);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    uint2* scr = a.scratch + (uint64_t)wave * (uint64_t)a.scratch_rows;
    unsigned item;
    MatPair pd;
    WalkPair wp;
    while (matrix_claim(a, lane, item)) {
        matrix_claimed_pair<TRACE>(a, item, pd, wp);
        BandPair bp{0, 0};
        if constexpr (BAND) {
            bp = band_of(pd.n, pd.m, pd.swap_or_band);
            pd.swap_or_band = 0;
        }
        int minus = 0;
        if constexpr (XLATE) {
            minus = pd.swap_or_band;
            pd.swap_or_band = 0;
        }
        matrix_pair<W, TRACE ? M_TRACE : M_SCORE, AM, BAND, PROFILE, XLATE>(a, pd, wp, lane, scr, s.tab, s.code, nullptr, 0, bp,
                                                                            minus, x.base, x.codon);
    }
}

// THE WALK: one lane a pair, from the end cell in state H along the recorded decisions, the
// operations (0 M, 1 I, 2 D) written last first.  Priorities (include/algoGPU.h): in local mode a
// cell with H = 0 ends the walk before anything else; in H the diagonal, then E, then F; in E and F
// opening before extending (both already decided by the fill: the bits say which).  Every iteration
// writes one operation and there are at most n + m; every cell read is checked against the pair and
// its trace.  Nothing here waits for anything.
//
// Global and semi-global: no H = 0 stop (source 0 is unused, and an error if met); the walk leaves
// the matrix at j < 0 -- the remaining i + 1 residues of seq1 are one leading I run, the top border
// H[i][-1] -- or at i < 0: global, the remaining j + 1 residues of seq2 are one leading D run;
// semi-global, it stops there.  A gap is never extended out of a border (E[-1][j] and F[i][-1] are
// minus infinity, so the fill recorded an opening), hence the walk leaves in state H.  Every M uses
// a residue of both sequences, an I one of seq1, a D one of seq2: n + m bytes are still enough.
//
// Where cell (i, j) lives is the trace's layout, a compile-time parameter: cell() gives the dword and
// the shift of the cell's nibble, or false for a cell the trace does not hold; first_column() is the
// column below which the walk has left the trace (on its left side: the resumable walk of LONG PAIRS).
// [strip - strip0][step][lane] dwords (WalkPair above).  A whole pair: strip0 = 0; the one-strip buffer
// of a long pair: strip0 = that strip.
struct StripTrace {
    int strip0, steps;
    unsigned bytes;
    __device__ int first_column() const { return strip0 * (64 * TRACE_W); }
    __device__ bool cell(int i, int j, unsigned long long& dw, int& shift) const {
        const int cl = i & (64 * TRACE_W - 1);
        dw = ((unsigned long long)(unsigned)(i / (64 * TRACE_W) - strip0) * (unsigned)steps + (unsigned)(j + cl)) * 64u +
             (unsigned)(cl >> 3);
        shift = 4 * (cl & 7);
        return dw * 4u < bytes;
    }
};
// [strip][lane][step - band_trace_origin] dwords, `steps` a lane; a cell outside the band is not held.
// (The fill never sends the walk there: an absent neighbour offers minus infinity, or in local mode
// 0, which is the H = 0 stop.)
struct BandTrace {
    BandPair bp;
    int steps;
    unsigned bytes;
    __device__ int first_column() const { return 0; }
    __device__ bool cell(int i, int j, unsigned long long& dw, int& shift) const {
        const int cl = i & (64 * TRACE_W - 1), i0 = i - cl;
        const int st = j + cl - band_trace_origin(i0, cl >> 3, bp.dlo);
        if (j - i < bp.dlo || j - i > bp.dhi || st < 0 || st >= steps) return false;
        dw = ((unsigned long long)(i0 / (64 * TRACE_W)) * 64u + (unsigned)(cl >> 3)) * (unsigned)steps + (unsigned)st;
        shift = 4 * (cl & 7);
        return dw * 4u < bytes;
    }
};

struct Walk {
    int i, j, state;       // where the walk stands: the cell, and 0 H, 1 E, 2 F
    int nops, err, done;   // operations written so far, WALK_* error, 1: the walk has ended
};

// Walks on from w until the walk has ended (done: a cell with H = 0 in local mode, or the walk has
// left the matrix and the border run is written), failed (err) or left the trace on its left side.
// The only definition of the nibble decode, the state transition and the operation write.
template <class TRACE>
__device__ __forceinline__ void matrix_walk(const TRACE t, const unsigned char* trace, unsigned char* ops, const int n,
                                            const int m, const int amode, Walk& w) {
    int i = w.i, j = w.j, state = w.state, nops = w.nops, err = 0;
    bool h0 = false;   // the walk met a cell with H = 0 in state H
    const long long limit = (long long)n + m;
    const unsigned* tr = reinterpret_cast<const unsigned*>(trace);
    const int lo = t.first_column();
    if (i < 0 || i >= n || j < 0 || j >= m) err = WALK_RANGE;
    while (err == 0 && i >= 0 && j >= 0 && i >= lo) {
        unsigned long long dw;
        int shift;
        if (!t.cell(i, j, dw, shift)) {
            err = WALK_RANGE;
            break;
        }
        const unsigned nib = (tr[dw] >> shift) & 15u;
        if (state == 0) {
            const unsigned src = nib & 3u;
            if (src == 0) {
                h0 = true;
                break;
            }
            state = (int)src - 1;   // the diagonal: stays in H; E: 1, F: 2
        }
        if (nops >= limit) {
            err = WALK_OVERRUN;
            break;
        }
        ops[nops++] = (unsigned char)state;   // M, I, D: the state's own number
        i -= state != 2;                      // M and I use a residue of seq1,
        j -= state != 1;                      // M and D one of seq2
        state = (nib >> (state + 1)) & 1u ? state : 0;   // E: bit 2, F: bit 3 extend; H stays H
    }
    if (h0 && amode != SW_MODE_LOCAL) err = WALK_RANGE;   // source 0 is local's stop only
    const int done = err == 0 && (h0 || i < 0 || j < 0);
    if (amode != SW_MODE_LOCAL && done) {   // the border exits
        const bool lead_i = j < 0;
        const int run = lead_i ? i + 1 : (amode == SW_MODE_GLOBAL ? j + 1 : 0);
        if (nops + (long long)run > limit) {
            err = WALK_OVERRUN;
        } else {
            for (int k = 0; k < run; ++k) ops[nops++] = lead_i ? 1 : 2;
            if (lead_i) i = -1;
            else if (run > 0) j = -1;
        }
    }
    w = Walk{i, j, state, nops, err, done};
}

struct WalkArgs {
    const MatPair* pairs;
    const WalkPair* walk;
    const unsigned char* trace;
    unsigned char* ops;
    TraceRes* res;
    int npairs;
    int amode;   // SW_MODE_*
};

// The walk of a whole traced launch, every mode; BAND: of a band launch.  A local pair without an
// alignment (score 0) never walks.
template <bool BAND>
__global__ void __launch_bounds__(64) sw_matrix_walk_kernel(WalkArgs w) {
    const int item = (int)(blockIdx.x * 64 + threadIdx.x);
    if (item >= w.npairs) return;
    const MatPair pd = w.pairs[item];
    const WalkPair wp = w.walk[item];
    TraceRes* r = w.res + pd.out_idx;
    Walk s{r->ei, r->ej, 0, 0, 0, 0};
    if (w.amode != SW_MODE_LOCAL || r->score > 0) {
        const unsigned char* trace = w.trace + wp.trace_off;
        unsigned char* ops = w.ops + wp.ops_off;
        if constexpr (BAND)
            matrix_walk(BandTrace{band_of(pd.n, pd.m, pd.swap_or_band), wp.steps, wp.trace_bytes}, trace, ops, pd.n, pd.m,
                        w.amode, s);
        else
            matrix_walk(StripTrace{0, wp.steps, wp.trace_bytes}, trace, ops, pd.n, pd.m, w.amode, s);
    }
    r->bi = s.i + 1;
    r->bj = s.j + 1;
    r->nops = s.nops;
    r->err = s.err;
}

// ---- LONG PAIRS: checkpointed traceback, one strip at a time (sw_align_matrix_long) -----------
//
// The only state that crosses a strip boundary is the right-edge column.  The locate pass
// (matrix_pair<TRACE_W, M_LOCATE>) keeps every strip's column instead of overwriting one scratch
// column, and reports the end cell.  Any strip can then be filled again on its own from the column
// on its left with the traced step: the same recurrence on the same integers, so the same 4 bits a
// cell as the whole traced fill would have stored.  The walk needs one strip at a time, right to
// left: a round fills, for every pair still walking, the strip its walk stands in -- rows [0, j]
// only, j the row at which the walk enters the strip -- into a one-strip buffer (the layout above
// with strip index 0), and sw_matrix_walk_strip_kernel walks on through it, appending operations,
// until the walk ends or leaves the strip on the left.  The host runs the rounds (below).  As in the
// kernels above no wave waits for another and every loop is bounded: chunks of the strip, n + m
// operations.
//
// LONG PAIRS IN A MODE (sw_align_matrix_long_mode).  The three fill kernels of this path
// -- locate, strip fill and, further down, the cooperative locate -- are templates on AM as every other fill
// kernel is, and the two resumable walks take the mode at run time, as sw_matrix_walk_kernel does.  Global and
// semi-global: the end is read from column n - 1, so it lies in the last strip and there is no merge of strips;
// a strip is filled again under AM's borders; every pair walks, whatever its score; and a walk may end in any
// strip by leaving the matrix at j < 0, its leading I run covering the strips still to the left.

struct LongPair {           // locate: per item, beside its MatPair
    uint64_t ckpt_off;      // bytes, from LongArgs::ckpt: checkpoint column 0 of the pair
    unsigned ckpt_stride;   // bytes a column: align_ckpt_stride(m) (m * 8 of them used)
    unsigned pad;
};
struct StripItem {          // strip fill and walk: one strip of one pair
    uint64_t col_off, row_off;   // as MatPair (seq1 across the lanes)
    uint64_t ckpt_in;       // bytes, from LongArgs::ckpt: checkpoint column strip - 1 (strip > 0)
    uint64_t trace_off;     // bytes, from LongArgs::trace: the item's one-strip buffer
    uint64_t ops_off;       // bytes, from WalkStripArgs::ops: the pair's n + m operation bytes
    int n, m;               // the pair
    int strip;              // seq1 positions [512 * strip, 512 * strip + 512)
    int rows;               // j + 1: rows [0, j] are filled
    unsigned trace_bytes;   // of the item's buffer: at least align_strip_trace_bytes(rows)
    int slot;               // the pair's WalkState
};
struct WalkState : Walk {   // 32 B a pair, read by the host after every round
    int pad0, pad1;
};
static_assert(sizeof(WalkState) == 32, "walk state");
struct LongArgs {
    const LongPair* lp;         // locate
    unsigned char* ckpt;
    const StripItem* items;     // strip fill: MatArgs::npairs of them
    unsigned char* trace;
};

// The locate pass: sw_matrix_kernel<8, true, AM> without the trace, every strip's right edge kept.
// a.res[out_idx] receives score, ei, ej (the first half of a TraceRes).  AM != AM_LOCAL: matrix_pair's own
// mode code -- AM's setup(), the left border as strip 0's inflow, the strict end update on column n - 1 --
// so ei = n - 1, and there is no merge of strips: the end cell is in the last one.
template <int AM>
__global__ void __launch_bounds__(256) sw_matrix_locate_kernel(MatArgs a, LongArgs x) {
    const MatLds s = matrix_stage(a);
    const int lane = threadIdx.x & 63;
    unsigned item;
    MatPair pd;
    WalkPair wp;
    while (matrix_claim(a, lane, item)) {
        matrix_claimed_pair<false>(a, item, pd, wp);
        pd.swap_or_band = 0;   // seq1 across the lanes
        const LongPair lraw = x.lp[item];
        unsigned char* ckpt = x.ckpt + uniform64(lraw.ckpt_off);
        const unsigned stride = __builtin_amdgcn_readfirstlane(lraw.ckpt_stride);
        matrix_pair<TRACE_W, M_LOCATE, AM>(a, pd, wp, lane, nullptr, s.tab, s.code, ckpt, stride);
    }
}

// One strip of one pair, traced, rows [0, it.rows): inflow from the checkpoint column on its left
// (the border for strip 0), no outflow, no end cell.  Every store of a step is inside the item's
// buffer by construction (align_strip_trace_bytes(rows) <= trace_bytes); the resource drops
// whatever is not.
// AM != AM_LOCAL: AM's setup() builds the top border H[512 * strip][-1] from the strip index, strip 0 takes
// the left border H[-1][j] as its inflow chunk by chunk (as matrix_pair does), and the step's bookkeeping
// of column n - 1 runs on a pair of `rows` rows and is dropped: the locate pass has the end.
template <int AM>
__device__ void matrix_strip_fill(const MatArgs& a, const LongArgs& x, const StripItem& it, const int lane,
                                  const signed char* s_tab, const unsigned char* s_code) {
    constexpr int W = TRACE_W, SW = 64 * W, C = MAT_C;
    const int m = it.rows;
    const int go = a.gap_init, ge = a.gap_ext;
    const bool l63 = lane == 63;
    const bool has_in = it.strip > 0;
    MatPair pd;
    pd.col_off = it.col_off;
    pd.row_off = it.row_off;
    pd.n = it.n;
    pd.m = m;
    pd.out_idx = 0;
    pd.swap_or_band = 0;
    const __amdgpu_buffer_rsrc_t row_rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(a.seq + it.row_off), 0, m, RSRC_FLAGS);
    const __amdgpu_buffer_rsrc_t in_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        x.ckpt + (has_in ? it.ckpt_in : 0), 0, has_in ? (int)((unsigned)m * 8u) : 0, RSRC_FLAGS);
    const __amdgpu_buffer_rsrc_t trc =
        __builtin_amdgcn_make_buffer_rsrc(x.trace + it.trace_off, 0, (int)it.trace_bytes, RSRC_FLAGS);
    const int nchunks = (m + SW - 1 + C - 1) / C;
    unsigned toff = (unsigned)lane * 4u;
    MStrip<W, M_TRACE, AM> S;
    S.setup(a, pd, it.strip, lane, s_code);
    if constexpr (AM == AM_LOCAL) {
        S.M = 0;
        S.Mkp = 0;
        S.kp8 = 0;
    } else {
        S.M = MAT_NEG;
        S.Mj = 0;
    }
    unsigned raw_nxt = mat_fetch_raw(row_rsrc, 0, lane, m);
    u32x2 g_nxt = has_in ? mat_fetch_edge(in_rsrc, 0, lane, m) : u32x2{0u, 0u};
    for (int c = 0; c < nchunks; ++c) {
        const int k0 = c * C;
        const unsigned raw = raw_nxt;
        const u32x2 g = g_nxt;
        raw_nxt = mat_fetch_raw(row_rsrc, k0 + C, lane, m);
        if (has_in) g_nxt = mat_fetch_edge(in_rsrc, k0 + C, lane, m);
        const bool live = k0 + lane < m;
        S.IOR = live ? (int)s_code[raw & 0xFFu] : a.k;
        if constexpr (AM == AM_LOCAL) {
            S.IOH = has_in && live ? (int)g.x : -go;
            S.IOE = has_in && live ? (int)g.y : -ge;
        } else {   // strip 0: the left border H[-1][j], and no E to extend out of it
            const int lb = AM == AM_GLOBAL ? -(go + (k0 + lane) * min(go, ge)) - go : -go;
            S.IOH = has_in && live ? (int)g.x : lb;
            S.IOE = has_in && live ? (int)g.y : MAT_NEG;
        }
        S.run(l63, go, ge, s_tab, trc, toff);
    }
}

template <int AM>
__global__ void __launch_bounds__(256) sw_matrix_strip_kernel(MatArgs a, LongArgs x) {
    const MatLds s = matrix_stage(a);
    const int lane = threadIdx.x & 63;
    unsigned item;
    while (matrix_claim(a, lane, item)) {
        const StripItem raw = x.items[item];
        StripItem it{};   // every field used provably wave-uniform
        it.col_off = uniform64(raw.col_off);
        it.row_off = uniform64(raw.row_off);
        it.ckpt_in = uniform64(raw.ckpt_in);
        it.trace_off = uniform64(raw.trace_off);
        it.n = __builtin_amdgcn_readfirstlane(raw.n);
        it.strip = __builtin_amdgcn_readfirstlane(raw.strip);
        it.rows = __builtin_amdgcn_readfirstlane(raw.rows);
        it.trace_bytes = __builtin_amdgcn_readfirstlane(raw.trace_bytes);
        matrix_strip_fill<AM>(a, x, it, lane, s.tab, s.code);
    }
}

// The resumable walk: matrix_walk from the pair's WalkState, while the cell is in the item's strip;
// the cell at column i - 512 * strip of the one-strip buffer (StripTrace with strip0 = strip, so the
// steps of a strip multiply 0).  Operations are
// appended at the running offset nops.  done: a cell with H = 0 met in state H (local), or i < 0, or j < 0.
// Otherwise the walk left the strip through its left side, in state H (after an M) or E (after an
// I): the state the last cell's extend bit decided, exactly as inside a strip.
// amode != SW_MODE_LOCAL: done also says that the walk has left the matrix and matrix_walk has written the
// leading run and set i or j to -1.  A leading I run may cover every strip still to the left: it is
// i + 1 <= n operations into the pair's n + m bytes, and no further round reads a trace for it.
struct WalkStripArgs {
    const StripItem* items;
    const unsigned char* trace;
    unsigned char* ops;
    WalkState* st;
    int nitems;
    int amode;   // SW_MODE_*
};

__global__ void __launch_bounds__(64) sw_matrix_walk_strip_kernel(WalkStripArgs w) {
    const int item = (int)(blockIdx.x * 64 + threadIdx.x);
    if (item >= w.nitems) return;
    const StripItem it = w.items[item];
    WalkState* st = w.st + it.slot;
    Walk s = *st;
    if (s.done || s.err) return;
    const int lo = it.strip * (64 * TRACE_W);
    if (s.i < lo || s.i >= lo + 64 * TRACE_W || s.j >= it.rows || s.nops < 0 || s.state < 0 || s.state > 2)
        s.err = WALK_RANGE;   // (matrix_walk checks the cell against the pair)
    else
        matrix_walk(StripTrace{it.strip, 0, it.trace_bytes}, w.trace + it.trace_off, w.ops + it.ops_off, it.n, it.m,
                    w.amode, s);
    *static_cast<Walk*>(st) = s;
}

// ---- COOPERATIVE SCORE: the strips of one pair on as many waves (sw_score_matrix_batch_coop) -----
//
// DESIGN.md section 16.  A work item is one strip of one pair, numbered pair-major and strip-minor,
// and the waves claim items strictly in order (matrix_claim).  The wave that holds strip s stores its
// right edge to edge column s of the pair -- a column of its own, m rows of 8 bytes {H - G_INIT,
// E - G_EXT}, the layout of the locate pass's checkpoints -- and the wave that holds strip s + 1 reads
// that column as its inflow while strip s is still running.  A column is written once and read once in
// a launch and never reused.  One 32-bit progress word an item says how many rows of the item's
// right edge are stored: after the stores of a chunk the producer drains them (s_waitcnt vmcnt(0); the
// stores are sc1, write-through) and one lane publishes the count with an sc1 store (what a relaxed
// agent-scope atomic store is on gfx950: cdna_hip_programming.md Guideline 16, form R1); the consumer polls
// its left neighbour's word, relaxed, until the rows of its next fetch are covered, then fences
// (acquire, agent scope) and fetches.  The words are zeroed by the host before every launch.
// Score-only, no band; the step (MStrip) is the one of every other fill kernel.

struct CoopPair {           // per pair, beside its MatPair
    uint64_t edge_off;      // bytes, from CoopArgs::edge: edge column 0 of the pair
    unsigned stride;        // bytes a column: m * 8
    int strips;
};
struct CoopItem {
    int pair, strip;
};
struct CoopArgs {
    const CoopPair* cp;
    const CoopItem* items;      // MatArgs::npairs of them
    unsigned char* edge;
    unsigned* progress;         // a word an item: rows [0, r) of the item's right edge are stored
    long long timeout_ticks;    // s_memrealtime ticks (100 MHz) before a poll gives up
    AlignEnd* ends;             // the cooperative locate pass only (below): an end-cell record an item
};

// The slow path of the consumer's poll, out of line as await_slow (sw_device.h) and for its reason.
// Polls the word at byte woff of the progress block until it is at least `need`: the rows published,
// or -1 when the launch has failed -- another wave's poll has given up (Ctrl::error is set), or this
// one's deadline has passed (it sets ERR_TIMEOUT and the item; every lane adds the same bits, so no
// branch on the lane).  Relaxed sc1 loads, a sleep between polls.
__device__ __noinline__ int coop_await(__amdgpu_buffer_rsrc_t prog_rsrc, __amdgpu_buffer_rsrc_t ctrl_rsrc, const unsigned woff,
                                       const unsigned need, const long long timeout_ticks, Ctrl* ctrl, const unsigned item) {
    SpinDeadline dl((long long)__builtin_amdgcn_s_memrealtime(), timeout_ticks);
    for (;;) {
        __builtin_amdgcn_s_sleep(SW_SPIN_SLEEP);
        const unsigned r = __builtin_amdgcn_readfirstlane(__builtin_amdgcn_raw_buffer_load_b32(prog_rsrc, woff, 0, AUX_SC1));
        if (r >= need) return (int)r;
        const unsigned e = __builtin_amdgcn_readfirstlane(
            __builtin_amdgcn_raw_buffer_load_b32(ctrl_rsrc, (unsigned)offsetof(Ctrl, error), 0, AUX_SC1));
        if (e != 0) return -1;
        if (dl.expired()) {
            atomicOr(&ctrl->error, ERR_TIMEOUT);
            atomicMax(&ctrl->err_item, item);
            return -1;
        }
    }
}

// One strip of one pair.  false: the launch has failed (coop_await) and the wave leaves.
// MODE: M_SCORE, the score path; M_LOCATE (W = TRACE_W, seq1 across the lanes), the cooperative
// locate pass of LONG PAIRS ON MANY WAVES below: the same consumer and producer on the pair's checkpoint
// columns, the end-cell bookkeeping of matrix_pair for this one strip, and an end-cell record an item
// instead of the atomicMax.  The score instantiations are the code they were.
// M_LOCATE in a mode (AM != AM_LOCAL): only the last strip holds column n - 1, so only its item has an end:
// it reduces (M, Mj) over its lanes as matrix_pair does and stores {score, n - 1, ej} as its record; every
// other item's store is out of range, and the host reads the last strip's record (align_mode_end).
template <int W, int AM, int MODE = M_SCORE>
__device__ __forceinline__ bool matrix_coop_strip(const MatArgs& a, const CoopArgs& x, const MatPair& pd, const CoopPair& cp,
                                                  const unsigned item, const int strip, const int lane,
                                                  const signed char* s_tab, const unsigned char* s_code) {
    constexpr int SW = 64 * W, C = MAT_C;
    const int m = pd.m;
    const int go = a.gap_init, ge = a.gap_ext;
    const bool l63 = lane == 63;
    const bool has_in = strip > 0;
    const bool has_out = strip < cp.strips - 1;
    const __amdgpu_buffer_rsrc_t row_rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(a.seq + pd.row_off), 0, m, RSRC_FLAGS);
    // a column that is not there (strip 0's left, the last strip's right) has no bytes
    unsigned char* col0 = x.edge + cp.edge_off;
    const __amdgpu_buffer_rsrc_t in_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        col0 + (uint64_t)(has_in ? strip - 1 : 0) * cp.stride, 0, has_in ? (int)((unsigned)m * 8u) : 0, RSRC_FLAGS);
    const __amdgpu_buffer_rsrc_t out_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        col0 + (uint64_t)(has_out ? strip : 0) * cp.stride, 0, has_out ? (int)((unsigned)m * 8u) : 0, RSRC_FLAGS);
    const __amdgpu_buffer_rsrc_t prog_rsrc =
        __builtin_amdgcn_make_buffer_rsrc(x.progress, 0, (int)((unsigned)a.npairs * 4u), RSRC_FLAGS);
    const __amdgpu_buffer_rsrc_t ctrl_rsrc = __builtin_amdgcn_make_buffer_rsrc(a.ctrl, 0, (int)sizeof(Ctrl), RSRC_FLAGS);
    const int nchunks = (m + SW - 1 + C - 1) / C;
    unsigned toff = 0;
    MStrip<W, MODE, AM> S;
    S.M = AM == AM_LOCAL ? 0 : MAT_NEG;
    S.setup(a, pd, strip, lane, s_code);
    if constexpr (MODE == M_LOCATE) {   // as matrix_pair starts every strip
        S.Mkp = 0;
        S.kp8 = 0;
        if constexpr (AM != AM_LOCAL) S.Mj = 0;
    }
    // THE CONSUMER.  `seen` rows of the left edge are known to be stored (strip 0 has no left edge).
    // Before the fetch of rows [k, k + 64) the word of item - 1 -- strip - 1 of this pair: items are
    // pair-major, strip-minor -- must have reached min(m, k + 64).  A poll that has matched is followed
    // by one agent-scope acquire: the edge loads are sc1, past the CU's cache, but each producing
    // wave signals for itself, several workgroups share a CU and the loads are 8-B buffer loads, which
    // is no row of the table of forms measured without the acquire, so it stays.
    int seen = has_in ? 0 : m;
    auto await_rows = [&](const int k) __attribute__((always_inline)) -> bool {
        const int need = min(m, k + C);
        if (seen >= need) return true;
        const unsigned woff = (item - 1u) * 4u;
        int r = (int)__builtin_amdgcn_readfirstlane(__builtin_amdgcn_raw_buffer_load_b32(prog_rsrc, woff, 0, AUX_SC1));
        if (r < need)   // (a call's result arrives in a vector register: made uniform again)
            r = __builtin_amdgcn_readfirstlane(coop_await(prog_rsrc, ctrl_rsrc, woff, (unsigned)need, x.timeout_ticks, a.ctrl, item));
        if (r < 0) return false;
        seen = r;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        return true;
    };
    if (!await_rows(0)) return false;
    unsigned raw_nxt = mat_fetch_raw(row_rsrc, 0, lane, m);
    u32x2 g_nxt = has_in ? mat_fetch_edge(in_rsrc, 0, lane, m) : u32x2{0u, 0u};
    for (int c = 0; c < nchunks; ++c) {
        const int k0 = c * C;
        const unsigned raw = raw_nxt;
        const u32x2 g = g_nxt;
        // the next chunk's rows in flight while this chunk computes
        if (k0 + C < m && !await_rows(k0 + C)) return false;
        raw_nxt = mat_fetch_raw(row_rsrc, k0 + C, lane, m);
        if (has_in) g_nxt = mat_fetch_edge(in_rsrc, k0 + C, lane, m);
        const bool live = k0 + lane < m;
        S.IOR = live ? (int)s_code[raw & 0xFFu] : a.k;
        if constexpr (AM == AM_LOCAL) {
            S.IOH = has_in && live ? (int)g.x : -go;
            S.IOE = has_in && live ? (int)g.y : -ge;
        } else {   // strip 0: the left border H[-1][j], and no E to extend out of it
            const int lb = AM == AM_GLOBAL ? -(go + (k0 + lane) * min(go, ge)) - go : -go;
            S.IOH = has_in && live ? (int)g.x : lb;
            S.IOE = has_in && live ? (int)g.y : MAT_NEG;
        }
        S.run(l63, go, ge, s_tab, row_rsrc, toff);
        // THE PRODUCER.  Lane l holds the right edge of row k0 + l - (SW - 1): after this chunk's
        // stores rows [0, k0 + 65 - SW) are stored, all m of them after the last chunk (k0 + 64 >=
        // m + SW - 1 there).  The count is published once the stores have left the wave's queue, by
        // lane 0 through a store that is out of range on every other lane (no branch on the lane:
        // the comment at matrix_pair's score store).
        const int pub = min(m, k0 + C + 1 - SW);
        if (has_out && pub > 0) {
            const int row_out = k0 + lane - (SW - 1);
            const bool st = row_out >= 0 && row_out < m;
            __builtin_amdgcn_raw_buffer_store_b64(u32x2{(unsigned)S.IOH, (unsigned)S.IOE}, out_rsrc,
                                                  st ? (unsigned)row_out * 8u : OOR, 0, AUX_SC1);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_raw_buffer_store_b32((unsigned)pub, prog_rsrc, lane == 0 ? item * 4u : OOR, 0, AUX_SC1);
        }
    }
    if constexpr (MODE == M_LOCATE && AM != AM_LOCAL) {   // one lane of the last strip holds the end; M is H - G_INIT
        int M = S.M, J = S.Mj;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const int oM = __shfl_xor(M, off), oJ = __shfl_xor(J, off);
            J = oM > M ? oJ : J;
            M = max(M, oM);
        }
        // lane 0's store without a branch on the lane (the comment at matrix_pair's score store)
        const int jlo = AM == AM_GLOBAL ? m - 1 : 0;
        const __amdgpu_buffer_rsrc_t end_rsrc =
            __builtin_amdgcn_make_buffer_rsrc(x.ends, 0, (int)((unsigned)a.npairs * (unsigned)sizeof(AlignEnd)), RSRC_FLAGS);
        __builtin_amdgcn_raw_buffer_store_b128(u32x4{(unsigned)(M + go), (unsigned)(pd.n - 1), (unsigned)(J + jlo), 0u}, end_rsrc,
                                               lane == 0 && !has_out ? item * (unsigned)sizeof(AlignEnd) : OOR, 0, 0);
        return true;
    }
    if constexpr (MODE == M_LOCATE) {
        // The item's end cell: the lane's cell of this strip (column lane * W + p, reached at step k), the
        // lanes merged by the three-key rule at the end of matrix_pair: the largest t, then the smallest
        // i + j, then the smallest j.  The host merges a pair's records by the same rule (align_merge_ends),
        // so no wave writes where another does: no atomics.  (t = 0: no cell, and d and j mean nothing.)
        const int k = S.Mkp >> 3, cl = lane * W + (S.Mkp & 7);
        int bM = S.M, bD = strip * SW + k, bJ = k - cl;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const int oM = __shfl_xor(bM, off), oD = __shfl_xor(bD, off), oJ = __shfl_xor(bJ, off);
            const bool better = oM > bM || (oM == bM && (oD < bD || (oD == bD && oJ < bJ)));
            bM = better ? oM : bM;
            bD = better ? oD : bD;
            bJ = better ? oJ : bJ;
        }
        // lane 0's store without a branch on the lane (the comment at matrix_pair's score store)
        const __amdgpu_buffer_rsrc_t end_rsrc =
            __builtin_amdgcn_make_buffer_rsrc(x.ends, 0, (int)((unsigned)a.npairs * (unsigned)sizeof(AlignEnd)), RSRC_FLAGS);
        __builtin_amdgcn_raw_buffer_store_b128(u32x4{(unsigned)bM, (unsigned)bD, (unsigned)bJ, 0u}, end_rsrc,
                                               lane == 0 ? item * (unsigned)sizeof(AlignEnd) : OOR, 0, 0);
        return true;
    }
    int M = S.M;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) M = max(M, __shfl_xor(M, off));
    if constexpr (AM == AM_LOCAL) {
        // every strip's maximum into the pair's score word, which the host has zeroed; every lane
        // offers the same value (no branch on the lane)
        atomicMax(a.scores + pd.out_idx, M);
    } else {   // the last strip alone holds the end cell / the last column; M is H - G_INIT
        const __amdgpu_buffer_rsrc_t sc_rsrc =
            __builtin_amdgcn_make_buffer_rsrc(a.scores, 0, (int)((unsigned)a.nscores * 4u), RSRC_FLAGS);
        __builtin_amdgcn_raw_buffer_store_b32(M + go, sc_rsrc, lane == 0 && !has_out ? (unsigned)pd.out_idx * 4u : OOR, 0, 0);
    }
    return true;
}

// PROGRESS, for any grid.  Claim: every claimed item finishes or the launch fails within the poll's
// deadline.  Items are claimed in order from one counter, and a wave claims its next item only after
// finishing the one it holds.  Item i = (pair, strip s) waits only for item i - 1 = (pair, s - 1),
// and only if s > 0.  Item i - 1 was claimed before item i, so by a wave that is already running: it
// holds i - 1 now or has finished it.  By induction over i, item i - 1 finishes (strip 0, and item 0,
// wait for nothing), publishing all m rows on the way, so every poll of item i is answered.  Nothing
// here asks two waves to be resident together, a dispatch order or a placement: a grid of one
// workgroup works through 20 strips four at a time.
template <int W, int AM>
__global__ void __launch_bounds__(256) sw_matrix_coop_kernel(MatArgs a, CoopArgs x) {
    const MatLds s = matrix_stage(a);
    const int lane = threadIdx.x & 63;
    unsigned item;
    MatPair pd;
    WalkPair wp;
    while (matrix_claim(a, lane, item)) {
        const CoopItem iraw = x.items[item];
        const int pair = __builtin_amdgcn_readfirstlane(iraw.pair);
        const int strip = __builtin_amdgcn_readfirstlane(iraw.strip);
        matrix_claimed_pair<false>(a, (unsigned)pair, pd, wp);
        const CoopPair craw = x.cp[pair];
        CoopPair cp;
        cp.edge_off = uniform64(craw.edge_off);
        cp.stride = __builtin_amdgcn_readfirstlane(craw.stride);
        cp.strips = __builtin_amdgcn_readfirstlane(craw.strips);
        if (!matrix_coop_strip<W, AM>(a, x, pd, cp, item, strip, lane, s.tab, s.code)) return;
    }
}

// ---- LONG PAIRS ON MANY WAVES: a cooperative locate pass, and rounds that trace a window of strips
// (sw_align_matrix_long_coop) -----
//
// The cooperative kernel's edge columns are the locate pass's checkpoint columns byte for byte: m rows of
// 8 bytes {H - G_INIT, E - G_EXT}, a column a strip.  So the locate pass of a long pair is the kernel above
// at W = 8 with seq1 across the lanes, MStrip<TRACE_W, M_LOCATE> for the step, column `strip` of the pair's
// checkpoints (CoopPair::edge_off from CoopArgs::edge, CoopPair::stride = align_ckpt_stride(m)) for the
// edge, and an end-cell record an item.  The hand-off and the progress argument are the ones above,
// unchanged: items are claimed in the same order and an item waits for the same one item.  It writes
// exactly what sw_matrix_locate_kernel writes, so sw_matrix_strip_kernel reads it as it is.
// In a mode (AM != AM_LOCAL) the progress argument above holds word for word: the claim order, the one item
// an item waits for, what it polls and what it publishes are the shared code, and none of them depends on
// AM.  What AM changes is the arithmetic of a step and which item stores an end record.
template <int AM>
__global__ void __launch_bounds__(256) sw_matrix_locate_coop_kernel(MatArgs a, CoopArgs x) {
    const MatLds s = matrix_stage(a);
    const int lane = threadIdx.x & 63;
    unsigned item;
    MatPair pd;
    WalkPair wp;
    while (matrix_claim(a, lane, item)) {
        const CoopItem iraw = x.items[item];
        const int pair = __builtin_amdgcn_readfirstlane(iraw.pair);
        const int strip = __builtin_amdgcn_readfirstlane(iraw.strip);
        matrix_claimed_pair<false>(a, (unsigned)pair, pd, wp);
        pd.swap_or_band = 0;   // seq1 across the lanes
        const CoopPair craw = x.cp[pair];
        CoopPair cp;
        cp.edge_off = uniform64(craw.edge_off);
        cp.stride = __builtin_amdgcn_readfirstlane(craw.stride);
        cp.strips = __builtin_amdgcn_readfirstlane(craw.strips);
        if (!matrix_coop_strip<TRACE_W, AM, M_LOCATE>(a, x, pd, cp, item, strip, lane, s.tab, s.code)) return;
    }
}

// The strip fills of a pair do not depend on one another: each reads only the checkpoint on its left.  The
// walk's j never grows as it moves left, so the row j at which it enters strip s bounds the rows of every
// strip further left, and a round may fill a WINDOW of G consecutive strips [s - G + 1, s] of a pair, all
// over rows [0, j], as G items of sw_matrix_strip_kernel on G waves.  Their one-strip buffers, `steps`
// steps each, lie end to end, which is StripTrace's [strip - strip0][step][lane] with strip0 = s - G + 1:
// matrix_walk crosses the strip boundaries inside the window as it does in a whole trace.
struct WindowItem {
    uint64_t trace_off;     // bytes, from WalkWindowArgs::trace: the buffer of the window's first strip
    uint64_t ops_off;       // bytes, from WalkWindowArgs::ops: the pair's n + m operation bytes
    int n, m;               // the pair
    int strip0, nstrips;    // seq1 positions [512 * strip0, 512 * (strip0 + nstrips))
    int steps;              // of every one-strip buffer of the window
    int rows;               // j + 1: rows [0, j] are filled
    unsigned trace_bytes;   // of the whole window: nstrips * steps * 256
    int slot;               // the pair's WalkState
};
struct WalkWindowArgs {
    const WindowItem* items;
    const unsigned char* trace;
    unsigned char* ops;
    WalkState* st;
    int nitems;
    int amode;   // SW_MODE_*
};

// sw_matrix_walk_strip_kernel for a window; a window of one strip walks what that kernel walks.
__global__ void __launch_bounds__(64) sw_matrix_walk_window_kernel(WalkWindowArgs w) {
    const int item = (int)(blockIdx.x * 64 + threadIdx.x);
    if (item >= w.nitems) return;
    const WindowItem it = w.items[item];
    WalkState* st = w.st + it.slot;
    Walk s = *st;
    if (s.done || s.err) return;
    const long long lo = (long long)it.strip0 * (64 * TRACE_W), hi = lo + (long long)it.nstrips * (64 * TRACE_W);
    if (s.i < lo || s.i >= hi || s.j >= it.rows || s.nops < 0 || s.state < 0 || s.state > 2 || it.nstrips < 1)
        s.err = WALK_RANGE;   // (matrix_walk checks the cell against the pair and the window's bytes)
    else
        matrix_walk(StripTrace{it.strip0, it.steps, it.trace_bytes}, w.trace + it.trace_off, w.ops + it.ops_off, it.n, it.m,
                    w.amode, s);
    *static_cast<Walk*>(st) = s;
}

// ---- host ------------------------------------------------------------------------------------

#define MCHK(expr)                                                                          \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) {                                                              \
            char m_[256];                                                                    \
            std::snprintf(m_, sizeof m_, "%s failed: %s", #expr, hipGetErrorString(e_));     \
            report_error(m_);                                                                \
            return -1;                                                                       \
        }                                                                                    \
    } while (0)

// A fill kernel and, once a launch has asked, its resident workgroups per CU.  One launch is one
// kernel: the run-time choice among the compiled ones is an index into MatCtx::fill.
struct FillKernel {
    const void* fn = nullptr;
    int wgs = 0;
    int dyn = 0;   // dynamic LDS bytes of a workgroup (the profile kernels' slabs): they count in wgs
};
constexpr int W_OF[4] = {1, 2, 4, 8};
constexpr int WI_TRACED = 4;   // a row of the table: the score-only kernels at W_OF, then the traced one
template <int AM, bool BAND>
void name_fill_kernels(FillKernel (&row)[5]) {
    row[0].fn = (const void*)sw_matrix_kernel<1, false, AM, BAND>;
    row[1].fn = (const void*)sw_matrix_kernel<2, false, AM, BAND>;
    row[2].fn = (const void*)sw_matrix_kernel<4, false, AM, BAND>;
    row[3].fn = (const void*)sw_matrix_kernel<8, false, AM, BAND>;
    row[WI_TRACED].fn = (const void*)sw_matrix_kernel<TRACE_W, true, AM, BAND>;
}

template <int AM>
void name_profile_kernels(FillKernel (&row)[5]) {   // as name_fill_kernels; a workgroup's slabs are dynamic LDS
    row[0].fn = (const void*)sw_matrix_kernel<1, false, AM, false, true>;
    row[1].fn = (const void*)sw_matrix_kernel<2, false, AM, false, true>;
    row[2].fn = (const void*)sw_matrix_kernel<4, false, AM, false, true>;
    row[3].fn = (const void*)sw_matrix_kernel<8, false, AM, false, true>;
    row[WI_TRACED].fn = (const void*)sw_matrix_kernel<TRACE_W, true, AM, false, true>;
    for (int k = 0; k < 5; ++k) row[k].dyn = profile_slab_bytes(k == WI_TRACED ? TRACE_W : W_OF[k]);
}

template <int AM>
void name_xlate_kernels(FillKernel (&row)[5]) {   // as name_fill_kernels: the translated kernels
    row[0].fn = (const void*)sw_matrix_kernel<1, false, AM, false, false, true>;
    row[1].fn = (const void*)sw_matrix_kernel<2, false, AM, false, false, true>;
    row[2].fn = (const void*)sw_matrix_kernel<4, false, AM, false, false, true>;
    row[3].fn = (const void*)sw_matrix_kernel<8, false, AM, false, false, true>;
    row[WI_TRACED].fn = (const void*)sw_matrix_kernel<TRACE_W, true, AM, false, false, true>;
}

template <int AM>
void name_coop_kernels(FillKernel (&row)[4]) {   // the cooperative score kernels at W_OF
    row[0].fn = (const void*)sw_matrix_coop_kernel<1, AM>;
    row[1].fn = (const void*)sw_matrix_coop_kernel<2, AM>;
    row[2].fn = (const void*)sw_matrix_coop_kernel<4, AM>;
    row[3].fn = (const void*)sw_matrix_coop_kernel<8, AM>;
}

template <int AM>
void name_long_kernels(FillKernel& locate, FillKernel& locate_coop, FillKernel& strip) {   // the long path's fills
    locate.fn = (const void*)sw_matrix_locate_kernel<AM>;
    locate_coop.fn = (const void*)sw_matrix_locate_coop_kernel<AM>;
    strip.fn = (const void*)sw_matrix_strip_kernel<AM>;
}

// device memory and a stream per (thread, device), as the engine's own context (sw_engine.hip)
enum {
    B_PAIRS = 0, B_CTRL, B_SCRATCH, B_ARENA, B_SCORES,   // every launch
    B_WALK, B_TRACE, B_RES, B_OPS,                       // traced launches: walk pairs, trace, results, operations
    B_LONG, B_CKPT, B_ITEMS, B_STATE,                    // long pairs: locate items, checkpoints, strip items, walk states
    B_CPAIRS, B_CITEMS, B_EDGE, B_PROGRESS,              // cooperative score: pairs, items, edge columns, progress words
    B_ENDS, B_WINDOWS,                                   // long pairs on many waves: end-cell records, a round's windows
    B_PROFILE,                                           // profile launches: the profile's device image; translated: the tables
    B_COUNT
};
struct MatCtx {
    int cus = 256;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr;
    void* buf[B_COUNT] = {};
    size_t cap[B_COUNT] = {};
    FillKernel fill[2][3][5];   // [band][SW_MODE_*][index into W_OF, or WI_TRACED]
    FillKernel locate[3], strip[3];   // [SW_MODE_*]: the long path
    FillKernel coop[3][4];      // [SW_MODE_*][index into W_OF]
    FillKernel locate_coop[3];  // [SW_MODE_*]
    FillKernel pfill[3][5];     // [SW_MODE_*][index into W_OF, or WI_TRACED]: the profile kernels
    FillKernel xfill[3][5];     // [SW_MODE_*][index into W_OF, or WI_TRACED]: the translated kernels
    MatCtx() {
        name_profile_kernels<AM_LOCAL>(pfill[AM_LOCAL]);
        name_profile_kernels<AM_GLOBAL>(pfill[AM_GLOBAL]);
        name_profile_kernels<AM_SEMI>(pfill[AM_SEMI]);
        name_long_kernels<AM_LOCAL>(locate[AM_LOCAL], locate_coop[AM_LOCAL], strip[AM_LOCAL]);
        name_long_kernels<AM_GLOBAL>(locate[AM_GLOBAL], locate_coop[AM_GLOBAL], strip[AM_GLOBAL]);
        name_long_kernels<AM_SEMI>(locate[AM_SEMI], locate_coop[AM_SEMI], strip[AM_SEMI]);
        name_coop_kernels<AM_LOCAL>(coop[AM_LOCAL]);
        name_coop_kernels<AM_GLOBAL>(coop[AM_GLOBAL]);
        name_coop_kernels<AM_SEMI>(coop[AM_SEMI]);
        name_fill_kernels<AM_LOCAL, false>(fill[0][AM_LOCAL]);
        name_fill_kernels<AM_GLOBAL, false>(fill[0][AM_GLOBAL]);
        name_fill_kernels<AM_SEMI, false>(fill[0][AM_SEMI]);
        name_fill_kernels<AM_LOCAL, true>(fill[1][AM_LOCAL]);
        name_fill_kernels<AM_GLOBAL, true>(fill[1][AM_GLOBAL]);
        name_fill_kernels<AM_SEMI, true>(fill[1][AM_SEMI]);
        name_xlate_kernels<AM_LOCAL>(xfill[AM_LOCAL]);
        name_xlate_kernels<AM_GLOBAL>(xfill[AM_GLOBAL]);
        name_xlate_kernels<AM_SEMI>(xfill[AM_SEMI]);
    }
};
thread_local float t_fill_ms = 0.f, t_walk_ms = 0.f;   // sw_last_align_ms
thread_local float t_locate_ms = 0.f;                  // sw_last_align_long_ms: the locate launches' share of t_fill_ms
thread_local int t_rounds = 0;                         // and the rounds, summed over the call's groups
thread_local std::map<int, MatCtx*> t_mctx;

MatCtx* get_mctx() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) {
        report_error("hipGetDevice failed: no HIP device");
        return nullptr;
    }
    auto it = t_mctx.find(dev);
    if (it != t_mctx.end()) return it->second;
    MatCtx* c = new MatCtx();
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess ||
        hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess ||
        hipEventCreate(&c->ev2) != hipSuccess) {
        report_error("matrix scoring: device properties / stream / event creation failed");
        delete c;
        return nullptr;
    }
    c->cus = prop.multiProcessorCount;
    t_mctx[dev] = c;
    return c;
}

int ensure(MatCtx* c, int which, size_t bytes) {
    if (c->buf[which] && bytes <= c->cap[which]) return 0;
    if (c->buf[which]) {
        MCHK(hipStreamSynchronize(c->stream));
        MCHK(hipFree(c->buf[which]));
        c->buf[which] = nullptr;
        c->cap[which] = 0;
    }
    const size_t want = std::max<size_t>(bytes + bytes / 4, 256);
    MCHK(hipMalloc(&c->buf[which], want));
    c->cap[which] = want;
    return 0;
}

// steps of one pair at W columns per lane with n columns, times an issue-slot estimate of a step
// (about 9 instructions a cell and 8 a step for the DPP moves and the I/O rotation)
long long pair_cost(long long n, long long m, int W) {
    const long long SW = 64LL * W;
    const long long strips = (n + SW - 1) / SW;
    const long long chunks = (m + SW - 1 + MAT_C - 1) / MAT_C;
    return strips * chunks * MAT_C * (9LL * W + 8);
}
// the same for a band: the steps its strips run (about width + 2 * 64 * W each), and 5 more
// instructions a cell and a step for the mask
long long band_pair_cost(long long n, long long m, int dlo, int dhi, int W) {
    long long mx = 0;
    return band_steps(n, m, dlo, dhi, W, &mx) * (14LL * W + 13);
}

bool gaps_ok(int gap_init, int gap_ext) {
    if (gap_init < 0 || gap_ext < 0 || gap_init > (1 << 20) || gap_ext > (1 << 20)) {
        char m[128];
        std::snprintf(m, sizeof m, "unsupported gap penalties (%d, %d): need 0 <= G_INIT, G_EXT <= 2^20", gap_init, gap_ext);
        report_error(m);
        return false;
    }
    return true;
}

struct DevSeq {
    int64_t a_off, b_off;
    int alen, blen, idx;
    int minus = 0;   // translated launches: b is the 3 * blen bases of a reading frame, and this a minus frame
};

// the byte-to-code map and both orientations of the table, as the kernel stages them in LDS
void stage_matrix(MatArgs& a, const sw_matrix* mx) {
    a.k = mx->k;
    std::memcpy(a.code, mx->code, 256);
    signed char tab[2 * MAT_TAB_BYTES];
    std::memset(tab, 0, sizeof tab);
    for (int o = 0; o < 2; ++o)
        for (int i = 0; i <= mx->k; ++i) {
            signed char* row = tab + o * MAT_TAB_BYTES + i * MAT_STRIDE;
            for (int j = 0; j < mx->k && i < mx->k; ++j) row[j] = o == 0 ? mx->sc[i * mx->k + j] : mx->sc[j * mx->k + i];
            row[mx->k] = (signed char)MAT_SENT;
        }
    std::memcpy(a.tab, tab, sizeof tab);
}

// ---- the steps every fill launch takes (launch, launch_traced, long_group) ----

// longest first: the waves claim in order.  launch sorts its pairs themselves (a search launches
// every record of a database); the traced launches, whose results go back by slot, sort indices.
struct Longer {
    bool operator()(const DevSeq& x, const DevSeq& y) const { return (long long)x.alen * x.blen > (long long)y.alen * y.blen; }
};
std::vector<int> longest_first(const std::vector<DevSeq>& act) {
    std::vector<int> order(act.size());
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return Longer()(act[(size_t)x], act[(size_t)y]); });
    return order;
}

// trace bytes of one pair: strips * steps * 256 (WalkPair)
long long trace_steps(long long m) { return (m + 64 * TRACE_W - 1 + MAT_C - 1) / MAT_C * MAT_C; }
long long trace_bytes(long long n, long long m) { return (n + 64 * TRACE_W - 1) / (64 * TRACE_W) * trace_steps(m) * 256; }

// The pair as the kernels take it; its result goes to slot out_idx.  swap: seq2 across the lanes.
// band >= 0: a band launch, which never swaps and carries the pair's B.  w (traced launches): the
// trace the pair holds, the whole matrix or the band; the offsets are the caller's.
MatPair make_pair(const DevSeq& p, int out_idx, bool swap, int band, WalkPair* w = nullptr) {
    MatPair d;
    d.col_off = (uint64_t)(swap ? p.b_off : p.a_off);
    d.row_off = (uint64_t)(swap ? p.a_off : p.b_off);
    d.n = swap ? p.blen : p.alen;
    d.m = swap ? p.alen : p.blen;
    d.out_idx = out_idx;
    d.swap_or_band = band >= 0 ? std::min(band, std::max(d.n, d.m)) : swap ? 1 : 0;
    if (w && band >= 0) {
        int dlo, dhi;
        band_range(d.n, d.m, band, &dlo, &dhi);
        w->trace_bytes = (unsigned)band_trace_bytes(d.n, d.m, dlo, dhi);
        w->steps = (int)band_trace_steps(d.m, dlo, dhi);
    } else if (w) {
        w->trace_bytes = (unsigned)trace_bytes(d.n, d.m);
        w->steps = (int)trace_steps(d.m);
    }
    return d;
}

// Workgroups of a claim-loop launch over `items` items: the resident ones (option "blocks" instead),
// no more than a wave an item, and, where every wave holds a scratch column of scratch_rows entries,
// at most 1 GiB of scratch in all.
int fill_blocks(MatCtx* c, FillKernel& k, size_t items, long long scratch_rows, long long* out) {
    if (k.wgs == 0) {
        int nb = 0;
        if (k.dyn > 64 * 1024) MCHK(raise_dyn_lds(k.fn, k.dyn));   // past the default limit of a launch's dynamic LDS
        MCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k.fn, 256, (size_t)k.dyn));
        k.wgs = std::max(1, std::min(nb, 8));
    }
    long long blocks = sw_get_option("blocks");
    if (blocks <= 0) blocks = (long long)c->cus * k.wgs;
    blocks = std::max<long long>(1, std::min<long long>(blocks, ((long long)items + 3) / 4));
    if (scratch_rows > 0) blocks = std::max<long long>(1, std::min<long long>(blocks, (1LL << 30) / (scratch_rows * 8 * 4)));
    *out = blocks;
    return 0;
}

// The pairs uploaded, the claim counter zeroed, the scratch sized (a right-edge column of scratch_rows
// entries per wave of `blocks` workgroups), and the MatArgs fields every fill kernel reads.  long_group
// passes scratch_rows = 0; its kernels never touch the scratch pointer, whatever it holds.
// pf: a profile launch: mx is its alphabet, and its image goes up into a buffer of its own.
int fill_args(MatCtx* c, const sw_matrix* mx, const unsigned char* d_arena, const std::vector<MatPair>& pairs, int nscores,
              int gap_init, int gap_ext, long long scratch_rows, long long blocks, MatArgs& a, const sw_profile* pf = nullptr,
              const Translated* xl = nullptr) {
    if (ensure(c, B_PAIRS, pairs.size() * sizeof(MatPair)) || ensure(c, B_CTRL, sizeof(Ctrl)) ||
        ensure(c, B_SCRATCH, (size_t)scratch_rows * 8 * 4 * (size_t)blocks))
        return -1;
    MCHK(hipMemcpyAsync(c->buf[B_PAIRS], pairs.data(), pairs.size() * sizeof(MatPair), hipMemcpyHostToDevice, c->stream));
    MCHK(hipMemsetAsync(c->buf[B_CTRL], 0, sizeof(Ctrl), c->stream));
    a.seq = d_arena;
    a.pairs = (const MatPair*)c->buf[B_PAIRS];
    a.ctrl = (Ctrl*)c->buf[B_CTRL];
    a.scratch = (uint2*)c->buf[B_SCRATCH];
    a.scratch_rows = scratch_rows;
    a.npairs = (int)pairs.size();
    a.nscores = nscores;
    a.gap_init = gap_init;
    a.gap_ext = gap_ext;
    stage_matrix(a, mx);
    if (pf) {
        if (ensure(c, B_PROFILE, pf->image.size())) return -1;
        MCHK(hipMemcpyAsync(c->buf[B_PROFILE], pf->image.data(), pf->image.size(), hipMemcpyHostToDevice, c->stream));
        a.prof = (const unsigned char*)c->buf[B_PROFILE];
    }
    if (xl) {   // base and codon lie back to back in Translated: one copy of 324 bytes
        static_assert(offsetof(Translated, codon) == offsetof(Translated, base) + 256, "the tables are one block");
        if (ensure(c, B_PROFILE, 256 + 68)) return -1;
        MCHK(hipMemcpyAsync(c->buf[B_PROFILE], xl->base, 256 + 68, hipMemcpyHostToDevice, c->stream));
        a.prof = (const unsigned char*)c->buf[B_PROFILE];
    }
    return 0;
}
// the scratch column of a launch: the rows of its widest pair of more than one strip, in whole chunks
long long scratch_rows_of(const std::vector<MatPair>& pairs, int SW) {
    long long rows = 0;
    for (const MatPair& d : pairs)
        if (d.n > SW) rows = std::max<long long>(rows, d.m);
    return (rows + 63) / 64 * 64;
}

// act: the pairs to launch (both lengths > 0); d_scores[idx] receives each score, every other
// entry of d_scores[0, nscores) is zeroed.  amode != SW_MODE_LOCAL: seq1 always across the lanes.
// band >= 0: the band launches (seq1 across the lanes in every mode); -1: none.
// pf: the profile launches: seq1 of every pair is the profile (alen = pf->n, a_off not read), always across the
// lanes, and mx its alphabet.
int launch(MatCtx* c, const sw_matrix* mx, const unsigned char* d_arena, std::vector<DevSeq>& act, int gap_init,
           int gap_ext, int* d_scores, int nscores, bool a_on_lanes, int amode, int band = -1, const sw_profile* pf = nullptr,
           const Translated* xl = nullptr) {
    const auto t0 = std::chrono::steady_clock::now();
    const bool banded = band >= 0;
    if (amode != AM_LOCAL || banded || pf || xl) a_on_lanes = true;
    sw_stats st{};
    st.mode = xl ? MODE_MATRIX_XLATE : pf ? MODE_MATRIX_PROFILE : banded ? MODE_MATRIX_BAND : MODE_MATRIX;
    st.variant = amode;   // free on score-only matrix launches: the alignment mode (SW_MODE_*)
    st.C = MAT_C;
    st.items = nscores;
    MCHK(hipMemsetAsync(d_scores, 0, (size_t)std::max(nscores, 1) * sizeof(int), c->stream));
    if (act.empty()) {
        MCHK(hipStreamSynchronize(c->stream));
        st.W = 1;
        st.total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        report_stats(st);
        return 0;
    }
    // columns per lane: the cheapest estimate over the launch (option "W" forces one)
    int wi = 0;
    const long long forced = sw_get_option("W");
    long long best = -1;
    for (int k = 0; k < 4; ++k) {
        if (forced > 0 && W_OF[k] != forced) continue;
        long long cost = 0;
        for (const DevSeq& p : act) {
            if (banded) {
                int dlo, dhi;
                band_range(p.alen, p.blen, band, &dlo, &dhi);
                cost += band_pair_cost(p.alen, p.blen, dlo, dhi, W_OF[k]);
                continue;
            }
            const long long ca = pair_cost(p.alen, p.blen, W_OF[k]);
            cost += a_on_lanes ? ca : std::min(ca, pair_cost(p.blen, p.alen, W_OF[k]));
        }
        if (best < 0 || cost < best) {
            best = cost;
            wi = k;
        }
    }
    const int W = W_OF[wi];
    std::stable_sort(act.begin(), act.end(), Longer());
    std::vector<MatPair> pairs(act.size());
    long long cells = 0;
    for (size_t k = 0; k < act.size(); ++k) {
        const DevSeq& p = act[k];
        const bool swap = !a_on_lanes && pair_cost(p.blen, p.alen, W) < pair_cost(p.alen, p.blen, W);
        const MatPair& d = pairs[k] = make_pair(p, p.idx, swap, band);
        if (xl) pairs[k].swap_or_band = p.minus;
        if (banded) {
            int dlo, dhi;
            band_range(d.n, d.m, band, &dlo, &dhi);
            cells += band_cells(d.n, d.m, dlo, dhi);
        } else {
            cells += (long long)d.n * d.m;
        }
    }
    FillKernel& kern = xl ? c->xfill[amode][wi] : pf ? c->pfill[amode][wi] : c->fill[banded][amode][wi];
    const long long scratch_rows = scratch_rows_of(pairs, 64 * W);
    long long blocks = 0;
    MatArgs a{};
    if (fill_blocks(c, kern, pairs.size(), scratch_rows, &blocks) ||
        fill_args(c, mx, d_arena, pairs, nscores, gap_init, gap_ext, scratch_rows, blocks, a, pf, xl))
        return -1;
    a.scores = d_scores;

    MCHK(hipEventRecord(c->ev0, c->stream));
    void* kargs[] = {&a};
    MCHK(hipLaunchKernel(kern.fn, dim3((unsigned)blocks), dim3(256), kargs, (size_t)kern.dyn, c->stream));
    MCHK(hipGetLastError());
    MCHK(hipEventRecord(c->ev1, c->stream));
    MCHK(hipStreamSynchronize(c->stream));
    MCHK(hipEventElapsedTime(&st.kernel_ms, c->ev0, c->ev1));
    st.W = W;
    st.cells = cells;
    st.blocks = (int)blocks;
    st.waves_per_cu = 4 * kern.wgs;
    st.boundary_bytes = scratch_rows * 8 * 4 * blocks;
    st.total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    report_stats(st);
    return 0;
}

// ---- the cooperative score path, host side (COOPERATIVE SCORE above) ----

constexpr int MODE_MATRIX_COOP = 11;
// Nanoseconds of a step by index into W_OF, measured (a global 32768 x 32768 pair, one
// wave a SIMD).  A lone wave's step is bound by its dependent chain -- the table lookup, the DPP moves, the
// maxima -- not by its instruction count (section 13's table: 22.75 / 34.75 / 56.25 / 103.25), so the
// counts overrate the cost of W = 2 and put the automatic W one notch too low at every N measured.
constexpr int COOP_STEP_NS[4] = {93, 106, 147, 263};

// One pair at one W: which sequence lies across the lanes, and what that costs.  The last strip is
// done after about m + strips * 64 * (W + 1) steps: its own m + 64 * W, and every hand-off before it
// starts it 64 * (W + 1) steps after its left neighbour (the first 64 rows of an edge are stored
// W chunks into a strip, and a chunk is fetched one chunk ahead).  The edge columns, (strips - 1)
// of m rows of 8 bytes, must fit the budget.  Semi-global keeps seq1 across the lanes; local and
// global take the cheaper orientation that fits (the plain one on a tie), or the one option "orient"
// names (1: seq1 across the lanes, 2: seq2).
struct CoopShape {
    int swap;
    long long strips, edge_bytes, cost;
};
bool coop_shape(long long alen, long long blen, int amode, int wi, long long budget, CoopShape& out, long long* least) {
    const long long SW = 64LL * W_OF[wi];
    const long long orient = amode == AM_SEMI ? 1 : sw_get_option("orient");
    bool found = false;
    for (int swap = 0; swap < 2; ++swap) {
        if ((orient == 1 && swap) || (orient == 2 && !swap)) continue;
        const long long n = swap ? blen : alen, m = swap ? alen : blen;
        CoopShape s;
        s.swap = swap;
        s.strips = (n + SW - 1) / SW;
        s.edge_bytes = (s.strips - 1) * m * 8;
        s.cost = (m + s.strips * 64 * (W_OF[wi] + 1)) * COOP_STEP_NS[wi];
        if (least && (*least < 0 || s.edge_bytes < *least)) *least = s.edge_bytes;
        if (s.edge_bytes > budget) continue;
        if (!found || s.cost < out.cost) out = s;
        found = true;
    }
    return found;
}

// The W of a launch over pairs (alen[k], blen[k]) with both lengths > 0: the cheapest estimate among
// the W at which every pair fits the budget (option "W" forces one).  A pair's bytes fall with W, so
// a pair that fits no allowed W does not fit the largest: it is refused with the bytes it needs there.
int coop_choose_w(const int* alen, const int* blen, int npairs, int amode, long long budget, const char* what) {
    const long long forced = sw_get_option("W");
    int wi = -1;
    long long best = -1;
    for (int k = 0; k < 4; ++k) {
        if (forced > 0 && W_OF[k] != forced) continue;
        long long cost = 0;
        bool fits = true;
        for (int p = 0; p < npairs && fits; ++p) {
            if (alen[p] == 0 || blen[p] == 0) continue;
            CoopShape s;
            fits = coop_shape(alen[p], blen[p], amode, k, budget, s, nullptr);
            if (fits) cost += s.cost;
        }
        if (fits && (best < 0 || cost < best)) {
            best = cost;
            wi = k;
        }
    }
    if (wi >= 0) return wi;
    const int kmax = forced > 0 ? (forced == 1 ? 0 : forced == 2 ? 1 : forced == 4 ? 2 : 3) : 3;
    for (int p = 0; p < npairs; ++p) {
        if (alen[p] == 0 || blen[p] == 0) continue;
        CoopShape s;
        long long least = -1;
        if (coop_shape(alen[p], blen[p], amode, kmax, budget, s, &least)) continue;
        char m[320];
        std::snprintf(m, sizeof m,
                      "%s %d: a %d x %d pair needs %lld bytes of edge columns on the cooperative path at W = %d, more than "
                      "option coop_mb = %lld MiB (edge columns are not recycled inside a launch)",
                      what, p, alen[p], blen[p], least, W_OF[kmax], budget >> 20);
        report_error(m);
        break;
    }
    return -1;
}

// One cooperative launch: act (both lengths > 0, idx = the slot of d_scores, which the caller has
// zeroed), every pair at W_OF[wi] in the orientation coop_shape gives.
int launch_coop(MatCtx* c, const sw_matrix* mx, const unsigned char* d_arena, const std::vector<DevSeq>& act, int wi,
                long long budget, int gap_init, int gap_ext, int* d_scores, int nscores, int amode, sw_stats& st) {
    const std::vector<int> order = longest_first(act);
    std::vector<MatPair> pairs(act.size());
    std::vector<CoopPair> cp(act.size());
    std::vector<CoopItem> items;
    uint64_t edge_total = 0;
    for (size_t k = 0; k < act.size(); ++k) {
        const DevSeq& p = act[(size_t)order[k]];
        CoopShape s;
        if (!coop_shape(p.alen, p.blen, amode, wi, budget, s, nullptr)) {
            report_error("sw_score_matrix_batch_coop: a pair of the launch does not fit its plan");
            return -1;
        }
        pairs[k] = make_pair(p, p.idx, s.swap != 0, -1);
        cp[k] = CoopPair{edge_total, (unsigned)((unsigned long long)pairs[k].m * 8u), (int)s.strips};
        edge_total += (uint64_t)s.edge_bytes;
        for (int q = 0; q < (int)s.strips; ++q) items.push_back(CoopItem{(int)k, q});
        st.cells += (long long)p.alen * p.blen;
    }
    const size_t ni = items.size();
    const size_t prog_bytes = (ni * 4 + 15) / 16 * 16;   // a block of its own, whole 16 bytes, zeroed as a whole
    FillKernel& kern = c->coop[amode][wi];
    long long blocks = 0;
    MatArgs a{};
    if (fill_blocks(c, kern, ni, 0, &blocks) || fill_args(c, mx, d_arena, pairs, nscores, gap_init, gap_ext, 0, blocks, a) ||
        ensure(c, B_CPAIRS, cp.size() * sizeof(CoopPair)) || ensure(c, B_CITEMS, ni * sizeof(CoopItem)) ||
        ensure(c, B_EDGE, (size_t)edge_total) || ensure(c, B_PROGRESS, prog_bytes))
        return -1;
    a.scores = d_scores;
    a.npairs = (int)ni;   // what the waves claim
    MCHK(hipMemcpyAsync(c->buf[B_CPAIRS], cp.data(), cp.size() * sizeof(CoopPair), hipMemcpyHostToDevice, c->stream));
    MCHK(hipMemcpyAsync(c->buf[B_CITEMS], items.data(), ni * sizeof(CoopItem), hipMemcpyHostToDevice, c->stream));
    MCHK(hipMemsetAsync(c->buf[B_PROGRESS], 0, prog_bytes, c->stream));
    // option "coop_poison": a row consumed before it was stored then carries H of about 10^9
    if (sw_get_option("coop_poison") && edge_total) MCHK(hipMemsetAsync(c->buf[B_EDGE], 0x3F, (size_t)edge_total, c->stream));
    CoopArgs x{};
    x.cp = (const CoopPair*)c->buf[B_CPAIRS];
    x.items = (const CoopItem*)c->buf[B_CITEMS];
    x.edge = (unsigned char*)c->buf[B_EDGE];
    x.progress = (unsigned*)c->buf[B_PROGRESS];
    x.timeout_ticks = sw_get_option("timeout") * 100000000LL;   // s_memrealtime: 100 MHz
    void* kargs[] = {&a, &x};
    MCHK(hipEventRecord(c->ev0, c->stream));
    MCHK(hipLaunchKernel(kern.fn, dim3((unsigned)blocks), dim3(256), kargs, 0, c->stream));
    MCHK(hipGetLastError());
    MCHK(hipEventRecord(c->ev1, c->stream));
    Ctrl ctrl{};
    MCHK(hipMemcpyAsync(&ctrl, c->buf[B_CTRL], sizeof ctrl, hipMemcpyDeviceToHost, c->stream));
    MCHK(hipStreamSynchronize(c->stream));
    float ms = 0.f;
    MCHK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    st.kernel_ms += ms;
    st.items += (int)ni;
    st.blocks = (int)blocks;
    st.waves_per_cu = 4 * kern.wgs;
    st.boundary_bytes = std::max(st.boundary_bytes, (long long)edge_total);
    if (ctrl.error != 0) {
        const unsigned it = std::min<unsigned>(ctrl.err_item, (unsigned)ni - 1);
        char m[256];
        std::snprintf(m, sizeof m,
                      "sw_score_matrix_batch_coop: item %u (pair %d, strip %d of %d) waited longer than option timeout = %lld s "
                      "for the strip on its left (error bits 0x%x)",
                      it, pairs[(size_t)items[it].pair].out_idx, items[it].strip, cp[(size_t)items[it].pair].strips,
                      (long long)sw_get_option("timeout"), ctrl.error);
        report_error(m);
        return -1;
    }
    return 0;
}

// act: the pairs of the call with both lengths > 0, in input order (idx = the input index), at the
// call's W (coop_choose_w under `budget`, the bytes of option "coop_mb"); the pairs packed in input
// order into launches of at most `budget` bytes of edge columns.
int score_coop(MatCtx* c, const sw_matrix* mx, const unsigned char* d_arena, const std::vector<DevSeq>& act, int wi,
               long long budget, int gap_init, int gap_ext, int* d_scores, int nscores, int amode) {
    const auto t0 = std::chrono::steady_clock::now();
    sw_stats st{};
    st.mode = MODE_MATRIX_COOP;
    st.variant = amode;
    st.C = MAT_C;
    st.W = W_OF[wi];
    MCHK(hipMemsetAsync(d_scores, 0, (size_t)std::max(nscores, 1) * sizeof(int), c->stream));
    std::vector<long long> need(act.size());
    for (size_t k = 0; k < act.size(); ++k) {
        CoopShape s{};
        coop_shape(act[k].alen, act[k].blen, amode, wi, budget, s, nullptr);
        need[k] = s.edge_bytes;
    }
    std::vector<int> ends;
    align_pack(need.data(), (int)act.size(), budget, ends);
    int lo = 0;
    for (const int hi : ends) {
        const std::vector<DevSeq> part(act.begin() + lo, act.begin() + hi);
        if (!part.empty() && launch_coop(c, mx, d_arena, part, wi, budget, gap_init, gap_ext, d_scores, nscores, amode, st))
            return -1;
        lo = hi;
    }
    MCHK(hipStreamSynchronize(c->stream));
    st.total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    report_stats(st);
    return 0;
}

// refused like check_range (sw_db.hip): the int32 engine's score range
bool range_ok(const sw_matrix* mx, int alen, int blen, const char* what, int idx) {
    if ((long long)std::min(alen, blen) * std::max(mx->max_entry, 0) >= (1LL << 28)) {
        char m[160];
        std::snprintf(m, sizeof m, "%s %d: score range exceeds the int32 engine (min length * largest entry >= 2^28)", what, idx);
        report_error(m);
        return false;
    }
    return true;
}

constexpr long long MAT_MAX_SEQ = (1LL << 27) - 1;   // the engine's longest sequence (8-B rows in a 32-bit resource)

int score_host(const sw_matrix* mx, const unsigned char* const* a, const int* alen, const unsigned char* const* b,
               const int* blen, int npairs, int gap_init, int gap_ext, int* out, int amode = AM_LOCAL, int band = -1,
               bool coop = false) {
    if (!gaps_ok(gap_init, gap_ext)) return -1;
    size_t total = 0;
    for (int k = 0; k < npairs; ++k) {
        if (alen[k] < 0 || blen[k] < 0 || (alen[k] > 0 && !a[k]) || (blen[k] > 0 && !b[k]) || alen[k] > MAT_MAX_SEQ ||
            blen[k] > MAT_MAX_SEQ) {
            char m[96];
            std::snprintf(m, sizeof m, "pair %d: invalid sequence pointer or length", k);
            report_error(m);
            return -1;
        }
        if (amode != AM_LOCAL && !mode_range_ok(alen[k], blen[k], gap_init, gap_ext, "pair", k)) return -1;
        if (alen[k] == 0 || blen[k] == 0) continue;
        if (!range_ok(mx, alen[k], blen[k], "pair", k)) return -1;
        for (int s = 0; s < 2; ++s) {
            const unsigned char* p = s ? b[k] : a[k];
            const long long bad = matrix_first_bad(mx, p, s ? blen[k] : alen[k]);
            if (bad >= 0) {
                char m[160];
                std::snprintf(m, sizeof m, "pair %d: seq%d position %lld: byte 0x%02x is outside the matrix alphabet", k,
                              s + 1, bad, p[bad]);
                report_error(m);
                return -1;
            }
        }
        total += ((size_t)alen[k] + 15) / 16 * 16 + ((size_t)blen[k] + 15) / 16 * 16;
    }
    const long long coop_budget = coop ? sw_get_option("coop_mb") << 20 : 0;
    int coop_wi = 0;   // refused before anything is launched
    if (coop && (coop_wi = coop_choose_w(alen, blen, npairs, amode, coop_budget, "pair")) < 0) return -1;
    MatCtx* c = get_mctx();
    if (!c) return -1;
    std::vector<unsigned char> arena(total);
    std::vector<DevSeq> act;
    size_t off = 0;
    for (int k = 0; k < npairs; ++k) {
        if (alen[k] == 0 || blen[k] == 0) continue;
        DevSeq p;
        p.a_off = (int64_t)off;
        std::memcpy(arena.data() + off, a[k], (size_t)alen[k]);
        off += ((size_t)alen[k] + 15) / 16 * 16;
        p.b_off = (int64_t)off;
        std::memcpy(arena.data() + off, b[k], (size_t)blen[k]);
        off += ((size_t)blen[k] + 15) / 16 * 16;
        p.alen = alen[k];
        p.blen = blen[k];
        p.idx = k;
        act.push_back(p);
    }
    if (ensure(c, B_ARENA, total) || ensure(c, B_SCORES, (size_t)npairs * sizeof(int))) return -1;
    if (total) MCHK(hipMemcpyAsync(c->buf[B_ARENA], arena.data(), total, hipMemcpyHostToDevice, c->stream));
    if (coop ? score_coop(c, mx, (const unsigned char*)c->buf[B_ARENA], act, coop_wi, coop_budget, gap_init, gap_ext,
                          (int*)c->buf[B_SCORES], npairs, amode)
             : launch(c, mx, (const unsigned char*)c->buf[B_ARENA], act, gap_init, gap_ext, (int*)c->buf[B_SCORES], npairs, false,
                      amode, band))
        return -1;
    MCHK(hipMemcpy(out, c->buf[B_SCORES], (size_t)npairs * sizeof(int), hipMemcpyDeviceToHost));
    if (amode != AM_LOCAL)   // empty sequences are answered on the host
        for (int k = 0; k < npairs; ++k)
            if (alen[k] == 0 || blen[k] == 0) out[k] = mode_empty_score(alen[k], blen[k], gap_init, gap_ext, amode);
    return 0;
}

// One traced launch: fill, then walk.  act: the pairs (both lengths > 0, idx = the slot of res and
// of ops_off), in input order.  res[idx] and the operations (ops, at ops_off[idx]) come back to the host.
struct TracedOut {
    std::vector<TraceRes> res;
    std::vector<unsigned char> ops;
    std::vector<uint64_t> ops_off;
    long long trace_total = 0;
    int blocks = 0;
};
int launch_traced(MatCtx* c, const sw_matrix* mx, const unsigned char* d_arena, const std::vector<DevSeq>& act,
                  int gap_init, int gap_ext, TracedOut& o, int amode, int band = -1, const sw_profile* pf = nullptr,
                  const Translated* xl = nullptr) {
    const bool banded = band >= 0;
    FillKernel& kern = xl ? c->xfill[amode][WI_TRACED] : pf ? c->pfill[amode][WI_TRACED] : c->fill[banded][amode][WI_TRACED];
    const size_t np = act.size();
    const std::vector<int> order = longest_first(act);
    std::vector<MatPair> pairs(np);
    std::vector<WalkPair> walk(np);
    o.ops_off.assign(np, 0);
    uint64_t ops_total = 0;
    for (size_t k = 0; k < np; ++k) {   // the operations in input order
        o.ops_off[k] = ops_total;
        ops_total += (uint64_t)act[k].alen + (uint64_t)act[k].blen;
    }
    long long trace_total = 0;
    for (size_t s = 0; s < np; ++s) {
        WalkPair& w = walk[s];
        pairs[s] = make_pair(act[(size_t)order[s]], order[s], false, band, &w);
        if (xl) pairs[s].swap_or_band = act[(size_t)order[s]].minus;
        w.trace_off = (uint64_t)trace_total;
        w.ops_off = o.ops_off[(size_t)order[s]];
        trace_total += (long long)w.trace_bytes;
    }
    const long long scratch_rows = scratch_rows_of(pairs, 64 * TRACE_W);
    long long blocks = 0;
    MatArgs a{};
    if (fill_blocks(c, kern, np, scratch_rows, &blocks) ||
        fill_args(c, mx, d_arena, pairs, (int)np, gap_init, gap_ext, scratch_rows, blocks, a, pf, xl) ||
        ensure(c, B_WALK, np * sizeof(WalkPair)) || ensure(c, B_TRACE, (size_t)trace_total) ||
        ensure(c, B_RES, np * sizeof(TraceRes)) || ensure(c, B_OPS, (size_t)ops_total))
        return -1;
    MCHK(hipMemcpyAsync(c->buf[B_WALK], walk.data(), np * sizeof(WalkPair), hipMemcpyHostToDevice, c->stream));
    MCHK(hipMemsetAsync(c->buf[B_RES], 0, np * sizeof(TraceRes), c->stream));
    a.walk = (const WalkPair*)c->buf[B_WALK];
    a.trace = (unsigned char*)c->buf[B_TRACE];
    a.res = (TraceRes*)c->buf[B_RES];
    WalkArgs w{a.pairs, a.walk, a.trace, (unsigned char*)c->buf[B_OPS], a.res, (int)np, amode};

    MCHK(hipEventRecord(c->ev0, c->stream));
    void* kargs[] = {&a};
    MCHK(hipLaunchKernel(kern.fn, dim3((unsigned)blocks), dim3(256), kargs, (size_t)kern.dyn, c->stream));
    MCHK(hipGetLastError());
    MCHK(hipEventRecord(c->ev1, c->stream));
    if (banded) hipLaunchKernelGGL(sw_matrix_walk_kernel<true>, dim3((unsigned)((np + 63) / 64)), dim3(64), 0, c->stream, w);
    else hipLaunchKernelGGL(sw_matrix_walk_kernel<false>, dim3((unsigned)((np + 63) / 64)), dim3(64), 0, c->stream, w);
    MCHK(hipGetLastError());
    MCHK(hipEventRecord(c->ev2, c->stream));
    o.res.resize(np);
    o.ops.resize((size_t)ops_total);
    MCHK(hipMemcpyAsync(o.res.data(), c->buf[B_RES], np * sizeof(TraceRes), hipMemcpyDeviceToHost, c->stream));
    MCHK(hipMemcpyAsync(o.ops.data(), c->buf[B_OPS], (size_t)ops_total, hipMemcpyDeviceToHost, c->stream));
    MCHK(hipStreamSynchronize(c->stream));
    float fill = 0.f, wk = 0.f;
    MCHK(hipEventElapsedTime(&fill, c->ev0, c->ev1));
    MCHK(hipEventElapsedTime(&wk, c->ev1, c->ev2));
    t_fill_ms += fill;
    t_walk_ms += wk;
    o.trace_total = trace_total;
    o.blocks = (int)blocks;
    return 0;
}

// ---- long pairs: the host side of the checkpointed traceback ----

int walk_failed(const char* what, int idx, int err) {
    char m[200];
    std::snprintf(m, sizeof m, "%s %d: the traceback walk failed (%s)", what, idx,
                  err == WALK_OVERRUN ? "more than n + m operations"
                  : err == WALK_RANGE ? "a cell outside the trace buffer"
                                      : "it did not leave its strip on the left");
    report_error(m);
    return -1;
}

// One group: pairs whose checkpoints are held together.  act: the pairs (both lengths > 0, idx = the
// input index, for messages), in input order.  The locate launch, then rounds of strip fill + walk;
// res[s], ws[s] and the operations (ops, at ops_off[s], ws[s].nops of them, last first) of act[s]
// come back to the host.
struct LongOut {
    std::vector<TraceRes> res;
    std::vector<WalkState> ws;
    std::vector<unsigned char> ops;
    std::vector<uint64_t> ops_off;
};
constexpr int MODE_MATRIX_LONG_COOP = 12;   // sw_align_matrix_long_coop: cooperative locate, a window of strips a round

// The cooperative locate launch of one group (LONG PAIRS ON MANY WAVES above): the items are the strips of
// its pairs, pair-major and strip-minor, the pairs longest first (pairs[k], with the checkpoint column 0 of
// pairs[k] at byte ckpt_off[pairs[k].out_idx] of B_CKPT).  o.res[slot] receives score, ei, ej of every pair,
// merged on the host from the records of its strips (local), or read from the record of its last strip (a mode:
// align_mode_end).  a: the launch's arguments, which the strip fills go on using.  *extra: the bytes of
// progress words and end records.
int locate_coop(MatCtx* c, const sw_matrix* mx, const unsigned char* d_arena, const std::vector<MatPair>& pairs,
                const std::vector<uint64_t>& ckpt_off, uint64_t ckpt_total, int gap_init, int gap_ext, const char* fn,
                const char* what, const std::vector<int>& name_of, MatArgs& a, sw_stats& st, LongOut& o, long long* extra,
                int amode) {
    FillKernel& kern = c->locate_coop[amode];
    const size_t np = pairs.size();
    std::vector<CoopPair> cp(np);
    std::vector<CoopItem> items;
    std::vector<size_t> first(np);
    for (size_t k = 0; k < np; ++k) {
        const MatPair& d = pairs[k];
        cp[k] = CoopPair{ckpt_off[(size_t)d.out_idx], (unsigned)align_ckpt_stride(d.m), (int)align_strips(d.n)};
        first[k] = items.size();
        for (int q = 0; q < cp[k].strips; ++q) items.push_back(CoopItem{(int)k, q});
    }
    const size_t ni = items.size();
    const size_t prog_bytes = (size_t)align_progress_bytes((long long)ni), end_bytes = (size_t)align_end_bytes((long long)ni);
    long long blocks = 0;
    if (fill_blocks(c, kern, ni, 0, &blocks) || fill_args(c, mx, d_arena, pairs, (int)np, gap_init, gap_ext, 0, blocks, a) ||
        ensure(c, B_CPAIRS, np * sizeof(CoopPair)) || ensure(c, B_CITEMS, ni * sizeof(CoopItem)) ||
        ensure(c, B_PROGRESS, prog_bytes) || ensure(c, B_ENDS, end_bytes))
        return -1;
    a.npairs = (int)ni;   // what the waves claim
    MCHK(hipMemcpyAsync(c->buf[B_CPAIRS], cp.data(), np * sizeof(CoopPair), hipMemcpyHostToDevice, c->stream));
    MCHK(hipMemcpyAsync(c->buf[B_CITEMS], items.data(), ni * sizeof(CoopItem), hipMemcpyHostToDevice, c->stream));
    MCHK(hipMemsetAsync(c->buf[B_PROGRESS], 0, prog_bytes, c->stream));
    MCHK(hipMemsetAsync(c->buf[B_ENDS], 0, end_bytes, c->stream));
    // option "coop_poison": a row consumed before it was stored then carries H of about 10^9
    if (sw_get_option("coop_poison") && ckpt_total) MCHK(hipMemsetAsync(c->buf[B_CKPT], 0x3F, (size_t)ckpt_total, c->stream));
    CoopArgs x{};
    x.cp = (const CoopPair*)c->buf[B_CPAIRS];
    x.items = (const CoopItem*)c->buf[B_CITEMS];
    x.edge = (unsigned char*)c->buf[B_CKPT];
    x.progress = (unsigned*)c->buf[B_PROGRESS];
    x.timeout_ticks = sw_get_option("timeout") * 100000000LL;   // s_memrealtime: 100 MHz
    x.ends = (AlignEnd*)c->buf[B_ENDS];
    void* kargs[] = {&a, &x};
    MCHK(hipEventRecord(c->ev0, c->stream));
    MCHK(hipLaunchKernel(kern.fn, dim3((unsigned)blocks), dim3(256), kargs, 0, c->stream));
    MCHK(hipGetLastError());
    MCHK(hipEventRecord(c->ev1, c->stream));
    Ctrl ctrl{};
    std::vector<AlignEnd> ends(ni);
    MCHK(hipMemcpyAsync(&ctrl, c->buf[B_CTRL], sizeof ctrl, hipMemcpyDeviceToHost, c->stream));
    MCHK(hipMemcpyAsync(ends.data(), c->buf[B_ENDS], end_bytes, hipMemcpyDeviceToHost, c->stream));
    MCHK(hipStreamSynchronize(c->stream));
    float ms = 0.f;
    MCHK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    t_fill_ms += ms;
    t_locate_ms += ms;
    st.items += (int)ni;
    st.blocks = (int)blocks;
    st.waves_per_cu = 4 * kern.wgs;
    *extra = (long long)(prog_bytes + end_bytes);
    if (ctrl.error != 0) {
        const unsigned it = std::min<unsigned>(ctrl.err_item, (unsigned)ni - 1);
        char m[256];
        std::snprintf(m, sizeof m,
                      "%s: item %u (%s %d, strip %d of %d) waited longer than option timeout = %lld s for the strip on its "
                      "left (error bits 0x%x)",
                      fn, it, what, name_of[(size_t)pairs[(size_t)items[it].pair].out_idx], items[it].strip,
                      cp[(size_t)items[it].pair].strips, (long long)sw_get_option("timeout"), ctrl.error);
        report_error(m);
        return -1;
    }
    o.res.assign(np, TraceRes{});
    for (size_t k = 0; k < np; ++k) {
        TraceRes& r = o.res[(size_t)pairs[k].out_idx];
        if (amode == AM_LOCAL) align_merge_ends(ends.data() + first[k], cp[k].strips, &r.score, &r.ei, &r.ej);
        else align_mode_end(ends.data() + first[k], cp[k].strips, &r.score, &r.ei, &r.ej);
    }
    return 0;
}

// coop: the cooperative locate launch instead of the one-wave one, and rounds that fill a window of strips
// a pair (align_window) and walk it with sw_matrix_walk_window_kernel; else a window is one strip and the
// launches are the ones they were.
// amode != AM_LOCAL (LONG PAIRS IN A MODE): the kernels of that mode, and every pair walks,
// whatever its score, from (n - 1, ej) in state H.
int long_group(MatCtx* c, const sw_matrix* mx, const unsigned char* d_arena, const std::vector<DevSeq>& act, int gap_init,
               int gap_ext, long long trace_budget, const char* what, const int* name_idx, sw_stats& st, LongOut& o,
               bool coop, int amode) {
    FillKernel& k_locate = c->locate[amode];
    FillKernel& k_strip = c->strip[amode];
    const size_t np = act.size();
    const std::vector<int> order = longest_first(act);
    std::vector<uint64_t> ckpt_off(np);
    o.ops_off.assign(np, 0);
    uint64_t ops_total = 0, ckpt_total = 0;
    long long max_strips = 0;
    for (size_t s = 0; s < np; ++s) {
        o.ops_off[s] = ops_total;
        ops_total += (uint64_t)act[s].alen + (uint64_t)act[s].blen;
        ckpt_off[s] = ckpt_total;
        ckpt_total += (uint64_t)((align_strips(act[s].alen) - 1) * align_ckpt_stride(act[s].blen));
        max_strips = std::max(max_strips, align_strips(act[s].alen));
    }
    std::vector<MatPair> pairs(np);
    std::vector<LongPair> lp(np);
    for (size_t k = 0; k < np; ++k) {
        const DevSeq& p = act[(size_t)order[k]];
        pairs[k] = make_pair(p, order[k], false, -1);
        lp[k] = LongPair{ckpt_off[(size_t)order[k]], (unsigned)align_ckpt_stride(p.blen), 0u};
    }
    long long blocks = 0;
    long long held = (long long)ckpt_total;   // bytes held beside the traces: checkpoints; coop: progress words, end records
    MatArgs a{};   // no scratch: every strip's right edge goes to a checkpoint column
    LongArgs x{};
    void* kargs[] = {&a, &x};
    if (ensure(c, B_CKPT, (size_t)ckpt_total) || ensure(c, B_OPS, (size_t)ops_total) || ensure(c, B_STATE, np * sizeof(WalkState)))
        return -1;
    if (coop) {
        std::vector<int> name_of(np);
        for (size_t s = 0; s < np; ++s) name_of[s] = name_idx ? name_idx[act[s].idx] : act[s].idx;
        long long extra = 0;
        if (locate_coop(c, mx, d_arena, pairs, ckpt_off, ckpt_total, gap_init, gap_ext,
                        name_idx ? "sw_db_align_matrix_long_coop" : "sw_align_matrix_long_coop", what, name_of, a, st, o, &extra,
                        amode))
            return -1;
        held += extra;
        x.ckpt = (unsigned char*)c->buf[B_CKPT];
    } else {
        if (fill_blocks(c, k_locate, np, 0, &blocks) || fill_args(c, mx, d_arena, pairs, (int)np, gap_init, gap_ext, 0, blocks, a) ||
            ensure(c, B_LONG, np * sizeof(LongPair)) || ensure(c, B_RES, np * sizeof(TraceRes)))
            return -1;
        MCHK(hipMemcpyAsync(c->buf[B_LONG], lp.data(), np * sizeof(LongPair), hipMemcpyHostToDevice, c->stream));
        MCHK(hipMemsetAsync(c->buf[B_RES], 0, np * sizeof(TraceRes), c->stream));
        a.res = (TraceRes*)c->buf[B_RES];
        x.lp = (const LongPair*)c->buf[B_LONG];
        x.ckpt = (unsigned char*)c->buf[B_CKPT];

        MCHK(hipEventRecord(c->ev0, c->stream));
        MCHK(hipLaunchKernel(k_locate.fn, dim3((unsigned)blocks), dim3(256), kargs, 0, c->stream));
        MCHK(hipGetLastError());
        MCHK(hipEventRecord(c->ev1, c->stream));
        o.res.resize(np);
        MCHK(hipMemcpyAsync(o.res.data(), c->buf[B_RES], np * sizeof(TraceRes), hipMemcpyDeviceToHost, c->stream));
        MCHK(hipStreamSynchronize(c->stream));
        float ms = 0.f;
        MCHK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
        t_fill_ms += ms;
        t_locate_ms += ms;
        st.blocks = (int)blocks;
        st.waves_per_cu = 4 * k_locate.wgs;
    }
    st.boundary_bytes = std::max(st.boundary_bytes, held);

    // every walk starts at its end cell in state H; a local pair without an alignment never walks, and in a
    // mode every pair walks, from column n - 1 (global: from the corner), whatever its score
    o.ws.assign(np, WalkState{});
    for (size_t s = 0; s < np; ++s) {
        const TraceRes& r = o.res[s];
        const bool walks = amode != AM_LOCAL || r.score > 0;
        if (walks && !align_long_end_ok(act[s].alen, act[s].blen, amode, r.ei, r.ej))
            return walk_failed(what, name_idx ? name_idx[act[s].idx] : act[s].idx, WALK_RANGE);
        o.ws[s].i = r.ei;
        o.ws[s].j = r.ej;
        o.ws[s].done = walks ? 0 : 1;
    }
    MCHK(hipMemcpyAsync(c->buf[B_STATE], o.ws.data(), np * sizeof(WalkState), hipMemcpyHostToDevice, c->stream));

    // rounds: every pair still walking has its current strip filled and walked; each round moves a
    // walk that has not ended exactly one strip to the left, so there are at most max_strips rounds
    // coop: a pair contributes a window of g strips (align_window), g items that end at its current strip, all over
    // the rows of that strip, their buffers end to end; a round still moves every walk that goes on to the strip
    // left of what was filled for it.  g = 1 otherwise, and the launches are the ones they were.
    const int long_window = coop ? (int)sw_get_option("long_window") : 1;
    std::vector<int> live, ends, win;
    std::vector<long long> need;
    std::vector<StripItem> items;
    std::vector<WindowItem> windows;
    for (long long round = 0;; ++round) {
        live.clear();
        need.clear();
        win.clear();
        long long live_bytes = 0;
        for (size_t s = 0; s < np; ++s)
            if (!o.ws[s].done) {
                live.push_back((int)s);
                live_bytes += align_strip_trace_bytes(act[s].blen);
            }
        if (live.empty()) break;
        if (round >= max_strips) return walk_failed(what, name_idx ? name_idx[act[(size_t)live[0]].idx] : act[(size_t)live[0]].idx, 0);
        for (const int s : live) {
            const long long one = align_strip_trace_bytes(act[(size_t)s].blen);
            const int g = coop ? align_window(one, live_bytes, trace_budget, long_window, o.ws[(size_t)s].i / ALIGN_STRIP) : 1;
            win.push_back(g);
            need.push_back(g * one);
        }
        align_pack(need.data(), (int)live.size(), trace_budget, ends);
        t_rounds += 1;
        int lo = 0;
        for (const int hi : ends) {   // one launch pair: strip fill, walk
            items.clear();
            windows.clear();
            uint64_t trace_total = 0;
            for (int k = lo; k < hi; ++k) {
                const size_t s = (size_t)live[(size_t)k];
                const DevSeq& p = act[s];
                const int g = win[(size_t)k], last = o.ws[s].i / ALIGN_STRIP;
                const uint64_t one = (uint64_t)need[(size_t)k] / (uint64_t)g;
                WindowItem wi{};
                wi.trace_off = trace_total;
                wi.ops_off = o.ops_off[s];
                wi.n = p.alen;
                wi.m = p.blen;
                wi.strip0 = last - g + 1;
                wi.nstrips = g;
                wi.steps = (int)align_strip_steps(p.blen);
                wi.rows = o.ws[s].j + 1;
                wi.trace_bytes = (unsigned)need[(size_t)k];
                wi.slot = (int)s;
                windows.push_back(wi);
                for (int q = 0; q < g; ++q) {
                    StripItem it{};
                    it.col_off = (uint64_t)p.a_off;
                    it.row_off = (uint64_t)p.b_off;
                    it.n = p.alen;
                    it.m = p.blen;
                    it.strip = wi.strip0 + q;
                    it.rows = wi.rows;
                    it.ckpt_in = it.strip > 0 ? ckpt_off[s] + (uint64_t)(it.strip - 1) * (uint64_t)align_ckpt_stride(p.blen) : 0;
                    it.trace_off = trace_total;
                    it.trace_bytes = (unsigned)one;
                    it.ops_off = o.ops_off[s];
                    it.slot = (int)s;
                    trace_total += one;
                    items.push_back(it);
                }
            }
            std::stable_sort(items.begin(), items.end(), [](const StripItem& p, const StripItem& q) { return p.rows > q.rows; });
            const size_t ni = items.size(), nw = windows.size();
            if (fill_blocks(c, k_strip, ni, 0, &blocks)) return -1;
            if (ensure(c, B_ITEMS, ni * sizeof(StripItem)) || ensure(c, B_TRACE, (size_t)trace_total)) return -1;
            if (coop && ensure(c, B_WINDOWS, nw * sizeof(WindowItem))) return -1;
            MCHK(hipMemcpyAsync(c->buf[B_ITEMS], items.data(), ni * sizeof(StripItem), hipMemcpyHostToDevice, c->stream));
            if (coop)
                MCHK(hipMemcpyAsync(c->buf[B_WINDOWS], windows.data(), nw * sizeof(WindowItem), hipMemcpyHostToDevice, c->stream));
            MCHK(hipMemsetAsync(c->buf[B_CTRL], 0, sizeof(Ctrl), c->stream));
            a.pairs = nullptr;
            a.npairs = (int)ni;
            x.items = (const StripItem*)c->buf[B_ITEMS];
            x.trace = (unsigned char*)c->buf[B_TRACE];
            MCHK(hipEventRecord(c->ev0, c->stream));
            MCHK(hipLaunchKernel(k_strip.fn, dim3((unsigned)blocks), dim3(256), kargs, 0, c->stream));
            MCHK(hipGetLastError());
            MCHK(hipEventRecord(c->ev1, c->stream));
            if (coop) {
                WalkWindowArgs w{(const WindowItem*)c->buf[B_WINDOWS], x.trace, (unsigned char*)c->buf[B_OPS],
                                 (WalkState*)c->buf[B_STATE], (int)nw, amode};
                hipLaunchKernelGGL(sw_matrix_walk_window_kernel, dim3((unsigned)((nw + 63) / 64)), dim3(64), 0, c->stream, w);
            } else {
                WalkStripArgs w{x.items, x.trace, (unsigned char*)c->buf[B_OPS], (WalkState*)c->buf[B_STATE], (int)ni, amode};
                hipLaunchKernelGGL(sw_matrix_walk_strip_kernel, dim3((unsigned)((ni + 63) / 64)), dim3(64), 0, c->stream, w);
            }
            MCHK(hipGetLastError());
            MCHK(hipEventRecord(c->ev2, c->stream));
            MCHK(hipMemcpyAsync(o.ws.data(), c->buf[B_STATE], np * sizeof(WalkState), hipMemcpyDeviceToHost, c->stream));
            MCHK(hipStreamSynchronize(c->stream));
            float fill = 0.f, wk = 0.f;
            MCHK(hipEventElapsedTime(&fill, c->ev0, c->ev1));
            MCHK(hipEventElapsedTime(&wk, c->ev1, c->ev2));
            t_fill_ms += fill;
            t_walk_ms += wk;
            st.variant += 1;
            st.blocks = (int)blocks;
            st.waves_per_cu = 4 * k_strip.wgs;
            st.boundary_bytes = std::max(st.boundary_bytes, held + (long long)trace_total);
            for (const WindowItem& it : windows) {   // an error stops the call; a walk that goes on stands in the strip left of the window
                const WalkState& s = o.ws[(size_t)it.slot];
                const int idx = name_idx ? name_idx[act[(size_t)it.slot].idx] : act[(size_t)it.slot].idx;
                if (s.err != 0 || s.nops < 0 || s.nops > (long long)it.n + it.m) return walk_failed(what, idx, s.err ? s.err : WALK_OVERRUN);
                if (!s.done && (it.strip0 == 0 || s.i != it.strip0 * ALIGN_STRIP - 1 || s.j < 0 || s.j >= it.rows || s.state < 0 ||
                                s.state > 1))
                    return walk_failed(what, idx, 0);
            }
            lo = hi;
        }
    }
    o.ops.resize((size_t)ops_total);
    if (ops_total) MCHK(hipMemcpy(o.ops.data(), c->buf[B_OPS], (size_t)ops_total, hipMemcpyDeviceToHost));
    return 0;
}

}  // namespace

int matrix_align_long_device(const sw_matrix* mx, const unsigned char* d_arena, const int64_t* a_off, const int* alen,
                             const int64_t* b_off, const int* blen, const int* name_idx, int npairs, int gap_init,
                             int gap_ext, const char* what, AlignSink& sink, bool coop, int amode) {
    const auto t0 = std::chrono::steady_clock::now();
    if (!gaps_ok(gap_init, gap_ext)) return -1;
    const long long trace_budget = sw_get_option("trace_mb") << 20;
    long long ckpt_budget = 0;
    if (align_ckpt_budget(&ckpt_budget)) return -1;
    std::vector<long long> need((size_t)npairs, 0);
    for (int k = 0; k < npairs; ++k) {   // refused before anything is launched
        if (amode != AM_LOCAL && !mode_range_ok(alen[k], blen[k], gap_init, gap_ext, what, name_idx ? name_idx[k] : k))
            return -1;
        sw_align_plan p;
        if (align_long_plan(alen[k], blen[k], trace_budget, ckpt_budget, what, name_idx ? name_idx[k] : k, &p)) return -1;
        need[(size_t)k] = p.ckpt_bytes;
    }
    MatCtx* c = get_mctx();
    if (!c) return -1;
    t_fill_ms = t_walk_ms = t_locate_ms = 0.f;
    t_rounds = 0;
    sw_stats st{};
    st.mode = coop ? MODE_MATRIX_LONG_COOP : MODE_MATRIX_LONG;
    st.W = TRACE_W;
    st.C = MAT_C;
    st.items = coop ? 0 : npairs;   // coop: the items of the locate launches (locate_coop)
    std::vector<int> ends;
    align_pack(need.data(), npairs, ckpt_budget, ends);   // groups: the checkpoints held at once
    std::vector<DevSeq> act;
    LongOut o;
    int lo = 0;
    for (const int hi : ends) {
        act.clear();
        for (int k = lo; k < hi; ++k)
            if (alen[k] > 0 && blen[k] > 0) {
                act.push_back(DevSeq{a_off[k], b_off[k], alen[k], blen[k], k});
                st.cells += (long long)alen[k] * blen[k];
            }
        if (!act.empty() && long_group(c, mx, d_arena, act, gap_init, gap_ext, trace_budget, what, name_idx, st, o, coop, amode))
            return -1;
        size_t s = 0;
        for (int k = lo; k < hi; ++k) {
            if (alen[k] == 0 || blen[k] == 0) {
                if (amode != AM_LOCAL) align_mode_empty(sink, k, alen[k], blen[k], gap_init, gap_ext, amode);
                else sink.set_empty(k);
                continue;
            }
            const TraceRes& r = o.res[s];
            const WalkState& w = o.ws[s];
            if (amode == AM_LOCAL && r.score <= 0) sink.set_empty(k);
            else sink.set(k, r.score, w.i + 1, r.ei + 1, w.j + 1, r.ej + 1, o.ops.data() + o.ops_off[s], w.nops);
            ++s;
        }
        lo = hi;
    }
    st.variant |= amode << 28;   // bits 28-29: the alignment mode (SW_MODE_*), as the traced launches report it
    st.kernel_ms = t_fill_ms;
    st.total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    report_stats(st);
    return 0;
}

int matrix_align_device(const sw_matrix* mx, const unsigned char* d_arena, const int64_t* a_off, const int* alen,
                        const int64_t* b_off, const int* blen, const int* name_idx, int npairs, int gap_init,
                        int gap_ext, const char* what, AlignSink& sink, int amode, int band, const sw_profile* pf,
                        const Translated* xl) {
    const auto t0 = std::chrono::steady_clock::now();
    if (!gaps_ok(gap_init, gap_ext)) return -1;
    const long long budget = sw_get_option("trace_mb") << 20;
    const bool banded = band >= 0;
    // the trace a pair holds: the whole matrix (section 11), or the band's strips
    auto pair_trace = [&](int n, int m) {
        if (!banded) return trace_bytes(n, m);
        int dlo, dhi;
        band_range(n, m, band, &dlo, &dhi);
        return band_trace_bytes(n, m, dlo, dhi);
    };
    auto pair_cells = [&](int n, int m) {
        if (!banded) return (long long)n * m;
        int dlo, dhi;
        band_range(n, m, band, &dlo, &dhi);
        return band_cells(n, m, dlo, dhi);
    };
    for (int k = 0; k < npairs; ++k) {   // refused before anything is launched
        if (amode != AM_LOCAL && !mode_range_ok(alen[k], blen[k], gap_init, gap_ext, what, name_idx ? name_idx[k] : k))
            return -1;
        if (alen[k] == 0 || blen[k] == 0) continue;
        const long long need = pair_trace(alen[k], blen[k]);
        if (need > budget) {
            char m[400];
            if (xl)
                std::snprintf(m, sizeof m,
                              "%s %d: a %d x %d alignment needs %lld bytes of trace memory, more than option trace_mb = %lld "
                              "MiB, and there is no long path against a translated frame",
                              what, name_idx ? name_idx[k] : k, alen[k], blen[k], need, budget >> 20);
            else if (pf)
                std::snprintf(m, sizeof m,
                              "%s %d: a %d x %d alignment needs %lld bytes of trace memory, more than option trace_mb = %lld "
                              "MiB, and there is no long path with a profile",
                              what, name_idx ? name_idx[k] : k, alen[k], blen[k], need, budget >> 20);
            else if (banded)
                std::snprintf(m, sizeof m,
                              "%s %d: a %d x %d alignment in a band of %d needs %lld bytes of trace memory, more than option "
                              "trace_mb = %lld MiB: a narrower band or a larger trace_mb aligns this pair",
                              what, name_idx ? name_idx[k] : k, alen[k], blen[k], band, need, budget >> 20);
            else if (amode != AM_LOCAL)
                std::snprintf(m, sizeof m,
                              "%s %d: a %d x %d alignment needs %lld bytes of trace memory, more than option trace_mb = %lld "
                              "MiB, and the long=True routing of this call is local only (sw_align_matrix_long_mode / "
                              "sw_db_align_matrix_long_mode align such pairs in a mode, a strip at a time)",
                              what, name_idx ? name_idx[k] : k, alen[k], blen[k], need, budget >> 20);
            else
                std::snprintf(m, sizeof m,
                              "%s %d: a %d x %d alignment needs %lld bytes of trace memory, more than option trace_mb = %lld MiB "
                              "(sw_align_matrix_long / sw_db_align_matrix_long align such pairs a strip at a time)",
                              what, name_idx ? name_idx[k] : k, alen[k], blen[k], need, budget >> 20);
            report_error(m);
            return -1;
        }
    }
    MatCtx* c = get_mctx();
    if (!c) return -1;
    t_fill_ms = t_walk_ms = t_locate_ms = 0.f;
    t_rounds = 0;
    sw_stats st{};
    st.mode = xl ? MODE_MATRIX_XLATE_TRACE : pf ? MODE_MATRIX_PROFILE_TRACE : banded ? MODE_MATRIX_BAND_TRACE : MODE_MATRIX_TRACE;
    st.W = TRACE_W;
    st.C = MAT_C;
    st.items = npairs;
    std::vector<DevSeq> act;
    TracedOut o;
    int lo = 0;
    while (lo < npairs) {   // pairs [lo, hi): as many as fit the budget, in input order
        int hi = lo;
        long long sum = 0;
        act.clear();
        for (; hi < npairs; ++hi) {
            if (alen[hi] == 0 || blen[hi] == 0) continue;
            const long long need = pair_trace(alen[hi], blen[hi]);
            if (!act.empty() && sum + need > budget) break;
            sum += need;
            act.push_back(DevSeq{a_off[hi], b_off[hi], alen[hi], blen[hi], hi, xl && xl->minus ? xl->minus[hi] : 0});
            st.cells += pair_cells(alen[hi], blen[hi]);
        }
        if (!act.empty()) {
            if (launch_traced(c, mx, d_arena, act, gap_init, gap_ext, o, amode, band, pf, xl)) return -1;
            st.variant += 1;
            st.blocks = o.blocks;
            st.waves_per_cu =
                4 * (xl ? c->xfill[amode][WI_TRACED] : pf ? c->pfill[amode][WI_TRACED] : c->fill[banded][amode][WI_TRACED]).wgs;
            st.boundary_bytes = std::max(st.boundary_bytes, o.trace_total);
        }
        size_t s = 0;
        for (int k = lo; k < hi; ++k) {
            if (alen[k] == 0 || blen[k] == 0) {
                if (amode != AM_LOCAL) align_mode_empty(sink, k, alen[k], blen[k], gap_init, gap_ext, amode);
                else sink.set_empty(k);
                continue;
            }
            const TraceRes& r = o.res[s];
            if (r.err != 0 || r.nops < 0 || r.nops > alen[k] + (long long)blen[k]) {
                char m[200];
                std::snprintf(m, sizeof m, "%s %d: the traceback walk failed (%s)", what, name_idx ? name_idx[k] : k,
                              r.err == WALK_OVERRUN ? "more than n + m operations" : "a cell outside the trace buffer");
                report_error(m);
                return -1;
            }
            if (amode == AM_LOCAL && r.score <= 0) sink.set_empty(k);
            else sink.set(k, r.score, r.bi, r.ei + 1, r.bj, r.ej + 1, o.ops.data() + o.ops_off[s], r.nops);
            ++s;
        }
        lo = hi;
    }
    st.variant |= amode << 28;   // bits 28-29: the alignment mode (SW_MODE_*); the launches below them
    st.kernel_ms = t_fill_ms;
    st.total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    report_stats(st);
    return 0;
}

int matrix_score_device(const sw_matrix* mx, const unsigned char* d_arena, const int64_t* a_off, const int* alen,
                        const int64_t* b_off, const int* blen, int npairs, int gap_init, int gap_ext, int* d_scores,
                        bool a_on_lanes, int amode) {
    if (!gaps_ok(gap_init, gap_ext)) return -1;
    MatCtx* c = get_mctx();
    if (!c) return -1;
    std::vector<DevSeq> act;
    for (int k = 0; k < npairs; ++k)
        if (alen[k] > 0 && blen[k] > 0) act.push_back(DevSeq{a_off[k], b_off[k], alen[k], blen[k], k});
    return launch(c, mx, d_arena, act, gap_init, gap_ext, d_scores, npairs, a_on_lanes, amode);
}

int profile_score_device(const sw_profile* pf, const unsigned char* d_arena, const int64_t* b_off, const int* blen, int nseq,
                         int gap_init, int gap_ext, int* d_scores, int amode) {
    if (!gaps_ok(gap_init, gap_ext)) return -1;
    MatCtx* c = get_mctx();
    if (!c) return -1;
    std::vector<DevSeq> act;
    for (int k = 0; k < nseq; ++k)
        if (blen[k] > 0) act.push_back(DevSeq{0, b_off[k], pf->n, blen[k], k});
    return launch(c, &pf->alpha, d_arena, act, gap_init, gap_ext, d_scores, nseq, true, amode, -1, pf);
}

int profile_align_device(const sw_profile* pf, const unsigned char* d_arena, const int64_t* b_off, const int* blen,
                         const int* name_idx, int nseq, int gap_init, int gap_ext, const char* what, AlignSink& sink,
                         int amode) {
    const std::vector<int64_t> a_off((size_t)nseq, 0);
    const std::vector<int> alen((size_t)nseq, pf->n);
    return matrix_align_device(&pf->alpha, d_arena, a_off.data(), alen.data(), b_off, blen, name_idx, nseq, gap_init, gap_ext,
                               what, sink, amode, -1, pf);
}

// ---- translated search, host side (XLATE above) ----

// Six items a pair, one a non-empty frame, out_idx = 6 * pair + frame index; launch orders them longest first by
// n * m and sizes the scratch, W and the cells from residues.  The empty frames and queries are answered here.
int translated_score_device(const sw_matrix* mx, const Translated& xl, const unsigned char* d_arena, const int64_t* a_off,
                            const int* alen, const int64_t* d_off, const int* dlen, int npairs, int gap_init, int gap_ext,
                            int amode, int* scores_out) {
    if (!gaps_ok(gap_init, gap_ext)) return -1;
    if (npairs > (1 << 30) / 6) {
        report_error("translated scoring: more than 2^30 / 6 pairs or records in one call");
        return -1;
    }
    MatCtx* c = get_mctx();
    if (!c) return -1;
    const int nscores = 6 * npairs;
    std::vector<DevSeq> act;
    for (int k = 0; k < npairs; ++k)
        for (int f = 0; f < 6 && alen[k] > 0; ++f) {
            const int m = frame_residues(dlen[k], f);
            if (m > 0) act.push_back(DevSeq{a_off[k], d_off[k] + frame_region(dlen[k], f), alen[k], m, 6 * k + f, f >= 3 ? 1 : 0});
        }
    if (ensure(c, B_SCORES, (size_t)std::max(nscores, 1) * sizeof(int))) return -1;
    if (launch(c, mx, d_arena, act, gap_init, gap_ext, (int*)c->buf[B_SCORES], nscores, true, amode, -1, nullptr, &xl)) return -1;
    if (nscores) MCHK(hipMemcpy(scores_out, c->buf[B_SCORES], (size_t)nscores * sizeof(int), hipMemcpyDeviceToHost));
    if (amode != AM_LOCAL)
        for (int k = 0; k < npairs; ++k)
            for (int f = 0; f < 6; ++f) {
                const int m = frame_residues(dlen[k], f);
                if (alen[k] == 0 || m == 0) scores_out[6 * k + f] = mode_empty_score(alen[k], m, gap_init, gap_ext, amode);
            }
    return 0;
}

int translated_align_device(const sw_matrix* mx, const Translated& xl, const unsigned char* d_arena, const int64_t* a_off,
                            const int* alen, const int64_t* d_off, const int* dlen, const int* fidx, const int* name_idx,
                            int npairs, int gap_init, int gap_ext, const char* what, AlignSink& sink, int amode) {
    std::vector<int64_t> b_off((size_t)npairs);
    std::vector<int> blen((size_t)npairs), minus((size_t)npairs);
    for (int k = 0; k < npairs; ++k) {
        b_off[(size_t)k] = d_off[k] + frame_region(dlen[k], fidx[k]);
        blen[(size_t)k] = frame_residues(dlen[k], fidx[k]);
        minus[(size_t)k] = fidx[k] >= 3 ? 1 : 0;
    }
    Translated x = xl;
    x.minus = minus.data();
    return matrix_align_device(mx, d_arena, a_off, alen, b_off.data(), blen.data(), name_idx, npairs, gap_init, gap_ext, what,
                               sink, amode, -1, nullptr, &x);
}

}  // namespace swmi

using namespace swmi;

extern "C" {

int sw_score_matrix_batch(const sw_matrix* mx, const unsigned char* const* a, const int* alen,
                          const unsigned char* const* b, const int* blen, int npairs, int gap_init, int gap_ext,
                          int* scores_out) {
    if (!mx || npairs < 0 || (npairs > 0 && (!a || !alen || !b || !blen || !scores_out))) {
        report_error("sw_score_matrix_batch: invalid arguments");
        return -1;
    }
    if (npairs == 0) return 0;
    return score_host(mx, a, alen, b, blen, npairs, gap_init, gap_ext, scores_out);
}

int sw_score_matrix(const sw_matrix* mx, const unsigned char* seq1, const unsigned char* seq2, int n, int m,
                    int gap_init, int gap_ext) {
    if (!mx || n < 0 || m < 0) {
        report_error("sw_score_matrix: invalid arguments");
        return -1;
    }
    int out = 0;
    if (score_host(mx, &seq1, &n, &seq2, &m, 1, gap_init, gap_ext, &out)) return -1;
    return out;
}

// sw_align_matrix_batch and sw_align_matrix_long: the checks, the upload, then the traced launches of
// whole pairs or (long_pairs; 2: on many waves, sw_align_matrix_long_coop) the checkpointed traceback
static int align_host(const char* fn, int long_pairs, const sw_matrix* mx, const unsigned char* const* a, const int* alen,
                      const unsigned char* const* b, const int* blen, int npairs, int gap_init, int gap_ext,
                      sw_alignment* out, unsigned* cigar, long long cigar_cap, long long* cigar_used, int amode = SW_MODE_LOCAL,
                      int band = -1) {
    if (align_check(fn, mx, a, alen, b, blen, npairs, gap_init, gap_ext, out, cigar, cigar_cap, cigar_used)) return -1;
    AlignSink sink{out, {}};
    if (npairs == 0) return sink.finish(cigar, cigar_cap, cigar_used);
    // the long path in a mode: the range refusal before any device work
    if (long_pairs && align_long_mode_check(fn, amode, alen, blen, nullptr, npairs, gap_init, gap_ext, "pair")) return -1;
    MatCtx* c = get_mctx();
    if (!c) return -1;
    // the sequences of the pairs with both lengths > 0, as score_host lays them out
    std::vector<int64_t> a_off((size_t)npairs, 0), b_off((size_t)npairs, 0);
    size_t total = 0;
    for (int k = 0; k < npairs; ++k) {
        if (alen[k] == 0 || blen[k] == 0) continue;
        a_off[(size_t)k] = (int64_t)total;
        total += ((size_t)alen[k] + 15) / 16 * 16;
        b_off[(size_t)k] = (int64_t)total;
        total += ((size_t)blen[k] + 15) / 16 * 16;
    }
    std::vector<unsigned char> arena(total);
    for (int k = 0; k < npairs; ++k) {
        if (alen[k] == 0 || blen[k] == 0) continue;
        std::memcpy(arena.data() + a_off[(size_t)k], a[k], (size_t)alen[k]);
        std::memcpy(arena.data() + b_off[(size_t)k], b[k], (size_t)blen[k]);
    }
    if (ensure(c, B_ARENA, total)) return -1;
    // (synchronous: a refusal below returns before anything is launched or waited for)
    if (total) MCHK(hipMemcpy(c->buf[B_ARENA], arena.data(), total, hipMemcpyHostToDevice));
    if (long_pairs ? matrix_align_long_device(mx, (const unsigned char*)c->buf[B_ARENA], a_off.data(), alen, b_off.data(), blen,
                                              nullptr, npairs, gap_init, gap_ext, "pair", sink, long_pairs == 2, amode)
                   : matrix_align_device(mx, (const unsigned char*)c->buf[B_ARENA], a_off.data(), alen, b_off.data(), blen,
                                         nullptr, npairs, gap_init, gap_ext, "pair", sink, amode, band))
        return -1;
    return sink.finish(cigar, cigar_cap, cigar_used);
}

int sw_score_matrix_batch_band(const sw_matrix* mx, const unsigned char* const* a, const int* alen,
                               const unsigned char* const* b, const int* blen, int npairs, int gap_init, int gap_ext,
                               int mode, int band, int* scores_out) {
    if (!mx || npairs < 0 || (npairs > 0 && (!a || !alen || !b || !blen || !scores_out))) {
        report_error("sw_score_matrix_batch_band: invalid arguments");
        return -1;
    }
    if (!mode_ok("sw_score_matrix_batch_band", mode) || !band_ok("sw_score_matrix_batch_band", band)) return -1;
    if (npairs == 0) return 0;
    return score_host(mx, a, alen, b, blen, npairs, gap_init, gap_ext, scores_out, mode, band);
}

int sw_align_matrix_batch_band(const sw_matrix* mx, const unsigned char* const* a, const int* alen,
                               const unsigned char* const* b, const int* blen, int npairs, int gap_init, int gap_ext,
                               int mode, int band, sw_alignment* out, unsigned* cigar, long long cigar_cap,
                               long long* cigar_used) {
    if (!mode_ok("sw_align_matrix_batch_band", mode) || !band_ok("sw_align_matrix_batch_band", band)) return -1;
    return align_host("sw_align_matrix_batch_band", 0, mx, a, alen, b, blen, npairs, gap_init, gap_ext, out, cigar,
                      cigar_cap, cigar_used, mode, band);
}

int sw_score_matrix_batch_mode(const sw_matrix* mx, const unsigned char* const* a, const int* alen,
                               const unsigned char* const* b, const int* blen, int npairs, int gap_init, int gap_ext,
                               int mode, int* scores_out) {
    if (!mx || npairs < 0 || (npairs > 0 && (!a || !alen || !b || !blen || !scores_out))) {
        report_error("sw_score_matrix_batch_mode: invalid arguments");
        return -1;
    }
    if (!mode_ok("sw_score_matrix_batch_mode", mode)) return -1;
    if (npairs == 0) return 0;
    return score_host(mx, a, alen, b, blen, npairs, gap_init, gap_ext, scores_out, mode);
}

int sw_score_matrix_batch_coop(const sw_matrix* mx, const unsigned char* const* a, const int* alen,
                               const unsigned char* const* b, const int* blen, int npairs, int gap_init, int gap_ext,
                               int mode, int* scores_out) {
    if (!mx || npairs < 0 || (npairs > 0 && (!a || !alen || !b || !blen || !scores_out))) {
        report_error("sw_score_matrix_batch_coop: invalid arguments");
        return -1;
    }
    if (!mode_ok("sw_score_matrix_batch_coop", mode)) return -1;
    if (npairs == 0) return 0;
    return score_host(mx, a, alen, b, blen, npairs, gap_init, gap_ext, scores_out, mode, -1, true);
}

int sw_matrix_coop_plan(int n, int m, int mode, sw_coop_plan* out) {
    if (n < 0 || m < 0 || n > MAT_MAX_SEQ || m > MAT_MAX_SEQ || !out) {
        report_error("sw_matrix_coop_plan: invalid arguments");
        return -1;
    }
    if (!mode_ok("sw_matrix_coop_plan", mode)) return -1;
    sw_coop_plan p{0, 0, 0, 0, 0};
    if (n > 0 && m > 0) {
        const long long budget = sw_get_option("coop_mb") << 20;
        const int wi = coop_choose_w(&n, &m, 1, mode, budget, "pair");
        if (wi < 0) return -1;
        CoopShape s{};
        coop_shape(n, m, mode, wi, budget, s, nullptr);
        p.W = W_OF[wi];
        p.strips = (int)s.strips;
        p.swap = s.swap;
        p.edge_bytes = s.edge_bytes;
        p.items = s.strips;
    }
    *out = p;
    return 0;
}

int sw_align_matrix_batch_mode(const sw_matrix* mx, const unsigned char* const* a, const int* alen,
                               const unsigned char* const* b, const int* blen, int npairs, int gap_init, int gap_ext,
                               int mode, sw_alignment* out, unsigned* cigar, long long cigar_cap, long long* cigar_used) {
    if (!mode_ok("sw_align_matrix_batch_mode", mode)) return -1;
    return align_host("sw_align_matrix_batch_mode", 0, mx, a, alen, b, blen, npairs, gap_init, gap_ext, out, cigar,
                      cigar_cap, cigar_used, mode);
}

int sw_align_matrix_batch(const sw_matrix* mx, const unsigned char* const* a, const int* alen,
                          const unsigned char* const* b, const int* blen, int npairs, int gap_init, int gap_ext,
                          sw_alignment* out, unsigned* cigar, long long cigar_cap, long long* cigar_used) {
    return align_host("sw_align_matrix_batch", 0, mx, a, alen, b, blen, npairs, gap_init, gap_ext, out, cigar, cigar_cap,
                      cigar_used);
}

int sw_align_matrix_long(const sw_matrix* mx, const unsigned char* const* a, const int* alen,
                         const unsigned char* const* b, const int* blen, int npairs, int gap_init, int gap_ext,
                         sw_alignment* out, unsigned* cigar, long long cigar_cap, long long* cigar_used) {
    return align_host("sw_align_matrix_long", 1, mx, a, alen, b, blen, npairs, gap_init, gap_ext, out, cigar, cigar_cap,
                      cigar_used);
}

int sw_align_matrix_long_coop(const sw_matrix* mx, const unsigned char* const* a, const int* alen,
                              const unsigned char* const* b, const int* blen, int npairs, int gap_init, int gap_ext,
                              sw_alignment* out, unsigned* cigar, long long cigar_cap, long long* cigar_used) {
    return align_host("sw_align_matrix_long_coop", 2, mx, a, alen, b, blen, npairs, gap_init, gap_ext, out, cigar, cigar_cap,
                      cigar_used);
}

// the long path in a mode; local mode through them is the calls above
int sw_align_matrix_long_mode(const sw_matrix* mx, const unsigned char* const* a, const int* alen,
                              const unsigned char* const* b, const int* blen, int npairs, int gap_init, int gap_ext,
                              int mode, sw_alignment* out, unsigned* cigar, long long cigar_cap, long long* cigar_used) {
    if (!mode_ok("sw_align_matrix_long_mode", mode)) return -1;
    if (mode == SW_MODE_LOCAL)
        return sw_align_matrix_long(mx, a, alen, b, blen, npairs, gap_init, gap_ext, out, cigar, cigar_cap, cigar_used);
    return align_host("sw_align_matrix_long_mode", 1, mx, a, alen, b, blen, npairs, gap_init, gap_ext, out, cigar, cigar_cap,
                      cigar_used, mode);
}

int sw_align_matrix_long_coop_mode(const sw_matrix* mx, const unsigned char* const* a, const int* alen,
                                   const unsigned char* const* b, const int* blen, int npairs, int gap_init, int gap_ext,
                                   int mode, sw_alignment* out, unsigned* cigar, long long cigar_cap, long long* cigar_used) {
    if (!mode_ok("sw_align_matrix_long_coop_mode", mode)) return -1;
    if (mode == SW_MODE_LOCAL)
        return sw_align_matrix_long_coop(mx, a, alen, b, blen, npairs, gap_init, gap_ext, out, cigar, cigar_cap, cigar_used);
    return align_host("sw_align_matrix_long_coop_mode", 2, mx, a, alen, b, blen, npairs, gap_init, gap_ext, out, cigar,
                      cigar_cap, cigar_used, mode);
}

int sw_align_long_coop_plan(int n, int m, sw_align_coop_plan* out) {
    if (n < 0 || m < 0 || n > MAT_MAX_SEQ || m > MAT_MAX_SEQ || !out) {
        report_error("sw_align_long_coop_plan: invalid arguments");
        return -1;
    }
    long long ckpt_budget = 0;
    if (align_ckpt_budget(&ckpt_budget)) return -1;
    return align_long_coop_plan(n, m, sw_get_option("trace_mb") << 20, ckpt_budget, (int)sw_get_option("long_window"), "pair", 0,
                                out);
}

int sw_align_long_plan(int n, int m, sw_align_plan* out) {
    if (n < 0 || m < 0 || n > MAT_MAX_SEQ || m > MAT_MAX_SEQ || !out) {
        report_error("sw_align_long_plan: invalid arguments");
        return -1;
    }
    long long ckpt_budget = 0;
    if (align_ckpt_budget(&ckpt_budget)) return -1;
    return align_long_plan(n, m, sw_get_option("trace_mb") << 20, ckpt_budget, "pair", 0, out);
}

// The sequences of a profile call in one arena, as score_host lays seq2 out (the profile has no bytes there).
static int profile_upload(MatCtx* c, const unsigned char* const* seqs, const int* lens, int nseq, std::vector<int64_t>& b_off) {
    b_off.assign((size_t)nseq, 0);
    size_t total = 0;
    for (int k = 0; k < nseq; ++k) {
        b_off[(size_t)k] = (int64_t)total;
        total += ((size_t)lens[k] + 15) / 16 * 16;
    }
    std::vector<unsigned char> arena(total);
    for (int k = 0; k < nseq; ++k)
        if (lens[k] > 0) std::memcpy(arena.data() + b_off[(size_t)k], seqs[k], (size_t)lens[k]);
    if (ensure(c, B_ARENA, total)) return -1;
    if (total) MCHK(hipMemcpy(c->buf[B_ARENA], arena.data(), total, hipMemcpyHostToDevice));
    return 0;
}

int sw_score_profile_batch(const sw_profile* pf, const unsigned char* const* seqs, const int* lens, int nseq, int gap_init,
                           int gap_ext, int mode, int* scores_out) {
    if (profile_check("sw_score_profile_batch", pf, seqs, lens, nseq, gap_init, gap_ext, mode)) return -1;
    if (nseq > 0 && !scores_out) {
        report_error("sw_score_profile_batch: invalid arguments");
        return -1;
    }
    if (nseq == 0) return 0;
    MatCtx* c = get_mctx();
    if (!c) return -1;
    std::vector<int64_t> b_off;
    if (profile_upload(c, seqs, lens, nseq, b_off) || ensure(c, B_SCORES, (size_t)nseq * sizeof(int))) return -1;
    if (profile_score_device(pf, (const unsigned char*)c->buf[B_ARENA], b_off.data(), lens, nseq, gap_init, gap_ext,
                             (int*)c->buf[B_SCORES], mode))
        return -1;
    MCHK(hipMemcpy(scores_out, c->buf[B_SCORES], (size_t)nseq * sizeof(int), hipMemcpyDeviceToHost));
    if (mode != SW_MODE_LOCAL)   // empty sequences are answered on the host
        for (int k = 0; k < nseq; ++k)
            if (lens[k] == 0) scores_out[k] = mode_empty_score(pf->n, 0, gap_init, gap_ext, mode);
    return 0;
}

int sw_align_profile_batch(const sw_profile* pf, const unsigned char* const* seqs, const int* lens, int nseq, int gap_init,
                           int gap_ext, int mode, sw_alignment* out, unsigned* cigar, long long cigar_cap,
                           long long* cigar_used) {
    if (profile_align_check("sw_align_profile_batch", pf, seqs, lens, nseq, gap_init, gap_ext, mode, out, cigar, cigar_cap,
                            cigar_used))
        return -1;
    AlignSink sink{out, {}};
    if (nseq == 0) return sink.finish(cigar, cigar_cap, cigar_used);
    MatCtx* c = get_mctx();
    if (!c) return -1;
    std::vector<int64_t> b_off;
    if (profile_upload(c, seqs, lens, nseq, b_off)) return -1;
    if (profile_align_device(pf, (const unsigned char*)c->buf[B_ARENA], b_off.data(), lens, nullptr, nseq, gap_init, gap_ext,
                             "sequence", sink, mode))
        return -1;
    return sink.finish(cigar, cigar_cap, cigar_used);
}

// The sequences of a translated call in one arena: the query then the DNA of every pair, as score_host lays pairs out.
static int translated_upload(MatCtx* c, const unsigned char* const* a, const int* alen, const unsigned char* const* dna,
                             const int* dlen, int npairs, std::vector<int64_t>& a_off, std::vector<int64_t>& d_off) {
    a_off.assign((size_t)npairs, 0);
    d_off.assign((size_t)npairs, 0);
    size_t total = 0;
    for (int k = 0; k < npairs; ++k) {
        a_off[(size_t)k] = (int64_t)total;
        total += ((size_t)alen[k] + 15) / 16 * 16;
        d_off[(size_t)k] = (int64_t)total;
        total += ((size_t)dlen[k] + 15) / 16 * 16;
    }
    std::vector<unsigned char> arena(total);
    for (int k = 0; k < npairs; ++k) {
        if (alen[k] > 0) std::memcpy(arena.data() + a_off[(size_t)k], a[k], (size_t)alen[k]);
        if (dlen[k] > 0) std::memcpy(arena.data() + d_off[(size_t)k], dna[k], (size_t)dlen[k]);
    }
    if (ensure(c, B_ARENA, total)) return -1;
    if (total) MCHK(hipMemcpy(c->buf[B_ARENA], arena.data(), total, hipMemcpyHostToDevice));
    return 0;
}

int sw_score_matrix_translated_batch(const sw_matrix* mx, const unsigned char* const* a, const int* alen,
                                     const unsigned char* const* dna, const int* dlen, int npairs, int gap_init,
                                     int gap_ext, int mode, const unsigned char* code64, int* scores_out) {
    const char* fn = "sw_score_matrix_translated_batch";
    if (npairs > 0 && !scores_out) {
        report_error("sw_score_matrix_translated_batch: invalid arguments (a null pointer)");
        return -1;
    }
    Translated xl;
    if (translated_check(fn, mx, a, alen, dna, dlen, nullptr, npairs, gap_init, gap_ext, mode, code64, &xl)) return -1;
    if (npairs == 0) return 0;
    MatCtx* c = get_mctx();
    if (!c) return -1;
    std::vector<int64_t> a_off, d_off;
    if (translated_upload(c, a, alen, dna, dlen, npairs, a_off, d_off)) return -1;
    return translated_score_device(mx, xl, (const unsigned char*)c->buf[B_ARENA], a_off.data(), alen, d_off.data(), dlen, npairs,
                                   gap_init, gap_ext, mode, scores_out);
}

int sw_align_matrix_translated_batch(const sw_matrix* mx, const unsigned char* const* a, const int* alen,
                                     const unsigned char* const* dna, const int* dlen, const int* frames, int npairs,
                                     int gap_init, int gap_ext, int mode, const unsigned char* code64, sw_alignment* out,
                                     unsigned* cigar, long long cigar_cap, long long* cigar_used) {
    const char* fn = "sw_align_matrix_translated_batch";
    if (cigar_cap < 0 || !cigar_used || (cigar_cap > 0 && !cigar) || (npairs > 0 && (!out || !frames))) {
        report_error("sw_align_matrix_translated_batch: invalid arguments (a null pointer)");
        return -1;
    }
    Translated xl;
    if (translated_check(fn, mx, a, alen, dna, dlen, frames, npairs, gap_init, gap_ext, mode, code64, &xl)) return -1;
    AlignSink sink{out, {}};
    if (npairs == 0) return sink.finish(cigar, cigar_cap, cigar_used);
    MatCtx* c = get_mctx();
    if (!c) return -1;
    std::vector<int64_t> a_off, d_off;
    if (translated_upload(c, a, alen, dna, dlen, npairs, a_off, d_off)) return -1;
    std::vector<int> fidx((size_t)npairs);
    for (int k = 0; k < npairs; ++k) fidx[(size_t)k] = frame_index(frames[k]);
    if (translated_align_device(mx, xl, (const unsigned char*)c->buf[B_ARENA], a_off.data(), alen, d_off.data(), dlen, fidx.data(),
                                nullptr, npairs, gap_init, gap_ext, "sw_align_matrix_translated_batch: pair", sink, mode))
        return -1;
    return sink.finish(cigar, cigar_cap, cigar_used);
}

void sw_last_align_ms(float* fill_ms, float* walk_ms) {
    if (fill_ms) *fill_ms = t_fill_ms;
    if (walk_ms) *walk_ms = t_walk_ms;
}

void sw_last_align_long_ms(float* locate_ms, float* strip_ms, float* walk_ms, int* rounds) {
    if (locate_ms) *locate_ms = t_locate_ms;
    if (strip_ms) *strip_ms = t_fill_ms - t_locate_ms;
    if (walk_ms) *walk_ms = t_walk_ms;
    if (rounds) *rounds = t_rounds;
}

}  // extern "C"
