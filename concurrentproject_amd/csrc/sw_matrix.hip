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
#include "sw_device.h"
#include "sw_matrix_host.h"
#include "../../include/algoGPU.h"

#include <algorithm>
#include <chrono>
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

struct MatPair {
    uint64_t col_off;   // the sequence across the lanes
    uint64_t row_off;   // the sequence that streams
    int n, m;           // columns, rows (> 0)
    int out_idx;
    int swapped;        // 1: the columns are seq2 (table 1)
};

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
};
static_assert(sizeof(MatArgs) <= 4096, "kernel arguments");
static_assert(MAT_TAB_BYTES % 4 == 0, "table words");

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

template <int W>
struct MStrip {
    int cb[W], tb[W];                       // LDS offset of the column's table row / bias
    int hgA[W], hgB[W], eh[W], r[W], fh[W]; // DP state, as Strip (sw_kernels.hip)
    int L0, M, IOH, IOE, IOR;

    __device__ __forceinline__ void setup(const MatArgs& a, const MatPair& pd, int strip, int lane,
                                          const unsigned char* s_code) {
        constexpr int SW = 64 * W;
        const int go = a.gap_init, ge = a.gap_ext;
        const unsigned char* colseq = a.seq + pd.col_off;
        const int tbase = pd.swapped ? MAT_TAB_BYTES : 0;
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
#pragma unroll
        for (int p = 0; p < W; ++p) {   // everything starts at the border (H = E = F = 0)
            hgA[p] = -go; hgB[p] = -go; eh[p] = -ge; fh[p] = -ge; r[p] = a.k;
        }
        L0 = -go; IOH = -go; IOE = -ge; IOR = a.k;
    }

    // One anti-diagonal step (Strip::step with the score from the LDS table).
    __device__ __forceinline__ void step(int (&hgCur)[W], const int (&hgPrev)[W], const bool l63, const int go,
                                         const int ge, const signed char* s_tab) {
        const int ioh = dpp_rol1(IOH), ioe = dpp_rol1(IOE), ior = dpp_rol1(IOR);
        const int hgL0 = dpp_shr1(IOH, hgPrev[W - 1]);
        const int ehL0 = dpp_shr1(IOE, eh[W - 1]);
        const int rL0 = dpp_shr1(IOR, r[W - 1]);
        // the W lookups first (they need only the row codes): their LDS latencies overlap
        int sv[W];
#pragma unroll
        for (int p = 0; p < W; ++p) sv[p] = (int)s_tab[cb[p] + (p > 0 ? r[p - 1] : rL0)];   // ds_read_i8
#pragma unroll
        for (int p = W - 1; p >= 0; --p) {
            const int q = p > 0 ? p - 1 : 0;
            const int hgL = p > 0 ? hgPrev[q] : hgL0;
            const int ehL = p > 0 ? eh[q] : ehL0;
            const int rL = p > 0 ? r[q] : rL0;
            const int hgD = p > 0 ? hgCur[q] : L0;
            const int t = hgD + sv[p] + tb[p];           // H[i-1][j-1] + s(q_j, d_i)
            const int E = max3i(ehL, hgL, 0);            // clamped E
            const int F = max3i(fh[p], hgPrev[p], 0);    // clamped F
            const int H = vmax3(t, E, F);
            M = max(M, t);
            hgCur[p] = H - go;
            eh[p] = E - ge;
            fh[p] = F - ge;
            r[p] = rL;
        }
        L0 = hgL0;
        IOH = l63 ? hgCur[W - 1] : ioh;   // lane 63 <- this step's right-edge output
        IOE = l63 ? eh[W - 1] : ioe;
        IOR = ior;
    }

    __device__ __forceinline__ void run(const bool l63, const int go, const int ge, const signed char* s_tab) {
#pragma unroll 2
        for (int s = 0; s < MAT_C; s += 2) {
            step(hgA, hgB, l63, go, ge, s_tab);
            step(hgB, hgA, l63, go, ge, s_tab);
        }
    }
};

__device__ __forceinline__ unsigned mat_fetch_raw(const __amdgpu_buffer_rsrc_t row_rsrc, int k0, int lane, int m) {
    const int row = k0 + lane;
    return __builtin_amdgcn_raw_buffer_load_b8(row_rsrc, row < m ? (unsigned)row : OOR, 0, 0);
}
__device__ __forceinline__ u32x2 mat_fetch_edge(const __amdgpu_buffer_rsrc_t scr_rsrc, int k0, int lane, int m) {
    const int row = k0 + lane;
    return __builtin_amdgcn_raw_buffer_load_b64(scr_rsrc, row < m ? (unsigned)row * 8u : OOR, 0, AUX_SC1);
}

// All strips of one pair on this wave; scr: the wave's scratch (at least m entries when the pair has
// more than one strip).
template <int W>
__device__ void matrix_pair(const MatArgs& a, const MatPair& pd, const int lane, uint2* scr,
                            const signed char* s_tab, const unsigned char* s_code) {
    constexpr int SW = 64 * W, C = MAT_C;
    const int m = pd.m;
    const int go = a.gap_init, ge = a.gap_ext;
    const bool l63 = lane == 63;
    const int strips = (pd.n + SW - 1) / SW;
    const __amdgpu_buffer_rsrc_t row_rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(a.seq + pd.row_off), 0, m, RSRC_FLAGS);
    // a single strip never touches the scratch: a resource of no bytes drops every access
    const __amdgpu_buffer_rsrc_t scr_rsrc =
        __builtin_amdgcn_make_buffer_rsrc(scr, 0, strips > 1 ? (int)((unsigned)m * 8u) : 0, RSRC_FLAGS);
    const int nchunks = (m + SW - 1 + C - 1) / C;
    MStrip<W> S;
    S.M = 0;
    for (int strip = 0; strip < strips; ++strip) {
        S.setup(a, pd, strip, lane, s_code);
        const bool has_in = strip > 0;
        const bool has_out = strip < strips - 1;
        unsigned raw_nxt = mat_fetch_raw(row_rsrc, 0, lane, m);
        u32x2 g_nxt = has_in ? mat_fetch_edge(scr_rsrc, 0, lane, m) : u32x2{0u, 0u};
        for (int c = 0; c < nchunks; ++c) {
            const int k0 = c * C;
            const unsigned raw = raw_nxt;
            const u32x2 g = g_nxt;
            // the next chunk's rows in flight while this chunk computes
            raw_nxt = mat_fetch_raw(row_rsrc, k0 + C, lane, m);
            if (has_in) g_nxt = mat_fetch_edge(scr_rsrc, k0 + C, lane, m);
            const bool live = k0 + lane < m;
            S.IOR = live ? (int)s_code[raw & 0xFFu] : a.k;
            S.IOH = has_in && live ? (int)g.x : -go;
            S.IOE = has_in && live ? (int)g.y : -ge;
            S.run(l63, go, ge, s_tab);
            if (has_out) {   // lane l holds the right edge of row k0 + l - (SW - 1)
                const int row_out = k0 + lane - (SW - 1);
                const bool st = row_out >= 0 && row_out < m;
                __builtin_amdgcn_raw_buffer_store_b64(u32x2{(unsigned)S.IOH, (unsigned)S.IOE}, scr_rsrc,
                                                      st ? (unsigned)row_out * 8u : OOR, 0, AUX_SC1);
            }
        }
        // the next strip (or the next pair's) reads what this one stored
        if (has_out) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
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

template <int W>
__global__ void __launch_bounds__(256) sw_matrix_kernel(MatArgs a) {
    __shared__ unsigned s_tabw[2 * MAT_TAB_BYTES / 4];
    __shared__ unsigned s_codew[64];
    for (int i = threadIdx.x; i < 2 * MAT_TAB_BYTES / 4; i += 256) s_tabw[i] = a.tab[i];
    if (threadIdx.x < 64) s_codew[threadIdx.x] = a.code[threadIdx.x];
    __syncthreads();
    const signed char* s_tab = reinterpret_cast<const signed char*>(s_tabw);
    const unsigned char* s_code = reinterpret_cast<const unsigned char*>(s_codew);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    uint2* scr = a.scratch + (uint64_t)wave * (uint64_t)a.scratch_rows;
    for (;;) {
        unsigned item = 0;
        if (lane == 0) item = atomicAdd(&a.ctrl->next_item, 1u);
        item = __builtin_amdgcn_readfirstlane(item);
        if ((int)item >= a.npairs) return;
        const MatPair raw = a.pairs[item];
        MatPair pd;   // every field provably wave-uniform (buffer descriptors live in SGPRs)
        pd.col_off = uniform64(raw.col_off);
        pd.row_off = uniform64(raw.row_off);
        pd.n = __builtin_amdgcn_readfirstlane(raw.n);
        pd.m = __builtin_amdgcn_readfirstlane(raw.m);
        pd.out_idx = __builtin_amdgcn_readfirstlane(raw.out_idx);
        pd.swapped = __builtin_amdgcn_readfirstlane(raw.swapped);
        matrix_pair<W>(a, pd, lane, scr, s_tab, s_code);
    }
}

// ---- host ------------------------------------------------------------------------------------

#define MCHK(expr)                                                                           \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) {                                                              \
            char m_[256];                                                                    \
            std::snprintf(m_, sizeof m_, "%s failed: %s", #expr, hipGetErrorString(e_));     \
            report_error(m_);                                                                \
            return -1;                                                                       \
        }                                                                                    \
    } while (0)

// device memory and a stream per (thread, device), as the engine's own context (sw_engine.hip)
struct MatCtx {
    int cus = 256;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    void* buf[5] = {};      // pairs, ctrl, scratch, arena, scores
    size_t cap[5] = {};
    int wgs[4] = {0, 0, 0, 0};   // resident workgroups per CU per W variant
};
enum { B_PAIRS = 0, B_CTRL, B_SCRATCH, B_ARENA, B_SCORES };
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
        hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess) {
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

constexpr int W_OF[4] = {1, 2, 4, 8};

const void* kernel_of(int wi) {
    switch (wi) {
        case 0: return (const void*)sw_matrix_kernel<1>;
        case 1: return (const void*)sw_matrix_kernel<2>;
        case 2: return (const void*)sw_matrix_kernel<4>;
        default: return (const void*)sw_matrix_kernel<8>;
    }
}

// steps of one pair at W columns per lane with n columns, times an issue-slot estimate of a step
// (about 9 instructions a cell and 8 a step for the DPP moves and the I/O rotation)
long long pair_cost(long long n, long long m, int W) {
    const long long SW = 64LL * W;
    const long long strips = (n + SW - 1) / SW;
    const long long chunks = (m + SW - 1 + MAT_C - 1) / MAT_C;
    return strips * chunks * MAT_C * (9LL * W + 8);
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
};

// act: the pairs to launch (both lengths > 0); d_scores[idx] receives each score, every other
// entry of d_scores[0, nscores) is zeroed.
int launch(MatCtx* c, const sw_matrix* mx, const unsigned char* d_arena, std::vector<DevSeq>& act, int gap_init,
           int gap_ext, int* d_scores, int nscores, bool a_on_lanes) {
    const auto t0 = std::chrono::steady_clock::now();
    sw_stats st{};
    st.mode = MODE_MATRIX;
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
            const long long ca = pair_cost(p.alen, p.blen, W_OF[k]);
            cost += a_on_lanes ? ca : std::min(ca, pair_cost(p.blen, p.alen, W_OF[k]));
        }
        if (best < 0 || cost < best) {
            best = cost;
            wi = k;
        }
    }
    const int W = W_OF[wi], SW = 64 * W;
    // longest first: the waves claim in order
    std::stable_sort(act.begin(), act.end(), [](const DevSeq& x, const DevSeq& y) {
        return (long long)x.alen * x.blen > (long long)y.alen * y.blen;
    });
    std::vector<MatPair> pairs(act.size());
    long long scratch_rows = 0, cells = 0;
    for (size_t k = 0; k < act.size(); ++k) {
        const DevSeq& p = act[k];
        const bool swap = !a_on_lanes && pair_cost(p.blen, p.alen, W) < pair_cost(p.alen, p.blen, W);
        MatPair& d = pairs[k];
        d.col_off = (uint64_t)(swap ? p.b_off : p.a_off);
        d.row_off = (uint64_t)(swap ? p.a_off : p.b_off);
        d.n = swap ? p.blen : p.alen;
        d.m = swap ? p.alen : p.blen;
        d.out_idx = p.idx;
        d.swapped = swap ? 1 : 0;
        if (d.n > SW) scratch_rows = std::max<long long>(scratch_rows, d.m);
        cells += (long long)d.n * d.m;
    }
    if (c->wgs[wi] == 0) {
        int nb = 0;
        MCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel_of(wi), 256, 0));
        c->wgs[wi] = std::max(1, std::min(nb, 8));
    }
    long long blocks = sw_get_option("blocks");
    if (blocks <= 0) blocks = (long long)c->cus * c->wgs[wi];
    blocks = std::max<long long>(1, std::min<long long>(blocks, ((long long)act.size() + 3) / 4));
    // the scratch: a right-edge column per resident wave, at most 1 GiB in all
    scratch_rows = (scratch_rows + 63) / 64 * 64;
    if (scratch_rows > 0) blocks = std::max<long long>(1, std::min<long long>(blocks, (1LL << 30) / (scratch_rows * 8 * 4)));
    const size_t scratch_bytes = (size_t)scratch_rows * 8 * 4 * (size_t)blocks;
    if (ensure(c, B_PAIRS, pairs.size() * sizeof(MatPair)) || ensure(c, B_CTRL, sizeof(Ctrl)) ||
        ensure(c, B_SCRATCH, scratch_bytes))
        return -1;
    MCHK(hipMemcpyAsync(c->buf[B_PAIRS], pairs.data(), pairs.size() * sizeof(MatPair), hipMemcpyHostToDevice, c->stream));
    MCHK(hipMemsetAsync(c->buf[B_CTRL], 0, sizeof(Ctrl), c->stream));

    MatArgs a{};
    a.seq = d_arena;
    a.pairs = (const MatPair*)c->buf[B_PAIRS];
    a.ctrl = (Ctrl*)c->buf[B_CTRL];
    a.scores = d_scores;
    a.scratch = (uint2*)c->buf[B_SCRATCH];
    a.scratch_rows = scratch_rows;
    a.npairs = (int)pairs.size();
    a.nscores = nscores;
    a.gap_init = gap_init;
    a.gap_ext = gap_ext;
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

    MCHK(hipEventRecord(c->ev0, c->stream));
    const dim3 grid((unsigned)blocks), block(256);
    switch (wi) {
        case 0: hipLaunchKernelGGL(sw_matrix_kernel<1>, grid, block, 0, c->stream, a); break;
        case 1: hipLaunchKernelGGL(sw_matrix_kernel<2>, grid, block, 0, c->stream, a); break;
        case 2: hipLaunchKernelGGL(sw_matrix_kernel<4>, grid, block, 0, c->stream, a); break;
        default: hipLaunchKernelGGL(sw_matrix_kernel<8>, grid, block, 0, c->stream, a); break;
    }
    MCHK(hipGetLastError());
    MCHK(hipEventRecord(c->ev1, c->stream));
    MCHK(hipStreamSynchronize(c->stream));
    MCHK(hipEventElapsedTime(&st.kernel_ms, c->ev0, c->ev1));
    st.W = W;
    st.cells = cells;
    st.blocks = (int)blocks;
    st.waves_per_cu = 4 * c->wgs[wi];
    st.boundary_bytes = (long long)scratch_bytes;
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
               const int* blen, int npairs, int gap_init, int gap_ext, int* out) {
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
    if (launch(c, mx, (const unsigned char*)c->buf[B_ARENA], act, gap_init, gap_ext, (int*)c->buf[B_SCORES], npairs, false))
        return -1;
    MCHK(hipMemcpy(out, c->buf[B_SCORES], (size_t)npairs * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

}  // namespace

int matrix_score_device(const sw_matrix* mx, const unsigned char* d_arena, const int64_t* a_off, const int* alen,
                        const int64_t* b_off, const int* blen, int npairs, int gap_init, int gap_ext, int* d_scores,
                        bool a_on_lanes) {
    if (!gaps_ok(gap_init, gap_ext)) return -1;
    MatCtx* c = get_mctx();
    if (!c) return -1;
    std::vector<DevSeq> act;
    for (int k = 0; k < npairs; ++k)
        if (alen[k] > 0 && blen[k] > 0) act.push_back(DevSeq{a_off[k], b_off[k], alen[k], blen[k], k});
    return launch(c, mx, d_arena, act, gap_init, gap_ext, d_scores, npairs, a_on_lanes);
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

}  // extern "C"
