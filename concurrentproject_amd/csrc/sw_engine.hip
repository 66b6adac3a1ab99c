// sw_engine.hip -- C++ host layer of libswmi355.so: the drop-in C-ABI of
// include/algoGPU.h over the gfx950 strip kernel (sw_kernels.hip).
//
// Replaces the host drivers of the reference GPU engines
// (simpleGPU.cu:109-163, cudaLazy.cu:58-99, cudaSmithM.cu:128-189,
// SmithDiagonalGPUrefactored.cu:174-230).  Differences that are deliberate:
//   * one persistent launch per call instead of m+n-1 launches;
//   * no (m+1)(n+1) matrices: device state is O(n) per pair plus one strip
//     boundary column per strip (H-G_INIT, E-G_EXT per row);
//   * the max is reduced on the device; one int per pair comes back;
//   * every HIP call is checked; failures return -1 with sw_last_error();
//   * device memory and a non-blocking stream are cached per (thread, device).
#include "sw_internal.h"
#include "../../include/algoGPU.h"

#include <rccl/rccl.h>
#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <thread>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <vector>

namespace swmi {
namespace {

thread_local std::string t_err;
thread_local sw_stats t_stats{};

void set_err(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    t_err = buf;
}

#define HIPCHK(expr)                                                                   \
    do {                                                                               \
        hipError_t e_ = (expr);                                                        \
        if (e_ != hipSuccess) {                                                        \
            set_err("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return -1;                                                                 \
        }                                                                              \
    } while (0)

struct Params {
    int match = 1, mismatch = -1, gap_init = 1, gap_ext = 1;   // main.cpp:20-23
};

std::mutex g_param_mu;
Params g_params;

// ---- options (include/algoGPU.h "Tuning knobs") -----------------------------
// Every process-wide option once: X(key, default, lowest, highest, further test or nullptr, stored as 0 / 1).
// sw_set_option takes v in [lowest, highest] that passes the test; ANY: every value.
constexpr long long ANY_LO = INT64_MIN, ANY_HI = INT64_MAX;
bool opt_W_ok(long long v) { return v == 0 || v == 1 || v == 2 || v == 4 || v == 8; }
bool opt_C_ok(long long v) { return v == 0 || v == 16 || v == 32 || v == 64; }
bool opt_prio_ok(long long v) { return v <= 0 || v >= 6; }
bool opt_pow2_ok(long long v) { return (v & (v - 1)) == 0; }
#define SW_OPTIONS(X)                                                                                                 \
    X(W, 0, 0, 8, opt_W_ok, false)                                                                                    \
    X(C, 0, 0, 64, opt_C_ok, false)                                                                                   \
    X(bytes, 0, ANY_LO, ANY_HI, nullptr, true)                                                                        \
    X(timeout, 30, 1, 3600, nullptr, false)                                                                           \
    X(blocks, 0, 0, ANY_HI, nullptr, false)                                                                           \
    X(orient, 0, 0, 2, nullptr, false)                                                                                \
    X(mode, -1, -1, 5, nullptr, false)                                                                                \
    /* device buffer of 4 u64 per strip (tools only), 0 = off */                                                      \
    X(trace, 0, ANY_LO, ANY_HI, nullptr, false)                                                                       \
    /* MiB of trace memory a traced matrix launch may hold (sw_matrix.hip) */                                         \
    X(trace_mb, 1024, 1, 3072, nullptr, false)                                                                        \
    /* 1 = duo max3 through v_pk_maximum3_f16 when exact, 0 = u16 max only */                                         \
    X(duo16, 1, ANY_LO, ANY_HI, nullptr, true)                                                                        \
    /* 1 = flow2 streams row codes even when they fit in LDS (tests) */                                               \
    X(f2stream, 0, ANY_LO, ANY_HI, nullptr, true)                                                                     \
    /* flow2 one-pair group edges: -1 auto (rings above 1 GB of edges), 0 off, 1 on */                                \
    X(ring, -1, -1, 1, nullptr, false)                                                                                \
    /* rows per within-round ring: a power of two in [512, 2^20] */                                                   \
    X(ring_rows, 4096, 512, 1 << 20, opt_pow2_ok, false)                                                              \
    /* flow2 streamed kernel: workgroups per CU, 0 = auto, 1..F2_WGS_MAX */                                           \
    X(f2_wgs, 0, 0, F2_WGS_MAX, nullptr, false)                                                                       \
    /* flow2 columns per lane: 0 auto, 1, 2 (2: the linear-gap step only), 3 (flow3 ring mode: single long pairs    \
       and column slabs; auto there), 4 (four / five in that ring mode, one pair, every group in one round) */        \
    X(f2w, 0, 0, 4, nullptr, false)                                                                                   \
    /* int32 DNA batches on flow2, a pair per workgroup: -1 auto, 0 off, 1 forced */                                  \
    X(f2pwg, -1, -1, 1, nullptr, false)                                                                               \
    /* G_INIT == G_EXT: -1 auto (the linear-gap step), 0 = the affine step */                                         \
    X(linear, -1, -1, 0, nullptr, false)                                                                              \
    /* 1: staged W2 linear-gap launches on flow3 (sw_flow3.hip), 0: flow2 */                                          \
    X(f3, 1, 0, 1, nullptr, false)                                                                                    \
    /* 1: staged affine-step launches on flow3 (sw_flow3a_kernel), 0: flow2 */                                        \
    X(f3a, 1, 0, 1, nullptr, false)                                                                                   \
    /* 1: flow3 staged launches at C = 32 with half-chunk in-workgroup links (auto C: 32) */                          \
    X(f3hl, 1, 0, 1, nullptr, false)                                                                                  \
    /* 1: flow3 ring launches at C = 64 with half-chunk in-workgroup links */                                         \
    X(f3rhl, 0, 0, 1, nullptr, false)                                                                                 \
    /* 1: column slabs on flow3's ring kernel (sw_flow3rs_kernel), 0: flow2 */                                        \
    X(f3slab, 1, 0, 1, nullptr, false)                                                                                \
    /* 1: flow3 staged C = 32 half-chunk launches on the pool loops (slower) */                            \
    X(f3pool, 0, 0, 1, nullptr, false)                                                                                \
    /* 1: int32 batches on flow3's three-column ring step, a pair per workgroup (sw_flow3r3p / ra3p_kernel);         \
       0: flow2's pair-per-workgroup kernel */                                                                        \
    X(f3pwg, 1, ANY_LO, ANY_HI, nullptr, true)                                                                        \
    /* one pair on flow3's staged linear-gap kernel cut at a column and scored from both ends: -1 auto (pairs of     \
       F3_SPLIT_AUTO_N columns or more), 0 off, 1 whenever each half gets two strips */                               \
    X(f3split, -1, -1, 1, nullptr, false)                                                                             \
    /* 1: one pair over up to seven byte values on flow3's seven-letter kernels, 0: byte path */                      \
    X(hep, 1, 0, 1, nullptr, false)                                                                                   \
    /* 1: duo strip hand-offs in LDS when the wrap buffer fits, 0: HBM granules */                                    \
    X(duo_lds, 1, 0, 1, nullptr, false)                                                                               \
    /* duo LDS kernel row codes from an LDS table: 1 for one-pass batches, 2 whenever it fits, 0 carried by DPP */    \
    X(duo_tab, 1, 0, 2, nullptr, false)                                                                               \
    /* 1: duo strip roles complementary per SIMD across a CU's workgroups */                                          \
    X(duo_roles, 1, 0, 1, nullptr, false)                                                                             \
    /* 1: byte batches on the duo kernels (RAW penalty), 0: byte strip kernels */                                     \
    X(duo_raw, 1, 0, 1, nullptr, false)                                                                               \
    /* duo LDS kernel: -1 auto, 0 off, k in 6..20: a CU's workgroups alternate priority every 2^k ticks (10 ns) */    \
    X(duo_prio, -1, -1, 20, opt_prio_ok, false)                                                                       \
    /* 1: exported slab buffers may fall back to plain device memory */                                               \
    X(slab_plain, 0, 0, 1, nullptr, false)                                                                            \
    /* tests only: flow2's compute waves skip this item (-1 = none) */                                                \
    X(stall_item, -1, -1, ANY_HI, nullptr, false)
// The keys of the cooperative entry points, sw_score_matrix_batch_coop and sw_align_matrix_long_coop (sw_matrix.hip),
// set and read like the ones above but documented with those entry points and not listed by sw_option_name, whose
// list is the "Tuning knobs" of the header.
#define SW_OPTIONS_COOP(X)                                                                                            \
    /* MiB of edge columns a cooperative matrix launch may hold */                                                    \
    X(coop_mb, 1024, 1, 3072, nullptr, false)                                                                         \
    /* 1: the edge columns are filled with 0x3F bytes before every cooperative launch (tests) */                      \
    X(coop_poison, 0, 0, 1, nullptr, false)                                                                           \
    /* strips of a pair a round of sw_align_matrix_long_coop fills at once: 0 = automatic, 1 .. 64 */                 \
    X(long_window, 0, 0, 64, nullptr, false)

#define X(key, def, lo, hi, ok, flag) O_##key,
// OPT_COUNT: the listed keys; the rows of SW_OPTIONS_COOP follow them (OPT_REWIND_ puts the count back by one, so
// that the first of them takes the value OPT_COUNT); OPT_ALL: every row
enum Opt : int { SW_OPTIONS(X) OPT_COUNT, OPT_REWIND_ = OPT_COUNT - 1, SW_OPTIONS_COOP(X) OPT_ALL };
#undef X
struct OptRow {
    const char* key;
    long long def, lo, hi;
    bool (*ok)(long long);
    bool flag;
};
#define X(key, def, lo, hi, ok, flag) {#key, def, lo, hi, ok, flag},
constexpr OptRow OPT_ROWS[OPT_ALL] = {SW_OPTIONS(X) SW_OPTIONS_COOP(X)};
#undef X
#define X(key, def, lo, hi, ok, flag) {def},
std::atomic<long long> g_opt[OPT_ALL] = {SW_OPTIONS(X) SW_OPTIONS_COOP(X)};
#undef X

// The options as one call sees them: every entry point that plans or launches takes one snapshot and
// hands it down, so a sw_set_option from another thread never splits a launch between two values.
struct Opts {
    long long v[OPT_COUNT];
    // environment SWMI_F3WEDGE, read with the snapshot (A/B runs and small-shape tests; not an option):
    // 0 never plans a pair as two wedges (plan_wedge), 1 plans it wherever the geometry admits it, anything
    // else or unset leaves the choice to the measured thresholds
    int f3wedge = -1;
    // environment SWMI_F3WEDGE_DROPS = d0,d1,d2,d3, read with the snapshot (A/B runs and tests; not an option): the
    // wedge plan's drop pattern (plan_wedge; sw_internal.h steep_bounds), 64,64,64,64 being the uniform plan.
    // f3drops_set: 0 unset (the measured default), 1 set, -1 not four multiples of 64 in 64 .. WEDGE_DROP_MAX with
    // d0 == d2 (the launch fails)
    int f3drops_set = 0;
    int f3drops[4] = {64, 64, 64, 64};
    // environment SWMI_F3JOIN, read with the snapshot (A/B runs and tests; not an option): 0 = a wedge launch
    // stages its descriptors with copies, resets the claim counter and the score with memsets and joins its
    // chains in a combine kernel of its own; anything else or unset = the staged kernel does all of it
    // (sw_internal.h KParams::wedge_join)
    int f3join = 1;
    // environment SWMI_F3WEDGE_TRACE, read with the snapshot (tools/trace_wedge.py; not an option): 1 = a traced
    // launch (option trace) may still be planned as two wedges, and then the trace buffer holds 2 S rows of 16
    // words, chain * S + strip (S: the strips a chain of sw_internal.h steep_bounds / wedge_bounds, never more
    // than sw_last_stats' items * 2); anything else or unset = a traced launch stays one chain of 16-word rows
    // per strip
    int f3wtrace = 0;
    long long operator[](Opt o) const { return v[o]; }
};
Opts snapshot_opts() {
    Opts o;
    for (int i = 0; i < OPT_COUNT; ++i) o.v[i] = g_opt[i].load();
    const char* w = std::getenv("SWMI_F3WEDGE");
    o.f3wedge = w && w[0] == '0' && !w[1] ? 0 : w && w[0] == '1' && !w[1] ? 1 : -1;
    const char* j = std::getenv("SWMI_F3JOIN");
    o.f3join = j && j[0] == '0' && !j[1] ? 0 : 1;
    const char* t = std::getenv("SWMI_F3WEDGE_TRACE");
    o.f3wtrace = t && t[0] == '1' && !t[1] ? 1 : 0;
    if (const char* d = std::getenv("SWMI_F3WEDGE_DROPS")) {
        char tail = 0;
        const int got = std::sscanf(d, "%d,%d,%d,%d%c", &o.f3drops[0], &o.f3drops[1], &o.f3drops[2], &o.f3drops[3], &tail);
        o.f3drops_set = got == 4 && wedge_drops_ok(o.f3drops) ? 1 : -1;
    }
    return o;
}
int find_opt(const char* key) {
    for (int i = 0; i < OPT_ALL; ++i)
        if (std::strcmp(key, OPT_ROWS[i].key) == 0) return i;
    return -1;
}

// Longest sequence the engine takes: granule buffers of m rows keep m * 16 in the
// 32-bit record count of a buffer resource (sw_device.h linear_edge).
constexpr long long MAX_SEQ = (1LL << 27) - 1;
// flow2 ring mode (auto): when one-buffer-per-boundary edges would exceed this
constexpr long long RING_AUTO_BYTES = 1LL << 30;

// orientation: 0 = engine policy, 1 = seq1 across lanes (columns), 2 = seq2 across lanes
bool want_swap(const Opts& opt, bool single, long long len1, long long len2) {
    const long long o = opt[O_orient];
    if (o == 1) return false;
    if (o == 2) return true;
    return single ? (len2 > len1) : (len1 > len2);
}

bool params_ok(const Params& p) {
    if (p.gap_init < 0 || p.gap_ext < 0 || p.gap_init > (1 << 20) || p.gap_ext > (1 << 20)) {
        set_err("unsupported gap penalties (%d, %d): need 0 <= G_INIT, G_EXT <= 2^20", p.gap_init, p.gap_ext);
        return false;
    }
    if (p.mismatch > 0 || p.mismatch < -127 || p.match > 127 || p.match < p.mismatch) {
        set_err("unsupported scores (MATCH %d, MISMATCH %d): need -127 <= MISMATCH <= 0, MISMATCH <= MATCH <= 127",
                p.match, p.mismatch);
        return false;
    }
    return true;
}

template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;   // elements
    int ensure(size_t n, hipStream_t sync_first) {
        if (n <= cap && p) return 0;
        if (p) {
            HIPCHK(hipStreamSynchronize(sync_first));
            HIPCHK(hipFree(p));
            p = nullptr;
            cap = 0;
        }
        size_t want = std::max<size_t>(n, 1);
        want = want + want / 4;   // grow with slack
        HIPCHK(hipMalloc((void**)&p, want * sizeof(T)));
        cap = want;
        return 0;
    }
};

template <class T>
struct PinBuf {
    T* p = nullptr;
    size_t cap = 0;
    int ensure(size_t n) {
        if (n <= cap && p) return 0;
        if (p) { HIPCHK(hipHostFree(p)); p = nullptr; cap = 0; }
        size_t want = std::max<size_t>(n, 1);
        want = want + want / 4;
        HIPCHK(hipHostMalloc((void**)&p, want * sizeof(T), hipHostMallocDefault));
        cap = want;
        return 0;
    }
};

struct Ctx {
    int dev = -1;
    int cus = 256;
    hipStream_t own = nullptr;        // engine stream for synchronous calls
    hipStream_t last = nullptr;       // stream of the previous call
    hipEvent_t ev0 = nullptr, ev1 = nullptr, staged = nullptr;
    bool staged_pending = false;
    DevBuf<unsigned char> seq;
    DevBuf<PairDesc> desc;
    DevBuf<int> ibase;
    DevBuf<Granule> bnd;
    DevBuf<Ctrl> ctrl;
    DevBuf<int> scores;
    DevBuf<unsigned> flag;
    DevBuf<unsigned> cons;            // flow2 ring mode: consumer progress words
    DevBuf<unsigned char> hrows;      // a seven-letter ring launch: the pair's rows as perm selectors
    DevBuf<DuoDesc> duo;
    PinBuf<DuoDesc> hduo;
    PinBuf<unsigned char> hseq;
    PinBuf<PairDesc> hdesc;
    PinBuf<int> hibase;
    PinBuf<int> hscores;
    PinBuf<Ctrl> hctrl;
    unsigned epoch = 0;
    // a wedge launch that joins its chains in the staged kernel (KParams::wedge_join): the join words, zero
    // between launches (zeroed when allocated and after an error), and the value the launches so far have left
    // in the claim counter Ctrl::next_item.  Every other kind of launch memsets the counter and leaves its own
    // claims in it (item0_known false): the next joining launch resets it once more and counts from 0
    DevBuf<unsigned> join;
    unsigned item0 = 0;
    bool item0_known = false;
    std::map<int, int> waves_cache;   // variant key -> waves per CU
};

thread_local std::map<int, Ctx*> t_ctx;

Ctx* get_ctx() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) {
        set_err("hipGetDevice failed: no HIP device");
        return nullptr;
    }
    auto it = t_ctx.find(dev);
    if (it != t_ctx.end()) return it->second;
    Ctx* c = new Ctx();
    c->dev = dev;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) {
        set_err("hipGetDeviceProperties failed");
        delete c;
        return nullptr;
    }
    c->cus = prop.multiProcessorCount;
    if (hipStreamCreateWithFlags(&c->own, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess ||
        hipEventCreateWithFlags(&c->staged, hipEventDisableTiming) != hipSuccess) {
        set_err("stream/event creation failed");
        delete c;
        return nullptr;
    }
    t_ctx[dev] = c;
    return c;
}

// ---- problem description -------------------------------------------------

struct Job {
    // per active pair, after orientation
    std::vector<PairDesc> pairs;
    std::vector<int> item_base;
    long long cells = 0;
    uint64_t bnd_granules = 0;
    bool slab = false;           // a column slab (sw_score_slab_device): flow2 streams its rows
    int W = 1, C = 16;
    int mode = MODE_STRIP;
    bool dna = true;
    std::vector<DuoDesc> duos;   // MODE_DUO only
    bool duo_f16 = false;        // MODE_DUO: max3 through v_pk_maximum3_f16 (duo_f16_fits)
    bool f2_stream = false;      // MODE_FLOW2: row codes streamed (rows too long to stage in LDS)
    bool ring = false;           // MODE_FLOW2, one pair: group edges through per-block rings (O(m) state)
    bool f2w2 = false;           // MODE_FLOW2: two columns per lane (strips of 126 new columns, LIN step)
    bool f2w3 = false;           // ... three (strips of 189; with f2w2: flow3 ring mode only, sw_flow3r3_kernel)
    int w45_s4 = -1;             // with f2w3: four / five columns per lane instead (sw_flow3r45_kernel, plan_w45)
    bool f3pwg = false;          // with pwg: flow3's three-column ring step, a pair per workgroup (plan_pwg3)
    bool pwg = false;            // MODE_FLOW2 batch: a pair per workgroup (sw_flow2.hip PWG)
    int hep = 0;                 // one pair over 1..7 byte values not all in {A,C,G,T}: their count (planned as
                                 // DNA, run on flow3's staged kernels, sw_flow3.hip HEP); 0 otherwise
    unsigned char hsym[256] = {};   // with hep: each byte value's symbol 0..6
    bool wedge = false;          // one pair as two wedges (plan_wedge): pairs = {forward, mirrored chain}
    WedgePlan wplan{};           // ... its geometry
    int wedge_rows = 0;          // ... rows of one group edge
    uint64_t wedge_bnd[2] = {0, 0};   // ... granule offsets of the chains' boundary buffers
    int wedge_segr = 0;          // ... a steep plan: 8-B entries per strip of a chain's segment buffer
    uint64_t wedge_seg[2] = {0, 0};   // ... and the granule offsets of those buffers
};

bool is_dna_byte(unsigned char c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }

bool all_dna(const unsigned char* s, int len) {
    for (int i = 0; i < len; ++i)
        if (!is_dna_byte(s[i])) return false;
    return true;
}

int max_rows(const Job& job) {
    int m = 0;
    for (const PairDesc& d : job.pairs) m = std::max(m, d.m);
    return m;
}

// G_INIT == G_EXT: the exact linear-gap step (sw_flow2.hip LIN), unless option linear = 0
bool linear_gap(const Params& p, const Opts& opt) { return p.gap_init == p.gap_ext && opt[O_linear] != 0; }

int pick_W(const Opts& opt, const std::vector<PairDesc>& pairs, bool single) {
    long long forced = opt[O_W];
    if (forced) return (int)forced;
    if (single) {
        // single pair: enough strips to put ~1-2 waves on every SIMD while
        // keeping the per-step instruction stream short (the anti-diagonal
        // critical path is paid per step).  DESIGN.md, "Choosing W".
        const int n = pairs[0].n;
        for (int W : {1, 2, 4, 8})
            if ((n + 64 * W - 1) / (64 * W) <= 2048) return W;
        return 8;
    }
    // batch: inter-pair parallelism fills the GPU; amortise the per-step
    // overhead (W) against the per-strip fill (64W steps per m rows).
    std::vector<int> ns;
    ns.reserve(pairs.size());
    for (auto& p : pairs) ns.push_back(std::min(p.n, p.m));
    std::nth_element(ns.begin(), ns.begin() + ns.size() / 2, ns.end());
    const int med = ns[ns.size() / 2];
    if (med >= 4096) return 8;
    if (med >= 1024) return 4;
    if (med >= 256) return 2;
    return 1;
}

int pick_C(const Opts& opt, int W) {
    long long forced = opt[O_C];
    if (forced) return (int)forced;
    return W <= 2 ? 32 : 64;   // measured: C=32 beats 16 at W=1 (per-chunk overhead vs lag)
}

// Build descriptors for `np` pairs given their (col, row) lengths and arena
// offsets.  `single` selects the single-pair orientation policy.
int pick_mode(const Opts& opt, const std::vector<PairDesc>& pairs, bool single) {
    const long long forced = opt[O_mode];
    if (forced >= 0) return (int)forced;
    if (single) return pairs[0].strips >= 2 ? MODE_CHAIN : MODE_STRIP;
    std::vector<int> st;
    st.reserve(pairs.size());
    for (auto& p : pairs) st.push_back(p.strips);
    std::nth_element(st.begin(), st.begin() + st.size() / 2, st.end());
    return st[st.size() / 2] >= 4 ? MODE_PAIRWG : MODE_STRIP;
}

void plan(const Opts& opt, Job& job, int W, int C, bool single, int mode = -1) {
    job.W = W;
    job.C = C;
    for (auto& d : job.pairs) d.strips = (d.n + 64 * W - 1) / (64 * W);
    job.mode = mode >= 0 ? mode : pick_mode(opt, job.pairs, single);
    job.item_base.assign(job.pairs.size() + 1, 0);
    uint64_t g = 0;
    long long cells = 0;
    for (size_t k = 0; k < job.pairs.size(); ++k) {
        PairDesc& d = job.pairs[k];
        d.bnd_off = g;
        // chain mode hands off through LDS inside a group of 4 strips: granule
        // buffers only between groups; the other modes need one per strip boundary
        const uint64_t nb = grouped_mode(job.mode) ? (uint64_t)((d.strips + 3) / 4 - 1) : (uint64_t)(d.strips - 1);
        g += nb * (uint64_t)d.m;
        const int items = grouped_mode(job.mode) ? (d.strips + 3) / 4 : job.mode == MODE_STRIP ? d.strips : 1;
        job.item_base[k + 1] = job.item_base[k] + items;
        cells += (long long)d.n * (long long)d.m;
    }
    job.bnd_granules = g;
    job.cells = cells;
}

// Byte batches (any byte value) on the duo kernels with the penalty from the bytes (sw_kernels.hip
// SENT_RAW): its sentinel encoding needs MATCH - MISMATCH <= 127 and MISMATCH < 0 (dead and sentinel
// cells then score as mismatches, below the true maximum).  Option duo_raw = 0 keeps such batches on
// the byte-path strip kernels.
bool duo_raw_ok(const Params& p, const Opts& opt) {
    return opt[O_duo_raw] != 0 && p.mismatch < 0 && p.match - p.mismatch <= 127;
}

// Packed-u16 duo mode: exact when every H + MATCH fits 16 bits (H <= MATCH*min(n,m)).  MATCH < 0 is
// out: A = H + MATCH lives in an unsigned half, and the border's 0 + MATCH would read as 65535 (a NaN
// on the f16 max3 variant); such constants (every score 0) run the int32 kernels.
bool duo_fits(const Job& job, const Params& p, const Opts& opt) {
    if (p.match < 0) return false;
    if ((!job.dna && !duo_raw_ok(p, opt)) || p.gap_init + p.match > 65535 || p.gap_ext > 65535 || p.match - p.mismatch > 254)
        return false;
    for (auto& d : job.pairs)
        if ((long long)std::max(p.match, 1) * std::min(d.n, d.m) + p.match > 65535) return false;
    return true;
}

// The duo kernel's f16-max3 variant reads u16 values as f16 bit patterns, exact
// below 0x7C00 (no Inf/NaN encodings): every t, E, F, H and running max is at
// most max H + MATCH <= MATCH*(min(n,m)+1).
bool duo_f16_fits(const Job& job, const Params& p, const Opts& opt) {
    if (!opt[O_duo16]) return false;
    for (auto& d : job.pairs)
        if ((long long)std::max(p.match, 1) * (std::min(d.n, d.m) + 1) > 0x7BFF) return false;
    return true;
}

// Turn a planned pair list into duos: pairs sorted by shape, neighbours share a
// duo (padding to the larger shape), boundaries sized by the padded rows.
void plan_duos(Job& job) {
    std::vector<int> ord(job.pairs.size());
    for (size_t i = 0; i < ord.size(); ++i) ord[i] = (int)i;
    const auto by_shape = [&](int x, int y) {
        const PairDesc &a = job.pairs[x], &b = job.pairs[y];
        return a.n != b.n ? a.n > b.n : a.m > b.m;
    };
    // callers that pass pairs in shape order already (sw_db: records longest first) skip the sort
    if (!std::is_sorted(ord.begin(), ord.end(), by_shape)) std::sort(ord.begin(), ord.end(), by_shape);
    job.duos.clear();
    uint64_t g = 0;
    for (size_t i = 0; i < ord.size(); i += 2) {
        const PairDesc& a = job.pairs[ord[i]];
        const bool two = i + 1 < ord.size();
        const PairDesc& b = job.pairs[two ? ord[i + 1] : ord[i]];
        DuoDesc d{};
        d.col_off[0] = a.col_off; d.row_off[0] = a.row_off; d.n[0] = a.n; d.m[0] = a.m; d.out_idx[0] = a.out_idx;
        if (two) {
            d.col_off[1] = b.col_off; d.row_off[1] = b.row_off; d.n[1] = b.n; d.m[1] = b.m; d.out_idx[1] = b.out_idx;
        } else {
            d.col_off[1] = a.col_off; d.row_off[1] = a.row_off; d.n[1] = 0; d.m[1] = 0; d.out_idx[1] = -1;
        }
        d.n_pad = std::max(d.n[0], d.n[1]);
        d.m_pad = std::max(d.m[0], d.m[1]);
        d.strips = (d.n_pad + 64 * job.W - 1) / (64 * job.W);
        d.bnd_off = g;
        g += (uint64_t)(d.strips - 1) * (uint64_t)d.m_pad;
        job.duos.push_back(d);
    }
    job.bnd_granules = g;
    job.item_base.assign(job.duos.size() + 1, 0);
    for (size_t k = 0; k < job.duos.size(); ++k) job.item_base[k + 1] = (int)(k + 1);
}

// After the alphabet is known: promote an automatic pair-per-workgroup plan to
// the packed duo kernel when it is exact, or honour a forced duo request.
// MODE_FLOW2 (sw_flow2.hip): W = 1, DNA, every score byte s + G_INIT a signed
// byte above the -128 sentinel, and the row codes fit in LDS.
// Rows that fit in LDS are staged once per workgroup; longer ones (C5) stream
// through per-wave code rings (sw_flow2.hip, STREAM), as do all with "f2stream" = 1.
bool flow2_fits(const Job& job, const Params& p) {
    return job.dna && job.W == 1 && flow2_variant_exists(job.C) && p.match + p.gap_init <= 127 &&
           p.mismatch + p.gap_init >= -127;
}
bool flow2_staged(const Job& job, const Opts& opt, int max_m) {
    return opt[O_f2stream] == 0 && flow2_stage_bytes(max_m, job.C) <= flow2_stage_max(job.C);
}

// Two columns per lane (sw_flow2.hip W2) whenever the linear-gap step runs (G_INIT ==
// G_EXT, option linear not 0, C = 32 / 64); option f2w: 0 auto, 1 or 2 forced.
// Measured (kernel ms, W = 1 -> 2): C2 3.46 -> 3.17 (half the strip hops and half the
// wavefront's column term at a 25 instead of 17 ns step), C5 222 -> 181 (4.5 instead
// of 5.5 VALU per 64 cells, throughput-bound).
bool flow2_w2_wanted(const Job& job, const Params& p, const Opts& opt) {
    // (C = 16: flow3's staged kernel only, sw_flow3.hip; flow2 has no such two-column variant,
    // so streamed rows at C = 16 keep one column per lane)
    const int max_m = max_rows(job);
    const bool c16 = opt[O_f3] != 0 && !job.slab && flow2_staged(job, opt, max_m) && flow3_fits(max_m, 16);
    return linear_gap(p, opt) && (job.C != 16 || c16) && (opt[O_C] != 16 || c16) && opt[O_f2w] != 1;
}

// Four and five columns per lane (flow3 ring mode, linear-gap step, one pair): when the three-column
// strips need more groups than `slots` resident blocks (C5: 5549 strips in 1388 groups for 1024), the
// later groups run in a second round after the first ones end, at a fraction of the chip (C5 154 ms
// against a 115 ms issue bound; tools/sim_ring.py models it at 151).  Strips of 252 new columns, then
// g5 groups of 315, fit `slots` groups: 1008 (slots - g5) + 1260 g5 >= n.  A group's four strips share a
// width, so the split index s4 is a multiple of 4.  Modelled 142 ms for C5 (every strip resident), but
// measured 167 ms against W3's 154 (r06, profiles/r06_c5_w45.md): strip 0, which runs at the lone-wave
// pace, takes 42.5 ms at four columns against 29.7 at three, and the later strips end at the same
// 0.119 us per column in both.  So it is an option (f2w = 4), not the automatic plan.
// Returns false (plan unchanged) when n needs more than five columns per lane.
bool plan_w45(Job& job, int slots) {
    PairDesc& d = job.pairs[0];
    const long long n = d.n;
    const long long g5 = std::max(0LL, (n - 1008LL * slots + 251) / 252);
    if (g5 > slots || n < 4 * 256) return false;
    int s4 = 4 * (int)(slots - g5), s5 = 0;
    if (252LL * (s4 - 1) + 256 < n) {
        // W5 strips after s4 W4 strips: the last one's columns reach n - 1
        s5 = (int)std::max(1LL, (n - 320 - 252LL * s4 + 314) / 315 + 1);
    } else {
        // four columns cover it: the fewest W4 strips (no W5 strip, so the count may be anything)
        s4 = (int)std::max(1LL, (n - 256 + 251) / 252 + 1);
    }
    d.strips = s4 + s5;
    // the kernel takes a split index that is a multiple of 4 (a group's strips share a width): with W4
    // strips only, the next multiple of 4 at or above their count, so every strip stays below it
    job.w45_s4 = s5 > 0 ? s4 : (d.strips + 3) / 4 * 4;
    job.item_base[1] = job.item_base[0] + (d.strips + 3) / 4;
    return true;
}

// Re-plan a grouped job for MODE_FLOW2: strips of 64 columns overlapping by one
// (w2: 128 columns overlapping by two).  pwg: one item per pair, whose workgroup runs all
// of its strips with LDS hand-offs only (no granule edges).
void plan_flow2(const Opts& opt, Job& job, bool w2, bool pwg = false, bool w3 = false) {
    job.mode = MODE_FLOW2;
    job.f2w2 = w2 || w3;
    job.f2w3 = w3;
    job.pwg = pwg;
    uint64_t g = 0;
    for (size_t k = 0; k < job.pairs.size(); ++k) {
        PairDesc& d = job.pairs[k];
        d.strips = w3 ? flow2_strips_w3(d.n) : w2 ? flow2_strips_w2(d.n) : flow2_strips(d.n);
        d.bnd_off = g;
        if (!pwg) g += (uint64_t)((d.strips + 3) / 4 - 1) * (uint64_t)d.m;
        job.item_base[k + 1] = job.item_base[k] + (pwg ? 1 : (d.strips + 3) / 4);
    }
    job.bnd_granules = g;
    if (pwg) return;
    // Ring mode (sw_flow2.hip, KParams::ring_rows): one pair whose write-once group
    // edges would take more than RING_AUTO_BYTES (C5: 69.8 GB), or when forced.  Stream
    // positions are 32-bit and may wrap: slots are taken mod a power of two <= 2^24,
    // progress words are compared as serial numbers, and a slot's previous position
    // differs from the current one by the ring size (< 2^25), which the checksum's
    // 25 position bits always see.  Hence rows <= 2^24.
    if (job.pairs.size() == 1 && opt[O_ring] != 0 && job.item_base[1] > 1) {
        const PairDesc& d = job.pairs[0];
        const bool ok = d.m <= (1 << 24);
        job.ring = ok && (opt[O_ring] == 1 || (long long)(g * sizeof(Granule)) > RING_AUTO_BYTES);
    }
}

// The pair-per-workgroup kernel keeps a round's rows of its longest pair in LDS: at least
// `wgs` such workgroups must fit a CU (automatic choice: 2, m up to ~8.5k rows).
bool pwg_fits(const Job& job, const Params& prm, const Opts& opt, int wgs) {
    const int max_m = max_rows(job);
    const bool lin = flow2_w2_wanted(job, prm, opt);
    // the round buffer must also pass the launch's dynamic-LDS limit (sw_flow2.hip flow2_dyn_lds)
    return flow2_pwg_wgs(max_m, 64, lin) >= wgs &&
           flow2_pwg_row_bytes(lin) * flow2_pwg_rows(max_m, 64) <= flow2_stream_dyn_max(64);
}

// A batch on the pair-per-workgroup flow2 kernel: W = 1 strips, 64-row chunks, streamed
// codes; two columns per lane with the linear-gap step (G_INIT == G_EXT), else the affine
// step at one column per lane.
void plan_pwg(Job& job, const Params& prm, const Opts& opt) {
    job.W = 1;
    job.C = 64;
    plan_flow2(opt, job, flow2_w2_wanted(job, prm, opt), true);
    job.f2_stream = true;
}

// A batch whose scores need int32 on flow3's three-column ring step with a pair per workgroup
// (sw_flow3r3p_kernel): the linear-gap step only (G_INIT == G_EXT, option linear not 0), rows up to
// 2^16 (the block's edge ring holds a whole strip edge), option f3pwg not 0.  Against flow2's PWG
// kernel (two columns, compiled loop, 3 per CU by its round buffer): 12.5 + 1.6 instead of ~10.7
// VALU per step for 1.5x the columns, 4 workgroups per CU (a C3-sized batch in one pass).
// The general affine step takes the same organisation on the three-column affine ring step
// (sw_flow3ra3p_kernel, option f3a not 0) where `affine` allows it: C3-shaped at (2, -3, 5, 2) on int32
// flow2's PWG (one column per lane) runs 21.1 ms.
bool pwg3_fits(const Job& job, const Params& prm, const Opts& opt, bool affine = false) {
    return opt[O_f3pwg] != 0 && job.dna && (linear_gap(prm, opt) ? opt[O_f3] != 0 : affine && opt[O_f3a] != 0) &&
           prm.match + prm.gap_init <= 127 && prm.mismatch + prm.gap_init >= -127 && max_rows(job) <= (1 << 16) &&
           (opt[O_C] == 0 || opt[O_C] == 64) && opt[O_f2w] != 1 && opt[O_f2w] != 2;
}
void plan_pwg3(Job& job, const Opts& opt) {
    job.W = 1;
    job.C = 64;
    plan_flow2(opt, job, true, true, true);
    job.f3pwg = true;
    job.f2_stream = true;
}

// A DNA batch on the flow2 item claim: a pair's strip groups spread over many CUs (W = 1
// strips, 64-row chunks, streamed codes, 2 workgroups per CU from 4 groups per CU).
void plan_claim(Job& job, const Params& prm, const Opts& opt) {
    job.W = 1;
    job.C = 64;
    plan_flow2(opt, job, flow2_w2_wanted(job, prm, opt));
    job.f2_stream = true;
}

// A pair's byte set (256 bits) -> job.hep / job.hsym: at most seven values, not all within {A,C,G,T}
// (those take the DNA path), symbols in byte order.  Option hep = 0: never.
bool set_hep(Job& job, const Opts& opt, const uint32_t set[8]) {
    job.hep = 0;
    if (opt[O_hep] == 0) return false;
    int k = 0;
    unsigned char sym[256] = {};
    for (int b = 0; b < 256; ++b)
        if (set[b >> 5] >> (b & 31) & 1u) {
            if (k == 7) return false;
            sym[b] = (unsigned char)k++;
        }
    if (k == 0) return false;
    std::memcpy(job.hsym, sym, sizeof sym);
    job.hep = k;
    return true;
}

void byte_set(const unsigned char* p, int len, uint32_t set[8]) {
    for (int i = 0; i < len; ++i) set[p[i] >> 5] |= 1u << (p[i] & 31);
}

// ---- the launch a planned job makes -----------------------------------------
// Decided here and nowhere else: every field of LaunchCfg but the two that wait for the residency query
// (f2_wgs and blocks: size_grid), whether it is a ring launch, whether the pair was cut (plan_split), and
// the reason when the plan asks for a kernel that does not exist.
struct Variant {
    LaunchCfg cfg;
    bool ring = false;
    bool cut = false;
    bool wedge = false;
    bool steep = false;
    const char* err = nullptr;
};

// Duo batches at C = 64: strip hand-offs in LDS when the wrap buffer (a round's rows of both pairs) fits
// the default dynamic-LDS limit; no boundary buffers in HBM then.  And, at 4 or 8 columns per lane, the
// row codes from an LDS table when both fit two workgroups per CU and the duos run in one pass at that
// (C3, 512 duos: 6.80 -> 6.54 ms), or rows are 8192 or more; more duos of shorter rows keep the
// table-less kernel, whose smaller LDS admits 4 per CU.  With the CU's two workgroups taking turns at
// priority (duo_prio) the table wins at 8192 rows: 8192 pairs of 8192 51.8 -> 50.5 ms, 2048 pairs 13.2 ->
// 12.6, 4096 pairs of 1024 x 8192 4.59 -> 4.46; it loses at 4096 rows (4096 pairs of 4096: 7.88 -> 8.03)
// and on the ragged DB search (17.9 -> 19.7), r05_duo_prio.md
void select_duo_lds(const Job& job, const Opts& opt, int cus, LaunchCfg& cfg) {
    if (job.mode != MODE_DUO || job.C != 64 || opt[O_duo_lds] == 0) return;
    int max_mp = 0;
    for (const DuoDesc& d : job.duos) max_mp = std::max(max_mp, d.m_pad);
    const int slots = duo_wrap_slots(max_mp);
    const long long wrap_b = (long long)slots * (cfg.f2_lin ? 4 : 8);
    const int tab_w = DUO_TAB_OFF + max_mp + DUO_TAB_TAIL;
    const bool one_pass = (long long)job.duos.size() <= 2LL * cus || opt[O_duo_tab] == 2 || max_mp >= 8192;
    if (opt[O_duo_tab] != 0 && one_pass && job.W % 4 == 0 && wrap_b + 4LL * tab_w + 16 <= duo_lds_fit(cfg.f2_lin)) {
        cfg.duo_wrap = slots;
        cfg.duo_tab = tab_w;
    } else if (wrap_b <= 64 * 1024) {
        cfg.duo_wrap = slots;
    }
}

Variant select_variant(const Job& job, const Params& prm, const Opts& opt, int cus) {
    const bool flow2 = job.mode == MODE_FLOW2, slab = job.slab, ring = job.ring;
    Variant v;
    v.ring = ring;
    v.cut = !job.pairs.empty() && (job.pairs[0].flags & PAIR_HALF) != 0;
    v.wedge = job.wedge;
    v.steep = job.wedge && job.wplan.steep;
    LaunchCfg& cfg = v.cfg = LaunchCfg{job.W, job.C, job.dna, 0, job.mode, max_rows(job)};
    // flow2's ring and slab kernels always stream the row codes (sw_flow2.hip launch_v)
    const bool f2s = flow2 && (job.f2_stream || ring || slab);
    // the linear-gap step; the pair-per-workgroup kernel is built with it exactly at two columns per lane
    const bool lin = linear_gap(prm, opt);
    const bool f2_lin = job.f3pwg ? lin
                      : job.pwg   ? job.f2w2
                                  : lin && ((flow2 && (job.C == 32 || job.C == 64 || (job.C == 16 && job.f2w2))) ||
                                            (job.mode == MODE_DUO && job.duo_f16));
    // flow3 (sw_flow3.hip, hand-scheduled chunk loops) for the two-column linear-gap launches it
    // implements: the staged single-pair kernel (C = 16 / 32, rows in LDS: C2) and ring mode (C = 64
    // / 32, streamed rows, one pair: C5); option f3 = 0 keeps flow2
    const bool f3_base = opt[O_f3] != 0 && flow2 && job.f2w2 && f2_lin && !job.pwg;
    const bool f3_slab_ok = !slab || (opt[O_f3slab] != 0 && job.C == 64);
    const bool use_f3 = f3_base && ((!f2s && !ring && flow3_fits(cfg.max_m, job.C)) ||
                                    (ring && f3_slab_ok && (job.C == 64 || job.C == 32)));
    // the general affine step (G_INIT != G_EXT, or option linear = 0) on flow3's staged kernel: one
    // column per lane, rows in LDS, linear edges (C2 with affine constants); option f3a = 0 keeps flow2
    const bool use_f3a = opt[O_f3a] != 0 && flow2 && !job.f2w2 && !f2_lin && !job.pwg && !f2s && !ring && !slab &&
                         (job.C == 32 || job.C == 16) && flow3_fits(cfg.max_m, job.C, true);
    // ... and in ring mode at two columns per lane (finalize_mode planned the strips for it)
    const bool use_f3ra = opt[O_f3a] != 0 && flow2 && job.f2w2 && !f2_lin && !job.pwg && ring && f3_slab_ok && job.C == 64;
    cfg.duo_f16 = job.mode == MODE_DUO && job.duo_f16;
    cfg.f2_stream = f2s;
    cfg.f2_lin = f2_lin;
    cfg.f2_w2 = flow2 && job.f2w2;
    cfg.f2_pwg = flow2 && job.pwg;
    cfg.f3 = use_f3;
    // half-chunk links: staged at C = 32 (option f3hl), ring at C = 64 (f3rhl; the slab roles and the affine
    // ring step exist with whole-chunk links only)
    cfg.f3_hl = (use_f3 && !slab && ((!ring && job.C == 32 && opt[O_f3hl] != 0) || (ring && job.C == 64 && opt[O_f3rhl] != 0))) ||
                (use_f3a && job.C == 32 && opt[O_f3hl] != 0);
    cfg.f3a = use_f3a;
    cfg.f3ra = use_f3ra;
    cfg.f3_slab = (use_f3 || use_f3ra) && slab;
    // the pool loops (no I/O rotation, tools/gen_flow3.py gen_pool) for staged launches with half-chunk
    // links at C = 32, both steps, when option f3pool = 1 (default 0: measured slower)
    cfg.f3p = opt[O_f3pool] != 0 && cfg.f3_hl && job.C == 32 && !ring && (use_f3 || use_f3a);
    cfg.f3_w3 = job.f2w3 && job.w45_s4 < 0;
    cfg.f3_w45 = job.w45_s4 >= 0;
    cfg.hep = job.hep > 0;
    cfg.f3_pwg = job.f3pwg;
    select_duo_lds(job, opt, cus, cfg);
    const bool f3_ring = (use_f3 || use_f3ra) && ring;
    if (job.f3pwg && (slab || ring || !job.f2w3))
        v.err = "the pair-per-workgroup three-column kernel takes batches only";
    else if (cfg.hep && !((use_f3 && !f2s && !ring) || use_f3a || (f3_ring && cfg.f3_w3 && !slab && !job.f3pwg)))
        v.err = "a seven-letter alphabet runs flow3's staged kernels or its three-column ring kernels only (one pair)";
    else if (cfg.f3_w45 && !(use_f3 && ring && !slab))
        v.err = "four / five columns per lane run on flow3's linear-gap ring kernel only (one pair, not a slab)";
    else if (job.f2w3 && !job.f3pwg && !(f3_ring && job.C == 64 && !cfg.f3_hl))
        v.err = "three columns per lane run on flow3's ring kernel only (linear-gap step, C = 64, whole-chunk links)";
    else if (cfg.f2_w2 && job.C == 16 && !use_f3)
        v.err = "flow2: two columns per lane at C = 16 runs on flow3 only (rows staged in LDS, one GPU)";
    else if (cfg.f2_w2 && !f2_lin && !use_f3ra && !job.f3pwg)   // the strips were cut for two columns per lane
        v.err = "flow2: two columns per lane needs the linear-gap step (or flow3's affine ring kernel)";
    if (job.f3pwg) {   // the linear-gap ring step, or the affine one (sw_flow3ra3p_kernel)
        cfg.f3 = f2_lin;
        cfg.f3ra = !f2_lin;
    }
    return v;
}

// The variant word of sw_last_stats (include/algoGPU.h documents the bits)
int variant_word(const Variant& v) {
    const LaunchCfg& c = v.cfg;
    const bool bits[20] = {c.duo_f16, c.f2_stream, v.ring,     c.f2_lin, c.f2_w2, c.f2_pwg, c.f3,    c.duo_wrap > 0, c.duo_tab > 0,
                           c.f3_hl,   c.f3a || c.f3ra, c.f3_slab, c.f3p,  c.f3_w3, c.f3_w45, c.f3_pwg, c.hep,       v.cut,
                           v.wedge,   v.steep};
    int w = 0;
    for (int b = 0; b < 20; ++b) w |= (bits[b] ? 1 : 0) << b;
    return w;
}

// A seven-letter job (planned as DNA) launches one of the kernels with seven-letter forms: flow3's
// staged kernels (not the pool loops), or ring mode at three columns per lane (sw_flow3r3h / ra3h_kernel)
bool hep_launchable(const Job& job, const Params& prm, const Opts& opt, int cus) {
    if (job.pairs.size() != 1) return false;
    const Variant v = select_variant(job, prm, opt, cus);
    return !v.err && !v.cfg.f3p;
}

// One pair on flow3's staged two-column linear-gap kernel, cut at a column and scored from both ends at
// once: the left half, columns [0, c), runs forward; the right half, columns
// [c, n), runs on both sequences mirrored, with `lead` dead columns in front so that its last strip's
// last new column is the cut column too.  With one value per grid node the pair's score is the larger of
// the halves' maxima and of max over i of H_L[i][c] + H_R[m - i][n - c] (sw_flow3.hip
// sw_flow3_combine_kernel), so the two chains of half the strips run side by side.  c and
// n - c + lead are multiples of 126; each half gets at least two strips, hence n >= 379.
bool split_cols(int n, int* c, int* lead) {
    const int kl = std::max(2, (n + 125) / 126 / 2);   // half the strips, the odd one to the right
    if ((long long)n - 126LL * kl < 127) return false;
    *c = 126 * kl;
    *lead = (126 - (n - *c) % 126) % 126;
    return true;
}
// Narrowest pair the automatic plan cuts (option f3split = -1)
constexpr int F3_SPLIT_AUTO_N = 4096;

// Cuts a planned single-pair job in two PairDesc entries sharing one score slot when its launch is the
// staged flow3 linear-gap kernel with rotating loops (not ring mode, streamed rows, a slab, a batch or the
// pool loops) and is not traced.  Items stay in claim order, the left half's groups first: every group
// waits on a lower item only, whatever the grid.
bool plan_split(Job& job, const Params& prm, const Opts& opt, int cus) {
    const long long o = opt[O_f3split];
    if (o == 0 || job.pairs.size() != 1 || opt[O_trace] != 0) return false;
    const Variant v = select_variant(job, prm, opt, cus);
    if (v.err || !v.cfg.f3 || v.ring || v.cfg.f2_stream || v.cfg.f3p) return false;
    const PairDesc whole = job.pairs[0];
    int c = 0, lead = 0;
    if (!split_cols(whole.n, &c, &lead)) return false;
    if (o < 0 && whole.n < F3_SPLIT_AUTO_N) return false;
    PairDesc left = whole, right = whole;
    left.n = c;
    left.strips = c / 126;
    left.flags = PAIR_HALF;
    right.col_off = whole.col_off + (uint64_t)c;
    right.n = whole.n - c;
    right.strips = (right.n + lead) / 126;
    right.flags = PAIR_HALF | PAIR_REV;
    right.lead = lead;
    // a granule edge behind every group, the last one's for the combine kernel
    left.bnd_off = 0;
    right.bnd_off = (uint64_t)((left.strips + 3) / 4) * (uint64_t)whole.m;
    job.bnd_granules = right.bnd_off + (uint64_t)((right.strips + 3) / 4) * (uint64_t)whole.m;
    job.pairs = {left, right};
    job.item_base = {0, (left.strips + 3) / 4, (left.strips + 3) / 4 + (right.strips + 3) / 4};
    return true;
}

// One pair on flow3's staged two-column linear-gap kernel as two wedges cut along an anti-diagonal staircase
// (the identity and its geometry: tests/test_wedge_identity.py, sw_internal.h
// wedge_bounds).  The forward chain runs over all columns, strip s for e0 - 64 s rows; the mirrored chain
// the same from the far corner; every strip leaves the last two rows of H of its lanes, and the wedge combine
// kernel joins the two staircases.  No strip runs all m rows, so a chain ends about (m + 64 S) / 2 + S (lag - 1)
// steps in instead of the column cut's m + S / 2 (63 + lag).  Same admission as plan_split, and every strip
// must keep one 64-row body: m >= 64 S + 64.  The chains' groups alternate in the item order (F0, B0, F1, ...):
// a group waits on a lower item only, whatever the grid.
// Automatic (option f3split = -1, SWMI_F3WEDGE unset) from F3_WEDGE_AUTO_N columns, the narrowest width of the
// measured sweep (profiles/f3wedge_ab.jsonl: the wedge beats the cut at every admissible shape measured, rows
// from the admission edge up); below it the column cut's own rule stays.  f3split = 0 switches it off with the
// cut, f3split = 1 keeps forcing the column cut.
constexpr int F3_WEDGE_AUTO_N = 4096;
// The steep plan (sw_internal.h steep_bounds): a staircase that drops more than 64 rows behind some strips, so
// that the strips of a chain end closer together than the hand-off lag lets the uniform plan's (DESIGN.md
// section 4).  Taken with the pattern of SWMI_F3WEDGE_DROPS wherever it is admissible.  Without that variable,
// from F3_STEEP_AUTO_N columns (profiles/f3steep_ab.jsonl: 7 to 12 % under the uniform wedge at every admissible
// shape from 4096 columns): F3_STEEP_AUTO_DROPS, 384 rows a group, about the lag of a group's four hand-offs, so
// the strips of a chain end together; and where the launch has more groups than the GPU has CUs (a workgroup a
// CU: C2's 262 on 256), F3_STEEP_QUEUED_DROPS first, 448 rows a group: the queued groups wait for a resident one
// to end, and with the drops above the lag the late groups end first (C2: 1.41 ms uniform, 1.37 at 384 rows a
// group, 1.28 at 448, whichever links carry them).  Elsewhere the uniform plan.
constexpr int F3_STEEP_AUTO_N = 4096;
constexpr int F3_STEEP_AUTO_DROPS[4] = {64, 128, 64, 128};
constexpr int F3_STEEP_QUEUED_DROPS[4] = {128, 64, 128, 128};
bool plan_wedge(Job& job, const Params& prm, const Opts& opt, int cus) {
    if (opt[O_f3split] != -1 || opt.f3wedge == 0 || job.pairs.size() != 1 || (opt[O_trace] != 0 && !opt.f3wtrace))
        return false;
    const Variant v = select_variant(job, prm, opt, cus);
    if (v.err || !v.cfg.f3 || v.ring || v.cfg.f2_stream || v.cfg.f3p || job.slab) return false;
    const PairDesc whole = job.pairs[0];
    if (opt.f3wedge != 1 && whole.n < F3_WEDGE_AUTO_N) return false;
    WedgePlan w;
    const auto steep = [&](const int* d) {
        return std::max(std::max(d[0], d[1]), std::max(d[2], d[3])) > 64 && steep_bounds(whole.n, whole.m, d, &w);
    };
    const bool queued = 2 * ((((long long)whole.n - 2 + 125) / 126 + 3) / 4) > cus;
    const bool st = opt.f3drops_set ? steep(opt.f3drops)
                                    : whole.n >= F3_STEEP_AUTO_N &&
                                          ((queued && steep(F3_STEEP_QUEUED_DROPS)) || steep(F3_STEEP_AUTO_DROPS));
    if (!st && !wedge_bounds(whole.n, whole.m, &w)) return false;
    const int groups = (w.strips + 3) / 4;
    PairDesc f = whole, b = whole;
    f.strips = b.strips = w.strips;
    f.flags = PAIR_WEDGE;
    b.flags = PAIR_WEDGE | PAIR_REV;
    b.lead = w.lead;
    // a chain's group edges hold the rows its strips reach; behind both chains' edges the two boundary
    // buffers of two 16-B entries per strip and lane
    job.wedge_rows = std::max(w.e0[0], w.e0[1]) + 64;
    f.bnd_off = 0;
    b.bnd_off = (uint64_t)groups * (uint64_t)job.wedge_rows;
    job.wedge_bnd[0] = 2 * b.bnd_off;
    job.wedge_bnd[1] = job.wedge_bnd[0] + 128ull * (uint64_t)w.strips;
    job.bnd_granules = job.wedge_bnd[1] + 128ull * (uint64_t)w.strips;
    if (w.steep) {   // per chain and strip the longest hand-off column's 8-B entries (even: whole granules)
        job.wedge_segr = std::max(std::max(w.drop[0], w.drop[1]), std::max(w.drop[2], w.drop[3])) - 62;
        const uint64_t seg = (uint64_t)w.strips * (uint64_t)job.wedge_segr / 2;
        job.wedge_seg[0] = job.bnd_granules;
        job.wedge_seg[1] = job.wedge_seg[0] + seg;
        job.bnd_granules = job.wedge_seg[1] + seg;
    }
    job.pairs = {f, b};
    job.item_base = {0, groups, 2 * groups};
    job.wedge = true;
    job.wplan = w;
    return true;
}

int finalize_mode(Job& job, const Params& prm, const Opts& opt, int cus);

// finalize_mode, and for a seven-letter job (planned as DNA) the check that it lands on the staged flow3
// kernels; otherwise the job is re-planned on the byte path
int finalize_alphabet(Job& job, const Params& prm, const Opts& opt, int cus, bool single) {
    if (job.hep) job.dna = true;
    if (finalize_mode(job, prm, opt, cus)) return -1;
    if (!job.hep || hep_launchable(job, prm, opt, cus)) return 0;
    // a fresh job (the DNA attempt left its ring / column / stream flags behind) on the byte path
    Job bytes;
    bytes.pairs = job.pairs;
    bytes.slab = job.slab;
    bytes.dna = false;
    job = std::move(bytes);
    const int W = pick_W(opt, job.pairs, single);
    plan(opt, job, W, pick_C(opt, W), single);
    return finalize_mode(job, prm, opt, cus);
}

int finalize_mode(Job& job, const Params& prm, const Opts& opt, int cus) {
    const int max_m = max_rows(job);
    // a single pair too wide for W = 1 under the 2048-strip rule: flow2 still runs it
    // fastest at W = 1 (its 10.7-VALU step, rows streamed when they exceed the LDS;
    // C5: 545 ms vs 894 ms for the W = 8 chain)
    if (opt[O_mode] < 0 && opt[O_W] == 0 && job.mode == MODE_CHAIN && job.W > 1 &&
        job.pairs.size() == 1) {
        Job w1 = job;
        plan(opt, w1, 1, pick_C(opt, 1), true, MODE_CHAIN);
        if (flow2_fits(w1, prm)) job = w1;
    }
    if (job.mode == MODE_FLOW2 && job.pairs.size() > 1 && opt[O_f2pwg] == 1) {
        Job w1 = job;   // a forced flow2 batch, a pair per workgroup (W = 1 strips, C = 64)
        plan(opt, w1, 1, 64, false, MODE_FLOW2);
        if (flow2_fits(w1, prm) && pwg3_fits(w1, prm, opt, true)) {
            job = w1;
            plan_pwg3(job, opt);
            return 0;
        }
        if (flow2_fits(w1, prm) && pwg_fits(w1, prm, opt, 1)) {
            job = w1;
            plan_pwg(job, prm, opt);
            return 0;
        }
    }
    if (job.mode == MODE_FLOW2 || (opt[O_mode] < 0 && job.mode == MODE_CHAIN)) {
        if (flow2_fits(job, prm)) {
            plan_flow2(opt, job, flow2_w2_wanted(job, prm, opt));
            // the affine step in ring mode runs flow3's two-column affine kernel (sw_flow3ra_kernel:
            // ring mode is throughput-bound, and two columns per lane issue 9 VALU per 64 cells
            // against 10.5 at one): re-plan with two-column strips when they still take ring mode
            if (job.ring && !job.f2w2 && !job.slab && opt[O_f3a] != 0 && opt[O_f2w] != 1 &&
                (opt[O_C] == 0 || opt[O_C] == 64)) {
                Job w2 = job;
                plan_flow2(opt, w2, true);
                if (w2.ring) job = w2;
            }
            // a column slab (f-1) runs flow3's ring kernel with its slab roles (sw_flow3rs_kernel /
            // sw_flow3ras_kernel): two columns per lane, ring edges between its own groups (forced
            // for any size; with one group there are none), option f3slab = 0 keeps flow2's slab kernel
            const bool lin = linear_gap(prm, opt);
            if (job.slab && opt[O_f3slab] != 0 && (lin ? opt[O_f3] != 0 : opt[O_f3a] != 0) &&
                opt[O_f2w] != 1 && opt[O_ring] != 0 && (opt[O_C] == 0 || opt[O_C] == 64)) {
                if (!job.f2w2) plan_flow2(opt, job, true);
                job.ring = true;
            }
            // three columns per lane (flow3 ring mode, linear-gap step, C = 64; option f2w = 0 or 3): a
            // third fewer strips at 12.5 VALU per 192 cells instead of 9 per 128. C5 165.0 -> 159.5 ms;
            // slab 0 of 8 38.6 -> 33.1 ms (its 1041 two-column strips need 261 groups for 256 CUs, and
            // the 5 CUs running two pace the chain; 694 three-column strips fit 174 groups).  A slab
            // with f3slab = 0 stays on flow2's slab kernel, which has no three-column form.
            if (job.ring && job.f2w2 && (!job.slab || opt[O_f3slab] != 0) && (lin ? opt[O_f3] != 0 && opt[O_f3rhl] == 0 : opt[O_f3a] != 0) &&
                (opt[O_f2w] == 3 || opt[O_f2w] == 0 || opt[O_f2w] == 4) &&
                (opt[O_C] == 0 || opt[O_C] == 64)) {
                plan_flow2(opt, job, true, false, true);
                job.ring = true;
                // ... or four and five with option f2w = 4 (every group resident in one round; measured
                // slower on C5, 167 against 154 ms: plan_w45).  Its grid is F2_WGS_MAX blocks per CU, or
                // option blocks (tests cut small pairs into both widths with it)
                const int slots = opt[O_blocks] > 0 ? (int)opt[O_blocks] : cus * F2_WGS_MAX;
                if (lin && !job.slab && job.pairs.size() == 1 && opt[O_f2w] == 4) plan_w45(job, slots);
            }
            job.f2_stream = job.ring || !flow2_staged(job, opt, max_m);   // ring mode runs with streamed codes
            // ring mode (one pair of many groups per CU, C5): throughput-bound, so 64-row chunks
            // (half the per-chunk work per step) beat the shorter hand-off lag of 32 (C5 249 -> 220 ms)
            if (job.ring && opt[O_C] == 0) job.C = 64;
            // the staged two-column kernel on flow3 (C2): 32-row chunks whose in-workgroup links hand
            // off every half chunk (option f3hl, default 1: C = 32's per-chunk work at a 63 + 16-step
            // lag, 2.645 -> 2.600 ms); with f3hl = 0, 16-row chunks (2.70 -> 2.65 ms against plain 32)
            if (!job.ring && !job.f2_stream && !job.slab && job.f2w2 && opt[O_C] == 0 && opt[O_f3] != 0 &&
                opt[O_f3hl] == 0 && flow3_fits(max_m, 16))
                job.C = 16;
            return 0;
        }
        if (job.mode == MODE_FLOW2) {
            set_err("flow2 mode needs W=1, C in {16,32,64}, {A,C,G,T} sequences and "
                    "-127 <= MISMATCH+G_INIT, MATCH+G_INIT <= 127");
            return -1;
        }
    }
    // single long DNA pairs: the barrier-free flow kernel when the row codes fit in LDS
    if (job.mode == MODE_FLOW || (opt[O_mode] < 0 && job.mode == MODE_CHAIN)) {
        const bool fits = job.dna && flow_stage_rows(max_m, job.W, job.C) <= flow_stage_max(job.W, job.C);
        if (fits) {
            job.mode = MODE_FLOW;
        } else if (job.mode == MODE_FLOW) {
            if (opt[O_mode] == MODE_FLOW) {
                set_err("flow mode needs {A,C,G,T} rows that fit in LDS (m <= %d at W=%d)",
                        flow_stage_max(job.W, job.C) - 64 * job.W - 2 * job.C - 80, job.W);
                return -1;
            }
            job.mode = MODE_CHAIN;
        }
    }
    const bool forced_duo = job.mode == MODE_DUO;
    if (forced_duo || (opt[O_mode] < 0 && job.mode == MODE_PAIRWG)) {
        // DNA batches by size (measured, DESIGN.md section 8, kernel ms for duo / PWG / item claim):
        //   fewer pairs than CUs: the flow2 item claim spreads each pair's strip groups
        //     (128 x 8192: 3.87 / 3.53 / 2.46; 128 x 16384: 14.2 / 12.1 / 8.9; 16 x 65536: pairwg
        //     316 / - / 17-18);
        //   fewer than 2 per CU: a pair per workgroup (256 x 8192: 3.92 / 3.24 / 4.68;
        //     256 x 4096: 1.27 / 0.96 / 1.38);
        //   more: the 16-bit duos when exact (512 x 8192: 4.02 / 5.40 / 8.83; C3: 7.29 / 9.95 /
        //     15.1), else a pair per workgroup, else the item claim.
        const int P = (int)job.pairs.size();
        const bool flow2_auto = !forced_duo && P > 1 && job.dna && opt[O_f2pwg] != 0;
        Job w1 = job;
        if (flow2_auto) plan(opt, w1, 1, 64, false, MODE_CHAIN);
        const bool f2ok = flow2_auto && flow2_fits(w1, prm);
        if (f2ok && P < cus) {
            job = w1;
            plan_claim(job, prm, opt);
            return 0;
        }
        // (256 x 8192, kernel ms, flow2 PWG / flow3 PWG at three columns: 3.30 / 2.87; 384: 5.25 / 5.05;
        // 16384 rows, 256 pairs: 12.4 / 11.1; profiles/r06_pwg3_sweep.jsonl)
        if (f2ok && P < 2 * cus && pwg3_fits(w1, prm, opt)) {
            job = w1;
            plan_pwg3(job, opt);
            return 0;
        }
        if (f2ok && P < 2 * cus && pwg_fits(w1, prm, opt, 2)) {
            job = w1;
            plan_pwg(job, prm, opt);
            return 0;
        }
        if (duo_fits(job, prm, opt)) {
            job.mode = MODE_DUO;
            job.duo_f16 = duo_f16_fits(job, prm, opt);
            plan_duos(job);
            return 0;
        }
        if (forced_duo) {
            set_err("duo mode needs MATCH >= 0, a batch whose scores fit 16 bits (MATCH*min(n,m)+MATCH <= 65535) and, for bytes "
                    "outside {A,C,G,T}, MISMATCH < 0 and MATCH - MISMATCH <= 127");
            return -1;
        }
        // scores that need int32: flow3's three-column step with a pair per workgroup at the linear-gap
        // step (C3-shaped batch on int32: 8.88-9.39 ms against flow2's PWG 9.70-9.88 on the same box), else
        // the flow2 step with a pair per workgroup when its round buffer fits (pairwg 18.8 ms -> PWG 9.95
        // ms), else the item claim
        if (f2ok) {
            job = w1;
            if (pwg3_fits(w1, prm, opt, true)) plan_pwg3(job, opt);
            else if (pwg_fits(w1, prm, opt, 2)) plan_pwg(job, prm, opt);
            else plan_claim(job, prm, opt);
        }
    }
    return 0;
}

// Plan of ONE column slab of a pair split across GPUs.
// sw_score_slab_device and sw_slab_bounds share it, so the bounds a rank
// computes are cut for exactly the kernel every rank runs.  W = 1 unless
// forced: the narrowest strips give the shortest wavefront through the ranks.
// Returns the column quantum a slab with an outflow edge must be a multiple
// of -- 63 for flow2 (its last strip's lane 62 is then the slab's last column),
// 64*W for chain / flow (no dead columns at the edge) -- or -1.
int plan_slab(Job& job, int n, int m, bool dna, const Params& prm, const Opts& opt) {
    job.pairs.assign(1, PairDesc{});
    PairDesc& d = job.pairs[0];
    d.n = n;
    d.m = m;
    d.out_idx = 0;
    job.dna = dna;
    job.slab = true;
    const long long fw = opt[O_W];
    const int W = fw ? (int)fw : 1;
    const long long fm = opt[O_mode];
    plan(opt, job, W, pick_C(opt, W), true, fm >= 0 ? (int)fm : MODE_CHAIN);
    if (finalize_mode(job, prm, opt, 256)) return -1;   // one pair: the CU count plays no part
    if (!grouped_mode(job.mode)) {
        set_err("a column slab needs a grouped kernel (chain, flow or flow2), not mode %d", job.mode);
        return -1;
    }
    return job.mode == MODE_FLOW2 ? (job.f2w3 ? 189 : job.f2w2 ? 126 : 63) : 64 * job.W;
}

// Alphabet of a slab call: stated by the caller, never scanned, because every
// rank must plan the same kernel family for its slab.
int slab_dna(const Opts& opt, int flags, bool* dna) {
    const bool bytes = (flags & SW_FLAG_BYTES) || opt[O_bytes];
    if (!bytes && !(flags & SW_FLAG_DNA)) {
        set_err("column slabs need SW_FLAG_DNA or SW_FLAG_BYTES: every rank must plan the same kernel");
        return -1;
    }
    *dna = !bytes;
    return 0;
}

void profile_words(const Params& p, unsigned out[4]) {
    for (int q = 0; q < 4; ++q) {
        unsigned w = 0;
        for (int r = 0; r < 4; ++r) {
            const int s = (r == q ? p.match : p.mismatch) + 128;
            w |= (unsigned)(s & 0xFF) << (8 * r);
        }
        out[q] = w;
    }
}

int waves_per_cu(Ctx* c, const LaunchCfg& cfg) {
    // the duo LDS kernel: its dynamic LDS (wrap buffer, code table) bounds the residency
    const int dkb = cfg.duo_wrap > 0 ? (duo_lds_dyn(cfg) + 1023) / 1024 : 0;
    const int key = (cfg.duo_wrap > 0 ? (dkb * 8 + (cfg.f2_lin ? 1 : 0) + (cfg.duo_f16 ? 2 : 0) + (cfg.duo_tab > 0 ? 4 : 0) + 1) *
                                            1000000 : 0) +
                    cfg.mode * 100000 + cfg.W * 1000 + cfg.C * 2 + (cfg.dna ? 1 : 0);
    auto it = c->waves_cache.find(key);
    if (it != c->waves_cache.end()) return it->second;
    int w = cfg.mode == MODE_FLOW2 ? flow2_waves_per_cu(cfg.C) : kernel_waves_per_cu(cfg);
    if (w <= 0) w = 4;
    c->waves_cache[key] = w;
    return w;
}

// Edges of a column slab (sw_score_slab_device): granule buffers of the left
// and right slab boundaries and the epoch every rank tags them with.
struct SlabEdge {
    Granule* in;
    Granule* out;
    unsigned epoch;
};

// A seven-letter ring launch's rows as perm selectors (sw_flow3.hip HEP: 4 + s for symbols 0..3,
// s - 3 for 4..6), streamed by the ring loops as they are
struct HepSel {
    unsigned char sel[256];
};
__global__ void hep_rows_kernel(const unsigned char* rows, int m, unsigned char* out, HepSel t) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x) out[i] = t.sel[rows[i]];
}

// ---- enqueue: the steps of one launch ---------------------------------------
// What the residency query and the grid rules add to a Variant: workgroups per CU of the streamed flow2 /
// flow3 kernels, the grid, and the ring rows of the wrap ring (ring mode) or of each block's edge ring
// (a pair per workgroup at three columns)
struct Grid {
    int f2_wgs = 1, blocks = 0, wpc = 0, wrap_rows = 0;
};

// flow2 workgroups per CU: the staged kernel (C2) keeps one (a lone wave per SIMD: its step latency is
// the critical path); the streamed kernel of a pair with many strip groups per CU (C5) is
// throughput-bound, and more waves per SIMD hide each other's issue latency (sw_flow2.hip launch_c sizes
// the LDS pad).  Measured (kernel ms, ring | linear edges, 1/2/3/4 per CU):
//   N = 2^17 (520 groups)   9.8 9.7 9.6 9.6   | 9.4 10.8 12.5 12.8
//   N = 2^18 (1040)         32.4 25.2 26.2 26.4 | 31.7 26.3 34.2 32.1
//   N = 2^19 (2080)         116 83.9 80.1 78.9  | 117 83.2 88.5 96.2
//   N = 2^20 (4162, C5)     437 312 287 283     | 454 307 299 -
// ring: one per 2 CUs' worth of groups, up to 4, or one round of all groups when they fit (size_ring);
// three columns per lane: 4 (C5's 1388 groups: 2 / 3 / 4 per CU 159.5 / 156.6 / 155.6 ms; 694 or 925
// blocks 166.4 / 159.3); linear edges: 2 from 4 groups per CU
int pick_f2_wgs(const Job& job, const Variant& v, const Opts& opt, int cus, int items) {
    if (!v.cfg.f2_stream) return 1;
    if (opt[O_f2_wgs] > 0) return (int)opt[O_f2_wgs];
    const int per_cu = items / cus;
    // a pair per workgroup: every pair resident in one pass when the LDS admits it
    // (ceil: cus < P < 2 cus needs 2 per CU, not a second pass of P - cus pairs)
    const int per_cu_ceil = (items + cus - 1) / cus;
    if (v.ring) return items <= cus * F2_WGS_MAX || job.f2w3 ? F2_WGS_MAX : std::min(F2_WGS_MAX, std::max(1, per_cu / 2));
    if (job.f3pwg) return std::min(F2_WGS_MAX, std::max(1, per_cu_ceil));
    if (job.pwg) return std::min({F2_WGS_MAX, std::max(1, per_cu_ceil), flow2_pwg_wgs(v.cfg.max_m, job.C, job.f2w2)});
    return per_cu >= 4 ? 2 : 1;
}

// Ring mode deals groups to blocks statically, so every block must be resident at once: ask the runtime
// how many workgroups of the kernel this launch runs fit a CU (registers, waves and the LDS pad of
// f2_wgs), take no more per CU than that, and size the grid (g.blocks) and the ring arena from it.
int size_ring(Job& job, const Variant& v, const Opts& opt, int cus, int items, Grid& g) {
    LaunchCfg probe = v.cfg;
    int fit = 0;
    for (;; --g.f2_wgs) {
        probe.f2_wgs = g.f2_wgs;
        fit = v.cfg.f3 || v.cfg.f3ra ? flow3_ring_resident(probe) : flow2_stream_resident(probe, true, job.slab);
        if (fit >= g.f2_wgs || g.f2_wgs == 1) break;
    }
    if (fit < 1) {
        set_err("flow2 ring mode: the runtime reports %d resident workgroups per CU for its kernel", fit);
        return -1;
    }
    g.blocks = std::min(items, cus * g.f2_wgs);
    if (opt[O_f2_wgs] <= 0 && items <= cus * g.f2_wgs) {
        // every group in one round (one block each) when they fit the resident blocks:
        // a second round of a few groups runs them alone on their SIMDs after the rest.
        // Measured (column slab 0 alone): 1/8 of C5, 260 groups: 256 blocks (2 rounds)
        // 51.7 ms -> 260 blocks 42.7 ms; 1/4, 520 groups: 512 blocks 77.8 -> 520 60.8 ms.
        // More groups than that keep one block per 2 CUs' worth of groups, a multiple of
        // the CU count (the dispatcher then loads every CU evenly: C5's 2081 groups on
        // 1024 blocks 181.8 ms, on 1041 blocks at up to 5 per CU 205.7 ms).
        g.blocks = items;
        g.f2_wgs = std::max(1, (items + cus - 1) / cus);
    }
    if (opt[O_blocks] > 0) g.blocks = (int)std::min<long long>(opt[O_blocks], items);
    if (g.blocks > cus * fit) {
        set_err("flow2 ring mode needs all %d workgroups co-resident (%d fit per CU, %d CUs)", g.blocks, fit, cus);
        return -1;
    }
    g.wrap_rows = 1;
    while (g.wrap_rows < job.pairs[0].m) g.wrap_rows *= 2;
    job.bnd_granules = (uint64_t)(g.blocks - 1) * (uint64_t)opt[O_ring_rows] + (uint64_t)g.wrap_rows;
    return 0;
}

// The grid of a launch and, where the kernel keeps its edges in rings, their size (job.bnd_granules)
int size_grid(Ctx* c, Job& job, Variant& v, const Opts& opt, size_t np, Grid& g) {
    const int items = job.item_base[np];
    g.f2_wgs = pick_f2_wgs(job, v, opt, c->cus, items);
    if (v.cfg.duo_wrap > 0) job.bnd_granules = 0;   // strip hand-offs in LDS
    if (v.ring && size_ring(job, v, opt, c->cus, items, g)) return -1;
    v.cfg.f2_wgs = g.f2_wgs;
    g.wpc = waves_per_cu(c, v.cfg);
    long long blocks = opt[O_blocks];
    if (blocks <= 0) {
        const int wpb = job.mode == MODE_DUO ? DUO_WAVES : 4;   // waves per workgroup
        const long long cap = (long long)c->cus * std::max(1, g.wpc / wpb);
        // strip mode: 4 independent waves per block; chain: one block per group;
        // pair-per-workgroup: one block per pair (grid-stride over pairs)
        const long long want = job.mode == MODE_STRIP ? (items + 3) / 4 : grouped_mode(job.mode) ? items : (long long)np;   // pairwg/duo: np workgroups
        blocks = std::min<long long>(want, cap);
        // flow2 holds one workgroup per CU (its LDS size forces it); a grid larger than
        // the CU count would only park extra workgroups until a CU frees up
        if (job.mode == MODE_FLOW2) blocks = std::min<long long>(blocks, (long long)c->cus * g.f2_wgs);
    }
    if (v.ring) blocks = g.blocks;   // checked co-resident (size_ring)
    if (job.f3pwg) {
        // one edge ring per block (a pair's strip edge, >= max m rows); the grid: a block per pair up
        // to f2_wgs per CU, blocks running further pairs in turn (no block waits on another)
        blocks = std::min<long long>(np, opt[O_blocks] > 0 ? opt[O_blocks] : (long long)c->cus * g.f2_wgs);
        g.wrap_rows = 64;
        while (g.wrap_rows < v.cfg.max_m) g.wrap_rows *= 2;
        job.bnd_granules = (uint64_t)blocks * (uint64_t)g.wrap_rows;
    }
    v.cfg.blocks = g.blocks = (int)std::max<long long>(1, blocks);
    return 0;
}

// The job's descriptors into the pinned staging buffers, and device buffers for them
int stage_descriptors(Ctx* c, const Job& job, size_t np, bool join, hipStream_t s) {
    const bool duo = job.mode == MODE_DUO;
    const Ctrl* ctrl_before = c->ctrl.p;
    if (join) {   // the descriptors travel in the kernel's arguments: the control block and the join words only
        const size_t join_before = c->join.cap;   // (a grown buffer may come back at the old address)
        const size_t words = (size_t)JOIN_UNITS + (size_t)job.wplan.strips;
        if (c->ctrl.ensure(1, s) || c->join.ensure(words, s)) return -1;
        if (c->ctrl.p != ctrl_before) {
            HIPCHK(hipMemsetAsync(c->ctrl.p, 0, sizeof(Ctrl), s));
            c->item0 = 0;
            c->item0_known = true;
        } else if (!c->item0_known) {   // the launch before was of another kind
            HIPCHK(hipMemsetAsync(c->ctrl.p, 0, sizeof(unsigned), s));
            c->item0 = 0;
            c->item0_known = true;
        }
        if (c->join.cap != join_before) HIPCHK(hipMemsetAsync(c->join.p, 0, c->join.cap * sizeof(unsigned), s));
        return 0;
    }
    // staging buffers may still be read by the previous call's async copies
    if (c->staged_pending) {
        HIPCHK(hipEventSynchronize(c->staged));
        c->staged_pending = false;
    }
    if (c->hdesc.ensure(np) || c->hibase.ensure(np + 1) || c->hduo.ensure(np)) return -1;
    if (duo) std::memcpy(c->hduo.p, job.duos.data(), np * sizeof(DuoDesc));
    else std::memcpy(c->hdesc.p, job.pairs.data(), np * sizeof(PairDesc));
    std::memcpy(c->hibase.p, job.item_base.data(), (np + 1) * sizeof(int));
    if (c->desc.ensure(np, s) || c->duo.ensure(np, s) || c->ibase.ensure(np + 1, s) || c->ctrl.ensure(1, s)) return -1;
    // a fresh control block holds whatever the allocator recycled: clear the sticky
    // error fields once (afterwards only check_ctrl resets them, after reporting)
    if (c->ctrl.p != ctrl_before) HIPCHK(hipMemsetAsync(c->ctrl.p, 0, sizeof(Ctrl), s));
    return 0;
}

// Device-side state of the launch, in stream order: progress / role words zeroed, the edge arena, the
// descriptor copies, the control block and the scores zeroed, and a seven-letter ring launch's rows as
// selectors (m bytes, before the timed kernel)
int prepare_device(Ctx* c, const Job& job, const Variant& v, const Opts& opt, const unsigned char* d_seq, int* d_scores,
                   int nscores, size_t np, bool join, hipStream_t s) {
    // ring mode: a consumer progress word per block; duo roles: one word per CU (XCC, SE, SH, CU of HW_ID)
    const size_t cons = v.ring ? (size_t)v.cfg.blocks * RING_CONS_STRIDE
                        : v.cfg.duo_wrap > 0 && opt[O_duo_roles] != 0 ? (size_t)DUO_CU_WORDS : 0;
    if (cons) {
        if (c->cons.ensure(cons, s)) return -1;
        HIPCHK(hipMemsetAsync(c->cons.p, 0, cons * sizeof(unsigned), s));
    }
    if (job.bnd_granules) {
        size_t freeb = 0, totb = 0;
        HIPCHK(hipMemGetInfo(&freeb, &totb));
        const size_t need = job.bnd_granules * sizeof(Granule);
        if (need > c->bnd.cap * sizeof(Granule) && need > freeb / 10 * 9) {
            set_err("strip-boundary buffers need %.2f GB, %.2f GB free", need / 1e9, freeb / 1e9);
            return -1;
        }
        if (c->bnd.ensure(job.bnd_granules, s)) return -1;
    }
    if (join) {
        // nothing to copy or clear: the claim counter runs on (Ctx::item0) and the kernel's last strip writes the
        // pair's score slot; only the slots of a call's empty pairs are zeroed
        if (nscores > 1) HIPCHK(hipMemsetAsync(d_scores, 0, (size_t)nscores * sizeof(int), s));
        return 0;
    }
    if (job.mode == MODE_DUO) HIPCHK(hipMemcpyAsync(c->duo.p, c->hduo.p, np * sizeof(DuoDesc), hipMemcpyHostToDevice, s));
    else HIPCHK(hipMemcpyAsync(c->desc.p, c->hdesc.p, np * sizeof(PairDesc), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(c->ibase.p, c->hibase.p, (np + 1) * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipEventRecord(c->staged, s));
    c->staged_pending = true;
    HIPCHK(hipMemsetAsync(c->ctrl.p, 0, sizeof(unsigned), s));   // next_item only; error stays sticky
    c->item0_known = false;   // (this launch's kernel leaves its claims in the counter)
    HIPCHK(hipMemsetAsync(d_scores, 0, (size_t)nscores * sizeof(int), s));
    if (v.cfg.hep && v.ring) {
        const PairDesc& d = job.pairs[0];
        if (c->hrows.ensure((size_t)d.m, s)) return -1;
        HepSel t{};
        for (int b = 0; b < 256; ++b) {
            const unsigned sym = job.hsym[b];
            t.sel[b] = (unsigned char)(sym < 4 ? 4 + sym : sym - 3);
        }
        hipLaunchKernelGGL(hep_rows_kernel, dim3((unsigned)std::min(1024, (d.m + 255) / 256)), dim3(256), 0, s,
                           d_seq + d.row_off, d.m, c->hrows.p, t);
        HIPCHK(hipGetLastError());
    }
    return 0;
}

// The score words of the kernels' profile lookups: pure functions of the constants and, for a
// seven-letter alphabet, of the byte-to-symbol map (hsym, else null)
void fill_score_words(KParams& kp, const Params& prm, const unsigned char* hsym) {
    kp.match = prm.match;
    kp.mismatch = prm.mismatch;
    kp.gap_init = prm.gap_init;
    kp.gap_ext = prm.gap_ext;
    profile_words(prm, kp.prof);
    for (int q = 0; q < 4; ++q) {
        unsigned w2 = 0, w3 = 0, pen = 0;
        for (int r = 0; r < 4; ++r) {
            const int sc = r == q ? prm.match : prm.mismatch;
            w2 |= (unsigned)((sc + prm.gap_init) & 0xFF) << (8 * r);
            w3 |= (unsigned)(sc & 0xFF) << (8 * r);
            pen |= (unsigned)(prm.match - sc) << (8 * r);
        }
        kp.prof2[q] = w2;   // flow2: signed bytes s(q, r) + G_INIT
        kp.prof3[q] = w3;   // flow2 W2 column B: signed bytes s(q, r)
        kp.pen[q] = pen;    // duo: penalty bytes MATCH - s(r, q)
    }
    if (!hsym) return;
    // seven-letter alphabet: per column symbol c, row symbols 0..3 high, 4..6 low (sw_flow3.hip HEP)
    std::memcpy(kp.hsym, hsym, sizeof kp.hsym);
    for (int c = 0; c < 7; ++c) {
        unsigned p2 = 0, q2 = 0x80u, p3 = 0, q3 = 0x80u;
        for (int r = 0; r < 7; ++r) {
            const int sc = r == c ? prm.match : prm.mismatch;
            const unsigned b2 = (unsigned)((sc + prm.gap_init) & 0xFF), b3 = (unsigned)(sc & 0xFF);
            if (r < 4) {
                p2 |= b2 << (8 * r);
                p3 |= b3 << (8 * r);
            } else {
                q2 |= b2 << (8 * (r - 3));
                q3 |= b3 << (8 * (r - 3));
            }
        }
        kp.hp2[c] = p2;
        kp.hq2[c] = q2;
        kp.hp3[c] = p3;
        kp.hq3[c] = q3;
    }
}

KParams fill_kparams(Ctx* c, const Job& job, const Variant& v, const Grid& g, const Params& prm, const Opts& opt,
                     const unsigned char* d_seq, int* d_scores, size_t np, const SlabEdge* edge, bool join, hipStream_t s,
                     int* err) {
    KParams kp{};
    kp.seq = d_seq;
    kp.pairs = c->desc.p;
    kp.duos = c->duo.p;
    kp.item_base = c->ibase.p;
    kp.bnd = c->bnd.p;
    kp.ctrl = c->ctrl.p;
    kp.scores = d_scores;
    kp.npairs = (int)np;
    kp.total_items = job.item_base[np];
    // epochs are never 0 (tag of a zeroed granule), nor one that makes flow3's granule key
    // k = epoch ^ 0x5BD1E995 zero in its low 5 bits: a zeroed 8-B granule passes its check when
    // its second word equals k (staged) or k ^ (position << 5) (ring edges), which needs exactly that;
    // the affine granules' E half is keyed k ^ 0x9E3779B9, held to the same rule
    const unsigned epoch_before = c->epoch;
    do ++c->epoch;
    while (c->epoch == 0 || ((c->epoch ^ 0x5BD1E995u) & 31u) == 0 || ((c->epoch ^ 0x5BD1E995u ^ 0x9E3779B9u) & 31u) == 0);
    kp.epoch = c->epoch;
    // (the score word of the joining wedge launches orders its values by epoch: cleared when the epochs wrap)
    if (c->epoch < epoch_before && c->join.p &&
        hipMemsetAsync(c->join.p + JOIN_SCORE, 0, 2 * sizeof(unsigned), s) != hipSuccess)
        *err = -1;
    fill_score_words(kp, prm, v.cfg.hep ? job.hsym : nullptr);
    if (v.cfg.duo_wrap > 0) {
        kp.wrap_rows = v.cfg.duo_wrap;
        if (opt[O_duo_roles] != 0) kp.ring_cons = c->cons.p;   // per-CU role words (zeroed by prepare_device)
        // auto (-1): turn-taking in 1.3 ms slices whenever the LDS row-code table is used.  That is the
        // one-pass batches (one duo per workgroup: the CU's two workgroups would otherwise end ~3 ms
        // apart, C3 6.48 -> 6.30 ms) and, since the table also serves multi-pass batches of rows >= 8192,
        // those too (8192 pairs of 8192: 51.8 -> 50.5 ms with table + turns); the table-less kernel runs
        // without turns (profiles/r05_duo_prio.md)
        const int dp = (int)opt[O_duo_prio];
        kp.duo_prio = dp >= 0 ? dp : v.cfg.duo_tab > 0 ? 17 : 0;
    }
    kp.timeout_ticks = opt[O_timeout] * 100000000LL;   // s_memrealtime: 100 MHz
    kp.stall_item = (int)opt[O_stall_item];
    kp.w45_s4 = v.cfg.f3_w45 ? job.w45_s4 : -1;
    kp.trace = reinterpret_cast<unsigned long long*>(opt[O_trace]);
    if (v.ring) {   // the ring arena is sized (size_ring) and addressed with the one snapshot's ring_rows
        kp.ring_rows = (int)opt[O_ring_rows];
        kp.wrap_rows = g.wrap_rows;
        kp.ring_cons = c->cons.p;
    }
    if (job.f3pwg) kp.wrap_rows = g.wrap_rows;   // each block's edge ring (kp.ring_rows stays 0)
    if (v.wedge) {
        kp.wedge = 1;
        kp.wedge_e0[0] = job.wplan.e0[0];
        kp.wedge_e0[1] = job.wplan.e0[1];
        kp.wedge_rlead = job.wplan.rlead;
        kp.wedge_rows = job.wedge_rows;
        kp.wedge_bnd[0] = job.wedge_bnd[0];
        kp.wedge_bnd[1] = job.wedge_bnd[1];
        for (int j = 0; j < 4; ++j) kp.wedge_drop[j] = job.wplan.drop[j];
        kp.wedge_segr = job.wedge_segr;
        kp.wedge_seg[0] = job.wedge_seg[0];
        kp.wedge_seg[1] = job.wedge_seg[1];
        if (join) {
            kp.wedge_join = c->join.p;
            kp.item0 = c->item0;
            kp.wedge_pair[0] = job.pairs[0];
            kp.wedge_pair[1] = job.pairs[1];
        }
    }
    if (v.cfg.hep && v.ring) kp.hrows = c->hrows.p;
    if (edge) {   // (flow2 then runs its slab kernel, which streams the row codes)
        kp.slab_in = edge->in;
        kp.slab_out = edge->out;
        kp.slab_epoch = edge->epoch;
    }
    return kp;
}

// Enqueue the launch for a planned job whose sequences are in `d_seq`: decide the variant, size the grid,
// stage, launch, record the stats.  edge: the job is a column slab (plan_slab), these are its edges.
int enqueue(Ctx* c, Job& job, const Params& prm, const Opts& opt, const unsigned char* d_seq, int* d_scores, int nscores,
            hipStream_t s, bool time_kernel, const SlabEdge* edge = nullptr) {
    if (job.mode == MODE_FLOW2 ? !flow2_variant_exists(job.C) : !variant_exists(job.W, job.C)) {
        set_err("no kernel variant for W=%d C=%d", job.W, job.C);
        return -1;
    }
    if (opt.f3drops_set < 0) {
        set_err("SWMI_F3WEDGE_DROPS: need d0,d1,d2,d3, multiples of 64 from 64 to %d with d0 == d2", WEDGE_DROP_MAX);
        return -1;
    }
    // one long pair on the staged flow3 linear-gap kernel: two wedges, or two half pairs, from here on
    if (!plan_wedge(job, prm, opt, c->cus)) plan_split(job, prm, opt, c->cus);
    Variant v = select_variant(job, prm, opt, c->cus);
    if (v.err) {
        set_err("%s", v.err);
        return -1;
    }
    const size_t np = job.mode == MODE_DUO ? job.duos.size() : job.pairs.size();
    Grid g;
    // a wedge launch joins its chains inside the staged kernel (sw_flow3.hip f3_join_strip) unless SWMI_F3JOIN=0
    const bool join = v.wedge && opt.f3join != 0;
    if (stage_descriptors(c, job, np, join, s) || size_grid(c, job, v, opt, np, g) ||
        prepare_device(c, job, v, opt, d_seq, d_scores, nscores, np, join, s))
        return -1;
    int kerr = 0;
    const KParams kp = fill_kparams(c, job, v, g, prm, opt, d_seq, d_scores, np, edge, join, s, &kerr);
    if (kerr) {
        set_err("clearing the join words failed");
        return -1;
    }

    if (time_kernel) HIPCHK(hipEventRecord(c->ev0, s));
    HIPCHK(v.cfg.f3 || v.cfg.f3a || v.cfg.f3ra ? launch_sw_flow3(v.cfg, kp, s)
           : job.mode == MODE_FLOW2           ? launch_sw_flow2(v.cfg, kp, s) : launch_sw_strip(v.cfg, kp, s));
    if (v.cut) {   // the crossing term from the halves' final edges (inside the timed span)
        const PairDesc& l = job.pairs[0];
        const PairDesc& r = job.pairs[1];
        const Granule* gl = c->bnd.p + l.bnd_off + (uint64_t)((l.strips + 3) / 4 - 1) * (uint64_t)l.m;
        const Granule* gr = c->bnd.p + r.bnd_off + (uint64_t)((r.strips + 3) / 4 - 1) * (uint64_t)r.m;
        HIPCHK(launch_sw_flow3_combine(gl, gr, l.m, prm.gap_init, kp.epoch, c->ctrl.p, d_scores + l.out_idx, s));
    }
    if (join) {   // (its workgroups claim every item once and one claim more each)
        c->item0 += (unsigned)kp.total_items + (unsigned)v.cfg.blocks;
    } else if (v.steep) {   // the crossing term from the chains' staircases and hand-off columns (inside the timed span)
        const SteepJoin j = {c->bnd.p + job.wedge_bnd[0], c->bnd.p + job.wedge_bnd[1], c->bnd.p + job.pairs[0].bnd_off,
                             c->bnd.p + job.pairs[1].bnd_off, c->bnd.p + job.wedge_seg[0], c->bnd.p + job.wedge_seg[1],
                             job.wedge_rows, job.wedge_segr, job.pairs[0].m, prm.gap_init};
        HIPCHK(launch_sw_flow3_steep_combine(j, job.wplan, kp.epoch, c->ctrl.p, d_scores + job.pairs[0].out_idx, s));
    } else if (v.wedge)   // the crossing term from the chains' staircases (inside the timed span)
        HIPCHK(launch_sw_flow3_wedge_combine(c->bnd.p + job.wedge_bnd[0], c->bnd.p + job.wedge_bnd[1], job.wplan,
                                             job.pairs[0].m, kp.epoch, c->ctrl.p, d_scores + job.pairs[0].out_idx, s));
    if (time_kernel) HIPCHK(hipEventRecord(c->ev1, s));

    t_stats = sw_stats{};
    t_stats.cells = job.cells;
    t_stats.W = job.W;
    t_stats.C = job.C;
    t_stats.dna = job.hep ? 2 : job.dna ? 1 : 0;   // 2: a seven-letter alphabet on the DNA kernels
    t_stats.blocks = v.cfg.blocks;
    t_stats.waves_per_cu = g.wpc;
    t_stats.items = job.item_base[np];
    t_stats.mode = job.mode;
    t_stats.variant = variant_word(v);
    t_stats.boundary_bytes = (long long)(job.bnd_granules * sizeof(Granule));
    c->last = s;
    return 0;
}

int check_ctrl(Ctx* c, hipStream_t s) {
    if (c->hctrl.ensure(1)) return -1;
    HIPCHK(hipMemcpyAsync(c->hctrl.p, c->ctrl.p, sizeof(Ctrl), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (c->hctrl.p->error) {
        if (c->hctrl.p->error == ERR_EDGE)
            set_err("a cut pair's final edge held a row that this launch never wrote (error %u)", c->hctrl.p->error);
        else
            set_err("strip hand-off timed out (error %u, strip %u): a producer strip never published",
                    c->hctrl.p->error, c->hctrl.p->err_item);
        HIPCHK(hipMemsetAsync(c->ctrl.p, 0, sizeof(Ctrl), s));
        c->item0 = 0;
        c->item0_known = true;
        // (a launch that gave up may have left join counters and claims half way)
        if (c->join.p) HIPCHK(hipMemsetAsync(c->join.p, 0, c->join.cap * sizeof(unsigned), s));
        HIPCHK(hipStreamSynchronize(s));
        return -1;
    }
    return 0;
}

struct HostPair {
    const unsigned char* s1;
    int n;   // seq1 length (reference: columns)
    const unsigned char* s2;
    int m;   // seq2 length (reference: rows)
};

// Host pairs validated for the engine (lengths, pointers, score range).
int check_host_pairs(const HostPair* in, int npairs, const Params& prm) {
    if (npairs < 0 || (npairs > 0 && !in)) {
        set_err("invalid arguments");
        return -1;
    }
    if (!params_ok(prm)) return -1;
    for (int k = 0; k < npairs; ++k) {
        if (in[k].n < 0 || in[k].m < 0 || (in[k].n > 0 && !in[k].s1) || (in[k].m > 0 && !in[k].s2)) {
            set_err("pair %d: invalid sequence pointer/length", k);
            return -1;
        }
        if ((long long)std::min(in[k].n, in[k].m) * std::max(prm.match, 1) >= (1LL << 28)) {
            set_err("pair %d: score range exceeds the int32 engine (min length * MATCH >= 2^28)", k);
            return -1;
        }
        if (in[k].n > MAX_SEQ || in[k].m > MAX_SEQ) {
            set_err("pair %d: sequences longer than 2^27 - 1 bytes are not supported", k);
            return -1;
        }
    }
    return 0;
}

// Stage the non-empty pairs in[act[i]] and launch them on c's own stream (asynchronous).
// Pair act[i]'s score goes to d_scores[full ? act[i] : i]; enqueue zeroes the nscores
// ints of d_scores first, so empty pairs of a full-index launch read 0.
int launch_host(Ctx* c, const HostPair* in, const std::vector<int>& act, const Params& prm, const Opts& opt,
                int* d_scores, int nscores, bool full) {
    hipStream_t s = c->own;
    if (c->last && c->last != s) HIPCHK(hipStreamSynchronize(c->last));
    Job job;
    const bool single = act.size() == 1;
    bool dna = opt[O_bytes] == 0;
    size_t bytes = 0;
    for (int k : act) {
        if (dna && !(all_dna(in[k].s1, in[k].n) && all_dna(in[k].s2, in[k].m))) dna = false;
        bytes += ((size_t)in[k].n + 15) / 16 * 16 + ((size_t)in[k].m + 15) / 16 * 16;
    }
    job.dna = dna;
    if (c->hseq.ensure(bytes)) return -1;
    // orientation: a single pair spreads its LONGER sequence over lanes (more
    // strips = more waves); a batch streams its longer sequence as rows (fewer
    // strip fills per cell).  The score is symmetric either way.
    size_t off = 0;
    job.pairs.resize(act.size());
    for (size_t i = 0; i < act.size(); ++i) {
        const HostPair& p = in[act[i]];
        const bool swap = want_swap(opt, single, p.n, p.m);
        const unsigned char* colp = swap ? p.s2 : p.s1;
        const unsigned char* rowp = swap ? p.s1 : p.s2;
        const int n = swap ? p.m : p.n, m = swap ? p.n : p.m;
        PairDesc& d = job.pairs[i];
        d.col_off = off;
        std::memcpy(c->hseq.p + off, colp, (size_t)n);
        off += ((size_t)n + 15) / 16 * 16;
        d.row_off = off;
        std::memcpy(c->hseq.p + off, rowp, (size_t)m);
        off += ((size_t)m + 15) / 16 * 16;
        d.n = n;
        d.m = m;
        d.out_idx = full ? act[i] : (int)i;
    }
    if (!dna && single && opt[O_bytes] == 0) {
        uint32_t set[8] = {};
        byte_set(in[act[0]].s1, in[act[0]].n, set);
        byte_set(in[act[0]].s2, in[act[0]].m, set);
        set_hep(job, opt, set);
    }
    const int W = pick_W(opt, job.pairs, single);
    plan(opt, job, W, pick_C(opt, W), single);
    if (finalize_alphabet(job, prm, opt, c->cus, single)) return -1;
    if (c->seq.ensure(bytes, s)) return -1;
    HIPCHK(hipMemcpyAsync(c->seq.p, c->hseq.p, bytes, hipMemcpyHostToDevice, s));
    return enqueue(c, job, prm, opt, c->seq.p, d_scores, nscores, s, true);
}

// Synchronous host-buffer path shared by every host API entry.
int score_host(const HostPair* in, int npairs, const Params& prm, int* out) {
    const auto t0 = std::chrono::steady_clock::now();
    const Opts opt = snapshot_opts();
    if (npairs > 0 && !out) {
        set_err("invalid arguments");
        return -1;
    }
    if (check_host_pairs(in, npairs, prm)) return -1;
    std::vector<int> act;
    for (int k = 0; k < npairs; ++k) {
        out[k] = 0;   // empty pairs score 0 (main.cpp:74-90 with empty loops)
        if (in[k].n > 0 && in[k].m > 0) act.push_back(k);
    }
    if (act.empty()) return 0;
    Ctx* c = get_ctx();
    if (!c) return -1;
    hipStream_t s = c->own;
    if (c->scores.ensure(act.size(), s) || c->hscores.ensure(act.size())) return -1;
    if (launch_host(c, in, act, prm, opt, c->scores.p, (int)act.size(), false)) return -1;
    HIPCHK(hipMemcpyAsync(c->hscores.p, c->scores.p, act.size() * sizeof(int), hipMemcpyDeviceToHost, s));
    if (check_ctrl(c, s)) return -1;   // synchronises
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    for (size_t i = 0; i < act.size(); ++i) out[act[i]] = c->hscores.p[i];
    t_stats.kernel_ms = ms;
    t_stats.total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return 0;
}

// One device's shard of a multi-GPU batch (sw_score_batch_multi): the scores of
// in[0..npairs) stay in device memory, *d_out (npairs ints of this thread's context).
int score_host_device(const HostPair* in, int npairs, const Params& prm, const Opts& opt, int** d_out, float* kernel_ms) {
    *kernel_ms = 0.f;
    Ctx* c = get_ctx();
    if (!c) return -1;
    hipStream_t s = c->own;
    if (c->scores.ensure((size_t)std::max(npairs, 1), s)) return -1;
    *d_out = c->scores.p;
    std::vector<int> act;
    for (int k = 0; k < npairs; ++k)
        if (in[k].n > 0 && in[k].m > 0) act.push_back(k);
    if (act.empty()) {
        if (npairs > 0) HIPCHK(hipMemsetAsync(c->scores.p, 0, (size_t)npairs * sizeof(int), s));
        HIPCHK(hipStreamSynchronize(s));
        return 0;
    }
    if (launch_host(c, in, act, prm, opt, c->scores.p, npairs, true)) return -1;
    if (check_ctrl(c, s)) return -1;   // synchronises
    HIPCHK(hipEventElapsedTime(kernel_ms, c->ev0, c->ev1));
    return 0;
}

Params current_params() {
    std::lock_guard<std::mutex> g(g_param_mu);
    return g_params;
}

int score_one(const unsigned char* s1, const unsigned char* s2, int n, int m, const Params& prm) {
    HostPair hp{s1, n, s2, m};
    int sc = 0;
    if (score_host(&hp, 1, prm, &sc)) return -1;
    return sc;
}

// flag[0] |= 1 when a byte outside {A,C,G,T} occurs; with set (one pair): flag[1..8] |= the byte set.
// Pair blockIdx.x / per, its n + m bytes split over `per` blocks.
__global__ void alphabet_kernel(const unsigned char* arena, const PairDesc* pairs, int npairs, unsigned* flag, int set,
                                int per) {
    __shared__ unsigned bits[8];
    const int k = (int)blockIdx.x / per, slice = (int)blockIdx.x % per;
    if (k >= npairs) return;
    if (threadIdx.x < 8) bits[threadIdx.x] = 0u;
    __syncthreads();
    const PairDesc d = pairs[k];
    unsigned bad = 0;
    for (int i = slice * blockDim.x + threadIdx.x; i < d.n + d.m; i += per * blockDim.x) {
        const unsigned char ch = i < d.n ? arena[d.col_off + i] : arena[d.row_off + (i - d.n)];
        const bool b = !(ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T');
        bad |= b;
        // (a read before the atomic: only a value's first sightings write)
        if (set && !(bits[ch >> 5] >> (ch & 31) & 1u)) atomicOr(&bits[ch >> 5], 1u << (ch & 31));
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1u);
    __syncthreads();
    if (set && threadIdx.x < 8 && bits[threadIdx.x]) atomicOr(flag + 1 + threadIdx.x, bits[threadIdx.x]);
}

}  // namespace

// the thread's sw_last_error() text, for the other host modules (sw_db.hip)
void report_error(const char* msg) { set_err("%s", msg); }
// the thread's sw_last_stats(), for a launch made by another module (sw_matrix.hip)
void report_stats(const sw_stats& s) { t_stats = s; }

// ---- multi-GPU batch (sw_score_batch_multi) ---------------------------------
// Contiguous shard of pair rank r of ngpus (sizes differ by <= 1): the partition of
// concurrentproject_amd/dist.py shard_bounds.
void batch_shard(int npairs, int ngpus, int r, int* lo, int* hi) {
    const int base = npairs / ngpus, extra = npairs % ngpus;
    *lo = r * base + std::min(r, extra);
    *hi = *lo + base + (r < extra ? 1 : 0);
}

// RCCL, loaded at first use (dlopen: the library has no link-time RCCL dependency, and a
// process that already holds librccl.so.1 -- PyTorch's -- shares that copy).
struct Rccl {
    bool tried = false, ok = false;
    std::string why;
    ncclResult_t (*comm_init_all)(ncclComm_t*, int, const int*) = nullptr;
    ncclResult_t (*group_start)() = nullptr;
    ncclResult_t (*group_end)() = nullptr;
    ncclResult_t (*send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    const char* (*err)(ncclResult_t) = nullptr;
    bool load() {
        if (tried) return ok;
        tried = true;
        void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) {
            why = std::string("dlopen librccl.so.1: ") + dlerror();
            return false;
        }
        comm_init_all = (decltype(comm_init_all))dlsym(h, "ncclCommInitAll");
        group_start = (decltype(group_start))dlsym(h, "ncclGroupStart");
        group_end = (decltype(group_end))dlsym(h, "ncclGroupEnd");
        send = (decltype(send))dlsym(h, "ncclSend");
        recv = (decltype(recv))dlsym(h, "ncclRecv");
        err = (decltype(err))dlsym(h, "ncclGetErrorString");
        ok = comm_init_all && group_start && group_end && send && recv && err;
        if (!ok) why = "librccl.so.1 lacks ncclCommInitAll/ncclGroupStart/ncclGroupEnd/ncclSend/ncclRecv";
        return ok;
    }
};

// One host thread per device, created once: its thread-local engine context (stream,
// buffers) then lives as long as the process, like a caller's own thread.
struct DevWorker {
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    std::function<void()> job;
    bool busy = false;
    void start() {
        th = std::thread([this] {
            for (;;) {
                std::function<void()> f;
                {
                    std::unique_lock<std::mutex> g(mu);
                    cv.wait(g, [this] { return busy && job; });
                    f = std::move(job);
                }
                f();
                {
                    std::lock_guard<std::mutex> g(mu);
                    busy = false;
                }
                cv.notify_all();
            }
        });
        th.detach();
    }
    void post(std::function<void()> f) {
        std::lock_guard<std::mutex> g(mu);
        job = std::move(f);
        busy = true;
        cv.notify_all();
    }
    void wait() {
        std::unique_lock<std::mutex> g(mu);
        cv.wait(g, [this] { return !busy; });
    }
};

struct MultiState {
    std::mutex mu;                          // one multi-GPU call at a time
    Rccl rccl;
    std::vector<DevWorker*> workers;        // per device
    std::map<int, std::vector<ncclComm_t>> comms;   // ngpus -> communicator clique of devices 0..ngpus-1
    std::vector<hipStream_t> streams;       // per device, for the gather
    int* d_gather = nullptr;                // device 0
    size_t gather_cap = 0;
    int* h_scores = nullptr;                // pinned
    size_t h_cap = 0;
};
MultiState& multi_state() {
    static MultiState* st = new MultiState();   // never destroyed: detached workers use it
    return *st;
}

// The gather of a multi-GPU batch: device r's shard [lo_r, hi_r) of the
// int32 scores lands in device 0's gather buffer at offset lo_r.  Entry r of the plan: the
// count device r sends and the offset it lands at (r = 0: the local device-to-device copy).
// Host-only, so the send/recv plan is testable without a second GPU (sw_batch_gather_plan).
void gather_plan(int npairs, int ngpus, int* count, int* offset) {
    for (int r = 0; r < ngpus; ++r) {
        int lo = 0, hi = 0;
        batch_shard(npairs, ngpus, r, &lo, &hi);
        count[r] = hi - lo;
        offset[r] = lo;
    }
}

// Restores the calling thread's HIP device on every exit path of score_multi.
struct DeviceGuard {
    int dev = -1;
    ~DeviceGuard() {
        if (dev >= 0) (void)hipSetDevice(dev);
    }
};

#define NCCLCHK(expr)                                                                   \
    do {                                                                                \
        ncclResult_t r_ = (expr);                                                       \
        if (r_ != ncclSuccess) {                                                        \
            set_err("%s failed: %s", #expr, st.rccl.err ? st.rccl.err(r_) : "rccl");   \
            return -1;                                                                  \
        }                                                                               \
    } while (0)

// Inside ncclGroupStart/End: on a failed send or recv the group is closed before returning,
// so the thread's RCCL group state is clean for the next call.
#define NCCLCHK_GROUP(expr)                                                             \
    do {                                                                                \
        ncclResult_t r_ = (expr);                                                       \
        if (r_ != ncclSuccess) {                                                        \
            set_err("%s failed: %s", #expr, st.rccl.err ? st.rccl.err(r_) : "rccl");   \
            (void)st.rccl.group_end();                                                  \
            return -1;                                                                  \
        }                                                                               \
    } while (0)

int score_multi(const HostPair* in, int npairs, const Params& prm, int* out, int ngpus) {
    const auto t0 = std::chrono::steady_clock::now();
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (ngpus < 1 || ngpus > ndev) {
        set_err("sw_score_batch_multi: ngpus = %d, but %d HIP device(s) are visible", ngpus, ndev);
        return -1;
    }
    if (npairs > 0 && !out) {
        set_err("invalid arguments");
        return -1;
    }
    if (check_host_pairs(in, npairs, prm)) return -1;
    if (npairs == 0) return 0;
    const Opts opt = snapshot_opts();   // one for every device's worker
    MultiState& st = multi_state();
    std::lock_guard<std::mutex> g(st.mu);
    if (ngpus > 1 && !st.rccl.load()) {
        set_err("sw_score_batch_multi: %s", st.rccl.why.c_str());
        return -1;
    }
    while ((int)st.workers.size() < ngpus) {
        st.workers.push_back(new DevWorker());
        st.workers.back()->start();
    }
    // every device scores its contiguous shard on its own host thread and stream
    std::vector<int> rc(ngpus, 0), cnt(ngpus), off(ngpus);
    gather_plan(npairs, ngpus, cnt.data(), off.data());
    std::vector<int*> dptr(ngpus, nullptr);
    std::vector<float> kms(ngpus, 0.f);
    std::vector<std::string> errs(ngpus);
    for (int r = 0; r < ngpus; ++r) {
        st.workers[r]->post([&, r] {
            if (hipSetDevice(r) != hipSuccess) {
                rc[r] = -1;
                errs[r] = "hipSetDevice failed";
                return;
            }
            rc[r] = score_host_device(in + off[r], cnt[r], prm, opt, &dptr[r], &kms[r]);
            if (rc[r]) errs[r] = t_err;
        });
    }
    for (int r = 0; r < ngpus; ++r) st.workers[r]->wait();
    for (int r = 0; r < ngpus; ++r)
        if (rc[r]) {
            set_err("sw_score_batch_multi: device %d: %s", r, errs[r].c_str());
            return -1;
        }
    DeviceGuard dg;
    HIPCHK(hipGetDevice(&dg.dev));
    while ((int)st.streams.size() < ngpus) {
        HIPCHK(hipSetDevice((int)st.streams.size()));
        hipStream_t sx = nullptr;
        HIPCHK(hipStreamCreateWithFlags(&sx, hipStreamNonBlocking));
        st.streams.push_back(sx);
    }
    HIPCHK(hipSetDevice(0));
    if ((size_t)npairs > st.gather_cap) {
        // allocate the new buffers first, commit them only when both exist
        int* dg_new = nullptr;
        int* hs_new = nullptr;
        HIPCHK(hipMalloc((void**)&dg_new, (size_t)npairs * sizeof(int)));
        if (hipHostMalloc((void**)&hs_new, (size_t)npairs * sizeof(int), hipHostMallocDefault) != hipSuccess) {
            (void)hipFree(dg_new);
            set_err("sw_score_batch_multi: hipHostMalloc of %d scores failed", npairs);
            return -1;
        }
        if (st.d_gather) (void)hipFree(st.d_gather);
        if (st.h_scores) (void)hipHostFree(st.h_scores);
        st.d_gather = dg_new;
        st.h_scores = hs_new;
        st.gather_cap = (size_t)npairs;
    }
    // device 0's own shard, then the others' int32 scores over RCCL (the only exchange)
    if (cnt[0] > 0)
        HIPCHK(hipMemcpyAsync(st.d_gather + off[0], dptr[0], (size_t)cnt[0] * sizeof(int), hipMemcpyDeviceToDevice,
                              st.streams[0]));
    if (ngpus > 1) {
        auto it = st.comms.find(ngpus);
        if (it == st.comms.end()) {
            std::vector<ncclComm_t> cl(ngpus);
            std::vector<int> devs(ngpus);
            for (int r = 0; r < ngpus; ++r) devs[r] = r;
            NCCLCHK(st.rccl.comm_init_all(cl.data(), ngpus, devs.data()));
            it = st.comms.emplace(ngpus, cl).first;
        }
        const std::vector<ncclComm_t>& cl = it->second;
        NCCLCHK(st.rccl.group_start());
        for (int r = 1; r < ngpus; ++r) {
            if (!cnt[r]) continue;
            NCCLCHK_GROUP(st.rccl.send(dptr[r], (size_t)cnt[r], ncclInt32, 0, cl[r], st.streams[r]));
            NCCLCHK_GROUP(st.rccl.recv(st.d_gather + off[r], (size_t)cnt[r], ncclInt32, r, cl[0], st.streams[0]));
        }
        NCCLCHK(st.rccl.group_end());
    }
    HIPCHK(hipSetDevice(0));
    HIPCHK(hipMemcpyAsync(st.h_scores, st.d_gather, (size_t)npairs * sizeof(int), hipMemcpyDeviceToHost,
                          st.streams[0]));
    for (int r = 0; r < ngpus; ++r) {
        HIPCHK(hipSetDevice(r));
        HIPCHK(hipStreamSynchronize(st.streams[r]));
    }
    std::memcpy(out, st.h_scores, (size_t)npairs * sizeof(int));
    t_stats = sw_stats{};
    for (int r = 0; r < ngpus; ++r) t_stats.kernel_ms = std::max(t_stats.kernel_ms, kms[r]);
    for (int k = 0; k < npairs; ++k) t_stats.cells += (long long)in[k].n * in[k].m;
    t_stats.total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return 0;
}
#undef NCCLCHK
#undef NCCLCHK_GROUP

hipError_t raise_dyn_lds(const void* fn, int bytes) {
    static std::mutex mu;
    static std::set<std::pair<const void*, int>> done;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> g(mu);
    if (done.count({fn, dev})) return hipSuccess;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) done.insert({fn, dev});
    return e;
}

}  // namespace swmi

using namespace swmi;

extern "C" {

int SequentialSmithWatermanScoreGPU(unsigned char* seq1, unsigned char* seq2, int len1, int len2) {
    return score_one(seq1, seq2, len1, len2, current_params());
}

int SmithWatermanLazyGPU(const unsigned char* seq1, const unsigned char* seq2, int n, int m) {
    return score_one(seq1, seq2, n, m, current_params());
}

int SmithWatermanScoreCUDA(const unsigned char* seq1, const unsigned char* seq2, int n, int m) {
    return score_one(seq1, seq2, n, m, current_params());
}

int SmithDiagonalGPU(unsigned char* seq1, unsigned char* seq2, int n, int m) {
    Params p = current_params();
    p.gap_ext = p.gap_init;   // linear gap (SmithDiagonalGPU.cu:59-66)
    return score_one(seq1, seq2, n, m, p);
}

int sw_set_params(int match, int mismatch, int gap_init, int gap_ext) {
    Params p;
    p.match = match;
    p.mismatch = mismatch;
    p.gap_init = gap_init;
    p.gap_ext = gap_ext;
    if (!params_ok(p)) return -1;
    std::lock_guard<std::mutex> g(g_param_mu);
    g_params = p;
    return 0;
}

void sw_get_params(int* match, int* mismatch, int* gap_init, int* gap_ext) {
    Params p = current_params();
    if (match) *match = p.match;
    if (mismatch) *mismatch = p.mismatch;
    if (gap_init) *gap_init = p.gap_init;
    if (gap_ext) *gap_ext = p.gap_ext;
}

int sw_score_params(const unsigned char* seq1, const unsigned char* seq2, int n, int m, int match, int mismatch,
                    int gap_init, int gap_ext) {
    Params p;
    p.match = match;
    p.mismatch = mismatch;
    p.gap_init = gap_init;
    p.gap_ext = gap_ext;
    return score_one(seq1, seq2, n, m, p);
}

int sw_score_batch(const unsigned char* const* a, const int* alen, const unsigned char* const* b, const int* blen,
                   int npairs, int* scores_out) {
    if (npairs < 0 || (npairs > 0 && (!a || !alen || !b || !blen || !scores_out))) {
        set_err("sw_score_batch: invalid arguments");
        return -1;
    }
    std::vector<HostPair> v((size_t)npairs);
    for (int k = 0; k < npairs; ++k) v[k] = HostPair{a[k], alen[k], b[k], blen[k]};
    return score_host(v.data(), npairs, current_params(), scores_out);
}

int sw_score_batch_multi(const unsigned char* const* a, const int* alen, const unsigned char* const* b,
                         const int* blen, int npairs, int* scores_out, int ngpus) {
    if (npairs < 0 || (npairs > 0 && (!a || !alen || !b || !blen || !scores_out))) {
        set_err("sw_score_batch_multi: invalid arguments");
        return -1;
    }
    std::vector<HostPair> v((size_t)npairs);
    for (int k = 0; k < npairs; ++k) v[k] = HostPair{a[k], alen[k], b[k], blen[k]};
    return score_multi(v.data(), npairs, current_params(), scores_out, ngpus);
}

int sw_batch_shard(int npairs, int ngpus, int rank, int* lo, int* hi) {
    if (npairs < 0 || ngpus < 1 || rank < 0 || rank >= ngpus || !lo || !hi) {
        set_err("sw_batch_shard: invalid arguments");
        return -1;
    }
    batch_shard(npairs, ngpus, rank, lo, hi);
    return 0;
}

int sw_batch_gather_plan(int npairs, int ngpus, int* count, int* offset) {
    if (npairs < 0 || ngpus < 1 || !count || !offset) {
        set_err("sw_batch_gather_plan: invalid arguments");
        return -1;
    }
    gather_plan(npairs, ngpus, count, offset);
    return 0;
}

int sw_score_batch_device(const unsigned char* d_arena, const int64_t* a_off, const int* alen, const int64_t* b_off,
                          const int* blen, int npairs, int* d_scores, int flags, void* stream) {
    const auto t0 = std::chrono::steady_clock::now();
    if (npairs <= 0 || !d_arena || !a_off || !alen || !b_off || !blen || !d_scores) {
        set_err("sw_score_batch_device: invalid arguments");
        return -1;
    }
    const Params prm = current_params();
    const Opts opt = snapshot_opts();
    if (!params_ok(prm)) return -1;
    Ctx* c = get_ctx();
    if (!c) return -1;
    hipStream_t s = stream ? (hipStream_t)stream : c->own;
    if (c->last && c->last != s) HIPCHK(hipStreamSynchronize(c->last));
    Job job;
    std::vector<int> idx;   // non-empty pairs; empty ones keep the memset 0
    for (int k = 0; k < npairs; ++k) {
        if (alen[k] < 0 || blen[k] < 0 || a_off[k] < 0 || b_off[k] < 0) {
            set_err("pair %d: negative length/offset", k);
            return -1;
        }
        if ((long long)std::min(alen[k], blen[k]) * std::max(prm.match, 1) >= (1LL << 28)) {
            set_err("pair %d: score range exceeds the int32 engine", k);
            return -1;
        }
        if (alen[k] > MAX_SEQ || blen[k] > MAX_SEQ) {
            set_err("pair %d: sequences longer than 2^27 - 1 bytes are not supported", k);
            return -1;
        }
        if (alen[k] > 0 && blen[k] > 0) idx.push_back(k);
    }
    job.pairs.resize(idx.size());
    const bool single = idx.size() == 1;
    for (size_t i = 0; i < idx.size(); ++i) {
        const int k = idx[i];
        const bool swap = want_swap(opt, single, alen[k], blen[k]);
        PairDesc& d = job.pairs[i];
        d.col_off = (uint64_t)(swap ? b_off[k] : a_off[k]);
        d.row_off = (uint64_t)(swap ? a_off[k] : b_off[k]);
        d.n = swap ? blen[k] : alen[k];
        d.m = swap ? alen[k] : blen[k];
        d.out_idx = k;
    }
    if (job.pairs.empty()) {
        HIPCHK(hipMemsetAsync(d_scores, 0, (size_t)npairs * sizeof(int), s));
        if (!stream) HIPCHK(hipStreamSynchronize(s));
        return 0;
    }
    const int W = pick_W(opt, job.pairs, single);
    plan(opt, job, W, pick_C(opt, W), single);
    if (flags & SW_FLAG_BYTES || opt[O_bytes]) {
        job.dna = false;
    } else if (flags & SW_FLAG_DNA) {
        job.dna = true;
    } else {
        // scan the alphabet on the device (one block per pair)
        const size_t np = job.pairs.size();
        if (c->staged_pending) {
            HIPCHK(hipEventSynchronize(c->staged));
            c->staged_pending = false;
        }
        // (one pair: the byte set too, for the seven-letter path)
        const int set = single && opt[O_hep] != 0 ? 1 : 0;
        // (the pinned control block, 3 x 16 B, takes the flag and the byte set back)
        if (c->hdesc.ensure(np) || c->desc.ensure(np, s) || c->flag.ensure(9, s) || c->hctrl.ensure(3)) return -1;
        std::memcpy(c->hdesc.p, job.pairs.data(), np * sizeof(PairDesc));
        HIPCHK(hipMemcpyAsync(c->desc.p, c->hdesc.p, np * sizeof(PairDesc), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemsetAsync(c->flag.p, 0, 9 * sizeof(unsigned), s));
        // one pair: its bytes over up to 128 blocks (a C5 pair is 2 MB); a batch: one block per pair
        long long longest = 0;
        for (const PairDesc& d : job.pairs) longest = std::max(longest, (long long)d.n + d.m);
        const int per = np == 1 ? (int)std::max(1LL, std::min(128LL, longest / 8192)) : 1;
        hipLaunchKernelGGL(alphabet_kernel, dim3((unsigned)(np * per)), dim3(256), 0, s, d_arena, c->desc.p, (int)np,
                           c->flag.p, set, per);
        HIPCHK(hipGetLastError());
        unsigned* hflag = reinterpret_cast<unsigned*>(c->hctrl.p);
        HIPCHK(hipMemcpyAsync(hflag, c->flag.p, 9 * sizeof(unsigned), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        job.dna = hflag[0] == 0;
        if (!job.dna && set) {
            uint32_t bits[8];
            std::memcpy(bits, hflag + 1, sizeof bits);
            set_hep(job, opt, bits);
        }
    }
    if (finalize_alphabet(job, prm, opt, c->cus, single)) return -1;
    if (enqueue(c, job, prm, opt, d_arena, d_scores, npairs, s, !stream)) return -1;
    if (!stream) {
        if (check_ctrl(c, s)) return -1;
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
        t_stats.kernel_ms = ms;
    }
    t_stats.total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return 0;
}

int sw_slab_bounds(long long n, int m, int nslabs, int flags, long long* bounds) {
    if (n <= 0 || n > (1LL << 30) || m <= 0 || nslabs <= 0 || !bounds) {
        set_err("sw_slab_bounds: invalid arguments");
        return -1;
    }
    const Opts opt = snapshot_opts();
    bool dna = true;
    if (slab_dna(opt, flags, &dna)) return -1;
    Job job;
    const int q = plan_slab(job, (int)n, m, dna, current_params(), opt);   // the quantum does not depend on n
    if (q < 0) return -1;
    const long long per = n / nslabs / q * q;
    if (nslabs > 1 && per == 0) {
        set_err("%lld columns cannot be cut into %d slabs of a multiple of %d columns", n, nslabs, q);
        return -1;
    }
    for (int r = 0; r < nslabs; ++r) bounds[r] = per * r;   // the last slab takes the remainder
    bounds[nslabs] = n;
    return q;
}

int sw_split_bounds(int n, int* cut, int* lead) {
    if (n <= 0 || !cut || !lead) {
        set_err("sw_split_bounds: invalid arguments");
        return -1;
    }
    int c = 0, l = 0;
    if (!split_cols(n, &c, &l)) return 0;
    *cut = c;
    *lead = l;
    return c / 126 + (n - c + l) / 126;
}

int sw_score_slab_device(const unsigned char* d_arena, int64_t col_off, int n, int64_t row_off, int m,
                         void* d_inflow, void* d_outflow, unsigned epoch, int* d_score, int flags, void* stream) {
    const auto t0 = std::chrono::steady_clock::now();
    if (!d_arena || !d_score || n <= 0 || m <= 0 || col_off < 0 || row_off < 0) {
        set_err("sw_score_slab_device: invalid arguments");
        return -1;
    }
    if ((d_inflow || d_outflow) && epoch == 0) {
        set_err("sw_score_slab_device: epoch 0 is the tag of a never-written granule");
        return -1;
    }
    const Opts opt = snapshot_opts();
    bool dna = true;
    if (slab_dna(opt, flags, &dna)) return -1;
    const Params prm = current_params();
    if (!params_ok(prm)) return -1;
    // H of any cell is at most MATCH * (its row), whatever the slab's column range
    if ((long long)m * std::max(prm.match, 1) >= (1LL << 28)) {
        set_err("slab: rows * MATCH >= 2^28 exceeds the int32 engine");
        return -1;
    }
    if (m > MAX_SEQ) {
        set_err("slab: more than 2^27 - 1 rows are not supported");
        return -1;
    }
    Ctx* c = get_ctx();
    if (!c) return -1;
    hipStream_t s = stream ? (hipStream_t)stream : c->own;
    if (c->last && c->last != s) HIPCHK(hipStreamSynchronize(c->last));
    Job job;
    const int q = plan_slab(job, n, m, dna, prm, opt);
    if (q < 0) return -1;
    if (d_outflow && n % q != 0) {
        set_err("a slab with an outflow edge must be a multiple of %d columns (sw_slab_bounds), got %d", q, n);
        return -1;
    }
    job.pairs[0].col_off = (uint64_t)col_off;
    job.pairs[0].row_off = (uint64_t)row_off;
    const SlabEdge edge{static_cast<Granule*>(d_inflow), static_cast<Granule*>(d_outflow), epoch};
    if (enqueue(c, job, prm, opt, d_arena, d_score, 1, s, !stream, &edge)) return -1;
    if (!stream) {
        if (check_ctrl(c, s)) return -1;
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
        t_stats.kernel_ms = ms;
    }
    t_stats.total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return 0;
}

int sw_slab_alloc(int m, void** d_buf, void* ipc_handle) {
    if (m <= 0 || !d_buf) {
        set_err("sw_slab_alloc: invalid arguments");
        return -1;
    }
    const size_t bytes = (size_t)m * sizeof(Granule);
    // fine-grained: coherent for a peer GPU's writes while the consuming kernel polls
    // (DESIGN.md section 7).  A buffer exported for another process (ipc_handle) is the
    // inflow of a cross-GPU slab edge: it must be fine-grained, and the plain-memory
    // fallback is refused unless option slab_plain = 1 (one-GPU tests only); a buffer
    // of this process alone may fall back to plain device memory.
    const int last_kind = ipc_handle && !sw_get_option("slab_plain") ? 1 : 2;
    for (int kind = 1; kind <= last_kind; ++kind) {
        void* p = nullptr;
        const hipError_t e = kind == 1 ? hipExtMallocWithFlags(&p, bytes, hipDeviceMallocFinegrained)
                                       : hipMalloc(&p, bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            if (kind == last_kind) {
                set_err(kind == 1 ? "sw_slab_alloc: fine-grained device memory unavailable (%s): a slab edge "
                                    "written by another GPU needs it (option slab_plain = 1 allows plain memory "
                                    "for one-GPU tests)"
                                  : "sw_slab_alloc: %s",
                        hipGetErrorString(e));
                return -1;
            }
            continue;
        }
        HIPCHK(hipMemset(p, 0, bytes));   // tag 0: no granule is valid before its epoch is written
        if (ipc_handle) {
            hipIpcMemHandle_t h;
            const hipError_t ei = hipIpcGetMemHandle(&h, p);
            if (ei != hipSuccess) {
                (void)hipGetLastError();
                (void)hipFree(p);
                if (kind == last_kind) {
                    set_err(kind == 1 ? "sw_slab_alloc: fine-grained memory cannot be exported (hipIpcGetMemHandle: "
                                        "%s): a slab edge written by another GPU needs it (option slab_plain = 1 "
                                        "allows plain memory for one-GPU tests)"
                                      : "hipIpcGetMemHandle failed: %s",
                            hipGetErrorString(ei));
                    return -1;
                }
                continue;
            }
            std::memcpy(ipc_handle, &h, sizeof h);
        }
        *d_buf = p;
        return kind;
    }
    return -1;
}

int sw_slab_free(void* d_buf) {
    if (d_buf) HIPCHK(hipFree(d_buf));
    return 0;
}

int sw_ipc_open(const void* ipc_handle, void** d_ptr) {
    if (!ipc_handle || !d_ptr) {
        set_err("sw_ipc_open: invalid arguments");
        return -1;
    }
    hipIpcMemHandle_t h;
    std::memcpy(&h, ipc_handle, sizeof h);
    HIPCHK(hipIpcOpenMemHandle(d_ptr, h, hipIpcMemLazyEnablePeerAccess));
    return 0;
}

int sw_ipc_close(void* d_ptr) {
    if (d_ptr) HIPCHK(hipIpcCloseMemHandle(d_ptr));
    return 0;
}

int sw_stream_status(void* stream) {
    Ctx* c = get_ctx();
    if (!c) return -1;
    hipStream_t s = stream ? (hipStream_t)stream : c->own;
    if (!c->ctrl.p) return 0;
    const int rc = check_ctrl(c, s);   // synchronises s
    // Nothing of this context is pending on a caller's stream any more, so the next call need not
    // wait for it -- and must not: the caller may destroy the stream now (sw_db_close destroys the
    // database's after sw_db_search_db), and launch_host would synchronise a dead handle.
    if (c->last == s && s != c->own) c->last = nullptr;
    return rc;
}

int sw_set_option(const char* key, long long v) {
    if (!key) return -1;
    const int i = find_opt(key);
    if (i < 0) {
        set_err("unknown option '%s'", key);
        return -1;
    }
    const OptRow& r = OPT_ROWS[i];
    if (v < r.lo || v > r.hi || (r.ok && !r.ok(v))) return -1;
    g_opt[i] = r.flag ? (v != 0) : v;
    return 0;
}

long long sw_get_option(const char* key) {
    const int i = key ? find_opt(key) : -1;
    return i < 0 ? -1 : g_opt[i].load();
}

const char* sw_option_name(int i) { return i >= 0 && i < OPT_COUNT ? OPT_ROWS[i].key : nullptr; }

int sw_last_stats(sw_stats* out) {
    if (!out) return -1;
    *out = t_stats;
    return 0;
}

const char* sw_last_error(void) { return t_err.c_str(); }

int sw_version(void) { return 1; }

}  // extern "C"

// ---- synthetic inputs (bench / harness; not on the score path) -------------
// std::mt19937_64(seed) with a[i] then b[i] per position (cudaSmithM.cu:204-212).
// uniform_int_distribution<int>(0,3) over a 64-bit engine is, in libstdc++ 11
// (bits/uniform_int_dist.h _S_nd), (draw * 4) >> 64 == draw >> 62; written out
// here so the bytes do not depend on the host's C++ library.
#include <random>
extern "C" {
void sw_gen_pair(uint64_t seed, int len, unsigned char* a, unsigned char* b) {
    static const char nts[4] = {'A', 'C', 'G', 'T'};
    std::mt19937_64 g(seed);
    for (int i = 0; i < len; ++i) {
        a[i] = (unsigned char)nts[g() >> 62];
        b[i] = (unsigned char)nts[g() >> 62];
    }
}
// npairs pairs of length len, pair k from seed seed_base + k, laid out
// [a_0 | b_0 | a_1 | b_1 | ...] in `arena` (2*len*npairs bytes).
void sw_gen_batch(uint64_t seed_base, int npairs, int len, unsigned char* arena) {
    for (int k = 0; k < npairs; ++k)
        sw_gen_pair(seed_base + (uint64_t)k, len, arena + (size_t)2 * len * k, arena + (size_t)2 * len * k + len);
}
}
