// Sanitizer driver for the host arithmetic of long pairs on many waves (test infrastructure; built by
// `make -C concurrentproject_amd/csrc asan-align-long-coop` with -fsanitize=address,undefined together
// with sw_align_host.cpp and sw_matrix_host.cpp, the product's own host code, and run by
// tests/test_align_long_coop_cpu.py).  No device code, nothing preloaded.
//
//   align_long_coop_asan   the planner (align_long_coop_plan) over a grid of lengths against the formulas
//                          restated here, both refusals, n or m = 0 and the longest sequence (2^27 - 1: no
//                          overflow); the window rule (align_window), automatic and forced, against a plain
//                          restatement and its three promises (1 <= g <= min(64, strip + 1), the pair's
//                          window within the budget, a round's automatic windows within the budget); the
//                          host merge of end-cell records (align_merge_ends) against a brute-force search
//                          of the same records in every order.
//                          Prints "ok <plans> <windows> <merges>".
// Exit 0, or 3 with a line on stderr at the first disagreement.  Sanitizer findings abort.
#include <algorithm>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "sw_matrix_host.h"
#include "../../include/algoGPU.h"

namespace {
thread_local std::string g_err;

int fail(const char* what, long long a = 0, long long b = 0) {
    std::fprintf(stderr, "align_long_coop_driver: %s (%lld, %lld) %s\n", what, a, b, g_err.c_str());
    return 3;
}

// the window rule restated (include/algoGPU.h)
long long window_plain(long long strip_bytes, long long live_bytes, long long budget, int long_window, int strip) {
    long long g = long_window == 0 ? budget / live_bytes : std::min<long long>(long_window, budget / strip_bytes);
    if (g > 64) g = 64;
    if (g > strip + 1) g = strip + 1;
    return g < 1 ? 1 : g;
}
}  // namespace

namespace swmi {
// the product defines this in sw_engine.hip (device code); the driver keeps the text itself
void report_error(const char* msg) { g_err = msg ? msg : ""; }
}  // namespace swmi

int main() {
    using namespace swmi;
    const long long MiB = 1LL << 20;
    long long plans = 0, windows = 0, merges = 0;
    const int ns[] = {0, 1, 511, 512, 513, 1024, 1025, 1100, 1537, 2600, 65536, 131072, (1 << 27) - 1};
    const int ms[] = {0, 1, 63, 64, 65, 300, 576, 700, 5000, 65536, (1 << 27) - 1};
    for (const int n : ns)
        for (const int m : ms)
            for (const int lw : {0, 1, 3, 64}) {
                sw_align_coop_plan p{-1, -1, -1, -1, -1, -1};
                sw_align_plan q{-1, -1, -1, -1};
                g_err.clear();
                const long long budget = 3072 * MiB;
                const int rc = align_long_coop_plan(n, m, budget, 1LL << 50, lw, "pair", 7, &p);
                const std::string err = g_err;
                const int rq = align_long_plan(n, m, budget, 1LL << 50, "pair", 7, &q);
                if (rc != rq || err != g_err) return fail("refuses as align_long_plan", n, m);
                const long long strips = n && m ? (n + 511LL) / 512 : 0;
                const long long strip_b = n && m ? (m + 511LL + 63) / 64 * 64 * 256 : 0;
                const long long ckpt = n && m ? (strips - 1) * ((m + 63LL) / 64 * 64 * 8) : 0;
                const long long win = strips ? window_plain(strip_b, strip_b, budget, lw, (int)strips - 1) : 0;
                if (p.strips != strips || p.ckpt_bytes != ckpt || p.progress_bytes != (strips * 4 + 15) / 16 * 16 ||
                    p.end_bytes != strips * 16 || p.window != win || p.window_trace_bytes != win * strip_b)
                    return fail("plan", n, m);
                if (p.progress_bytes % 16 || p.window_trace_bytes < 0 || (rc == 0 && p.window_trace_bytes > budget))
                    return fail("plan bounds", n, m);
                ++plans;
            }
    {   // pinned values and the two refusals at a budget of 1 MiB each
        sw_align_coop_plan p;
        if (align_long_coop_plan(2600, 300, MiB, MiB, 0, "pair", 0, &p) || p.strips != 6 || p.ckpt_bytes != 5 * 320 * 8 ||
            p.progress_bytes != 32 || p.end_bytes != 96 || p.window != 4 || p.window_trace_bytes != 4 * 212992)
            return fail("2600 x 300");
        if (align_long_coop_plan(1537, 700, MiB, MiB, 0, "pair", 0, &p) || p.strips != 4 || p.window != 3 ||
            p.window_trace_bytes != 3 * 311296)
            return fail("1537 x 700");
        if (align_long_coop_plan(1537, 700, MiB, MiB, 2, "pair", 0, &p) || p.window != 2) return fail("1537 x 700 forced 2");
        if (align_long_coop_plan(1537, 700, MiB, MiB, 64, "pair", 0, &p) || p.window != 3) return fail("1537 x 700 forced 64");
        if (align_long_coop_plan(600, 5000, MiB, MiB, 0, "pair", 3, &p) != -1 ||
            g_err.find("pair 3: a 600 x 5000 alignment needs 1425408 bytes of trace memory for one strip") != 0 ||
            g_err.find("trace_mb = 1 MiB") == std::string::npos)
            return fail("strip refusal");
        if (align_long_coop_plan(131072, 576, MiB, MiB, 0, "record", 9, &p) != -1 || p.ckpt_bytes != 255LL * 576 * 8 ||
            g_err.find("record 9: a 131072 x 576 alignment needs 1175040 bytes of checkpoints") != 0 ||
            g_err.find("SWMI_ALIGN_CKPT_MB = 1 MiB") == std::string::npos)
            return fail("checkpoint refusal");
        if (align_long_coop_plan((1 << 27) - 1, (1 << 27) - 1, 3072 * MiB, 4096 * MiB, 0, "pair", 0, &p) != -1 ||
            p.strips != 262144 || p.ckpt_bytes != 262143LL * (1LL << 30) || p.end_bytes != 262144LL * 16)
            return fail("the longest pair");
        plans += 7;
    }
    {   // the window rule
        std::mt19937_64 rng(17);
        for (int r = 0; r < 20000; ++r) {
            const long long budget = (1 + (long long)(rng() % 3072)) * MiB;
            const int live = 1 + (int)(rng() % 12);
            std::vector<long long> one((size_t)live);
            long long sum = 0;
            for (auto& x : one) {
                x = (1 + (long long)(rng() % (unsigned long long)(budget / 256 / 64))) * 64 * 256;   // each fits alone
                sum += x;
            }
            const int lw = r % 3 == 0 ? 0 : (int)(rng() % 65);
            long long round_bytes = 0;
            for (int k = 0; k < live; ++k) {
                const int strip = (int)(rng() % 300);
                const int g = align_window(one[(size_t)k], sum, budget, lw, strip);
                if (g != window_plain(one[(size_t)k], sum, budget, lw, strip)) return fail("window against the restatement", r, g);
                if (g < 1 || g > 64 || g > strip + 1) return fail("window out of range", r, g);
                if (g * one[(size_t)k] > budget) return fail("a window over the budget", r, g);
                if (lw == 1 && g != 1) return fail("long_window = 1", r, g);
                round_bytes += g * one[(size_t)k];
                ++windows;
            }
            if (lw == 0 && sum <= budget && round_bytes > budget) return fail("an automatic round over the budget", r, round_bytes);
        }
        if (align_window(311296, 6 * 311296, MiB, 0, 3) != 1 || align_window(311296, 311296, MiB, 0, 3) != 3 ||
            align_window(311296, 311296, MiB, 0, 1) != 2 || align_window(311296, 6 * 311296, MiB, 3, 3) != 3 ||
            align_window(212992, 212992, 1024 * MiB, 0, 100) != 64 || align_window(212992, 212992, 1024 * MiB, 0, 0) != 1)
            return fail("window pinned");
        windows += 6;
    }
    {   // the merge: the largest t, then the smallest i + j, then the smallest j; t <= 0 is no cell
        int sc = -1, ei = -1, ej = -1;
        align_merge_ends(nullptr, 0, &sc, &ei, &ej);
        if (sc != 0 || ei != 0 || ej != 0) return fail("merge nothing");
        const AlignEnd none[2] = {{0, 512, -8, 0}, {0, 1024, -504, 0}};
        align_merge_ends(none, 2, &sc, &ei, &ej);
        if (sc != 0 || ei != 0 || ej != 0) return fail("merge of empty strips");
        const AlignEnd tie[3] = {{70, 600, 69, 0}, {70, 138, 69, 0}, {70, 138, 70, 0}};   // A x 1100 against A x 70: (69, 69)
        align_merge_ends(tie, 3, &sc, &ei, &ej);
        if (sc != 70 || ei != 69 || ej != 69) return fail("merge ties", ei, ej);
        merges += 3;
        std::mt19937_64 rng(18);
        for (int r = 0; r < 4000; ++r) {
            const int n = 1 + (int)(rng() % 9);
            std::vector<AlignEnd> rec((size_t)n);
            for (auto& x : rec) {
                x.t = (int)(rng() % 4);   // many ties, some empty
                x.j = (int)(rng() % 6);
                x.d = x.j + (int)(rng() % 6);
                x.pad = 0;
            }
            int bt = 0, bd = 0, bj = 0;   // brute force: the lexicographic best of (-t, d, j) among t > 0
            for (const auto& x : rec)
                if (x.t > 0 && (bt == 0 || x.t > bt || (x.t == bt && (x.d < bd || (x.d == bd && x.j < bj))))) {
                    bt = x.t;
                    bd = x.d;
                    bj = x.j;
                }
            for (int order = 0; order < 3; ++order) {   // the result does not depend on the order of the records
                align_merge_ends(rec.data(), n, &sc, &ei, &ej);
                if (sc != bt || ei != (bt ? bd - bj : 0) || ej != (bt ? bj : 0)) return fail("merge against brute force", r, order);
                std::shuffle(rec.begin(), rec.end(), rng);
                ++merges;
            }
        }
    }
    std::printf("ok %lld %lld %lld\n", plans, windows, merges);
    return 0;
}
