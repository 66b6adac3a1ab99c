// Sanitizer driver for the host arithmetic of long pairs in a mode (test infrastructure; built by
// `make -C concurrentproject_amd/csrc asan-align-long-mode` with -fsanitize=address,undefined together
// with sw_align_host.cpp and sw_matrix_host.cpp, the product's own host code, and run by
// tests/test_align_long_modes_cpu.py).  No device code, nothing preloaded.
//
//   align_long_mode_asan   the end record of a global or semi-global pair from the records of the cooperative
//                          locate pass (align_mode_end: the last strip's, whatever the others hold); the end
//                          cell a walk may start from (align_long_end_ok) against a restatement, every mode;
//                          the answers for pairs with an empty sequence (align_mode_empty through an AlignSink:
//                          score, ranges, operations) against the formulas of include/algoGPU.h; the refusals
//                          of the _long_mode entry points (align_long_mode_check: an unknown mode, a pair over
//                          the range bound named by its index or by its record) and that local mode and pairs
//                          under the bound pass.
//                          Prints "ok <ends> <cells> <empties> <refusals>".
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
    std::fprintf(stderr, "align_long_mode_driver: %s (%lld, %lld) %s\n", what, a, b, g_err.c_str());
    return 3;
}
}  // namespace

namespace swmi {
// the product defines this in sw_engine.hip (device code); the driver keeps the text itself
void report_error(const char* msg) { g_err = msg ? msg : ""; }
}  // namespace swmi

int main() {
    using namespace swmi;
    long long ends = 0, cells = 0, empties = 0, refusals = 0;
    std::mt19937_64 rng(19);
    {   // the end record: the last strip's
        int sc = -1, ei = -1, ej = -1;
        align_mode_end(nullptr, 0, &sc, &ei, &ej);
        if (sc != 0 || ei != 0 || ej != 0) return fail("no record");
        ++ends;
        for (int r = 0; r < 4000; ++r) {
            const int n = 1 + (int)(rng() % 40);
            std::vector<AlignEnd> rec((size_t)n);
            for (auto& x : rec) x = AlignEnd{(int)(rng() % 2001) - 1000, (int)(rng() % 100000), (int)(rng() % 100000), 0};
            rec.shrink_to_fit();   // a read past the last record is a finding
            align_mode_end(rec.data(), n, &sc, &ei, &ej);
            const AlignEnd& last = rec[(size_t)n - 1];
            if (sc != last.t || ei != last.d || ej != last.j) return fail("the last strip's record", r, n);
            ++ends;
        }
        const AlignEnd neg[3] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {-522, 1099, 214, 0}};   // a negative score is a score
        align_mode_end(neg, 3, &sc, &ei, &ej);
        if (sc != -522 || ei != 1099 || ej != 214) return fail("a negative score");
        ++ends;
    }
    {   // the end cell a walk may start from
        for (int r = 0; r < 20000; ++r) {
            const int n = 1 + (int)(rng() % 6), m = 1 + (int)(rng() % 6);
            const int ei = (int)(rng() % 9) - 1, ej = (int)(rng() % 9) - 1;
            for (int mode = 0; mode < 3; ++mode) {
                bool want = ei >= 0 && ei < n && ej >= 0 && ej < m;
                if (mode != SW_MODE_LOCAL) want = want && ei == n - 1;
                if (mode == SW_MODE_GLOBAL) want = want && ej == m - 1;
                if (align_long_end_ok(n, m, mode, ei, ej) != want) return fail("end cell", r, mode);
                ++cells;
            }
        }
        const int big = (1 << 27) - 1;
        if (!align_long_end_ok(big, big, SW_MODE_GLOBAL, big - 1, big - 1) || align_long_end_ok(big, big, SW_MODE_GLOBAL, big - 1, 0) ||
            !align_long_end_ok(big, big, SW_MODE_SEMIGLOBAL, big - 1, 0) || align_long_end_ok(big, big, SW_MODE_SEMIGLOBAL, 0, 0))
            return fail("end cell of the longest pair");
        cells += 4;
    }
    {   // empty sequences: include/algoGPU.h EMPTY SEQUENCES
        const int gaps[][2] = {{12, 1}, {5, 0}, {0, 0}, {1, 3}, {1 << 17, 1}};
        for (const auto& g : gaps)
            for (const int L : {0, 1, 2, 40, 1700})
                for (int mode = 1; mode < 3; ++mode)
                    for (int side = 0; side < 2; ++side) {
                        const int alen = side ? L : 0, blen = side ? 0 : L;
                        std::vector<sw_alignment> out(3);
                        AlignSink sink{out.data(), {}};
                        sink.set_empty(0);
                        align_mode_empty(sink, 1, alen, blen, g[0], g[1], mode);
                        sink.set_empty(2);
                        std::vector<unsigned> cig(4);
                        long long used = -1;
                        if (sink.finish(cig.data(), (long long)cig.size(), &used)) return fail("finish", L, mode);
                        const bool run = L > 0 && (mode == SW_MODE_GLOBAL || side == 1);
                        const int score = run ? -(g[0] + (L - 1) * std::min(g[0], g[1])) : 0;
                        const sw_alignment& x = out[1];
                        if (x.score != score || x.score != mode_empty_score(alen, blen, g[0], g[1], mode)) return fail("score", L, mode);
                        if (x.beg1 != 0 || x.beg2 != 0 || x.end1 != (run ? alen : 0) || x.end2 != (run ? blen : 0))
                            return fail("ranges", L, mode);
                        if (x.ncigar != (run ? 1 : 0) || used != x.ncigar) return fail("operations", L, mode);
                        if (run && cig[(size_t)x.cigar_off] != (((unsigned)L << 4) | (side ? 1u : 2u))) return fail("the run", L, mode);
                        ++empties;
                    }
    }
    {   // the refusals of the _long_mode entry points
        const int alen[3] = {40, 1 << 22, 0}, blen[3] = {40, 4, 700}, rec[3] = {7, 11, 13};
        for (const int bad : {-1, 3, 4, 1 << 30}) {
            g_err.clear();
            if (align_long_mode_check("sw_align_matrix_long_mode", bad, alen, blen, nullptr, 3, 12, 1, "pair") != -1 ||
                g_err.find("sw_align_matrix_long_mode: unknown alignment mode") != 0)
                return fail("unknown mode", bad);
            ++refusals;
        }
        g_err.clear();
        if (align_long_mode_check("f", SW_MODE_LOCAL, alen, blen, nullptr, 3, 12, 1, "pair") != 0 || !g_err.empty())
            return fail("local is not checked against the mode bound");
        for (int mode = 1; mode < 3; ++mode) {
            g_err.clear();
            if (align_long_mode_check("f", mode, alen, blen, nullptr, 3, 12, 1, "pair") != -1 ||
                g_err.find("pair 1: score range exceeds the int32 engine in this mode") != 0)
                return fail("range refusal by index", mode);
            if (align_long_mode_check("f", mode, alen, blen, rec, 3, 12, 1, "record") != -1 ||
                g_err.find("record 11: score range exceeds the int32 engine in this mode") != 0)
                return fail("range refusal by record", mode);
            g_err.clear();
            if (align_long_mode_check("f", mode, alen, blen, nullptr, 1, 12, 1, "pair") != 0 || !g_err.empty())
                return fail("a pair under the bound", mode);
            if (align_long_mode_check("f", mode, alen, blen, nullptr, 1, 1 << 20, 1, "pair") != -1 || g_err.find("pair 0:") != 0)
                return fail("the gap penalty in the bound", mode);
            if (align_long_mode_check("f", mode, nullptr, nullptr, nullptr, 0, 12, 1, "pair") != 0) return fail("no pairs", mode);
            refusals += 5;
        }
        // the bound itself: (n + m + 1024) * max(G_INIT, G_EXT, 127) < 2^28
        for (int r = 0; r < 20000; ++r) {
            const int n = (int)(rng() % (1u << 22)), m = (int)(rng() % (1u << 22));
            const int go = (int)(rng() % 300), ge = (int)(rng() % 300);
            const bool want = ((long long)n + m + 1024) * std::max(std::max(go, ge), 127) < (1LL << 28);
            if ((align_long_mode_check("f", 1 + r % 2, &n, &m, nullptr, 1, go, ge, "pair") == 0) != want) return fail("bound", n, m);
            ++refusals;
        }
    }
    std::printf("ok %lld %lld %lld %lld\n", ends, cells, empties, refusals);
    return 0;
}
