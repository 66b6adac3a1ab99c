// Sanitizer driver for the banded CPU aligner and the band's arithmetic (test infrastructure; built by
// `make -C concurrentproject_amd/csrc asan-align-band` with -fsanitize=address,undefined together
// with sw_align_host.cpp and sw_matrix_host.cpp, the product's own host code, and run by
// tests/test_band_cpu.py).  No device code, nothing preloaded.
//
//   align_band_asan SEED NPAIRS   NPAIRS random small pairs over 6 symbols (lengths 1..40, every
//                                 eighth pair with n = 1 or m = 1, every third a mutated copy, every
//                                 16th with seq1 empty, every 16th with seq2 empty) through
//                                 sw_align_matrix_cpu_band in batches of 16, in all three modes,
//                                 with bands 0, 1, 3, 7 and 64, under gaps (3, 1), (0, 0) and (1, 3),
//                                 with a cigar buffer of exact size; every alignment is re-scored
//                                 here from its operations, every aligned column must lie in the
//                                 band, and global / semi-global ones must consume both sequences /
//                                 all of seq1.  sw_band_plan of every pair against a count of the
//                                 cells done here.  Then a negative band and an unknown mode, which
//                                 must be refused by name.
//                                 Prints "ok <pairs aligned> <sum of scores> <cigar entries>".
// Exit 0, or 3 with a line on stderr at the first disagreement.  Sanitizer findings abort.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "sw_matrix_host.h"
#include "../../include/algoGPU.h"

namespace {
thread_local std::string g_err;

int fail(const char* what, long long a = 0, long long b = 0) {
    std::fprintf(stderr, "align_band_driver: %s (%lld, %lld) %s\n", what, a, b, g_err.c_str());
    return 3;
}
}  // namespace

namespace swmi {
// the product defines this in sw_engine.hip (device code); the driver keeps the text itself
void report_error(const char* msg) { g_err = msg ? msg : ""; }
}  // namespace swmi

int main(int argc, char** argv) {
    if (argc != 3) return fail("usage: align_band_asan SEED NPAIRS");
    std::mt19937_64 rng((unsigned long long)std::atoll(argv[1]));
    const int npairs = std::atoi(argv[2]);
    const int K = 6;
    const unsigned char sym[K] = {'A', 'C', 'G', 'T', 'N', 'x'};
    signed char tab[K * K];
    for (int i = 0; i < K; ++i)
        for (int j = 0; j < K; ++j) tab[i * K + j] = (signed char)(i == j ? 3 + (int)(rng() % 5) : -4 + (int)(rng() % 6));
    sw_matrix* mx = sw_matrix_create(sym, K, tab, -1, 0);
    if (!mx) return fail("sw_matrix_create");
    const int gaps[3][2] = {{3, 1}, {0, 0}, {1, 3}};
    const int modes[3] = {SW_MODE_LOCAL, SW_MODE_GLOBAL, SW_MODE_SEMIGLOBAL};
    const int bands[5] = {0, 1, 3, 7, 64};
    long long aligned = 0, score_sum = 0, entries = 0;
    for (int base = 0; base < npairs; base += 16) {
        const int nb = std::min(16, npairs - base);
        std::vector<std::vector<unsigned char>> A((size_t)nb), B((size_t)nb);
        for (int k = 0; k < nb; ++k) {
            int n = 1 + (int)(rng() % 40), m = 1 + (int)(rng() % 40);
            if ((base + k) % 8 == 3) n = 1;
            if ((base + k) % 8 == 7) m = 1;
            for (int i = 0; i < n; ++i) A[(size_t)k].push_back(sym[rng() % K]);
            if ((base + k) % 3 == 0 && n > 4) {   // a copy with one residue dropped and one changed
                B[(size_t)k] = A[(size_t)k];
                B[(size_t)k].erase(B[(size_t)k].begin() + (long)(rng() % (unsigned)n));
                B[(size_t)k][rng() % B[(size_t)k].size()] = sym[rng() % K];
            } else {
                for (int j = 0; j < m; ++j) B[(size_t)k].push_back(sym[rng() % K]);
            }
            if ((base + k) % 16 == 9) A[(size_t)k].clear();
            if ((base + k) % 16 == 14) B[(size_t)k].clear();
        }
        std::vector<const unsigned char*> ap, bp;
        std::vector<int> al, bl;
        for (int k = 0; k < nb; ++k) {
            ap.push_back(A[(size_t)k].empty() ? nullptr : A[(size_t)k].data());
            bp.push_back(B[(size_t)k].empty() ? nullptr : B[(size_t)k].data());
            al.push_back((int)A[(size_t)k].size());
            bl.push_back((int)B[(size_t)k].size());
        }
        for (const int band : bands) {
            for (int k = 0; k < nb; ++k) {   // the plan against a count done here
                const long long n = al[(size_t)k], m = bl[(size_t)k];
                sw_band_plan_t p;
                if (sw_band_plan((int)n, (int)m, band, &p) != 0) return fail("sw_band_plan", base + k, band);
                if (p.dlo != std::min(0LL, m - n) - band || p.dhi != std::max(0LL, m - n) + band) return fail("plan range", base + k, band);
                long long cells = 0;
                for (long long i = 0; i < n; ++i)
                    for (long long j = 0; j < m; ++j) cells += j - i >= p.dlo && j - i <= p.dhi;
                if (cells != p.cells) return fail("plan cells", cells, p.cells);
                if ((n > 0 && m > 0) != (p.trace_bytes > 0) || (n > 0 && m > 0) != (p.full_trace_bytes > 0))
                    return fail("plan bytes", base + k, band);
            }
            for (const int mode : modes)
                for (const auto& g : gaps) {
                    std::vector<sw_alignment> out((size_t)nb);
                    long long used = -1;
                    int rc = sw_align_matrix_cpu_band(mx, ap.data(), al.data(), bp.data(), bl.data(), nb, g[0], g[1], mode, band,
                                                      out.data(), nullptr, 0, &used);
                    if (used < 0 || (rc == 0) != (used == 0)) return fail("need without a buffer", rc, used);
                    const long long need = used;
                    std::vector<unsigned> cig((size_t)need);   // exactly what is passed: a write past it is a finding
                    rc = sw_align_matrix_cpu_band(mx, ap.data(), al.data(), bp.data(), bl.data(), nb, g[0], g[1], mode, band,
                                                  out.data(), need ? cig.data() : nullptr, need, &used);
                    if (rc != 0 || used != need) return fail("exact buffer", rc, used);
                    for (int k = 0; k < nb; ++k) {
                        const sw_alignment& o = out[(size_t)k];
                        const int n = al[(size_t)k], m = bl[(size_t)k];
                        const long long dlo = std::min(0, m - n) - band, dhi = std::max(0, m - n) + band;
                        if (o.cigar_off < 0 || o.cigar_off + o.ncigar > need) return fail("cigar range", base + k);
                        long long i = o.beg1, j = o.beg2, sc = 0;
                        for (int e = 0; e < o.ncigar; ++e) {
                            const unsigned ent = cig[(size_t)(o.cigar_off + e)];
                            const long long len = ent >> 4;
                            const unsigned op = ent & 15u;
                            if (len <= 0 || op > 2) return fail("cigar entry", base + k, ent);
                            if (op == 0)
                                for (long long t = 0; t < len; ++t, ++i, ++j) {
                                    if (i >= n || j >= m) return fail("M outside the pair", base + k);
                                    if (j - i < dlo || j - i > dhi) return fail("M outside the band", base + k, band);
                                    int v = 0;
                                    sw_matrix_score(mx, A[(size_t)k][(size_t)i], B[(size_t)k][(size_t)j], &v);
                                    sc += v;
                                }
                            else {
                                sc -= g[0] + (len - 1) * std::min(g[0], g[1]);
                                (op == 1 ? i : j) += len;
                            }
                        }
                        if (i != o.end1 || j != o.end2 || sc != o.score || i > n || j > m) return fail("re-score", base + k, sc);
                        if (mode == SW_MODE_GLOBAL && (o.beg1 != 0 || o.end1 != n || o.beg2 != 0 || o.end2 != m))
                            return fail("global does not cover both sequences", base + k, mode);
                        if (mode == SW_MODE_SEMIGLOBAL && (o.beg1 != 0 || o.end1 != n)) return fail("semi-global does not cover seq1", base + k);
                        ++aligned;
                        score_sum += o.score;
                        entries += o.ncigar;
                    }
                }
        }
    }
    // refusals by name: a negative band, an unknown mode
    {
        const unsigned char one = 'A';
        const unsigned char* p = &one;
        const int l1 = 1;
        sw_alignment o;
        long long used = 0;
        unsigned cig[4];
        sw_band_plan_t pl;
        if (sw_align_matrix_cpu_band(mx, &p, &l1, &p, &l1, 1, 3, 1, SW_MODE_GLOBAL, -1, &o, cig, 4, &used) != -1 ||
            g_err.find("sw_align_matrix_cpu_band: band -1") == std::string::npos)
            return fail("negative band accepted");
        if (sw_align_matrix_cpu_band(mx, &p, &l1, &p, &l1, 1, 3, 1, 3, 5, &o, cig, 4, &used) != -1 ||
            g_err.find("sw_align_matrix_cpu_band: unknown alignment mode 3") == std::string::npos)
            return fail("unknown mode accepted");
        if (sw_band_plan(10, 10, -2, &pl) != -1 || g_err.find("sw_band_plan: band -2") == std::string::npos)
            return fail("negative band planned");
    }
    sw_matrix_free(mx);
    std::printf("ok %lld %lld %lld\n", aligned, score_sum, entries);
    return 0;
}
