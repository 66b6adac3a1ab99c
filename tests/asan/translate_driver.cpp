// Sanitizer driver for the host side of translated search (test infrastructure; built by
// `make -C concurrentproject_amd/csrc asan-translate` with -fsanitize=address,undefined together with
// sw_align_host.cpp and sw_matrix_host.cpp, the product's own host code, and run by
// tests/test_translate_cpu.py).  No device code, nothing preloaded.
//
//   translate_asan SEED   For DNA lengths 0..8, 189..197, 391 and 905 (random bases, about 3 % N, lower case
//                         and U), all six frames: sw_translate into a buffer of exactly the residue count
//                         (a write past it is a finding), checked against a restatement written here;
//                         sw_translated_range of random residue ranges, whose bases translated on their own
//                         must give those residues; the composed tables against sw_matrix_score; and
//                         sw_align_matrix_translated_cpu in the three modes with a cigar buffer of exact size,
//                         every alignment re-scored over the translated frame.  Then every refusal: frames 0
//                         and 4, null pointers, a buffer too small, a length over 2^27 - 1, a matrix without
//                         '*' and one without 'X', a query byte outside the matrix, an unknown mode.
//                         Prints "ok <translations> <ranges> <alignments> <sum of scores>".
// Exit 0, or 3 with a line on stderr at the first disagreement.  Sanitizer findings abort.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "sw_matrix_host.h"
#include "../../include/algoGPU.h"

namespace {
thread_local std::string g_err;

int fail(const char* what, long long a = 0, long long b = 0) {
    std::fprintf(stderr, "translate_driver: %s (%lld, %lld) %s\n", what, a, b, g_err.c_str());
    return 3;
}

const char CODE[65] = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG";

int cls(unsigned char b) {
    const char* p = std::strchr("TCAG", b >= 'a' && b <= 'z' ? b - 32 : b);
    if (b == 'U' || b == 'u') return 0;
    return b && p ? (int)(p - "TCAG") : 4;
}

// the rules restated: the reverse complement as a sequence of classes, then codon by codon
std::vector<unsigned char> restate(const std::vector<unsigned char>& dna, int frame) {
    std::vector<int> c;
    for (unsigned char b : dna) c.push_back(cls(b));
    if (frame < 0) {
        std::reverse(c.begin(), c.end());
        for (int& x : c) x = x < 4 ? x ^ 2 : 4;
    }
    std::vector<unsigned char> out;
    for (size_t i = (size_t)std::abs(frame) - 1; i + 3 <= c.size(); i += 3)
        out.push_back(c[i] > 3 || c[i + 1] > 3 || c[i + 2] > 3 ? 'X' : (unsigned char)CODE[16 * c[i] + 4 * c[i + 1] + c[i + 2]]);
    return out;
}
}  // namespace

namespace swmi {
// the product defines this in sw_engine.hip (device code); the driver keeps the text itself
void report_error(const char* msg) { g_err = msg ? msg : ""; }
}  // namespace swmi

int main(int argc, char** argv) {
    if (argc != 2) return fail("usage: translate_asan SEED");
    std::mt19937_64 rng((unsigned long long)std::atoll(argv[1]));
    const int frames[6] = {1, 2, 3, -1, -2, -3};
    const unsigned char sym[] = "ARNDCQEGHILKMFPSTWYVBZX*";
    const int K = 24;
    std::vector<signed char> tab((size_t)K * K);
    for (int i = 0; i < K; ++i)
        for (int j = 0; j < K; ++j) tab[(size_t)(i * K + j)] = (signed char)(i == j ? 4 + (int)(rng() % 8) : -4 + (int)(rng() % 8));
    sw_matrix* mx = sw_matrix_create(sym, K, tab.data(), -1, 0);
    if (!mx) return fail("sw_matrix_create");

    unsigned char std_code[64];
    sw_standard_code(std_code);
    if (std::memcmp(std_code, CODE, 64) != 0) return fail("sw_standard_code");

    // the composed tables
    unsigned char base[256], codon[65];
    if (sw_translated_tables(mx, nullptr, base, codon) != 0) return fail("sw_translated_tables");
    for (int b = 0; b < 256; ++b)
        if (base[b] != cls((unsigned char)b)) return fail("base class", b, base[b]);
    for (int c = 0; c <= 64; ++c) {
        const unsigned char aa = c < 64 ? (unsigned char)CODE[c] : 'X';
        if (codon[c] >= K || sym[codon[c]] != aa) return fail("codon table", c, codon[c]);
    }

    std::vector<int> lens;
    for (int L = 0; L <= 8; ++L) lens.push_back(L);
    for (int L = 189; L <= 197; ++L) lens.push_back(L);
    lens.push_back(391);
    lens.push_back(905);
    const int modes[3] = {SW_MODE_LOCAL, SW_MODE_GLOBAL, SW_MODE_SEMIGLOBAL};
    long long translations = 0, ranges = 0, aligned = 0, score_sum = 0;
    for (const int L : lens) {
        std::vector<unsigned char> dna((size_t)L);
        for (auto& b : dna) {
            b = (unsigned char)"ACGT"[rng() % 4];
            const unsigned r = (unsigned)(rng() % 100);
            if (r == 0) b = 'N';
            else if (r == 1) b = (unsigned char)(b | 0x20);
            else if (r == 2 && b == 'T') b = 'U';
        }
        const unsigned char* dp = L ? dna.data() : nullptr;
        for (const int f : frames) {
            const std::vector<unsigned char> want = restate(dna, f);
            std::vector<unsigned char> got(want.size());   // exactly the residues
            const int m = sw_translate(dp, L, f, nullptr, got.empty() ? nullptr : got.data(), (int)got.size());
            if (m != (int)want.size() || got != want) return fail("sw_translate", L, f);
            ++translations;
            for (int t = 0; t < 4; ++t) {
                const int beg2 = (int)(rng() % (unsigned)(m + 1)), end2 = beg2 + (int)(rng() % (unsigned)(m - beg2 + 1));
                int lo = -1, hi = -1;
                if (sw_translated_range(L, f, beg2, end2, &lo, &hi) != 0) return fail("sw_translated_range", L, f);
                if (lo < 0 || hi > L || hi - lo != 3 * (end2 - beg2)) return fail("range bounds", lo, hi);
                const std::vector<unsigned char> piece(dna.begin() + lo, dna.begin() + hi);
                const std::vector<unsigned char> sub = restate(piece, f < 0 ? -1 : 1);
                if (sub != std::vector<unsigned char>(want.begin() + beg2, want.begin() + end2)) return fail("range residues", L, f);
                ++ranges;
            }
            // the CPU aligner: a query cut out of the frame (or random when the frame is empty), every mode
            std::vector<unsigned char> q;
            if (m >= 4) q.assign(want.begin() + m / 4, want.begin() + std::min(m, m / 4 + 40));
            else for (int i = 0; i < 5; ++i) q.push_back(sym[rng() % 20]);
            if (L == 7) q.clear();   // an empty query once
            const unsigned char* qp = q.empty() ? nullptr : q.data();
            const int ql = (int)q.size();
            for (const int mode : modes) {
                sw_alignment o;
                long long used = -1;
                int rc = sw_align_matrix_translated_cpu(mx, &qp, &ql, &dp, &L, &f, 1, 12, 1, mode, nullptr, &o, nullptr, 0, &used);
                if (used < 0 || (rc == 0) != (used == 0)) return fail("need without a buffer", rc, used);
                std::vector<unsigned> cig((size_t)used);
                const long long need = used;
                rc = sw_align_matrix_translated_cpu(mx, &qp, &ql, &dp, &L, &f, 1, 12, 1, mode, nullptr, &o, need ? cig.data() : nullptr,
                                                    need, &used);
                if (rc != 0 || used != need) return fail("exact buffer", rc, used);
                long long i = o.beg1, j = o.beg2, sc = 0;
                for (int e = 0; e < o.ncigar; ++e) {
                    const unsigned ent = cig[(size_t)(o.cigar_off + e)];
                    const long long len = ent >> 4;
                    const unsigned op = ent & 15u;
                    if (len <= 0 || op > 2) return fail("cigar entry", L, ent);
                    if (op == 0)
                        for (long long t = 0; t < len; ++t, ++i, ++j) {
                            if (i >= ql || j >= m) return fail("M outside the pair", L, f);
                            int v = 0;
                            sw_matrix_score(mx, q[(size_t)i], want[(size_t)j], &v);
                            sc += v;
                        }
                    else {
                        sc -= 12 + (len - 1);
                        (op == 1 ? i : j) += len;
                    }
                }
                if (i != o.end1 || j != o.end2 || sc != o.score) return fail("re-score", L, f);
                if (mode != SW_MODE_LOCAL && (o.beg1 != 0 || o.end1 != ql)) return fail("the query is not covered", L, f);
                if (mode == SW_MODE_LOCAL && m >= 4 && ql > 0 && o.score <= 0) return fail("a planted query scores nothing", L, f);
                ++aligned;
                score_sum += o.score;
            }
        }
    }

    // refusals
    {
        const unsigned char dna[] = "GCTCGTAACGAT", q[] = "ARND", bad_q[] = "AoND";
        const unsigned char *dp = dna, *qp = q, *bp = bad_q, *null = nullptr;
        const int dl = 12, ql = 4, big = 1 << 27;
        int f1 = 1, lo, hi;
        unsigned char out[8];
        sw_alignment o;
        long long used = 0;
        unsigned cig[8];
        for (const int f : {0, 4, -4}) {
            if (sw_translate(dna, dl, f, nullptr, out, 8) != -1 || g_err.find("sw_translate: frame") == std::string::npos)
                return fail("sw_translate took a bad frame", f);
            if (sw_translated_range(dl, f, 0, 1, &lo, &hi) != -1 || g_err.find("sw_translated_range: frame") == std::string::npos)
                return fail("sw_translated_range took a bad frame", f);
            if (sw_align_matrix_translated_cpu(mx, &qp, &ql, &dp, &dl, &f, 1, 12, 1, 0, nullptr, &o, cig, 8, &used) != -1 ||
                g_err.find("sw_align_matrix_translated_cpu: pair 0: frame") == std::string::npos)
                return fail("the aligner took a bad frame", f);
        }
        if (sw_translate(nullptr, dl, 1, nullptr, out, 8) != -1) return fail("sw_translate took a null DNA");
        if (sw_translate(dna, dl, 1, nullptr, out, 3) != -1 || g_err.find("do not fit") == std::string::npos)
            return fail("sw_translate took a small buffer");
        if (sw_translate(dna, dl, 1, nullptr, nullptr, 0) != -1) return fail("sw_translate took a null buffer");
        if (sw_translated_range(dl, 1, 0, 5, &lo, &hi) != -1 || sw_translated_range(dl, 1, 3, 2, &lo, &hi) != -1 ||
            sw_translated_range(dl, 1, 0, 1, nullptr, &hi) != -1)
            return fail("sw_translated_range took a bad range");
        if (sw_align_matrix_translated_cpu(mx, &qp, &ql, &dp, &big, &f1, 1, 12, 1, 0, nullptr, &o, cig, 8, &used) != -1 ||
            g_err.find("is outside [0, 2^27 - 1]") == std::string::npos)
            return fail("an oversized length was accepted");
        if (sw_align_matrix_translated_cpu(mx, &qp, &ql, &null, &dl, &f1, 1, 12, 1, 0, nullptr, &o, cig, 8, &used) != -1 ||
            g_err.find("a null sequence pointer") == std::string::npos)
            return fail("a null DNA was accepted");
        if (sw_align_matrix_translated_cpu(mx, &qp, &ql, &dp, &dl, nullptr, 1, 12, 1, 0, nullptr, &o, cig, 8, &used) != -1)
            return fail("null frames were accepted");
        if (sw_align_matrix_translated_cpu(mx, &bp, &ql, &dp, &dl, &f1, 1, 12, 1, 0, nullptr, &o, cig, 8, &used) != -1 ||
            g_err.find("byte 0x6f is outside the matrix alphabet") == std::string::npos)
            return fail("a query byte outside the matrix was accepted");
        if (sw_align_matrix_translated_cpu(mx, &qp, &ql, &dp, &dl, &f1, 1, 12, 1, 3, nullptr, &o, cig, 8, &used) != -1 ||
            g_err.find("unknown alignment mode 3") == std::string::npos)
            return fail("an unknown mode was accepted");
        if (sw_align_matrix_translated_cpu(mx, &qp, &ql, &dp, &dl, &f1, 1, -1, 1, 0, nullptr, &o, cig, 8, &used) != -1)
            return fail("a negative gap penalty was accepted");
        for (const int drop : {22, 23}) {   // without 'X'; without '*'
            std::vector<unsigned char> s2;
            std::vector<signed char> t2;
            for (int i = 0; i < K; ++i)
                if (i != drop) s2.push_back(sym[i]);
            t2.assign((size_t)(K - 1) * (K - 1), 1);
            sw_matrix* m2 = sw_matrix_create(s2.data(), K - 1, t2.data(), -1, 0);
            if (!m2) return fail("sw_matrix_create", drop);
            if (sw_translated_tables(m2, nullptr, base, codon) != -1 ||
                g_err.find(drop == 22 ? "0x58" : "0x2a") == std::string::npos)
                return fail("a matrix that cannot score the code was accepted", drop);
            if (sw_align_matrix_translated_cpu(m2, &qp, &ql, &dp, &dl, &f1, 1, 12, 1, 0, nullptr, &o, cig, 8, &used) != -1 ||
                g_err.find("sw_align_matrix_translated_cpu:") == std::string::npos)
                return fail("the aligner took a matrix that cannot score the code", drop);
            sw_matrix_free(m2);
            sw_matrix* m3 = sw_matrix_create(s2.data(), K - 1, t2.data(), 0, 0);   // covered by `other`
            if (!m3 || sw_translated_tables(m3, nullptr, base, codon) != 0) return fail("`other` does not cover the byte", drop);
            sw_matrix_free(m3);
        }
    }
    sw_matrix_free(mx);
    std::printf("ok %lld %lld %lld %lld\n", translations, ranges, aligned, score_sum);
    return 0;
}
