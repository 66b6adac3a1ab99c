// Host-only check of the wedge planner's arithmetic (sw_internal.h wedge_bounds, steep_bounds): a sweep of n and m
// with the invariants the kernel and the combine kernels rely on.  Stand-alone, so it can be built with host sanitizers:
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined --offload-arch=gfx950 \
//       -I concurrentproject_amd/csrc tools/wedge_bounds_check.cpp -o build/wedge_bounds_check
#include <algorithm>
#include <cstdio>
#include <vector>

#include "sw_internal.h"

using swmi::WedgePlan;

static int fails = 0;
#define CHECK(c)                                                                       \
    do {                                                                               \
        if (!(c)) {                                                                    \
            if (fails++ < 20) std::printf("n=%d m=%d: %s\n", n, m, #c);                \
        }                                                                              \
    } while (0)

static void check(int n, int m) {
    WedgePlan w{};
    const long long S = n >= 253 ? ((long long)n - 2 + 125) / 126 : 0;
    const bool ok = swmi::wedge_bounds(n, m, &w);
    CHECK(ok == (n >= 253 && m >= 64 * S + 64));
    if (!ok) return;
    CHECK(w.strips == S && w.strips >= 2);
    CHECK(w.lead >= 0 && w.lead < 126 && 126LL * w.strips + 2 - w.lead == n);
    CHECK(w.rlead >= 0 && w.rlead < 64);
    CHECK(w.e0[0] % 64 == 0 && w.e0[1] % 64 == 0);
    CHECK((long long)w.e0[0] + w.e0[1] == (long long)m + w.rlead - 2 + 64LL * w.strips);
    CHECK(w.e0[1] - w.e0[0] == 0 || w.e0[1] - w.e0[0] == 64);
    // the last strip keeps one 64-row body; the first strip's extra step stays inside the rows
    CHECK(w.e0[0] - 64LL * (w.strips - 1) >= 64 && w.e0[1] - 64LL * (w.strips - 1) >= 64);
    CHECK(w.e0[0] <= m - 1 && w.e0[1] <= m + w.rlead - 1);
    // every boundary entry index of a chain is inside its buffer of 128 granules per strip
    if (w.strips > 4096) return;
    std::vector<char> seen((size_t)128 * w.strips, 0);
    for (int s = 0; s < w.strips; s += (w.strips > 64 ? w.strips - 1 : 1))
        for (int l = 0; l < 64; ++l)
            for (int k = 0; k < 2; ++k) seen.at((size_t)2 * (64 * s + l) + k) = 1;
}

// The steep plan with drop pattern d: admission, the row sums, and every index the kernel's segment stores and
// the steep combine kernel's segment pass form (sw_flow3.hip sw_flow3_steep_combine_kernel).
static void check_steep(int n, int m, const int d[4]) {
    WedgePlan w{};
    const long long S = n >= 253 ? (((long long)n - 2 + 125) / 126 + 3) / 4 * 4 : 0;
    const long long D = S ? swmi::steep_cum(d, S - 1) : 0;
    const bool ok = swmi::steep_bounds(n, m, d, &w);
    CHECK(ok == (n >= 253 && n <= 126 * S && m >= D + 65));
    if (!ok) return;
    CHECK(w.steep && w.strips == S && S % 4 == 0);
    CHECK(w.lead >= 0 && w.lead < 4 * 126 && 126LL * S - w.lead == n);
    CHECK(w.rlead >= 0 && w.rlead < 64 && (m + w.rlead) % 64 == 3);
    CHECK(w.e0[0] % 64 == 0 && w.e0[1] % 64 == 0);
    CHECK((long long)w.e0[0] + w.e0[1] == (long long)m + w.rlead + 61 + D);
    CHECK(w.e0[1] - w.e0[0] == 0 || w.e0[1] - w.e0[0] == 64);
    CHECK(w.e0[0] - D >= 64 && w.e0[1] - D >= 64);
    CHECK(w.e0[0] <= m - 1 && w.e0[1] <= m + w.rlead - 1);
    const long long edge_rows = std::max(w.e0[0], w.e0[1]) + 64;
    const long long segr = std::max(std::max(d[0], d[1]), std::max(d[2], d[3])) - 62;
    for (long long s = 0; s + 1 < S; s += (S > 64 && s > 8 && s + 10 < S ? S / 7 : 1)) {
        const long long s2 = S - 2 - s, drop = d[s & 3];
        // the mirrored chain's drops are the forward chain's read from the far end: the same pattern
        CHECK(d[s2 & 3] == drop && ((s & 3) == 3) == ((s2 & 3) == 3));
        const long long endf = w.e0[0] - swmi::steep_cum(d, s), endb = w.e0[1] - swmi::steep_cum(d, s2);
        for (long long k = 0; k < drop - 60; ++k) {
            const long long i = endf - drop + k;                               // node row on the hand-off column
            const long long kb = (long long)m - 1 + w.rlead - i - (endb - drop - 1);
            CHECK(kb == drop - 61 - k);
            for (const long long t : {k, kb}) {                                 // the sources of steep_col_h
                const long long end = t == k ? endf : endb;
                if (t <= drop - 64) CHECK(end - drop - 1 + t >= 0 && end - drop - 1 + t <= end - 65 && end - 65 < edge_rows);
                if (t <= drop - 64) CHECK(1 + t < segr);
            }
        }
    }
}

// The join units of a launch that joins its chains in the staged kernel (sw_internal.h join_unit_*; sw_flow3.hip
// f3_join_strip) against the index sets of the combine kernels, whose arithmetic is repeated here: the units visit
// every thread index of the combine kernel exactly once, every entry a unit loads belongs to forward strip s or to
// a mirrored strip of the range it waits for, that range is tight, the strips that count into a unit are exactly
// those it reads, and a unit's full count is their number.
static void check_units(int n, int m, const WedgePlan& w, const int d[4]) {
    const int S = w.strips;
    const bool steep = w.steep;
    const int maxcol = std::max(std::max(d[0], d[1]), std::max(d[2], d[3])) - 60;
    const int W = 126 * S + 2, pshift = steep ? 4 : 2;
    const long long threads = 64LL * S + (steep ? (long long)(S - 1) * maxcol : 0);
    std::vector<int> visits((size_t)threads, 0);
    std::vector<int> readers((size_t)S, 0);   // per unit: mirrored strips that count into it
    for (int t = 0; t < S; ++t) {             // f3_join_strip's range of a mirrored strip
        const int u0 = std::max(S - t - 2, 0), u1 = std::min(S - t - (steep ? 1 : 0), S - 1);
        CHECK(u0 <= u1);
        for (int u = u0; u <= u1; ++u) {
            CHECK(swmi::join_unit_lo(S, u, steep) <= t && t <= swmi::join_unit_hi(S, u, steep));
            ++readers[(size_t)u];
        }
    }
    for (int s = 0; s < S; ++s) {
        const int lo = swmi::join_unit_lo(S, s, steep), hi = swmi::join_unit_hi(S, s, steep);
        CHECK(0 <= lo && lo <= hi && hi < S);
        CHECK(swmi::join_unit_full(S, s, steep) == 1 + readers[(size_t)s] && readers[(size_t)s] == hi - lo + 1);
        std::vector<char> used((size_t)S, 0);
        for (int l = 0; l < 64; ++l) {   // the diagonal threads [64 s, 64 s + 64)
            ++visits.at((size_t)(64 * s + l));
            const int c = 126 * s + 2 * l;
            for (int col = 0; col < 2; ++col) {
                const int p = W - pshift - c - 2 * col;
                if (p < 0) continue;
                const int sp = p / 126, lp = (p % 126) >> 1;
                for (int dup = 0; dup < 2; ++dup) {
                    const int s2 = sp - dup;
                    if (s2 < 0 || s2 >= S || (dup && lp != 0)) continue;
                    CHECK(lo <= s2 && s2 <= hi);
                    used[(size_t)s2] = 1;
                }
            }
        }
        if (steep && s < S - 1) {        // the hand-off column: k = lane, lane + 64, ... below maxcol
            for (int lane = 0; lane < 64; ++lane)
                for (int k = lane; k < maxcol; k += 64) ++visits.at((size_t)(64LL * S + (long long)s * maxcol + k));
            const int s2 = S - 2 - s;    // its lanes, its segment entries, its group edge: all that strip's stores
            CHECK(lo <= s2 && s2 <= hi);
            used[(size_t)s2] = 1;
        }
        // tight but for dead columns: the mirrored strips in front of the frame's last live column are all read
        for (int t = lo; t <= hi; ++t) CHECK(used[(size_t)t] || W - pshift - (126 * s + 126) - 2 < 0);
    }
    for (long long i = 0; i < threads; ++i) CHECK(visits[(size_t)i] == 1);
}

int main() {
    {   // the join units of every planned shape of the sweeps below, thinned by the strip count
        const int uni[4] = {64, 64, 64, 64};
        const int upats[][4] = {{64, 64, 64, 128}, {64, 128, 64, 128}, {128, 64, 128, 128}, {256, 64, 256, 64}};
        for (int n = 253; n <= 70000; n += (n < 3000 ? 1 : 977)) {
            const int m = n + 4000;
            WedgePlan w{};
            if (swmi::wedge_bounds(n, m, &w)) check_units(n, m, w, uni);
            for (const auto& d : upats) {
                WedgePlan v{};
                if (swmi::steep_bounds(n, 4 * n + 4000, d, &v)) check_units(n, 4 * n + 4000, v, d);
            }
        }
    }
    for (int n = 1; n <= 3000; ++n)
        for (int m = 1; m <= 2200; m += (n % 7 == 0 ? 1 : 61)) check(n, m);
    const int pats[][4] = {{64, 64, 64, 128}, {64, 128, 64, 128}, {128, 128, 128, 128}, {64, 64, 64, 192}, {256, 64, 256, 64}};
    const int bad[][4] = {{64, 64, 128, 64}, {64, 96, 64, 128}, {0, 64, 0, 64}, {64, 64, 64, 320}};
    for (const auto& d : bad) {
        WedgePlan w{};
        if (swmi::wedge_drops_ok(d) || swmi::steep_bounds(1000, 100000, d, &w)) ++fails;
    }
    for (const auto& d : pats) {
        for (int n = 240; n <= 1600; ++n)
            for (int m = 1; m <= 6000; m += (n % 25 == 0 ? 1 : 53)) check_steep(n, m, d);
        const int bign[] = {4096, 16384, 65536, 1 << 20};
        const int bigm[] = {4096, 16384, 65536, 1 << 20, (1 << 27) - 1};
        for (int n : bign)
            for (int m : bigm)
                for (int e = -70; e <= 70; e += 7) check_steep(n, m + e > (1 << 27) - 1 ? m : m + e, d);
    }
    const int big[] = {4096, 16384, 65536, 1 << 20, (1 << 27) - 1};
    for (int n : big)
        for (int m : big)
            for (int d = -70; d <= 70; ++d)
                if (m + d > 0 && (long long)m + d <= (1LL << 27) - 1) check(n, m + d);
    std::printf("wedge_bounds_check: %d failures\n", fails);
    return fails ? 1 : 0;
}
