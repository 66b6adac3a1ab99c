// sw_align_host.cpp -- alignments under a substitution matrix, host only (no HIP): the argument
// checks shared by the GPU and the CPU entry points, the reverse-and-encode routine that turns a
// walk's operations into run-length encoded cigar entries, and sw_align_matrix_cpu, a plain
// full-matrix aligner with exactly the end-cell rule and the walk priorities of the traced kernel
// (sw_matrix.hip; include/algoGPU.h states both).  It checks the GPU path and is a usable
// fallback for a machine without a device; it needs n * m bytes a pair.  Also the arithmetic of
// the checkpointed traceback of long pairs (sw_align_matrix_long): strips, checkpoint and strip
// trace bytes, the two budgets' refusals and the greedy packing of groups and rounds; the exported
// sw_align_long_plan (sw_matrix.hip) only reads option "trace_mb" and calls it.  The same for the long path on
// many waves (sw_align_matrix_long_coop): the merge of the strips' end-cell records, the window of strips a round
// fills, and the plan behind sw_align_long_coop_plan.
// And the host side of global and semi-global alignment (SW_MODE_*): the mode and score-range checks,
// the answers for empty sequences, and sw_align_matrix_cpu_mode, the same plain aligner for those modes.
// And banded alignment (sw_*_band): the band's arithmetic (range, cells, the strips' chunks, trace bytes),
// sw_band_plan, and sw_align_matrix_cpu_band, the plain aligner restricted to a band, every mode.
// And position-specific scoring (sw_*_profile_*): the entry points' checks, and sw_align_profile_cpu: the local and
// the mode aligner are templates on where a cell's score comes from, a table row by residue or a profile row by position.
#include "sw_matrix_host.h"
#include "../../include/algoGPU.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace swmi {

namespace {
constexpr long long ALIGN_MAX_SEQ = (1LL << 27) - 1;   // the engine's longest sequence (sw_matrix.hip)
constexpr long long CPU_MAX_CELLS = 1LL << 32;         // the CPU aligner's matrix: a byte a cell
}  // namespace

int align_check(const char* fn, const sw_matrix* mx, const unsigned char* const* a, const int* alen,
                const unsigned char* const* b, const int* blen, int npairs, int gap_init, int gap_ext,
                const sw_alignment* out, const unsigned* cigar, long long cigar_cap, const long long* cigar_used) {
    char m[200];
    if (!mx || npairs < 0 || cigar_cap < 0 || !cigar_used || (cigar_cap > 0 && !cigar) ||
        (npairs > 0 && (!a || !alen || !b || !blen || !out))) {
        std::snprintf(m, sizeof m, "%s: invalid arguments", fn);
        report_error(m);
        return -1;
    }
    if (gap_init < 0 || gap_ext < 0 || gap_init > (1 << 20) || gap_ext > (1 << 20)) {
        std::snprintf(m, sizeof m, "unsupported gap penalties (%d, %d): need 0 <= G_INIT, G_EXT <= 2^20", gap_init, gap_ext);
        report_error(m);
        return -1;
    }
    for (int k = 0; k < npairs; ++k) {
        if (alen[k] < 0 || blen[k] < 0 || (alen[k] > 0 && !a[k]) || (blen[k] > 0 && !b[k]) || alen[k] > ALIGN_MAX_SEQ ||
            blen[k] > ALIGN_MAX_SEQ) {
            std::snprintf(m, sizeof m, "pair %d: invalid sequence pointer or length", k);
            report_error(m);
            return -1;
        }
        if (alen[k] == 0 || blen[k] == 0) continue;
        if (!align_range_ok(mx, alen[k], blen[k], "pair", k)) return -1;
        for (int s = 0; s < 2; ++s) {
            const unsigned char* p = s ? b[k] : a[k];
            const long long bad = matrix_first_bad(mx, p, s ? blen[k] : alen[k]);
            if (bad >= 0) {
                std::snprintf(m, sizeof m, "pair %d: seq%d position %lld: byte 0x%02x is outside the matrix alphabet", k,
                              s + 1, bad, p[bad]);
                report_error(m);
                return -1;
            }
        }
    }
    return 0;
}

bool align_range_ok(const sw_matrix* mx, int alen, int blen, const char* what, int idx) {
    if ((long long)std::min(alen, blen) * std::max(mx->max_entry, 0) >= (1LL << 28)) {
        char m[160];
        std::snprintf(m, sizeof m, "%s %d: score range exceeds the int32 engine (min length * largest entry >= 2^28)", what, idx);
        report_error(m);
        return false;
    }
    return true;
}

// ops_rev[0, nops): the walk's operations, last first.  Appends the run-length encoded entries
// ((length << 4) | op), first operation first, to out; returns how many.  A run longer than
// 2^28 - 1 is split.
int encode_ops(const unsigned char* ops_rev, long long nops, std::vector<unsigned>& out) {
    int added = 0;
    long long k = nops - 1;
    while (k >= 0) {
        const unsigned op = ops_rev[k];
        unsigned run = 0;
        while (k >= 0 && ops_rev[k] == op && run < (1u << 28) - 1) {
            ++run;
            --k;
        }
        out.push_back((run << 4) | (op & 15u));
        ++added;
    }
    return added;
}

void AlignSink::set(int k, int score, int beg1, int end1, int beg2, int end2, const unsigned char* ops_rev, long long nops) {
    sw_alignment& o = out[k];
    o.score = score;
    o.beg1 = beg1;
    o.end1 = end1;
    o.beg2 = beg2;
    o.end2 = end2;
    o.cigar_off = (long long)cig.size();
    o.ncigar = encode_ops(ops_rev, nops, cig);
}

void AlignSink::set_empty(int k) {
    sw_alignment& o = out[k];
    o.score = o.beg1 = o.end1 = o.beg2 = o.end2 = o.ncigar = 0;
    o.cigar_off = (long long)cig.size();
}

int AlignSink::finish(unsigned* cigar, long long cigar_cap, long long* cigar_used) {
    *cigar_used = (long long)cig.size();
    if ((long long)cig.size() > cigar_cap) {
        char m[160];
        std::snprintf(m, sizeof m, "cigar buffer too small: %lld entries needed, cigar_cap is %lld", (long long)cig.size(),
                      cigar_cap);
        report_error(m);
        return -1;
    }
    if (!cig.empty()) std::memcpy(cigar, cig.data(), cig.size() * sizeof(unsigned));
    return 0;
}

// ---- position-specific scoring: the checks of the sw_*_profile_* entry points (sw_matrix_host.h) ----

bool profile_range_ok(const sw_profile* pf, int len, int gap_init, int gap_ext, int amode, const char* what, int idx) {
    if (amode != SW_MODE_LOCAL && !mode_range_ok(pf->n, len, gap_init, gap_ext, what, idx)) return false;
    return len == 0 || align_range_ok(&pf->alpha, pf->n, len, what, idx);
}

int profile_check(const char* fn, const sw_profile* pf, const unsigned char* const* seqs, const int* lens, int nseq,
                  int gap_init, int gap_ext, int mode) {
    char m[200];
    if (!pf || nseq < 0 || (nseq > 0 && (!seqs || !lens))) {
        std::snprintf(m, sizeof m, "%s: invalid arguments", fn);
        report_error(m);
        return -1;
    }
    if (!mode_ok(fn, mode)) return -1;
    if (gap_init < 0 || gap_ext < 0 || gap_init > (1 << 20) || gap_ext > (1 << 20)) {
        std::snprintf(m, sizeof m, "unsupported gap penalties (%d, %d): need 0 <= G_INIT, G_EXT <= 2^20", gap_init, gap_ext);
        report_error(m);
        return -1;
    }
    for (int k = 0; k < nseq; ++k) {
        if (lens[k] < 0 || (lens[k] > 0 && !seqs[k]) || lens[k] > ALIGN_MAX_SEQ) {
            std::snprintf(m, sizeof m, "sequence %d: invalid sequence pointer or length", k);
            report_error(m);
            return -1;
        }
        if (!profile_range_ok(pf, lens[k], gap_init, gap_ext, mode, "sequence", k)) return -1;
        const long long bad = matrix_first_bad(&pf->alpha, seqs[k], lens[k]);
        if (bad >= 0) {
            std::snprintf(m, sizeof m, "sequence %d: position %lld: byte 0x%02x is outside the profile alphabet", k, bad,
                          seqs[k][bad]);
            report_error(m);
            return -1;
        }
    }
    return 0;
}

int profile_align_check(const char* fn, const sw_profile* pf, const unsigned char* const* seqs, const int* lens, int nseq,
                        int gap_init, int gap_ext, int mode, const sw_alignment* out, const unsigned* cigar,
                        long long cigar_cap, const long long* cigar_used) {
    if (cigar_cap < 0 || !cigar_used || (cigar_cap > 0 && !cigar) || (nseq > 0 && !out)) {
        char m[200];
        std::snprintf(m, sizeof m, "%s: invalid arguments", fn);
        report_error(m);
        return -1;
    }
    return profile_check(fn, pf, seqs, lens, nseq, gap_init, gap_ext, mode);
}

// ---- translated search: the checks of the sw_*_matrix_translated_* entry points (sw_matrix_host.h) ----

bool translated_range_ok(const char* fn, const sw_matrix* mx, int alen, int dlen, int gap_init, int gap_ext, int amode,
                         const char* what, int idx) {
    const int m = frame_residues(dlen, 0);   // frame +1 is the longest, and both bounds grow with m
    char w[96];
    std::snprintf(w, sizeof w, "%s: %s", fn, what);
    if (amode != SW_MODE_LOCAL && !mode_range_ok(alen, m, gap_init, gap_ext, w, idx)) return false;
    return alen == 0 || m == 0 || align_range_ok(mx, alen, m, w, idx);
}

int translated_check(const char* fn, const sw_matrix* mx, const unsigned char* const* a, const int* alen,
                     const unsigned char* const* dna, const int* dlen, const int* frames, int npairs, int gap_init,
                     int gap_ext, int mode, const unsigned char* code64, Translated* xl) {
    char m[240];
    if (!mx || npairs < 0 || (npairs > 0 && (!a || !alen || !dna || !dlen))) {
        std::snprintf(m, sizeof m, "%s: invalid arguments (a null pointer)", fn);
        report_error(m);
        return -1;
    }
    if (!mode_ok(fn, mode)) return -1;
    if (gap_init < 0 || gap_ext < 0 || gap_init > (1 << 20) || gap_ext > (1 << 20)) {
        std::snprintf(m, sizeof m, "%s: unsupported gap penalties (%d, %d): need 0 <= G_INIT, G_EXT <= 2^20", fn, gap_init,
                      gap_ext);
        report_error(m);
        return -1;
    }
    if (translated_tables(fn, mx, code64, xl)) return -1;
    for (int k = 0; k < npairs; ++k) {
        if (frames && frame_index(frames[k]) < 0) {
            std::snprintf(m, sizeof m, "%s: pair %d: frame %d is not one of +1, +2, +3, -1, -2, -3", fn, k, frames[k]);
            report_error(m);
            return -1;
        }
        if (alen[k] < 0 || dlen[k] < 0 || alen[k] > ALIGN_MAX_SEQ || dlen[k] > ALIGN_MAX_SEQ) {
            std::snprintf(m, sizeof m, "%s: pair %d: a length of %d residues / %d bases is outside [0, 2^27 - 1]", fn, k, alen[k],
                          dlen[k]);
            report_error(m);
            return -1;
        }
        if ((alen[k] > 0 && !a[k]) || (dlen[k] > 0 && !dna[k])) {
            std::snprintf(m, sizeof m, "%s: pair %d: a null sequence pointer", fn, k);
            report_error(m);
            return -1;
        }
        if (!translated_range_ok(fn, mx, alen[k], dlen[k], gap_init, gap_ext, mode, "pair", k)) return -1;
        const long long bad = matrix_first_bad(mx, a[k], alen[k]);
        if (bad >= 0) {
            std::snprintf(m, sizeof m, "%s: pair %d: seq1 position %lld: byte 0x%02x is outside the matrix alphabet", fn, k, bad,
                          a[k][bad]);
            report_error(m);
            return -1;
        }
    }
    return 0;
}

// ---- long pairs: the plan of a checkpointed traceback (sw_matrix_host.h) ----

long long align_strip_steps(long long m) { return (m + ALIGN_STRIP - 1 + 63) / 64 * 64; }
long long align_strip_trace_bytes(long long m) { return align_strip_steps(m) * 256; }
long long align_ckpt_stride(long long m) { return (m + 63) / 64 * 64 * 8; }
long long align_strips(long long n) { return (n + ALIGN_STRIP - 1) / ALIGN_STRIP; }

int align_long_plan(int n, int m, long long trace_budget, long long ckpt_budget, const char* what, int idx,
                    sw_align_plan* out) {
    sw_align_plan p{0, 0, 0, 0};
    if (n > 0 && m > 0) {
        p.strips = (int)align_strips(n);
        p.ckpt_bytes = (long long)(p.strips - 1) * align_ckpt_stride(m);
        p.strip_trace_bytes = align_strip_trace_bytes(m);
        p.full_trace_bytes = (long long)p.strips * p.strip_trace_bytes;
    }
    *out = p;
    char msg[256];
    if (p.ckpt_bytes > ckpt_budget) {
        std::snprintf(msg, sizeof msg,
                      "%s %d: a %d x %d alignment needs %lld bytes of checkpoints, more than SWMI_ALIGN_CKPT_MB = %lld MiB",
                      what, idx, n, m, p.ckpt_bytes, ckpt_budget >> 20);
        report_error(msg);
        return -1;
    }
    if (p.strip_trace_bytes > trace_budget) {
        std::snprintf(msg, sizeof msg,
                      "%s %d: a %d x %d alignment needs %lld bytes of trace memory for one strip, more than option "
                      "trace_mb = %lld MiB",
                      what, idx, n, m, p.strip_trace_bytes, trace_budget >> 20);
        report_error(msg);
        return -1;
    }
    return 0;
}

int align_ckpt_budget(long long* bytes) {
    long long mb = 4096;
    if (const char* e = std::getenv("SWMI_ALIGN_CKPT_MB")) {
        char* end = nullptr;
        mb = std::strtoll(e, &end, 10);
        if (end == e || *end != 0 || mb < 1 || mb > (1LL << 40)) {
            report_error("SWMI_ALIGN_CKPT_MB must be a whole number of MiB, at least 1");
            return -1;
        }
    }
    *bytes = mb << 20;
    return 0;
}

void align_pack(const long long* need, int n, long long budget, std::vector<int>& end) {
    end.clear();
    int k = 0;
    while (k < n) {
        long long sum = 0;
        for (; k < n; ++k) {
            if (sum > 0 && need[k] > 0 && sum + need[k] > budget) break;
            sum += need[k];
        }
        end.push_back(k);
    }
}

// ---- long pairs on many waves: records, windows and the plan (sw_matrix_host.h) ----

void align_merge_ends(const AlignEnd* rec, int nrec, int* score, int* ei, int* ej) {
    int bM = 0, bD = 0, bJ = 0;
    for (int k = 0; k < nrec; ++k) {
        const AlignEnd& r = rec[k];
        if (r.t <= 0) continue;   // a strip without a cell
        const bool better = r.t > bM || (r.t == bM && (r.d < bD || (r.d == bD && r.j < bJ)));
        bM = better ? r.t : bM;
        bD = better ? r.d : bD;
        bJ = better ? r.j : bJ;
    }
    *score = bM;
    *ei = bM > 0 ? bD - bJ : 0;
    *ej = bM > 0 ? bJ : 0;
}

long long align_progress_bytes(long long items) { return (items * 4 + 15) / 16 * 16; }
long long align_end_bytes(long long items) { return items * (long long)sizeof(AlignEnd); }

int align_window(long long strip_bytes, long long live_bytes, long long trace_budget, int long_window, int strip) {
    long long g = long_window > 0 ? std::min<long long>(long_window, trace_budget / std::max<long long>(strip_bytes, 1))
                                  : trace_budget / std::max<long long>(live_bytes, 1);
    g = std::min<long long>(g, ALIGN_WINDOW_MAX);
    g = std::min<long long>(g, (long long)strip + 1);
    return (int)std::max<long long>(g, 1);
}

int align_long_coop_plan(int n, int m, long long trace_budget, long long ckpt_budget, int long_window, const char* what,
                         int idx, sw_align_coop_plan* out) {
    sw_align_plan p;
    const int rc = align_long_plan(n, m, trace_budget, ckpt_budget, what, idx, &p);
    sw_align_coop_plan q{0, 0, 0, 0, 0, 0};
    if (p.strips > 0) {
        q.strips = p.strips;
        q.ckpt_bytes = p.ckpt_bytes;
        q.progress_bytes = align_progress_bytes(p.strips);
        q.end_bytes = align_end_bytes(p.strips);
        q.window = align_window(p.strip_trace_bytes, p.strip_trace_bytes, trace_budget, long_window, p.strips - 1);
        q.window_trace_bytes = q.window * p.strip_trace_bytes;
    }
    *out = q;
    return rc;
}

bool mode_ok(const char* fn, int mode) {
    if (mode == SW_MODE_LOCAL || mode == SW_MODE_GLOBAL || mode == SW_MODE_SEMIGLOBAL) return true;
    char m[160];
    std::snprintf(m, sizeof m, "%s: unknown alignment mode %d (0 local, 1 global, 2 semi-global)", fn, mode);
    report_error(m);
    return false;
}

bool mode_range_ok(int alen, int blen, int gap_init, int gap_ext, const char* what, int idx) {
    const long long unit = std::max<long long>(std::max(gap_init, gap_ext), 127);
    if (((long long)alen + blen + 1024) * unit >= (1LL << 28)) {
        char m[200];
        std::snprintf(m, sizeof m,
                      "%s %d: score range exceeds the int32 engine in this mode ((n + m + 1024) * max(G_INIT, G_EXT, 127) >= 2^28)",
                      what, idx);
        report_error(m);
        return false;
    }
    return true;
}

int mode_empty_score(int alen, int blen, int gap_init, int gap_ext, int mode) {
    const int L = mode == SW_MODE_GLOBAL ? std::max(alen, blen) : mode == SW_MODE_SEMIGLOBAL ? alen : 0;
    return L > 0 ? -(gap_init + (L - 1) * std::min(gap_ext, gap_init)) : 0;
}

void align_mode_empty(AlignSink& sink, int k, int alen, int blen, int gap_init, int gap_ext, int mode) {
    const int score = mode_empty_score(alen, blen, gap_init, gap_ext, mode);
    const bool seq1 = alen > 0;   // the run: I over seq1, or (global only) D over seq2
    const int L = mode == SW_MODE_GLOBAL ? std::max(alen, blen) : mode == SW_MODE_SEMIGLOBAL ? alen : 0;
    if (L == 0) {
        sink.set_empty(k);
        return;
    }
    const std::vector<unsigned char> ops((size_t)L, (unsigned char)(seq1 ? 1 : 2));
    sink.set(k, score, 0, seq1 ? L : 0, 0, seq1 ? 0 : L, ops.data(), L);
}

// ---- long pairs in a mode: the end record, the end cell and the refusals (sw_matrix_host.h) ----

void align_mode_end(const AlignEnd* rec, int nrec, int* score, int* ei, int* ej) {
    const AlignEnd none{0, 0, 0, 0};
    const AlignEnd& r = nrec > 0 ? rec[nrec - 1] : none;   // only the last strip holds column n - 1
    *score = r.t;
    *ei = r.d;
    *ej = r.j;
}

bool align_long_end_ok(int n, int m, int mode, int ei, int ej) {
    if (ei < 0 || ei >= n || ej < 0 || ej >= m) return false;
    if (mode == SW_MODE_LOCAL) return true;
    return ei == n - 1 && (mode != SW_MODE_GLOBAL || ej == m - 1);
}

int align_long_mode_check(const char* fn, int mode, const int* alen, const int* blen, const int* name_idx, int npairs,
                          int gap_init, int gap_ext, const char* what) {
    if (!mode_ok(fn, mode)) return -1;
    if (mode == SW_MODE_LOCAL) return 0;
    for (int k = 0; k < npairs; ++k)
        if (!mode_range_ok(alen[k], blen[k], gap_init, gap_ext, what, name_idx ? name_idx[k] : k)) return -1;
    return 0;
}

// ---- banded alignment: the arithmetic of a band (sw_matrix_host.h) ----

bool band_ok(const char* fn, int band) {
    if (band >= 0) return true;
    char m[160];
    std::snprintf(m, sizeof m, "%s: band %d is negative (a band is the distance from the corner-to-corner diagonal, >= 0)", fn,
                  band);
    report_error(m);
    return false;
}

void band_range(int n, int m, int band, int* dlo, int* dhi) {
    const int B = std::min(band, std::max(n, m));
    *dlo = std::min(0, m - n) - B;
    *dhi = std::max(0, m - n) + B;
}

long long band_cells(long long n, long long m, long long dlo, long long dhi) {
    long long cells = 0;
    for (long long i = 0; i < n; ++i) cells += std::max(0LL, std::min(m - 1, i + dhi) - std::max(0LL, i + dlo) + 1);
    return cells;
}

long long band_first(long long i0, long long dlo) { return std::max(0LL, i0 + dlo - 1) / 64 * 64; }
long long band_chunks(long long i0, long long SW, long long m, long long dlo, long long dhi) {
    return (std::min(m - 1, i0 + SW - 1 + dhi) + SW - 1 - band_first(i0, dlo)) / 64 + 1;
}

long long band_steps(long long n, long long m, long long dlo, long long dhi, int W, long long* most) {
    const long long SW = 64LL * W;
    long long sum = 0, mx = 0;
    for (long long i0 = 0; i0 < n; i0 += SW) {
        const long long st = 64 * band_chunks(i0, SW, m, dlo, dhi);
        sum += st;
        mx = std::max(mx, st);
    }
    *most = mx;
    return sum;
}

long long band_trace_steps(long long m, long long dlo, long long dhi) { return std::min(dhi - dlo, m - 1) + 15; }
long long band_trace_bytes(long long n, long long m, long long dlo, long long dhi) {
    return align_strips(n) * 64 * band_trace_steps(m, dlo, dhi) * 4;
}

namespace {

constexpr int CPU_NEG = -(1 << 30);   // "minus infinity": mode_range_ok keeps every cell far above it

// One pair in a band, both lengths > 0, any mode: align_pair / align_pair_mode over the cells with
// dlo <= j - i <= dhi.  A neighbour outside the band is absent: in local mode the border state
// H = E = F = 0; else it offers minus infinity to E and to F, open and extend alike (what the kernel's
// forced cell offers, so that every recorded bit is the kernel's).  The borders are not masked.  The
// diagonal neighbour lies on the cell's own diagonal: in the band, or a border.
void align_pair_band(const sw_matrix* mx, const unsigned char* a, int n, const unsigned char* b, int m, int go, int ge,
                     int mode, int dlo, int dhi, std::vector<unsigned char>& cell, std::vector<int>& hup, std::vector<int>& fup,
                     std::vector<unsigned char>& ops, int k, AlignSink& sink) {
    const bool local = mode == SW_MODE_LOCAL;
    const int gx = std::min(go, ge);
    cell.assign((size_t)n * (size_t)m, 0);
    hup.resize((size_t)n);
    fup.assign((size_t)n, local ? 0 : CPU_NEG);
    for (int i = 0; i < n; ++i) hup[(size_t)i] = local ? 0 : -(go + i * gx);   // H[i][-1]
    int best = local ? 0 : CPU_NEG, bi = local ? 0 : n - 1, bj = 0;
    for (int j = 0; j < m; ++j) {
        const int cb = mx->code[b[j]];
        const int ilo = (int)std::max<long long>(0, (long long)j - dhi), ihi = (int)std::min<long long>(n - 1, (long long)j - dlo);
        if (ilo > ihi) continue;   // (never: the band holds a cell of every row)
        // the cell left of ilo: the border H[-1][j] (E[-1][j] is minus infinity), or absent
        const bool left_absent = ilo > 0;
        int hleft = local || mode == SW_MODE_SEMIGLOBAL ? 0 : -(go + j * gx);
        int eleft = local ? 0 : CPU_NEG;
        int hdiag = ilo > 0 ? hup[(size_t)ilo - 1] : (local || mode == SW_MODE_SEMIGLOBAL || j == 0 ? 0 : -(go + (j - 1) * gx));
        unsigned char* row = cell.data() + (size_t)j * (size_t)n;
        for (int i = ilo; i <= ihi; ++i) {
            const bool la = left_absent && i == ilo;
            const bool ua = j > 0 && (long long)j - 1 - i < dlo;   // the cell above: absent (row -1 is a border)
            int eo = hleft - go, ee = eleft - ge;
            int fo = hup[(size_t)i] - go, fe = fup[(size_t)i] - ge;
            if (la) {
                eo = local ? -go : CPU_NEG;
                ee = local ? -ge : CPU_NEG;
            }
            if (ua) {
                fo = local ? -go : CPU_NEG;
                fe = local ? -ge : CPU_NEG;
            }
            int E = std::max(eo, ee), F = std::max(fo, fe);
            if (local) E = std::max(E, 0), F = std::max(F, 0);
            const int t = hdiag + mx->sc[mx->code[a[i]] * mx->k + cb];
            const int H = std::max(t, std::max(E, F));
            row[i] = (unsigned char)((local && H == 0 ? 0 : t == H ? 1 : E == H ? 2 : 3) | (ee > eo ? 4 : 0) | (fe > fo ? 8 : 0));
            if (local && (t > best || (t == best && t > 0 && (i + j < bi + bj || (i + j == bi + bj && j < bj))))) {
                best = t;
                bi = i;
                bj = j;
            }
            hdiag = hup[(size_t)i];
            hup[(size_t)i] = H;
            fup[(size_t)i] = F;
            hleft = H;
            eleft = E;
        }
        if (!local && ihi == n - 1) {   // the end: (n-1, m-1) (global); the largest H[n-1][j] in the band, the smallest such j
            const int h = hup[(size_t)n - 1];
            if (mode == SW_MODE_GLOBAL ? j == m - 1 : h > best) {
                best = h;
                bj = j;
            }
        }
    }
    if (local && best <= 0) {
        sink.set_empty(k);
        return;
    }
    ops.resize((size_t)n + (size_t)m);
    long long nops = 0;
    int i = bi, j = bj, state = 0;   // 0 H, 1 E, 2 F
    while (i >= 0 && j >= 0 && nops < (long long)n + m) {
        const int c = cell[(size_t)j * (size_t)n + (size_t)i];
        if (state == 0) {
            const int src = c & 3;
            if (src == 0) break;   // local: H = 0 (also a cell outside the band, which the walk never enters)
            if (src == 1) {
                ops[(size_t)nops++] = 0;
                --i;
                --j;
            } else {
                state = src == 2 ? 1 : 2;
            }
        } else if (state == 1) {
            ops[(size_t)nops++] = 1;
            state = (c & 4) ? 1 : 0;
            --i;
        } else {
            ops[(size_t)nops++] = 2;
            state = (c & 8) ? 2 : 0;
            --j;
        }
    }
    if (!local) {   // the border exits of align_pair_mode
        if (j < 0) {
            for (; i >= 0 && nops < (long long)n + m; --i) ops[(size_t)nops++] = 1;
        } else if (i < 0 && mode == SW_MODE_GLOBAL) {
            for (; j >= 0 && nops < (long long)n + m; --j) ops[(size_t)nops++] = 2;
        }
    }
    sink.set(k, best, i + 1, bi + 1, j + 1, bj + 1, ops.data(), nops);
}

// The score of a cell, the one thing align_pair_mode and align_pair do not know: s(i, cb), i a position of seq1
// and cb the code of seq2's residue.  Under a matrix it is the table row of seq1's residue; under a profile
// (sw_align_profile_cpu) the row of position i itself.
struct MatrixScore {
    const sw_matrix* mx;
    const unsigned char* a;
    int operator()(int i, int cb) const { return mx->sc[mx->code[a[i]] * mx->k + cb]; }
};
struct ProfileScore {
    const sw_profile* pf;
    int operator()(int i, int cb) const { return pf->sc[(size_t)i * (size_t)pf->alpha.k + (size_t)cb]; }
};

// Global and semi-global (include/algoGPU.h): one pair, both lengths > 0, three full rows of state
// and a byte a cell as align_pair below, the unclamped recurrence with its borders, the end rule and
// the walk with its border exits.
template <class SCORE>
void align_pair_mode(const SCORE& s, const unsigned char* code, int n, const unsigned char* b, int m, int go, int ge,
                     int mode, std::vector<unsigned char>& cell, std::vector<int>& hup, std::vector<int>& fup,
                     std::vector<unsigned char>& ops, int k, AlignSink& sink) {
    const int gx = std::min(go, ge);
    cell.assign((size_t)n * (size_t)m, 0);
    hup.resize((size_t)n);
    fup.assign((size_t)n, CPU_NEG);
    for (int i = 0; i < n; ++i) hup[(size_t)i] = -(go + i * gx);   // H[i][-1]
    int best = CPU_NEG, bj = 0;
    for (int j = 0; j < m; ++j) {
        const int cb = code[b[j]];
        // H[-1][j] and H[-1][j-1]; E[-1][j] is minus infinity
        int hleft = mode == SW_MODE_GLOBAL ? -(go + j * gx) : 0;
        int hdiag = j == 0 || mode != SW_MODE_GLOBAL ? 0 : -(go + (j - 1) * gx);
        int eleft = CPU_NEG;
        unsigned char* row = cell.data() + (size_t)j * (size_t)n;
        for (int i = 0; i < n; ++i) {
            const int eo = hleft - go, ee = eleft - ge;
            const int fo = hup[(size_t)i] - go, fe = fup[(size_t)i] - ge;
            const int E = std::max(eo, ee);
            const int F = std::max(fo, fe);
            const int t = hdiag + s(i, cb);
            const int H = std::max(t, std::max(E, F));
            row[i] = (unsigned char)((t == H ? 1 : E == H ? 2 : 3) | (ee > eo ? 4 : 0) | (fe > fo ? 8 : 0));
            hdiag = hup[(size_t)i];
            hup[(size_t)i] = H;
            fup[(size_t)i] = F;
            hleft = H;
            eleft = E;
        }
        // the end: H[n-1][m-1] (global); the largest H[n-1][j], the smallest such j (semi-global)
        const int h = hup[(size_t)n - 1];
        if (mode == SW_MODE_GLOBAL ? j == m - 1 : h > best) {
            best = h;
            bj = j;
        }
    }
    ops.resize((size_t)n + (size_t)m);
    long long nops = 0;
    int i = n - 1, j = bj, state = 0;   // 0 H, 1 E, 2 F
    while (i >= 0 && j >= 0 && nops < (long long)n + m) {
        const int c = cell[(size_t)j * (size_t)n + (size_t)i];
        if (state == 0) {
            const int src = c & 3;
            if (src == 1) {
                ops[(size_t)nops++] = 0;
                --i;
                --j;
            } else {
                state = src == 2 ? 1 : 2;
            }
        } else if (state == 1) {
            ops[(size_t)nops++] = 1;
            state = (c & 4) ? 1 : 0;
            --i;
        } else {
            ops[(size_t)nops++] = 2;
            state = (c & 8) ? 2 : 0;
            --j;
        }
    }
    // the border exits: at j < 0 the rest of seq1 is one leading I run; at i < 0 the rest of seq2 is
    // one leading D run (global) or free (semi-global: beg2 = j + 1)
    if (j < 0) {
        for (; i >= 0 && nops < (long long)n + m; --i) ops[(size_t)nops++] = 1;
    } else if (i < 0 && mode == SW_MODE_GLOBAL) {
        for (; j >= 0 && nops < (long long)n + m; --j) ops[(size_t)nops++] = 2;
    }
    sink.set(k, best, i + 1, n, j + 1, bj + 1, ops.data(), nops);
}

// One pair, both lengths > 0.  cell[j * n + i]: bits 0-1 where H came from (0 none: H = 0, 1 diagonal,
// 2 E, 3 F), bit 2 E extended a gap (else opened one), bit 3 the same for F; E runs along seq1
// (operation I), F along seq2 (operation D).  The clamped form of the kernel: E and F are kept as
// max(E, 0), max(F, 0), which changes no H and no decision at a cell the walk can visit.
template <class SCORE>
void align_pair(const SCORE& s, const unsigned char* code, int n, const unsigned char* b, int m, int go, int ge,
                std::vector<unsigned char>& cell, std::vector<int>& hup, std::vector<int>& fup,
                std::vector<unsigned char>& ops, int k, AlignSink& sink) {
    cell.assign((size_t)n * (size_t)m, 0);
    hup.assign((size_t)n, 0);
    fup.assign((size_t)n, 0);
    int best = 0, bi = 0, bj = 0;
    for (int j = 0; j < m; ++j) {
        const int cb = code[b[j]];
        int hleft = 0, eleft = 0, hdiag = 0;
        unsigned char* row = cell.data() + (size_t)j * (size_t)n;
        for (int i = 0; i < n; ++i) {
            const int eo = hleft - go, ee = eleft - ge;
            const int fo = hup[(size_t)i] - go, fe = fup[(size_t)i] - ge;
            const int E = std::max(std::max(eo, ee), 0);
            const int F = std::max(std::max(fo, fe), 0);
            const int t = hdiag + s(i, cb);
            const int H = std::max(t, std::max(E, F));
            row[i] = (unsigned char)((H == 0 ? 0 : t == H ? 1 : E == H ? 2 : 3) | (ee > eo ? 4 : 0) | (fe > fo ? 8 : 0));
            // the end cell: largest t, then smallest i + j, then smallest j
            if (t > best || (t == best && t > 0 && (i + j < bi + bj || (i + j == bi + bj && j < bj)))) {
                best = t;
                bi = i;
                bj = j;
            }
            hdiag = hup[(size_t)i];
            hup[(size_t)i] = H;
            fup[(size_t)i] = F;
            hleft = H;
            eleft = E;
        }
    }
    if (best <= 0) {
        sink.set_empty(k);
        return;
    }
    // the walk: from the end cell in state H, operations last first
    ops.resize((size_t)n + (size_t)m);
    long long nops = 0;
    int i = bi, j = bj, state = 0;   // 0 H, 1 E, 2 F
    while (i >= 0 && j >= 0 && nops < (long long)n + m) {
        const int c = cell[(size_t)j * (size_t)n + (size_t)i];
        if (state == 0) {
            const int src = c & 3;
            if (src == 0) break;
            if (src == 1) {
                ops[(size_t)nops++] = 0;
                --i;
                --j;
            } else {
                state = src == 2 ? 1 : 2;
            }
        } else if (state == 1) {
            ops[(size_t)nops++] = 1;
            state = (c & 4) ? 1 : 0;
            --i;
        } else {
            ops[(size_t)nops++] = 2;
            state = (c & 8) ? 2 : 0;
            --j;
        }
    }
    sink.set(k, best, i + 1, bi + 1, j + 1, bj + 1, ops.data(), nops);
}

}  // namespace
}  // namespace swmi

using namespace swmi;

extern "C" {

int sw_align_matrix_cpu(const sw_matrix* mx, const unsigned char* const* a, const int* alen,
                        const unsigned char* const* b, const int* blen, int npairs, int gap_init, int gap_ext,
                        sw_alignment* out, unsigned* cigar, long long cigar_cap, long long* cigar_used) {
    if (align_check("sw_align_matrix_cpu", mx, a, alen, b, blen, npairs, gap_init, gap_ext, out, cigar, cigar_cap, cigar_used))
        return -1;
    for (int k = 0; k < npairs; ++k)
        if ((long long)alen[k] * blen[k] > CPU_MAX_CELLS) {
            char m[160];
            std::snprintf(m, sizeof m, "pair %d: %lld cells are more than the CPU aligner's full matrix holds (2^32)", k,
                          (long long)alen[k] * blen[k]);
            report_error(m);
            return -1;
        }
    AlignSink sink{out, {}};
    std::vector<unsigned char> cell, ops;
    std::vector<int> hup, fup;
    for (int k = 0; k < npairs; ++k) {
        if (alen[k] == 0 || blen[k] == 0) sink.set_empty(k);
        else align_pair(MatrixScore{mx, a[k]}, mx->code, alen[k], b[k], blen[k], gap_init, gap_ext, cell, hup, fup, ops, k, sink);
    }
    return sink.finish(cigar, cigar_cap, cigar_used);
}

int sw_align_matrix_cpu_mode(const sw_matrix* mx, const unsigned char* const* a, const int* alen,
                             const unsigned char* const* b, const int* blen, int npairs, int gap_init, int gap_ext, int mode,
                             sw_alignment* out, unsigned* cigar, long long cigar_cap, long long* cigar_used) {
    if (!mode_ok("sw_align_matrix_cpu_mode", mode)) return -1;
    if (mode == SW_MODE_LOCAL)
        return sw_align_matrix_cpu(mx, a, alen, b, blen, npairs, gap_init, gap_ext, out, cigar, cigar_cap, cigar_used);
    if (align_check("sw_align_matrix_cpu_mode", mx, a, alen, b, blen, npairs, gap_init, gap_ext, out, cigar, cigar_cap,
                    cigar_used))
        return -1;
    for (int k = 0; k < npairs; ++k) {
        if (!mode_range_ok(alen[k], blen[k], gap_init, gap_ext, "pair", k)) return -1;
        if ((long long)alen[k] * blen[k] > CPU_MAX_CELLS) {
            char m[160];
            std::snprintf(m, sizeof m, "pair %d: %lld cells are more than the CPU aligner's full matrix holds (2^32)", k,
                          (long long)alen[k] * blen[k]);
            report_error(m);
            return -1;
        }
    }
    AlignSink sink{out, {}};
    std::vector<unsigned char> cell, ops;
    std::vector<int> hup, fup;
    for (int k = 0; k < npairs; ++k) {
        if (alen[k] == 0 || blen[k] == 0) align_mode_empty(sink, k, alen[k], blen[k], gap_init, gap_ext, mode);
        else align_pair_mode(MatrixScore{mx, a[k]}, mx->code, alen[k], b[k], blen[k], gap_init, gap_ext, mode, cell, hup, fup, ops, k,
                             sink);
    }
    return sink.finish(cigar, cigar_cap, cigar_used);
}

int sw_align_matrix_cpu_band(const sw_matrix* mx, const unsigned char* const* a, const int* alen,
                             const unsigned char* const* b, const int* blen, int npairs, int gap_init, int gap_ext, int mode,
                             int band, sw_alignment* out, unsigned* cigar, long long cigar_cap, long long* cigar_used) {
    if (!mode_ok("sw_align_matrix_cpu_band", mode) || !band_ok("sw_align_matrix_cpu_band", band)) return -1;
    if (align_check("sw_align_matrix_cpu_band", mx, a, alen, b, blen, npairs, gap_init, gap_ext, out, cigar, cigar_cap,
                    cigar_used))
        return -1;
    for (int k = 0; k < npairs; ++k) {
        if (mode != SW_MODE_LOCAL && !mode_range_ok(alen[k], blen[k], gap_init, gap_ext, "pair", k)) return -1;
        if ((long long)alen[k] * blen[k] > CPU_MAX_CELLS) {
            char m[160];
            std::snprintf(m, sizeof m, "pair %d: %lld cells are more than the CPU aligner's full matrix holds (2^32)", k,
                          (long long)alen[k] * blen[k]);
            report_error(m);
            return -1;
        }
    }
    AlignSink sink{out, {}};
    std::vector<unsigned char> cell, ops;
    std::vector<int> hup, fup;
    for (int k = 0; k < npairs; ++k) {
        if (alen[k] == 0 || blen[k] == 0) {
            if (mode != SW_MODE_LOCAL) align_mode_empty(sink, k, alen[k], blen[k], gap_init, gap_ext, mode);
            else sink.set_empty(k);
            continue;
        }
        int dlo, dhi;
        band_range(alen[k], blen[k], band, &dlo, &dhi);
        align_pair_band(mx, a[k], alen[k], b[k], blen[k], gap_init, gap_ext, mode, dlo, dhi, cell, hup, fup, ops, k, sink);
    }
    return sink.finish(cigar, cigar_cap, cigar_used);
}

int sw_align_profile_cpu(const sw_profile* pf, const unsigned char* const* seqs, const int* lens, int nseq, int gap_init,
                         int gap_ext, int mode, sw_alignment* out, unsigned* cigar, long long cigar_cap, long long* cigar_used) {
    if (profile_align_check("sw_align_profile_cpu", pf, seqs, lens, nseq, gap_init, gap_ext, mode, out, cigar, cigar_cap,
                            cigar_used))
        return -1;
    for (int k = 0; k < nseq; ++k)
        if ((long long)pf->n * lens[k] > CPU_MAX_CELLS) {
            char m[160];
            std::snprintf(m, sizeof m, "sequence %d: %lld cells are more than the CPU aligner's full matrix holds (2^32)", k,
                          (long long)pf->n * lens[k]);
            report_error(m);
            return -1;
        }
    AlignSink sink{out, {}};
    std::vector<unsigned char> cell, ops;
    std::vector<int> hup, fup;
    const ProfileScore s{pf};
    for (int k = 0; k < nseq; ++k) {
        if (lens[k] == 0) {
            if (mode != SW_MODE_LOCAL) align_mode_empty(sink, k, pf->n, 0, gap_init, gap_ext, mode);
            else sink.set_empty(k);
        } else if (mode == SW_MODE_LOCAL) {
            align_pair(s, pf->alpha.code, pf->n, seqs[k], lens[k], gap_init, gap_ext, cell, hup, fup, ops, k, sink);
        } else {
            align_pair_mode(s, pf->alpha.code, pf->n, seqs[k], lens[k], gap_init, gap_ext, mode, cell, hup, fup, ops, k, sink);
        }
    }
    return sink.finish(cigar, cigar_cap, cigar_used);
}

int sw_align_matrix_translated_cpu(const sw_matrix* mx, const unsigned char* const* a, const int* alen,
                                   const unsigned char* const* dna, const int* dlen, const int* frames, int npairs,
                                   int gap_init, int gap_ext, int mode, const unsigned char* code64, sw_alignment* out,
                                   unsigned* cigar, long long cigar_cap, long long* cigar_used) {
    const char* fn = "sw_align_matrix_translated_cpu";
    if (cigar_cap < 0 || !cigar_used || (cigar_cap > 0 && !cigar) || (npairs > 0 && (!out || !frames))) {
        report_error("sw_align_matrix_translated_cpu: invalid arguments (a null pointer)");
        return -1;
    }
    Translated xl;
    if (translated_check(fn, mx, a, alen, dna, dlen, frames, npairs, gap_init, gap_ext, mode, code64, &xl)) return -1;
    // sw_translate, then the aligner of the matrix path over the frames' residues
    std::vector<std::vector<unsigned char>> prot((size_t)npairs);
    std::vector<const unsigned char*> bp((size_t)npairs);
    std::vector<int> bl((size_t)npairs);
    for (int k = 0; k < npairs; ++k) {
        std::vector<unsigned char>& p = prot[(size_t)k];
        p.resize((size_t)dlen[k] / 3 + 1);
        const int m = sw_translate(dna[k], dlen[k], frames[k], code64, p.data(), (int)p.size());
        if (m < 0) return -1;
        bp[(size_t)k] = p.data();
        bl[(size_t)k] = m;
    }
    return sw_align_matrix_cpu_mode(mx, a, alen, bp.data(), bl.data(), npairs, gap_init, gap_ext, mode, out, cigar, cigar_cap,
                                    cigar_used);
}

int sw_band_plan(int n, int m, int band, sw_band_plan_t* out) {
    if (n < 0 || m < 0 || n > ALIGN_MAX_SEQ || m > ALIGN_MAX_SEQ || !out) {
        report_error("sw_band_plan: invalid arguments");
        return -1;
    }
    if (!band_ok("sw_band_plan", band)) return -1;
    sw_band_plan_t p{0, 0, 0, 0, 0};
    p.dlo = std::min<long long>(0, (long long)m - n) - band;
    p.dhi = std::max<long long>(0, (long long)m - n) + band;
    if (n > 0 && m > 0) {
        int dlo, dhi;
        band_range(n, m, band, &dlo, &dhi);
        p.cells = band_cells(n, m, dlo, dhi);
        p.trace_bytes = band_trace_bytes(n, m, dlo, dhi);
        p.full_trace_bytes = align_strips(n) * align_strip_trace_bytes(m);
    }
    *out = p;
    return 0;
}

}  // extern "C"
