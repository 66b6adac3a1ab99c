// sw_matrix_host.cpp -- substitution matrices, host only (no HIP): creation from a table, the
// NCBI text format, the byte-to-code map the kernel uses (sw_matrix.hip stages this very array)
// and the accessors of include/algoGPU.h.  No named matrix is compiled in: users pass a file.
// And profiles (sw_profile_*): n positions over a matrix object's alphabet, their text format and the device image.
#include "sw_matrix_host.h"
#include "../../include/algoGPU.h"

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace swmi {
namespace {

std::atomic<unsigned long long> g_next_id{1};

sw_matrix* fail(const char* fmt, long long a = 0, long long b = 0) {
    char m[200];
    std::snprintf(m, sizeof m, fmt, a, b);
    report_error(m);
    return nullptr;
}

sw_matrix* make(const unsigned char* symbols, int k, const signed char* scores, int other, int flags) {
    if (k < 1 || k > SW_MATRIX_MAX_K) return fail("matrix: %lld symbols (need 1 to 32)", k);
    if (!symbols || !scores) return fail("matrix: null table");
    if (other < -1 || other >= k) return fail("matrix: 'other' index %lld is not a symbol index or -1", other);
    if (flags & ~SW_MATRIX_FOLD_CASE) return fail("matrix: unknown flags %lld", flags);
    bool seen[256] = {};
    for (int i = 0; i < k; ++i) {
        if (seen[symbols[i]]) return fail("matrix: duplicate symbol 0x%02llx", symbols[i]);
        seen[symbols[i]] = true;
    }
    for (int i = 0; i < k * k; ++i)
        if (scores[i] < -127) return fail("matrix: entry %lld is outside [-127, 127]", scores[i]);
    sw_matrix* m = new sw_matrix();
    m->k = k;
    m->other = other;
    m->flags = flags;
    std::memcpy(m->sym, symbols, (size_t)k);
    std::memcpy(m->sc, scores, (size_t)k * (size_t)k);
    for (int i = 0; i < k * k; ++i) m->max_entry = scores[i] > m->max_entry ? scores[i] : m->max_entry;
    for (int b = 0; b < 256; ++b) m->code[b] = (unsigned char)(other >= 0 ? other : SW_MATRIX_NOCODE);
    if (flags & SW_MATRIX_FOLD_CASE)   // a-z as A-Z, wherever the lower-case byte is not itself a symbol
        for (int i = 0; i < k; ++i)
            if (symbols[i] >= 'A' && symbols[i] <= 'Z' && !seen[symbols[i] + 32]) m->code[symbols[i] + 32] = (unsigned char)i;
    for (int i = 0; i < k; ++i) m->code[symbols[i]] = (unsigned char)i;
    m->id = g_next_id.fetch_add(1);
    return m;
}

bool blank(char c) { return c == ' ' || c == '\t' || c == '\r' || c == '\v' || c == '\f'; }

// the blank-separated tokens of one line
void split(const char* p, const char* end, std::vector<std::string>& out) {
    out.clear();
    while (p < end) {
        while (p < end && blank(*p)) ++p;
        const char* q = p;
        while (q < end && !blank(*q)) ++q;
        if (q > p) out.emplace_back(p, q);
        p = q;
    }
}

// a decimal integer with an optional sign; false if the token is anything else
bool to_int(const std::string& t, long long* v) {
    size_t i = (t[0] == '-' || t[0] == '+') ? 1 : 0;
    if (i >= t.size() || t.size() - i > 9) return false;
    long long x = 0;
    for (; i < t.size(); ++i) {
        if (t[i] < '0' || t[i] > '9') return false;
        x = x * 10 + (t[i] - '0');
    }
    *v = t[0] == '-' ? -x : x;
    return true;
}

sw_matrix* parse(const char* text, size_t nbytes) {
    std::vector<std::string> tok;
    unsigned char sym[SW_MATRIX_MAX_K];
    signed char sc[SW_MATRIX_MAX_K * SW_MATRIX_MAX_K];
    int k = 0, rows = 0, other = -1, line_no = 0;
    const char* p = text;
    const char* const end = text + nbytes;
    while (p < end) {
        const char* e = (const char*)std::memchr(p, '\n', (size_t)(end - p));
        if (!e) e = end;
        ++line_no;
        split(p, e, tok);
        p = e < end ? e + 1 : end;
        if (tok.empty() || tok[0][0] == '#') continue;
        if (k == 0) {   // the header: one symbol per token
            if (tok.size() > (size_t)SW_MATRIX_MAX_K) return fail("matrix file: %lld symbols (at most 32)", (long long)tok.size());
            for (const std::string& t : tok) {
                if (t.size() != 1) return fail("matrix file line %lld: a symbol must be one byte", line_no);
                for (int i = 0; i < k; ++i)
                    if (sym[i] == (unsigned char)t[0]) return fail("matrix file: duplicate symbol 0x%02llx", (unsigned char)t[0]);
                if (t[0] == '*') other = k;
                sym[k++] = (unsigned char)t[0];
            }
            continue;
        }
        if (rows >= k) return fail("matrix file line %lld: more rows than the %lld symbols of the header (not square)", line_no, k);
        if (tok[0].size() != 1 || (unsigned char)tok[0][0] != sym[rows])
            return fail("matrix file line %lld: the row label disagrees with symbol %lld of the header", line_no, rows);
        if (tok.size() != (size_t)k + 1)
            return fail("matrix file line %lld: %lld entries in the row (not square)", line_no, (long long)tok.size() - 1);
        for (int j = 0; j < k; ++j) {
            long long v = 0;
            if (!to_int(tok[(size_t)j + 1], &v)) return fail("matrix file line %lld: entry %lld is not an integer", line_no, j);
            if (v < -127 || v > 127) return fail("matrix file line %lld: entry %lld is outside [-127, 127]", line_no, v);
            sc[rows * k + j] = (signed char)v;
        }
        ++rows;
    }
    if (k == 0) return fail("matrix file: no header line and no rows");
    if (rows == 0) return fail("matrix file: no rows at all");
    if (rows != k) return fail("matrix file: %lld rows for %lld symbols (not square)", rows, k);
    return make(sym, k, sc, other, 0);
}

// ---- profiles: n positions over a matrix object's alphabet ----

sw_profile* pfail(const char* fmt, long long a = 0, long long b = 0) {
    fail(fmt, a, b);
    return nullptr;
}

// scores: n * k entries, row-major by position (long long: the parser's values, checked here)
template <class T>
sw_profile* make_profile(const unsigned char* symbols, int k, const T* scores, long long n, int other, int flags) {
    if (k < 1 || k > SW_MATRIX_MAX_K) return pfail("profile: %lld symbols (need 1 to 32)", k);
    if (n < 1) return pfail("profile: %lld positions (need at least 1)", n);
    if (n > SW_PROFILE_MAX_N) return pfail("profile: %lld positions are more than SW_PROFILE_MAX_LENGTH = %lld", n, SW_PROFILE_MAX_N);
    if (!symbols || !scores) return pfail("profile: null table");
    for (long long i = 0; i < n * k; ++i)
        if (scores[i] < -127 || scores[i] > 127)
            return pfail("profile: position %lld: entry %lld is outside [-127, 127]", i / k, (long long)scores[i]);
    // the alphabet is a matrix object's: its checks (duplicates, other, flags), its byte-to-code map, an id
    const signed char none[SW_MATRIX_MAX_K * SW_MATRIX_MAX_K] = {};
    sw_matrix* al = make(symbols, k, none, other, flags);
    if (!al) return nullptr;
    sw_profile* p = new sw_profile();
    p->alpha = *al;
    delete al;
    p->n = (int)n;
    p->sc.resize((size_t)n * (size_t)k);
    p->image.assign(((size_t)n + 1) * SW_PROFILE_STRIDE, 0);
    for (long long i = 0; i <= n; ++i) {
        signed char* row = p->image.data() + (size_t)i * SW_PROFILE_STRIDE;
        for (int c = 0; c < k && i < n; ++c) {
            const signed char v = (signed char)scores[i * k + c];
            p->sc[(size_t)(i * k + c)] = v;
            row[c] = v;
            p->alpha.max_entry = v > p->alpha.max_entry ? v : p->alpha.max_entry;
        }
        row[k] = (signed char)SW_PROFILE_SENT;
    }
    return p;
}

// The profile text format (include/algoGPU.h): '#' comment lines, a header line of K symbols, then one row
// a position: a one-byte label (the consensus residue, not read) and K integers.
sw_profile* parse_profile(const char* text, size_t nbytes) {
    std::vector<std::string> tok;
    unsigned char sym[SW_MATRIX_MAX_K];
    std::vector<long long> sc;
    int k = 0, other = -1, line_no = 0;
    long long rows = 0;
    const char* p = text;
    const char* const end = text + nbytes;
    while (p < end) {
        const char* e = (const char*)std::memchr(p, '\n', (size_t)(end - p));
        if (!e) e = end;
        ++line_no;
        split(p, e, tok);
        p = e < end ? e + 1 : end;
        if (tok.empty() || tok[0][0] == '#') continue;   // (so '#' cannot label a row)
        if (k == 0) {   // the header: one symbol per token
            if (tok.size() > (size_t)SW_MATRIX_MAX_K) return pfail("profile file: %lld symbols (at most 32)", (long long)tok.size());
            for (const std::string& t : tok) {
                if (t.size() != 1) return pfail("profile file line %lld: a symbol must be one byte", line_no);
                for (int i = 0; i < k; ++i)
                    if (sym[i] == (unsigned char)t[0]) return pfail("profile file: duplicate symbol 0x%02llx", (unsigned char)t[0]);
                if (t[0] == '*') other = k;
                sym[k++] = (unsigned char)t[0];
            }
            continue;
        }
        if (rows >= SW_PROFILE_MAX_N)
            return pfail("profile file line %lld: more than SW_PROFILE_MAX_LENGTH = %lld positions", line_no, SW_PROFILE_MAX_N);
        if (tok[0].size() != 1) return pfail("profile file line %lld: the row label must be one byte", line_no);
        if (tok.size() != (size_t)k + 1)
            return pfail("profile file line %lld: %lld entries in the row, not one a symbol", line_no, (long long)tok.size() - 1);
        for (int j = 0; j < k; ++j) {
            long long v = 0;
            if (!to_int(tok[(size_t)j + 1], &v)) return pfail("profile file line %lld: entry %lld is not an integer", line_no, j);
            if (v < -127 || v > 127) return pfail("profile file line %lld: entry %lld is outside [-127, 127]", line_no, v);
            sc.push_back(v);
        }
        ++rows;
    }
    if (k == 0) return pfail("profile file: no header line and no rows");
    if (rows == 0) return pfail("profile file: no rows at all");
    return make_profile(sym, k, sc.data(), rows, other, 0);
}

}  // namespace

long long matrix_first_bad(const sw_matrix* m, const unsigned char* p, long long len) {
    if (m->other >= 0) return -1;
    for (long long i = 0; i < len; ++i)
        if (m->code[p[i]] == SW_MATRIX_NOCODE) return i;
    return -1;
}

// ---- translated search: bases, frames and the composed tables (include/algoGPU.h; sw_matrix_host.h) ----

namespace {
const char STANDARD_CODE[65] = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG";

int base_class(unsigned char b) {
    switch (b) {
    case 'T': case 't': case 'U': case 'u': return 0;
    case 'C': case 'c': return 1;
    case 'A': case 'a': return 2;
    case 'G': case 'g': return 3;
    default: return XL_AMBIGUOUS;
    }
}
}  // namespace

int frame_index(int frame) { return frame >= 1 && frame <= 3 ? frame - 1 : frame <= -1 && frame >= -3 ? 2 - frame : -1; }

int frame_residues(int len, int fi) {
    const int o = fi % 3;
    return len >= o + 3 ? (len - o) / 3 : 0;
}

int frame_region(int len, int fi) {
    const int o = fi % 3;
    return fi < 3 ? o : len - o - 3 * frame_residues(len, fi);
}

int translated_tables(const char* fn, const sw_matrix* mx, const unsigned char* code64, Translated* out) {
    const unsigned char* code = code64 ? code64 : reinterpret_cast<const unsigned char*>(STANDARD_CODE);
    for (int b = 0; b < 256; ++b) out->base[b] = (unsigned char)base_class((unsigned char)b);
    std::memset(out->codon, 0, sizeof out->codon);
    for (int c = 0; c <= 64; ++c) {
        const unsigned char aa = c < 64 ? code[c] : (unsigned char)'X';
        if (mx->code[aa] == SW_MATRIX_NOCODE) {
            char m[200];
            if (c < 64)
                std::snprintf(m, sizeof m, "%s: the genetic code emits byte 0x%02x ('%c', codon %d), which the matrix does not score",
                              fn, aa, aa >= 32 && aa < 127 ? aa : '?', c);
            else
                std::snprintf(m, sizeof m, "%s: a codon with an ambiguous base translates to byte 0x58 ('X'), which the matrix "
                              "does not score", fn);
            report_error(m);
            return -1;
        }
        out->codon[c] = mx->code[aa];
    }
    return 0;
}

}  // namespace swmi

using namespace swmi;

extern "C" {

sw_matrix* sw_matrix_create(const unsigned char* symbols, int k, const signed char* scores, int other, int flags) {
    return make(symbols, k, scores, other, flags);
}

sw_matrix* sw_matrix_parse(const char* text, long long nbytes) {
    if (nbytes < 0 || (nbytes > 0 && !text)) return fail("sw_matrix_parse: invalid arguments");
    return parse(text, (size_t)nbytes);
}

sw_matrix* sw_matrix_open(const char* path) {
    if (!path) return fail("sw_matrix_open: null path");
    std::FILE* f = std::fopen(path, "rb");
    if (!f) {
        const std::string msg = std::string("cannot open matrix file ") + path;
        report_error(msg.c_str());
        return nullptr;
    }
    std::vector<char> buf;
    char chunk[4096];
    size_t got = 0;
    while ((got = std::fread(chunk, 1, sizeof chunk, f)) > 0) {
        buf.insert(buf.end(), chunk, chunk + got);
        if (buf.size() > (1u << 20)) break;   // 32 rows of 32 entries: anything larger is not a matrix
    }
    std::fclose(f);
    if (buf.size() > (1u << 20)) return fail("matrix file: larger than 1 MiB");
    return parse(buf.data(), buf.size());
}

int sw_matrix_size(const sw_matrix* m) { return m ? m->k : -1; }

int sw_matrix_symbols(const sw_matrix* m, unsigned char* out) {
    if (!m || !out) {
        report_error("sw_matrix_symbols: invalid arguments");
        return -1;
    }
    std::memcpy(out, m->sym, (size_t)m->k);
    return m->k;
}

int sw_matrix_score(const sw_matrix* m, unsigned char a, unsigned char b, int* out) {
    if (!m || !out) {
        report_error("sw_matrix_score: invalid arguments");
        return -1;
    }
    const int ca = m->code[a], cb = m->code[b];
    if (ca == SW_MATRIX_NOCODE || cb == SW_MATRIX_NOCODE) {
        char msg[96];
        std::snprintf(msg, sizeof msg, "byte 0x%02x is outside the matrix alphabet", ca == SW_MATRIX_NOCODE ? a : b);
        report_error(msg);
        return -1;
    }
    *out = m->sc[ca * m->k + cb];
    return 0;
}

void sw_matrix_free(sw_matrix* m) { delete m; }

sw_profile* sw_profile_create(const unsigned char* symbols, int k, const signed char* scores, int n, int other, int flags) {
    return make_profile(symbols, k, scores, n, other, flags);
}

sw_profile* sw_profile_from_matrix(const sw_matrix* mx, const unsigned char* query, int qlen) {
    if (!mx || qlen < 0 || (qlen > 0 && !query)) return pfail("sw_profile_from_matrix: invalid arguments");
    if (qlen < 1) return pfail("profile: %lld positions (need at least 1)", qlen);
    if (qlen > SW_PROFILE_MAX_N) return pfail("profile: %lld positions are more than SW_PROFILE_MAX_LENGTH = %lld", qlen, SW_PROFILE_MAX_N);
    std::vector<signed char> sc((size_t)qlen * (size_t)mx->k);
    for (int i = 0; i < qlen; ++i) {
        const int c = mx->code[query[i]];
        if (c == SW_MATRIX_NOCODE) return pfail("query position %lld: byte 0x%02llx is outside the matrix alphabet", i, query[i]);
        std::memcpy(sc.data() + (size_t)i * (size_t)mx->k, mx->sc + c * mx->k, (size_t)mx->k);
    }
    return make_profile(mx->sym, mx->k, sc.data(), qlen, mx->other, mx->flags);
}

sw_profile* sw_profile_parse(const char* text, long long nbytes) {
    if (nbytes < 0 || (nbytes > 0 && !text)) return pfail("sw_profile_parse: invalid arguments");
    return parse_profile(text, (size_t)nbytes);
}

sw_profile* sw_profile_open(const char* path) {
    if (!path) return pfail("sw_profile_open: null path");
    std::FILE* f = std::fopen(path, "rb");
    if (!f) {
        const std::string msg = std::string("cannot open profile file ") + path;
        report_error(msg.c_str());
        return nullptr;
    }
    constexpr size_t LIMIT = (size_t)1 << 30;   // SW_PROFILE_MAX_LENGTH rows of 32 entries fit; anything larger is refused
    std::vector<char> buf;
    char chunk[65536];
    size_t got = 0;
    while ((got = std::fread(chunk, 1, sizeof chunk, f)) > 0) {
        buf.insert(buf.end(), chunk, chunk + got);
        if (buf.size() > LIMIT) break;
    }
    std::fclose(f);
    if (buf.size() > LIMIT) return pfail("profile file: larger than 1 GiB");
    return parse_profile(buf.data(), buf.size());
}

int sw_profile_length(const sw_profile* p) { return p ? p->n : -1; }

int sw_profile_size(const sw_profile* p) { return p ? p->alpha.k : -1; }

int sw_profile_symbols(const sw_profile* p, unsigned char* out) {
    if (!p || !out) {
        report_error("sw_profile_symbols: invalid arguments");
        return -1;
    }
    std::memcpy(out, p->alpha.sym, (size_t)p->alpha.k);
    return p->alpha.k;
}

int sw_profile_score(const sw_profile* p, int pos, unsigned char byte, int* out) {
    if (!p || !out) {
        report_error("sw_profile_score: invalid arguments");
        return -1;
    }
    char msg[96];
    if (pos < 0 || pos >= p->n) {
        std::snprintf(msg, sizeof msg, "position %d is outside the profile's [0, %d)", pos, p->n);
        report_error(msg);
        return -1;
    }
    const int c = p->alpha.code[byte];
    if (c == SW_MATRIX_NOCODE) {
        std::snprintf(msg, sizeof msg, "byte 0x%02x is outside the profile alphabet", byte);
        report_error(msg);
        return -1;
    }
    *out = p->sc[(size_t)pos * (size_t)p->alpha.k + (size_t)c];
    return 0;
}

void sw_profile_free(sw_profile* p) { delete p; }

void sw_standard_code(unsigned char out[64]) {
    if (out) std::memcpy(out, STANDARD_CODE, 64);
}

int sw_translate(const unsigned char* dna, int len, int frame, const unsigned char* code64, unsigned char* out, int cap) {
    const int fi = frame_index(frame);
    char msg[160];
    if (fi < 0) {
        std::snprintf(msg, sizeof msg, "sw_translate: frame %d is not one of +1, +2, +3, -1, -2, -3", frame);
        report_error(msg);
        return -1;
    }
    if (len < 0 || cap < 0 || (len > 0 && !dna)) {
        report_error("sw_translate: invalid arguments");
        return -1;
    }
    const int m = frame_residues(len, fi), o = fi % 3;
    if (m > cap || (m > 0 && !out)) {
        std::snprintf(msg, sizeof msg, "sw_translate: %d residues do not fit the output buffer of %d", m, cap);
        report_error(msg);
        return -1;
    }
    const unsigned char* code = code64 ? code64 : reinterpret_cast<const unsigned char*>(STANDARD_CODE);
    for (int r = 0; r < m; ++r) {
        int c[3];
        for (int t = 0; t < 3; ++t)
            c[t] = fi < 3 ? base_class(dna[3 * r + o + t]) : base_class(dna[len - 1 - 3 * r - o - t]) ^ 2;
        out[r] = ((c[0] | c[1] | c[2]) & XL_AMBIGUOUS) ? (unsigned char)'X' : code[16 * c[0] + 4 * c[1] + c[2]];
    }
    return m;
}

int sw_translated_range(int len, int frame, int beg2, int end2, int* dna_beg, int* dna_end) {
    const int fi = frame_index(frame);
    char msg[200];
    if (fi < 0) {
        std::snprintf(msg, sizeof msg, "sw_translated_range: frame %d is not one of +1, +2, +3, -1, -2, -3", frame);
        report_error(msg);
        return -1;
    }
    if (len < 0 || !dna_beg || !dna_end) {
        report_error("sw_translated_range: invalid arguments");
        return -1;
    }
    const int m = frame_residues(len, fi), o = fi % 3;
    if (beg2 < 0 || beg2 > end2 || end2 > m) {
        std::snprintf(msg, sizeof msg, "sw_translated_range: residues [%d, %d) are outside frame %d of %d bases (%d residues)",
                      beg2, end2, frame, len, m);
        report_error(msg);
        return -1;
    }
    // (a DNA shorter than the offset has an empty frame, whose empty range is kept inside [0, len])
    const int lo = fi < 3 ? 3 * beg2 + o : len - o - 3 * end2, hi = fi < 3 ? 3 * end2 + o : len - o - 3 * beg2;
    *dna_beg = std::min(std::max(lo, 0), len);
    *dna_end = std::min(std::max(hi, 0), len);
    return 0;
}

int sw_translated_tables(const sw_matrix* mx, const unsigned char* code64, unsigned char base_out[256],
                         unsigned char codon_out[65]) {
    if (!mx || !base_out || !codon_out) {
        report_error("sw_translated_tables: invalid arguments");
        return -1;
    }
    Translated t;
    if (translated_tables("sw_translated_tables", mx, code64, &t)) return -1;
    std::memcpy(base_out, t.base, 256);
    std::memcpy(codon_out, t.codon, 65);
    return 0;
}

}  // extern "C"
