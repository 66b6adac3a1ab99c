// sw_db.hip -- FASTA databases and query x database scoring.
//
// The reference reaches databases only through the external CUDASW++4 tool
// (timing.sh:3-8: `makedb SwissProt.fasta benchdb/sp`, then
// `align --query q.fa --db benchdb/sp`; Makefile_CUDASW4.mak:44-56), which is
// not vendored.  This module gives the same workflow over this engine: the
// FASTA parse and the binary database file (host only, sw_db_host.cpp), and
// searches that score one query against every record with ONE batch launch
// (sw_score_batch_device) over residues kept resident in HBM.  Scoring is the reference's (byte equality + affine
// gaps, main.cpp:28-66), so every score equals SmithWatermanScore of the pair.
//
// Layout: all records' residues back to back in one arena (host, and once per
// device), the query in a tail slot of the device arena behind them.  Records
// are launched longest first (the work-claiming kernels take pairs in order, so
// the long tail starts early); scores come back in record order.
#include "sw_internal.h"
#include "sw_db_host.h"
#include "sw_matrix_host.h"
#include "../../include/algoGPU.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <numeric>
#include <string>
#include <vector>

namespace swmi {
namespace {

#define DBCHK(expr)                                                                          \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) {                                                              \
            char m_[256];                                                                    \
            std::snprintf(m_, sizeof m_, "%s failed: %s", #expr, hipGetErrorString(e_));     \
            report_error(m_);                                                                \
            return -1;                                                                       \
        }                                                                                    \
    } while (0)

// the database's device arena on the current device, with two query slots of at least qlen
// bytes behind the residues and two score buffers (sw_db_search_db alternates them).  A new
// arena is built in locals and committed to the Dev entry only when every step succeeded (a
// failed copy must not leave an arena that looks ready).
int device_arena(sw_db* db, int qlen, sw_db::Dev** out) {
    int d = 0;
    DBCHK(hipGetDevice(&d));
    sw_db::Dev& v = db->dev[d];
    if (!v.arena || v.qcap < (size_t)qlen) {
        if (v.arena) DBCHK(hipFree(v.arena));
        if (v.scores) DBCHK(hipFree(v.scores));
        v.arena = nullptr;
        v.scores = nullptr;
        v.qcap = 0;
        const size_t qcap = (std::max<size_t>((size_t)qlen + (size_t)qlen / 4, 4096) + 15) / 16 * 16;
        unsigned char* arena = nullptr;
        int* scores = nullptr;
        hipError_t e = hipMalloc((void**)&arena, db->res.size() + 2 * qcap);
        if (e == hipSuccess) e = hipMalloc((void**)&scores, 2 * std::max<size_t>(db->len.size(), 1) * sizeof(int));
        if (e == hipSuccess && !db->res.empty())
            e = hipMemcpy(arena, db->res.data(), db->res.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            if (arena) (void)hipFree(arena);
            if (scores) (void)hipFree(scores);
            char m[256];
            std::snprintf(m, sizeof m, "database device arena: %s", hipGetErrorString(e));
            report_error(m);
            return -1;
        }
        v.arena = arena;
        v.scores = scores;
        v.qcap = qcap;
    }
    *out = &v;
    return 0;
}

bool all_dna(const unsigned char* p, size_t n) {
    unsigned bad = 0;
    for (size_t i = 0; i < n; ++i) bad |= !(p[i] == 'A' || p[i] == 'C' || p[i] == 'G' || p[i] == 'T');
    return bad == 0;
}

// the engine's int32 score range, checked here so an error names the record
int check_range(const sw_db* db, int qlen) {
    int match = 1;
    sw_get_params(&match, nullptr, nullptr, nullptr);
    for (size_t r = 0; r < db->len.size(); ++r) {
        if ((long long)std::min(qlen, db->len[r]) * std::max(match, 1) >= (1LL << 28)) {
            char m[160];
            std::snprintf(m, sizeof m, "record %d: score range exceeds the int32 engine (min length * MATCH >= 2^28)", (int)r);
            report_error(m);
            return -1;
        }
    }
    return 0;
}

// the alphabet the engine would scan for on the device (its alphabet_kernel), known on the host:
// the records' once per database, the query's per search
int search_flags(sw_db* db, const unsigned char* query, int qlen) {
    if (db->dna < 0) db->dna = all_dna(db->res.data(), db->res.size()) ? 1 : 0;
    return db->dna == 1 && all_dna(query, (size_t)qlen) ? SW_FLAG_DNA : SW_FLAG_BYTES;
}

// Launch one query's search on `stream` (null: synchronous) into score buffer / query slot `slot`;
// records are launched longest first (b_off / blen in db->order)
int launch_query(sw_db* db, sw_db::Dev* v, const unsigned char* query, int qlen, int slot, hipStream_t stream,
                 const std::vector<int64_t>& b_off, const std::vector<int>& blen) {
    const int nrec = (int)db->len.size();
    const int64_t qoff = (int64_t)db->res.size() + (int64_t)slot * (int64_t)v->qcap;
    if (qlen > 0) {
        if (stream) DBCHK(hipMemcpyAsync(v->arena + qoff, query, (size_t)qlen, hipMemcpyHostToDevice, stream));
        else DBCHK(hipMemcpy(v->arena + qoff, query, (size_t)qlen, hipMemcpyHostToDevice));
    }
    std::vector<int64_t> a_off((size_t)nrec, qoff);
    std::vector<int> alen((size_t)nrec, qlen);
    return sw_score_batch_device(v->arena, a_off.data(), alen.data(), b_off.data(), blen.data(), nrec,
                                 v->scores + (size_t)slot * (size_t)nrec, search_flags(db, query, qlen), stream);
}

void record_order(const sw_db* db, std::vector<int64_t>& b_off, std::vector<int>& blen) {
    const size_t nrec = db->len.size();
    b_off.resize(nrec);
    blen.resize(nrec);
    for (size_t k = 0; k < nrec; ++k) {   // slot k scores record order[k]
        const int r = db->order[k];
        b_off[k] = db->off[r];
        blen[k] = db->len[r];
    }
}

// qslot: room to reserve for the query (>= qlen)
int search(sw_db* db, const unsigned char* query, int qlen, int* scores_out, int qslot) {
    const int nrec = (int)db->len.size();
    if (nrec == 0) return 0;
    if (check_range(db, qlen)) return -1;
    sw_db::Dev* v = nullptr;
    if (device_arena(db, std::max(qlen, qslot), &v)) return -1;
    std::vector<int64_t> b_off;
    std::vector<int> blen;
    record_order(db, b_off, blen);
    if (launch_query(db, v, query, qlen, 0, nullptr, b_off, blen)) return -1;
    std::vector<int> got((size_t)nrec);
    DBCHK(hipMemcpy(got.data(), v->scores, (size_t)nrec * sizeof(int), hipMemcpyDeviceToHost));
    for (int k = 0; k < nrec; ++k) scores_out[db->order[k]] = got[k];
    return 0;
}

// Every query of `queries` against the database, pipelined on the database's own stream: query q
// is planned and launched into slot q % 2 (its query slot, score buffer and pinned host copy) while
// query q - 1 runs; slot q % 2's scores (query q - 2) are collected first.  The host's per-search
// planning (~1.5 ms for 65536 records) then overlaps the kernels instead of adding to them.
int search_many(sw_db* db, const sw_db* queries, int* scores_out) {
    const int nrec = (int)db->len.size(), nq = (int)queries->len.size();
    if (nrec == 0 || nq == 0) return 0;
    int longest = 0;
    for (int l : queries->len) longest = std::max(longest, l);
    if (check_range(db, longest)) return -1;
    sw_db::Dev* v = nullptr;
    if (device_arena(db, longest, &v)) return -1;
    if (!v->stream) {
        hipStream_t st = nullptr;
        DBCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        v->stream = st;
    }
    for (int k = 0; k < 2; ++k)
        if (!v->done[k]) {
            hipEvent_t ev = nullptr;
            DBCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            v->done[k] = ev;
        }
    if (!v->hscores) DBCHK(hipHostMalloc((void**)&v->hscores, 2 * (size_t)nrec * sizeof(int), hipHostMallocDefault));
    hipStream_t st = (hipStream_t)v->stream;
    std::vector<int64_t> b_off;
    std::vector<int> blen;
    record_order(db, b_off, blen);
    const auto collect = [&](int q) -> int {   // query q's scores, from its slot's pinned copy
        const int slot = q & 1;
        DBCHK(hipEventSynchronize((hipEvent_t)v->done[slot]));
        const int* got = v->hscores + (size_t)slot * (size_t)nrec;
        int* out = scores_out + (size_t)q * (size_t)nrec;
        for (int k = 0; k < nrec; ++k) out[db->order[k]] = got[k];
        return 0;
    };
    for (int q = 0; q < nq; ++q) {
        const int slot = q & 1;
        if (q >= 2 && collect(q - 2)) return -1;
        if (launch_query(db, v, queries->res.data() + queries->off[q], queries->len[q], slot, st, b_off, blen)) return -1;
        DBCHK(hipMemcpyAsync(v->hscores + (size_t)slot * (size_t)nrec, v->scores + (size_t)slot * (size_t)nrec,
                             (size_t)nrec * sizeof(int), hipMemcpyDeviceToHost, st));
        DBCHK(hipEventRecord((hipEvent_t)v->done[slot], st));
    }
    for (int q = std::max(0, nq - 2); q < nq; ++q)
        if (collect(q)) return -1;
    return sw_stream_status(st);   // a kernel's hand-off timeout surfaces here
}

// ---- substitution-matrix searches (sw_matrix.hip's kernel over the same arena and query slot) ----

// every residue of the database has a code in mx: checked once per (database, matrix); a profile's alphabet is
// a matrix object with an id of its own, so once per (database, profile) too (`alphabet` words the message)
int check_records(sw_db* db, const sw_matrix* mx, const char* alphabet = "matrix") {
    if (db->matrix_ok.count(mx->id)) return 0;
    const long long bad = matrix_first_bad(mx, db->res.data(), (long long)db->res.size());
    if (bad >= 0) {
        // the record that holds residue `bad`: the last one whose offset is <= bad and that is not empty
        int rec = 0;
        for (size_t r = 0; r < db->len.size(); ++r)
            if (db->len[r] > 0 && db->off[r] <= bad && bad < db->off[r] + db->len[r]) rec = (int)r;
        char m[160];
        std::snprintf(m, sizeof m, "record %d: position %lld: byte 0x%02x is outside the %s alphabet", rec,
                      bad - (long long)db->off[rec], db->res[(size_t)bad], alphabet);
        report_error(m);
        return -1;
    }
    db->matrix_ok.insert(mx->id);
    return 0;
}

int check_query(const sw_db* db, const sw_matrix* mx, const unsigned char* query, int qlen, int qidx, int amode = SW_MODE_LOCAL,
                int gap_init = 0, int gap_ext = 0) {
    const long long bad = matrix_first_bad(mx, query, qlen);
    if (bad >= 0) {
        char m[160];
        std::snprintf(m, sizeof m, "query %d: position %lld: byte 0x%02x is outside the matrix alphabet", qidx, bad,
                      query[bad]);
        report_error(m);
        return -1;
    }
    for (size_t r = 0; r < db->len.size(); ++r) {
        if (amode != SW_MODE_LOCAL && !mode_range_ok(qlen, db->len[r], gap_init, gap_ext, "record", (int)r)) return -1;
        if ((long long)std::min(qlen, db->len[r]) * mx->max_entry >= (1LL << 28)) {
            char m[160];
            std::snprintf(m, sizeof m, "record %d: score range exceeds the int32 engine (min length * largest entry >= 2^28)", (int)r);
            report_error(m);
            return -1;
        }
    }
    return 0;
}

// the query spread across the lanes against every record, longest first; scores in record order
int search_matrix(sw_db* db, const sw_matrix* mx, const unsigned char* query, int qlen, int gap_init, int gap_ext,
                  int* scores_out, int qslot, int qidx, int amode = SW_MODE_LOCAL) {
    const int nrec = (int)db->len.size();
    if (nrec == 0) return 0;
    if (check_records(db, mx) || check_query(db, mx, query, qlen, qidx, amode, gap_init, gap_ext)) return -1;
    sw_db::Dev* v = nullptr;
    if (device_arena(db, std::max(qlen, qslot), &v)) return -1;
    std::vector<int64_t> b_off;
    std::vector<int> blen;
    record_order(db, b_off, blen);
    const int64_t qoff = (int64_t)db->res.size();
    if (qlen > 0) DBCHK(hipMemcpy(v->arena + qoff, query, (size_t)qlen, hipMemcpyHostToDevice));
    std::vector<int64_t> a_off((size_t)nrec, qoff);
    std::vector<int> alen((size_t)nrec, qlen);
    if (matrix_score_device(mx, v->arena, a_off.data(), alen.data(), b_off.data(), blen.data(), nrec, gap_init, gap_ext,
                            v->scores, true, amode))
        return -1;
    std::vector<int> got((size_t)nrec);
    DBCHK(hipMemcpy(got.data(), v->scores, (size_t)nrec * sizeof(int), hipMemcpyDeviceToHost));
    if (amode != SW_MODE_LOCAL)   // an empty query or record is answered on the host
        for (int k = 0; k < nrec; ++k)
            if (qlen == 0 || blen[(size_t)k] == 0) got[(size_t)k] = mode_empty_score(qlen, blen[(size_t)k], gap_init, gap_ext, amode);
    for (int k = 0; k < nrec; ++k) scores_out[db->order[k]] = got[k];
    return 0;
}

// the query (seq1, across the lanes) aligned with the chosen records, out of the device arena;
// long_pairs: by checkpointed traceback (sw_db_align_matrix_long); coop: on many waves (sw_db_align_matrix_long_coop);
// both in amode through the _mode entry points, whose range refusal comes before any device work
int align_matrix(sw_db* db, const sw_matrix* mx, const unsigned char* query, int qlen, const int* record_idx, int nidx,
                 int gap_init, int gap_ext, AlignSink& sink, bool long_pairs, int amode = SW_MODE_LOCAL, bool coop = false) {
    const int nrec = (int)db->len.size();
    for (int k = 0; k < nidx; ++k)
        if (record_idx[k] < 0 || record_idx[k] >= nrec) {
            char m[160];
            std::snprintf(m, sizeof m, "sw_db_align_matrix%s%s: record index %d (entry %d) is outside [0, %d)",
                          coop ? "_long_coop" : long_pairs ? "_long" : "", long_pairs && amode != SW_MODE_LOCAL ? "_mode" : "",
                          record_idx[k], k, nrec);
            report_error(m);
            return -1;
        }
    if (nidx == 0) return 0;
    if (check_records(db, mx) || check_query(db, mx, query, qlen, 0)) return -1;
    const int64_t qoff = (int64_t)db->res.size();
    std::vector<int64_t> a_off((size_t)nidx, qoff), b_off((size_t)nidx);
    std::vector<int> alen((size_t)nidx, qlen), blen((size_t)nidx);
    for (int k = 0; k < nidx; ++k) {
        b_off[(size_t)k] = db->off[(size_t)record_idx[k]];
        blen[(size_t)k] = db->len[(size_t)record_idx[k]];
    }
    if (long_pairs && align_long_mode_check(coop ? "sw_db_align_matrix_long_coop_mode" : "sw_db_align_matrix_long_mode", amode,
                                            alen.data(), blen.data(), record_idx, nidx, gap_init, gap_ext, "record"))
        return -1;
    sw_db::Dev* v = nullptr;
    if (device_arena(db, qlen, &v)) return -1;
    if (qlen > 0) DBCHK(hipMemcpy(v->arena + qoff, query, (size_t)qlen, hipMemcpyHostToDevice));
    if (long_pairs)
        return matrix_align_long_device(mx, v->arena, a_off.data(), alen.data(), b_off.data(), blen.data(), record_idx, nidx,
                                        gap_init, gap_ext, "record", sink, coop, amode);
    return matrix_align_device(mx, v->arena, a_off.data(), alen.data(), b_off.data(), blen.data(), record_idx, nidx, gap_init,
                               gap_ext, "record", sink, amode);
}

// ---- profile searches (include/algoGPU.h sw_db_*_profile): the profile in the query's place, nothing of it in the arena ----

// the profile (seq1, across the lanes) against every record, longest first; scores in record order
int search_profile(sw_db* db, const sw_profile* pf, int gap_init, int gap_ext, int amode, int* scores_out) {
    const int nrec = (int)db->len.size();
    if (nrec == 0) return 0;
    if (check_records(db, &pf->alpha, "profile")) return -1;
    for (int r = 0; r < nrec; ++r)
        if (!profile_range_ok(pf, db->len[(size_t)r], gap_init, gap_ext, amode, "record", r)) return -1;
    sw_db::Dev* v = nullptr;
    if (device_arena(db, 0, &v)) return -1;
    std::vector<int64_t> b_off;
    std::vector<int> blen;
    record_order(db, b_off, blen);
    if (profile_score_device(pf, v->arena, b_off.data(), blen.data(), nrec, gap_init, gap_ext, v->scores, amode)) return -1;
    std::vector<int> got((size_t)nrec);
    DBCHK(hipMemcpy(got.data(), v->scores, (size_t)nrec * sizeof(int), hipMemcpyDeviceToHost));
    if (amode != SW_MODE_LOCAL)   // an empty record is answered on the host
        for (int k = 0; k < nrec; ++k)
            if (blen[(size_t)k] == 0) got[(size_t)k] = mode_empty_score(pf->n, 0, gap_init, gap_ext, amode);
    for (int k = 0; k < nrec; ++k) scores_out[db->order[k]] = got[k];
    return 0;
}

// the profile aligned with the chosen records, out of the device arena
int align_profile(sw_db* db, const sw_profile* pf, const int* record_idx, int nidx, int gap_init, int gap_ext, int amode,
                  AlignSink& sink) {
    const int nrec = (int)db->len.size();
    for (int k = 0; k < nidx; ++k)
        if (record_idx[k] < 0 || record_idx[k] >= nrec) {
            char m[160];
            std::snprintf(m, sizeof m, "sw_db_align_profile: record index %d (entry %d) is outside [0, %d)", record_idx[k], k, nrec);
            report_error(m);
            return -1;
        }
    if (nidx == 0) return 0;
    if (check_records(db, &pf->alpha, "profile")) return -1;
    std::vector<int64_t> b_off((size_t)nidx);
    std::vector<int> blen((size_t)nidx);
    for (int k = 0; k < nidx; ++k) {
        b_off[(size_t)k] = db->off[(size_t)record_idx[k]];
        blen[(size_t)k] = db->len[(size_t)record_idx[k]];
        if (!profile_range_ok(pf, blen[(size_t)k], gap_init, gap_ext, amode, "record", record_idx[k])) return -1;
    }
    sw_db::Dev* v = nullptr;
    if (device_arena(db, 0, &v)) return -1;
    return profile_align_device(pf, v->arena, b_off.data(), blen.data(), record_idx, nidx, gap_init, gap_ext, "record", sink,
                                amode);
}

// ---- translated searches (include/algoGPU.h sw_db_*_matrix_translated): the records are DNA, the query a protein ----

// the query against the matrix alphabet and, for every record it will meet, the range refusals; the records are
// not checked (any byte is a DNA byte) and matrix_ok is not touched
int check_translated(const char* fn, const sw_db* db, const sw_matrix* mx, const unsigned char* query, int qlen, const int* record_idx,
                     int nidx, int gap_init, int gap_ext, int amode) {
    const long long bad = matrix_first_bad(mx, query, qlen);
    if (bad >= 0) {
        char m[200];
        std::snprintf(m, sizeof m, "%s: query position %lld: byte 0x%02x is outside the matrix alphabet", fn, bad, query[bad]);
        report_error(m);
        return -1;
    }
    const int n = record_idx ? nidx : (int)db->len.size();
    for (int k = 0; k < n; ++k) {
        const int r = record_idx ? record_idx[k] : k;
        if (db->len[(size_t)r] > (1 << 27) - 1 || qlen > (1 << 27) - 1) {
            char m[200];
            std::snprintf(m, sizeof m, "%s: record %d: a length of %d residues / %d bases is outside [0, 2^27 - 1]", fn, r, qlen,
                          db->len[(size_t)r]);
            report_error(m);
            return -1;
        }
        if (!translated_range_ok(fn, mx, qlen, db->len[(size_t)r], gap_init, gap_ext, amode, "record", r)) return -1;
    }
    return 0;
}

int search_translated(sw_db* db, const sw_matrix* mx, const Translated& xl, const unsigned char* query, int qlen, int gap_init,
                      int gap_ext, int amode, int* scores_out) {
    const char* fn = "sw_db_search_matrix_translated";
    const int nrec = (int)db->len.size();
    if (nrec == 0) return 0;
    if (check_translated(fn, db, mx, query, qlen, nullptr, 0, gap_init, gap_ext, amode)) return -1;
    sw_db::Dev* v = nullptr;
    if (device_arena(db, qlen, &v)) return -1;
    const int64_t qoff = (int64_t)db->res.size();
    if (qlen > 0) DBCHK(hipMemcpy(v->arena + qoff, query, (size_t)qlen, hipMemcpyHostToDevice));
    std::vector<int64_t> a_off((size_t)nrec, qoff), d_off((size_t)nrec);
    std::vector<int> alen((size_t)nrec, qlen);
    for (int r = 0; r < nrec; ++r) d_off[(size_t)r] = db->off[(size_t)r];
    return translated_score_device(mx, xl, v->arena, a_off.data(), alen.data(), d_off.data(), db->len.data(), nrec, gap_init,
                                   gap_ext, amode, scores_out);
}

int align_translated(sw_db* db, const sw_matrix* mx, const Translated& xl, const unsigned char* query, int qlen,
                     const int* record_idx, const int* frames, int nidx, int gap_init, int gap_ext, int amode, AlignSink& sink) {
    const char* fn = "sw_db_align_matrix_translated";
    const int nrec = (int)db->len.size();
    char m[200];
    std::vector<int> fidx((size_t)nidx);
    for (int k = 0; k < nidx; ++k) {
        if (record_idx[k] < 0 || record_idx[k] >= nrec) {
            std::snprintf(m, sizeof m, "%s: record index %d (entry %d) is outside [0, %d)", fn, record_idx[k], k, nrec);
            report_error(m);
            return -1;
        }
        if ((fidx[(size_t)k] = frame_index(frames[k])) < 0) {
            std::snprintf(m, sizeof m, "%s: entry %d: frame %d is not one of +1, +2, +3, -1, -2, -3", fn, k, frames[k]);
            report_error(m);
            return -1;
        }
    }
    if (nidx == 0) return 0;
    if (check_translated(fn, db, mx, query, qlen, record_idx, nidx, gap_init, gap_ext, amode)) return -1;
    sw_db::Dev* v = nullptr;
    if (device_arena(db, qlen, &v)) return -1;
    const int64_t qoff = (int64_t)db->res.size();
    if (qlen > 0) DBCHK(hipMemcpy(v->arena + qoff, query, (size_t)qlen, hipMemcpyHostToDevice));
    std::vector<int64_t> a_off((size_t)nidx, qoff), d_off((size_t)nidx);
    std::vector<int> alen((size_t)nidx, qlen), dlen((size_t)nidx);
    for (int k = 0; k < nidx; ++k) {
        d_off[(size_t)k] = db->off[(size_t)record_idx[k]];
        dlen[(size_t)k] = db->len[(size_t)record_idx[k]];
    }
    return translated_align_device(mx, xl, v->arena, a_off.data(), alen.data(), d_off.data(), dlen.data(), fidx.data(), record_idx,
                                   nidx, gap_init, gap_ext, "sw_db_align_matrix_translated: record", sink, amode);
}

}  // namespace
}  // namespace swmi

using namespace swmi;

extern "C" {

int sw_db_search_matrix_translated(sw_db* db, const sw_matrix* mx, const unsigned char* query, int qlen, int gap_init,
                                   int gap_ext, int mode, const unsigned char* code64, int* scores_out) {
    const char* fn = "sw_db_search_matrix_translated";
    if (!db || !mx || qlen < 0 || (qlen > 0 && !query) || (!db->len.empty() && !scores_out)) {
        report_error("sw_db_search_matrix_translated: invalid arguments (a null pointer or a negative length)");
        return -1;
    }
    Translated xl;
    if (!mode_ok(fn, mode) || translated_tables(fn, mx, code64, &xl)) return -1;
    std::lock_guard<std::mutex> g(db->mu);
    return search_translated(db, mx, xl, query, qlen, gap_init, gap_ext, mode, scores_out);
}

int sw_db_align_matrix_translated(sw_db* db, const sw_matrix* mx, const unsigned char* query, int qlen, const int* record_idx,
                                  const int* frames, int nidx, int gap_init, int gap_ext, int mode, const unsigned char* code64,
                                  sw_alignment* out, unsigned* cigar, long long cigar_cap, long long* cigar_used) {
    const char* fn = "sw_db_align_matrix_translated";
    if (!db || !mx || qlen < 0 || (qlen > 0 && !query) || nidx < 0 || cigar_cap < 0 || !cigar_used || (cigar_cap > 0 && !cigar) ||
        (nidx > 0 && (!record_idx || !frames || !out))) {
        report_error("sw_db_align_matrix_translated: invalid arguments (a null pointer or a negative length)");
        return -1;
    }
    Translated xl;
    if (!mode_ok(fn, mode) || translated_tables(fn, mx, code64, &xl)) return -1;
    std::lock_guard<std::mutex> g(db->mu);
    AlignSink sink{out, {}};
    if (align_translated(db, mx, xl, query, qlen, record_idx, frames, nidx, gap_init, gap_ext, mode, sink)) return -1;
    return sink.finish(cigar, cigar_cap, cigar_used);
}

int sw_db_search_profile(sw_db* db, const sw_profile* pf, int gap_init, int gap_ext, int mode, int* scores_out) {
    if (!db || !pf || (!db->len.empty() && !scores_out)) {
        report_error("sw_db_search_profile: invalid arguments");
        return -1;
    }
    if (!mode_ok("sw_db_search_profile", mode)) return -1;
    std::lock_guard<std::mutex> g(db->mu);
    return search_profile(db, pf, gap_init, gap_ext, mode, scores_out);
}

int sw_db_align_profile(sw_db* db, const sw_profile* pf, const int* record_idx, int nidx, int gap_init, int gap_ext, int mode,
                        sw_alignment* out, unsigned* cigar, long long cigar_cap, long long* cigar_used) {
    if (!db || !pf || nidx < 0 || cigar_cap < 0 || !cigar_used || (cigar_cap > 0 && !cigar) ||
        (nidx > 0 && (!record_idx || !out))) {
        report_error("sw_db_align_profile: invalid arguments");
        return -1;
    }
    if (!mode_ok("sw_db_align_profile", mode)) return -1;
    std::lock_guard<std::mutex> g(db->mu);
    AlignSink sink{out, {}};
    if (align_profile(db, pf, record_idx, nidx, gap_init, gap_ext, mode, sink)) return -1;
    return sink.finish(cigar, cigar_cap, cigar_used);
}

int sw_db_search_matrix(sw_db* db, const sw_matrix* mx, const unsigned char* query, int qlen, int gap_init,
                        int gap_ext, int* scores_out) {
    if (!db || !mx || qlen < 0 || (qlen > 0 && !query) || (!db->len.empty() && !scores_out)) {
        report_error("sw_db_search_matrix: invalid arguments");
        return -1;
    }
    std::lock_guard<std::mutex> g(db->mu);
    return search_matrix(db, mx, query, qlen, gap_init, gap_ext, scores_out, qlen, 0);
}

int sw_db_search_matrix_mode(sw_db* db, const sw_matrix* mx, const unsigned char* query, int qlen, int gap_init,
                             int gap_ext, int mode, int* scores_out) {
    if (!db || !mx || qlen < 0 || (qlen > 0 && !query) || (!db->len.empty() && !scores_out)) {
        report_error("sw_db_search_matrix_mode: invalid arguments");
        return -1;
    }
    if (!mode_ok("sw_db_search_matrix_mode", mode)) return -1;
    std::lock_guard<std::mutex> g(db->mu);
    return search_matrix(db, mx, query, qlen, gap_init, gap_ext, scores_out, qlen, 0, mode);
}

int sw_db_align_matrix_mode(sw_db* db, const sw_matrix* mx, const unsigned char* query, int qlen, const int* record_idx,
                            int nidx, int gap_init, int gap_ext, int mode, sw_alignment* out, unsigned* cigar,
                            long long cigar_cap, long long* cigar_used) {
    if (!db || !mx || qlen < 0 || (qlen > 0 && !query) || nidx < 0 || cigar_cap < 0 || !cigar_used ||
        (cigar_cap > 0 && !cigar) || (nidx > 0 && (!record_idx || !out))) {
        report_error("sw_db_align_matrix_mode: invalid arguments");
        return -1;
    }
    if (!mode_ok("sw_db_align_matrix_mode", mode)) return -1;
    std::lock_guard<std::mutex> g(db->mu);
    AlignSink sink{out, {}};
    if (align_matrix(db, mx, query, qlen, record_idx, nidx, gap_init, gap_ext, sink, false, mode)) return -1;
    return sink.finish(cigar, cigar_cap, cigar_used);
}

// (one query after another: the pipelining of sw_db_search_db is not done for matrix searches)
int sw_db_search_db_matrix(sw_db* db, const sw_db* queries, const sw_matrix* mx, int gap_init, int gap_ext,
                           int* scores_out) {
    if (!db || !queries || !mx || (!db->len.empty() && !queries->len.empty() && !scores_out)) {
        report_error("sw_db_search_db_matrix: invalid arguments");
        return -1;
    }
    std::lock_guard<std::mutex> g(db->mu);
    const size_t nrec = db->len.size();
    int longest = 0;
    for (int l : queries->len) longest = std::max(longest, l);
    for (size_t q = 0; q < queries->len.size(); ++q)
        if (search_matrix(db, mx, queries->res.data() + queries->off[q], queries->len[q], gap_init, gap_ext,
                          scores_out + q * nrec, longest, (int)q))
            return -1;
    return 0;
}

int sw_db_align_matrix(sw_db* db, const sw_matrix* mx, const unsigned char* query, int qlen, const int* record_idx,
                       int nidx, int gap_init, int gap_ext, sw_alignment* out, unsigned* cigar, long long cigar_cap,
                       long long* cigar_used) {
    if (!db || !mx || qlen < 0 || (qlen > 0 && !query) || nidx < 0 || cigar_cap < 0 || !cigar_used ||
        (cigar_cap > 0 && !cigar) || (nidx > 0 && (!record_idx || !out))) {
        report_error("sw_db_align_matrix: invalid arguments");
        return -1;
    }
    std::lock_guard<std::mutex> g(db->mu);
    AlignSink sink{out, {}};
    if (align_matrix(db, mx, query, qlen, record_idx, nidx, gap_init, gap_ext, sink, false)) return -1;
    return sink.finish(cigar, cigar_cap, cigar_used);
}

int sw_db_align_matrix_long(sw_db* db, const sw_matrix* mx, const unsigned char* query, int qlen, const int* record_idx,
                            int nidx, int gap_init, int gap_ext, sw_alignment* out, unsigned* cigar, long long cigar_cap,
                            long long* cigar_used) {
    if (!db || !mx || qlen < 0 || (qlen > 0 && !query) || nidx < 0 || cigar_cap < 0 || !cigar_used ||
        (cigar_cap > 0 && !cigar) || (nidx > 0 && (!record_idx || !out))) {
        report_error("sw_db_align_matrix_long: invalid arguments");
        return -1;
    }
    std::lock_guard<std::mutex> g(db->mu);
    AlignSink sink{out, {}};
    if (align_matrix(db, mx, query, qlen, record_idx, nidx, gap_init, gap_ext, sink, true)) return -1;
    return sink.finish(cigar, cigar_cap, cigar_used);
}

int sw_db_align_matrix_long_coop(sw_db* db, const sw_matrix* mx, const unsigned char* query, int qlen, const int* record_idx,
                                 int nidx, int gap_init, int gap_ext, sw_alignment* out, unsigned* cigar, long long cigar_cap,
                                 long long* cigar_used) {
    if (!db || !mx || qlen < 0 || (qlen > 0 && !query) || nidx < 0 || cigar_cap < 0 || !cigar_used ||
        (cigar_cap > 0 && !cigar) || (nidx > 0 && (!record_idx || !out))) {
        report_error("sw_db_align_matrix_long_coop: invalid arguments");
        return -1;
    }
    std::lock_guard<std::mutex> g(db->mu);
    AlignSink sink{out, {}};
    if (align_matrix(db, mx, query, qlen, record_idx, nidx, gap_init, gap_ext, sink, true, SW_MODE_LOCAL, true)) return -1;
    return sink.finish(cigar, cigar_cap, cigar_used);
}

// the long path in a mode; local mode through them is the calls above
static int db_align_long_mode(const char* fn, bool coop, sw_db* db, const sw_matrix* mx, const unsigned char* query, int qlen,
                              const int* record_idx, int nidx, int gap_init, int gap_ext, int mode, sw_alignment* out,
                              unsigned* cigar, long long cigar_cap, long long* cigar_used) {
    if (!mode_ok(fn, mode)) return -1;
    if (mode == SW_MODE_LOCAL)
        return (coop ? sw_db_align_matrix_long_coop : sw_db_align_matrix_long)(db, mx, query, qlen, record_idx, nidx, gap_init,
                                                                               gap_ext, out, cigar, cigar_cap, cigar_used);
    if (!db || !mx || qlen < 0 || (qlen > 0 && !query) || nidx < 0 || cigar_cap < 0 || !cigar_used ||
        (cigar_cap > 0 && !cigar) || (nidx > 0 && (!record_idx || !out))) {
        char m[96];
        std::snprintf(m, sizeof m, "%s: invalid arguments", fn);
        report_error(m);
        return -1;
    }
    std::lock_guard<std::mutex> g(db->mu);
    AlignSink sink{out, {}};
    if (align_matrix(db, mx, query, qlen, record_idx, nidx, gap_init, gap_ext, sink, true, mode, coop)) return -1;
    return sink.finish(cigar, cigar_cap, cigar_used);
}

int sw_db_align_matrix_long_mode(sw_db* db, const sw_matrix* mx, const unsigned char* query, int qlen, const int* record_idx,
                                 int nidx, int gap_init, int gap_ext, int mode, sw_alignment* out, unsigned* cigar,
                                 long long cigar_cap, long long* cigar_used) {
    return db_align_long_mode("sw_db_align_matrix_long_mode", false, db, mx, query, qlen, record_idx, nidx, gap_init, gap_ext,
                              mode, out, cigar, cigar_cap, cigar_used);
}

int sw_db_align_matrix_long_coop_mode(sw_db* db, const sw_matrix* mx, const unsigned char* query, int qlen,
                                      const int* record_idx, int nidx, int gap_init, int gap_ext, int mode, sw_alignment* out,
                                      unsigned* cigar, long long cigar_cap, long long* cigar_used) {
    return db_align_long_mode("sw_db_align_matrix_long_coop_mode", true, db, mx, query, qlen, record_idx, nidx, gap_init,
                              gap_ext, mode, out, cigar, cigar_cap, cigar_used);
}

int sw_db_search(sw_db* db, const unsigned char* query, int qlen, int* scores_out) {
    if (!db || qlen < 0 || (qlen > 0 && !query) || (!db->len.empty() && !scores_out)) {
        report_error("sw_db_search: invalid arguments");
        return -1;
    }
    std::lock_guard<std::mutex> g(db->mu);
    return search(db, query, qlen, scores_out, qlen);
}

int sw_db_search_db(sw_db* db, const sw_db* queries, int* scores_out) {
    if (!db || !queries || (!db->len.empty() && !queries->len.empty() && !scores_out)) {
        report_error("sw_db_search_db: invalid arguments");
        return -1;
    }
    std::lock_guard<std::mutex> g(db->mu);
    return search_many(db, queries, scores_out);
}

void sw_db_close(sw_db* db) {
    if (!db) return;
    int cur = 0;
    const bool have = hipGetDevice(&cur) == hipSuccess;
    for (auto& kv : db->dev) {
        if (hipSetDevice(kv.first) != hipSuccess) continue;
        if (kv.second.stream) (void)hipStreamSynchronize((hipStream_t)kv.second.stream);
        if (kv.second.arena) (void)hipFree(kv.second.arena);
        if (kv.second.scores) (void)hipFree(kv.second.scores);
        if (kv.second.hscores) (void)hipHostFree(kv.second.hscores);
        for (void* ev : kv.second.done)
            if (ev) (void)hipEventDestroy((hipEvent_t)ev);
        if (kv.second.stream) (void)hipStreamDestroy((hipStream_t)kv.second.stream);
    }
    if (have && !db->dev.empty()) (void)hipSetDevice(cur);
    delete db;
}

}  // extern "C"
