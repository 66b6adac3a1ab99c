// sw_matrix_host.h -- the host side of substitution-matrix scoring: the matrix
// object, its byte-to-code map and the NCBI text parser, plain C++ with no HIP
// (as sw_db_host.h), so that they build both into libswmi355.so and into the
// sanitizer test binary (make -C concurrentproject_amd/csrc asan).
#pragma once
#include <cstddef>
#include <cstdint>

constexpr int SW_MATRIX_MAX_K = 32;
constexpr int SW_MATRIX_NOCODE = 0xFF;   // code[] of a byte outside the alphabet when other = -1

// Immutable after creation: any thread may read it at once.
struct sw_matrix {
    int k = 0;                                            // symbols
    unsigned char sym[SW_MATRIX_MAX_K] = {};              // distinct bytes
    signed char sc[SW_MATRIX_MAX_K * SW_MATRIX_MAX_K] = {};   // sc[i * k + j]: symbol i of seq1 / the query
                                                          // against symbol j of seq2 / the record
    int other = -1;                                       // index every byte outside the alphabet maps to, or -1
    int flags = 0;                                        // SW_MATRIX_FOLD_CASE
    unsigned char code[256] = {};                         // byte -> symbol index, SW_MATRIX_NOCODE = refused
    int max_entry = 0;                                    // max(0, largest entry)
    unsigned long long id = 0;                            // unique per created matrix (never reused): the key of
                                                          // a database's "records checked" cache
};

namespace swmi {
// sets the calling thread's sw_last_error() text (sw_engine.hip)
void report_error(const char* msg);

// first byte of p[0, len) outside m's alphabet: its position, or -1 when every byte has a code
long long matrix_first_bad(const sw_matrix* m, const unsigned char* p, long long len);

// One launch of the matrix kernel over pairs resident in device memory (sw_matrix.hip): pair k is
// d_arena[a_off[k], +alen[k]) (seq1: the table's first index) against d_arena[b_off[k], +blen[k]);
// d_scores[k] (device) receives its score.  Synchronous.  a_on_lanes: every pair spreads seq1 across
// the lanes (database search: the query); else the orientation is chosen per pair.  The bytes must
// have been checked against the alphabet.  0 or -1.
int matrix_score_device(const sw_matrix* m, const unsigned char* d_arena, const int64_t* a_off, const int* alen,
                        const int64_t* b_off, const int* blen, int npairs, int gap_init, int gap_ext,
                        int* d_scores, bool a_on_lanes);
}  // namespace swmi
