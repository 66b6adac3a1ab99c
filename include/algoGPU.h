/*
 * algoGPU.h -- drop-in C-ABI of the MI355X (gfx950) Smith-Waterman score engine
 * (libswmi355.so).  Link this library in place of the reference's
 * simpleGPU.o / cudaLazy.o / cudaSmithM.o (reference Makefile2:15) and keep the
 * reference's TestFileWithGPU.cpp and CPU sources unchanged.
 *
 * Semantics shared by every entry point:
 *   - the return value is the best local-alignment score max H >= 0 of the
 *     affine-gap recurrence of main.cpp:54-66 (E from the left, F from above,
 *     borders 0, score byte equality main.cpp:28-33), bit-exact;
 *   - seq1 has length n (len1), seq2 has length m (len2); the score is
 *     symmetric; any byte values are allowed (an {A,C,G,T}-only input takes
 *     the 2-bit profile path, anything else the raw-byte path);
 *   - n == 0 or m == 0 returns 0 (main.cpp:74-90 with empty loops);
 *   - the call is synchronous and re-entrant per host thread; the caller owns
 *     the host buffers, which are only read; device memory and the HIP stream
 *     are cached per (thread, device) and are not observable;
 *   - on an internal HIP failure, an invalid argument or unsupported scoring
 *     constants the return value is -1 and sw_last_error() says why (the
 *     reference had no error channel; cudaSmithM.cu:168-173 returned a
 *     partial score instead).
 *   - the scoring constants default to the reference's
 *     MATCH=1, MISMATCH=-1, G_INIT=1, G_EXT=1 (main.cpp:20-23) and can be
 *     changed with sw_set_params().
 */
#ifndef SWMI355_ALGOGPU_H
#define SWMI355_ALGOGPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the reference's algoGPU.h:5-9 surface (exact signatures) ---------------- */

/* replaces simpleGPU.cu:109-163 (reference: one launch + device sync per
 * anti-diagonal, only correct for len2 <= len1 and N < 46341). */
int SequentialSmithWatermanScoreGPU(unsigned char* seq1, unsigned char* seq2, int len1, int len2);

/* replaces cudaLazy.cu:58-99 (reference: full-matrix anti-diagonal kernel). */
int SmithWatermanLazyGPU(const unsigned char* seq1, const unsigned char* seq2, int n, int m);

/* replaces cudaSmithM.cu:128-189 (reference: full-matrix, no per-diagonal sync). */
int SmithWatermanScoreCUDA(const unsigned char* seq1, const unsigned char* seq2, int n, int m);

/* replaces SmithDiagonalGPUrefactored.cu:174-230 (extern "C" but never declared
 * in the reference's algoGPU.h).  That kernel is LINEAR-gap (gap = G_INIT per
 * residue, SmithDiagonalGPU.cu:59-66); this entry keeps its semantics: it is
 * the affine engine with G_EXT := G_INIT, which is exactly the linear model. */
int SmithDiagonalGPU(unsigned char* seq1, unsigned char* seq2, int n, int m);

/* ---- extensions (no reference counterpart) ---------------------------------- */

/* Scoring constants for later calls from ANY thread (process-wide).
 * Supported: 0 <= gap_init, gap_ext <= 1<<20; -127 <= mismatch <= 0;
 * mismatch <= match <= 127.  match <= 0 is supported: every score is then 0
 * (match < 0 never runs the packed 16-bit duos, whose H + match is unsigned).
 * Returns 0, or -1 if unsupported. */
int sw_set_params(int match, int mismatch, int gap_init, int gap_ext);
void sw_get_params(int* match, int* mismatch, int* gap_init, int* gap_ext);

/* One pair with explicit constants (does not change the process-wide ones). */
int sw_score_params(const unsigned char* seq1, const unsigned char* seq2, int n, int m,
                    int match, int mismatch, int gap_init, int gap_ext);

/* Batch of independent pairs (host buffers); scores_out[k] = score(a[k], b[k]).
 * One launch for the whole batch.  Returns 0 or -1. */
int sw_score_batch(const unsigned char* const* a, const int* alen,
                   const unsigned char* const* b, const int* blen,
                   int npairs, int* scores_out);

/* The same batch over the first ngpus visible GPUs of the node (SURVEY.md 8(b), configs
 * C3/C4): pairs are cut into contiguous shards (sw_batch_shard: sizes differ by at most
 * one), each scored by its own host thread and stream on its own device, and the int32
 * scores of devices 1..ngpus-1 are gathered to device 0 over RCCL (ncclSend/ncclRecv in
 * one group; RCCL is loaded at the first call with ngpus > 1) -- the only exchange, no
 * data-path collective.  Synchronous like the reference ABI; scores_out in pair order.
 * Returns 0, or -1 with sw_last_error() (e.g. ngpus above the visible devices).
 * Callers: the reference harness's batched loops (TestFileWithGPU.cpp:82-94).
 * UNVERIFIED ON HARDWARE for ngpus > 1: the build's GPU boxes have one GPU, so the RCCL
 * branch has only run through its host-side plan (sw_batch_gather_plan, CPU-tested).
 * Lifetime: the first call starts one host worker thread per device used; the threads are
 * detached and live for the rest of the process (never joined), as do their engine contexts,
 * streams and the RCCL communicators. */
int sw_score_batch_multi(const unsigned char* const* a, const int* alen,
                         const unsigned char* const* b, const int* blen,
                         int npairs, int* scores_out, int ngpus);
/* Shard [*lo, *hi) of rank `rank` of ngpus for npairs pairs (no GPU call).  0 or -1. */
int sw_batch_shard(int npairs, int ngpus, int rank, int* lo, int* hi);
/* The gather sw_score_batch_multi runs (no GPU call): count[r] scores of device r land in
 * device 0's gather buffer at offset[r] (r = 0: the local copy; r > 0: one ncclSend from
 * device r matched by one ncclRecv on device 0, skipped when count[r] == 0).  count and
 * offset hold ngpus ints.  0 or -1. */
int sw_batch_gather_plan(int npairs, int ngpus, int* count, int* offset);

/* Batch whose sequences are already resident in device memory (one arena,
 * byte offsets per sequence).  Offsets/lengths are HOST arrays; d_scores is a
 * device array of npairs ints.  Asynchronous on `stream` (a hipStream_t; NULL =
 * the engine's own stream, and then the call is synchronous).
 * flags: SW_FLAG_DNA asserts every byte is in {A,C,G,T} (skips the alphabet
 * scan), SW_FLAG_BYTES forces the raw-byte path.  After an asynchronous call,
 * sw_stream_status(stream) synchronises and reports kernel-side failures; it is also
 * the point after which the engine no longer refers to the caller's stream, so call it
 * before destroying a stream that such a call ran on. */
#define SW_FLAG_DNA   1
#define SW_FLAG_BYTES 2
int sw_score_batch_device(const unsigned char* d_arena,
                          const int64_t* a_off, const int* alen,
                          const int64_t* b_off, const int* blen,
                          int npairs, int* d_scores, int flags, void* stream);
int sw_stream_status(void* stream);

/* ---- one pair split into column slabs across GPUs (no reference counterpart;
 * the C5 pair N = 2^20 over the GPUs of a node) ---------
 * Rank r of R scores columns [bounds[r], bounds[r+1]) of seq1 against all of
 * seq2.  Its left edge (H - G_INIT, E - G_EXT of the previous slab's last
 * column, one 16-byte tagged granule per row) is written straight into rank
 * r's inflow buffer by rank r-1's kernel, through an IPC mapping of that
 * buffer (xGMI stores, no host staging); the pair's score is the max of the
 * R slab maxima (an all-reduce(MAX) of one int).  dist.ColumnSlabs drives it.
 *
 * sw_slab_bounds: R+1 column bounds; every slab but the last is a multiple of
 *   the kernel's column quantum (returned, > 0; 126 at two flow2 columns per lane,
 *   63 at one, 64*W for chain / flow).  flags must say
 *   SW_FLAG_DNA or SW_FLAG_BYTES (all ranks must plan the same kernel).
 * sw_score_slab_device: one slab, sequences resident in device memory:
 *   columns d_arena[col_off, col_off+n), rows d_arena[row_off, row_off+m).
 *   d_inflow / d_outflow: granule buffers of m rows (NULL = the matrix border
 *   / the pair's last column); epoch != 0, the same on every rank and fresh
 *   for every launch over the same buffers.  *d_score = this slab's max H.
 *   Asynchronous on `stream` as sw_score_batch_device.
 * sw_slab_alloc: a zeroed inflow buffer of m granules; returns 1 (fine-grained
 *   memory) or 2 (device memory), -1 on error; ipc_handle (SW_IPC_HANDLE_BYTES,
 *   may be NULL) receives its hipIpcMemHandle_t for the writing rank.  An exported
 *   buffer (ipc_handle != NULL: the edge another GPU writes) must be fine-grained:
 *   without it the call fails (-1) unless option "slab_plain" is 1.
 * sw_ipc_open / sw_ipc_close: map / unmap another process's buffer. */
#define SW_IPC_HANDLE_BYTES 64
int sw_slab_bounds(long long n, int m, int nslabs, int flags, long long* bounds);
/* sw_split_bounds: where option "f3split" cuts one pair of n columns that runs the staged two-column
 *   linear-gap kernel: the left half is columns [0, *cut), the right half columns [*cut, n) read
 *   mirrored behind *lead dead columns; *cut and n - *cut + *lead are multiples of 126.  Returns the
 *   strips of both halves together, 0 when n is too narrow for two strips each (n < 379; outputs
 *   untouched), -1 on bad arguments.  Needs no device. */
int sw_split_bounds(int n, int* cut, int* lead);
int sw_score_slab_device(const unsigned char* d_arena, int64_t col_off, int n, int64_t row_off, int m,
                         void* d_inflow, void* d_outflow, unsigned epoch, int* d_score, int flags, void* stream);
int sw_slab_alloc(int m, void** d_buf, void* ipc_handle);
int sw_slab_free(void* d_buf);
int sw_ipc_open(const void* ipc_handle, void** d_ptr);
int sw_ipc_close(void* d_ptr);

/* ---- FASTA databases: query x database scoring (no reference counterpart;
 * SURVEY.md 8(f) f-4, the makedb / align workflow of the reference's timing.sh:3-8
 * around the external CUDASW++4 tool, Makefile_CUDASW4.mak:44-56) ------------
 * These entry points score by byte equality (MATCH/MISMATCH, affine gaps,
 * main.cpp:28-66); sw_db_search_matrix below scores under a substitution matrix
 * read from a file (BLOSUM62 is not compiled in).  A database holds its residues
 * host-side and, after the first search, once in device memory (one arena,
 * per device); searches launch one batch over all of its records, longest
 * first, and return the scores in record order.
 *
 * sw_db_open: a FASTA file ('>' header lines; sequence lines of any width,
 *   whitespace and '\r' dropped, bytes otherwise kept as they are; ';' comment
 *   lines skipped; records may be empty) or a file written by sw_db_save.
 *   NULL on error (sw_last_error).
 * sw_db_from_fasta: the same parse over a buffer in memory.
 * sw_db_save: the binary database (the "makedb" step), 0 or -1.
 * sw_db_count / sw_db_residues: records, total residues.
 * sw_db_record: record i's residues, length and header (pointers owned by db).
 * sw_db_search: scores_out[i] = score(query, record i) for every record; the
 *   query is a byte string of qlen bytes.  Synchronous; 0 or -1.
 * sw_db_search_db: scores_out[q * count(db) + i] for every record q of queries.
 * sw_db_close: frees host and device memory. */
typedef struct sw_db sw_db;
sw_db* sw_db_open(const char* path);
sw_db* sw_db_from_fasta(const char* text, long long nbytes);
int sw_db_save(const sw_db* db, const char* path);
int sw_db_count(const sw_db* db);
long long sw_db_residues(const sw_db* db);
int sw_db_record(const sw_db* db, int i, const unsigned char** seq, int* len, const char** header);
int sw_db_search(sw_db* db, const unsigned char* query, int qlen, int* scores_out);
int sw_db_search_db(sw_db* db, const sw_db* queries, int* scores_out);
void sw_db_close(sw_db* db);

/* ---- substitution-matrix scoring (no reference counterpart; the scoring of the
 * CUDASW++4 search that timing.sh:3-8 runs) ------------------------------------
 * The same recurrence (main.cpp:54-66: E from the left, F from above, borders 0,
 * H = max(0, diag + s, E, F), score = max H, int32, bit-exact) with s(a, b) read
 * from a table instead of a byte compare.
 *
 * A matrix is K distinct byte symbols (1 <= K <= 32), a K x K table of entries in
 * [-127, 127] -- scores[i*K + j] scores symbol i of seq1 / the query against symbol
 * j of seq2 / the record; it need not be symmetric, and score(b, a, transpose) ==
 * score(a, b, M) -- `other`, the index of the symbol that every byte outside the
 * alphabet maps to, or -1, and flags: SW_MATRIX_FOLD_CASE maps a-z to A-Z wherever
 * the lower-case byte is not itself a symbol.  With other = -1 a byte outside the
 * alphabet is an error: the call returns -1 and sw_last_error() names the pair,
 * record or query index, the position and the byte (checked on the host: a
 * database's records once per (database, matrix), the query on every search).
 * A matrix is immutable and may be used from any thread at once.
 *
 * Gaps: a gap of L residues costs gap_init + (L-1) * gap_ext, the engine's model;
 * BLAST-style "open 11, extend 1" is gap_init = 12, gap_ext = 1.  Matrix calls take
 * the two as arguments (0 <= gap_init, gap_ext <= 1<<20, either may be the larger)
 * and neither read nor write sw_set_params' process-wide constants.
 *
 * sw_matrix_create: from a table.  NULL on error (sw_last_error).
 * sw_matrix_parse / sw_matrix_open: the NCBI text format: '#' comment lines, one
 *   header line of symbols, then K rows of a symbol and K integers; any run of
 *   blanks separates tokens, CRLF and a missing final newline are accepted, a '*'
 *   symbol becomes `other`.  NULL (with a message) for a table that is not square, a
 *   row label that disagrees with the header, a duplicate symbol, more than 32
 *   symbols, an entry outside +-127, a token that is not an integer, or no rows.
 *   No named matrix (BLOSUM, PAM) is compiled in: pass a file.
 * sw_matrix_size / sw_matrix_symbols: K (symbols copies the K bytes and returns K).
 * sw_matrix_score: *out = the entry for bytes (a, b) through the byte-to-code map
 *   the kernel uses (other, fold case); -1 if either byte has no code.
 * sw_score_matrix: one pair; the score, or -1.
 * sw_score_matrix_batch: scores_out[k] = score(a[k], b[k]); one launch; 0 or -1.
 *   n == 0 or m == 0 scores 0; npairs == 0 returns 0; a pair with
 *   max(0, largest entry) * min(n, m) >= 2^28 is refused before anything is launched.
 * sw_db_search_matrix / sw_db_search_db_matrix: as sw_db_search / sw_db_search_db
 *   (scores in record order; the database's device arena and query slot, no second
 *   copy of the residues); the query is seq1.  The queries of search_db run one
 *   after another (not pipelined).  Equality and matrix searches of one open database
 *   may alternate.
 * Limits: ONE WAVE scores one pair (sw_matrix.hip), so a launch needs thousands of
 * pairs to fill the GPU and one long pair runs at a few GCUPS; 16-bit packed
 * kernels and a multi-wave pair are not built. */
typedef struct sw_matrix sw_matrix;
#define SW_MATRIX_FOLD_CASE 1
sw_matrix* sw_matrix_create(const unsigned char* symbols, int k, const signed char* scores, int other, int flags);
sw_matrix* sw_matrix_parse(const char* text, long long nbytes);
sw_matrix* sw_matrix_open(const char* path);
int  sw_matrix_size(const sw_matrix*);
int  sw_matrix_symbols(const sw_matrix*, unsigned char* out /* k bytes */);
int  sw_matrix_score(const sw_matrix*, unsigned char a, unsigned char b, int* out);
void sw_matrix_free(sw_matrix*);
int  sw_score_matrix(const sw_matrix*, const unsigned char* seq1, const unsigned char* seq2, int n, int m,
                     int gap_init, int gap_ext);                       /* score, or -1 */
int  sw_score_matrix_batch(const sw_matrix*, const unsigned char* const* a, const int* alen,
                           const unsigned char* const* b, const int* blen, int npairs,
                           int gap_init, int gap_ext, int* scores_out); /* 0 or -1 */
int  sw_db_search_matrix(sw_db*, const sw_matrix*, const unsigned char* query, int qlen,
                         int gap_init, int gap_ext, int* scores_out);
int  sw_db_search_db_matrix(sw_db*, const sw_db* queries, const sw_matrix*,
                            int gap_init, int gap_ext, int* scores_out);

/* ---- alignments under a substitution matrix (no reference counterpart: the reference
 * scores only) -------------------------------------------------------------------
 * Per pair: the score (the one sw_score_matrix returns), the half-open ranges
 * [beg1, end1) of seq1 and [beg2, end2) of seq2 that the alignment covers, and its
 * operations, run-length encoded, first operation first, as ncigar entries
 * (length << 4) | op at cigar[cigar_off]: op 0 = M (a residue of seq1 aligned with one
 * of seq2), 1 = I (a residue of seq1 against a gap), 2 = D (a residue of seq2 against a
 * gap).  The M entries' table scores minus gap_init + (L-1) * min(gap_ext, gap_init) for
 * every maximal run of L equal gap operations add up to the score exactly (where extending
 * costs more than opening, the recurrence itself opens a new gap for every residue).
 *
 * Which alignment, where several reach the score -- stated in sequence positions only,
 * so it does not depend on the kernel's tiling, the grid or the rest of the batch:
 *   END CELL.  Positions i in seq1 and j in seq2 (0-based), t(i, j) = H[i-1][j-1] +
 *     s(seq1[i], seq2[j]) the diagonal arrival.  Among the cells with t(i, j) == score
 *     the end cell is the one with the smallest i + j and, among those, the smallest j.
 *     (t, not H: with gap_init = 0 a cell can reach the score through a free gap, and an
 *     alignment does not end in a gap.)  end1 = i + 1, end2 = j + 1.
 *   WALK.  From the end cell in state H, backwards.  In state H: a cell with H = 0 ends
 *     the walk (tested before anything else, so the first and the last operation are M);
 *     else H = t takes the diagonal (M), else H = E enters state E, else state F.  State E
 *     emits I and steps to i - 1, state F emits D and steps to j - 1; each returns to
 *     state H if the gap was opened there (E = H[i-1][j] - gap_init) and stays if it was
 *     extended, OPENING BEFORE EXTENDING on a tie.  An I may therefore stand next to a D
 *     (the gap opened from a cell whose H came from the other gap state): they are two
 *     gaps and cost two openings.
 * A pair with score 0 or an empty sequence yields score 0, the four coordinates 0 and no
 * operations (cigar_off still points into the buffer's used part).
 *
 * sw_align_matrix_batch: the GPU path: the traced variant of the matrix kernel records 4
 *   bits a cell (sw_matrix.hip), a second kernel walks them, the host reverses and encodes.
 *   seq1 always lies across the lanes: no per-pair swap.  Trace memory is about n * m / 2
 *   bytes a pair plus 128 KiB per strip of 512 seq1 positions, and a launch holds at most
 *   option "trace_mb" MiB of it (default 1024): a batch that does not fit runs as several
 *   launches, packed greedily in input order; ONE PAIR THAT DOES NOT FIT ALONE IS REFUSED
 *   (-1, sw_last_error names the pair and the bytes); sw_align_matrix_long (below) aligns
 *   such pairs.  Arguments, gap penalties, the score range and the alphabet are
 *   checked as sw_score_matrix_batch checks them.  cigar_cap: entries of cigar;
 *   *cigar_used receives the entries needed, and too small a cigar_cap returns -1 (out is
 *   filled, cigar is not).  Option "W" is not honoured (one traced instantiation, W = 8);
 *   "blocks" is.  sw_last_stats: mode 7, boundary_bytes = trace bytes of the largest
 *   launch, blocks = workgroups of the last, variant = launches, kernel_ms = the fill
 *   kernels; sw_last_align_ms splits the device time into fill and walk.
 * sw_align_matrix_cpu: the same result from a plain full-matrix aligner on the host (n * m
 *   bytes a pair, at most 2^32 cells): the checker of the GPU path, and a fallback.
 * sw_db_align_matrix: the query (seq1) against records record_idx[0, nidx) of the
 *   database, out of its device arena: only the query is uploaded.  out[k] belongs to
 *   record_idx[k]; an index may repeat.
 * sw_align_matrix_long, sw_db_align_matrix_long: the same arguments, outputs and cigar
 *   protocol, and bit for bit the same alignments, for pairs whose whole trace does not
 *   fit: CHECKPOINTED TRACEBACK, one strip at a time.  A locate pass (the traced kernel's
 *   end-cell bookkeeping, no trace stores) finds the score and the end cell and keeps the
 *   right-edge column of every strip of 512 seq1 positions but the last (a checkpoint:
 *   H - gap_init and E - gap_ext, 8 bytes a seq2 position).  Then rounds: every pair still
 *   walking has the one strip its walk stands in filled again from the checkpoint on its
 *   left, traced, over seq2 positions [0, j] only (j: where the walk enters the strip) --
 *   the same recurrence on the same integers, hence the same 4 bits a cell -- and the walk
 *   runs on through that strip, appending its operations, until it ends or leaves the strip
 *   on the left.  At most ceil(n / 512) rounds; nothing on the device waits for anything.
 *   Memory, for an n x m pair with s = ceil(n / 512) strips:
 *     checkpoints  (s - 1) * roundup(m, 64) * 8 bytes    (about n * m / 64)
 *     one strip    ceil((m + 511) / 64) * 64 * 256 bytes (about 128 m + 128 KiB)
 *   Strip traces of a round's launch share the trace_mb budget (a round that does not fit
 *   runs as several launches, packed greedily in input order); the checkpoints of the pairs
 *   in flight share the budget of the environment variable SWMI_ALIGN_CKPT_MB (whole MiB,
 *   at least 1, default 4096, read on every call), and a batch that exceeds it runs as
 *   several groups, greedy in input order.  One pair is refused before anything is launched
 *   (-1, sw_last_error names the pair, both lengths, the bytes and the limit) when its
 *   checkpoints alone exceed that budget or one of its strips alone exceeds trace_mb.
 *   sw_last_stats: mode 8, W 8, C 64, items = npairs, variant = strip-fill launches,
 *   boundary_bytes = the most device bytes of checkpoints plus strip traces held at once,
 *   kernel_ms = locate plus strip fills; sw_last_align_ms: fill = locate plus strip fills,
 *   walk = the walks.  One wave still runs one pair, so a long pair is slow: seconds for
 *   32768 x 32768.
 * sw_align_long_plan: no GPU call.  For one n x m pair under the current trace_mb and
 *   SWMI_ALIGN_CKPT_MB: strips, checkpoint bytes, bytes of the largest strip trace, bytes
 *   sw_align_matrix_batch would need.  0, or -1 (sw_last_error) when sw_align_matrix_long
 *   would refuse the pair (out is filled either way when the lengths are valid).
 * Limits: one wave fills one pair and one lane walks it, so this is for the hits of a
 * search, not for every pair of it. */
typedef struct { int score, beg1, end1, beg2, end2, ncigar; long long cigar_off; } sw_alignment;
int  sw_align_matrix_batch(const sw_matrix*, const unsigned char* const* a, const int* alen,
                           const unsigned char* const* b, const int* blen, int npairs,
                           int gap_init, int gap_ext, sw_alignment* out,
                           unsigned* cigar, long long cigar_cap, long long* cigar_used);
int  sw_align_matrix_cpu(const sw_matrix*, const unsigned char* const* a, const int* alen,
                         const unsigned char* const* b, const int* blen, int npairs,
                         int gap_init, int gap_ext, sw_alignment* out,
                         unsigned* cigar, long long cigar_cap, long long* cigar_used);
int  sw_db_align_matrix(sw_db*, const sw_matrix*, const unsigned char* query, int qlen,
                        const int* record_idx, int nidx, int gap_init, int gap_ext,
                        sw_alignment* out, unsigned* cigar, long long cigar_cap, long long* cigar_used);
int  sw_align_matrix_long(const sw_matrix*, const unsigned char* const* a, const int* alen,
                          const unsigned char* const* b, const int* blen, int npairs,
                          int gap_init, int gap_ext, sw_alignment* out,
                          unsigned* cigar, long long cigar_cap, long long* cigar_used);
int  sw_db_align_matrix_long(sw_db*, const sw_matrix*, const unsigned char* query, int qlen,
                             const int* record_idx, int nidx, int gap_init, int gap_ext,
                             sw_alignment* out, unsigned* cigar, long long cigar_cap, long long* cigar_used);
typedef struct { int strips; long long ckpt_bytes, strip_trace_bytes, full_trace_bytes; } sw_align_plan;
int  sw_align_long_plan(int n, int m, sw_align_plan* out);
/* device time of this thread's last sw_align_matrix_batch / sw_db_align_matrix (or _long) call,
 * summed over its launches (either pointer may be NULL) */
void sw_last_align_ms(float* fill_ms, float* walk_ms);
/* the same for this thread's last sw_align_matrix_long / sw_db_align_matrix_long call, the fill
 * split into the locate launches and the strip fills, and the call's rounds, summed over its
 * groups (any pointer may be NULL; zeros after a call of the other kind) */
void sw_last_align_long_ms(float* locate_ms, float* strip_ms, float* walk_ms, int* rounds);

/* ---- global and semi-global alignment under a substitution matrix ----
 * Everything above is LOCAL alignment.  The *_mode entry points take an alignment mode:
 *   SW_MODE_LOCAL       what every call above does, bit for bit (through either entry point)
 *   SW_MODE_GLOBAL      seq1 and seq2 both end to end (Needleman-Wunsch with Gotoh's affine gaps)
 *   SW_MODE_SEMIGLOBAL  seq1 (the query) end to end; seq2 (the record) free at both ends
 *
 * THE RECURRENCE.  i in seq1 (across the lanes, n residues), j in seq2 (the rows that stream, m
 * residues); s = matrix[seq1[i]][seq2[j]]; E runs along seq1 (operation I), F along seq2
 * (operation D).  A run of L gap operations costs G_INIT + (L-1) * min(G_EXT, G_INIT), which is
 * what the local recurrence charges in the interior; the borders charge the same, so that one
 * re-scoring rule (above) covers all modes.  gx = min(G_EXT, G_INIT).
 *     E[i][j] = max(E[i-1][j] - G_EXT, H[i-1][j] - G_INIT)
 *     F[i][j] = max(F[i][j-1] - G_EXT, H[i][j-1] - G_INIT)
 *     H[i][j] = max(H[i-1][j-1] + s, E[i][j], F[i][j])           no clamp at 0
 *   Borders:
 *     H[-1][-1] = 0
 *     H[i][-1]  = -(G_INIT + i * gx)      both modes: i + 1 residues of seq1 against gaps
 *     H[-1][j]  = -(G_INIT + j * gx)      global
 *     H[-1][j]  = 0                       semi-global
 *     E[-1][j], F[i][-1] = minus infinity: a gap cannot be extended out of a border
 *   SCORE AND END CELL.  Global: H[n-1][m-1].  Semi-global: the maximum over j in [0, m) of
 *     H[n-1][j]; the end cell is the smallest such j.  (H, not the diagonal arrival t of the
 *     local rule: an end-to-end alignment may end in a gap.)  end1 = n, end2 = j + 1.
 *   WALK.  From the end cell in state H, backwards, with the local priorities: in H the diagonal
 *     (H == t) first, then E, then F; in E and F opening before extending.  There is no H = 0 stop.
 *     The walk leaves the matrix at j < 0 -- the remaining i + 1 residues of seq1 become one
 *     leading I run -- or at i < 0: global, the remaining j + 1 residues of seq2 become one
 *     leading D run; semi-global, the walk stops and beg2 = j + 1.
 *   Ranges: global [0, n) x [0, m); semi-global [0, n) x [beg2, end2).  Unlike local, an
 *   alignment may begin or end with a gap, and scores may be negative: every function here
 *   returns 0 or -1, never a score.
 *   EMPTY SEQUENCES are answered on the host.  Global with one side empty, the other of length
 *   L: score -(G_INIT + (L-1) * gx), one gap run (I over seq1 or D over seq2); both empty: 0.
 *   Semi-global: n = 0 scores 0 (no operations, all coordinates 0); m = 0 is the all-I run.
 *   SCORE RANGE.  A pair with (n + m + 1024) * max(G_INIT, G_EXT, 127) >= 2^28 is refused before
 *   any launch (-1, sw_last_error names the pair): below that bound every cell of the matrix lies
 *   within +-2^28 and no cell outside it -- those now hold unclamped values that start at
 *   "minus infinity" = -2^30 -- can wrap int32 or reach a cell of the matrix.  The local bound
 *   (min length * largest entry < 2^28) is checked as well.
 *
 * sw_score_matrix_batch_mode: as sw_score_matrix_batch.  One launch is one mode; in the new modes
 *   seq1 always lies across the lanes (the modes are not symmetric in the sequences).  Options
 *   "W" and "blocks" are honoured.  sw_last_stats: mode 6 as before, and variant = the alignment
 *   mode (variant is otherwise unused on score-only matrix launches; 0 = local as ever).
 * sw_align_matrix_batch_mode: as sw_align_matrix_batch (trace memory, packing, cigar protocol).
 *   sw_last_stats: mode 7; variant = launches as before in bits 0-27, the alignment mode in
 *   bits 28-29.  A pair whose trace does not fit option "trace_mb" alone is refused with a
 *   message that says so and names sw_align_matrix_long_mode (below), which aligns such pairs in a
 *   mode; this call never takes that path by itself.
 * sw_align_matrix_cpu_mode: the plain full-matrix host aligner with the same end rule and walk.
 * sw_db_search_matrix_mode, sw_db_align_matrix_mode: as sw_db_search_matrix / sw_db_align_matrix;
 *   the query is seq1, so semi-global finds the whole query inside a record.
 * An unknown mode returns -1 with a message.  Not built in the new modes: sw_db_search_db_matrix.
 * The long path in a mode has entry points of its own (sw_align_matrix_long_mode, below). */
#define SW_MODE_LOCAL      0
#define SW_MODE_GLOBAL     1
#define SW_MODE_SEMIGLOBAL 2
int  sw_score_matrix_batch_mode(const sw_matrix*, const unsigned char* const* a, const int* alen,
                                const unsigned char* const* b, const int* blen, int npairs,
                                int gap_init, int gap_ext, int mode, int* scores_out);
int  sw_align_matrix_batch_mode(const sw_matrix*, const unsigned char* const* a, const int* alen,
                                const unsigned char* const* b, const int* blen, int npairs,
                                int gap_init, int gap_ext, int mode, sw_alignment* out,
                                unsigned* cigar, long long cigar_cap, long long* cigar_used);
int  sw_align_matrix_cpu_mode(const sw_matrix*, const unsigned char* const* a, const int* alen,
                              const unsigned char* const* b, const int* blen, int npairs,
                              int gap_init, int gap_ext, int mode, sw_alignment* out,
                              unsigned* cigar, long long cigar_cap, long long* cigar_used);
int  sw_db_search_matrix_mode(sw_db*, const sw_matrix*, const unsigned char* query, int qlen,
                              int gap_init, int gap_ext, int mode, int* scores_out);
int  sw_db_align_matrix_mode(sw_db*, const sw_matrix*, const unsigned char* query, int qlen,
                             const int* record_idx, int nidx, int gap_init, int gap_ext, int mode,
                             sw_alignment* out, unsigned* cigar, long long cigar_cap, long long* cigar_used);

/* ---- banded alignment under a substitution matrix ----
 * The *_band entry points compute only the cells within a fixed distance of the corner-to-corner
 * diagonal: work and trace memory fall from n * m to n * width.
 *
 * THE BAND.  For a pair with n = len(seq1), m = len(seq2) and a band B >= 0:
 *     dlo = min(0, m - n) - B        dhi = max(0, m - n) + B
 *     cell (i, j), 0 <= i < n, 0 <= j < m, is in the band  iff  dlo <= j - i <= dhi
 *   Both corners (0, 0) and (n-1, m-1) are in the band, and every row and column holds a cell of it.
 *   A cell outside the band does not exist: in global and semi-global mode its H, E and F are minus
 *   infinity; in local mode it is the border state H = E = F = 0 (equivalent there), and it is never
 *   a candidate for the maximum or the end.
 *   The borders are boundary conditions, not cells, and are NOT masked: H[i][-1] and H[-1][j] are
 *   what the modes above define (0 in local mode).  Every cell in the band is reachable from a
 *   border along its own diagonal, so its value is finite.
 *   Everything else is the local rule (sw_align_matrix_batch) and the modes above, restricted to
 *   cells in the band.  END CELL: local, the largest t, ties by the smallest i + j, then the smallest
 *   j; global, (n-1, m-1); semi-global, the largest H[n-1][j] over j in the band, the smallest such j.
 *   WALK: the same priorities and the same border exits.
 *   With B >= max(n, m) the band is the whole matrix and the result equals the unbanded call's bit
 *   for bit.  A call with a band always runs the band kernels.
 *
 * sw_score_matrix_batch_band / sw_align_matrix_batch_band: as the *_mode calls, every mode
 *   (SW_MODE_LOCAL too), seq1 always across the lanes.  band < 0 and an unknown mode return -1 with
 *   a message that names the function; the alphabet, gap, score-range and (global, semi-global)
 *   mode-range checks are the *_mode calls'.  The traced launch holds the band's trace only --
 *   sw_band_plan's trace_bytes a pair -- and a pair whose band does not fit option "trace_mb" alone
 *   is refused before anything is launched.  Empty sequences are answered on the host as above.
 *   sw_last_stats: mode 9 (scores) or 10 (traced); variant as modes 6 / 7; cells = the cells in the
 *   bands.
 * sw_align_matrix_cpu_band: the plain host aligner restricted to the band (full-matrix storage):
 *   the yardstick of the GPU path, bit for bit.
 * sw_band_plan: host arithmetic, no GPU call: dlo and dhi by the formula, the cells in the band,
 *   the trace bytes the traced band launch holds for the pair and what the unbanded launch would.
 * Not built with a band: the database calls, the long path, sw_db_search_db_matrix, X-drop or
 *   adaptive bands, a band given as a diagonal range. */
typedef struct {
    long long dlo, dhi;            /* the diagonal range of j - i */
    long long cells;               /* cells in the band */
    long long trace_bytes;         /* sw_align_matrix_batch_band holds this much trace for the pair */
    long long full_trace_bytes;    /* sw_align_matrix_batch(_mode) would hold this much */
} sw_band_plan_t;
int  sw_score_matrix_batch_band(const sw_matrix*, const unsigned char* const* a, const int* alen,
                                const unsigned char* const* b, const int* blen, int npairs,
                                int gap_init, int gap_ext, int mode, int band, int* scores_out);
int  sw_align_matrix_batch_band(const sw_matrix*, const unsigned char* const* a, const int* alen,
                                const unsigned char* const* b, const int* blen, int npairs,
                                int gap_init, int gap_ext, int mode, int band, sw_alignment* out,
                                unsigned* cigar, long long cigar_cap, long long* cigar_used);
int  sw_align_matrix_cpu_band(const sw_matrix*, const unsigned char* const* a, const int* alen,
                              const unsigned char* const* b, const int* blen, int npairs,
                              int gap_init, int gap_ext, int mode, int band, sw_alignment* out,
                              unsigned* cigar, long long cigar_cap, long long* cigar_used);
int  sw_band_plan(int n, int m, int band, sw_band_plan_t* out);

/* ---- one long pair on many waves: the cooperative score path ----
 *
 * Every call above runs one pair on one wave.  sw_score_matrix_batch_coop runs the strips of a pair
 * -- a strip is the 64 * W columns one wave sweeps top to bottom -- on as many waves as there are
 * strips, each wave handing its strip's right edge to the wave on its right inside one launch.
 * Scores only, no band; opt-in: no other call takes this path.
 *
 * sw_score_matrix_batch_coop: the arguments, checks, messages and return value of
 *   sw_score_matrix_batch_mode, and the same scores bit for bit.  Semi-global lays seq1 across the
 *   lanes; local and global lay a pair either way, by the estimate below, unless option "orient"
 *   names one (1: seq1 across the lanes, 2: seq2).
 *   W: option "W" when set; else, per call, the W with the smallest estimate of steps,
 *   m + strips * 64 * (W + 1), times the measured time of a step at that W, among the W whose edge
 *   columns fit.
 *   MEMORY: a pair of more than one strip holds (strips - 1) * m * 8 bytes of edge columns (m: the
 *   sequence that streams), every column written once and read once in a launch.  Columns are NOT
 *   recycled through a ring inside a launch.  Option "coop_mb" (MiB, default 1024, 1 .. 3072) caps a
 *   launch: a batch that does not fit runs as several launches, pairs packed in input order, and a
 *   pair that does not fit alone at the largest W allowed is refused before anything is launched,
 *   with a message that gives the bytes it needs.
 *   A wave waits only for the strip on its left, which an earlier claim holds; the wait is bounded
 *   by option "timeout", after which the call returns -1 and sw_last_error names the item (pair and
 *   strip).
 *   Option "coop_poison" (0 / 1, default 0; tests): the host fills the edge columns with 0x3F bytes
 *   before every launch, so that a row consumed before it was stored carries H of about 10^9 into
 *   the score.  Both options are set and read with sw_set_option / sw_get_option.
 *   sw_last_stats: mode 11; W; items = the strips of all pairs; cells; boundary_bytes = the edge
 *   bytes of the largest launch; variant = the alignment mode.
 * sw_matrix_coop_plan: host arithmetic, no GPU call: what the call would choose for one n x m pair
 *   under the current options.  -1 with the refusal's message where the call would refuse. */
typedef struct {
    int W;                  /* columns per lane */
    int strips;             /* = waves the pair can use */
    int swap;               /* 1: seq2 lies across the lanes */
    long long edge_bytes;   /* (strips - 1) * rows * 8 */
    long long items;        /* work items: strips */
} sw_coop_plan;
int  sw_score_matrix_batch_coop(const sw_matrix*, const unsigned char* const* a, const int* alen,
                                const unsigned char* const* b, const int* blen, int npairs,
                                int gap_init, int gap_ext, int mode, int* scores_out);
int  sw_matrix_coop_plan(int n, int m, int mode, sw_coop_plan* out);

/* ---- long pairs on many waves: cooperative locate, a window of strips a round ----
 *
 * sw_align_matrix_long runs the locate pass of a pair on one wave and fills one strip of it a round.
 * sw_align_matrix_long_coop, sw_db_align_matrix_long_coop: the arguments, checks, refusals, messages and
 *   cigar protocol of their _long namesakes, and bit for bit the same alignments.  Local alignment (the
 *   other modes: sw_align_matrix_long_coop_mode, below); opt-in: no other call takes this path.  Two things differ:
 *   LOCATE ON MANY WAVES.  A work item is one strip (512 seq1 positions) of one pair, claimed in order;
 *   the wave of strip s + 1 follows the wave of strip s down the pair through checkpoint column s, by the
 *   hand-off of sw_score_matrix_batch_coop (a progress word an item, a bounded poll: option "timeout",
 *   after which the call returns -1 and sw_last_error names the item, its pair and its strip).  The
 *   checkpoints are the ones sw_align_matrix_long keeps, same bytes, same layout.  Every item reports the
 *   end cell of its strip in a 16-byte record and the host merges a pair's records by the end-cell rule
 *   above.  Beyond the checkpoints: 4 bytes of progress word and 16 bytes of record a strip.
 *   A WINDOW OF STRIPS A ROUND.  The walk's seq2 position never grows as it moves left, so the position j
 *   at which it enters strip s bounds the rows of every strip further left: a round fills the G strips
 *   [s - G + 1, s] of a pair at once, each over seq2 positions [0, j] from the checkpoint on its own left,
 *   on G waves, and the walk runs on through all of them.  Rounds fall from the strips a walk covers to
 *   ceil(that / G).  Option "long_window" (0 .. 64, default 0; set and read with sw_set_option /
 *   sw_get_option, read by these two calls and sw_align_long_coop_plan only):
 *     0        automatic: in every round each pair still walking gets
 *              G = max(1, min(64, floor(trace_mb bytes / sum over those pairs of one strip's trace)))
 *     1 .. 64  that G, cut to what fits trace_mb for the pair alone; 1 takes the rounds of
 *              sw_align_matrix_long
 *   and either is cut to the strips that are left (s + 1).  A strip is budgeted at its full height, a
 *   launch never holds more than trace_mb of trace, and a round that does not fit runs as several
 *   launches as before.  Option "coop_poison" = 1 fills the checkpoint columns with 0x3F bytes before
 *   the locate launch.
 *   sw_last_stats: mode 12, W 8, C 64, items = the strips of all pairs (the items of the locate launches),
 *   variant = strip-fill launches, boundary_bytes = the most device bytes of checkpoints, progress words,
 *   end records and window traces held at once, kernel_ms = locate plus strip fills;
 *   sw_last_align_long_ms and sw_last_align_ms as after sw_align_matrix_long.
 * sw_align_long_coop_plan: no GPU call.  For one n x m pair under the current trace_mb, SWMI_ALIGN_CKPT_MB
 *   and long_window: strips, checkpoint bytes, the bytes of progress words and of end records, the window
 *   the pair would get alone in its first round if its walk began in the last strip, and that window's
 *   trace bytes.  Refuses exactly as sw_align_long_plan refuses. */
typedef struct {
    int strips;                     /* = items of the locate launch */
    long long ckpt_bytes;           /* as sw_align_plan */
    long long progress_bytes;       /* a 4-byte word a strip, a whole number of 16 bytes */
    long long end_bytes;            /* a 16-byte end-cell record a strip */
    int window;                     /* strips a round fills at once */
    long long window_trace_bytes;   /* window * one strip's trace */
} sw_align_coop_plan;
int  sw_align_matrix_long_coop(const sw_matrix*, const unsigned char* const* a, const int* alen,
                               const unsigned char* const* b, const int* blen, int npairs,
                               int gap_init, int gap_ext, sw_alignment* out,
                               unsigned* cigar, long long cigar_cap, long long* cigar_used);
int  sw_db_align_matrix_long_coop(sw_db*, const sw_matrix*, const unsigned char* query, int qlen,
                                  const int* record_idx, int nidx, int gap_init, int gap_ext,
                                  sw_alignment* out, unsigned* cigar, long long cigar_cap, long long* cigar_used);
int  sw_align_long_coop_plan(int n, int m, sw_align_coop_plan* out);

/* ---- long pairs in a mode: checkpointed traceback, global and semi-global ----
 *
 * sw_align_matrix_long_mode, sw_db_align_matrix_long_mode: sw_align_matrix_long / sw_db_align_matrix_long
 *   with an alignment mode (SW_MODE_*) before `out`; sw_align_matrix_long_coop_mode,
 *   sw_db_align_matrix_long_coop_mode: the same for the _long_coop calls.  SW_MODE_LOCAL through them is a
 *   call of the entry point without _mode.  In SW_MODE_GLOBAL and SW_MODE_SEMIGLOBAL the result equals,
 *   bit for bit, what sw_align_matrix_cpu_mode and sw_align_matrix_batch_mode return for the pair: score,
 *   the four coordinates and the operations; the end-cell rule and the walk priorities are the ones above,
 *   run on the same 4 bits a cell.  What differs from the local long path:
 *     the locate pass reads the end from column n - 1 (global: the corner), so the end is always in the last
 *       strip; on many waves only that strip's item stores an end record, and the host reads that one;
 *     every pair with two non-empty sequences walks, whatever its score (scores may be negative or 0); a pair
 *       with an empty sequence is answered on the host as under sw_align_matrix_batch_mode;
 *     a strip is filled again under the mode's borders: the top border H[512 s][-1] from the strip index, and
 *       for strip 0 the left border H[-1][j] as its inflow;
 *     the walk may leave the matrix at j < 0 in any strip: the leading I run then covers every strip still to
 *       the left and no further round is run for the pair (global: likewise the leading D run at i < 0).
 *   Refused before any device work: an unknown mode (-1, the message names the entry point); a pair over the
 *   SCORE RANGE bound above (the message names the pair or the record) -- the bound holds for a strip filled
 *   on its own over seq2 positions [0, j] as it does for the whole pair, which has no fewer steps; and
 *   whatever sw_align_long_plan refuses, with its text.  sw_align_long_plan and sw_align_long_coop_plan do
 *   not depend on the mode: the checkpoints, a strip's trace, the progress words, the records and the
 *   window are the same bytes in every mode.
 *   sw_last_stats: mode 8 (mode 12 for the _coop calls) as before, and the alignment mode in bits 28-29 of
 *   variant, the strip-fill launches below them, as mode 7 reports it; a local call reports what it did.
 *   Options trace_mb, long_window, blocks, timeout, coop_poison and SWMI_ALIGN_CKPT_MB as for the local calls. */
int  sw_align_matrix_long_mode(const sw_matrix*, const unsigned char* const* a, const int* alen,
                               const unsigned char* const* b, const int* blen, int npairs,
                               int gap_init, int gap_ext, int mode, sw_alignment* out,
                               unsigned* cigar, long long cigar_cap, long long* cigar_used);
int  sw_align_matrix_long_coop_mode(const sw_matrix*, const unsigned char* const* a, const int* alen,
                                    const unsigned char* const* b, const int* blen, int npairs,
                                    int gap_init, int gap_ext, int mode, sw_alignment* out,
                                    unsigned* cigar, long long cigar_cap, long long* cigar_used);
int  sw_db_align_matrix_long_mode(sw_db*, const sw_matrix*, const unsigned char* query, int qlen,
                                  const int* record_idx, int nidx, int gap_init, int gap_ext, int mode,
                                  sw_alignment* out, unsigned* cigar, long long cigar_cap, long long* cigar_used);
int  sw_db_align_matrix_long_coop_mode(sw_db*, const sw_matrix*, const unsigned char* query, int qlen,
                                       const int* record_idx, int nidx, int gap_init, int gap_ext, int mode,
                                       sw_alignment* out, unsigned* cigar, long long cigar_cap, long long* cigar_used);

/* ---- position-specific scoring: profiles ------------------------------------------
 * A PROFILE is n positions (1 <= n <= SW_PROFILE_MAX_LENGTH) over an alphabet of K <= 32 byte symbols, and a
 * table of entries in [-127, 127]: scores[i*K + c] is what symbol c of the sequence scores at position i.  The
 * alphabet is a matrix object's: `other`, SW_MATRIX_FOLD_CASE and the same 256-byte byte-to-code map.  A PSSM,
 * a family profile, a query with masked or up-weighted positions, a DNA query with degenerate positions are
 * such tables: the score of a cell depends on the query POSITION, not on a query residue.  A profile is
 * immutable and may be used from any thread at once.
 *
 * SEMANTICS.  The recurrence, the three modes (SW_MODE_*), the gap model, the end-cell rule, the walk and the
 * tie rules of sw_score_matrix_batch_mode / sw_align_matrix_batch_mode hold word for word with s(seq1[i], seq2[j])
 * replaced by P[i][code(seq[j])].  The profile is seq1, index i: an I consumes a profile position, beg1 and end1
 * are profile positions, and in SW_MODE_SEMIGLOBAL the profile is the query that is covered end to end.  The
 * sequence is seq2.  The profile is never laid on the streaming side (it has no bytes to stream).
 *
 * sw_profile_create: from a table of n*k entries, row-major by position.  NULL on error (sw_last_error): n < 1 or
 *   above SW_PROFILE_MAX_LENGTH (named), k outside 1..32, a duplicate symbol, a bad `other` or flags, an entry -128.
 * sw_profile_from_matrix: row i is the matrix row of query byte i, P[i][c] = T[code(q_i)][c], so that the profile
 *   calls give what the matrix calls give for that query as seq1.  A query byte outside the matrix alphabet is an
 *   error that names the position.
 * sw_profile_parse / sw_profile_open: a text format of this library's own (it is not any other tool's PSSM
 *   format): a line whose first token begins with '#' is a comment; the first other line is the header, K symbols
 *   of one byte each ('*' becomes `other`); every further line is one position: a one-byte label (the position's
 *   consensus residue: not read when scoring, and not '#') and K integers.  Any run of blanks separates tokens;
 *   CRLF and a missing final newline are accepted.  NULL with a message for a row that has not K entries, a label
 *   or symbol wider than a byte, a duplicate symbol, more than 32 symbols, an entry outside +-127, a token that
 *   is not an integer, no header, no rows, or more than SW_PROFILE_MAX_LENGTH rows.
 * sw_profile_length / sw_profile_size / sw_profile_symbols: n; K; the K bytes (returns K).
 * sw_profile_score: *out = P[pos][code(byte)]; -1 for a position outside [0, n) or a byte without a code.
 * sw_score_profile_batch: scores_out[k] = the score of the profile against seqs[k] in `mode`; one launch; 0 or -1.
 *   An empty sequence is answered on the host: 0 in SW_MODE_LOCAL, else the profile as one gap run,
 *   -(gap_init + (n - 1) * min(gap_ext, gap_init)).  Refused before anything is launched: an unknown mode, a
 *   sequence with min(n, len) * max(0, largest entry) >= 2^28, in the two other modes a sequence over the SCORE
 *   RANGE bound of sw_score_matrix_batch_mode with the profile as seq1, and a byte outside the alphabet (-1;
 *   sw_last_error names "sequence k", the position and the byte).
 *   The kernels are one more instantiation of the matrix kernels (sw_matrix.hip PROFILE): score-only at 1, 2, 4
 *   and 8 columns a lane, chosen by the matrix kernels' cost estimate (option "W" forces one); every wave keeps
 *   the rows of its strip's columns in an LDS slab of its own (9216 * W bytes a workgroup), copied before each
 *   strip from a device image of the profile, (n + 1) * 36 bytes uploaded on every call.  Option "blocks" is
 *   honoured.  sw_last_stats: mode 13, W, variant = the alignment mode, as mode 6.
 * sw_align_profile_batch: an alignment per sequence, by the traced instantiation (W = 8) and the matrix path's
 *   walk; out, cigar, cigar_cap, cigar_used and option "trace_mb" as sw_align_matrix_batch_mode, with n the
 *   profile's length.  A sequence whose trace does not fit trace_mb alone is refused: there is no long path
 *   with a profile.  sw_last_stats: mode 14, otherwise as mode 7.
 * sw_align_profile_cpu: the same arguments and, bit for bit, the same alignments from the host aligner of
 *   sw_align_matrix_cpu / sw_align_matrix_cpu_mode (n * len bytes a sequence, at most 2^32 cells).
 * sw_db_search_profile / sw_db_align_profile: as sw_db_search_matrix_mode / sw_db_align_matrix_mode with the
 *   profile in the query's place: nothing of it enters the arena.  The records are checked against the
 *   profile's alphabet once per (database, profile).
 * Not built: a band, the cooperative and the long paths with a profile; many profiles in one call;
 * position-specific gap penalties; building a profile from an alignment. */
typedef struct sw_profile sw_profile;
#define SW_PROFILE_MAX_LENGTH (1 << 22)
sw_profile* sw_profile_create(const unsigned char* symbols, int k, const signed char* scores /* n*k */, int n,
                              int other, int flags);
sw_profile* sw_profile_from_matrix(const sw_matrix*, const unsigned char* query, int qlen);
sw_profile* sw_profile_parse(const char* text, long long nbytes);
sw_profile* sw_profile_open(const char* path);
int  sw_profile_length(const sw_profile*);
int  sw_profile_size(const sw_profile*);
int  sw_profile_symbols(const sw_profile*, unsigned char* out /* k bytes */);
int  sw_profile_score(const sw_profile*, int pos, unsigned char byte, int* out);
void sw_profile_free(sw_profile*);
int  sw_score_profile_batch(const sw_profile*, const unsigned char* const* seqs, const int* lens, int nseq,
                            int gap_init, int gap_ext, int mode, int* scores_out);
int  sw_align_profile_batch(const sw_profile*, const unsigned char* const* seqs, const int* lens, int nseq,
                            int gap_init, int gap_ext, int mode, sw_alignment* out,
                            unsigned* cigar, long long cigar_cap, long long* cigar_used);
int  sw_align_profile_cpu(const sw_profile*, const unsigned char* const* seqs, const int* lens, int nseq,
                          int gap_init, int gap_ext, int mode, sw_alignment* out,
                          unsigned* cigar, long long cigar_cap, long long* cigar_used);
int  sw_db_search_profile(sw_db*, const sw_profile*, int gap_init, int gap_ext, int mode, int* scores_out);
int  sw_db_align_profile(sw_db*, const sw_profile*, const int* record_idx, int nidx, int gap_init, int gap_ext,
                         int mode, sw_alignment* out, unsigned* cigar, long long cigar_cap, long long* cigar_used);

/* ---- translated search: a protein query against DNA in six reading frames ----------
 * The tblastn / tfasty question: where does this protein occur in these DNA records?  seq1 is the protein
 * (the query), seq2 a reading frame of the DNA, translated by the kernel as it fetches: nothing is translated
 * ahead of time and the DNA stays in the arena as it is.
 *
 * BASES.  A byte's class: T, t, U, u = 0; C, c = 1; A, a = 2; G, g = 3; every other byte is ambiguous.  The
 *   complement of class x is x ^ 2.  Any byte is a legal DNA byte: the DNA is not checked against the matrix
 *   alphabet (and a database's record of checked matrices is not touched).
 * GENETIC CODE.  64 bytes, one amino-acid byte a codon, at index 16*b1 + 4*b2 + b3 over the classes above
 *   (NCBI's TCAG order).  A codon with an ambiguous base translates to 'X'; degenerate codons are NOT resolved
 *   (CTN is 'X', not 'L').  code64 = NULL is the standard code (sw_standard_code):
 *   FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG.
 * FRAMES.  +1, +2, +3, -1, -2, -3 (BLAST's numbering); arrays of six hold them in this order.  Frame +-k has
 *   offset o = k - 1 and m = (L - o) / 3 residues if L >= o + 3, else 0.  Residue r of a plus frame is the codon
 *   dna[3r+o .. 3r+o+2]; of a minus frame the codon comp(dna[L-1-3r-o]), comp(dna[L-2-3r-o]), comp(dna[L-3-3r-o])
 *   (the reverse complement read forward).
 * ALPHABET.  The matrix must score every byte the code can emit: the distinct bytes of the 64 and 'X', each a
 *   symbol of the matrix or covered by `other`.  A missing byte is refused before any launch and named.  The
 *   query is checked against the matrix as in every matrix call.
 * SCORING.  Everything else is the matrix path's: the recurrence, the gap model, the three modes (SW_MODE_*),
 *   the end-cell rule, the walk, the tie rules, and the range refusals with m the frame's residue count.  The
 *   query lies across the lanes, the frame streams: never swapped.  An empty frame or an empty query is
 *   answered on the host as an empty sequence is (local: 0 and an empty alignment).
 * COORDINATES.  beg2 / end2 of an alignment are residues of the frame.  [beg2, end2) covers the bases
 *   [3*beg2 + o, 3*end2 + o) in a plus frame, [L - o - 3*end2, L - o - 3*beg2) on the forward strand in a minus
 *   frame (sw_translated_range).
 *
 * sw_standard_code: the 64 bytes above.
 * sw_translate: out[0, m) = the residues of `frame` of dna[0, len) under code64 (NULL: standard); returns m, or
 *   -1 for a frame outside +-1..+-3, a null pointer, len < 0, or cap < m.  The single host statement of the
 *   rules above; with a minus frame it also gives the other direction (blastx): translate the DNA query into
 *   six protein queries and call the existing matrix search with each.
 * sw_translated_range: the DNA range of residues [beg2, end2) of `frame` of a DNA of `len` bases; -1 for a bad
 *   frame or a range outside the frame.
 * sw_translated_tables: what the kernel stages, composed from (matrix, code): base[256] the class of every byte
 *   (0..3, 4 = ambiguous) and codon[65] the matrix code of each codon's amino acid, entry 64 that of 'X'.  -1
 *   with the missing byte named when the matrix does not score a byte the code can emit.
 * sw_score_matrix_translated_batch: scores_out[6*k + f] = the score of a[k] against frame index f of dna[k] in
 *   `mode`; one launch of up to 6 * npairs items, longest first.  sw_last_stats: mode 15, variant the alignment
 *   mode, cells the sum of n * m over the frames; options "W" and "blocks" as mode 6.
 * sw_align_matrix_translated_batch: one alignment a pair, in the frame frames[k] names (+-1..+-3), by the traced
 *   instantiation (W = 8) and the matrix path's walk; sw_alignment as it is, in residues of the frame.  A pair
 *   whose trace does not fit trace_mb alone is refused: there is no long path here.  sw_last_stats: mode 16.
 * sw_align_matrix_translated_cpu: the same arguments and, bit for bit, the same alignments: sw_translate, then
 *   the host aligner of sw_align_matrix_cpu_mode.
 * sw_db_search_matrix_translated: scores_out[6*r + f] for every record r of a DNA database, out of the arena.
 * sw_db_align_matrix_translated: the query aligned with frame frames[k] of record record_idx[k].
 * Every refusal names the call: a frame outside +-1..+-3, a null pointer, a DNA longer than 2^27 - 1 bases, a
 *   byte of the code the matrix does not score, a pair whose trace does not fit.
 * Not built: band=, coop=, the long path and profiles against translated frames; many queries in one call;
 *   degenerate-codon resolution; frameshift-aware alignment; start-codon tables; a both-strand
 *   nucleotide-against-nucleotide search; 16-bit packing. */
void sw_standard_code(unsigned char out[64]);
int  sw_translate(const unsigned char* dna, int len, int frame, const unsigned char* code64, unsigned char* out, int cap);
int  sw_translated_range(int len, int frame, int beg2, int end2, int* dna_beg, int* dna_end);
int  sw_translated_tables(const sw_matrix*, const unsigned char* code64, unsigned char base_out[256],
                          unsigned char codon_out[65]);
int  sw_score_matrix_translated_batch(const sw_matrix*, const unsigned char* const* a, const int* alen,
                                      const unsigned char* const* dna, const int* dlen, int npairs, int gap_init,
                                      int gap_ext, int mode, const unsigned char* code64, int* scores_out /* 6*npairs */);
int  sw_align_matrix_translated_batch(const sw_matrix*, const unsigned char* const* a, const int* alen,
                                      const unsigned char* const* dna, const int* dlen, const int* frames, int npairs,
                                      int gap_init, int gap_ext, int mode, const unsigned char* code64, sw_alignment* out,
                                      unsigned* cigar, long long cigar_cap, long long* cigar_used);
int  sw_align_matrix_translated_cpu(const sw_matrix*, const unsigned char* const* a, const int* alen,
                                    const unsigned char* const* dna, const int* dlen, const int* frames, int npairs,
                                    int gap_init, int gap_ext, int mode, const unsigned char* code64, sw_alignment* out,
                                    unsigned* cigar, long long cigar_cap, long long* cigar_used);
int  sw_db_search_matrix_translated(sw_db*, const sw_matrix*, const unsigned char* query, int qlen, int gap_init,
                                    int gap_ext, int mode, const unsigned char* code64, int* scores_out /* 6*records */);
int  sw_db_align_matrix_translated(sw_db*, const sw_matrix*, const unsigned char* query, int qlen, const int* record_idx,
                                   const int* frames, int nidx, int gap_init, int gap_ext, int mode,
                                   const unsigned char* code64, sw_alignment* out, unsigned* cigar, long long cigar_cap,
                                   long long* cigar_used);

/* Tuning knobs (process-wide).  Keys:
 *   "W"        columns per lane: 0 = auto, 1, 2, 4, 8
 *   "C"        rows per strip hand-off chunk: 0 = auto, 16, 32, 64
 *   "bytes"    1 = force the raw-byte path
 *   "timeout"  seconds before a stalled strip hand-off gives up (default 30)
 *   "blocks"   0 = auto persistent grid, else workgroups per launch
 *   "orient"   0 = auto, 1 = seq1 spread across lanes, 2 = seq2 across lanes
 *   "mode"     -1 = auto, 0 = independent strip waves, 1 = workgroup per pair,
 *              2 = lock-step strip groups (single long pairs),
 *              3 = packed 16-bit pair duos (MATCH >= 0, batches with scores < 65535: DNA, and any bytes
 *                  when MISMATCH < 0 and MATCH - MISMATCH <= 127, option duo_raw),
 *              4 = free-running strip groups, rows staged in LDS (long DNA pairs),
 *              5 = the flow2 / flow3 wavefront step (DNA, one column per lane or more, chunked
 *                  LDS / granule hand-offs; the automatic plan for single long pairs, column
 *                  slabs and batches whose scores need int32)
 *              (sw_last_stats also reports mode 6 = wave per pair, substitution matrix: the
 *              sw_*_matrix entry points, which honour "blocks" and "W" only; and mode 7 = the
 *              traced launches of sw_align_matrix_batch / sw_db_align_matrix: "blocks", "trace_mb";
 *              and mode 8 = their _long counterparts, which honour the same two; and modes 9 and 10 =
 *              the band launches, score-only and traced: sw_*_band, as modes 6 and 7; and modes 13 and 14 =
 *              the profile launches, score-only and traced: sw_*_profile_*, as modes 6 and 7; and modes 15 and
 *              16 = the translated launches, score-only and traced: sw_*_matrix_translated*, as modes 6 and 7)
 *   "trace_mb" MiB of trace memory one traced launch may hold, 1..3072 (default 1024)
 *   "duo16"    1 = (default) packed duos take max3 through v_pk_maximum3_f16 when every
 *              value stays below 0x7C00 (MATCH*(min(n,m)+1) <= 31743), 0 = u16 max only
 *   "linear"   -1 = (default) the exact linear-gap step when G_INIT == G_EXT
 *              (flow2 C = 32 or 64, f16 duos), 0 = always the affine step
 *   "f2w"      flow2 columns per lane: 0 = (default) two whenever the linear-gap
 *              step runs (three in flow3 ring mode: C5, column slabs), one otherwise;
 *              1 = always one; 2 = two (linear-gap step only); 3 = three where ring mode runs;
 *              4 = four / five in ring mode for one pair, every strip group resident in one round
 *              (sw_flow3r45_kernel; measured slower than three on C5, so never automatic)
 *   "f3pool"   1 = flow3 staged launches on the loops without the I/O rotation (measured
 *              slower; default 0)
 *   "ring"     -1 = (default) ring edges for a single flow2 pair whose linear edges
 *              would exceed 1 GB, 0 = never, 1 = always (one pair per launch)
 *   "ring_rows" rows per within-round ring, a power of two in [512, 2^20] (4096)
 *   "f2_wgs"   flow2 streamed kernel: workgroups per CU, 0 = auto, 1..4 (ring mode:
 *              lowered to what the runtime reports resident for its kernel)
 *   "f2stream" 1 = flow2 streams the row codes even when they fit in LDS (tests)
 *   "f2pwg"    DNA batches whose scores need int32 (no 16-bit duos): -1 = (default) the
 *              flow2 step with a pair per workgroup when its constants fit, 0 = never
 *              (the pair-per-workgroup strip kernel), 1 = also for a forced mode 5 batch
 *   "f3"       1 = (default) a two-column linear-gap flow2 launch runs the flow3 kernel
 *              (hand-scheduled chunk loops): staged codes at C = 32 / 16 (C2), ring edges at
 *              C = 64 (C5); 0 = the compiled flow2 kernel
 *   "f3hl"     1 = (default) flow3 staged launches run 32-row chunks whose in-workgroup links
 *              hand off every half chunk (16 rows); 0 = whole-chunk links at C = 16 (auto C)
 *   "f3rhl"    1 = flow3 ring launches (C = 64) with half-chunk in-workgroup links (32 rows),
 *              0 = (default) whole-chunk links (measured faster on C5)
 *   "f3a"      1 = (default) the general affine step runs on flow3 (staged: sw_flow3a_kernel, one
 *              column per lane, C2 with G_INIT != G_EXT; ring: sw_flow3ra(3)_kernel, C5), 0 = flow2
 *   "f3split"  one pair on the staged two-column linear-gap flow3 kernel (C2) cut at a column and scored
 *              from both ends at once, the right half on both sequences mirrored, joined by a small
 *              combine kernel (sw_split_bounds): -1 = (default) automatic, for pairs at least the
 *              measured threshold wide; 0 = never; 1 = whenever each half gets two strips (n >= 379).
 *              Traced launches (option trace), ring mode, slabs, batches and the affine step run uncut.
 *              Under -1 a pair tall and wide enough is scored as two wedges cut along an anti-diagonal
 *              staircase instead (variant bit 18; 0 switches that off too, 1 keeps the column cut); the
 *              environment variable SWMI_F3WEDGE (0 = never, 1 = wherever every strip keeps 64 rows)
 *              overrides the measured thresholds for A/B runs and tests, and SWMI_F3WEDGE_DROPS =
 *              d0,d1,d2,d3 sets the staircase's drop behind strip j to d[j % 4] rows wherever the steep
 *              plan admits it (variant bit 19; multiples of 64 from 64 to 256 with d0 == d2, anything
 *              else fails the launch; 64,64,64,64 is the uniform staircase; unset: the measured default).
 *              A two-wedge launch is one kernel: the staged kernel joins the chains itself, carries the two
 *              descriptors in its arguments and neither copies nor clears anything first.  The environment
 *              variable SWMI_F3JOIN = 0 (A/B runs and tests) keeps the earlier launch instead: descriptor
 *              copies, memsets of the claim counter and the score, and a combine kernel behind the staged one.
 *              SWMI_F3WEDGE_TRACE = 1 lets a traced launch (option trace) keep its two wedges: the trace buffer
 *              then holds 16 words at row chain * S + strip, S the strips a chain (tools/trace_wedge.py)
 *   "f3pwg"    1 = (default) DNA batches on a pair-per-workgroup plan (scores that need int32, or 1-2
 *              pairs per CU) run flow3's three-column ring step (sw_flow3r3p / ra3p_kernel), 0 = flow2's
 *   "f3slab"   1 = (default) column slabs run flow3's ring kernel with slab roles
 *              (sw_flow3rs / ras / r3s / ra3s_kernel), 0 = flow2's slab kernel
 *   "duo_lds"  1 = (default) duo batches at C = 64 hand strip edges on in LDS when a round's
 *              rows fit (m <= 16384 linear-gap step, 8192 affine), 0 = through HBM granules
 *   "duo_roles" 1 = (default) the two duo LDS workgroups of a CU take complementary strip roles
 *              on each SIMD (one wave starts early, one late), 0 = roles by wave index
 *   "duo_tab"  1 = (default) the duo LDS kernel reads its row codes from an LDS table (4 or 8
 *              columns per lane, when the table and the wrap buffer fit two workgroups per CU
 *              and the duos run in one pass at that), 2 = whenever it fits, 0 = the codes travel
 *              lane to lane by DPP
 *   "hep"      1 = (default) one pair over at most seven byte values not all in {A,C,G,T} (ACGTN,
 *              lower case, RNA) runs flow3's staged kernels with 3-bit row symbols (sw_flow3h /
 *              sw_flow3ah_kernel; rows that fit in LDS, else the byte path), 0 = the byte path
 *   "duo_raw"  1 = (default) byte batches (any byte outside {A,C,G,T}: protein, N, lower case) run the
 *              duo kernels with the penalty from the bytes (one XOR and one v_pk_min_u16 per position
 *              for the DNA step's v_perm_b32; needs MISMATCH < 0, MATCH - MISMATCH <= 127), 0 = the
 *              byte-path strip kernels
 *   "duo_prio" -1 = (default) auto: 17 for the duo LDS kernel with the row-code table, else 0;
 *              k in 6..20: a CU's two duo workgroups take turns at issue priority (s_setprio) in
 *              slices of 2^k ticks (10 ns) of the clock from their start; 0 = off (timing only)
 *   "slab_plain" 1 = an exported slab buffer may fall back to plain device memory (one-GPU
 *              tests only; cross-GPU edges need fine-grained memory), 0 = (default) refuse
 *   "trace"    device address of a 16 x u64 per-strip trace buffer, 0 = off (tools)
 *   "stall_item" tests only: flow2's compute waves skip this item (its edges are never
 *              published, so its consumers' bounded waits expire: ERR_TIMEOUT); -1 = (default) none
 * Returns 0, or -1 for an unknown key / bad value. */
int sw_set_option(const char* key, long long value);
long long sw_get_option(const char* key);
/* The keys above, in the library's own order: key i for 0 <= i < their number, else NULL. */
const char* sw_option_name(int i);

/* Details of the last launch made by this thread (for the harness / bench). */
typedef struct {
    float kernel_ms;        /* HIP-event time of the score kernel alone */
    float total_ms;         /* wall time of the whole call incl. copies */
    long long cells;        /* sum of n*m over the launched pairs */
    int W, C, dna, blocks, waves_per_cu, items;
    long long boundary_bytes;
    int mode;
    int variant;            /* (mode 6: the alignment mode SW_MODE_*; mode 7: launches in bits 0-27, the alignment
                               mode in bits 28-29; mode 8: strip-fill launches; modes 9 and 10: as 6 and 7, and
                               cells = the cells in the bands; the bits below are the engine's)
                               bit 0: duo max3 via v_pk_maximum3_f16; bit 1: flow2 streams row codes;
                               bit 2: flow2 ring edges; bit 3: the linear-gap step;
                               bit 4: flow2 two columns per lane; bit 5: flow2 pair per workgroup;
                               bit 6: the flow3 kernel (sw_flow3.hip);
                               bit 7: duo strip hand-offs in LDS (no boundary buffers);
                               bit 8: duo row codes from an LDS table;
                               bit 9: flow3 half-chunk LDS links (option f3hl);
                               bit 10: the general affine step on flow3 (sw_flow3a / sw_flow3ra kernels);
                               bit 11: a flow3 column slab (peer-edge roles, sw_flow3*s_kernel);
                               bit 12: flow3 pool loops (option f3pool);
                               bit 13: flow3 ring at three columns per lane (sw_flow3r3 / ra3 kernels);
                               bit 14: flow3 ring at four / five columns per lane (sw_flow3r45_kernel);
                               bit 15: flow3 three-column ring step with a pair per workgroup
                                       (sw_flow3r3p_kernel / sw_flow3ra3p_kernel: int32 batches);
                               bit 16: a pair over up to seven byte values on flow3's staged kernels
                                       (option hep; dna = 2 then);
                               bit 17: one pair cut at a column, both halves in one launch (option f3split;
                                       items and blocks count both halves);
                               bit 18: one pair scored as two wedges cut along an anti-diagonal staircase,
                                       both chains in one launch (automatic under option f3split = -1;
                                       items and blocks count both chains);
                               bit 19: with bit 18, the steep plan: a staircase that drops more than 64
                                       rows behind some strips, joined along the strips' hand-off
                                       columns too (environment SWMI_F3WEDGE_DROPS forces a pattern) */
} sw_stats;
int sw_last_stats(sw_stats* out);

const char* sw_last_error(void);
int sw_version(void);

/* Synthetic {A,C,G,T} inputs (not on the score path): std::mt19937_64(seed),
 * a[i] then b[i] per position -- the generator of cudaSmithM.cu:200-212. */
void sw_gen_pair(uint64_t seed, int len, unsigned char* a, unsigned char* b);
/* npairs pairs, pair k seeded seed_base+k, laid out [a_0|b_0|a_1|b_1|...]. */
void sw_gen_batch(uint64_t seed_base, int npairs, int len, unsigned char* arena);

#ifdef __cplusplus
}
#endif

#endif /* SWMI355_ALGOGPU_H */
