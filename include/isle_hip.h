/* include/isle_hip.h — C ABI of libisle_hip.so: the MI355X (gfx950) implementation of ISLE's
 * training hot path (truncated SVD of the thresholded word-document matrix B by restarted block
 * Krylov-Schur on B*B^T, k-means++ / Lloyd in the projected space, lift, Lloyd on sparse B).
 *
 * This is the drop-in boundary: each entry point replaces one public method of the reference's
 * ISLE::FPSparseMatrix<float> (or the ProdOp plug-in of BlockKs) — cited per function as
 * file:line relative to the reference root.  The reference-side binding a maintainer would add
 * is shown in INTEGRATION.md.
 *
 * Conventions
 *  - plain C types only; every function returns 0 on success or a negative ISLE_E_* code and
 *    records a message retrievable with isle_hip_last_error(); no exception crosses the ABI.
 *  - all pointers are HOST pointers owned by the caller unless a name ends in _dev.
 *  - one context = one GPU = one process (multi-GPU: one process per GPU, documents
 *    column-sharded; see isle_hip_comm_init).  A context is not thread-safe.
 *  - matrices named *_colmajor are column-major with leading dimension = number of rows, as
 *    in the reference (Armadillo fmat / cblas ColMajor).
 *  - there is NO CPU fallback: without a visible gfx950 device isle_hip_create fails.
 */
#ifndef ISLE_HIP_H
#define ISLE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct isle_ctx isle_ctx;

enum {
  ISLE_OK = 0,
  ISLE_E_ARG = -1,      /* bad argument / state */
  ISLE_E_HIP = -2,      /* HIP runtime error */
  ISLE_E_NOCONV = -3,   /* eigensolver exhausted maxit restarts (Ritz values still returned) */
  ISLE_E_NUMERIC = -4,  /* breakdown: rank repair / small EVD failed */
  ISLE_E_COMM = -5      /* RCCL error */
};

/* ---- context --------------------------------------------------------------------------- */
/* Creates a context on HIP device `device_id`.  Returns NULL (and prints to stderr) on failure. */
isle_ctx* isle_hip_create(int device_id);
void isle_hip_destroy(isle_ctx* ctx);
const char* isle_hip_last_error(isle_ctx* ctx);

/* Multi-GPU (documents column-sharded, one process per GPU).  rank 0 calls
 * isle_hip_comm_unique_id (128 bytes), distributes the bytes by any host channel
 * (bench.py uses torch.distributed), then every rank calls isle_hip_comm_init.
 * doc_offset / docs_global place this rank's shard in the global column numbering. */
int isle_hip_comm_unique_id(void* out128);
int isle_hip_comm_init(isle_ctx* ctx, int world_size, int rank, const void* unique_id128);

/* Rehearsal transport for tests: RCCL refuses two ranks on one device, so to run the sharded path with several
 * ranks on ONE GPU (tests/test_gpu_multirank.py) every collective is staged through host memory and handed to
 * `fn` (the tests pass a torch.distributed/gloo exchange).  kind: ISLE_XCHG_*; dtype: 0 f32, 1 f64, 2 i32, 3 u32,
 * 4 u64.  All-reduce: `buf` holds `count` elements, reduced in place.  All-gather: `buf` holds world * count
 * elements with this rank's part already at rank * count; fill the rest.  Return 0 on success.  Collectives then
 * cost two PCIe copies and two stream synchronisations each: never use it for measurements (bench.py does not). */
enum { ISLE_XCHG_ALLREDUCE_SUM = 0, ISLE_XCHG_ALLREDUCE_MAX = 1, ISLE_XCHG_ALLGATHER = 2 };
typedef int (*isle_host_exchange_fn)(void* user, int kind, void* buf, uint64_t count, int dtype);
int isle_hip_comm_init_host(isle_ctx* ctx, int world_size, int rank, isle_host_exchange_fn fn, void* user);

/* Contiguous, nnz-balanced document ranges for `parts` shards (pure host function, no GPU):
 * bounds[p] .. bounds[p+1] are the columns of shard p; bounds has parts+1 entries. */
int isle_hip_plan_shards(uint64_t num_docs, const int64_t* offsets_CSC, int parts, uint64_t* bounds);

/* ---- input: the matrix B -------------------------------------------------------------- */
/* Uploads this rank's column shard of B (CSC: vals_CSC / rows_CSC / offsets_CSC of
 * include/sparseMatrix.h:23-56; rows ascending within a column, as threshold_and_copy builds
 * them, src/sparseMatrix.cpp:1328-1361).  `num_docs` columns local to this rank;
 * offsets[0] == 0, offsets[num_docs] == nnz.  rows are the reference's 8-byte word_id_t
 * (include/types.h:24) in the _u64 flavour, or 4-byte in the _u32 flavour.
 * doc_offset = global id of local column 0, docs_global = total columns over all ranks
 * (pass 0 and num_docs for single-GPU). */
int isle_hip_upload_csc_u64(isle_ctx* ctx, uint64_t vocab_size, uint64_t num_docs, uint64_t nnz,
                            const float* vals, const uint64_t* rows, const int64_t* offsets,
                            uint64_t doc_offset, uint64_t docs_global);
int isle_hip_upload_csc_u32(isle_ctx* ctx, uint64_t vocab_size, uint64_t num_docs, uint64_t nnz,
                            const float* vals, const uint32_t* rows, const int64_t* offsets,
                            uint64_t doc_offset, uint64_t docs_global);

/* ---- upstream stage: thresholding on the device ------------------- */
/* Uploads this rank's column shard of A, the word-document COUNT matrix in CSC as
 * SparseMatrix<T>::populate_CSC builds it (src/sparseMatrix.cpp:58-133: rows ascending within a
 * column, duplicates merged, counts > 0).  doc_offset / docs_global as for isle_hip_upload_csc. */
int isle_hip_upload_counts_u32(isle_ctx* ctx, uint64_t vocab_size, uint64_t num_docs, uint64_t nnz,
                               const float* counts, const uint32_t* rows, const int64_t* offsets,
                               uint64_t doc_offset, uint64_t docs_global);

/* tdf ingest on the device: DocWordEntriesReader::fill_doc_word_entries
 * (include/utils.h:158-228) + the sort / de-duplication of ISLETrainer::finalize_data
 * (src/trainer.cpp:236-247) + SparseMatrix::populate_CSC (src/sparseMatrix.cpp:58-87).
 * `text`: the bytes of a tdf file ("<doc> <word> <count>" per line, 1-based ids, blanks or tabs between
 * fields, optional '\r', last newline optional).  The result is this context's count matrix, exactly
 * as if it had been passed to isle_hip_upload_counts_u32 (single rank: doc_offset 0).  max_entries:
 * the reference asserts the file holds exactly that many lines; 0 = do not check.  Of several
 * lines with the same (doc, word) the first in the file survives (the reference keeps an unspecified
 * one).  entries_read / nnz (nullable): lines parsed / entries after de-duplication.
 * ISLE_E_ARG, with the kind and the 1-based number of the first bad line of the file: a character other than
 * a digit, blank, tab, '\r' or '\n'; more or fewer than three fields; a doc / word id that is 0 or exceeds
 * num_docs / vocab_size; a count of 0; a count that exceeds 4294967295 (counts are held in 32 bits before
 * they become floats).  Fields are read exactly, whatever their length: none wraps into range. */
int isle_hip_ingest_tdf(isle_ctx* ctx, const char* text, uint64_t nbytes, uint64_t vocab_size, uint64_t num_docs,
                        uint64_t max_entries, uint64_t* entries_read, uint64_t* nnz);
/* The count matrix from (doc, word, count) triples in any order, fed in batches: what ISLETrainer::feed_data / finalize_data
 * (src/trainer.cpp:214-371) do, with the sort, the de-duplication and the offsets on the device (the tail of isle_hip_ingest_tdf).
 * feed_begin opens a feed for a vocab_size x num_docs matrix (both 1 .. 0xfffffff0), discarding an open one; the context's
 * current count matrix stays as it is until feed_finalize.  reserve_entries: capacity hint (0 allowed); the entry store doubles
 * when a batch does not fit.
 * feed_entries: n entries, docs[i] the 0-based local column, words[i] the 0-based word id, counts[i] the count; the arrays are
 * the caller's again when the call returns; n == 0 is a no-op; batches of any size (large ones are cut inside).  An entry with
 * count 0 is skipped and takes no part in duplicate resolution.  A batch is taken whole or not at all: with docs[i] >= num_docs
 * or words[i] >= vocab_size anywhere in it (entries with count 0 included) the call returns ISLE_E_ARG, the message names
 * "document" or "word" and the 0-based ordinal of the first such entry, counted over every entry offered since feed_begin
 * (skipped ones included, rejected batches not), and the feed stays open holding what it held before the call.
 * feed_finalize: entries sorted by (doc, word); of several with the same (doc, word) the one offered first stays (call order,
 * then index); offsets with the empty documents.  The result is this context's count matrix exactly as if it had been passed to
 * isle_hip_upload_counts_u32 with the same doc_offset / docs_global (0 / 0 on a single rank), and the feed is released.
 * entries_fed / nnz (nullable): entries kept before / after de-duplication.  A feed without entries gives num_docs empty columns.
 * Allowed with several ranks: each feeds its own shard under local column numbers, no collective is involved.
 * ISLE_E_ARG: feed_entries / feed_finalize without an open feed, a null array with n > 0.  After an allocation or device
 * failure the feed is discarded. */
int isle_hip_feed_begin(isle_ctx* ctx, uint64_t vocab_size, uint64_t num_docs, uint64_t reserve_entries);
int isle_hip_feed_entries(isle_ctx* ctx, uint64_t n, const uint32_t* docs, const uint32_t* words, const uint32_t* counts);
/* isle_hip_feed_entries with the size of the pieces a batch is cut into given (0, or anything above the library's own 2^26 entries:
 * that size).  The result does not depend on it; it exists so that the cutting, the ordinals across pieces and the whole-batch
 * refusal can be tested on small batches. */
int isle_hip_feed_entries_pieces(isle_ctx* ctx, uint64_t n, const uint32_t* docs, const uint32_t* words, const uint32_t* counts,
                                 uint64_t piece_entries);
int isle_hip_feed_finalize(isle_ctx* ctx, uint64_t doc_offset, uint64_t docs_global, uint64_t* entries_fed, uint64_t* nnz);
/* The count matrix from tdf text that arrives in pieces: isle_hip_ingest_tdf without holding the text, on the host or on the device.
 * Let T be the concatenation of all bytes committed or written between tdf_begin and tdf_finalize.  Pieces may be cut anywhere: inside a
 * field, between '\r' and '\n', inside a run of blanks, one byte at a time.  After a successful tdf_finalize the context's count matrix,
 * entries_read and nnz are exactly what isle_hip_ingest_tdf(T, ..., max_entries) would have produced; where that call would fail, the stream
 * fails with ISLE_E_ARG, the same wording of the kind and the same 1-based line number of T ("<kind> on line <n>": lines are counted over
 * every '\n' since tdf_begin, blank lines included), and a max_entries mismatch reads as it does there.  A line may be of any length,
 * longer than a piece or than many; such a line is scanned again with every piece it outlasts, so its cost grows with the square of its
 * length.  Single rank only; vocab_size and num_docs 1 .. 0xfffffff0.
 * tdf_begin opens a stream, discarding an open stream or an open feed of triples (isle_hip_feed_begin likewise discards an open stream):
 * the two share one entry store and exclude each other, so isle_hip_feed_entries / feed_finalize on a text stream, and the tdf calls on a
 * feed or with no stream open, are ISLE_E_ARG.  reserve_entries: capacity hint for the store (0 allowed; it doubles when a piece might not
 * fit).  piece_bytes: 0 = the library's own piece size (16 MiB); a smaller value is honoured down to 1 (the result does not depend on it:
 * it exists so that tests can put cuts everywhere), a larger one means the library's own.  The context's current count matrix stays valid
 * until tdf_finalize succeeds: every check (last line, max_entries) comes before the sort installs anything.
 * tdf_acquire hands out one of the stream's two page-locked buffers, *cap = the piece size, for the caller to read or copy text into;
 * tdf_commit(nbytes) gives it back with its first nbytes bytes as the next piece (0: nothing is added).  At most one buffer is outstanding:
 * a second acquire, a commit without one and nbytes > cap are ISLE_E_ARG and leave the stream as it was.  tdf_commit queues the copy and the
 * piece's kernels and returns without waiting for them; it waits for the piece BEFORE, whose line, entry and carry counts (read back through
 * page-locked memory) size this one.  So one piece is on the device while the caller fills the other buffer, and tdf_acquire never waits
 * for more than that.  tdf_write is acquire, memcpy, commit in a loop for bytes that are elsewhere; they are the caller's again when it
 * returns.
 * Because the device trails the calls, the first bad line is reported by whichever of commit, write or finalize learns of it first, by
 * finalize at the latest; it is always the first bad line of T (pieces are parsed in order, the error word is an atomic minimum over
 * (line, kind)).  After an error, or an allocation or device failure, the stream is discarded: later tdf calls find no open stream.
 * tdf_finalize parses what stands behind the last '\n' as the last line, checks max_entries (0 = do not), then sorts, de-duplicates (the
 * first in T of equal (doc, word) pairs stays) and builds the offsets as isle_hip_feed_finalize does.  entries_read / nnz: nullable.  An empty
 * stream gives num_docs empty columns.  Device memory beyond the entry store (12 bytes an entry) and the sort's twin depends on the piece
 * size alone, about 34 bytes per byte of a piece: a piece of n bytes may hold n lines, and the host cannot ask how many without waiting. */
int isle_hip_tdf_begin(isle_ctx* ctx, uint64_t vocab_size, uint64_t num_docs, uint64_t reserve_entries, uint64_t piece_bytes);
int isle_hip_tdf_acquire(isle_ctx* ctx, char** buf, uint64_t* cap);
int isle_hip_tdf_commit(isle_ctx* ctx, uint64_t nbytes);
int isle_hip_tdf_write(isle_ctx* ctx, const char* bytes, uint64_t nbytes);
int isle_hip_tdf_finalize(isle_ctx* ctx, uint64_t max_entries, uint64_t* entries_read, uint64_t* nnz);
/* One tdf file onto document shards, in two passes over the file, without any rank holding the corpus (the reference reads the file on one
 * host, include/utils.h:158-228, and sorts it there, src/trainer.cpp:236-247; isle_hip_tdf_begin stays single-rank).  Pieces travel through
 * tdf_acquire / tdf_commit / tdf_write as above.
 * Pass 1, tdf_begin_counts ... tdf_finalize_counts: a stream that counts the valid lines of every document into a table of num_docs 32-bit
 * counters on the device and holds no entry.  Each rank streams its own part of the file, whole lines only: rank r of N takes the lines
 * whose first byte lies in [size * r / N, size * (r + 1) / N) (tdf_pump::file_range, isle_amd/host/tdf_pump.h).  The counting stream refuses
 * nothing about the text: a bad line is not counted, since line numbers inside a byte range are not the file's; pass 2 names the first bad
 * line of the whole file.  tdf_finalize_counts counts what stands behind the last '\n' as the last line and ends the stream.  With several
 * ranks it is collective: agree_tag (the file's size) must be alike on all ranks, or all of them return ISLE_E_COMM; the table is summed
 * over the ranks, and so is the line count.  More than 4294967295 lines in all are ISLE_E_ARG (a summed counter might have wrapped).
 * bounds (parts + 1 values): bounds[p] .. bounds[p + 1] are the documents of shard p, by the rule of isle_hip_plan_shards applied to the line
 * counts: bound p is the first document at or behind p / parts of the lines.  The balance is by lines, repeated (doc, word) pairs included,
 * not by nnz after de-duplication.  parts need not be the number of ranks: one process may plan for N.  doc_lines (nullable, num_docs
 * values): the table.  lines_local / lines_global (nullable): valid lines this rank streamed / all ranks streamed.
 * Pass 2, tdf_begin_window ... tdf_finalize: a text stream over the WHOLE file that keeps the entries of documents doc_begin <= doc <
 * doc_end (0-based) only.  Allowed with any number of ranks; no collective is inside it.  Every line is parsed and checked as by
 * tdf_begin: the first bad line of the file, its number and its kind are what isle_hip_ingest_tdf reports.  tdf_finalize checks max_entries
 * against the valid lines of the whole text and returns that number as entries_read.  The result is the columns [doc_begin, doc_end) of what
 * isle_hip_ingest_tdf of the same bytes gives, offsets rebased, bit for bit: num_docs of the context's count matrix is doc_end - doc_begin,
 * its doc_offset doc_begin, its docs_global num_docs (src/sparseMatrix.cpp:58-87 per shard).  doc_begin == doc_end gives a matrix of zero
 * columns.  The sort runs over ceil(log2(doc_end - doc_begin)) document bits, and device memory follows the shard: 12 bytes per held entry.
 * What is replicated: every rank reads and parses the whole file in pass 2. */
int isle_hip_tdf_begin_counts(isle_ctx* ctx, uint64_t vocab_size, uint64_t num_docs, uint64_t piece_bytes);
int isle_hip_tdf_finalize_counts(isle_ctx* ctx, int parts, uint64_t agree_tag, uint64_t* bounds, uint32_t* doc_lines, uint64_t* lines_local,
                                 uint64_t* lines_global);
int isle_hip_tdf_begin_window(isle_ctx* ctx, uint64_t vocab_size, uint64_t num_docs, uint64_t doc_begin, uint64_t doc_end,
                              uint64_t reserve_entries, uint64_t piece_bytes);
/* Copies the context's count matrix to the host (any pointer may be NULL); nnz via the call above
 * or offsets[num_docs]. */
int isle_hip_get_A(isle_ctx* ctx, float* counts, uint32_t* rows, int64_t* offsets);

/* normalize_docs (src/sparseMatrix.cpp:136-167) + list_word_freqs / compute_thresholds (:289-485)
 * + FPSparseMatrix(A, zetas) = threshold_and_copy (:1285-1361), or sampled_threshold_and_copy
 * (:1365-1435) when 0 < sample_rate < 1 — what ISLETrainer::train does at src/trainer.cpp:430-485.
 * B is built in device memory and becomes the context's matrix exactly as if it had been passed
 * to isle_hip_upload_csc (empty columns removed; its doc_offset / docs_global follow from the
 * shards' surviving column counts).  Thresholds use the GLOBAL corpus (token total, non-empty
 * documents and per-word histograms are all-reduced).  Sampling keys are drawn on the host from
 * sample_seed and the document's GLOBAL number (the reference uses unseeded rand()); with several
 * ranks all keys are gathered and every rank selects the same pivot, so the shards keep what a
 * single-rank run keeps.
 * Outputs (any may be NULL): docs_kept / nnz_kept describe this rank's shard of B;
 * entries_above_threshold is the global count before sampling (the reference's log line);
 * avg_doc_sz as computed at src/sparseMatrix.cpp:98. */
int isle_hip_threshold(isle_ctx* ctx, uint64_t num_topics, double sample_rate, uint64_t sample_seed,
                       uint64_t* docs_kept, uint64_t* nnz_kept, uint64_t* entries_above_threshold,
                       float* avg_doc_sz);

/* Copies the context's B (and, after isle_hip_threshold, original_cols[D] = global column of A
 * behind each column of B and zetas[V]) to the host; any pointer may be NULL.  Sizes: query with
 * isle_hip_shape. */
int isle_hip_get_B(isle_ctx* ctx, float* vals, uint32_t* rows, int64_t* offsets,
                   uint64_t* original_cols, float* zetas);
int isle_hip_shape(isle_ctx* ctx, uint64_t* vocab_size, uint64_t* num_docs, uint64_t* nnz,
                   uint64_t* doc_offset, uint64_t* docs_global);

/* FPSparseMatrix::frobenius  src/sparseMatrix.cpp:1096-1100  (sum of squares of all entries,
 * over all ranks). */
int isle_hip_frobenius(isle_ctx* ctx, float* out);

/* ---- eigensolver ----------------------------------------------------------------------- */
/* ProdOp::multiply of MKL_SpSpTrProd  include/matUtils.h:336-365:
 * Z (V x b, col-major) = B * (B^T * X), X V x b col-major, 1 <= b <= 32. */
int isle_hip_gram_apply(isle_ctx* ctx, const float* X_colmajor, int b, float* Z_colmajor);

/* Which form of the operator the last build chose for the current B (the operator is built by the first
 * isle_hip_gram_apply / isle_hip_block_ks after an upload, like the MKL_SpSpTrProd constructor
 * include/matUtils.h:52-273): *form = 1 LDS-banded form (every row of B holds one value, as threshold_and_copy
 * src/sparseMatrix.cpp:1285-1321 produces), 0 gather form (any CSC matrix), -1 not built yet.
 * Environment ISLE_GRAM_LDS=0 forces the gather form. */
int isle_hip_operator_form(isle_ctx* ctx, int* form);

/* The environment switches the library honours (no reference counterpart: the reference's choices are compile-time macros,
 * include/hyperparams.h).  Every switch is in ONE table (isle_amd/csrc/common.h IsleKnob); entry `index` of it: its name, its kind
 * ("form": selects between exact forms of one computation, "tuning", "diagnostic", "test hook") and a sentence on its effect.
 * Returns the number of switches (also for index out of range, with the outputs untouched).  Needs no context and no GPU. */
int isle_hip_switch_info(int index, const char** name, const char** kind, const char** what);

/* FPSparseMatrix::compute_block_ks  src/sparseMatrix.cpp:1195-1220  driving
 * BlockKs<ProdOp>(op, nev, ncv, maxit, blk, tol) init()+compute()
 * block-ks/restarted_block_ks.h:190-321.  The reference passes
 * (k, 2k + BLOCK_KS_BLOCK_SIZE, 100, 10, 1e-4) (include/hyperparams.h:38-40).
 * evals: nev Ritz values, descending (= sigma_i^2).  U (V x nev) stays on the device for the
 * k-means calls (fetch with isle_hip_get_U).  seed: start-block RNG seed (the reference uses
 * unseeded rand(); parity does not depend on it).  nev / ncv need not be multiples of blk: a
 * decomposition grows block by block until it has at least ncv rows (the reference overruns its
 * basis in that case).  Returns ISLE_E_NOCONV (not 0) if maxit
 * restarts were exhausted — the reference reports full convergence in that case
 * (SURVEY.md App. C #7); evals/U are still the last Ritz pairs.
 * nconv/restarts/napplies may be NULL. */
int isle_hip_block_ks(isle_ctx* ctx, int nev, int ncv, int maxit, int blk, float tol, uint64_t seed,
                      float* evals, int* nconv, int* restarts, int* napplies);

/* The same solver on a caller-supplied dense symmetric operator: BlockKs<ProdOp> is a template over any symmetric
 * operator with multiply()/rows()/cols() (block-ks/restarted_block_ks.h:18-40); this entry is its instantiation with
 * utils::ArmaMatProdOp (block-ks/ks_utils.h:167-182, multiply(X) = A * X), the operator the reference pairs with its
 * known-spectrum recipe utils::get_seed_eigs (ks_utils.h:136-165).  It runs the SAME host loop and device kernels as
 * isle_hip_block_ks (init / expand / truncate / compute, panel QR, rank repair, small EVD, Ritz rotation); only the
 * operator application is a dense product.  A: n x n col-major symmetric (host).  start_block: NULL, or n x blk
 * col-major values for the first draw of init()'s start block (:211-218 redraws at random while it is rank deficient).
 * evals: nev Ritz values, descending.  U (nullable): n x nev col-major Ritz vectors.  nconv: Ritz pairs that passed the
 * residual test of the last restart.  nconv_ref_rule (nullable): what the reference itself would report — equal to nconv
 * on convergence; after maxit restarts its rule (:303-317) looks at the expanded H without dividing and therefore says
 * nev, while this library returns ISLE_E_NOCONV with the honest count.  The context's B, U and
 * k-means state are not touched.  Single rank only. */
int isle_hip_block_ks_dense(isle_ctx* ctx, const float* A_colmajor, uint64_t n, int nev, int ncv, int maxit, int blk,
                            float tol, uint64_t seed, const float* start_block, float* evals, float* U_colmajor,
                            int* nconv, int* nconv_ref_rule, int* restarts, int* napplies);

/* U_colmajor (V x nev), what compute_block_ks memcpy's at src/sparseMatrix.cpp:1214. */
int isle_hip_get_U(isle_ctx* ctx, float* U_colmajor);
/* Test hook: install a caller-provided U (V x k col-major) instead of running the eigensolver. */
int isle_hip_set_U(isle_ctx* ctx, const float* U_colmajor, int k);

/* Dense symmetric eigendecomposition used inside truncate() (arma::eig_sym,
 * block-ks/restarted_block_ks.h:150-161): S n x n col-major symmetric -> evals descending,
 * vecs col-major.  Exposed for parity tests. */
int isle_hip_eig_sym(isle_ctx* ctx, const float* S_colmajor, int n, float* evals_desc, float* vecs_colmajor);

/* The same with only the nvec leading eigenvectors (1 <= nvec <= n), as truncate() calls the solver (nvec = keep):
 * vecs n x nvec col-major.  evals_desc has n entries.  evals_desc[0 .. nvec) are the nvec largest eigenvalues; evals_desc[nvec .. n) is
 * as the solver that answered leaves it: the tridiagonal solver locates only the leading nvec eigenvalues and leaves ZEROS there, the
 * Jacobi solver returns all n eigenvalues (isle_hip_eig_info says which of the two answered).  The upper triangle of S defines the
 * matrix (LAPACK 'U'); the strict lower triangle is not read.  A non-finite entry in the upper triangle is refused with ISLE_E_NUMERIC
 * before anything is launched (both entries). */
int isle_hip_eig_sym_leading(isle_ctx* ctx, const float* S_colmajor, int n, int nvec, float* evals_desc, float* vecs_colmajor);

/* What the most recent small symmetric EVD of this context did (isle_hip_eig_sym, isle_hip_eig_sym_leading, every truncate() of the
 * block Krylov-Schur solver).  info: ISLE_EIG_INFO_COUNT ints, indexed by the enumeration below; defect (nullable): the largest
 * orthogonality defect the tridiagonal solver's own check measured on its eigenvectors (0 where it did not get that far).
 * Host words only: nothing is launched or copied.  No reference counterpart (LAPACK's ssyevd does not say). */
enum {
  ISLE_EIG_SOLVER = 0,    /* who produced the returned pairs: 0 nobody yet (or the solve failed), 1 tridiagonal solver, 2 Jacobi solver */
  ISLE_EIG_TD_TRIED,      /* 1 if the tridiagonal solver was run */
  ISLE_EIG_TD_FORM,       /* the tridiagonalisation that produced its T: 0 none, 1 persistent (one launch), 2 launch chain */
  ISLE_EIG_TD_BAILED,     /* 1 if the persistent form gave up at a grid barrier in THIS solve (the chain then ran) */
  ISLE_EIG_TD_BACK,       /* back-transformation: 0 none, 1 compact WY, 2 reflector by reflector x 8 vectors, 3 x 4 vectors */
  ISLE_EIG_TD_REJECTED,   /* 1 if the tridiagonal solver's result failed its orthogonality check (the Jacobi solver then answered) */
  ISLE_EIG_JACOBI_SWEEPS, /* sweeps of the Jacobi solver (0 if it did not run) */
  ISLE_EIG_N,
  ISLE_EIG_NVEC,
  ISLE_EIG_INFO_COUNT
};
int isle_hip_eig_info(isle_ctx* ctx, int* info, float* defect);

/* ---- k-means --------------------------------------------------------------------------- */
/* FPSparseMatrix::kmeans_init_on_projected_space(k, reps = 1, seeds, centers_coords)
 * src/sparseMatrix.cpp:2212-2238 -> kmeanspp_on_projected_space :2133-2209.
 * inject_seeds: NULL, or k global doc ids that replace the D^2 draws (test hook; the round
 * schedule and min-distance updates still run).  seeds_out: k global doc ids.
 * C_lowd: k x k, centre c at offset c*k (the reference's centers_lowd).  residual: as
 * returned by the reference (App. C #9).  rng_seed seeds the host draw RNG (rand() stand-in). */
int isle_hip_kmeanspp_projected(isle_ctx* ctx, int k, const uint64_t* inject_seeds, uint64_t rng_seed,
                                uint64_t* seeds_out, float* C_lowd, float* residual, int* rounds);

/* Test hook, no context needed: the first n values of the host generator that stands in for the reference's rand() calls
 * (src/sparseMatrix.cpp:2150, include/matUtils.h:473-477) — glibc's rand() after srand(seed); seed 1 = never seeded. */
int isle_hip_host_rand(uint64_t seed, int n, uint32_t* out);

/* Optional test hook: copies the current min-distance array (local docs) after kmeanspp. */
int isle_hip_get_min_dist(isle_ctx* ctx, float* min_dist);

/* FPSparseMatrix::run_lloyds_on_projected_space(k, C_lowd, NULL, max_reps)
 * src/sparseMatrix.cpp:2016-2072.  C_lowd in/out.  assign_out (local docs, may be NULL). */
int isle_hip_lloyds_projected(isle_ctx* ctx, int k, float* C_lowd, int max_reps, int* iters_run,
                              uint32_t* assign_out);

/* FPSparseMatrix::left_multiply_by_U_Spectra(out, in, ld_in, ncols)
 * src/sparseMatrix.cpp:1438-1450: centers (V x ncols col-major) = U (V x k) * in (ld_in x ncols).
 * centers may be NULL: the result then only stays on the device as the start point of
 * isle_hip_lloyds_sparse. */
int isle_hip_lift_centers(isle_ctx* ctx, const float* in, int ld_in, int ncols, float* centers);

/* FPSparseMatrix::run_lloyds(k, centers, closest_docs, max_reps)  src/sparseMatrix.cpp:1690-1746.
 * centers_in: V x k col-major start centres, or NULL to use the device-resident result of
 * isle_hip_lift_centers.  centers_out: V x k col-major (may be NULL).  assign: local docs ->
 * centre index (the caller buckets it into closest_docs[k], ascending doc id). */
int isle_hip_lloyds_sparse(isle_ctx* ctx, int k, const float* centers_in, float* centers_out,
                           uint32_t* assign, int max_reps, int* iters_run);

/* The k-means objective of a partition, per cluster and in total, in word space or in span(U): what the reference's
 * lloyds_iter(..., compute_residual) returns (src/sparseMatrix.cpp:1649-1663, printed at :1714) and its projected twin leaves
 * unwritten (:1995-1998).
 *   doc_dist[d]     = max(0, |x_d - c_assign[d]|^2), evaluated in fp64 on the fp32 values the device holds; x_d = column d of B
 *                     (WORD) or row d of P = B^T U (PROJECTED).  local docs, nullable; the SHARD'S.
 *   cluster_sums[t] = the sum of doc_dist over the documents of cluster t on all ranks; 0 for an empty cluster.  k, nullable.
 *   cluster_sizes[t]: k, nullable.   total (nullable): the sum of cluster_sums, t ascending, formed on the host.
 * The sums are exact sums of the distances rounded to multiples of q = 2^(ex - 53), ex the binary exponent of the largest distance of
 * the corpus: they do not depend on the order the documents are visited in, nor on how the documents are spread over ranks, so two
 * runs can be compared bit for bit.
 *   assign:  local docs -> centre, uploaded into scratch; NULL: the partition resident from the last loop, which must have been the loop
 *            of `space` with this k (isle_hip_lloyds_sparse for WORD, isle_hip_lloyds_projected for PROJECTED).
 *   centers: WORD: vocab x k column-major; PROJECTED: k x k, centre c at c*k (C_lowd); uploaded into scratch.  NULL: the resident
 *            centres: of the last isle_hip_lloyds_sparse (or isle_hip_lift_centers) with this k, or of the last isle_hip_lloyds_projected.
 * A call leaves every resident buffer as it was (partition, centres, member lists): isle_hip_catchwords afterwards reads what it read
 * before.  PROJECTED forms P where it is not resident.
 * world > 1: COLLECTIVE, like isle_hip_catchwords: every rank calls it with the same space and k and with replicated centers, a rank
 * without documents too; cluster_sums, cluster_sizes and total are REPLICATED, bit-identical on every rank and equal to the single-rank
 * run on the concatenated corpus.
 * ISLE_E_ARG, before any work or collective: an unknown space, k < 1, no matrix, no resident partition or centres for that space and k,
 * an assign entry >= k, PROJECTED without U of k columns or with the projection the resident partition was computed on released (a new
 * U since).  Device time is booked under ISLE_T_SPARSE_ASSIGN (WORD) / ISLE_T_LLOYD_PROJ (PROJECTED). */
#define ISLE_SPACE_WORD      0   /* documents = columns of B, centres V x k            */
#define ISLE_SPACE_PROJECTED 1   /* documents = rows of P = B^T U, centres k x k (C_lowd) */
int isle_hip_kmeans_objective(isle_ctx* ctx, int space, int k, const uint32_t* assign, const float* centers,
                              double* cluster_sums, uint64_t* cluster_sizes, double* total, double* doc_dist);

/* Optional test hook: the rows of P = B^T U the device holds for this shard (local docs x k, row-major), formed where they are
 * not resident: the documents of ISLE_SPACE_PROJECTED.  ISLE_E_ARG without U of k columns. */
int isle_hip_get_projection(isle_ctx* ctx, int k, float* P);

/* Trace of the two Lloyd loops (default off: both loops run exactly as without it, no launch, allocation or synchronisation added).
 * on: each loop evaluates the total objective after every centre update — the new centres with the partition they were averaged from,
 * the reference's `residual` — and keeps one double per iteration run; the trace of a space is cleared when its loop is entered.  With
 * world > 1 every rank switches it alike (the evaluation is collective); the trace is replicated.
 * isle_hip_lloyds_trace_get: *n (nullable) = the entries of the last loop in `space`; objective (nullable) receives min(cap, *n). */
int isle_hip_lloyds_trace(isle_ctx* ctx, int on);
int isle_hip_lloyds_trace_get(isle_ctx* ctx, int space, double* objective, int cap, int* n);

/* ---- downstream stage: catchwords, topic model, edge topics ---
 * These operate on the count matrix A left in device memory by isle_hip_upload_counts_u32 and on the
 * partition of B's columns, mapped back to A's documents through original_cols exactly as
 * src/trainer.cpp:572-575 does.
 *
 * Several ranks (world > 1): rank r holds the documents [doc_offset, doc_offset + docs) of A, the columns of
 * B that thresholding kept of them and the partition of those columns.  isle_hip_catchwords,
 * isle_hip_topic_model and isle_hip_select_edge_pairs are then COLLECTIVE: every rank calls them, in the
 * same order, with the same num_topics, r, rho, rank_threshold, max_edge_topics and min_docs; a rank
 * without documents, or with documents but no column of B, calls them too.  What they state bit for bit
 * on one rank they state bit for bit, and equal to the single-rank run on the concatenated corpus.
 * REPLICATED (the whole corpus's, bit-identical on every rank): thresholds, catch_topic, num_catchwords,
 * model, model_threshold, the selected edge pairs with their counts.  The SHARD'S (this rank's own
 * documents, numbered from 0): top1 / top2, *doc_topic_sums and what isle_hip_get_doc_topic_sums returns.
 * The model is summed over the ranks in fp32 (its entries differ from a single-rank run's in the last
 * bits, as two single-rank runs do).  A rank that returns ISLE_E_ARG ahead of the first collective of a
 * call leaves the others waiting: the conditions below are the caller's to hold on every rank alike.
 * ISLE_E_COMM: the ranks disagree on a replicated count.  The readers of a model (isle_hip_edge_topics,
 * isle_hip_model_top_words, isle_hip_edge_top_words, isle_hip_model_text, isle_hip_edge_topics_text,
 * isle_hip_topic_diversity) involve no collective: each rank runs them for itself on the replicated catch
 * model, on a host model or on the model the rank loaded itself (isle_hip_load_model_text; ISLE_MODEL_AVG stays refused: nothing
 * builds the average model there).  Inference and the document reports run on the shards too, see "Document shards" at
 * isle_hip_infer_resident and isle_hip_doc_report_text.  isle_hip_avg_topic_model, isle_hip_topic_coherence,
 * isle_hip_log_combinatorial and isle_hip_distinct_top_five stay "single-rank only" (ISLE_E_ARG).
 *
 * isle_hip_catchwords = SparseMatrix::rth_highest_element for every topic (src/sparseMatrix.cpp:491-524,
 * called at src/trainer.cpp:586-590) + SparseMatrix::find_catchwords (:573-595).
 *   assign: this context's B columns -> topic (what isle_hip_lloyds_sparse returned), or NULL to use
 *           the partition still resident from the last isle_hip_lloyds_sparse call.
 *   r:      the rank of src/trainer.cpp:579-583 (>= 1).   rho: rho_c (include/hyperparams.h:11).
 *   thresholds (nullable): vocab x num_topics column-major, the reference's catchword_thresholds.
 *   catch_topic (nullable): vocab entries, the topic a word is a catchword of or -1 (the rule admits
 *           at most one topic per word); catchwords[t] of the reference = { w : catch_topic[w] == t }
 *           ascending.
 * world > 1: collective; assign holds this rank's columns of B; all three outputs are replicated.
 * ISLE_E_ARG: no count matrix, num_topics < 1, r < 1, an assign entry >= num_topics, no partition
 * (assign null and none resident), a B uploaded separately whose columns are not A's documents. */
int isle_hip_catchwords(isle_ctx* ctx, int num_topics, const uint32_t* assign, uint64_t r, double rho,
                        float* thresholds, int32_t* catch_topic, uint64_t* num_catchwords);

/* SparseMatrix::construct_topic_model (src/sparseMatrix.cpp:597-838) after isle_hip_catchwords.
 *   rank_threshold: src/sparseMatrix.cpp:720.
 *   model (nullable): vocab x num_topics column-major, L1-normalised topic vectors (DenseMatrix Model).
 *   model_threshold (nullable): num_topics.  top1/top2 (nullable): per document of A, the two heaviest
 *   catchword topics (top_topic_pairs, :687-708) or -1/-1.  doc_topic_sums (nullable): number of
 *   non-zero (document, topic) catchword sums; fetch them with isle_hip_get_doc_topic_sums.
 * world > 1: collective; model and model_threshold are replicated; top1 / top2 (docs(A) of this rank) and
 * *doc_topic_sums are the shard's.  ISLE_E_ARG: no count matrix, no isle_hip_catchwords(num_topics)
 * before, rank_threshold < 1. */
int isle_hip_topic_model(isle_ctx* ctx, int num_topics, uint64_t rank_threshold, float* model,
                         float* model_threshold, int32_t* top1, int32_t* top2, uint64_t* doc_topic_sums);
/* doc_offsets: docs(A) + 1 entries; topic / val: doc_topic_sums entries, (document, topic) ascending.  world > 1: the shard's own
 * documents, numbered and offset from 0. */
int isle_hip_get_doc_topic_sums(isle_ctx* ctx, int64_t* doc_offsets, uint32_t* topic, float* val);

/* The FPaxpy pair of ISLETrainer::construct_edge_topics_v2 (src/trainer.cpp:1152-1159) on the
 * device-resident Model: edge[:, e] = primary_ratio * Model[:, pairs[2e]] +
 * (1 - primary_ratio) * Model[:, pairs[2e+1]]; edge is vocab x n column-major. */
int isle_hip_edge_topics(isle_ctx* ctx, const int64_t* pairs, int n, float primary_ratio, float* edge);

/* construct_edge_topics_v2's selection (src/trainer.cpp:1120-1145), on the device: documents with top1 >= 0 and top2 >= 0 are counted per
 * ordered pair (top1, top2); pairs with >= max(min_docs, 1) documents are candidates; they are ordered by count descending, ties by
 * (primary, secondary) ascending (the reference's sort is unstable there); the first max_edge_topics are kept.
 * top1 / top2 NULL: the resident pairs of the last isle_hip_topic_model (n_docs, num_topics must be its own); else n_docs host entries
 * each, uploaded for the call.  pairs: room for cap triples (primary, secondary, documents); selected > cap is ISLE_E_ARG with
 * *n_selected set.  n_selected / n_candidates / threshold are nullable; *threshold = the count of the first candidate cut off.
 * The pairs are counted in a table of num_topics^2 32-bit counters (integer atomics: the result does not depend on arrival order).
 * world > 1: collective.  The resident form counts this rank's documents (n_docs = its docs(A)), the other form takes the top topics of
 * the rank's own documents; the table is summed over the ranks, the rest of the selection runs replicated: pairs, *n_selected,
 * *n_candidates and *threshold are those of the whole corpus on every rank (cap bounds them, not this rank's n_docs).
 * ISLE_E_ARG: num_topics < 1 or > 8192 (the table's limit), max_edge_topics < 0, exactly one of top1 / top2 null, n_docs
 * >= 2^32, a resident call before isle_hip_topic_model or with another size, a topic id >= num_topics or < -1 (the message names the
 * first such document; such an id is never used as an index). */
#define ISLE_EDGE_TABLE_MAX_TOPICS 8192 /* 256 MB of counters */
int isle_hip_select_edge_pairs(isle_ctx* ctx, const int32_t* top1, const int32_t* top2, uint64_t n_docs, int num_topics,
                               int64_t max_edge_topics, uint64_t min_docs, int64_t* pairs, uint64_t cap, uint64_t* n_selected,
                               uint64_t* n_candidates, uint64_t* threshold /* 0: nothing cut */);

/* UMass topic coherence, SparseMatrix::topic_coherence with compute_doc_frequency / compute_joint_doc_frequency
 * (src/sparseMatrix.cpp:841-1016), on the resident count matrix A (no partition or model needed; single rank).
 * top_words: num_topics x M row-major, M distinct word ids per topic, heaviest first (1 <= M <= 32).  With
 * D(w) = documents of A containing w and D(w_i, w_j) = documents containing both:
 *   coherence[t] = sum_{i=1..M-1} sum_{j=0..i-1} [ ln(D(w_i, w_j) + eps) - ln D(w_j) ]
 * evaluated in double, i ascending then j ascending (the reference's index order, :858-866); M = 1 gives 0; NaN where any
 * D(w_j) of a denominator (j < M-1) is 0 (the reference asserts there).
 * doc_freq (nullable): num_topics x M, D(w_i).  co_doc_freq (nullable): num_topics x M(M-1)/2, D(w_i, w_j) at i(i-1)/2 + j
 * for i = 1..M-1, j < i.  The counts are exact integers and the result is reproducible bit for bit.
 * Deviations from the reference: D counts over ALL of A's documents (the reference counts over B's columns only); the sum is
 * in double without the reference's float accumulation and its race on coherences[topic].
 * ISLE_E_ARG: no count matrix, world > 1, num_topics < 1, M < 1 or M > 32, a word id >= vocab, a word repeated in a topic. */
int isle_hip_topic_coherence(isle_ctx* ctx, int num_topics, int M, const uint32_t* top_words, double eps, double* coherence,
                             uint64_t* doc_freq, uint64_t* co_doc_freq);

/* The cluster-average topic model of ISLETrainer::output_avg_topic_coherence (src/trainer.cpp:705-745: construct_topic_model with
 * no catchwords): every topic is the L1-normalised sum of its cluster's documents.  Valid after isle_hip_catchwords(num_topics); it
 * reads the partition mapped onto A's documents there (documents dropped by sampling belong to no topic) and the normalised values
 * nv the catch model reads.  With s_t[w] = sum over the documents d of cluster t of nv[w, d]:
 *   model[:, t] = s_t / sum_w s_t[w]
 * s_t is the exact sum of the fp32 values (every value is an integer multiple of the smallest value's ulp: fixed-point integer
 * sums), divided in double and rounded once to float, so |m - m64| <= 2^-22 |m64| against fp64 sums of the same nv, entries with
 * no contribution are exactly 0, an empty cluster gives a NaN column (0 / 0, the catch model's rule), and two calls give the same
 * bits.  The model stays resident in a buffer of its own (the catch model is untouched) until A, the partition or the catchwords
 * change.  model (nullable): vocab x num_topics column-major.  ISLE_E_ARG: no count matrix, world > 1, no catchword pass with
 * num_topics.  ISLE_E_NUMERIC: the normalised values span more than the 2^64 range of the accumulator (a ratio above 2^40).
 * Deviation from the reference: it accumulates in fp32. */
int isle_hip_avg_topic_model(isle_ctx* ctx, int num_topics, float* model);

/* Models isle_hip_model_top_words and isle_hip_topic_diversity read. */
#define ISLE_MODEL_CATCH 0 /* the resident topic model of isle_hip_topic_model */
#define ISLE_MODEL_AVG 1   /* the resident average model of isle_hip_avg_topic_model */
#define ISLE_MODEL_HOST 2  /* model_host: vocab x ncols column-major, uploaded for the call */
#define ISLE_MODEL_LOADED 3 /* the resident model of isle_hip_load_model_text; vocab and ncols must be its own */

/* The n heaviest words of every column of a model (DenseMatrix::find_n_top_words, src/denseMatrix.cpp:92-107, with the trainer's
 * order): heaviest first, the lower word id first among equal weights (-0 == +0), NaN (and -inf) last.  Exact: a radix select on
 * the float bits per column, one read of the model.  ids: ncols x n row-major; weights (nullable): the model entries at those ids.
 * For CATCH and AVG, vocab and ncols must be the resident model's (V of A, num_topics), for LOADED the loaded model's; model_host is ignored.
 * ISLE_E_ARG: world > 1 with AVG or LOADED (CATCH is replicated, HOST the caller's: each rank reads for itself), n < 1 or n > min(vocab, 32), an unknown model, a resident model that does not exist (yet), a size mismatch,
 * ids or (HOST) model_host null. */
int isle_hip_model_top_words(isle_ctx* ctx, int which, const float* model_host, uint64_t vocab, int ncols, int n, uint32_t* ids, float* weights);

/* The n heaviest words of the edge topics primary_ratio * M[:, pairs[2e]] + (1 - primary_ratio) * M[:, pairs[2e + 1]], e < n_edge, of
 * model `which` (CATCH, AVG, LOADED, HOST as in isle_hip_model_top_words, with its conditions on model_host / vocab / ncols): order
 * and NaN rule of isle_hip_model_top_words, entries formed as isle_hip_edge_topics forms them (bit-equal), from the model's two columns
 * while they are read: no vocab x n_edge matrix is stored.  ids: n_edge x n row-major; weights (nullable): the entries at those ids.
 * ISLE_E_ARG also for: n_edge < 0, pairs or ids null with n_edge > 0, a pair id outside 0 .. ncols - 1. */
int isle_hip_edge_top_words(isle_ctx* ctx, int which, const float* model_host, uint64_t vocab, int ncols, const int64_t* pairs, int n_edge,
                            float primary_ratio, int n, uint32_t* ids, float* weights);

/* Topic diversity (ISLETrainer::output_topic_diversity, src/trainer.cpp:750-774) of a resident model (CATCH, AVG or LOADED), in double
 * with a fixed reduction order.  A topic is finite when every entry of its vector is; k' = the number of finite topics.
 *   abar = (1/k') sum over finite t of m_t      dist[t] = sum_w (m_t[w] - abar[w])^2      avg = mean of dist over finite t
 * Non-finite topics get dist = NaN; no finite topic gives avg = NaN.  dist: num_topics doubles (nullable); avg (nullable).
 * Deviations from the reference: its cross term uses topic 1's vector for every topic (:769-771) and it accumulates in fp32.
 * ISLE_E_ARG: world > 1 with AVG or LOADED, an unknown or HOST model, a resident model that does not exist, num_topics not the model's. */
int isle_hip_topic_diversity(isle_ctx* ctx, int which, int num_topics, double* dist, double* avg);

/* The reference's model files, formatted on the device (isle_amd/csrc/model_text.hip): MMappedOutput (include/utils.h:383-478) under
 * DenseMatrix::write_to_file_as_sparse / write_to_file (src/denseMatrix.cpp:124-186), as trainer_detail::weight_text, dense_entry_text,
 * write_dense_as_sparse and write_dense (isle_amd/host/trainer_hip.h) restate them; the bytes equal theirs.  model: vocab x ncols column-major.
 *   ISLE_TEXT_SPARSE  columns ascending, rows ascending in a column; every entry w > 1e-8f (float compare; NaN, zero, negative and tiny
 *                     entries are skipped) gives "<col+1>\t<row+1>\t<weight>\n"  (M_hat_catch_sparse, EdgeModel_sparse)
 *   ISLE_TEXT_DENSE   one column per line, every entry followed by '\t', the line ended by '\n'; zero and -0 give "0.0", NaN gives "nan",
 *                     anything else <weight>  (M_hat_avg)
 *   <weight>          (unsigned)w in decimal, at most its six low digits (1234567.875 -> 234567), '.', then six fraction digits:
 *                     rest = w - (float)(int)w; six times: rest *= 10; d = (int)rest; emit '0' + d; rest -= d — fp32, each operation
 *                     rounded on its own (never a fused multiply-add), truncating
 * An entry that would be printed and is negative, infinite or >= 2^31 is outside the writer's domain ((int)w and (unsigned)w are
 * undefined there): the call fails with ISLE_E_ARG naming the first such entry (column-major) before any byte is delivered.
 * One pass counts (bytes per tile, entries, the domain check), a 64-bit exclusive scan places every tile, one pass writes the text in
 * chunks of at most 16 MiB (whole columns; a longer column is split), each handed to `sink` in order on the calling thread while the
 * device formats the next; the concatenation of the pieces is the file.  A non-zero return of the sink ends the call with ISLE_E_ARG, no
 * further piece is delivered and the context stays usable.  sink == NULL: the size query (the counting pass alone).  nbytes / nentries
 * (nullable): the size of the text and the number of entries it holds (DENSE: every entry, vocab x ncols).  ncols == 0 (n == 0):
 * no bytes, no sink call, 0.  Single rank.
 * isle_hip_model_text: which / model_host / vocab / ncols and their ISLE_E_ARG conditions as isle_hip_model_top_words; ISLE_E_ARG also for
 * an unknown format.
 * isle_hip_edge_topics_text: the text of the edge model isle_hip_edge_topics(pairs, n, primary_ratio) would return (its ISLE_E_ARG
 * conditions), column e numbered e + 1; the entries are formed from the resident topic model as they are read (the same two fp32
 * operations), the vocab x n floats exist neither on the device nor on the host.
 * isle_hip_entry_text (host only, no context): one entry's text under `format` into out16 (NUL-terminated); returns its length,
 * 0 = skipped (SPARSE), -1 = outside the writer's domain or an unknown format.  The library's one copy of the digit rule: the kernels
 * compile the same function. */
#define ISLE_TEXT_SPARSE 0
#define ISLE_TEXT_DENSE 1
typedef int (*isle_text_sink_fn)(const char* bytes, uint64_t n, void* user);
int isle_hip_model_text(isle_ctx* ctx, int which, const float* model_host, uint64_t vocab, int ncols, int format, isle_text_sink_fn sink,
                        void* user, uint64_t* nbytes, uint64_t* nentries);
int isle_hip_edge_topics_text(isle_ctx* ctx, const int64_t* pairs, int n, float primary_ratio, int format, isle_text_sink_fn sink, void* user,
                              uint64_t* nbytes, uint64_t* nentries);
int isle_hip_entry_text(float w, int format, char* out16);

/* The same files read back on the device (isle_amd/csrc/model_load.hip), the inverse of isle_hip_model_text: read_sparse_model
 * (src/infer.cpp:125-208) and read_model (:8-76) as isle_amd/host/model_read.h restates them.  The text goes up in one copy and is parsed
 * into a resident model of its own, vocab x ncols column-major, ISLE_MODEL_LOADED: isle_hip_model_top_words, isle_hip_topic_diversity,
 * isle_hip_model_text and isle_hip_infer_resident take it wherever they take CATCH or AVG (vocab and ncols must be the loaded model's,
 * for isle_hip_infer_resident vocab must also be A's; ISLE_E_ARG when nothing is loaded).  It does not depend on A, B, the partition or
 * the catchwords and lives until the next successful load or isle_hip_destroy.  The text is parsed into scratch and swapped in on
 * success: a failed call leaves the previous model intact and the context usable.
 *   <weight>          <digits>[.<digits>], at least one digit (".5" and "5." are weights).  vb (before the point) and va (after it) are
 *                     accumulated in fp32 digit by digit, v = v * 10; v = v + d, each operation rounded on its own (never a fused
 *                     multiply-add); the value is (float)((double)vb + (double)va * P[n]), n = the digits after the point, P[n] = the
 *                     host's std::pow(0.1, n), computed once on the host (the device calls no pow).  A second '.', any other
 *                     character or a token longer than 64 bytes is an error.  Deviation: the reference has no length limit.
 *   ISLE_TEXT_SPARSE  lines end in '\n' (the last one may go without), '\r' is ignored everywhere, fields are separated by runs of
 *                     blanks or tabs, blanks may lead and trail, blank lines are skipped.  A line is "<topic> <word> <weight>", the ids
 *                     decimal with at most 18 digits; id - base (base 0 or 1) must lie in [0, ncols) and [0, vocab).  Cells no line
 *                     names are +0; of several lines naming one cell the LAST in the file wins, whatever the launch geometry.  nentries:
 *                     the lines parsed, repeated cells included.  An empty text is the zero model, 0 entries.  At most 2^34 - 16 bytes
 *                     (the order of the lines is kept in 32 bits), ISLE_E_ARG beyond.
 *   ISLE_TEXT_DENSE   one line per column, tokens separated by runs of blanks or tabs (the writer's trailing tab is fine), '\r' ignored,
 *                     blank lines skipped: token j of the t-th non-blank line is model[j, t].  "nan" is the quiet NaN 0x7fc00000, as
 *                     the library's dense writer prints it (SPARSE refuses it).  Every non-blank line must hold exactly vocab tokens,
 *                     there must be exactly ncols non-blank lines (an empty text is an error).  nentries: vocab x ncols.
 * Deviations from the reference readers: they assert, or only print "Bad format" and go on; here every violation is an error.  Two
 * limits beside the token's keep every walk of the parser short on a corrupt text, both refused as "bad character": a SPARSE line of
 * more than 4096 bytes (its '\n' excluded), more than 64 consecutive '\r' in a DENSE text.  The line named is the rule; where one line
 * holds several violations the kind named is one of them.
 * ISLE_E_ARG: an unknown format, base > 1, vocab 0 or above 0xfffffff0, ncols < 1, text null with nbytes > 0, and the parse
 * errors: the FIRST offending line of the file (whatever the launch order) is named, 1-based, with its kind, as
 * "load_model_text: line <n>: <kind>" in isle_hip_last_error; the kinds are "bad character", "too many fields", "too few fields",
 * "id zero or out of range", "token too long", "wrong token count", "wrong line count" (named at the last line).  Where the host
 * parser of model_read.h throws, this call fails.  Device time is booked under ISLE_T_INGEST.  world > 1: no collective, each rank
 * loads for itself (the same text on every rank, if the ranks are to agree).
 * isle_hip_get_loaded_model: the loaded model (vocab x ncols column-major) and its size, each nullable; ISLE_E_ARG when nothing is loaded.
 * isle_hip_parse_weight (host only, no context): the n bytes of one <weight> token under `format` into *out; 0, or -1 for a token
 * outside the grammar ("nan" under SPARSE, the empty token, '\r' included) or an unknown format.  The library's one copy of the weight
 * rule: the kernels compile the same function. */
int isle_hip_load_model_text(isle_ctx* ctx, const char* text, uint64_t nbytes, uint64_t vocab, int ncols, int format, unsigned base,
                             uint64_t* nentries);
int isle_hip_get_loaded_model(isle_ctx* ctx, float* model_colmajor, uint64_t* vocab, int* ncols);
int isle_hip_parse_weight(const char* token, uint64_t n, int format, float* out);

/* Corpus diagnostics of the trainer (print_log_combinatorial / print_distinct_top_five_sets, src/trainer.cpp:373-403) on the resident
 * count matrix A, right after ingest or upload (no partition or B needed; single rank; ISLE_E_ARG without A).
 *
 * Log-combinatorial, SparseMatrix::compute_log_combinatorial (src/sparseMatrix.cpp:1018-1043): out[d] for every document of A,
 *   N_d = sum of (int)count,  log_fact[0] = 0,  log_fact[i+1] = (float)((double)log_fact[i] + log(i+1)),
 *   out[d] = ((0 - log_fact[(int)c_0]) - log_fact[(int)c_1] - ...) + log_fact[N_d]   in fp32, entries in CSC order (bit-equal).
 * max_words (nullable): max N_d.  ISLE_E_ARG: out null, some N_d > INT_MAX (the reference indexes the table with an int).
 * Deviation: the shipped reference cannot run it (normalize_docs(true) frees vals_CSC, src/sparseMatrix.cpp:163-166, before it reads
 * them); this computes what the function says from the resident counts. */
int isle_hip_log_combinatorial(isle_ctx* ctx, float* out, uint64_t* max_words);

/* Distinct top-five sets, SparseMatrix::count_distint_top_five_words (src/sparseMatrix.cpp:170-215): for every document with at least
 * 5 entries, the 5 largest normalised values avg_doc_sz * (count / doc_sum) (the values the catchword stage uses), descending, with
 * multiplicity; the tuples sorted lexicographically ascending; num_distinct[i] = the reference's loop with min_distinct = m[i] over
 * them (see isle_hip_top_five_count_rule).  num_quintuples (nullable): the number of tuples ("top five vec size").  quintuples
 * (nullable, capacity docs(A) x 5): the sorted tuples, row-major.  run_lengths (nullable, capacity docs(A)) / num_runs (nullable): the
 * lengths of the runs of equal tuples in sorted order, for isle_hip_top_five_count_rule.
 * ISLE_E_ARG: n_m < 0, m or num_distinct null with n_m > 0, some m[i] < 2 (an assert in the reference).
 * Deviation: the reference copies a document into a stack buffer of 1 << 15 values (undefined beyond); any length is handled here. */
int isle_hip_distinct_top_five(isle_ctx* ctx, int n_m, const int32_t* m, uint64_t* num_distinct, uint64_t* num_quintuples, float* quintuples,
                               uint64_t* run_lengths, uint64_t* num_runs);

/* Host only: the counting loop of src/sparseMatrix.cpp:198-208 over n = sum(run_lengths) sorted tuples given as the lengths of their
 * runs of equal tuples.  Literally  num = 0; it = prev = 0; while (it != n) { if (q[it] == q[prev]) { ++it; continue; }
 * if (it - prev >= m) { prev = it; ++num; } ++it; }  (the trailing "if (prev - it >= m)" never fires), evaluated as jumps
 * p -> p + max(rem(p), m), rem(p) = distance from p to the end of its run, counting each jump that lands before n.
 * ISLE_E_ARG: out null, run_lengths null with n_runs > 0, a run of length 0, m < 2. */
int isle_hip_top_five_count_rule(const uint64_t* run_lengths, uint64_t n_runs, int32_t m, uint64_t* out);

/* ---- inference ---------------------------------------------------- */
/* ISLEInfer over a batch of documents: drivers/ISLEInfer.cpp:60-112 (normalize_docs(true, true),
 * infer_doc_in_file per document, heaviest topics) with ISLEInfer::mwu / grad / calculate_llh
 * src/infer.cpp:361-492.  model_by_word: vocab x num_topics ROW-major (element (word, topic) at
 * word * num_topics + topic), what load_model_from_sparse_file src/infer.cpp:32-70 builds from
 * M_hat_catch_sparse.  The documents are a count matrix in CSC (word ids ascending per document).
 * iters / Lf_guess: INFER_ITERS_DEFAULT 15 / INFER_LF_DEAFULT 10.0 (include/hyperparams.h:81-82).
 * avg_doc_sz: SparseMatrix::avg_doc_sz of the documents (src/sparseMatrix.cpp:98).
 * Outputs (host, each nullable): weights docs x num_topics row-major (1 / num_topics where inference did
 * not converge, as the dense writer prints them); top_topic / top_weight docs x 5, topics with weight >
 * 1 / num_topics in decreasing weight, -1 / 0 where there are fewer; llh docs x 2 (first = sum * avg_doc_sz,
 * second = sum * words in the document; 0, 0 when not converged); nconverged = documents with llh.first != 0.
 * Independent of the matrices held by the context. */
int isle_hip_infer(isle_ctx* ctx, uint64_t vocab_size, int num_topics, const float* model_by_word,
                   uint64_t num_docs, uint64_t nnz, const float* counts, const uint32_t* rows,
                   const int64_t* offsets, int iters, float Lf_guess, float avg_doc_sz, float* weights,
                   int32_t* top_topic, float* top_weight, float* llh, uint64_t* nconverged);

/* The same inference on what is resident: documents [doc_begin, doc_end) of the count matrix A (isle_hip_upload_counts_u32 or
 * isle_hip_ingest_tdf; the counts as they are, normalised per document by the kernel) under the catch model, the average model or a
 * caller's model, with the weights returned as sparse entries.  No B, partition or catchwords are needed with ISLE_MODEL_HOST.
 *   which / model_host / vocab / ncols: as isle_hip_model_top_words (ISLE_MODEL_HOST: vocab x ncols COLUMN-major, uploaded once for the
 *     call), with its ISLE_E_ARG conditions; vocab must be A's; ncols outside [1, 1024] is refused as by isle_hip_infer.  The model is
 *     transposed on the device into the row-major, zero-padded layout the iteration kernels read; the iterations are the launches of
 *     isle_hip_infer on the resident buffers, so for the same fp32 model and documents every output equals isle_hip_infer's bit for bit.
 *   iters / Lf_guess: as isle_hip_infer.  avg_doc_sz is the corpus value the context holds (the thresholding's, or computed here by the
 *     same rule, SparseMatrix::populate_CSC src/sparseMatrix.cpp:87-98: floor(sum of counts / number of non-empty documents) over ALL of
 *     A, not over the range): llh.first is scaled by the corpus average, whatever the range.
 *   top_topic / top_weight (range x 5), llh (range x 2), nconverged: as isle_hip_infer, over the range only (the first document of the
 *     range is row 0); each nullable.
 *   Entries: for every converged document (llh.first != 0) every topic with weight > min_weight, compared in float, topics ascending;
 *     min_weight < 0 selects 1.0f / (float)ncols, the rule of the top topics.  Documents that did not converge (empty ones, documents
 *     whose words are all absent from the model) have no entries.  nentries (nullable): their number.  They stay resident until the next
 *     call or until A changes; isle_hip_get_infer_entries copies them out: doc_offsets (doc_end - doc_begin) + 1 entries (64-bit: the
 *     count can reach docs x ncols), topic / weight nentries entries, (document, topic) ascending; each nullable.
 *   chunk_docs: documents per pass; the device holds the dense weights of one pass only (chunk_docs x ncols floats), never docs x ncols.
 *     0 = as many as keep them within 1 GiB (at most 2^22).  No result depends on it, bit for bit.
 * Document shards (world > 1): doc_begin / doc_end and every output are the rank's own documents', rows numbered from the call's doc_begin.
 * avg_doc_sz is the CORPUS value over all ranks' documents.  Where the thresholding has not left it behind (B came from the host) the call
 * all-reduces two 64-bit totals to form it, once per count matrix: isle_hip_infer_resident and isle_hip_avg_doc_sz are then COLLECTIVE,
 * called by every rank in the same order, a rank without documents included.  A document is computed from its own words, the model and
 * avg_doc_sz alone: the shards' entries side by side are the single-rank run's, bit for bit.  ISLE_MODEL_AVG is refused.
 * ISLE_E_ARG: no count matrix, doc_begin > doc_end, doc_end > docs(A), iters < 1, Lf_guess <= 0, the model conditions above.
 * doc_begin == doc_end is valid: no entries, nconverged = 0.  Every argument is checked before any work: after a refusal the context is
 * usable and the entries of the previous call are intact; a call that fails later (ISLE_E_HIP) leaves none (isle_hip_get_infer_entries
 * then returns ISLE_E_ARG, as it does before the first call and after a new A).  top_topic / top_weight of the call stay resident with the
 * entries, for isle_hip_infer_text.  Device time is booked under ISLE_T_INFER. */
int isle_hip_infer_resident(isle_ctx* ctx, int which, const float* model_host, uint64_t vocab, int ncols, uint64_t doc_begin,
                            uint64_t doc_end, int iters, float Lf_guess, float min_weight, uint64_t chunk_docs, int32_t* top_topic,
                            float* top_weight, float* llh, uint64_t* nconverged, uint64_t* nentries);
int isle_hip_get_infer_entries(isle_ctx* ctx, int64_t* doc_offsets, uint32_t* topic, float* weight);
/* The per-document topic files, formatted on the device (isle_amd/csrc/infer_text.hip) from the result of the last
 * isle_hip_infer_resident where it lies: row 0 is that call's doc_begin, the call formats rows [row_begin, row_end).  A line is
 *   "<row + number_base>\t<topic + 1>\t<weight>\n"
 * with the two integers in plain decimal (MMappedOutput::concat_int, include/utils.h:383-418) and <weight> exactly the <weight> of
 * ISLE_TEXT_SPARSE above (the same function).  trainer_detail::doc_line_text / write_doc_topic_lines (isle_amd/host/trainer_hip.h) restate
 * the bytes on the host.
 *   ISLE_DOCTEXT_ENTRIES  every resident entry of the rows, rows ascending, topics ascending within a row; rows without entries give
 *                         nothing  (ISLETrainer::output_doc_topic_weights, DocTopicWeights.tsv with number_base = 1)
 *   ISLE_DOCTEXT_TOP      for each row the slots i = 0..4 of top_topic / top_weight in order while top_topic[5 row + i] >= 0
 *                         (ISLEInfer's top_topics_* files, drivers/ISLEInfer.cpp:100-112, with number_base = <min_doc_id_in_infer_file>)
 * Domain: concat_int asserts num < 0x7fffffff, and the weight's (int)w / (unsigned)w are undefined outside [0, 2^31).  A printed
 * number (row + number_base or topic + 1) >= 0x7fffffff, or a printed weight that is negative, NaN, infinite or >= 2^31, fails the call
 * with ISLE_E_ARG naming the first such line, before any byte is delivered.
 * Delivery is isle_hip_model_text's: a counting pass (bytes per tile of 1024 lines, the line count, the domain check), a 64-bit
 * exclusive scan, a writing pass in pieces of at most 16 MiB, each non-empty and ending at a line end, handed to `sink` in order on the
 * calling thread while the device formats the next.  sink == NULL: the size query.  A non-zero return of the sink ends the call with
 * ISLE_E_ARG and the context stays usable.  nbytes / nlines (nullable): the size of the text and its lines.  No lines: no sink call, 0.
 * ISLE_E_ARG also for: an unknown `what`, row_begin > row_end, row_end beyond the rows of the last isle_hip_infer_resident, no valid
 * resident result (before the first call, after a new count matrix, after a call that failed).
 * Document shards (world > 1): no collective.  number_base stays the caller's: a rank whose isle_hip_infer_resident covered documents
 * [b, e) of its shard passes base + doc_offset(A) + b (isle_hip_counts_shape), and the ranks' texts in rank order are the corpus's file.
 * The call changes nothing resident: a second call gives the same bytes and isle_hip_get_infer_entries returns what it returned before.
 * Device time is booked under ISLE_T_INFER.
 * isle_hip_doc_line_text (host only, no context): one line for the printed numbers doc_number, topic_number (the + base and + 1 already
 * applied) and w into out40 (NUL-terminated); returns its length, -1 outside the writers' domain (a number >= 0x7fffffff, a weight as
 * above) or for a null out40.  It compiles the functions the kernels compile. */
#define ISLE_DOCTEXT_ENTRIES 0 /* the resident entries of the last isle_hip_infer_resident (DocTopicWeights.tsv) */
#define ISLE_DOCTEXT_TOP 1     /* its heaviest topics, at most five per document (ISLEInfer's top_topics_* files) */
int isle_hip_infer_text(isle_ctx* ctx, int what, uint64_t row_begin, uint64_t row_end, uint64_t number_base, isle_text_sink_fn sink,
                        void* user, uint64_t* nbytes, uint64_t* nlines);
int isle_hip_doc_line_text(uint64_t doc_number, uint64_t topic_number, float w, char* out40);
/* The trainer's three per-document report files, formatted on the device (isle_amd/csrc/doc_report.hip) from what isle_hip_catchwords and
 * isle_hip_topic_model left resident, for documents [doc_begin, doc_end) of A.  All are MMappedOutput text: integers in plain decimal
 * (concat_int), the weight exactly the <weight> of ISLE_TEXT_SPARSE; documents, words and topics are printed 1-based.
 * trainer_detail::doc_catchword_text / doc_topic_sums_text / top_two_text (isle_amd/host/trainer_hip.h) restate the bytes on the host.
 *   ISLE_DOCREPORT_CATCHWORDS         DocCatchword.tsv (ISLETrainer::output_doc_topic, src/trainer.cpp:946-964): documents ascending, the
 *                                     entries of a document in stored order; every entry of A whose word is a catchword gives
 *                                     "<doc + 1>\t<word + 1>\t<normalised value>\n"
 *   ISLE_DOCREPORT_TOPIC_SUMS         DocTopicCatchwordSums.tsv (:979-983): every non-zero (document, topic) catchword sum of the documents
 *                                     gives "<doc + 1>\t<topic + 1>\t<sum>\n", in the order construct_topic_model leaves the vector in
 *                                     (src/sparseMatrix.cpp:715-718): topic ascending, then value descending.  Deviation: the reference's
 *                                     sort is unstable, so equal (topic, value) pairs come in no stated order there; here they go by
 *                                     document ascending.  The range selects the documents whose sums are sorted and printed; a range
 *                                     with >= 2^32 sums is ISLE_E_ARG (write it in parts).
 *   ISLE_DOCREPORT_TOPIC_SUMS_BY_DOC  the same lines in the resident order: document ascending, then topic ascending
 *   ISLE_DOCREPORT_TOP_TWO            TopTwoTopicsPerDoc.txt (ISLETrainer::print_top_two_topics, :1029-1035): documents ascending; every
 *                                     document with top1 >= 0 and top2 >= 0 gives "<doc + 1>\t<top1 + 1>\t<top2 + 1>\n"
 * Domain, delivery, the size query (sink == NULL), a non-zero sink return and "no lines: no sink call" are isle_hip_infer_text's: a
 * printed number >= 0x7fffffff, or a printed weight that is negative, NaN, infinite or >= 2^31, fails the call with ISLE_E_ARG naming the
 * first such line before any byte is delivered; pieces of at most 16 MiB, each non-empty and ending at a line end.
 * Document shards (world > 1): doc_begin / doc_end are the rank's own documents; the document printed is doc_offset(A) + doc + 1, the
 * number in the corpus, and the domain check applies to it (the refusal names the local and the corpus's document).  With world == 1 the
 * offset is not applied, whatever the upload said.  CATCHWORDS, TOPIC_SUMS_BY_DOC and TOP_TWO involve no collective: the ranks' texts in
 * rank order are the corpus's file.  TOPIC_SUMS is one order over all ranks' sums and COLLECTIVE: ALL RANKS MUST ASK FOR TOPIC_SUMS
 * TOGETHER, in the same order among their collective calls, the size query (sink == NULL) and a rank without documents or sums included.
 * The keys of every rank's range are all-gathered with their corpus documents, sorted on every rank, and rank q's sink receives lines
 * [slice(q), slice(q + 1)) of the corpus's L lines, slice(q) = q floor(L / W) + min(q, L mod W): the ranks' texts in rank order are the
 * single-rank file, equal pairs by document ascending.  nbytes / nlines are the slice's.  L >= 2^32 is ISLE_E_ARG on every rank.  Every
 * collective of the call precedes its first sink call: a sink that refuses, or a line outside the domain, on one rank leaves the others
 * to complete.  Device memory of this form: about (W + 1) nmax 12 bytes and the sort's twin, nmax the largest count of a rank; NOT measured.
 * ISLE_E_ARG also for: an unknown `what`, doc_begin > doc_end, doc_end > docs(A), no count matrix, a call before
 * isle_hip_catchwords (CATCHWORDS) or before isle_hip_topic_model (the other kinds), a call after a new count matrix.
 * The call changes nothing resident: a second call gives the same bytes.  Device time is booked under ISLE_T_POST.
 * isle_hip_top_two_line_text (host only, no context): one TOP_TWO line for the numbers as printed into out40 (NUL-terminated); returns its
 * length, -1 for a number >= 0x7fffffff or a null out40.  It compiles the functions the kernels compile.  The lines of the other three
 * kinds are isle_hip_doc_line_text's. */
#define ISLE_DOCREPORT_CATCHWORDS 0
#define ISLE_DOCREPORT_TOPIC_SUMS 1        /* reference order */
#define ISLE_DOCREPORT_TOPIC_SUMS_BY_DOC 2 /* resident order */
#define ISLE_DOCREPORT_TOP_TWO 3
int isle_hip_doc_report_text(isle_ctx* ctx, int what, uint64_t doc_begin, uint64_t doc_end, isle_text_sink_fn sink, void* user,
                             uint64_t* nbytes, uint64_t* nlines);
int isle_hip_top_two_line_text(uint64_t doc_number, uint64_t t1_number, uint64_t t2_number, char* out40);
/* The n heaviest documents of every topic, selected on the device (isle_amd/csrc/topic_docs.hip) from entries that are stored by document,
 * where they lie: nothing is sorted and nothing is gathered per topic.  The rule is stated once, in isle_amd/csrc/topdocs_host.h:
 *   an entry is (row, topic, value); value is fp32 with bits b; the row's document is doc = doc_base + row, a 32-bit number in the corpus
 *   ord(b) = b ^ (b >> 31 ? 0xffffffff : 0x80000000)           (for positive finite values, as both resident sources hold, the numeric order)
 *   key    = (uint64)ord(b) << 32 | (uint32)~doc                the larger key wins: the heavier value, the smaller document among bit-equal
 *                                                               values (the tie rule of ISLE_DOCREPORT_TOPIC_SUMS)
 * For topic t the result is its min(n, cnt_t) largest keys in descending order, cnt_t the topic's entries over all ranks:
 * docs[t n + i] / values[t n + i] for i < counts[t] = min(n, cnt_t), the unused slots 0xffffffff / 0.0f; topic_entries[t] = cnt_t (nullable).
 * Values that are not positive finite go by ord as well (-0.0 below +0.0, negatives below, +inf above the finite values, NaN patterns by
 * their bits): no value is refused.  docs / values are num_topics x n, topic-major.
 *   ISLE_TOPDOCS_INFER  the resident entries of the last isle_hip_infer_resident; row 0 is that call's doc_begin
 *   ISLE_TOPDOCS_SUMS   the document-topic catchword sums of the last isle_hip_topic_model; a row is a document of A; num_topics is that call's
 *   ISLE_TOPDOCS_HOST   the caller's CSR: doc_offsets (num_rows + 1, ascending from 0), topic and value per entry, uploaded for the call; the
 *                       topics of a row ascend strictly.  For the other sources num_rows is ignored and the three arrays may be NULL.
 * doc_base is the caller's, as number_base is for isle_hip_infer_text: with document shards a rank passes doc_offset(A) (+ doc_begin for INFER).
 * Document shards (world > 1): COLLECTIVE.  ALL RANKS CALL TOGETHER, with the same source, num_topics and n (checked: ISLE_E_COMM otherwise), in
 * the same order among their collective calls, a rank without rows or with rows and no entries included.  The counts go through one u64
 * all-reduce, the select's bins (num_topics x 256 u32) through eight, the ranks' tables of winners (num_topics x n u64 each) through one
 * all-gather; the sort runs replicated.  Every rank returns the corpus's lists, bit-identical, and they are the lists one rank holding all
 * the entries returns.  The refusals below that depend on a rank's own arguments alone precede every collective: the ranks must agree on them.
 * A bad entry on one rank, or a topic with 2^31 entries or more (one rank: 2^32), is ISLE_E_ARG on every rank.
 * ISLE_E_ARG: an unknown source, num_topics < 1, n outside 1 .. ISLE_TOPDOCS_MAX_N, world x n > 8192 (the keys of a topic are sorted in
 * 64 KiB of LDS), doc_base + rows > 0xfffffff1, null docs / values / counts, HOST arrays null where there are rows / entries, doc_offsets
 * that do not ascend from 0, INFER without a valid resident result, SUMS before isle_hip_topic_model or with another num_topics; and, found on
 * the device, a topic >= num_topics or topics that do not ascend strictly within a row: the message names the first such entry and its row.
 * The call changes nothing resident and keeps nothing: a second call returns the same arrays, and isle_hip_infer_text,
 * isle_hip_get_infer_entries, isle_hip_get_doc_topic_sums and isle_hip_doc_report_text return what they returned before.
 * Device memory of the call: 4 bytes per entry (the entry's document), num_topics KiB of bins, (world + 1) num_topics n 8 bytes of tables
 * (HOST: and the uploaded arrays).  Device time is booked under ISLE_T_INFER for ISLE_TOPDOCS_INFER and under ISLE_T_POST otherwise.  Measured
 * on one rank at configuration 2 only (tools/top_docs_probe.py, profiles/top_docs_c2.jsonl); NO TIME IS MEASURED on several ranks, and the
 * bins' two homes were never timed at one num_topics. */
#define ISLE_TOPDOCS_INFER 0 /* the resident entries of the last isle_hip_infer_resident (row 0 = that call's doc_begin) */
#define ISLE_TOPDOCS_SUMS 1  /* the document-topic catchword sums of the last isle_hip_topic_model (row = document of A) */
#define ISLE_TOPDOCS_HOST 2  /* the caller's CSR: doc_offsets (num_rows + 1), topic, value, uploaded for the call */
#define ISLE_TOPDOCS_MAX_N 256
int isle_hip_topic_top_docs(isle_ctx* ctx, int source, int num_topics, int n, uint64_t doc_base, uint64_t num_rows, const int64_t* doc_offsets,
                            const uint32_t* topic, const float* value, uint32_t* docs, float* values, uint32_t* counts, uint64_t* topic_entries);
/* The n documents most similar to each of num_queries query documents, scored and selected on the device (isle_amd/csrc/similar_docs.hip and
 * the selection of topic_docs.hip) from sparse topic weights that are stored by document.  The rule is stated once, in
 * isle_amd/csrc/simdocs_host.h:
 *   a row is a document's entries (topic, weight), topics ascending strictly; its document is doc = doc_base + row.  A query is the same kind
 *   of list.  Every weight is finite, >= 0 and < 2^31 (-0.0 counts as 0); the first entry outside that domain is named in the refusal.
 *   candidates  row r is a candidate of query q when some topic is STORED in both, whatever the weights (a shared topic of weight 0 makes a
 *               candidate of score 0), unless doc_base + r == exclude[q] (0xffffffff: nothing is excluded).  candidates[q] counts them (all ranks).
 *   score       a the row's, b the query's weight at a common topic, common topics ascending:
 *     ISLE_SIM_DOT            s = sum (double)a (double)b                             score = (float)s
 *     ISLE_SIM_COSINE         s likewise; nr = sum over ALL entries of the row (double)a (double)a, nq likewise over the query;
 *                             den = sqrtf((float)nr) * sqrtf((float)nq) in fp32       score = den == 0 ? 0 : (float)s / den (fp32 division)
 *     ISLE_SIM_BHATTACHARYYA  s = sum (double)sqrtf(a * b), product and root in fp32  score = (float)s   (distributions: 1 - Hellinger^2)
 *   result      isle_hip_topic_top_docs' with the query in the place of the topic: key = ord(bits(score)) << 32 | ~doc, the larger key wins
 *               (the higher score, the smaller document among bit-equal scores).  docs[q n + i] / scores[q n + i] for
 *               i < counts[q] = min(n, candidates[q]), the unused slots 0xffffffff / 0.0f; candidates is nullable.
 * Device and host agree bit for bit: a product of two fp32 values is exact in double (s + a b rounds once with or without an fma), the rest
 * is single IEEE operations.  NOT CERTIFIED: fp32 products a * b that are subnormal (BHATTACHARYYA, weights below 2^-60).
 * source, doc_base, num_rows, doc_offsets / topic / value are isle_hip_topic_top_docs'.  num_topics is the column count of the last
 * isle_hip_infer_resident (INFER), the topic model's (SUMS); another value is refused.
 * The queries: query_rows non-null: rows query_rows[q] of the source, gathered on the device (q_* are ignored); where exclude is null,
 * exclude[q] defaults to doc_base + query_rows[q]: a document is not its own neighbour.  Otherwise the caller's CSR q_offsets
 * (num_queries + 1) / q_topic / q_weight, uploaded for the call and checked on the host in this order, each condition over all queries
 * before the next: the offsets ascend from 0, every topic < num_topics, the topics of a query ascend strictly, the weight domain.
 * ISLE_E_ARG, decided before any launch or collective: an unknown source or measure, num_queries outside 1 .. ISLE_SIMDOCS_MAX_QUERIES, n
 * outside 1 .. ISLE_TOPDOCS_MAX_N, world x n > 8192, doc_base + rows > 0xfffffff1, a query_rows[q] that is not below the rows, null docs /
 * scores / counts, a bad query, the sources' own conditions.  Found on the device: a row entry with a weight outside the domain (the text names
 * the entry, its row and its value), a topic >= num_topics or topics that do not ascend (HOST); 2^32 candidate pairs or more on a rank ("ask
 * with fewer queries").  After any refusal the context is usable and nothing resident has changed.
 * The queries are densified into a num_topics x Qp fp32 table (Qp = num_queries rounded up to a power of two) that lives in LDS, copied once
 * per workgroup, while it fits in 64 KiB, else in global memory (route_host.h route_simdocs_table).  isle_hip_simdocs_table_form sets which
 * home the context asks for: a setting of the context, not an environment variable; LDS where the table does not fit is global all the same.
 * Both homes give the same bits.
 * Document shards (world > 1): COLLECTIVE, as isle_hip_topic_top_docs.  ALL RANKS CALL TOGETHER with the same source, measure, num_topics, n,
 * num_queries (agreed: ISLE_E_COMM otherwise), the same queries and exclude (one agreed 64-bit hash: ISLE_E_COMM otherwise) and their own
 * doc_base.  A bad row entry or too many pairs on one rank travels as one all-reduced word ahead of the selection: every rank returns
 * ISLE_E_ARG, the rank that holds the entry names it.  Every rank returns the corpus's lists, bit-identical, the lists one rank holding all
 * rows returns.  query_rows WITH world > 1 IS REFUSED: the row lives on one rank, and exchanging it is out of scope.
 * The call changes nothing resident and keeps nothing: a second call returns the same arrays, and isle_hip_get_infer_entries,
 * isle_hip_infer_text, isle_hip_topic_top_docs and isle_hip_doc_report_text return what they returned before.  Device memory of a call
 * (derived, not measured): 12 bytes per candidate pair (query, score, document), 8 (rows + 1) bytes of offsets, 4 bytes per row of counts,
 * the table; every row a candidate of every query is 64 M pairs = 0.77 GB at 1 M rows x 64 queries.  Device time is booked under
 * ISLE_T_INFER for ISLE_TOPDOCS_INFER and under ISLE_T_POST otherwise.  Measured on one rank at configuration 2 only
 * (tools/similar_docs_probe.py, profiles/similar_docs_c2.jsonl; the README row); at the one shape where the table's two homes were timed
 * against each other (64 queries, 200 topics) the global home was the faster one.  NO TIME IS MEASURED on several ranks. */
#define ISLE_SIM_DOT 0
#define ISLE_SIM_COSINE 1
#define ISLE_SIM_BHATTACHARYYA 2
#define ISLE_SIMDOCS_MAX_QUERIES 64
#define ISLE_SIMDOCS_TABLE_AUTO 0   /* the rule's own choice */
#define ISLE_SIMDOCS_TABLE_LDS 1    /* LDS, copied once per workgroup, while the table fits in 64 KiB */
#define ISLE_SIMDOCS_TABLE_GLOBAL 2 /* global memory */
int isle_hip_similar_docs(isle_ctx* ctx, int source /* ISLE_TOPDOCS_INFER | _SUMS | _HOST */, int measure, int num_topics, int n, uint64_t doc_base,
                          uint64_t num_rows, const int64_t* doc_offsets, const uint32_t* topic, const float* value, int num_queries,
                          const uint64_t* query_rows /* nullable */, const int64_t* q_offsets, const uint32_t* q_topic, const float* q_weight,
                          const uint32_t* exclude /* nullable: num_queries documents, 0xffffffff = none */, uint32_t* docs, float* scores,
                          uint32_t* counts, uint64_t* candidates /* nullable */);
int isle_hip_simdocs_table_form(isle_ctx* ctx, int form);
/* Topic prevalence by group of documents, summed on the device (isle_amd/csrc/topic_prevalence.hip and api_stages.cpp): how much of the
 * corpus each topic is, and how that differs between parts of it.  The sources and the row form are isle_hip_topic_top_docs': the resident
 * inference entries (ISLE_TOPDOCS_INFER), the resident catchword sums (ISLE_TOPDOCS_SUMS), or a CSR doc_offsets / topic / value uploaded
 * for the call (ISLE_TOPDOCS_HOST), topics ascending strictly within a row; for INFER and SUMS num_rows and the three arrays are ignored.
 * The rule, stated once as plain C++ in isle_amd/csrc/prevalence_host.h:
 *   weights  every weight is finite, >= 0 and < 2^31; -0.0 counts as 0 (its term is +0.0)
 *   labels   groups: one uint32 per row, the caller's, uploaded for the call; NULL: every row has label 0 and num_groups must be 1.
 *            ISLE_GROUP_NONE: the row belongs to no group; it is counted in *unlabelled and nowhere else.  Any other label >= num_groups
 *            is refused.
 *   per row  rs_r = 0.0, then rs_r = rs_r + (double)w over the row's entries in stored order.  The term x_r(t) of a stored topic is
 *            (double)w, with normalise (double)w / rs_r (one IEEE division; +0.0 where rs_r == 0); +0.0 for a topic the row does not store.
 *            The dominant topic of a row with entries is the entry with the largest weight, the smaller topic among equal weights
 *            (-0 = +0); a row without entries has none.
 *   outputs  for every group g < num_groups and topic t < num_topics, the tables num_groups x num_topics group-major:
 *            docs[g]        the rows labelled g, rows without entries included
 *            count[g,t]     the rows of g that store t, whatever the weight
 *            dominant[g,t]  the rows of g whose dominant topic is t
 *            sum[g,t]       r_0 < r_1 < .. < r_{n-1} the rows of g: v0_i = x_{r_i}(t), v(j+1)_i = (((0.0 + vj_{64i}) + vj_{64i+1}) + ..
 *                           + vj_{64i+63}) over the indices that exist, every + one IEEE double addition, until one value is left
 *                           (at least once); n = 0 gives 0.0.
 * The radix-64 tree is part of the rule: every level is parallel, and the device and the header's host loop agree bit for bit, on every
 * call.  Against the exact rational sum, without normalise, the relative error is at most c u / (1 - c u), c = count[g,t], u = 2^-53
 * (Higham's bound for any order of summation).  The caller forms mean[g,t] = sum[g,t] / (double)docs[g], NaN where docs[g] == 0.
 * Limits: 1 <= num_topics <= 8192, 1 <= num_groups, num_groups x num_topics <= ISLE_PREVALENCE_MAX_CELLS, fewer than 2^32 rows.
 * ISLE_E_ARG, decided before any launch: an unknown source, normalise outside {0, 1}, the limits, NULL outputs (unlabelled may be NULL),
 * groups == NULL with num_groups != 1, the sources' own conditions as isle_hip_topic_top_docs states them, and world > 1, before any
 * collective: a bit-equal sum across ranks needs the list order exchanged, which is not built.  Found on the device, each naming the first
 * offender through one 64-bit atomicMin: a bad label (the first such row; reported before a bad entry), and the first entry with a topic
 * >= num_topics, topics that do not ascend, or a weight outside the domain.  After any refusal the context is usable.  The call changes
 * nothing resident and keeps nothing.  Device time: ISLE_T_INFER for INFER, ISLE_T_POST otherwise.
 * The private table of a block's owner holds one tile of topics: 1024 (8 KiB of doubles), or 64 where isle_hip_prevalence_tile_form asks
 * for the narrow form, which exists so that small tests cross tile edges; topics beyond a tile are taken tile after tile, and both forms
 * give the same bits.  The form is a setting of the context, not an environment switch.
 * Device memory of a call, derived, not measured (R rows, E entries, G groups, k topics, w = min(k, tile)): the tables 8 G (1 + 3 k)
 * bytes; 8 R bytes of row sums with normalise; with labels 28 R bytes of labels and sort pairs and 1.5 R of the sort's histogram (the
 * context's sort scratch, which stays with the context); the level bases 8 (L + 1) (G + 1), L <= 6; the level-0 partials
 * (R / 64 + G) w 8 bytes and their parents, a 64th of that, reused per tile; a HOST source adds its upload, 8 (R + 1) + 8 E. */
#define ISLE_GROUP_NONE 0xffffffffu
#define ISLE_PREVALENCE_MAX_CELLS (1u << 24)
#define ISLE_PREVALENCE_TILE_AUTO 0
#define ISLE_PREVALENCE_TILE_WIDE 1    /* 1024 topics per table */
#define ISLE_PREVALENCE_TILE_NARROW 2  /* 64 topics per table: for the tests */
int isle_hip_topic_prevalence(isle_ctx* ctx, int source /* ISLE_TOPDOCS_INFER | _SUMS | _HOST */, int num_topics, uint64_t num_rows,
                              const int64_t* doc_offsets, const uint32_t* topic, const float* value, const uint32_t* groups /* nullable */,
                              uint32_t num_groups, int normalise, uint64_t* docs, uint64_t* unlabelled /* nullable */, uint64_t* count,
                              uint64_t* dominant, double* sum);
int isle_hip_prevalence_tile_form(isle_ctx* ctx, int form);
/* Held-out scores per document on the device (isle_amd/csrc/score_docs.hip and api_stages.cpp): how well given topic weights predict the
 * entries of a sparse matrix of counts; with weights fitted on one part of every document and the other part scored, document completion.
 * The model is isle_hip_infer_resident's (`which`, model_host, vocab x ncols column-major).  The weights are the rows of the last
 * isle_hip_infer_resident (ISLE_TOPDOCS_INFER: num_rows must be its row count) or a CSR w_offsets / w_topic / w_weight uploaded for the call
 * (ISLE_TOPDOCS_HOST), topics ascending strictly within a row.  The entries are documents [doc_begin, doc_begin + num_rows) of the resident
 * A (ISLE_SCORE_RESIDENT; with ISLE_TOPDOCS_INFER doc_begin must be that call's doc_begin) or a CSC counts / rows / offsets uploaded for
 * the call (ISLE_SCORE_HOST: offsets num_rows + 1 ascending from 0, doc_begin ignored).  Row r of the weights scores document r of the entries.
 * The rule, stated once as plain C++ in isle_amd/csrc/score_host.h, for a document with weights (t_0 < t_1 < .., th_j) and an entry (w, c):
 *   weights  th'_j = (double)th_j; with normalise (double)th_j / s_d (one IEEE division), s_d the row's sum of (double)th_j in stored order
 *            from 0.0; a row whose sum is 0 then has no weights.  Every weight is finite, >= 0 and < 2^31.
 *   z        z = fma((double)M[w,t_j], th'_j, z) over j ascending from z = 0.0: fused, one rounding per stored topic.  Without normalise
 *            every product is exact in double, so an unfused loop gives the same bits.
 *   classes  z NaN, infinite or negative: unscored.  Else z < floor (floor > 0; z == 0 included): scored at floor and counted in floored.
 *            Else z == 0: unscored.  Else scored at z.  An unscored entry adds nothing to score and tokens and is counted in
 *            unscored_entries and, with (double)c, in unscored_tokens: a NaN column of a catch model never poisons a document.
 *   term     ISLE_SCORE_LOG: (double)c * log(z); ISLE_SCORE_PROB: (double)c * z; the product rounded once, never fused into the sum
 *   sums     per document of n entries: lane i < 64 adds the terms of the entries i, i + 64, .. ascending from 0.0, then
 *            p[i] = p[i] + p[i + s] for s = 32, 16, .., 1; the sum is p[0].  score, tokens (the (double)c of scored entries) and
 *            unscored_tokens are summed so.  z_out (nullable, ISLE_SCORE_HOST only): z of every entry, in entry order.
 * ISLE_SCORE_PROB without normalise equals the header's host loop bit for bit, as do z_out, tokens and the counters in every mode; two
 * calls give the same bits in every mode; for ISLE_SCORE_LOG |score - exact| <= g / (1 - g) sum c |ln z|, g = (2 K + 1 + ceil(n / 64) + 6)
 * 2^-53, K the device logarithm's error in ulps (profiles/score_certificate.md).  Corpus totals are not formed on the device:
 * isle_hip_score_total is the ascending sequential sum on the host (no context, no device), so that every caller gets the same bits and
 * the arrays of document shards side by side give the single-rank total; perplexity = exp(-total score / total tokens) for ISLE_SCORE_LOG.
 * ISLE_E_ARG, decided before any launch: an unknown source or measure, normalise outside {0, 1}, floor not finite or < 0, ncols outside
 * [1, 1024], the model's conditions as isle_hip_infer_resident states them (vocab must be A's with ISLE_SCORE_RESIDENT), no resident
 * result, num_rows or doc_begin that differ from the resident result's, a document range outside A, offsets that do not ascend from 0,
 * NULL arrays, z_out with ISLE_SCORE_RESIDENT.  Found on the device, each naming the first offender through one 64-bit atomicMin: a
 * weight entry with a topic >= ncols, topics that do not ascend, or a weight outside the domain (before any entry is read); then an entry
 * with a word >= vocab or a count that is not finite or < 0.  After any refusal the context is usable.  The call changes nothing resident
 * and keeps nothing.  Device time: ISLE_T_INFER.  world > 1: no collective; every rank scores its own rows, ISLE_MODEL_AVG is refused as
 * isle_hip_infer_resident refuses it, and the ranks' arrays side by side are the single-rank arrays bit for bit.
 * Device memory of a call, derived, not measured: the packed model 4 vocab round4(ncols) bytes, 8 num_rows of row sums, 32 num_rows of
 * outputs, 8 bytes per entry of z_out, and the uploads of the HOST forms. */
#define ISLE_SCORE_RESIDENT 0
#define ISLE_SCORE_HOST 1
#define ISLE_SCORE_LOG 0
#define ISLE_SCORE_PROB 1
int isle_hip_score_docs(isle_ctx* ctx, int which, const float* model_host, uint64_t vocab, int ncols, int weights_source, uint64_t num_rows,
                        const int64_t* w_offsets, const uint32_t* w_topic, const float* w_weight, int entries_source, uint64_t doc_begin,
                        const float* counts, const uint32_t* rows, const int64_t* offsets, int measure, int normalise, double floor,
                        double* score, double* tokens, uint32_t* unscored_entries, double* unscored_tokens, uint32_t* floored,
                        double* z_out /* nullable */);
int isle_hip_score_total(const double* v, uint64_t n, double* out);
/* The avg_doc_sz of the resident count matrix as the context holds it (see above; computed on first use).  world > 1: the corpus value
 * over all ranks' documents, collective where it has to be computed (see isle_hip_infer_resident).  ISLE_E_ARG: no count matrix, out null. */
int isle_hip_avg_doc_sz(isle_ctx* ctx, float* out);
/* The shape of the resident count matrix A and its place in the corpus as the upload, the feed or the windowed tdf stream gave them
 * (each nullable); separate from isle_hip_shape, which describes B.  ISLE_E_ARG: no count matrix. */
int isle_hip_counts_shape(isle_ctx* ctx, uint64_t* vocab_size, uint64_t* num_docs, uint64_t* nnz, uint64_t* doc_offset,
                          uint64_t* docs_global);

/* ---- the vocabulary pruned by document frequency, on the resident count matrix (isle_amd/csrc/vocab.hip) ----------------------------------
 * What filter_extremes / min_df / max_df do elsewhere, where A lies.  The rule is stated once, in isle_amd/csrc/vocab_host.h:
 *   df[w]     the documents of the whole corpus (all ranks) whose column of A holds word w (a column holds a word at most once: its entries)
 *   max_df'   max_df, or the corpus's document count (docs_global of isle_hip_counts_shape) where max_df == 0
 *   passes    min_df <= df[w] <= max_df'
 *   keep_n    > 0 and more than keep_n words pass: only the keep_n passers with the largest key (uint64)df[w] << 32 | (uint32)~w stay: the
 *             larger df wins, the smaller word id among equal df
 *   new ids   the kept words are numbered 0 .. new_vocab - 1 in ascending old id, kept_words[new] = old: every column stays sorted
 *   new A     every document keeps its entries of kept words in their order, counts bit for bit, rows renumbered; the documents, the document
 *             offset and docs_global stay; a document may become empty (empty documents are legal everywhere)
 *   emptied   the documents of the corpus that had entries and have none afterwards
 * isle_hip_word_doc_freq: df (vocab_size u32, nullable) and nothing else; it changes nothing resident.
 * isle_hip_prune_vocab: df (the OLD vocab_size, nullable), kept_words (room for the old vocab_size, new_vocab written, nullable), new_vocab,
 * nnz (this rank's entries afterwards), docs_emptied (the corpus's); each nullable.  One histogram over the entries (32-bit integer sums:
 * order-independent), the rule on the fetched table on the host (4 bytes per word), one ordered compaction (flags, a 64-bit scan, a pack into
 * twin buffers that are swapped in).  For everything resident the call is an ingest of the pruned matrix: what a fresh count matrix voids
 * (the corpus average, the catchwords, the models, the resident inference result) is void, what it leaves (B, U, the partition) stays; a
 * prune is followed by isle_hip_threshold like any ingest.
 * ISLE_E_ARG, decided before anything is rewritten (A and everything resident stay exactly as they were): no count matrix,
 * min_df > max_df', keep_n >= 2^32, no word kept.
 * Document shards (world > 1): both calls are COLLECTIVE.  ALL RANKS CALL TOGETHER, a rank without documents included, with the same
 * vocab_size, min_df, max_df and keep_n (checked: ISLE_E_COMM otherwise).  df is all-reduced (u32 sum over vocab_size), the rule runs
 * replicated, docs_emptied is all-reduced: df, kept_words, new_vocab, docs_emptied and the refusals that depend on df are bit-identical on
 * every rank; the new A and nnz are the shard's own, and equal the single-rank result cut at the same document bounds.
 * The histogram has two forms that give the same integers: counters private to a workgroup in LDS over vocabulary parts, flushed with one
 * atomic per (workgroup, word) (the default), and one global atomic per entry.  isle_hip_vocab_hist_form sets which one the context asks
 * for (the rule: route_host.h route_vocab_hist); the switch is the context's and not an environment variable.  Device memory of a prune:
 * 12 bytes per entry (flags, positions) and the twin buffers; device time is booked under ISLE_T_INGEST. */
#define ISLE_VOCAB_HIST_AUTO 0   /* the rule's own choice */
#define ISLE_VOCAB_HIST_LDS 1    /* workgroup-private counters in LDS, one atomic per (workgroup, word) */
#define ISLE_VOCAB_HIST_GLOBAL 2 /* one global atomic per entry */
int isle_hip_vocab_hist_form(isle_ctx* ctx, int form);
int isle_hip_word_doc_freq(isle_ctx* ctx, uint32_t* df);
int isle_hip_prune_vocab(isle_ctx* ctx, uint64_t min_df, uint64_t max_df, uint64_t keep_n, uint64_t* new_vocab, uint32_t* kept_words, uint32_t* df,
                         uint64_t* nnz, uint64_t* docs_emptied);

/* ---- documents pruned by length and as exact duplicates, on the resident count matrix (isle_amd/csrc/docs.hip) ----------------------------
 * The other half of the hygiene a front end does before training: documents of too few or too many words or tokens go, and of documents
 * with identical columns only the first stays.  The rule is stated once, in isle_amd/csrc/docs_host.h.  For a local document d:
 *   words[d]    its entries (distinct words; u32)          tokens[d]   the sum of (uint64)count over them (exact; u64)
 *   max_words'  max_words, or no bound where max_words == 0 (likewise max_tokens')
 *   passes      min_words <= words[d] <= max_words'  and  min_tokens <= tokens[d] <= max_tokens'
 *   equal       the same number of entries, the same rows and the same count BITS, entry by entry; all empty documents are equal
 *   first_of[d] with drop_duplicates: the smallest local document equal to d; without it: d
 *   kept        passes  and  first_of[d] == d
 *   new ids     the kept documents numbered 0 .. new_docs - 1 in ascending old id; kept_docs[new] = the old number in the corpus
 *               (doc_offset + d)
 *   new A       the kept documents' columns, entries in order, rows unchanged, counts bit for bit; the vocabulary stays
 * isle_hip_doc_lengths: words and tokens of this rank's documents (each nullable); changes nothing resident; never collective.
 * isle_hip_doc_duplicates: first_of over ALL local documents (nullable) and the number of documents that are not the first of their kind;
 * changes nothing resident.
 * isle_hip_prune_docs: new_docs and nnz are this rank's afterwards, kept_docs has room for the old document count (new_docs written),
 * first_of (the old document count, nullable) reports 0xffffffff for a document dropped by length and the representative's old local
 * number for one dropped as a duplicate; docs_global is the corpus's document count afterwards; dropped[3] the corpus's documents below
 * the bounds, above them, and duplicates among the passers (the first failing test decides, in the order words-min, tokens-min,
 * words-max, tokens-max).  Each output is nullable.  For everything resident the call is an ingest of the pruned matrix (as
 * isle_hip_prune_vocab): B is the old A's until isle_hip_threshold runs again.
 * ISLE_E_ARG, decided before anything is rewritten (A and everything resident stay exactly as they were): no count matrix,
 * min_words > max_words', min_tokens > max_tokens', drop_duplicates outside {0, 1}, no document kept in the corpus, and duplicates with
 * several ranks (below).
 * On the device: one pass over the entries gives words, tokens and a 64-bit hash per document (a commutative sum of a mix of
 * (row, count bits): order-independent); the documents are sorted by hash (stable: ascending within a hash), and inside every run of equal
 * hashes contents are compared with the run's current head, round by round, until every document has found the first of its kind: the hash
 * is mechanism, equality of content is the rule.  isle_hip_doc_hash_form cuts the hash to its 2 low bits (ISLE_DOC_HASH_NARROW) so that
 * every run holds many unequal documents: the same result by many more rounds, for the tests and the probe; a setting of the context, not
 * an environment variable.  Then a scan of the kept flags, a 64-bit scan of the kept lengths, a copy into twin buffers that are swapped in.
 * Device time is booked under ISLE_T_INGEST.
 * Document shards (world > 1): isle_hip_prune_docs with drop_duplicates == 0 is COLLECTIVE.  ALL RANKS CALL TOGETHER, a rank without
 * documents included, with the same vocab_size and the same five arguments (checked: ISLE_E_COMM otherwise).  dropped is all-reduced, the
 * ranks' kept counts are exchanged: each rank's new doc_offset is the sum over the lower ranks, docs_global the sum over all; "no document
 * kept" is the same refusal on every rank; a rank may end with no documents; every rank's new A is its slice of the single-rank result.
 * drop_duplicates != 0 and isle_hip_doc_duplicates are refused with ISLE_E_ARG where world > 1, before any collective: equality across
 * ranks needs the contents exchanged, which is out of scope. */
#define ISLE_DOC_HASH_AUTO 0
#define ISLE_DOC_HASH_FULL 1   /* 64-bit document hash */
#define ISLE_DOC_HASH_NARROW 2 /* the same hash cut to its 2 low bits: every run holds many unequal documents; for the tests and the probe */
int isle_hip_doc_hash_form(isle_ctx* ctx, int form);
int isle_hip_doc_lengths(isle_ctx* ctx, uint32_t* words, uint64_t* tokens);
int isle_hip_doc_duplicates(isle_ctx* ctx, uint32_t* first_of, uint64_t* n_duplicates);
int isle_hip_prune_docs(isle_ctx* ctx, uint64_t min_words, uint64_t max_words, uint64_t min_tokens, uint64_t max_tokens, int drop_duplicates,
                        uint64_t* new_docs, uint32_t* kept_docs, uint32_t* first_of, uint64_t* nnz, uint64_t* docs_global, uint64_t dropped[3]);

/* ---- two topic models compared: L1 distances and topic matching (isle_amd/csrc/model_compare.hip) ---------------------------------------
 * "Is this model the same as that one": this run against a file loaded back, the catch model against the average model, a run after a
 * prune against the run before, a recovered model against planted topics.  The rule is stated once, in isle_amd/csrc/match_host.h.
 *   dist[i][j]  sum over the words w of |(double)a[w, i] - (double)b[w, j]|, a (vocab x cols_a) and b (vocab x cols_b) column-major fp32;
 *               row-major cols_a x cols_b doubles.  Terms formed and summed in double, in an order that is a function of (vocab, cols_a,
 *               cols_b, slices) alone (no floating-point atomics: two calls give the same bits); |dist - exact| <= vocab 2^-53 exact.  A
 *               column with any non-finite entry (the average model's empty clusters) makes its row or column of dist NaN.
 *   matching    greedy: an edge (i, j) exists where dist[i][j] is finite; the edges are walked in the order (dist, i, j) (< on doubles:
 *               -0 equals +0) and (i, j) is matched when both are free.  match_a[i] = j or -1, match_b[j] = i or -1, match_dist[i] = the
 *               matched distance or NaN, mean_dist = the matched distances summed in ascending i over n_matched (NaN where nothing
 *               matched).  The optimal (Hungarian) assignment is out of scope; the greedy mean is an upper bound of the optimal one.
 *               On the device: rounds of mutually best pairs, one counter read back per round; rounds = the rounds that matched a pair.
 * isle_hip_compare_models: each side is named as in isle_hip_model_top_words (which / model_host / cols; ISLE_MODEL_HOST uploads the
 * caller's model for the call); both may be host models, both may name the same resident model (an exactly-0 diagonal).  The matcher runs
 * on the device matrix where match_a, match_b, match_dist, n_matched or mean_dist is asked for; every output is nullable and only what is
 * asked for is fetched.  Nothing resident changes.  Device time: ISLE_T_POST.  With several ranks every rank answers for itself, no
 * collective; ISLE_MODEL_AVG is refused there like in every reader of a model.
 * isle_hip_match_topics: the same matcher on the caller's na x nb row-major matrix (ties, +-0, +-inf and NaN patterns real distances never show).
 * isle_hip_model_dist_slices: how many word slices the distance kernel cuts the vocabulary into (0: the rule route_model_dist_slices of
 * isle_amd/csrc/route_host.h; >= 1: that many, capped at ceil(vocab / MC_CHUNK)); a setting of the context, not an environment variable.
 * ISLE_E_ARG, decided before any launch (texts: match_host.h): an unknown model, a resident model that does not exist, vocab or cols
 * other than a resident side's, vocab == 0 or > 0xfffffff0, cols_a or cols_b outside 1 .. 8192 (the matrix is cols_a cols_b 8 bytes,
 * 512 MB at the limit), a null host model with ISLE_MODEL_HOST, na or nb outside 1 .. 8192, a null dist_host, slices < 0. */
int isle_hip_model_dist_slices(isle_ctx* ctx, int slices);
int isle_hip_compare_models(isle_ctx* ctx, int which_a, const float* a_host, int cols_a, int which_b, const float* b_host, int cols_b, uint64_t vocab,
                            double* dist, int32_t* match_a, int32_t* match_b, double* match_dist, uint64_t* n_matched, double* mean_dist, uint32_t* rounds);
int isle_hip_match_topics(isle_ctx* ctx, const double* dist_host, int na, int nb, int32_t* match_a, int32_t* match_b, double* match_dist,
                          uint64_t* n_matched, double* mean_dist, uint32_t* rounds);

/* ---- measurement ----------------------------------------------------------------------- */
/* Per-kernel-family device time accumulated with HIP events on the context's stream since the
 * last reset (only while enabled; enabling adds event records around each launch).
 * Families: see ISLE_T_* below. */
enum {
  ISLE_T_GRAM_PASS1 = 0,   /* Y = B^T X   (CSC gather)            */
  ISLE_T_GRAM_PASS2 = 1,   /* Z = B Y     (chunked-CSR gather + chunk reduce) */
  ISLE_T_ORTHO = 2,        /* V^T F, F -= V H                      */
  ISLE_T_QR = 3,           /* panel QR (Gram, apply)               */
  ISLE_T_EVD = 4,          /* small symmetric EVD                  */
  ISLE_T_ROTATE = 5,       /* Ritz rotation (every restart + the final extraction of U) */
  ISLE_T_PROJECT = 6,      /* P = U^T B                            */
  ISLE_T_KMPP = 7,         /* k-means++ rounds                     */
  ISLE_T_LLOYD_PROJ = 8,   /* projected Lloyd assign + update      */
  ISLE_T_SPARSE_ASSIGN = 9,/* sparse Lloyd: distances + argmin     */
  ISLE_T_SPARSE_UPDATE = 10,/* sparse Lloyd: centroid update       */
  ISLE_T_BAND_BUILD = 11,  /* chunked-CSR copy of B (per solve)   */
  ISLE_T_COMM = 12,        /* collectives                          */
  ISLE_T_THRESHOLD = 13,   /* A -> B thresholding (upstream stage) */
  ISLE_T_POST = 14,        /* catchwords / topic model / edge topics (downstream stage) */
  ISLE_T_INGEST = 15,      /* tdf text -> count matrix */
  ISLE_T_INFER = 16,       /* ISLEInfer: multiplicative-weights inference */
  ISLE_T_LIFT = 17,        /* centres = U C_lowd (left_multiply_by_U_Spectra)  */
  ISLE_T_COUNT = 18
};
/* on: 0 = off, 1 = events around every launch, 2 = around the Gram applications only (what bench.py's timed region uses): the
 * LDS-banded form then books one event pair per application — both passes and the gap between them — under ISLE_T_GRAM_PASS1. */
int isle_hip_timing_enable(isle_ctx* ctx, int on);
int isle_hip_timing_reset(isle_ctx* ctx);
/* ms[ISLE_T_COUNT], launches[ISLE_T_COUNT] */
int isle_hip_timing_get(isle_ctx* ctx, double* ms, uint64_t* launches);
int isle_hip_synchronize(isle_ctx* ctx);

/* ---- near-duplicate documents found and pruned by MinHash, on the resident count matrix (isle_amd/csrc/near_dups.hip) ----------------------
 * Documents that differ only in a date, a signature or a boilerplate sentence do to the trainer what exact copies do; exact equality
 * (isle_hip_prune_docs) does not see them.  The standard answer, on the device: MinHash signatures over a document's word set, banding
 * to find candidate pairs, an exact Jaccard test on the candidates.  The rule is stated once, in isle_amd/csrc/neardup_host.h; every
 * quantity is an integer.  For a local document d:
 *   S_d          the rows of its entries (counts are ignored), n_d their number
 *   similar      inter den >= num uni in 64-bit integers, inter = |S_a & S_b|, uni = n_a + n_b - inter; the threshold is the rational
 *                num/den, 1 <= num <= den <= 65535.  Two empty documents are similar, an empty and a non-empty one never.
 *   sig[d][i]    the minimum over w in S_d of mix(((i + 1) << 32) | w), i < H = bands rows_per_band (mix: docs_host.h docs_mix); all ones
 *                for an empty document.  1 <= bands <= 64, 1 <= rows_per_band <= 8, H <= 128.
 *   key[b][d]    k = 0; k = mix(k ^ sig[d][b rows_per_band + j]) for j = 0 .. rows_per_band - 1
 *   resolution   parent[d] = d.  Band by band, in order: the live documents (parent[d] == d) are grouped by key[b]; inside a group, in
 *                ascending document order, the first document is a leader, every later one is tested against the group's leaders in the
 *                order they became leaders and takes the first similar one as its parent, or becomes a leader itself.
 *   parent[d]    the verified neighbour: parent[d] < d and similar(d, parent[d]) where d was attached, d itself otherwise
 *   first_of[d]  the root of the parent chain; kept <=> first_of[d] == d; n_dropped: the documents not kept
 *   pairs_tested the (document, leader) tests made; rounds: the largest number of leaders in a group, summed over the bands
 *   new A        the kept documents' columns in ascending old id, entries in order, counts bit for bit; kept_docs[new] = doc_offset + old
 * Documents with the same word set always share first_of; with num == den the partition is exactly "equal word sets".
 * isle_hip_neardup_key_form: ISLE_NEARDUP_KEY_NARROW cuts the band keys to their 2 low bits, so that every group holds many dissimilar
 * documents (for the tests); it decides which pairs become candidates, so first_of may differ between the forms where num < den: each
 * form answers as the rule states for that form.  A setting of the context, not an environment variable.
 * isle_hip_doc_signatures: sig (docs x H row-major, nullable) and the band keys, not cut (bands x docs band-major, nullable).
 * isle_hip_doc_jaccard: inter and uni (each nullable) of the caller's n_pairs pairs (a[i], b[i]) of local documents; a[i] == b[i] is
 * allowed; a document >= the local document count is refused, the first such pair named.
 * isle_hip_doc_near_duplicates: parent, first_of (the local document count each) and the three counters; each output nullable.
 * None of the three changes anything resident.
 * isle_hip_prune_near_docs: the documents not kept leave A.  new_docs and nnz are this rank's afterwards, kept_docs has room for the old
 * document count (new_docs written), parent and first_of are the old documents'; docs_global the corpus's document count afterwards.
 * Each output is nullable.  For everything resident the call is an ingest of the pruned matrix, as isle_hip_prune_docs is: B is the old
 * A's until isle_hip_threshold runs again.  Roots stay, so some document is always kept.
 * ISLE_E_ARG, decided before anything is launched or rewritten (A and everything resident stay exactly as they were; the texts:
 * neardup_host.h): no count matrix; num, den, bands or rows_per_band out of range; world > 1, before any collective (similarity across
 * ranks needs the contents exchanged: out of scope).
 * On the device: a wave per document, lane i owns hash function i; the band keys are folded inside the wave and stored band-major; per
 * band the live documents are sorted by key (stable) and resolved in rounds against their run's current leader: the length filter, then
 * the shorter document's rows searched in the longer one's; pointer jumping gives the roots; isle_hip_prune_docs's compaction builds the
 * new A.  Beyond A the call holds 8 bands docs bytes of keys and the sort's twin buffers.  Device time is booked under ISLE_T_INGEST. */
#define ISLE_NEARDUP_KEY_AUTO 0
#define ISLE_NEARDUP_KEY_FULL 1   /* the band's 64-bit key */
#define ISLE_NEARDUP_KEY_NARROW 2 /* the same key cut to its 2 low bits: every group holds many dissimilar documents; for the tests */
int isle_hip_neardup_key_form(isle_ctx* ctx, int form);
int isle_hip_doc_signatures(isle_ctx* ctx, int bands, int rows_per_band, uint64_t* sig, uint64_t* keys);
int isle_hip_doc_jaccard(isle_ctx* ctx, uint64_t n_pairs, const uint32_t* a, const uint32_t* b, uint32_t* inter, uint32_t* uni);
int isle_hip_doc_near_duplicates(isle_ctx* ctx, uint64_t num, uint64_t den, int bands, int rows_per_band, uint32_t* parent, uint32_t* first_of,
                                 uint64_t* n_dropped, uint64_t* pairs_tested, uint64_t* rounds);
int isle_hip_prune_near_docs(isle_ctx* ctx, uint64_t num, uint64_t den, int bands, int rows_per_band, uint64_t* new_docs, uint32_t* kept_docs,
                             uint32_t* parent, uint32_t* first_of, uint64_t* nnz, uint64_t* docs_global, uint64_t* n_dropped);

#ifdef __cplusplus
}
#endif
#endif /* ISLE_HIP_H */
