// isle_amd/csrc/common.h — internal declarations shared by the HIP translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <atomic>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <string>
#include <thread>
#include <vector>

#include "gl_plan.h"
#include "knobs.h"
#include "resident_host.h"
#include "route_host.h"

// ------------------------------------------------------------------------------------------
// Launch guard.  On this stack a kernel launch of 2^32 threads or more (grid x block) does not run and reports NO error — round 3's
// yy2_scan_k at 10 M documents left collapsed partitions that way.  Every launch of the library goes through this redefinition of
// hipLaunchKernelGGL: a launch that does not fit is not issued and is remembered (file:line), and the HIPCHK that follows every launch
// turns it into ISLE_E_ARG with that location.  Index spaces that can exceed the limit (D x k = 10^10 at config 3) are walked by
// grid-stride loops or chunked launches at their call sites; this guard is what makes a missed one loud.
// ------------------------------------------------------------------------------------------
struct IsleLaunchRefused {
  const char* file = nullptr;
  int line = 0;
  unsigned long long threads = 0;
};
inline IsleLaunchRefused& isle_launch_refused() {
  static thread_local IsleLaunchRefused r;
  return r;
}
inline bool isle_launch_fits(dim3 g, dim3 b, const char* file, int line) {
  const unsigned long long blocks = (unsigned long long)g.x * g.y * g.z, threads = blocks * ((unsigned long long)b.x * b.y * b.z);
  if (threads < (1ull << 32)) return true;  // (and with it every dimension's work-item count, which is what the dispatch packet holds in 32 bits)
  IsleLaunchRefused& r = isle_launch_refused();
  if (!r.file) {
    r.file = file;
    r.line = line;
    r.threads = threads;
  }
  fprintf(stderr, "[isle_hip] %s:%d: a launch of %llu threads (grid %u x %u x %u) was refused: 2^32 threads or more do not run on this stack\n", file, line, threads,
          g.x, g.y, g.z);
  return false;
}
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kern, grid, block, lds, stream, ...)                                   \
  do {                                                                                            \
    if (isle_launch_fits(dim3(grid), dim3(block), __FILE__, __LINE__)) kern<<<dim3(grid), dim3(block), (lds), (stream)>>>(__VA_ARGS__); \
  } while (0)

#include "../../include/isle_hip.h"

#define ISLE_WAVE 64

struct isle_event_pair {
  hipEvent_t a, b;
  int fam;
};

// Device buffer with explicit capacity (grows, never shrinks).
template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;
  hipError_t reserve(size_t n) {
    if (n <= cap) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    hipError_t e = hipMalloc((void**)&p, n * sizeof(T));
    if (e == hipSuccess) cap = n;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }  // every buffer of a context dies with it
};

// Pinned host buffer with explicit capacity (grows, never shrinks): the landing place of the model text (model_text.hip), the staging
// of the centre matrices (isle_ctx::pin_stage).
struct PinBuf {
  char* p = nullptr;
  size_t cap = 0;
  hipError_t reserve(size_t n) {
    if (n <= cap) return hipSuccess;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
    hipError_t e = hipHostMalloc((void**)&p, n, hipHostMallocDefault);
    if (e == hipSuccess) cap = n;
    return e;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
  }
  PinBuf() = default;
  PinBuf(const PinBuf&) = delete;
  PinBuf& operator=(const PinBuf&) = delete;
  ~PinBuf() { release(); }
};

// One side of the LDS-banded Gram apply (gram_lds.hip): a sliced-ELL stream of band-local u16 source ids.
// (GlDesc, one workgroup of gl_apply_k, and the host plan that fills it: gl_plan.h)
struct GlSide {
  uint32_t n_out = 0, n_src = 0, NB = 0, nslice = 0, nwv = 0, ndesc = 0;
  int G = 4;                  // groups of a wave = output items per lane (4 ... 8)
  uint32_t wpg = 16;          // waves per workgroup of the apply kernel on this side
  DevBuf<uint32_t> slice_of;  // nwv x G: slice (64 consecutive output positions) of (wave, group), 0xffffffff = none
  DevBuf<int64_t> roff;       // nwv x NB + 1: first super-round of (wave, band)
  DevBuf<uint16_t> cnt;       // nwv x NB x 8: super-rounds (4 nonzeros per lane) of (wave, band, group), zero beyond G
  DevBuf<uint2> ids;          // super-rounds x 64 lanes: four u16 band-local source ids per lane (+ prefetch slack)
  DevBuf<GlDesc> desc;
  int64_t total_sr = 0;
};

// The small page-locked region (isle_ctx::pin + PIN_SMALL): one member per user, so that no two of them share a word by accident.  The
// single words sit on cache lines of their own; the watchdog's is read by a second thread for the life of the communicator.
struct IslePinSmall {
  double kmpp_stage[(128u << 10) / 8];  // k-means++ rounds: [my 2 | tot 2 * world | local maxdraw] doubles, drawn maxdraw u64, 42 words of the search
  int cluster_sizes[(64u << 10) / 4];   // fetch_sizes (larger k: pageable memory)
  alignas(64) uint32_t stop_flag;       // StopRule: the partitions differ
  alignas(64) uint32_t active_count;    // Lloyd in span(U): documents up for re-examination
  alignas(64) int agree[2];             // agree_i32: (v, -v)
  alignas(64) uint32_t changed_count;   // k_proj_accumulate_delta: documents that changed centre
  alignas(64) uint32_t redo_count;      // dense.hip: rows the two-term pass of an assignment product left open
  alignas(64) volatile uint32_t wd_done;  // the watchdog's word (isle_ctx::wd_done)
  alignas(64) union {
    float movements[(32u << 10) / 4];     // fetch_delta (larger k: a blocking copy)
    float centre_norms[(32u << 10) / 4];  // Lloyd on B, regrouping (k <= 2048); each view is copied out right behind its own synchronisation
  };
};

// An open feed of (doc, word, count) triples (isle_hip_feed_begin ... isle_hip_feed_finalize; ingest.hip): the entries kept so far as
// sort keys (doc << wbits) | word and counts, in the order they were offered, and the staging of one chunk of a batch.
//
// The same store behind a stream of tdf text (isle_hip_tdf_begin ... isle_hip_tdf_finalize; `text` set): the text arrives in pieces cut
// anywhere.  One piece is on the device at a time: t_text[i & 1] holds [carry | piece i], the carry being the bytes behind the last '\n'
// of everything before, which piece i - 1's last kernel left at the front of that buffer.  What the kernels need of the stream's past is
// in t_state on the device; the host learns it one piece late, from the page-locked copy (t_back) that each piece ends with.
constexpr uint64_t ISLE_FEED_CHUNK = 1ull << 26;  // entries per upload + launch: larger batches are cut into these
constexpr uint64_t ISLE_TDF_PIECE = 16ull << 20;  // bytes of text per piece: of 1, 4, 16 and 64 MiB the best wall, level with 4 MiB, at less device time (profiles/tdf_stream_c2.jsonl)
struct IsleTdfState {
  unsigned long long lines;    // '\n' seen since tdf_begin: the 0-based number of the line the carry begins
  unsigned long long entries;  // entries in the store: the held ones (a windowed stream holds those of its documents, a counting stream none)
  unsigned long long carry;    // bytes of the unfinished last line
  unsigned long long err;      // all ones, or (0-based line << 3) | kind of the first bad line (ing_parse_k)
  unsigned long long seen;     // valid lines of the whole text so far; == entries on an ordinary stream
};
struct IsleFeed {
  bool open = false;
  bool text = false;           // the open feed is a text stream: the isle_hip_feed_* calls refuse it, and the other way round
  uint64_t piece = 0;          // text stream: capacity of t_pin[i]
  uint64_t pieces = 0;         // non-empty pieces committed
  bool acquired = false;       // t_pin[pieces & 1] is with the caller
  bool in_flight = false;      // a piece is queued whose state has not been read back
  bool counting = false;       // text stream of isle_hip_tdf_begin_counts: lines per document into t_doc_cnt, no entry store, no line refused
  bool windowed = false;       // text stream of isle_hip_tdf_begin_window: every line checked, the entries of documents [w_begin, w_end) held
  uint64_t w_begin = 0, w_end = 0;
  IsleTdfState known = {0, 0, 0, ~0ull, 0};  // t_state after the last piece that was waited for
  PinBuf t_pin[2], t_back;
  hipEvent_t t_done = nullptr;
  DevBuf<unsigned char> t_text[2];
  DevBuf<IsleTdfState> t_state;
  DevBuf<uint32_t> t_tile_cnt;
  DevBuf<int64_t> t_tile_off;
  DevBuf<uint64_t> t_line_start;
  DevBuf<uint32_t> t_doc_cnt;            // counting stream: valid lines per document, D counters
  DevBuf<unsigned long long> t_seen;     // counting / windowed stream: valid lines of the piece in flight
  uint64_t V = 0, D = 0;
  uint64_t n = 0;        // entries held (zero counts are not)
  uint64_t offered = 0;  // entries offered since feed_begin, skipped ones included: the ordinal an error names
  DevBuf<uint64_t> key;  // the entry store: grows by doubling, contents kept
  DevBuf<uint32_t> cnt;
  DevBuf<uint32_t> in_docs, in_words, in_cnt, t_cnt, t_valid;  // one chunk: as uploaded; keyed, before compaction
  DevBuf<uint64_t> t_key, t_err;
  DevBuf<int64_t> t_at, t_scratch;
  void release();
  ~IsleFeed() { release(); }
};

struct isle_ctx {
  // environment switches as read at the last C-ABI entry (isle_refresh_knobs): the typed values of the switches that select or tune a form
  // (what the rules of route_host.h read), and the strings for the diagnostics and the test hooks
  RouteEnv route;
  std::string knob_val[KN_COUNT];
  bool knob_set[KN_COUNT] = {};
  const char* knob(int id) const { return knob_set[id] ? knob_val[id].c_str() : nullptr; }
  bool knob_on(int id) const { return knob_set[id]; }  // set at all (any value)
  int device = 0;
  size_t total_mem = 0;  // bytes of device memory (isle_total_mem); 0: not asked yet
  hipStream_t stream = nullptr;
  std::string err;
  int num_cus = 256;
  IsleResident res;  // which of the products below still describe the current inputs (resident_host.h: read anywhere, written by its events only)

  // --- page-locked host memory for the small per-iteration copies of the control loops (mailboxes, scalars, flags): a
  // hipMemcpyAsync to or from pageable memory blocks the host until the copy has run, which serialises the enqueue-ahead
  // loops (api.cpp); PIN_* are fixed regions of it
  char* pin = nullptr;
  // growable page-locked staging for the k x k centre matrices that cross the boundary at the ends of the k-means calls (4 MB at
  // k = 1000): hipMemcpyAsync from freshly allocated pageable memory was seen to block for 26 ms there (api.cpp, lloyds_projected)
  PinBuf pin_stage;
  static constexpr size_t PIN_MAIL = 0, PIN_MAIL_SLOT = 1u << 20, PIN_SMALL = 2u << 20, PIN_BYTES = (2u << 20) + (256u << 10);
  IslePinSmall* pin_small() const { return reinterpret_cast<IslePinSmall*>(pin + PIN_SMALL); }

  // --- communicator (null for single GPU)
  ncclComm_t comm = nullptr;
  int world = 1, rank = 0;
  // rehearsal transport (isle_hip_comm_init_host): collectives staged through host memory and a caller-provided exchange
  // function, so that several ranks can share one GPU in tests (RCCL refuses two ranks on one device)
  isle_host_exchange_fn host_xchg = nullptr;
  void* host_xchg_user = nullptr;
  bool multi() const { return comm != nullptr || host_xchg != nullptr; }
  // watchdog of the RCCL collectives (api.cpp, wd_*): behind every collective the device writes its sequence number into a page-locked
  // word; a thread started with the communicator compares it with the number issued and, when collectives are pending and none has
  // completed for ISLE_COMM_TIMEOUT_S seconds, aborts the communicator — the stream drains, every HIPCHK from then on returns ISLE_E_COMM
  // and the caller gets an error instead of a hang (a rank that died, or a rank whose replicated state diverged and left the sequence)
  std::atomic<uint32_t> wd_issued{0};
  volatile uint32_t* wd_done = nullptr;  // page-locked, device-visible
  std::atomic<int> comm_dead{0};
  std::atomic<bool> wd_stop{false};
  std::thread wd_thread;
  double wd_timeout_s = 300.0;

  // --- B (this rank's column shard), CSC
  uint64_t V = 0, D = 0, nnz = 0, doc_offset = 0, D_global = 0;
  DevBuf<float> vals;
  DevBuf<uint32_t> rows;
  DevBuf<int64_t> offs;

  // --- A (word-document counts, this rank's column shard) and the thresholding workspaces (threshold.hip)
  uint64_t a_V = 0, a_D = 0, a_nnz = 0, a_doc_offset = 0, a_D_global = 0;
  IsleFeed feed;
  DevBuf<float> a_cnt;
  DevBuf<uint32_t> a_rows;
  DevBuf<int64_t> a_offs;
  DevBuf<uint16_t> a_q;        // rounded normalised counts, clamped to maxv
  DevBuf<uint32_t> a_hist;     // V x (maxv + 1)
  DevBuf<uint32_t> a_kept, a_flag;
  DevBuf<float> a_wgt;
  DevBuf<int64_t> a_off_all, a_col_of, a_scan;
  DevBuf<float> zetas;             // V
  DevBuf<uint64_t> original_cols;  // D (B column -> global document id of A)
  float a_avg = 0.f;               // avg_doc_sz of the whole corpus (src/sparseMatrix.cpp:98)
  int vocab_hist_form = 0;         // isle_hip_vocab_hist_form: what route_vocab_hist is asked with (0: the rule's own choice)
  int doc_hash_form = 0;           // isle_hip_doc_hash_form: what route_doc_hash is asked with (0: the rule's own choice)
  int neardup_key_form = 0;        // isle_hip_neardup_key_form: what route_neardup_key is asked with (0: the rule's own choice)
  int model_dist_slices = 0;       // isle_hip_model_dist_slices: what route_model_dist_slices is asked with (0: the rule's own choice)
  int simdocs_table_form = 0;      // isle_hip_simdocs_table_form: what route_simdocs_table is asked with (0: the rule's own choice)
  int prevalence_tile_form = 0;    // isle_hip_prevalence_tile_form: what prev_tile (prevalence_host.h) is asked with (0: the rule's own choice)

  // --- downstream stage (post.hip): catchwords, topic model, edge topics
  DevBuf<float> a_nv;              // normalised values of A
  DevBuf<int32_t> p_cluster_of;    // a_D
  DevBuf<uint32_t> p_cnt, p_min, p_slot;   // V x k, word-major
  DevBuf<float> p_thr;             // V x k, word-major catchword thresholds
  DevBuf<uint64_t> p_seg_id, p_seg_off, p_counters;
  DevBuf<uint32_t> p_seg_len, p_seg_rank, p_seg_cur;
  DevBuf<float> p_segvals;
  // several ranks (route_post_select): p_cnt / p_tcnt hold this rank's counts, these the counts summed over the ranks; the slots are
  // numbered by a scan of the qualifying pairs in pair order; per slot the prefix found and the rank left; the bins of one chunk of slots
  DevBuf<uint32_t> p_cnt_g, p_tcnt_g;  // V x k word-major; k counts, then k flags
  DevBuf<int64_t> p_slot_scan;         // V x k + 1
  DevBuf<uint32_t> p_sel_prefix, p_sel_rem, p_sel_bins;
  DevBuf<int32_t> p_catch;        // V: topic the word is a catchword of, or -1
  DevBuf<uint32_t> p_nz;
  DevBuf<int64_t> p_dts_off;       // a_D + 1
  DevBuf<uint32_t> p_dts_topic;
  DevBuf<float> p_dts_val;
  uint64_t p_dts_n = 0;
  DevBuf<int32_t> p_top1, p_top2;  // a_D
  DevBuf<uint32_t> p_tcnt;
  DevBuf<int64_t> p_toff;
  DevBuf<float> p_mthr;            // k
  DevBuf<float> p_model;           // V x k col-major
  DevBuf<uint64_t> p_avg_acc;      // V x k (lo, hi) pairs: exact fixed-point sums of the average model (avg_model.hip)
  DevBuf<float> p_avg_model;       // V x k col-major, the cluster-average model
  DevBuf<uint32_t> mt_sizes;       // the text formatters (model_text.hip, text_tiles.h): bytes per tile
  DevBuf<uint64_t> mt_offs, mt_blk, mt_stat;  // their exclusive scan (+ its scratch); entries emitted, first entry outside the domain
  DevBuf<unsigned char> mt_text[2];  // one chunk of text each (<= ISLE_TEXT_CHUNK_BYTES), formatted while the other one is copied and consumed
  PinBuf mt_pin[2];
  // document-topic weights of the last isle_hip_infer_resident (infer_resident.hip), CSR over its document range; void when A changes
  DevBuf<int64_t> inf_off;         // docs + 1
  DevBuf<uint32_t> inf_topic;
  DevBuf<float> inf_weight;
  DevBuf<int32_t> inf_top_topic;   // docs x 5, < 0 = no further topic: what isle_hip_infer_text(ISLE_DOCTEXT_TOP) prints
  DevBuf<float> inf_top_weight;
  uint64_t inf_docs = 0, inf_n = 0, inf_doc_begin = 0;  // inf_doc_begin: that call's first document of A
  int inf_cols = 0;               // the columns of that call's model: the topics of inf_topic
  // the model of the last successful isle_hip_load_model_text (model_load.hip): independent of A, B, the partition and the catchwords
  DevBuf<float> ml_model;          // ml_V x ml_cols col-major
  uint64_t ml_V = 0;
  int ml_cols = 0;

  // --- chunked-CSR copy of B for Z = B*Y (built per eigensolve, like the reference's operator ctor)
  uint32_t band_rows = 0;  // requested columns per chunk (0 = default), env ISLE_CHUNK_COLS
  uint32_t nbands = 0;     // number of column chunks (multiple of 8)
  uint32_t chunk_cols = 0;
  DevBuf<uint32_t> bcol;   // nnz   doc id
  DevBuf<float> bval;      // nnz
  DevBuf<int64_t> seg_off; // nchunks*V + 1
  DevBuf<float> Zpart;     // nchunks x V x BP partial rows

  // --- LDS-banded Gram apply (gram_lds.hip): used when every row of B holds a single value (B = diag(s) * pattern, which is
  // what threshold_and_copy produces, src/sparseMatrix.cpp:1285-1321); otherwise the gather kernels of spmm.hip run.
  GlSide gl1, gl2;           // pass 1 (outputs = documents, sources = words), pass 2 (outputs = words, sources = documents)
  DevBuf<float> rowval;      // V: the value of row w
  DevBuf<int> gl_flag;
  DevBuf<uint32_t> dperm, dpos, wperm, wpos;  // position -> document, document -> position, position -> word, word -> position
  DevBuf<uint64_t> gl_key_a, gl_key_b;
  DevBuf<uint32_t> gl_val_a, gl_val_b;
  DevBuf<uint32_t> gl_bst;   // D x (NB1 + 1): first entry of each word band inside a document's column
  DevBuf<uint16_t> gl_cellcnt;   // V x NB2: entries of (word, document band)
  DevBuf<uint32_t> gl_srsum, gl_sbase;
  DevBuf<uint32_t> gl_fb_cnt, gl_fb_tmp;  // pass-2 fill by buckets of word positions: entries per (band, bucket); the packed entries (nnz words = 4 GB at config 3).
                                          // KEPT between builds, like gl_pscratch below (7.7 GB at 10 M documents): every solve builds the operator again and a
                                          // hipFree / hipMalloc pair of that size per step costs more than the memory is worth on a 288 GB device; both count
                                          // against what route_scratch_ok sees as free — it decides from the device's TOTAL memory, so the routes do not depend on them
  DevBuf<int64_t> gl_fb_off;
  DevBuf<uint16_t> gl_scnt;  // super-rounds of (slice, band) of pass 2 (gl_sbase's indexing)
  DevBuf<uint32_t> gl_biglist;   // [count | (wave, band, group) triples whose pass-2 cells are too long for the register sort]
  DevBuf<uint32_t> ccount;       // k x V, centre-major: members of centre c that contain word w (sparse Lloyd centroid update)
  DevBuf<uint32_t> ccounted;     // D: the centre under which document d is counted in ccount
  DevBuf<int64_t> gl_scan;
  DevBuf<unsigned long long> gl_blocktot;
  DevBuf<uint32_t> gl_slab0, gl_nch;  // per word block: first partial slab, number of slabs
  uint32_t gl_block_items = 4096;     // words per word block of pass 2 (256 per wave of the block)
  DevBuf<float> gl_Xs, gl_part;       // scaled panel diag(s) X; partial rows of Z per (word block, band chunk)
  DevBuf<float> gl_pscratch;          // k-wide product, grouped form: up to 16 panels' rows, whole and in position order (D x 12 floats each), and the
                                      // rows' squared-norm partials per group of panels (k_gl_wide)
  DevBuf<uint32_t> rs_hist;           // radix sort scratch (ingest.hip: k_sort_pairs_u64)
  DevBuf<int64_t> rs_hist_off, rs_scratch;

  // --- gram-apply workspaces
  DevBuf<float> Xrm, Yrm, Zrm;   // V*BP, D*BP, V*BP
  DevBuf<float> Xcm, Zcm;        // staging for the host-pointer API

  // --- eigensolver state
  DevBuf<float> basis;     // V x (ncv + blk) col-major
  DevBuf<float> Fbuf;      // V x blk
  DevBuf<float> Tmp;       // V x nev (rotation target)
  DevBuf<double> part;     // partial reductions
  DevBuf<float> coef;      // 3 x (m x blk)
  DevBuf<double> gram;     // blk x blk
  DevBuf<double> pq_part, pq_R1;  // panel QR: partial Gram matrices, first triangular factor
  DevBuf<float> pq_T;             // panel QR: T (32 x 32) and R (32 x 32)
  DevBuf<int> pq_meta;            // panel QR: rank, status, pivots
  DevBuf<float> small;     // misc small device scratch
  DevBuf<double> jacW, jacV;  // n x n each
  DevBuf<double> jacS;        // per-pair Gram / rotation scratch
  DevBuf<float> Wf;        // n x n float eigenvectors
  DevBuf<float> evd_in;    // n x n: the fp32 matrix handed to the small EVD
  DevBuf<float> Ucm;       // V x k col-major  (copy of basis[:, :k])
  DevBuf<float> Urm;       // V x ldk row-major
  int ldk = 0;

  // --- k-means state
  DevBuf<float> P;         // D x ldk
  DevBuf<float> pnorm;     // D
  DevBuf<float> Pt;        // ldk x D coordinate-major copy (projected assignment), only for ldk <= 256
  DevBuf<float> dotsT;     // D x k centre-major dot products (first assignment of Lloyd on B through the projection)
  DevBuf<uint4> gemm_b3;   // the small operand of k_gemm_nn_assign split into three bf16 terms (gemm_bf16x3.h)
  DevBuf<float> yy_gmax2;     // G floats: the groups' largest movements without the movers
  DevBuf<float> yy_mdots;     // D x 12: dot products of every document with the movers' centres (YyMovers)
  DevBuf<float> cmax_buf;     // one float: the largest centre norm of a full projected pass
  DevBuf<uint32_t> ga_redo;   // rows the two-term pass of an assignment product left open (last = count), dense.hip gemm_assign_two_pass
  DevBuf<float> ga_bn;             // squared norms of the product's columns and their maximum
  DevBuf<float> ga_rows, ga_rown;  // those rows gathered coordinate-major, their squared norms
  bool ts_open = false;       // a TimeScope is open (nested scopes are not timed again)
  bool roctx_open = false;    // ... and a roctx range (ISLE_ROCTX; nested scopes push no second one)
  uint32_t ga_last_redo = 0;  // their number in the last product (diagnostic: isle_hip_measure)
  DevBuf<float> assign_part;  // per document and 64-column slot the best centre of the slot (16 bytes: k_gemm_assign_yy / _tiles, dense.hip)
  DevBuf<float> lift_C;    // the k x k coefficients the device-resident centres were lifted from (centres = U lift_C^T)
  DevBuf<uint4> Pt2;       // the coordinate-major copy split in two bf16 terms, as the LDS image of every (row block, slab): the A operand of the
                           // LDS-DMA assignment products (gemm_bf16x3.h, gemm_bf16x2_dma_k); by document or by position: res.Pt2
  DevBuf<float> min_dist;  // D
  DevBuf<double> cum;      // D + 1
  DevBuf<double> scan_blk;
  DevBuf<float> Cdev;      // k x ldk centres (projected)
  DevBuf<float> cnorm;     // k
  DevBuf<float> Csum;      // k x ldk + k
  DevBuf<uint32_t> assign, assign_prev;
  DevBuf<int> counts;
  DevBuf<uint32_t> members;  // documents grouped by centre
  DevBuf<int> moff;          // k+1 offsets, k cursors
  DevBuf<int> flags;
  DevBuf<float> centers_rm;   // V x ldk  (word-space centres, row-major)
  DevBuf<float> centers_cm;   // V x k col-major staging
  DevBuf<float> dnorm;     // D   |b_d|^2
  DevBuf<float> hub, hlb;  // D   Hamerly bounds (sparse Lloyd)
  DevBuf<float> yglb;      // D x G Yinyang group bounds (sparse Lloyd)
  DevBuf<float> ptlb;      // D x TL tile bounds (projected Lloyd at k > 224)
  DevBuf<uint32_t> pneed;  // D: tiles a document has to re-examine
  DevBuf<uint32_t> pcand;  // D + 1: candidates of the first filter stage (last = count)
  DevBuf<int> seg_desc;    // projected centroid sums: chunk descriptors (beg, end) and the centres' first chunks
  DevBuf<float> seg_part;  // one partial row per chunk
  DevBuf<uint32_t> proj_counted;  // D: the centre under which a document is counted in the projected sums (k_proj_accumulate_delta)
  DevBuf<uint32_t> proj_nch;      // number of documents that changed centre
  DevBuf<float> proj_dpart;       // k x 8 x ldk partial sums of the changes
  DevBuf<float> Csum_local;       // several ranks: this rank's sums (Csum holds the all-reduced ones)
  DevBuf<uint32_t> active; // D + 1 (last = count)
  DevBuf<unsigned long long> dbg_cnt;  // diagnostics (ISLE_DEBUG_HAMERLY)
  // what the k-means++ rounds keep for Lloyd's first assignment in span(U) (kmeans.hip kmpp_min_dots_track_k)
  DevBuf<uint32_t> kmpp_arg;   // nearest seed so far
  DevBuf<float> kmpp_m2a;      // smallest distance to the other seeds of its tile
  DevBuf<float> kmpp_tmin;     // smallest distance per tile of 32 seeds, tile-major [tile][document]
  DevBuf<float> kmpp_best;     // distances to the nearest of ALL k seeds (min_dist does not include the last batch)
  bool kmpp_track = false;     // every round so far went through the tracking kernel
  int kmpp_track_seeds = 0;    // seeds folded in
  std::vector<float> kmpp_C_host;  // the seeds' coordinates as handed to the caller (k x k)
  // Yinyang iteration ordered by group (spmm.hip, k_yy2_assign)
  DevBuf<float> yy_cg;                 // centres group-major: G tables of V x 8 floats
  DevBuf<uint32_t> yy_map;             // regrouped Yinyang groups: id_of_slot (8 G) then slot_of_id (k)
  DevBuf<float> yy_cns;                // squared centre norms by slot (8 G)
  DevBuf<float> yy_liftC;              // the lift coefficients' rows by slot (first assignment through the projection)
  DevBuf<uint32_t> yy_own, yy_res;     // YyRes (3 words) per active slot / per pair
  DevBuf<unsigned long long> yy_need;  // per active slot: bit mask of the groups to scan
  DevBuf<uint32_t> yy_cnt, yy_off;     // pairs per active slot, their exclusive scan
  DevBuf<uint8_t> yy_pgrp;             // group of every pair (slot-major order)
  DevBuf<float> centers_old;  // V x ldk
  DevBuf<float> Pa, pna, Cold; // compacted active rows (ldk x n), their norms, previous projected centres
  // the k-means objective (objective.hip, isle_hip_kmeans_objective): scratch of its own, so that a call leaves every resident buffer as it was
  DevBuf<double> ob_dd, ob_cn, ob_sums;  // D distances, k centre norms, k cluster sums
  DevBuf<unsigned long long> ob_acc;     // k (lo, hi) pairs, k sizes, the largest distance's high word
  DevBuf<uint32_t> ob_assign;            // an explicit partition
  DevBuf<float> ob_centres, ob_cm;       // explicit centres as the kernels read them; their column-major upload
  DevBuf<int> ob_cnt;                    // k local sizes for the member lists
  bool lloyd_trace = false;               // isle_hip_lloyds_trace
  std::vector<double> lloyd_trace_v[2];   // the total objective after every centre update of the last loop, per space

  // block Krylov-Schur, pipelined expand loop: device mailbox [rank, status, pivots | R | coefficients] of a step, fetched by
  // one copy; the events that mark its arrival
  hipEvent_t ks_ev[2] = {nullptr, nullptr};
  hipEvent_t ks_ev_ready[2] = {nullptr, nullptr};  // the step's mailbox is complete on the main stream (the copy stream waits for it)
  hipStream_t copy_stream = nullptr;               // the mailbox's way to the host: beside the main stream, not in it (api_ks.cpp expand)
  DevBuf<float> ks_mail;
  DevBuf<float> ks_top;     // truncation: the locked rows of H next to the rotated block, and their product with the Ritz rotation
  DevBuf<float> ks_gather;  // row-sharded orthogonalisation: the ranks' slices of F (world x nloc x blk)

  // largest dynamic-LDS size requested so far per kernel ON THIS CONTEXT'S DEVICE (hipFuncSetAttribute is per device; a
  // process-wide flag would leave the kernels of a second GPU at the 64 KB default)
  std::vector<std::pair<const void*, int>> lds_attr;
  bool td_persist_failed = false;  // the persistent tridiagonalisation hit its barrier time-out once (GPU shared): launch chain from now on
  // what the most recent small EVD of this context did (isle_hip_eig_info): host words written where the host decides anyway
  int eig_info[ISLE_EIG_INFO_COUNT] = {0};
  float eig_defect = 0.f;  // the orthogonality defect td_check_k measured (0 where the tridiagonal solver did not get that far)

  // --- timing
  bool timing = false;
  uint32_t timing_mask = 0xffffffffu;  // families whose launches are bracketed by events while timing is on
  std::vector<isle_event_pair> ev_used;
  std::vector<isle_event_pair> ev_free;
  double t_ms[ISLE_T_COUNT] = {0};
  uint64_t t_n[ISLE_T_COUNT] = {0};
};

static_assert(sizeof(IslePinSmall) <= isle_ctx::PIN_BYTES - isle_ctx::PIN_SMALL, "the small page-locked region holds every slot");

int isle_fail(isle_ctx* c, int code, const char* fmt, ...);
// A new matrix of D documents and nnz entries replaces the context's: the largest derived buffers (projection and its copies, product scratch,
// build scratch) are released where they are sized for a far larger matrix — everything derived from the old one is void anyway (api.cpp)
void isle_trim_derived(isle_ctx* c, uint64_t D, uint64_t nnz);
// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (context = device, kernel, size): api.cpp
int isle_max_lds(isle_ctx* c, const void* fn, int bytes);
bool isle_total_mem(isle_ctx* c);  // asks the device for its total memory, once (c->total_mem); false: it could not be asked
// A rule of route_host.h that may need the device's total memory, rule(total_mem, &ask): asked for only where the decision gets that far
template <class Rule>
auto isle_route_mem(isle_ctx* c, Rule rule) -> decltype(rule((uint64_t)0, (bool*)nullptr)) {
  bool ask = false;
  auto r = rule((uint64_t)c->total_mem, &ask);
  if (ask && isle_total_mem(c)) r = rule((uint64_t)c->total_mem, &ask);
  return r;
}
void isle_refresh_knobs(isle_ctx* c);
int isle_enter(isle_ctx* c);  // entry of a C-ABI call: the context's device becomes current, the environment switches are read
// ISLE_HOST_TRACE=1: host wall time since the previous mark, to stderr (marks that follow within 0.2 ms stay silent).  Finds GPU-idle
// stretches that are host work, which no kernel profile shows.
void isle_host_mark(const char* what);

#define HIPCHK(ctx, call)                                                                   \
  do {                                                                                      \
    hipError_t e__ = (call);                                                                \
    if ((ctx) && (ctx)->comm_dead.load(std::memory_order_relaxed))                          \
      return isle_fail((ctx), ISLE_E_COMM, "%s:%d: a collective did not complete within %.0f s (ISLE_COMM_TIMEOUT_S): the communicator was aborted", __FILE__, __LINE__, (ctx)->wd_timeout_s); \
    if (e__ != hipSuccess)                                                                  \
      return isle_fail((ctx), ISLE_E_HIP, "%s:%d %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(e__)); \
    if (isle_launch_refused().file) {                                                       \
      const IsleLaunchRefused r__ = isle_launch_refused();                                  \
      isle_launch_refused() = IsleLaunchRefused();                                          \
      return isle_fail((ctx), ISLE_E_ARG, "%s:%d: kernel launch of %llu threads refused (2^32 or more do not run)", r__.file, r__.line, r__.threads); \
    }                                                                                       \
  } while (0)

#define ISLECHK(call)            \
  do {                           \
    int rc__ = (call);           \
    if (rc__ != 0) return rc__;  \
  } while (0)

// One device word on the host: through its page-locked slot (IslePinSmall), behind a synchronisation of the stream.
inline int isle_fetch_u32(isle_ctx* c, const uint32_t* dev, uint32_t* slot, uint32_t* out) {
  HIPCHK(c, hipMemcpyAsync(slot, dev, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *out = *slot;
  return 0;
}

// RAII timing scope: records an event pair on the stream when timing is enabled.
struct TimeScope {
  isle_ctx* c;
  isle_event_pair ep;
  bool on;
  bool marker = false;  // a roctx range is open for this scope (ISLE_ROCTX)
  TimeScope(isle_ctx* c_, int fam);
  ~TimeScope();
};

static inline uint64_t isle_scan_scratch(uint64_t n) { return (n + 4095) / 4096 + 1; }  // = isle_scan::scan_scratch_elems
static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// ---------------- kernel launchers (each defined in one .hip file) -------------------------
// api.cpp: collectives on c->stream: RCCL, or the host-staged rehearsal transport; no-ops without a communicator
enum { ISLE_DT_F32 = 0, ISLE_DT_F64 = 1, ISLE_DT_I32 = 2, ISLE_DT_U32 = 3, ISLE_DT_U64 = 4 };
int isle_allreduce(isle_ctx* c, void* buf, size_t count, int dtype, bool max_op = false);  // in place
int isle_allgather(isle_ctx* c, const void* send, void* recv, size_t count_per_rank, int dtype);  // recv: world * count_per_rank
// spmm.hip
int k_pack_rm(isle_ctx* c, const float* Xcm, uint64_t V, int b, int BP, float* Xrm);
int k_unpack_cm(isle_ctx* c, const float* Zrm, uint64_t V, int b, int BP, float* Zcm);
int k_gram_pass1(isle_ctx* c, int BP);   // Yrm = B^T Xrm
int k_gram_pass2(isle_ctx* c, int BP);   // Zrm = B Yrm
int k_band_build(isle_ctx* c);
int k_band_build_chunked(isle_ctx* c);   // chunk-major cells for the gather path (spmm.hip)
int k_dots_assign(isle_ctx* c, int k, int ldk, const float* cn, const float* dn, uint32_t* assign, float* ub, float* lb, int G);
int k_dots_assign_cm(isle_ctx* c, const float* dotsT, int k, int G, const float* cn, const float* dn, const float* cn_max_dev, uint32_t* assign, float* ub,
                     float* lb);  // the same from column-major dot products, Yinyang bounds
int k_frobenius(isle_ctx* c, double* out_host);
int k_spmm_wide_project(isle_ctx* c, const float* Mrm, int k, int ldk, float* P, float* norms, void* A2pos = nullptr, bool* a2_done = nullptr);
int k_spmm_wide_assign(isle_ctx* c, const float* Mrm, int k, int ldk, const float* cn, const float* dn, uint32_t* assign,
                       const uint32_t* perm /*nullable: slot -> doc*/, const uint32_t* nslots = nullptr /*device slot count*/,
                       float* ub = nullptr, float* lb = nullptr, int G = 0 /*> 0: lb holds G Yinyang group bounds per document*/);
// The centres of a Yinyang iteration that moved far (at most ten: one thin pass): they are left out of their groups' movements and bounded by
// their exact new distances instead (yy2_filter_tighten_k)
struct YyMovers {
  int n = 0, ld = 0;   // ld = 4 ceil(n / 4): row stride of the D x n dot products
  uint32_t id[10] = {};
};
// Which centres share a Yinyang group.  Null pointers: group g = centres 8 g .. 8 g + 7 (the identity).  Otherwise the groups are made
// of SLOTS: slot s = 8 g + t holds centre id_of_slot[s] (s < k; the slots behind are padding), slot_of_id is the inverse.  The kernels
// of the by-group iteration index tables and bounds by slot and report centres by id; ties between equal distances go to the smaller ID
// whatever the slots' order, as the reference's isamin does (src/sparseMatrix.cpp:1553-1572).  ONE exception, stated in INTEGRATION.md: the
// FIRST assignment (the product through the projection, columns in slot order: tile_epilogue / yy_first_combine_k) keeps the earlier COLUMN
// on a bit-exact tie, i.e. the smaller slot = the smaller squared norm; identical centres keep their id order (the slot order is a stable
// sort by norm), so only two DIFFERENT centres at bit-equal distances from a document can fall the other way, in that one iteration.
struct YyMap {
  const uint32_t* id_of_slot = nullptr;
  const uint32_t* slot_of_id = nullptr;
#if defined(__HIPCC__)
  __device__ inline uint32_t id(uint32_t s) const { return id_of_slot ? id_of_slot[s] : s; }
  __device__ inline uint32_t slot(uint32_t i) const { return slot_of_id ? slot_of_id[i] : i; }
#endif
};
int k_yy_filter_tighten(isle_ctx* c, const uint32_t* order, const uint32_t* assign, float* ub, float* glb, int G, const float* delta_dev,
                        const float* gmax_dev, uint32_t* active, uint32_t* nactive, const float* Cg, int k, int ld, const float* cn, const float* dn,
                        const float* cn_max, const YyMovers& mv, const float* Crm, const YyMap& map = YyMap(), const float* cn_by_id = nullptr);
// the maps of a regrouping (host arrays of 8 G and k entries) on the device; cn_slot[s] = cn[id_of_slot[s]]; rows of a small matrix by slot;
// labels written by slot turned into ids
int k_yy_map_upload(isle_ctx* c, const uint32_t* id_of_slot_host, const uint32_t* slot_of_id_host, int k, int G, YyMap* map);
int k_yy_gather_by_slot(isle_ctx* c, const YyMap& map, int k, int G, const float* cn, float* cn_slot);
int k_yy_rows_by_slot(isle_ctx* c, const YyMap& map, int k, const float* in, int ld, float* out);
int k_yy_labels_to_ids(isle_ctx* c, const YyMap& map, uint32_t* assign, uint64_t D);
int k_yy_filter(isle_ctx* c, const uint32_t* order, const uint32_t* assign, float* ub, float* glb, int G, const float* delta_dev, const float* gmax_dev,
                uint32_t* active, uint32_t* nactive);
int k_yy_dbg_margins(isle_ctx* c, const uint32_t* active, const uint32_t* nactive, const uint32_t* assign, const float* ub, const float* glb, int G,
                     const YyMap& map, unsigned long long* hist_host);
int k_yy_pack_groups(isle_ctx* c, const float* Crm, int ld, int G, const YyMap& map = YyMap());  // c->yy_cg = the centres group-major (V x 8 floats per group)
int k_yy_scan(isle_ctx* c, const float* Crm, const float* Cg /*nullable*/, int k, int ld, int G, const float* cn, const float* dn, const float* cn_max_dev,
              const uint32_t* active, const uint32_t* nactive, uint32_t* assign, float* ub, float* glb, unsigned long long* dbg = nullptr,
              const YyMap& map = YyMap());
int k_yy2_assign(isle_ctx* c, const float* Cg, int k, int ld, int G, const float* cn, const float* dn, const float* cn_max_dev, const uint32_t* active,
                 const uint32_t* nactive, uint32_t* assign, float* ub, float* glb, bool* done, unsigned long long* pairs_out = nullptr, bool pre_tightened = false,
                 const YyMap& map = YyMap());
struct HamTop {  // largest and second largest centre movement of an iteration (Hamerly's bound update), device resident
  uint32_t amax;
  float d1, d2, pad;
};
int k_ham_delta(isle_ctx* c, float* delta_dev /*in: squared movements, out: rounded-up movements*/, int k, HamTop* top_dev);
int k_hamerly_filter(isle_ctx* c, const uint32_t* order, const uint32_t* assign, float* ub, float* lb, const float* delta_dev, const HamTop* top_dev,
                     uint32_t* active, uint32_t* nactive, int fam = ISLE_T_SPARSE_ASSIGN);
int k_csc_validate(isle_ctx* c, unsigned long long* err_host2);  // the uploaded CSC arrays on the device: [0] first bad column + 1 (0 = fine), [1] what (spmm.hip)
int k_doc_norms(isle_ctx* c, float* dn);
int k_centers_from_rows(isle_ctx* c, const uint32_t* assign, int k, int ldk, float* Crm, bool first_of_run = true);
int k_pt_filter(isle_ctx* c, const uint32_t* order, const uint32_t* assign, float* ub, float* tlb, int T, int TL, const float* delta_dev,
                const float* tmove_dev, uint32_t* need, uint32_t* active, uint32_t* nactive, const YyMovers& mv, const float* mdots, const float* cn, const float* pn);
int k_pt_tighten(isle_ctx* c, const float* P, const float* pn, int ldk, const float* C, const float* cn, const uint32_t* assign, const uint32_t* cand,
                 const uint32_t* ncand, float* ub, const float* tlb, int T, int TL, uint32_t* need, uint32_t* active, uint32_t* nactive);
// gram_lds.hip
int k_gl_detect(isle_ctx* c);            // sets c->res.gl_mode for the current B (no-op once decided)
int k_centers_counts(isle_ctx* c, const uint32_t* assign, int k, int ldk, float* Crm, bool fresh);  // fresh: needs c->members grouped by `assign`
int k_gl_build(isle_ctx* c);
int k_gl_wide(isle_ctx* c, const float* Mrm, int k, int ld, float* Out, float* norms = nullptr /*also the rows' squared norms (selects the grouped form)*/,
              void* A2pos = nullptr /*grouped form only: also the split copy of Out by POSITION (k_gemm_split_a_bytes(D, k) bytes)*/, bool* a2_done = nullptr);
int k_gl_thin(isle_ctx* c, const float* Wcm, int nc, int ld, float* Out, bool by_position = false);  // Out (D x ld) = B^T W, W V x nc col-major, nc <= 32  // Out (D x ld) = B^T M, LDS-banded form only
int k_gl_apply_cm(isle_ctx* c, const float* Xcm, int b, int BP, float* Zcm);  // Zcm (V x b col-major) = B (B^T Xcm), b columns in a panel of BP in {4, 8, 12}
int k_gl_panel_width(const isle_ctx* c);  // columns per pass of the k-wide / thin products through the pass-1 stream (gram_lds.hip)

// threshold.hip
int k_th_stats(isle_ctx* c, uint64_t* tokens_nz_dev);
int k_th_round_hist(isle_ctx* c, float avg, uint32_t maxv);
int k_th_zetas(isle_ctx* c, uint32_t maxv, uint64_t count_gr, uint64_t count_eq);
int k_th_count(isle_ctx* c, bool with_weights);
int k_th_drop(isle_ctx* c, const uint8_t* drop_dev);
int k_th_scans(isle_ctx* c);
int k_th_emit(isle_ctx* c, uint64_t doc_base);

// ingest.hip
int k_sort_pairs_u64(isle_ctx* c, uint64_t* key_a, uint32_t* val_a, uint64_t* key_b, uint32_t* val_b, uint64_t n, int key_bits, bool* in_a);
int k_ingest_tdf(isle_ctx* c, const unsigned char* text_dev, uint64_t n, uint64_t V, uint64_t D, uint64_t* entries_read, uint64_t* err_out);
int k_feed_chunk(isle_ctx* c, const uint32_t* docs, const uint32_t* words, const uint32_t* counts, uint64_t n, uint64_t* bad);
int k_feed_finalize(isle_ctx* c);
int k_tdf_open(isle_ctx* c);                                                      // the device state and the event of a text stream
int k_tdf_piece(isle_ctx* c, const char* bytes, uint64_t n, bool last_line);      // queues [carry | n bytes from page-locked memory]; last_line: the carry alone
int k_tdf_open_counts(isle_ctx* c);                                               // the zeroed table of a counting stream
int k_tdf_plan(isle_ctx* c, uint64_t lines_global, int parts, uint64_t* bounds);  // the counting stream's table (summed over the ranks) -> parts + 1 bounds
int k_tdf_wait(isle_ctx* c);                                                      // -> IsleFeed::known is the state after everything queued
void k_tdf_release_text(isle_ctx* c);

// infer.hip
int k_infer(isle_ctx* c, uint64_t V, int k, const float* model_by_word, uint64_t D, uint64_t nnz, const float* counts, const uint32_t* rows,
            const int64_t* offs, int iters, float Lfguess, float avg_doc_sz, float* weights, int32_t* top_topic, float* top_weight, float* llh,
            uint64_t* nconverged);
// its steps on device pointers: the rows of a packed model (V x round4(k) row-major, zero padding) that take part; D documents given by
// offs[0 .. D] (positions in counts / rows / fw / fa) prepared and iterated, outputs indexed from 0, *nconverged added to
int k_infer_rowok(isle_ctx* c, const float* M, uint64_t V, int k, unsigned char* ok);
int k_infer_docs(isle_ctx* c, const float* M, int k, uint64_t D, const float* counts, const uint32_t* rows, const int64_t* offs,
                 const unsigned char* ok, uint32_t* fw, float* fa, uint32_t* nkeep, int iters, float Lfguess, float avg_doc_sz, float* weights,
                 int32_t* top_topic, float* top_weight, float* llh, unsigned int* nconverged);

// infer_resident.hip: documents [doc_begin, doc_end) of the resident A under a V x k column-major device model, in chunks of chunk_docs
// (0 = ISLE_INFER_CHUNK_BYTES of dense weights); the entries above min_weight into c->inf_off / inf_topic / inf_weight
int k_infer_resident(isle_ctx* c, const float* model_cm_dev, int k, uint64_t doc_begin, uint64_t doc_end, int iters, float Lfguess,
                     float avg_doc_sz, float min_weight, uint64_t chunk_docs, int32_t* top_topic, float* top_weight, float* llh,
                     uint64_t* nconverged, uint64_t* nentries);

// post.hip
int k_post_normalize(isle_ctx* c, float avg);
int k_post_cluster_of(isle_ctx* c, const uint32_t* assign_dev, bool identity);
int k_post_catch_thresholds(isle_ctx* c, uint32_t k, uint32_t r, const int* sizes_dev);
int k_post_find_catchwords(isle_ctx* c, uint32_t k, double rho, uint64_t* ncatch_host);
int k_post_thr_colmajor(isle_ctx* c, uint32_t k, float* out_dev);
int k_post_doc_topic_sums(isle_ctx* c, uint32_t k, uint64_t* n_out);
int k_post_model_thresholds(isle_ctx* c, uint32_t k, uint32_t rank);
int k_post_model_accumulate(isle_ctx* c, uint32_t k);  // this rank's documents into a zeroed V x k
int k_post_model_normalize(isle_ctx* c, uint32_t k);
// ... the steps of the thresholds with several ranks (route_post_select == POST_SELECT_HISTOGRAM), between the collectives of api_stages.cpp
int k_post_pair_counts(isle_ctx* c, uint32_t k);       // p_cnt, p_min of this rank's documents; p_cnt_g = p_cnt, p_min as complements (post_min_flip_k)
int k_post_min_restore(isle_ctx* c, uint32_t* p, uint64_t n);  // the all-reduced complements back to value bits
int k_post_topic_counts(isle_ctx* c, uint32_t k);      // p_tcnt, p_toff, the sums gathered per topic; p_tcnt_g = p_tcnt; p_mthr = 0
// ids with cnt_g > above get a slot, numbered in id order: seg_id, seg_len = cnt_l, seg_off (off_l, or the scan of the lengths), prefix 0,
// rank left `rank`; flag: n words of scratch; slot_of: n words or null
int k_post_number_slots(isle_ctx* c, const uint32_t* cnt_g, const uint32_t* cnt_l, uint64_t n, uint32_t above, uint32_t rank, const int64_t* off_l,
                        uint32_t* flag, uint32_t* slot_of, uint64_t* nslots);
int k_post_scatter_segments(isle_ctx* c, uint32_t k, uint64_t nslots);
int k_post_select_hist(isle_ctx* c, uint64_t first, uint64_t count, int shift);              // -> p_sel_bins, count x 256
int k_post_select_step(isle_ctx* c, uint64_t first, uint64_t count, int shift, float* out);  // shift == 0: out[seg_id] = the value
int k_post_thr_final(isle_ctx* c, uint32_t k, uint32_t r, const int* sizes_dev);
int k_post_edge(isle_ctx* c, const int64_t* pairs_dev, int n, float a, float b, float* edge_dev);

// model_text.hip: the reference's text of a V x ncols column-major device model (ISLE_TEXT_SPARSE / ISLE_TEXT_DENSE) handed to `sink` in
// pieces of at most ISLE_TEXT_CHUNK_BYTES; pairs_dev != null: column e is a * model[:, pairs[2e]] + b * model[:, pairs[2e + 1]] (post_edge_k's
// arithmetic) formed while it is read.  sink == null: the counting pass only.
constexpr uint64_t ISLE_TEXT_CHUNK_BYTES = 16ull << 20;
int k_model_text(isle_ctx* c, const float* model_dev, uint64_t V, uint64_t ncols, const int64_t* pairs_dev, float a, float b, int format,
                 isle_text_sink_fn sink, void* user, uint64_t* nbytes, uint64_t* nentries);
// ... and the delivery every text formatter shares: a text of `total` > 0 bytes whose ntiles tiles lie at offs_dev (ntiles + 1 offsets on
// the device) goes to `sink` in chunks of at most ISLE_TEXT_CHUNK_BYTES cut between tiles (at multiples of `group` tiles where possible);
// write(t0, n, out) launches the formatting of tiles [t0, t0 + n) into out on the context's stream
int k_text_pump(isle_ctx* c, const char* who, const uint64_t* offs_dev, uint64_t ntiles, uint64_t total, uint64_t group, isle_text_sink_fn sink,
                void* user, const std::function<int(uint64_t, uint64_t, unsigned char*)>& write);

// infer_text.hip: the lines "<row + base>\t<topic + 1>\t<weight>\n" of rows [row_begin, row_end) of the resident inference result
// (ISLE_DOCTEXT_ENTRIES: c->inf_off / inf_topic / inf_weight; ISLE_DOCTEXT_TOP: c->inf_top_topic / inf_top_weight), delivered as k_model_text
// delivers.  The caller has checked the range and c->res.inf_valid.
int k_infer_text(isle_ctx* c, int what, uint64_t row_begin, uint64_t row_end, uint64_t base, isle_text_sink_fn sink, void* user, uint64_t* nbytes,
                 uint64_t* nlines);

// doc_report.hip: the trainer's per-document report files (ISLE_DOCREPORT_*) for documents [doc_begin, doc_end) of A from the resident
// catchword map, (document, topic) sums and top-two topics, delivered as k_model_text delivers.  The caller has checked the range and
// that the stage that made the source has run.
int k_doc_report_text(isle_ctx* c, int what, uint64_t doc_begin, uint64_t doc_end, isle_text_sink_fn sink, void* user, uint64_t* nbytes,
                      uint64_t* nlines);
// ... and the steps of ISLE_DOCREPORT_TOPIC_SUMS over document shards (route_topic_sums == TOPIC_SUMS_GATHERED), between the collectives of
// api_stages.cpp: the range's sums; this rank's block of (key, global document) pairs padded to nmax; the replicated sort of the L gathered
// pairs and the lines [L0, L1) of the corpus's file
int k_dr_sums_range(isle_ctx* c, uint64_t doc_begin, uint64_t doc_end, uint64_t* first, uint64_t* n);
int k_dr_sums_keys(isle_ctx* c, uint64_t doc_begin, uint64_t doc_end, uint64_t first, uint64_t n, uint64_t nmax, uint64_t* key, uint32_t* doc);
int k_dr_sums_gathered_text(isle_ctx* c, uint64_t* key_a, uint32_t* doc_a, uint64_t* key_b, uint32_t* doc_b, uint64_t L, uint64_t L0, uint64_t L1,
                            isle_text_sink_fn sink, void* user, uint64_t* nbytes, uint64_t* nlines);

// topic_docs.hip: the device steps of isle_hip_topic_top_docs (the rule: topdocs_host.h) on a CSR of (topic, value) over `rows` rows, between
// the collectives of api_stages.cpp.  Every buffer is the call's; device time goes to `fam`.
struct TdView {
  const int64_t* off;  // rows + 1, off[0] = 0
  const uint32_t* topic;
  const float* value;
  uint64_t rows, nnz, doc_base;
  uint32_t num_topics, n;
  int fam;
};
int k_td_docs(isle_ctx* c, const TdView& v, uint32_t* doc, uint64_t* cnt, uint64_t* err_dev, uint64_t* bad);
int k_td_init(isle_ctx* c, const TdView& v, const uint64_t* cnt, uint64_t* prefix, uint32_t* rem);
int k_td_hist(isle_ctx* c, const TdView& v, const uint32_t* doc, const uint64_t* prefix, int shift, uint32_t* bins);
int k_td_step(isle_ctx* c, const TdView& v, const uint32_t* bins, const uint64_t* cnt, int shift, uint64_t* prefix, uint32_t* rem);
int k_td_collect(isle_ctx* c, const TdView& v, const uint32_t* doc, const uint64_t* tau, uint32_t* fill, uint64_t* table);
int k_td_sort(isle_ctx* c, const TdView& v, const uint64_t* tables, uint32_t world, const uint64_t* cnt, uint32_t* docs, float* values, uint32_t* counts);

// similar_docs.hip: the device steps of isle_hip_similar_docs (the rule: simdocs_host.h) ahead of that selection.  v: the source's rows, its
// num_topics the table's; lds: the table's home (route_simdocs_table); Qp = simdocs_qp(Q).  Every buffer is the call's, on the device unless
// named host.  k_sd_gather_offsets / k_sd_gather: the queries are rows qrows_dev of the source -> the query CSR.  k_sd_table: table
// (num_topics x Qp) and nq (Qp) from the query CSR.  k_sd_count: cnt (rows), pair_off (rows + 1; blk: scan scratch of `rows`), *bad: ~0, or
// (entry << 2) | what of the first bad entry of a row (1, 2: topdocs_entry_fault; SIMDOCS_BAD_WEIGHT), *pairs: this rank's candidate
// pairs.  k_sd_score: (query, score) of every pair at pair_off: with pair_off a TdView whose topic is the query.  exclude: Qp documents.
int k_sd_gather_offsets(isle_ctx* c, const TdView& v, const uint64_t* qrows_dev, uint32_t Q, int64_t* q_off_dev, int64_t* q_off_host);
int k_sd_gather(isle_ctx* c, const TdView& v, const uint64_t* qrows_dev, uint32_t Q, const int64_t* q_off_dev, uint32_t* q_topic, float* q_weight);
int k_sd_table(isle_ctx* c, int fam, uint32_t Q, uint32_t num_topics, const int64_t* q_off, const uint32_t* q_topic, const float* q_weight, float* table,
               double* nq);
int k_sd_count(isle_ctx* c, const TdView& v, bool lds, uint32_t Q, const float* table, const uint32_t* exclude, uint32_t* cnt, int64_t* pair_off, int64_t* blk,
               uint64_t* err_dev, uint64_t* bad, uint64_t* pairs);
int k_sd_score(isle_ctx* c, const TdView& v, int measure, bool lds, uint32_t Q, const float* table, const uint32_t* exclude, const double* nq,
               const int64_t* pair_off, uint32_t* qid, float* score);

// topic_prevalence.hip: the device steps of isle_hip_topic_prevalence (the rule: prevalence_host.h).  v: the source's rows, its num_topics k;
// G groups.  Every buffer is the call's, on the device unless named host; device time goes to v.fam.
// k_tp_rows: docs (G + 1: the last counts the rows of no group), count and dominant (G x k), zeroed there; rs (rows, nullable): the row
//   sums; label / rowid (rows each, nullable): the pairs of the sort by label; *bad_row: ~0, or the first row with a bad label;
//   *bad_entry: ~0, or (entry << 2) | what of the first bad entry (1, 2: topdocs_entry_fault; PREV_BAD_WEIGHT).  Drained when it returns.
// k_tp_bases: bases ((levels + 1) x (G + 1)): per level the exclusive scan of every group's values, level 0 the rows; cnt: G words,
//   blk: scan scratch of G.
// k_tp_tile: topics [t0, t0 + tw) of sum (G x k, zeroed by the caller) through every level; list: the rows by group (null: the identity);
//   totals (host, levels + 1): the values of each level over all groups; part_a / part_b: totals[1] x tw and totals[2] x tw doubles.
int k_tp_rows(isle_ctx* c, const TdView& v, const uint32_t* groups_dev, uint32_t G, uint64_t* docs, uint64_t* count, uint64_t* dominant, double* rs,
              uint64_t* label, uint32_t* rowid, uint64_t* err_dev, uint64_t* bad_row, uint64_t* bad_entry);
int k_tp_bases(isle_ctx* c, int fam, const uint64_t* docs, uint32_t G, int levels, uint64_t* bases, uint64_t* cnt, uint64_t* blk);
int k_tp_tile(isle_ctx* c, const TdView& v, const uint32_t* list, const double* rs, uint32_t G, const uint64_t* bases, int levels, const uint64_t* totals,
              uint32_t t0, uint32_t tw, double* part_a, double* part_b, double* sum);

// infer_resident.hip: a V x k column-major device model into `out`, V x round4(k) row-major with zero padding (inf_pack_k)
int k_inf_pack(isle_ctx* c, const float* model_cm_dev, uint64_t V, int k, float* out);
// score_docs.hip: the device steps of isle_hip_score_docs (the rule: score_host.h).  w: the weight rows, its num_topics the model's columns.
// Every buffer is the call's; device time goes to ISLE_T_INFER.
// k_sc_rows: every weight row checked, rs (rows) = the row sums s_d; *bad: ~0, or (entry << 2) | what of the first bad weight entry (1, 2:
//   topdocs_entry_fault; SCORE_BAD_WEIGHT).  Drained when it returns.
// k_sc_walk: M: the packed model, vocab x ld; document r has the entries [off[r], off[r + 1]) of cnt / word (off need not begin at 0);
//   rs: the row sums, or null without normalise; the five per-document outputs (rows each); z_out: null, or z of entry e at z_out[e];
//   *bad: ~0, or (entry << 1) | what of the first bad entry (SCORE_BAD_WORD, SCORE_BAD_COUNT).  Drained when it returns.
int k_sc_rows(isle_ctx* c, const TdView& w, double* rs, uint64_t* err_dev, uint64_t* bad);
int k_sc_walk(isle_ctx* c, const TdView& w, const float* M, int ld, uint64_t vocab, const float* cnt, const uint32_t* word, const int64_t* off,
              const double* rs, int measure, double floor, double* score, double* tokens, uint32_t* unscored_entries, double* unscored_tokens,
              uint32_t* floored, double* z_out, uint64_t* err_dev, uint64_t* bad);

// vocab.hip: the device steps of isle_hip_word_doc_freq / isle_hip_prune_vocab on the resident A (the rule: vocab_host.h).  k_vocab_df: df_dev
// (a_V words, zeroed there) = this rank's entries per word.  k_vocab_compact: A under remap_dev (a_V words: the new id, or 0xffffffff) out of
// place into the caller's twin buffers, sized there; *emptied: this rank's documents that lost all of their entries.  Device time: ISLE_T_INGEST.
int k_vocab_df(isle_ctx* c, VocabHist form, uint32_t* df_dev);
int k_vocab_compact(isle_ctx* c, const uint32_t* remap_dev, DevBuf<float>& new_cnt, DevBuf<uint32_t>& new_rows, DevBuf<int64_t>& new_offs, uint64_t* total,
                    uint64_t* emptied);

// docs.hip: the device steps of isle_hip_doc_lengths / isle_hip_doc_duplicates / isle_hip_prune_docs on the resident A (the rule:
// docs_host.h).  Every array is the caller's, a_D elements (at least one).  Nothing resident is written.  Device time: ISLE_T_INGEST.
// k_docs_len_hash: words, tokens and the 64-bit hash of every document (hash nullable).
// k_docs_first_of: first_of[d] = the smallest document with d's content; hash is consumed (it becomes the sort's keys, cut as the form
//   says); *dups: the documents that are not the first of their kind; *rounds: the rounds of the resolution.
// k_docs_keep: the rule's flags.  first_of is read where dups (and rewritten as reported), written otherwise; keep[d] = 1 where d stays;
//   dropped[3] and *kept are this rank's.
// k_docs_compact: the kept columns out of place into the caller's twin buffers, sized there, and kept_docs (new_docs elements) =
//   a_doc_offset + the old number; new_docs as k_docs_keep counted them.
int k_docs_len_hash(isle_ctx* c, uint32_t* words, uint64_t* tokens, uint64_t* hash);
int k_docs_first_of(isle_ctx* c, DocHash form, const uint32_t* words, uint64_t* hash, uint32_t* first_of, uint64_t* dups, uint64_t* rounds);
int k_docs_keep(isle_ctx* c, const uint32_t* words, const uint64_t* tokens, const uint64_t bounds[4], bool dups, uint32_t* first_of, uint32_t* keep,
                uint64_t dropped[3], uint64_t* kept);
int k_docs_compact(isle_ctx* c, const uint32_t* keep, const uint32_t* words, uint64_t new_docs, DevBuf<float>& new_cnt, DevBuf<uint32_t>& new_rows,
                   DevBuf<int64_t>& new_offs, uint32_t* kept_docs, uint64_t* total);

// near_dups.hip: the device steps of isle_hip_doc_signatures / isle_hip_doc_jaccard / isle_hip_doc_near_duplicates /
// isle_hip_prune_near_docs on the resident A (the rule: neardup_host.h).  Every array is the caller's, on the device.  Nothing resident is
// written.  Device time: ISLE_T_INGEST.
// k_nd_signatures: sig (a_D x H row-major, nullable) and the band keys, not cut (bands x a_D band-major, nullable); queued, not drained.
// k_nd_jaccard: inter and uni of the n_pairs pairs (a[i], b[i]), every id < a_D (the caller has checked); queued, not drained.
// k_nd_resolve: the resolution across the bands from the keys: parent, first_of and keep (a_D each); *kept, *pairs_tested and *rounds are
//   on the host when it returns.
int k_nd_signatures(isle_ctx* c, int bands, int rows_per_band, uint64_t* sig, uint64_t* keys);
int k_nd_jaccard(isle_ctx* c, uint64_t n_pairs, const uint32_t* a, const uint32_t* b, uint32_t* inter, uint32_t* uni);
int k_nd_resolve(isle_ctx* c, NdKey form, uint64_t num, uint64_t den, int bands, const uint64_t* keys, uint32_t* parent, uint32_t* first_of, uint32_t* keep,
                 uint64_t* kept, uint64_t* pairs_tested, uint64_t* rounds);

// model_compare.hip: the device steps of isle_hip_compare_models / isle_hip_match_topics (the rule: match_host.h).  Every array is the
// caller's, on the device.  Nothing resident is written.  Device time: ISLE_T_POST.
// k_mc_dist: dist (ka x kb row-major doubles) = the L1 distances of the columns of a (V x ka) and b (V x kb), column-major fp32, the words
//   cut into `slices` slices (route_model_dist_slices); a and b may be one buffer.  Its scratch goes with the call: the stream is drained when it returns.
// k_mc_match: the greedy matching of dist (na x nb) by rounds of mutually best pairs; match_a (na), match_b (nb), match_dist (na);
//   *n_matched and *rounds (the rounds that matched a pair) are on the host when it returns.
int k_mc_dist(isle_ctx* c, const float* a, int ka, const float* b, int kb, uint64_t V, uint32_t slices, double* dist);
int k_mc_match(isle_ctx* c, const double* dist, int na, int nb, int32_t* match_a, int32_t* match_b, double* match_dist, uint64_t* n_matched, uint32_t* rounds);

// model_load.hip: the text of a model file (n bytes on the device, ISLE_TEXT_SPARSE / ISLE_TEXT_DENSE) parsed into model_dev (V x ncols
// column-major).  *err_key: ~0 = none, else (byte position << 3) | kind of the first offending byte (isle_hip_load_model_text names them);
// *nentries: lines parsed (SPARSE), tokens (DENSE)
int k_load_model_text(isle_ctx* c, const unsigned char* text_dev, uint64_t n, uint64_t V, uint32_t ncols, int format, unsigned base, float* model_dev,
                      uint64_t* nentries, uint64_t* err_key);

// coherence.hip: D(w) for the distinct top words U (ascending) and D(lo, hi) for the distinct pairs of their local ids (CSR keyed by lo),
// over the count matrix A; counts = |U| + |P| entries on the host
int k_coherence_counts(isle_ctx* c, const std::vector<uint32_t>& U, const std::vector<uint32_t>& part_off, const std::vector<uint32_t>& part_hi,
                       std::vector<uint32_t>& counts, int* passes);

// avg_model.hip: the cluster-average model into c->p_avg_model (needs a_nv and p_cluster_of); the n heaviest words of every column of a
// device model (ids / weights: ncols x n on the device); topic diversity of a device model (dist, abar: device; kprime: host)
int k_avg_model(isle_ctx* c, uint32_t k);
int k_model_top_words(isle_ctx* c, const float* model_dev, uint64_t V, uint32_t ncols, int n, uint32_t* ids_dev, float* weights_dev);
int k_topic_diversity(isle_ctx* c, const float* model_dev, uint64_t V, uint32_t k, double* dist_dev, double* abar_dev, int32_t* finite_dev,
                      uint32_t* kprime);
// ... and the n heaviest words of the edge topics a * model[:, pairs[2e]] + b * model[:, pairs[2e + 1]] (post_edge_k's arithmetic), formed
// while they are read: no V x n_edge buffer
int k_edge_top_words(isle_ctx* c, const float* model_dev, uint64_t V, const int64_t* pairs_dev, uint32_t n_edge, float a, float b, int n,
                     uint32_t* ids_dev, float* weights_dev);

// edge_select.hip: the pair selection of construct_edge_topics_v2 over D device-resident (top1, top2), k <= ISLE_EDGE_TABLE_MAX_TOPICS.
// pairs_host: min(*n_selected, cap) triples (primary, secondary, documents); *threshold: the count of the first candidate cut off, 0 when
// nothing is cut; *bad_doc: ~0, or the first document whose id is >= k or < -1 (nothing else is defined then)
int k_edge_select(isle_ctx* c, const int32_t* top1_dev, const int32_t* top2_dev, uint64_t D, uint32_t k, uint64_t max_edge_topics, uint64_t min_docs,
                  int64_t* pairs_host, uint64_t cap, uint64_t* n_selected, uint64_t* n_candidates, uint64_t* threshold, uint64_t* bad_doc);

// corpus_stats.hip: the trainer's corpus diagnostics on A.  k_log_combinatorial: out (host, a_D floats), max_words (nullable);
// k_top_five_runs (needs a_nv): the number of documents with >= 5 entries, the run lengths of their sorted top-five tuples, the
// tuples (nullable, host, n x 5)
int k_log_combinatorial(isle_ctx* c, float* out, uint64_t* max_words);
int k_top_five_runs(isle_ctx* c, uint64_t* n_out, std::vector<uint64_t>& runs, float* tuples);

// dense.hip
int k_ensure_pt(isle_ctx* c);  // the coordinate-major f32 copy of the projection, made from P when a route asks for it (dense.hip)
int k_vtf(isle_ctx* c, const float* Vb, uint64_t n, int m, const float* F, int b, float* coef /*m x b col-major dev*/, uint64_t ld = 0);
int k_update(isle_ctx* c, float* F, uint64_t n, int b, const float* Vb, int m, const float* coef, uint64_t ld = 0);
int k_panel_qr(isle_ctx* c, float* F, uint64_t n, int w, float* Qdst, float* R_host /*w*w*/, int* rank_out);
int k_panel_qr_kernels(isle_ctx* c, float* F, uint64_t n, int w, float* Qdst, int* meta_dev /*2 + 32*/, float* Rout_dev /*w*w*/);
int k_randu(isle_ctx* c, float* F, uint64_t count, uint64_t seed);
int k_gemm_nn(isle_ctx* c, const float* A, uint64_t M, int K, const float* B, int ldb, int N, float* C, int family = ISLE_T_ROTATE);  // col-major, lda = ldc = M
// the same product for the D x k x k dot products of the assignment steps: bf16 matrix cores, operands split in three bf16 terms (gemm_bf16x3.h)
int k_gemm_nn_assign(isle_ctx* c, const float* A, uint64_t M, int K, const float* B, int ldb, int N, float* C, int family);
int k_gemm_assign_yy(isle_ctx* c, const float* A, const float* Arm, int lda_rm, const float* an, uint64_t M, int K, const float* B, int ldb, int N, int G,
                     const float* cn, const float* dn, const float* cn_max, uint32_t* assign, float* ub, float* lb, int family, const void* A2 = nullptr,
                     const uint32_t* map2 = nullptr /*row of A2 -> document when A2 lies by position; A may be null then (made on demand)*/);
int k_gemm_assign_tiles(isle_ctx* c, const float* A, const float* Arm, int lda_rm, uint64_t M, int K, const float* B, int ldb, int N, int TL, const float* cn,
                        const float* pn, const float* cmax, uint32_t* assign, float* ub, float* tlb, int family, const uint32_t* map0 = nullptr,
                        const void* A2 = nullptr, const uint32_t* map2 = nullptr);
// A2 = the two bf16 terms of a coordinate-major M x K operand in the layout gemm_bf16x2_dma_k stages by LDS-DMA (gemm_bf16x3.h); bytes it needs
int k_gemm_split_a(isle_ctx* c, const float* A, uint64_t M, int K, void* A2);
size_t k_gemm_split_a_bytes(uint64_t M, int K);
int k_transpose(isle_ctx* c, const float* in, uint64_t rows, uint64_t cols, uint64_t ld_in, float* out, uint64_t ld_out);  // out[c*ld_out + r]... see impl
int k_jacobi_eig(isle_ctx* c, const float* S_host, int n, float* evals_host, float* vecs_dev /*n x n col-major*/);
int k_eig_small(isle_ctx* c, const float* S_host, int n, float* evals_host, float* vecs_dev /*n x nvec col-major*/, int nvec);
int k_colnorms_rm(isle_ctx* c, const float* Mrm, uint64_t rows, int k, int ldk, float* out, const float* Sub = nullptr);
int k_scale_centers(isle_ctx* c, float* Crm, uint64_t rows, int k, int ldk, const int* counts);

// evd_tridiag.hip
int k_tridiag_eig(isle_ctx* c, const float* S_host, int n, float* evals_host, float* vecs_dev, int nvec);  // evd_tridiag.hip; 1 = use another solver; evals_host[nvec..n) = 0

// kmeans.hip
int k_member_lists(isle_ctx* c, const uint32_t* assign, uint64_t D, int k, const int* counts_dev, int* max_out, std::vector<int>* counts_host = nullptr);
int k_member_lists_dev(isle_ctx* c, const uint32_t* assign, uint64_t D, int k, const int* counts_dev);  // no host round trip
int k_yy_delta(isle_ctx* c, float* delta_dev, int k, int G, int group, float* gmax_dev, const uint32_t* id_of_slot = nullptr);
int k_max_f32(isle_ctx* c, const float* v, int n, float* out_dev);
int k_compact_rows(isle_ctx* c, const float* P, const float* pn, int ldk, const uint32_t* active, uint32_t n, float* Pa, float* pna);
// s_old = seeds before the nc new ones; track: also keep the nearest seed and the tile minima where the route allows (c->kmpp_track)
int k_kmpp_update(isle_ctx* c, const float* P, const float* pn, uint64_t D, int k, int ldk, const float* newC, int nc, float* min_dist, int s_old = -1,
                  bool track = false);
int k_kmpp_to_tiles(isle_ctx* c, uint64_t D, int k, const float* pn, const float* cn, const float* best, uint32_t* assign, float* ub, int TL);
int k_scan_f2d(isle_ctx* c, const float* in, uint64_t n, double* cum /*n+1*/);
int k_search(isle_ctx* c, const double* cum, uint64_t n, const double* dice_dev, int nd, uint64_t* out_dev);
int k_search_args(isle_ctx* c, const double* cum, uint64_t n, const double* dice_host, int nd /*<= 16*/, uint64_t* out_dev);
int k_fetch_rows(isle_ctx* c, const float* P, int ldk, const uint64_t* local_ids /*~0: not on this rank*/, int n, float* dst);
int k_pack2(isle_ctx* c, const double* a, const float* b /*nullable*/, double* out2);
int k_search_frac(isle_ctx* c, const double* cum, uint64_t n, const float* last /*nullable*/, const double* frac_host, int nd /*<= 40*/,
                  uint64_t* out_dev /*42 x 8 bytes: positions, then {cum[n], last[0]} as doubles*/);
int k_proj_assign(isle_ctx* c, const float* P, const float* pn, uint64_t D, int k, int ldk, const float* C, const float* cn, uint32_t* assign,
                  float* ub = nullptr, float* lb = nullptr);
int k_proj_assign_active(isle_ctx* c, const float* P, const float* pn, int k, int ldk, const float* C, const float* cn,
                         const uint32_t* active, uint32_t n, float* Pa, float* pna, uint32_t* assign, float* ub, float* lb);
bool k_proj_full_by_gemm(isle_ctx* c, uint64_t D, int k);  // the full tile-bound pass goes through the library GEMM (kmeans.hip)
int k_proj_assign_tiles(isle_ctx* c, const float* P, const float* pn, uint64_t D, int k, int ldk, const float* C, const float* cn, uint32_t* assign,
                        float* ub, float* tlb, int TL, const uint32_t* active, uint32_t n, const uint32_t* need, float* Pa, float* pna);
int k_rownorms_diff(isle_ctx* c, const float* A, const float* B, int rows, int k, int ldk, float* out);
int k_rownorms(isle_ctx* c, const float* M, int rows, int k, int ldk, float* out);
int k_proj_accumulate(isle_ctx* c, const float* P, uint64_t D, int k, int ldk, const uint32_t* assign, float* Csum, int* counts);
int k_proj_accumulate_delta(isle_ctx* c, const float* P, uint64_t D, int k, int ldk, const uint32_t* assign, uint32_t* counted, float* Csum,
                            const int* counts, bool* done);
int k_proj_finalize(isle_ctx* c, const float* Csum, const int* counts, int k, int ldk, float* C);
int k_count_sizes(isle_ctx* c, const uint32_t* assign, uint64_t D, int k, int* counts);
// objective.hip: c->ob_dd[d] = max(0, |x_d - c_assign[d]|^2) in fp64 for the local documents, c->ob_sums / c->ob_acc[2k, 3k) the clusters'
// sums and sizes over all ranks (collective).  space WORD: centres V x ld row-major, order (nullable) a permutation of the local documents
// that only shapes the visiting order; PROJECTED: centres k x ld, documents = rows of c->P.  fam: the timing family of the kernels.
int k_objective(isle_ctx* c, int space, int k, const uint32_t* assign, const float* centres, int ld, const uint32_t* order, int fam);
int k_compare_u32(isle_ctx* c, const uint32_t* a, const uint32_t* b, uint64_t n, int* flag_dev);
int k_fill_f32(isle_ctx* c, float* p, uint64_t n, float v);
