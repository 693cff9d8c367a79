// isle_amd/host/fpsparse_hip.h — C++ host side above the C ABI: the hot-path subset of the reference's
// ISLE::FPSparseMatrix<float> (include/sparseMatrix.h:204-467) with the SAME method names, argument meaning
// and error behaviour, each forwarding to libisle_hip.so.  Header-only; link with -lisle_hip.
//
// A maintainer of the reference would paste these bodies into src/sparseMatrix.cpp;
// this class exists so that the call sequence of ISLETrainer::train() (src/trainer.cpp:490-571) can be
// compiled and run against the GPU library without the reference's MKL-dependent sources.
#pragma once
#include <sys/stat.h>

#include <cassert>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <stdexcept>
#include <algorithm>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/isle_hip.h"
#include "model_read.h"
#include "tdf_pump.h"

namespace ISLE {

// include/types.h:24-36 under -DMKL_ILP64 -DSINGLE
typedef uint64_t word_id_t;
typedef uint64_t doc_id_t;
typedef int64_t offset_t;
typedef float FPTYPE;
typedef uint32_t count_t;  // include/types.h:29

// include/hyperparams.h
#define ISLE_BLOCK_KS_MAX_ITERS 100
#define ISLE_BLOCK_KS_BLOCK_SIZE 10
#define ISLE_BLOCK_KS_TOLERANCE 1e-4f
#define ISLE_W0_C (1.0)            // :8
#define ISLE_EPS2_C (1.0 / 3.0)    // :10
#define ISLE_RHO_C (1.1)           // :11
#define ISLE_EPS3_C (5.0)          // :12
#define ISLE_EDGE_TOPIC_MIN_DOCS 1          // :77
#define ISLE_EDGE_TOPIC_PRIMARY_RATIO 0.7   // :79
#define ISLE_DEFAULT_COHERENCE_EPS (1e-5)   // :74
#define ISLE_DEFAULT_COHERENCE_NUM_WORDS 5  // :75
#define ISLE_INFER_ITERS_DEFAULT 15  // :81
#define ISLE_INFER_LF_DEFAULT 10.0f  // :82 (INFER_LF_DEAFULT there)

namespace fpsparse_detail {

// The pair selection of ISLETrainer::construct_edge_topics_v2 (src/trainer.cpp:1120-1145) on the host: THE RULE that
// isle_hip_select_edge_pairs (isle_amd/csrc/edge_select.hip) and hot_path.select_edge_pairs restate, and the path taken for more than
// ISLE_EDGE_TABLE_MAX_TOPICS topics.  Documents with top1 >= 0 and top2 >= 0 are counted per ordered pair; pairs with >= min_docs
// documents are candidates; candidates are ordered by count descending, ties by (primary, secondary) ascending (the reference's sort
// is unstable there); the first max_edge_topics are kept.  *threshold: the count of the first candidate cut off, 0 when nothing is cut.
inline void select_edge_pairs_host(const int32_t* top1, const int32_t* top2, const uint64_t n_docs, const int64_t max_edge_topics, const uint64_t min_docs,
                                   std::vector<std::tuple<int, int, uint64_t>>& selected_pairs, uint64_t* candidates, uint64_t* threshold) {
  std::vector<std::pair<int, int>> pairs;
  for (uint64_t d = 0; d < n_docs; ++d)
    if (top1[d] >= 0 && top2[d] >= 0) pairs.push_back(std::make_pair((int)top1[d], (int)top2[d]));
  std::sort(pairs.begin(), pairs.end());  // (primary, secondary) ascending
  selected_pairs.clear();
  for (size_t i = 0; i < pairs.size();) {
    size_t j = i;
    while (j < pairs.size() && pairs[j] == pairs[i]) ++j;
    if ((uint64_t)(j - i) >= min_docs) selected_pairs.push_back(std::make_tuple(pairs[i].first, pairs[i].second, (uint64_t)(j - i)));
    i = j;
  }
  if (candidates) *candidates = selected_pairs.size();
  std::stable_sort(selected_pairs.begin(), selected_pairs.end(),
                   [](const std::tuple<int, int, uint64_t>& l, const std::tuple<int, int, uint64_t>& r) { return std::get<2>(l) > std::get<2>(r); });
  if (threshold) *threshold = 0;
  const size_t keep = (size_t)std::max<int64_t>(max_edge_topics, 0);
  if (selected_pairs.size() > keep) {
    if (threshold) *threshold = std::get<2>(selected_pairs[keep]);
    selected_pairs.resize(keep);
  }
}

}  // namespace fpsparse_detail

class FPSparseMatrixHip {
  word_id_t vocab_size_;
  doc_id_t num_docs_;
  offset_t nnzs_ = 0;
  isle_ctx* ctx_ = nullptr;
  bool uploaded_ = false;
  doc_id_t U_cols_ = 0;
  bool compute_residual_ = false;  // set_compute_residual: the loops print and return the reference's residual
  int last_nconv_ = 0;  // Ritz pairs that really passed the residual test in the last compute_block_ks
  doc_id_t a_docs_ = 0;  // documents of the count matrix A (from_counts / from_tdf)
  std::vector<uint64_t> top5_runs_;  // count_distint_top_five_words: run lengths of the sorted tuples, from the first call
  uint64_t top5_n_ = 0;
  bool top5_ready_ = false;
  doc_id_t post_topics_ = 0;  // num_topics of the last find_catchwords: the columns of the resident models
  word_id_t loaded_vocab_ = 0;  // the model of the last load_model_file (ISLE_MODEL_LOADED)
  doc_id_t loaded_cols_ = 0;
  word_id_t model_vocab(int which) const { return which == ISLE_MODEL_LOADED ? loaded_vocab_ : vocab_size_; }
  doc_id_t model_cols(int which) const { return which == ISLE_MODEL_LOADED ? loaded_cols_ : post_topics_; }

  static int text_to_file(const char* bytes, uint64_t n, void* fp) { return std::fwrite(bytes, 1, (size_t)n, (FILE*)fp) == (size_t)n ? 0 : 1; }

  void check(int rc, const char* what) const {
    if (rc != 0) throw std::runtime_error(std::string(what) + ": " + isle_hip_last_error(ctx_));
  }
  void upload() {
    if (uploaded_) return;
    check(isle_hip_upload_csc_u64(ctx_, vocab_size_, num_docs_, (uint64_t)nnzs_, vals_CSC, rows_CSC, offsets_CSC, 0, num_docs_),
          "upload_csc");
    uploaded_ = true;
  }
  void fill_partition(const uint32_t* assign, std::vector<doc_id_t>* closest_docs, doc_id_t num_centers) const {
    if (!closest_docs) return;
    for (doc_id_t c = 0; c < num_centers; ++c) closest_docs[c].clear();
    for (doc_id_t d = 0; d < num_docs_; ++d) closest_docs[assign[d]].push_back(d);  // ascending, as :1669-1672
  }

  void threshold_on_device(doc_id_t num_topics, double sample_rate, std::vector<doc_id_t>& original_cols, std::vector<FPTYPE>* zetas,
                           uint64_t* entries_above_threshold, float* avg_doc_sz) {
    uint64_t docs_kept = 0, nnz_kept = 0;
    check(isle_hip_threshold(ctx_, num_topics, sample_rate, 0, &docs_kept, &nnz_kept, entries_above_threshold, avg_doc_sz), "threshold");
    num_docs_ = docs_kept;
    nnzs_ = (offset_t)nnz_kept;
    uploaded_ = true;
    original_cols.resize(docs_kept);
    static_assert(sizeof(doc_id_t) == sizeof(uint64_t), "doc_id_t is 8 bytes (include/types.h:25)");
    if (zetas) zetas->resize(vocab_size_);
    check(isle_hip_get_B(ctx_, nullptr, nullptr, nullptr, (uint64_t*)original_cols.data(), zetas ? zetas->data() : nullptr), "get_B");
  }

 public:
  // the reference re-exports these as public (include/sparseMatrix.h:216,227-230)
  FPTYPE* vals_CSC = nullptr;
  word_id_t* rows_CSC = nullptr;
  offset_t* offsets_CSC = nullptr;

  FPSparseMatrixHip(word_id_t d, doc_id_t s, int device = 0) : vocab_size_(d), num_docs_(s) {
    ctx_ = isle_hip_create(device);
    if (!ctx_) throw std::runtime_error("isle_hip_create failed: no MI355X device (there is no CPU fallback)");
    offsets_CSC = new offset_t[s + 1]();
  }
  ~FPSparseMatrixHip() {
    delete[] vals_CSC;
    delete[] rows_CSC;
    delete[] offsets_CSC;
    isle_hip_destroy(ctx_);
  }
  FPSparseMatrixHip(const FPSparseMatrixHip&) = delete;

  // Device-side equivalent of SparseMatrix::normalize_docs + compute_thresholds (src/sparseMatrix.cpp:136-167, :357-485)
  // followed by FPSparseMatrix(A_sp, true) + threshold_and_copy / sampled_threshold_and_copy (:1285-1435), i.e. what
  // ISLETrainer::train does at src/trainer.cpp:430-485.  `counts`/`rows`/`offsets` are A_sp's CSC (populate_CSC layout).
  // B is built in device memory (the host CSC pointers of the returned object stay NULL); original_cols maps its columns
  // back to A's, zetas (optional) receives the per-word thresholds.
  static FPSparseMatrixHip* from_counts(word_id_t vocab_size, doc_id_t num_docs, const float* counts, const uint32_t* rows,
                                        const offset_t* offsets, doc_id_t num_topics, double sample_rate,
                                        std::vector<doc_id_t>& original_cols, std::vector<FPTYPE>* zetas = nullptr,
                                        uint64_t* entries_above_threshold = nullptr, float* avg_doc_sz = nullptr, int device = 0) {
    FPSparseMatrixHip* B = new FPSparseMatrixHip(vocab_size, 0, device);
    try {
      B->check(isle_hip_upload_counts_u32(B->ctx_, vocab_size, num_docs, (uint64_t)offsets[num_docs], counts, rows, offsets, 0, num_docs),
               "upload_counts");
      B->a_docs_ = num_docs;
      B->threshold_on_device(num_topics, sample_rate, original_cols, zetas, entries_above_threshold, avg_doc_sz);
    } catch (...) {
      delete B;
      throw;
    }
    return B;
  }

  // The same from (doc, word, count) triples in any order, fed in batches (ISLETrainer::feed_data / finalize_data, src/trainer.cpp:214-371):
  // begin_feed makes the object and opens the feed (isle_hip_feed_begin), feed appends a batch (0-based columns and word ids; zero counts are
  // skipped, an id out of range throws and leaves the feed as it was), from_feed sorts, keeps the first fed of equal (doc, word) pairs, builds
  // A and thresholds it, with from_counts' outputs; on failure it deletes the object like from_counts.
  static FPSparseMatrixHip* begin_feed(word_id_t vocab_size, doc_id_t num_docs, uint64_t reserve_entries, int device = 0) {
    FPSparseMatrixHip* B = new FPSparseMatrixHip(vocab_size, 0, device);
    try {
      B->check(isle_hip_feed_begin(B->ctx_, vocab_size, num_docs, reserve_entries), "feed_begin");
      B->a_docs_ = num_docs;
    } catch (...) {
      delete B;
      throw;
    }
    return B;
  }
  void feed(uint64_t n, const uint32_t* docs, const uint32_t* words, const uint32_t* counts) {
    check(isle_hip_feed_entries(ctx_, n, docs, words, counts), "feed_entries");
  }
  static FPSparseMatrixHip* from_feed(FPSparseMatrixHip* B, doc_id_t num_topics, double sample_rate, std::vector<doc_id_t>& original_cols,
                                      std::vector<FPTYPE>* zetas = nullptr, uint64_t* entries_above_threshold = nullptr, float* avg_doc_sz = nullptr,
                                      uint64_t* entries_fed = nullptr, uint64_t* entries_in_A = nullptr) {
    try {
      B->check(isle_hip_feed_finalize(B->ctx_, 0, 0, entries_fed, entries_in_A), "feed_finalize");
      B->threshold_on_device(num_topics, sample_rate, original_cols, zetas, entries_above_threshold, avg_doc_sz);
    } catch (...) {
      delete B;
      throw;
    }
    return B;
  }

  // The same with the ingest on the device as well: `text` holds the bytes of the tdf file
  // (DocWordEntriesReader::fill_doc_word_entries include/utils.h:158-228, the sort / de-duplication of
  // ISLETrainer::finalize_data src/trainer.cpp:236-247 and SparseMatrix::populate_CSC src/sparseMatrix.cpp:58-87).
  static FPSparseMatrixHip* from_tdf(word_id_t vocab_size, doc_id_t num_docs, const char* text, uint64_t nbytes, offset_t max_entries,
                                     doc_id_t num_topics, double sample_rate, std::vector<doc_id_t>& original_cols,
                                     uint64_t* entries_in_A = nullptr, uint64_t* entries_above_threshold = nullptr, float* avg_doc_sz = nullptr,
                                     int device = 0) {
    FPSparseMatrixHip* B = new FPSparseMatrixHip(vocab_size, 0, device);
    try {
      B->check(isle_hip_ingest_tdf(B->ctx_, text, nbytes, vocab_size, num_docs, (uint64_t)max_entries, nullptr, entries_in_A), "ingest_tdf");
      B->a_docs_ = num_docs;
      B->threshold_on_device(num_topics, sample_rate, original_cols, nullptr, entries_above_threshold, avg_doc_sz);
    } catch (...) {
      delete B;
      throw;
    }
    return B;
  }

  // The same from the file itself, never held whole: tdf_pump.h reads it piece by piece into the library's page-locked buffers
  // (isle_hip_tdf_acquire / _commit), each piece is copied and parsed while the next is read.  A equals from_tdf's on the file's bytes.
  static FPSparseMatrixHip* from_tdf_file(word_id_t vocab_size, doc_id_t num_docs, const std::string& path, offset_t max_entries, doc_id_t num_topics,
                                          double sample_rate, std::vector<doc_id_t>& original_cols, uint64_t* entries_in_A = nullptr,
                                          uint64_t* entries_above_threshold = nullptr, float* avg_doc_sz = nullptr, int device = 0, uint64_t piece_bytes = 0) {
    FPSparseMatrixHip* B = new FPSparseMatrixHip(vocab_size, 0, device);
    try {
      struct stat st;  // room for max_entries at once, where the file can hold that many ("1 1 1\n" is six bytes)
      const uint64_t room = ::stat(path.c_str(), &st) == 0 ? (uint64_t)st.st_size / 6 + 1 : 0;
      B->check(isle_hip_tdf_begin(B->ctx_, vocab_size, num_docs, std::min<uint64_t>((uint64_t)max_entries, room), piece_bytes), "tdf_begin");
      isle_ctx* ctx = B->ctx_;
      B->check(tdf_pump::file(path, [ctx](char** buf, uint64_t* cap) { return isle_hip_tdf_acquire(ctx, buf, cap); },
                              [ctx](uint64_t n) { return isle_hip_tdf_commit(ctx, n); }),
               "tdf stream");
      B->check(isle_hip_tdf_finalize(B->ctx_, (uint64_t)max_entries, nullptr, entries_in_A), "tdf_finalize");
      B->a_docs_ = num_docs;
      B->threshold_on_device(num_topics, sample_rate, original_cols, nullptr, entries_above_threshold, avg_doc_sz);
    } catch (...) {
      delete B;
      throw;
    }
    return B;
  }

  void allocate(offset_t nnzs) {  // SparseMatrix::allocate
    delete[] vals_CSC;
    delete[] rows_CSC;
    nnzs_ = nnzs;
    vals_CSC = new FPTYPE[nnzs];
    rows_CSC = new word_id_t[nnzs];
    uploaded_ = false;
  }
  word_id_t vocab_size() const { return vocab_size_; }
  doc_id_t num_docs() const { return num_docs_; }
  offset_t get_nnzs() const { return nnzs_; }

  FPTYPE frobenius() {  // src/sparseMatrix.cpp:1096-1100
    assert(offsets_CSC[0] == 0);
    upload();
    float f = 0.f;
    check(isle_hip_frobenius(ctx_, &f), "frobenius");
    return f;
  }
  void initialize_for_eigensolver(const doc_id_t num_topics) {  // :1150-1158 (device buffers are sized on demand)
    U_cols_ = num_topics;
    upload();
  }
  void compute_block_ks(const doc_id_t num_topics, std::vector<FPTYPE>& evalues) {  // :1195-1220
    upload();
    std::vector<float> ev(num_topics);
    int nconv = 0, restarts = 0, napplies = 0;
    const int rc = isle_hip_block_ks(ctx_, (int)num_topics, (int)(2 * num_topics + ISLE_BLOCK_KS_BLOCK_SIZE), ISLE_BLOCK_KS_MAX_ITERS,
                                     ISLE_BLOCK_KS_BLOCK_SIZE, ISLE_BLOCK_KS_TOLERANCE, 1, ev.data(), &nconv, &restarts, &napplies);
    // the reference reports nconv = nev even when maxit is exhausted and asserts on it (:1207)
    if (rc != 0 && rc != ISLE_E_NOCONV) check(rc, "compute_block_ks");
    if (rc == ISLE_E_NOCONV) {
      // the reference's log line says nconv = num_topics here and its assert passes; keep its line, but say what happened
      std::fprintf(stderr, "WARNING: block Krylov-Schur used all %d restarts; only %d of %d Ritz pairs passed the residual test "
                           "(tolerance %g). The unconverged Ritz vectors are used as they are, as the reference does.\n",
                   ISLE_BLOCK_KS_MAX_ITERS, nconv, (int)num_topics, (double)ISLE_BLOCK_KS_TOLERANCE);
      last_nconv_ = nconv;
    } else {
      last_nconv_ = (int)num_topics;
    }
    std::printf("Completed with %d restarts, nconv = %d\n", restarts, rc == ISLE_E_NOCONV ? (int)num_topics : nconv);
    for (doc_id_t i = 0; i < num_topics; ++i) evalues.push_back(ev[i]);
    U_cols_ = num_topics;
  }
  // the trace of the last loop in `space` as the reference prints its residuals; -> the last residual (0 with the flag clear)
  FPTYPE print_residuals(const int space) {
    if (!compute_residual_) return 0.0f;
    int n = 0;
    check(isle_hip_lloyds_trace_get(ctx_, space, nullptr, 0, &n), "lloyds_trace_get");
    std::vector<double> tr(n);
    check(isle_hip_lloyds_trace_get(ctx_, space, tr.data(), n, nullptr), "lloyds_trace_get");
    for (int i = 0; i < n; ++i) std::cout << "Lloyd's iter " << i << "  dist_sq residual: " << std::sqrt((FPTYPE)tr[i]) << "\n";
    return n ? (FPTYPE)tr[n - 1] : 0.0f;
  }
  void cleanup_after_eigensolver() {}  // :1264-1275 (U stays device-resident until the context dies)

  FPTYPE kmeans_init_on_projected_space(const int num_centers, const int max_reps, std::vector<doc_id_t>& best_seed,
                                        FPTYPE* const best_centers_coords) {  // :2212-2238
    FPTYPE best = 3.402823466e+38f;
    std::vector<uint64_t> seeds(num_centers), best_s;
    std::vector<float> coords((size_t)num_centers * num_centers);
    for (int rep = 0; rep < max_reps; ++rep) {
      float dist = 0.f;
      check(isle_hip_kmeanspp_projected(ctx_, num_centers, nullptr, 1 + rep, seeds.data(), coords.data(), &dist, nullptr),
            "kmeans_init_on_projected_space");
      std::cout << "k-means init residual: " << dist << std::endl;
      if (dist < best) {
        best = dist;
        best_s = seeds;
        if (best_centers_coords) std::memcpy(best_centers_coords, coords.data(), coords.size() * sizeof(float));
      }
    }
    best_seed.assign(best_s.begin(), best_s.end());
    return best;
  }
  FPTYPE run_lloyds_on_projected_space(const doc_id_t num_centers, FPTYPE* projected_centers, std::vector<doc_id_t>* closest_docs,
                                       const int max_reps) {  // :2016-2072
    if (closest_docs)
      for (doc_id_t c = 0; c < num_centers; ++c) assert(closest_docs[c].size() == 0);
    std::vector<uint32_t> assign(num_docs_);
    int iters = 0;
    check(isle_hip_lloyds_projected(ctx_, (int)num_centers, projected_centers, max_reps, &iters, assign.data()),
          "run_lloyds_on_projected_space");
    const FPTYPE residual = print_residuals(ISLE_SPACE_PROJECTED);  // the reference's loop prints none and returns 0 (:1995-1998)
    if (iters < max_reps) std::cout << "Lloyds converged\n";
    fill_partition(assign.data(), closest_docs, num_centers);
    return residual;
  }
  // out == NULL: the product stays on the device as the start point of run_lloyds(k, NULL, ...)
  void left_multiply_by_U_Spectra(FPTYPE* const out, const FPTYPE* in, const doc_id_t ld_in, const doc_id_t ncols) {  // :1438-1450
    assert(ld_in >= U_cols_);
    check(isle_hip_lift_centers(ctx_, in, (int)ld_in, (int)ncols, out), "left_multiply_by_U_Spectra");
  }
  // centers == NULL: start from the centres left_multiply_by_U_Spectra(NULL, ...) left on the device and do not copy the result back
  // (src/trainer.cpp reads only closest_docs after this call; V x k floats are 400 MB at vocab 100k, k = 1000).
  FPTYPE run_lloyds(const doc_id_t num_centers, FPTYPE* centers, std::vector<doc_id_t>* closest_docs, const int max_reps) {  // :1690-1746
    if (closest_docs)
      for (doc_id_t c = 0; c < num_centers; ++c) assert(closest_docs[c].size() == 0);
    upload();
    std::vector<uint32_t> assign(num_docs_);
    int iters = 0;
    check(isle_hip_lloyds_sparse(ctx_, (int)num_centers, centers, centers, assign.data(), max_reps, &iters), "run_lloyds");
    FPTYPE residual = 0.0f;
    if (compute_residual_) residual = print_residuals(ISLE_SPACE_WORD);  // :1714, sqrt of lloyds_iter's residual (:1649-1663)
    else
      for (int i = 0; i < iters; ++i) std::cout << "Lloyd's iter " << i << "  dist_sq residual: " << 0 << "\n";  // :1714 (residual disabled)
    if (iters < max_reps) std::cout << "Lloyds converged\n";
    fill_partition(assign.data(), closest_docs, num_centers);
    return residual;
  }

  // lloyds_iter(..., compute_residual) of the reference (:1649-1663): with the flag set both loops evaluate sum_d |b_d - c_a(d)|^2
  // after every centre update on the device (isle_hip_lloyds_trace), print the reference's residual lines and return the last residual;
  // with the flag clear (the default) they print and return what they always did.
  void set_compute_residual(const bool on) {
    compute_residual_ = on;
    check(isle_hip_lloyds_trace(ctx_, on ? 1 : 0), "set_compute_residual");
  }
  // The objective of the partition and centres the last loop in `space` (ISLE_SPACE_*) left on the device: sums[t] (num_centers
  // doubles, nullable) per cluster, *total their sum.
  void kmeans_objective(const int space, const doc_id_t num_centers, double* sums, double* total, uint64_t* sizes = nullptr) {
    check(isle_hip_kmeans_objective(ctx_, space, (int)num_centers, nullptr, nullptr, sums, sizes, total, nullptr), "kmeans_objective");
  }

  // ---- the stage after the hot path, on the count matrix this object was built from (from_counts) --------------------
  // src/trainer.cpp:577-627: A_sp->rth_highest_element(r, closest_docs[t], ...) for every topic, then
  // A_sp->find_catchwords(num_topics, catchword_thresholds, catchwords).  The partition is the one run_lloyds left on the
  // device (its closest_docs, mapped through original_cols exactly as :572-575 does).
  void find_catchwords(const doc_id_t num_topics, const uint64_t r, FPTYPE* catchword_thresholds /*vocab x topics, col-major*/,
                       std::vector<word_id_t>* catchwords /*[num_topics]*/) {
    std::vector<int32_t> catch_topic(vocab_size_);
    uint64_t n = 0;
    check(isle_hip_catchwords(ctx_, (int)num_topics, nullptr, r, ISLE_RHO_C, catchword_thresholds, catch_topic.data(), &n), "find_catchwords");
    post_topics_ = num_topics;
    for (doc_id_t t = 0; t < num_topics; ++t) catchwords[t].clear();
    for (word_id_t w = 0; w < vocab_size_; ++w)
      if (catch_topic[w] >= 0) catchwords[catch_topic[w]].push_back(w);
  }
  // A_sp->construct_topic_model(Model, num_topics, closest_docs, catchwords, ..., &top_topic_pairs, ...)
  // src/sparseMatrix.cpp:597-838; rank_threshold as at :720.
  void construct_topic_model(FPTYPE* Model /*vocab x topics, col-major*/, const doc_id_t num_topics, const doc_id_t num_docs_A,
                             std::vector<std::tuple<int, int, doc_id_t>>* top_topic_pairs) {
    const uint64_t rank_threshold = (doc_id_t)(ISLE_EPS3_C * ISLE_W0_C * (FPTYPE)num_docs_A / ((FPTYPE)num_topics * 2.0));
    std::vector<int32_t> t1, t2;
    if (top_topic_pairs) {
      t1.resize(num_docs_A);
      t2.resize(num_docs_A);
    }
    check(isle_hip_topic_model(ctx_, (int)num_topics, rank_threshold, Model, nullptr, top_topic_pairs ? t1.data() : nullptr,
                               top_topic_pairs ? t2.data() : nullptr, nullptr),
          "construct_topic_model");
    if (top_topic_pairs) {
      top_topic_pairs->clear();
      for (doc_id_t d = 0; d < num_docs_A; ++d)
        if (t1[d] >= 0 && t2[d] >= 0) top_topic_pairs->push_back(std::make_tuple((int)t1[d], (int)t2[d], d));
    }
  }
  // SparseMatrix::topic_coherence (src/sparseMatrix.cpp:841-870) on the count matrix this object was built from: the first M words of
  // each top_words[t] (heaviest first), coherences[t] = the UMass sum of include/isle_hip.h (isle_hip_topic_coherence), NaN where a
  // word in a denominator occurs in no document.  The reference's model argument only fed an assert and is dropped; coherences are
  // double here (the reference accumulates in float, racing on coherences[topic]).
  void topic_coherence(const doc_id_t num_topics, const word_id_t& M, const std::vector<std::pair<word_id_t, FPTYPE>>* top_words,
                       std::vector<double>& coherences, const double coherence_eps = ISLE_DEFAULT_COHERENCE_EPS) {
    std::vector<uint32_t> tw((size_t)num_topics * M);
    for (doc_id_t t = 0; t < num_topics; ++t) {
      if (top_words[t].size() < M) throw std::runtime_error("topic_coherence: topic " + std::to_string(t) + " has fewer than M top words");
      for (word_id_t i = 0; i < M; ++i) tw[(size_t)t * M + i] = (uint32_t)top_words[t][i].first;
    }
    coherences.assign(num_topics, 0.0);
    check(isle_hip_topic_coherence(ctx_, (int)num_topics, (int)M, tw.data(), coherence_eps, coherences.data(), nullptr, nullptr), "topic_coherence");
  }
  // The cluster-average topic model (src/trainer.cpp:712-716: construct_topic_model with no catchwords) on the partition and the
  // normalised values of the last construct_topic_model: exact sums, bitwise reproducible, NaN for an empty cluster
  // (isle_hip_avg_topic_model).  It stays on the device; AvgModel (nullable): vocab x num_topics, column-major.
  void construct_avg_topic_model(FPTYPE* AvgModel, const doc_id_t num_topics) {
    check(isle_hip_avg_topic_model(ctx_, (int)num_topics, AvgModel), "avg_topic_model");
  }
  // The n heaviest words of every topic of a resident model (ISLE_MODEL_CATCH, ISLE_MODEL_AVG or ISLE_MODEL_LOADED), by the trainer's rule (heaviest
  // first, lower id first among equal weights, NaN last), selected on the device (isle_hip_model_top_words).
  void model_top_words(const int which, const doc_id_t num_topics, const word_id_t n, std::vector<std::pair<word_id_t, FPTYPE>>* top_words) {
    std::vector<uint32_t> ids((size_t)num_topics * n);
    std::vector<float> w((size_t)num_topics * n);
    check(isle_hip_model_top_words(ctx_, which, nullptr, model_vocab(which), (int)num_topics, (int)n, ids.data(), w.data()), "model_top_words");
    for (doc_id_t t = 0; t < num_topics; ++t) {
      top_words[t].clear();
      for (word_id_t i = 0; i < n; ++i) top_words[t].push_back(std::make_pair((word_id_t)ids[(size_t)t * n + i], w[(size_t)t * n + i]));
    }
  }
  // Topic diversity of a resident model in double (isle_hip_topic_diversity): dist[t] = squared L2 distance of topic t to the mean
  // topic of the finite topics (NaN for the others), avg = their mean.
  void topic_diversity(const int which, const doc_id_t num_topics, std::vector<double>& dist, double& avg) {
    dist.assign(num_topics, 0.0);
    check(isle_hip_topic_diversity(ctx_, which, (int)num_topics, dist.data(), &avg), "topic_diversity");
  }
  // Topic weights of documents [doc_begin, doc_end) of the count matrix this object was built from, under a resident model
  // (ISLE_MODEL_CATCH / ISLE_MODEL_AVG) or, with ISLE_MODEL_HOST, under model_host (vocab x ncols column-major): ISLEInfer's iterations
  // (src/infer.cpp:361-492) on the device-resident data (isle_hip_infer_resident).  For every converged document the topics with
  // weight > min_weight (negative: 1 / topics), ascending: doc_offsets (range + 1), topic, weight.  Returns the converged documents.
  uint64_t infer_documents(const int which, const doc_id_t doc_begin, const doc_id_t doc_end, const int iters, const FPTYPE Lf,
                           std::vector<int64_t>& doc_offsets, std::vector<uint32_t>& topic, std::vector<FPTYPE>& weight,
                           const FPTYPE min_weight = -1.0f, const FPTYPE* model_host = nullptr, const doc_id_t ncols = 0,
                           const uint64_t chunk_docs = 0) {
    uint64_t n = 0;
    const uint64_t nconv = infer_documents_resident(which, doc_begin, doc_end, iters, Lf, min_weight, model_host, ncols, chunk_docs, &n);
    doc_offsets.assign((size_t)(doc_end - doc_begin) + 1, 0);
    topic.assign(n, 0);
    weight.assign(n, 0.0f);
    check(isle_hip_get_infer_entries(ctx_, doc_offsets.data(), topic.data(), weight.data()), "get_infer_entries");
    return nconv;
  }
  // The same inference with the entries (and the five heaviest topics of every document) left on the device, where write_infer_text
  // formats them.  Returns the converged documents; nentries (nullable): the entries.
  uint64_t infer_documents_resident(const int which, const doc_id_t doc_begin, const doc_id_t doc_end, const int iters, const FPTYPE Lf,
                                    const FPTYPE min_weight = -1.0f, const FPTYPE* model_host = nullptr, const doc_id_t ncols = 0,
                                    const uint64_t chunk_docs = 0, uint64_t* nentries = nullptr) {
    uint64_t nconv = 0;
    const bool host = which == ISLE_MODEL_HOST;
    check(isle_hip_infer_resident(ctx_, which, model_host, vocab_size_, (int)(host ? ncols : model_cols(which)), doc_begin, doc_end, iters, Lf,
                                  min_weight, chunk_docs, nullptr, nullptr, nullptr, &nconv, nentries), "infer_documents");
    return nconv;
  }
  // The lines "<row + number_base>\t<topic + 1>\t<weight>\n" of rows [row_begin, row_end) of the last inference (row 0 = its doc_begin),
  // formatted on the device (isle_hip_infer_text) and streamed to the file: what = ISLE_DOCTEXT_ENTRIES (every entry; DocTopicWeights.tsv)
  // or ISLE_DOCTEXT_TOP (the at most five heaviest topics; ISLEInfer's top_topics_* files).  Returns the bytes written; nlines nullable.
  uint64_t write_infer_text(const std::string& filename, const int what, const doc_id_t row_begin, const doc_id_t row_end,
                            const uint64_t number_base, uint64_t* nlines = nullptr) {
    FILE* fp = std::fopen(filename.c_str(), "wb");
    if (!fp) throw std::runtime_error("cannot open " + filename);
    uint64_t nbytes = 0;
    const int rc = isle_hip_infer_text(ctx_, what, row_begin, row_end, number_base, text_to_file, fp, &nbytes, nlines);
    std::fclose(fp);
    check(rc, "write_infer_text");
    return nbytes;
  }
  uint64_t infer_text_size(const int what, const doc_id_t row_begin, const doc_id_t row_end, const uint64_t number_base, uint64_t* nlines = nullptr) {
    uint64_t nbytes = 0;
    check(isle_hip_infer_text(ctx_, what, row_begin, row_end, number_base, nullptr, nullptr, &nbytes, nlines), "infer_text_size");
    return nbytes;
  }
  // A per-document report file of the trainer for every document of A, formatted on the device from what find_catchwords /
  // construct_topic_model left resident (isle_hip_doc_report_text) and streamed to the file: what = ISLE_DOCREPORT_CATCHWORDS
  // (DocCatchword.tsv), ISLE_DOCREPORT_TOPIC_SUMS (DocTopicCatchwordSums.tsv; _BY_DOC: the same lines in resident order) or
  // ISLE_DOCREPORT_TOP_TWO (TopTwoTopicsPerDoc.txt).  Returns the bytes written; nlines nullable.
  uint64_t write_doc_report(const std::string& filename, const int what, uint64_t* nlines = nullptr) {
    FILE* fp = std::fopen(filename.c_str(), "wb");
    if (!fp) throw std::runtime_error("cannot open " + filename);
    uint64_t nbytes = 0;
    const int rc = isle_hip_doc_report_text(ctx_, what, 0, a_docs_, text_to_file, fp, &nbytes, nlines);
    std::fclose(fp);
    check(rc, "write_doc_report");
    return nbytes;
  }
  // What those files print, fetched: the count matrix A (CSC over its documents) with the corpus' avg_doc_sz, and the (document, topic)
  // catchword sums of the last construct_topic_model as CSR over A's documents.  For the host statements of the files
  // (trainer_detail::doc_catchword_text / doc_topic_sums_text / top_two_text) and their yardstick isle_amd/host/doc_report_main.cpp.
  void get_count_matrix(std::vector<FPTYPE>& counts, std::vector<uint32_t>& rows, std::vector<int64_t>& offs, float* avg_doc_sz) {
    offs.assign((size_t)a_docs_ + 1, 0);
    check(isle_hip_get_A(ctx_, nullptr, nullptr, offs.data()), "get_A");
    counts.assign((size_t)offs[a_docs_], 0.0f);
    rows.assign((size_t)offs[a_docs_], 0);
    check(isle_hip_get_A(ctx_, counts.data(), rows.data(), nullptr), "get_A");
    if (avg_doc_sz) check(isle_hip_avg_doc_sz(ctx_, avg_doc_sz), "avg_doc_sz");
  }
  // The vocabulary of the count matrix A pruned by document frequency on the device (isle_hip_prune_vocab; the rule:
  // isle_amd/csrc/vocab_host.h): words in fewer than min_df or more than max_df (0: no upper bound) documents go, of the rest the keep_n
  // (0: no cap) most frequent stay; kept_words[new id] = old id.  For everything resident an ingest of the pruned A: B is the old A's until
  // threshold_again.  A refusal throws and leaves A as it was.  df (the old vocabulary), entries (A's afterwards), emptied: nullable.
  void prune_vocabulary(const uint64_t min_df, const uint64_t max_df, const uint64_t keep_n, std::vector<uint32_t>& kept_words,
                        std::vector<uint32_t>* df = nullptr, uint64_t* entries = nullptr, uint64_t* emptied = nullptr) {
    uint64_t new_vocab = 0;
    kept_words.assign((size_t)vocab_size_, 0);
    if (df) df->assign((size_t)vocab_size_, 0);
    check(isle_hip_prune_vocab(ctx_, min_df, max_df, keep_n, &new_vocab, kept_words.data(), df ? df->data() : nullptr, entries, emptied), "prune_vocab");
    kept_words.resize((size_t)new_vocab);
    vocab_size_ = (word_id_t)new_vocab;
    top5_ready_ = false;
  }
  // The documents of the count matrix A pruned by length and as exact duplicates on the device (isle_hip_prune_docs; the rule:
  // isle_amd/csrc/docs_host.h): documents of fewer than min_words or more than max_words entries, of fewer than min_tokens or more than
  // max_tokens tokens go (a maximum of 0: no bound), and with drop_duplicates every document whose column equals an earlier one's bit for
  // bit; kept_docs[new id] = old id.  For everything resident an ingest of the pruned A: B is the old A's until threshold_again.  A
  // refusal throws and leaves A as it was.  first_of (the old documents), entries (A's afterwards), dropped[3]: nullable.
  void prune_documents(const uint64_t min_words, const uint64_t max_words, const uint64_t min_tokens, const uint64_t max_tokens, const bool drop_duplicates,
                       std::vector<uint32_t>& kept_docs, std::vector<uint32_t>* first_of = nullptr, uint64_t* entries = nullptr, uint64_t* dropped = nullptr) {
    uint64_t new_docs = 0;
    kept_docs.assign(std::max<size_t>((size_t)a_docs_, 1), 0);
    if (first_of) first_of->assign(std::max<size_t>((size_t)a_docs_, 1), 0);
    check(isle_hip_prune_docs(ctx_, min_words, max_words, min_tokens, max_tokens, drop_duplicates ? 1 : 0, &new_docs, kept_docs.data(),
                              first_of ? first_of->data() : nullptr, entries, nullptr, dropped),
          "prune_docs");
    kept_docs.resize((size_t)new_docs);
    if (first_of) first_of->resize((size_t)a_docs_);
    a_docs_ = (doc_id_t)new_docs;
    top5_ready_ = false;
  }
  // which key the near-duplicate calls sort a band's documents by: ISLE_NEARDUP_KEY_AUTO / _FULL / _NARROW (isle_hip_neardup_key_form)
  void neardup_key_form(const int form) { check(isle_hip_neardup_key_form(ctx_, form), "neardup_key_form"); }
  // MinHash signatures (docs x bands rows_per_band, row-major) and band keys (bands x docs, band-major) of A's documents; each nullable
  void doc_signatures(const int bands, const int rows_per_band, std::vector<uint64_t>* sig, std::vector<uint64_t>* keys) {
    if (sig) sig->assign(std::max<size_t>((size_t)a_docs_ * bands * rows_per_band, 1), 0);
    if (keys) keys->assign(std::max<size_t>((size_t)a_docs_ * bands, 1), 0);
    check(isle_hip_doc_signatures(ctx_, bands, rows_per_band, sig ? sig->data() : nullptr, keys ? keys->data() : nullptr), "doc_signatures");
    if (sig) sig->resize((size_t)a_docs_ * bands * rows_per_band);
    if (keys) keys->resize((size_t)a_docs_ * bands);
  }
  // the exact sizes of the intersection and the union of the word sets of A's documents a[i] and b[i]
  void doc_jaccard(const std::vector<uint32_t>& a, const std::vector<uint32_t>& b, std::vector<uint32_t>& inter, std::vector<uint32_t>& uni) {
    if (a.size() != b.size()) throw std::runtime_error("doc_jaccard: the two lists differ in length");
    inter.assign(std::max<size_t>(a.size(), 1), 0);
    uni.assign(std::max<size_t>(a.size(), 1), 0);
    check(isle_hip_doc_jaccard(ctx_, a.size(), a.data(), b.data(), inter.data(), uni.data()), "doc_jaccard");
    inter.resize(a.size());
    uni.resize(a.size());
  }
  // The near duplicates among the documents of the count matrix A, by MinHash banding and an exact Jaccard test on the device
  // (isle_hip_doc_near_duplicates; the rule: isle_amd/csrc/neardup_host.h): parent[d] the verified earlier neighbour (d where it has
  // none), first_of[d] the root of the parent chain.  Nothing resident changes.  -> the documents that are not their own root.
  uint64_t near_duplicates(const uint64_t num, const uint64_t den, const int bands, const int rows_per_band, std::vector<uint32_t>& parent,
                           std::vector<uint32_t>& first_of, uint64_t* pairs_tested = nullptr, uint64_t* rounds = nullptr) {
    uint64_t dropped = 0;
    parent.assign(std::max<size_t>((size_t)a_docs_, 1), 0);
    first_of.assign(std::max<size_t>((size_t)a_docs_, 1), 0);
    check(isle_hip_doc_near_duplicates(ctx_, num, den, bands, rows_per_band, parent.data(), first_of.data(), &dropped, pairs_tested, rounds), "doc_near_duplicates");
    parent.resize((size_t)a_docs_);
    first_of.resize((size_t)a_docs_);
    return dropped;
  }
  // ... and pruned (isle_hip_prune_near_docs): every document that is not its own root goes; kept_docs[new id] = old id.  For everything
  // resident an ingest of the pruned A: B is the old A's until threshold_again.  A refusal throws and leaves A as it was.  parent and
  // first_of are the old documents'; inter and uni (nullable) the exact sizes of every old document with its parent, taken before the prune.
  void prune_near_duplicates(const uint64_t num, const uint64_t den, const int bands, const int rows_per_band, std::vector<uint32_t>& kept_docs,
                             std::vector<uint32_t>& parent, std::vector<uint32_t>& first_of, std::vector<uint32_t>* inter = nullptr,
                             std::vector<uint32_t>* uni = nullptr, uint64_t* entries = nullptr) {
    const size_t old_docs = (size_t)a_docs_;
    if (inter || uni) {
      near_duplicates(num, den, bands, rows_per_band, parent, first_of);
      std::vector<uint32_t> self(old_docs), in(std::max<size_t>(old_docs, 1)), un(std::max<size_t>(old_docs, 1));
      for (size_t d = 0; d < old_docs; ++d) self[d] = (uint32_t)d;
      check(isle_hip_doc_jaccard(ctx_, old_docs, self.data(), parent.data(), in.data(), un.data()), "doc_jaccard");
      in.resize(old_docs), un.resize(old_docs);
      if (inter) inter->swap(in);
      if (uni) uni->swap(un);
    }
    uint64_t new_docs = 0;
    kept_docs.assign(std::max<size_t>(old_docs, 1), 0);
    parent.assign(std::max<size_t>(old_docs, 1), 0);
    first_of.assign(std::max<size_t>(old_docs, 1), 0);
    check(isle_hip_prune_near_docs(ctx_, num, den, bands, rows_per_band, &new_docs, kept_docs.data(), parent.data(), first_of.data(), entries, nullptr, nullptr),
          "prune_near_docs");
    kept_docs.resize((size_t)new_docs);
    parent.resize(old_docs);
    first_of.resize(old_docs);
    a_docs_ = (doc_id_t)new_docs;
    top5_ready_ = false;
  }
  void doc_lengths(std::vector<uint32_t>& words, std::vector<uint64_t>& tokens) {
    words.assign(std::max<size_t>((size_t)a_docs_, 1), 0);
    tokens.assign(std::max<size_t>((size_t)a_docs_, 1), 0);
    check(isle_hip_doc_lengths(ctx_, words.data(), tokens.data()), "doc_lengths");
    words.resize((size_t)a_docs_);
    tokens.resize((size_t)a_docs_);
  }
  std::vector<uint32_t> word_doc_freq() {
    std::vector<uint32_t> df((size_t)vocab_size_, 0);
    check(isle_hip_word_doc_freq(ctx_, df.data()), "word_doc_freq");
    return df;
  }
  // B again from the resident A, with from_counts' outputs: what follows a prune_vocabulary
  void threshold_again(doc_id_t num_topics, double sample_rate, std::vector<doc_id_t>& original_cols, uint64_t* entries_above_threshold = nullptr,
                       float* avg_doc_sz = nullptr) {
    threshold_on_device(num_topics, sample_rate, original_cols, nullptr, entries_above_threshold, avg_doc_sz);
  }
  void get_doc_topic_sums(std::vector<int64_t>& offs, std::vector<uint32_t>& topic, std::vector<FPTYPE>& val) {
    offs.assign((size_t)a_docs_ + 1, 0);
    check(isle_hip_get_doc_topic_sums(ctx_, offs.data(), nullptr, nullptr), "get_doc_topic_sums");
    topic.assign((size_t)offs[a_docs_], 0);
    val.assign((size_t)offs[a_docs_], 0.0f);
    check(isle_hip_get_doc_topic_sums(ctx_, nullptr, topic.data(), val.data()), "get_doc_topic_sums");
  }
  // The n heaviest documents of every topic, selected on the device (isle_hip_topic_top_docs; the rule: isle_amd/csrc/topdocs_host.h) from
  // a resident source, ISLE_TOPDOCS_SUMS (the catchword sums of the last construct_topic_model) or ISLE_TOPDOCS_INFER (the entries of the
  // last infer_documents_resident; doc_base = its doc_begin): docs / values num_topics x n topic-major, the unused slots 0xffffffff / 0.0f;
  // counts[t] = min(n, the topic's entries); entries (nullable): the topics' entry counts.
  void topic_top_docs(const int source, const doc_id_t num_topics, const int n, const uint64_t doc_base, std::vector<uint32_t>& docs,
                      std::vector<FPTYPE>& values, std::vector<uint32_t>& counts, std::vector<uint64_t>* entries = nullptr) {
    docs.assign((size_t)num_topics * n, 0);
    values.assign((size_t)num_topics * n, 0.0f);
    counts.assign((size_t)num_topics, 0);
    if (entries) entries->assign((size_t)num_topics, 0);
    check(isle_hip_topic_top_docs(ctx_, source, (int)num_topics, n, doc_base, 0, nullptr, nullptr, nullptr, docs.data(), values.data(), counts.data(),
                                  entries ? entries->data() : nullptr), "topic_top_docs");
  }
  // The n documents most similar to each query row of a resident source, scored and selected on the device (isle_hip_similar_docs; the
  // rule: isle_amd/csrc/simdocs_host.h): source ISLE_TOPDOCS_SUMS or ISLE_TOPDOCS_INFER as topic_top_docs, measure ISLE_SIM_*, the queries
  // rows query_rows of the source (a query's own document is not its neighbour).  docs / scores query_rows.size() x n query-major, the
  // unused slots 0xffffffff / 0.0f; counts[q] = min(n, the query's candidates); candidates (nullable): the candidate counts.
  void similar_documents(const int source, const int measure, const doc_id_t num_topics, const int n, const uint64_t doc_base,
                         const std::vector<uint64_t>& query_rows, std::vector<uint32_t>& docs, std::vector<FPTYPE>& scores, std::vector<uint32_t>& counts,
                         std::vector<uint64_t>* candidates = nullptr) {
    const size_t Q = query_rows.size();
    docs.assign(Q * (size_t)n, 0);
    scores.assign(Q * (size_t)n, 0.0f);
    counts.assign(Q, 0);
    if (candidates) candidates->assign(Q, 0);
    check(isle_hip_similar_docs(ctx_, source, measure, (int)num_topics, n, doc_base, 0, nullptr, nullptr, nullptr, (int)Q, query_rows.data(), nullptr, nullptr,
                                nullptr, nullptr, docs.data(), scores.data(), counts.data(), candidates ? candidates->data() : nullptr), "similar_docs");
  }
  // Topic prevalence by group of documents, summed on the device (isle_hip_topic_prevalence; the rule: isle_amd/csrc/prevalence_host.h)
  // from a resident source, ISLE_TOPDOCS_SUMS or ISLE_TOPDOCS_INFER as topic_top_docs.  groups: one label per row of the source
  // (ISLE_GROUP_NONE: no group), or empty: every row has label 0 and num_groups is 1.  docs (num_groups); count, dominant, sum (num_groups x
  // num_topics group-major); the sums are added in the rule's order: the same bits on every call.  -> the rows of no group.
  struct TopicPrevalence {
    std::vector<uint64_t> docs, count, dominant;
    std::vector<double> sum;
    uint64_t unlabelled = 0;
  };
  TopicPrevalence topic_prevalence(const int source, const doc_id_t num_topics, const std::vector<uint32_t>& groups, const uint32_t num_groups,
                                   const bool normalise) {
    TopicPrevalence p;
    if (source == ISLE_TOPDOCS_SUMS && !groups.empty() && groups.size() != (size_t)a_docs_)  // (the library reads one label per row)
      throw std::runtime_error("topic_prevalence: " + std::to_string(groups.size()) + " labels for " + std::to_string((size_t)a_docs_) + " documents");
    const size_t cells = (size_t)num_groups * (size_t)num_topics;
    p.docs.assign(num_groups, 0);
    p.count.assign(cells, 0);
    p.dominant.assign(cells, 0);
    p.sum.assign(cells, 0.0);
    check(isle_hip_topic_prevalence(ctx_, source, (int)num_topics, 0, nullptr, nullptr, nullptr, groups.empty() ? nullptr : groups.data(), num_groups,
                                    normalise ? 1 : 0, p.docs.data(), &p.unlabelled, p.count.data(), p.dominant.data(), p.sum.data()), "topic_prevalence");
    return p;
  }
  // Held-out scores per document on the device (isle_hip_score_docs; the rule: isle_amd/csrc/score_host.h) with the weights of the last
  // infer_documents_resident (ISLE_TOPDOCS_INFER; doc_begin = its doc_begin, num_rows = its documents) under the model `which` (model_host
  // and ncols with ISLE_MODEL_HOST only).  held == nullptr: the entries are those documents of the resident count matrix; else the caller's
  // CSC (counts, rows, offsets of num_rows documents), e.g. the held-out part of every document.  measure ISLE_SCORE_LOG / _PROB; floor > 0:
  // an entry with z < floor is scored at floor.  Per document score, tokens, unscored_entries, unscored_tokens, floored; the totals are
  // isle_hip_score_total's ascending sums, perplexity = exp(-total_score / total_tokens) (ISLE_SCORE_LOG).  Nothing resident changes.
  struct HeldEntries {
    const FPTYPE* counts;
    const uint32_t* rows;
    const int64_t* offsets;
  };
  struct DocScores {
    std::vector<double> score, tokens, unscored_tokens;
    std::vector<uint32_t> unscored_entries, floored;
    double total_score = 0.0, total_tokens = 0.0, perplexity = 0.0;
  };
  DocScores score_documents(const int which, const doc_id_t doc_begin, const doc_id_t num_rows, const int measure, const bool normalise, const double floor,
                            const HeldEntries* held = nullptr, const FPTYPE* model_host = nullptr, const doc_id_t ncols = 0) {
    DocScores s;
    const size_t n = (size_t)num_rows;
    s.score.assign(n, 0.0), s.tokens.assign(n, 0.0), s.unscored_tokens.assign(n, 0.0);
    s.unscored_entries.assign(n, 0), s.floored.assign(n, 0);
    const bool host = which == ISLE_MODEL_HOST;
    check(isle_hip_score_docs(ctx_, which, model_host, model_vocab(which), (int)(host ? ncols : model_cols(which)), ISLE_TOPDOCS_INFER, num_rows, nullptr,
                              nullptr, nullptr, held ? ISLE_SCORE_HOST : ISLE_SCORE_RESIDENT, doc_begin, held ? held->counts : nullptr,
                              held ? held->rows : nullptr, held ? held->offsets : nullptr, measure, normalise ? 1 : 0, floor, s.score.data(), s.tokens.data(),
                              s.unscored_entries.data(), s.unscored_tokens.data(), s.floored.data(), nullptr), "score_docs");
    isle_hip_score_total(s.score.data(), n, &s.total_score);
    isle_hip_score_total(s.tokens.data(), n, &s.total_tokens);
    s.perplexity = std::exp(-s.total_score / s.total_tokens);
    return s;
  }
  // Two models compared on the device (isle_hip_compare_models; the rule: isle_amd/csrc/match_host.h): dist (cols_a x cols_b row-major) =
  // the L1 distances of their topics in double, and the greedy matching of the topics by it: match_a[i] = the matched topic of b or -1,
  // match_b the inverse, match_dist[i] = the matched distance or NaN, mean_dist over the n_matched pairs.  A side is a resident model
  // (ISLE_MODEL_CATCH / ISLE_MODEL_AVG / ISLE_MODEL_LOADED; host null, cols ignored) or, with ISLE_MODEL_HOST, host (vocab x cols
  // column-major); vocab is read from a resident side.  dist is nullable.  -> the rounds of the matcher.
  struct TopicMatch {
    std::vector<int32_t> match_a, match_b;
    std::vector<double> match_dist;
    uint64_t n_matched = 0;
    double mean_dist = 0.0;
    uint32_t rounds = 0;
  };
  TopicMatch compare_models(const int which_a, const int which_b, std::vector<double>* dist = nullptr, const FPTYPE* a_host = nullptr, const doc_id_t cols_a = 0,
                            const FPTYPE* b_host = nullptr, const doc_id_t cols_b = 0, const word_id_t vocab = 0) {
    const doc_id_t ka = which_a == ISLE_MODEL_HOST ? cols_a : model_cols(which_a), kb = which_b == ISLE_MODEL_HOST ? cols_b : model_cols(which_b);
    const word_id_t V = which_a != ISLE_MODEL_HOST ? model_vocab(which_a) : which_b != ISLE_MODEL_HOST ? model_vocab(which_b) : vocab;
    TopicMatch m;
    m.match_a.assign(std::max<size_t>((size_t)ka, 1), -1);
    m.match_b.assign(std::max<size_t>((size_t)kb, 1), -1);
    m.match_dist.assign(std::max<size_t>((size_t)ka, 1), 0.0);
    if (dist) dist->assign(std::max<size_t>((size_t)ka * kb, 1), 0.0);
    check(isle_hip_compare_models(ctx_, which_a, a_host, (int)ka, which_b, b_host, (int)kb, V, dist ? dist->data() : nullptr, m.match_a.data(), m.match_b.data(),
                                  m.match_dist.data(), &m.n_matched, &m.mean_dist, &m.rounds),
          "compare_models");
    m.match_a.resize((size_t)ka);
    m.match_b.resize((size_t)kb);
    m.match_dist.resize((size_t)ka);
    if (dist) dist->resize((size_t)ka * kb);
    return m;
  }
  // The same matcher on the caller's na x nb row-major matrix (isle_hip_match_topics)
  TopicMatch match_topics(const std::vector<double>& dist, const int na, const int nb) {
    TopicMatch m;
    m.match_a.assign((size_t)std::max(na, 1), -1);
    m.match_b.assign((size_t)std::max(nb, 1), -1);
    m.match_dist.assign((size_t)std::max(na, 1), 0.0);
    check(isle_hip_match_topics(ctx_, dist.empty() ? nullptr : dist.data(), na, nb, m.match_a.data(), m.match_b.data(), m.match_dist.data(), &m.n_matched, &m.mean_dist,
                                &m.rounds),
          "match_topics");
    m.match_a.resize((size_t)std::max(na, 0));
    m.match_b.resize((size_t)std::max(nb, 0));
    m.match_dist.resize((size_t)std::max(na, 0));
    return m;
  }
  void model_dist_slices(const int slices) { check(isle_hip_model_dist_slices(ctx_, slices), "model_dist_slices"); }
  doc_id_t count_docs() const { return a_docs_; }  // documents of the count matrix A (B may hold fewer after sampling)
  // DenseMatrix::write_to_file_as_sparse (format = ISLE_TEXT_SPARSE) / write_to_file (ISLE_TEXT_DENSE), src/denseMatrix.cpp:124-186, of a
  // resident model (ISLE_MODEL_CATCH / ISLE_MODEL_AVG), or with ISLE_MODEL_HOST of model_host (vocab x ncols column-major): the text is
  // formatted on the device (isle_hip_model_text) and its pieces go straight to the file.  Returns the bytes written.
  uint64_t write_model_text(const int which, const int format, const std::string& filename, const FPTYPE* model_host = nullptr,
                            const word_id_t vocab = 0, const doc_id_t ncols = 0) {
    FILE* fp = std::fopen(filename.c_str(), "wb");
    if (!fp) throw std::runtime_error("cannot open " + filename);
    uint64_t nbytes = 0;
    const bool host = which == ISLE_MODEL_HOST;
    const int rc = isle_hip_model_text(ctx_, which, model_host, host ? vocab : model_vocab(which), (int)(host ? ncols : model_cols(which)), format, text_to_file,
                                       fp, &nbytes, nullptr);
    std::fclose(fp);
    check(rc, "write_model_text");
    return nbytes;
  }
  // The inverse: a model file (ISLE_TEXT_SPARSE: "<topic> <word> <weight>" lines, ids minus `base`; ISLE_TEXT_DENSE: one line per column)
  // read into the resident model ISLE_MODEL_LOADED, parsed on the device (isle_hip_load_model_text; model_read.h states the rule).  It
  // does not depend on the matrices of this object; model_top_words, topic_diversity, infer_documents and write_model_text take it as
  // `which`.  Returns the entries read (SPARSE: lines, DENSE: vocab x ncols).  A refused file leaves the previous model in place.
  uint64_t load_model_file(const std::string& filename, const word_id_t vocab, const doc_id_t ncols, const int format, const unsigned base = 1) {
    const std::vector<char> text = model_read::read_file(filename);
    uint64_t n = 0;
    check(isle_hip_load_model_text(ctx_, text.data(), text.size(), vocab, (int)ncols, format, base, &n), "load_model_file");
    loaded_vocab_ = vocab;
    loaded_cols_ = ncols;
    return n;
  }
  void get_loaded_model(std::vector<FPTYPE>& model) {  // vocab x ncols, column-major
    model.assign((size_t)loaded_vocab_ * loaded_cols_, 0.0f);
    check(isle_hip_get_loaded_model(ctx_, model.data(), nullptr, nullptr), "get_loaded_model");
  }
  // ISLETrainer::write_edgemodel_to_file (src/trainer.cpp:687-693) for the edge topics of `pairs` (primary, secondary per edge topic):
  // the FPaxpy pair of construct_edge_topics and the sparse text in one pass on the device (isle_hip_edge_topics_text).
  uint64_t write_edge_model_text(const std::vector<int64_t>& pairs, const FPTYPE primary_ratio, const std::string& filename) {
    FILE* fp = std::fopen(filename.c_str(), "wb");
    if (!fp) throw std::runtime_error("cannot open " + filename);
    uint64_t nbytes = 0;
    const int rc = isle_hip_edge_topics_text(ctx_, pairs.data(), (int)(pairs.size() / 2), primary_ratio, ISLE_TEXT_SPARSE, text_to_file, fp, &nbytes,
                                             nullptr);
    std::fclose(fp);
    check(rc, "write_edge_model_text");
    return nbytes;
  }
  // SparseMatrix::compute_log_combinatorial (src/sparseMatrix.cpp:1018-1043) on the count matrix this object was built from: every
  // document's log(N_d! / prod count!) with the reference's fp32 table and order (isle_hip_log_combinatorial), bit for bit.
  void compute_log_combinatorial(std::vector<FPTYPE>& docs_log_fact) {
    if (!docs_log_fact.empty()) throw std::runtime_error("compute_log_combinatorial: docs_log_fact must be empty");  // :1036
    docs_log_fact.resize(a_docs_);
    if (a_docs_) check(isle_hip_log_combinatorial(ctx_, docs_log_fact.data(), nullptr), "compute_log_combinatorial");
  }
  // SparseMatrix::count_distint_top_five_words (src/sparseMatrix.cpp:170-215; the reference's spelling): the device sorts the documents'
  // top-five tuples once, the run lengths stay here, and every call evaluates the counting loop for its min_distinct on them
  // (isle_hip_top_five_count_rule).  Prints "top five vec size: " as the reference does on every call.
  size_t count_distint_top_five_words(int min_distinct) {
    if (min_distinct < 2) throw std::runtime_error("count_distint_top_five_words: min_distinct < 2");  // :172
    if (!top5_ready_) {
      top5_runs_.assign(std::max<doc_id_t>(a_docs_, 1), 0);
      uint64_t nr = 0;
      check(isle_hip_distinct_top_five(ctx_, 0, nullptr, nullptr, &top5_n_, nullptr, top5_runs_.data(), &nr), "count_distint_top_five_words");
      top5_runs_.resize(nr);
      top5_ready_ = true;
    }
    std::cout << "top five vec size: " << top5_n_ << std::endl;
    uint64_t num = 0;
    check(isle_hip_top_five_count_rule(top5_runs_.data(), top5_runs_.size(), min_distinct, &num), "top_five_count_rule");
    return (size_t)num;
  }
  // ISLETrainer::construct_edge_topics_v2's selection (src/trainer.cpp:1116-1148), on the device over the resident top-two topics of the
  // last construct_topic_model (isle_hip_select_edge_pairs; nothing is fetched).  host_pairs non-null: the host rule on those pairs
  // instead (fpsparse_detail::select_edge_pairs_host) — the path for more than ISLE_EDGE_TABLE_MAX_TOPICS topics.  Ties in the count
  // ordering are broken by (primary, secondary) ascending (the reference's sort is unstable).  The edge model itself is not formed
  // here: edge_model(), write_edge_model_text() and edge_top_words() form its entries from the resident model when they are asked.
  void construct_edge_topics(const std::vector<std::tuple<int, int, doc_id_t>>* host_pairs, const int max_edge_topics,
                             std::vector<std::tuple<int, int, uint64_t>>& selected_pairs) {
    uint64_t candidates = 0, threshold = 0;
    if (host_pairs) {
      std::vector<int32_t> t1(host_pairs->size()), t2(host_pairs->size());
      for (size_t i = 0; i < host_pairs->size(); ++i) {
        t1[i] = (int32_t)std::get<0>((*host_pairs)[i]);
        t2[i] = (int32_t)std::get<1>((*host_pairs)[i]);
      }
      fpsparse_detail::select_edge_pairs_host(t1.data(), t2.data(), t1.size(), max_edge_topics, ISLE_EDGE_TOPIC_MIN_DOCS, selected_pairs, &candidates,
                                              &threshold);
    } else {
      const uint64_t k = post_topics_;
      const uint64_t cap = std::min<uint64_t>(std::min<uint64_t>((uint64_t)std::max(max_edge_topics, 0), k * k), a_docs_);
      std::vector<int64_t> triples(3 * cap + 1);
      uint64_t n = 0;
      check(isle_hip_select_edge_pairs(ctx_, nullptr, nullptr, a_docs_, (int)k, max_edge_topics, ISLE_EDGE_TOPIC_MIN_DOCS, triples.data(), cap, &n, &candidates,
                                       &threshold),
            "construct_edge_topics");
      selected_pairs.clear();
      for (uint64_t e = 0; e < n; ++e) selected_pairs.push_back(std::make_tuple((int)triples[3 * e], (int)triples[3 * e + 1], (uint64_t)triples[3 * e + 2]));
    }
    std::cout << "#Candidates for edge topics: " << candidates << std::endl;
    if (candidates > selected_pairs.size()) std::cout << "Edge topic threshold: " << threshold << std::endl;
    std::cout << "#Edge topics: " << selected_pairs.size() << std::endl;
    std::cout << "Completed edge topic construction" << std::endl;
  }
  static std::vector<int64_t> pair_ids(const std::vector<std::tuple<int, int, uint64_t>>& selected_pairs) {  // (primary, secondary) per edge topic
    std::vector<int64_t> pq(2 * selected_pairs.size());
    for (size_t e = 0; e < selected_pairs.size(); ++e) {
      pq[2 * e] = std::get<0>(selected_pairs[e]);
      pq[2 * e + 1] = std::get<1>(selected_pairs[e]);
    }
    return pq;
  }
  // The FPaxpy pair of construct_edge_topics_v2 (:1150-1160) on the device (isle_hip_edge_topics): EdgeModel = vocab x #edge, column-major.
  void edge_model(const std::vector<std::tuple<int, int, uint64_t>>& selected_pairs, std::vector<FPTYPE>& EdgeModel) {
    const std::vector<int64_t> pq = pair_ids(selected_pairs);
    EdgeModel.assign((size_t)vocab_size_ * selected_pairs.size(), 0.f);
    check(isle_hip_edge_topics(ctx_, pq.data(), (int)selected_pairs.size(), (float)ISLE_EDGE_TOPIC_PRIMARY_RATIO, EdgeModel.data()), "edge_model");
  }
  // The n heaviest words of every edge topic (DenseMatrix::find_n_top_words on EdgeModel, :1221), selected on the device from the two
  // columns of the resident catch model without storing the edge model (isle_hip_edge_top_words): entries bit-equal to edge_model()'s.
  void edge_top_words(const std::vector<std::tuple<int, int, uint64_t>>& selected_pairs, const word_id_t n, std::vector<uint32_t>& ids, std::vector<FPTYPE>& weights) {
    const std::vector<int64_t> pq = pair_ids(selected_pairs);
    ids.assign(selected_pairs.size() * n, 0);
    weights.assign(selected_pairs.size() * n, 0.f);
    check(isle_hip_edge_top_words(ctx_, ISLE_MODEL_CATCH, nullptr, vocab_size_, (int)post_topics_, pq.data(), (int)selected_pairs.size(),
                                  (float)ISLE_EDGE_TOPIC_PRIMARY_RATIO, (int)n, ids.data(), weights.data()),
          "edge_top_words");
  }
};

}  // namespace ISLE
