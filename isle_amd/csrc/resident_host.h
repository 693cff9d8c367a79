// isle_amd/csrc/resident_host.h — what a context holds from one C-ABI call to the next, and which event voids it.  A context carries about
// twenty products (A, B, the operator, U, the projection P and its two copies, the lifted centres, the partition, the member lists, the
// k-means++ tile minima, the projected centres, catchwords, the two models, the loaded model, the inference result); whether each of them
// still describes the current inputs is the ledger below (isle_ctx::res).  Everybody reads the fields; only the events of this header
// write them, one function per event, so that "which event voids which product" is stated once.  Plain C++ (no HIP type, no isle_ctx):
// ../host/resident_host_main.cpp applies the events to a script, tests/test_resident_host_cpu.py states every field after every event.
// A forgotten line here raises no error: it yields a wrong partition, or a report about another corpus.
#pragma once
#include <cstdint>

// the split copy of the projection (isle_ctx::Pt2): the two bf16 terms of the coordinate-major copy, as the LDS image of every (row block, slab)
enum IslePt2 {
  ISLE_PT2_ABSENT = 0,
  ISLE_PT2_BY_DOCUMENT = 1,  // row m = document m: split from the f32 transposed copy
  ISLE_PT2_BY_POSITION = 2,  // row m = document dperm[m] (the length order): written by the grouped projection on its way
};

struct IsleResident {
  // ---- the two matrices
  bool a_ready = false;           // a_cnt / a_rows / a_offs hold the count matrix that a_V / a_D / a_nnz describe
  bool a_avg_valid = false;       // a_avg is avg_doc_sz of the current A over all ranks
  bool b_from_threshold = false;  // B's columns are the kept documents of A (original_cols, zetas are its); false: B came from the host
  // ---- the Gram operator of the current B
  int gl_mode = -1;               // -1 not decided for the current B, 0 gather form, 1 LDS-banded form
  bool band_ready = false;        // the transposed copy that form needs is built (void at every solve: the reference builds per solve)
  // ---- U and the projection P = B^T U
  int U_k = 0;                    // columns of U in Ucm / Urm; 0: none
  bool P_ready = false;           // P / pnorm hold B^T U and its squared row norms for the current B and U (not dot products of an assignment)
  bool Pt_ready = false;          // Pt is the f32 coordinate-major copy of that P
  IslePt2 Pt2 = ISLE_PT2_ABSENT;  // the split copy of that P, and what its rows are
  uint64_t P_gen = 0;             // projections made so far: "made on projection n" is compared by the predicates below and nowhere else
  // ---- k-means++ and Lloyd in span(U)
  int kmpp_track_k = 0;           // 0: nothing to start from; k: kmpp_arg / _m2a / _tmin / _best are complete for the k seeds in kmpp_C_host ...
  uint64_t kmpp_P_gen = 0;        // ... and were computed on this projection
  int km_proj_k = 0;              // Cdev holds the centres of a finished loop in span(U) with this k (0: seeds, or nothing) ...
  uint64_t km_proj_P_gen = 0;     // ... computed on this projection
  // ---- word-space centres and the partition
  bool centers_ready = false;     // centers_rm holds centers_k word-space centres of the current B and U
  int centers_k = 0;
  bool lift_valid = false;        // those centres are U lift_C^T exactly as isle_hip_lift_centers left them (lift_k columns, row stride lift_ld):
  int lift_ld = 0, lift_k = 0;    // Lloyd on B may take its first assignment through the projection
  bool assign_valid = false;      // `assign` is a partition of the current B's documents that a finished Lloyd on B or the caller put there
  int km_last_space = -1;         // the loop that wrote `assign` last and iterated at least once (ISLE_SPACE_*; -1: none, or the caller's partition) ...
  int km_last_k = 0;              // ... and its k
  // `members` is SOME permutation of the local documents grouped by a centre.  It does NOT say "grouped by the current `assign`": the lists
  // shape only the order in which documents are visited (cache locality of the centre rows), never a result, so a new partition does not
  // clear this.  It is cleared where the lists would not be a permutation of the current documents (a new B), and by the callers that want
  // the next reader to build fresh lists (a caller's partition, the centroid update by changed documents, the objective's own lists).
  bool members_valid = false;
  // ---- downstream stage and inference
  int p_k = 0;                    // num_topics of the last catchword pass
  bool p_catch_ready = false;     // p_catch / p_thr / p_cluster_of are the catchwords of the current A, B and partition for p_k topics
  bool p_model_ready = false;     // p_model, p_top1 / p_top2 and the document-topic sums are the topic model of those catchwords
  bool p_avg_ready = false;       // p_avg_model is the cluster-average model of those catchwords
  bool ml_ready = false;          // ml_model is the last model read by isle_hip_load_model_text (independent of A, B and the partition)
  bool inf_valid = false;         // inf_* are the document-topic weights of the last resident inference over the current A

  // ---- predicates: what the call sites ask ------------------------------------------------------------------------------------------------
  bool Pt2_ready() const { return Pt2 != ISLE_PT2_ABSENT; }
  bool Pt2_by_position() const { return Pt2 == ISLE_PT2_BY_POSITION; }
  // the state the k-means++ rounds kept was computed on the projection that is resident now (ProjFacts::kmpp_same_P)
  bool kmpp_same_P() const { return kmpp_P_gen == P_gen; }
  // b_d^T (U c) can go through the pass-1 stream of the LDS-banded operator as a thin product: the operator is built in that form, U has k columns
  bool thin_product_possible(int k) const { return gl_mode == 1 && band_ready && U_k == k; }
  // isle_hip_kmeans_objective without a partition: `assign` is the one the loop of `space` left for k (the word space also wants it whole) ...
  bool loop_partition_resident(int space, int k, bool word) const { return km_last_space == space && km_last_k == k && (!word || assign_valid); }
  // ... the projection the loop in span(U) ran on is still the resident one ...
  bool loop_projection_resident() const { return P_ready && P_gen == km_proj_P_gen; }
  // ... and without centres: centers_rm / Cdev hold that loop's
  bool loop_centres_resident(bool word, int k) const { return word ? centers_ready && centers_k == k : km_proj_k == k; }

  // ---- events: the only writers ---------------------------------------------------------------------------------------------------------------
  // A is being rewritten: a_cnt / a_rows / a_offs or a_V / a_D / a_nnz change from here on, and nothing says yet that the new A will be accepted
  void A_rewrite_begins() { a_ready = false; }
  // A installed: the buffers and sizes describe one accepted count matrix; what was read off the previous one is void
  void A_installed() {
    a_ready = true;
    a_avg_valid = false;
    inf_valid = false;  // the entries of isle_hip_infer_resident are about A's documents
    void_downstream();
  }
  // the corpus statistics of the current A were computed (thresholding, or the first catchword pass on a B from the host)
  void corpus_average_known() { a_avg_valid = true; }
  // B replaced, by an upload (from_threshold false) or by the thresholding of A: everything derived from the previous B is void, whether or
  // not the new one is accepted
  void B_replaced(bool from_threshold) {
    band_ready = false;
    gl_mode = -1;
    void_projection();
    lift_valid = false;
    members_valid = false;
    U_k = 0;
    centers_ready = false;
    assign_valid = false;
    kmpp_track_k = 0;
    km_last_space = -1;
    km_proj_k = 0;
    void_downstream();
    b_from_threshold = from_threshold;
  }
  // operator form decided for the current B.  k_gl_detect raises it twice: with the gather form before its device work, so that a failure
  // there leaves a form every kernel can run, then with the answer
  void operator_form_decided(bool lds_banded) { gl_mode = lds_banded ? 1 : 0; }
  void operator_built() { band_ready = true; }
  // operator must be rebuilt: every solve builds its own, as the reference's operator constructor does
  void operator_must_be_rebuilt() { band_ready = false; }
  // U installed with k columns: the projection and the word-space centres were made with another U
  void U_installed(int k) {
    U_k = k;
    void_projection();
    lift_valid = false;
    centers_ready = false;
  }
  // projection about to be made: P is not ready (or this would not run), and its copies are those of an earlier P
  void projection_begins() {
    Pt_ready = false;
    Pt2 = ISLE_PT2_ABSENT;
  }
  // projection made; the grouped form may have written the split copy by position on its way
  void projection_made(bool split_by_position) {
    P_ready = true;
    P_gen++;
    if (split_by_position) Pt2 = ISLE_PT2_BY_POSITION;
  }
  void transposed_copy_made() { Pt_ready = true; }          // the f32 coordinate-major copy (k_ensure_pt)
  void split_copy_made() { Pt2 = ISLE_PT2_BY_DOCUMENT; }    // split from that transposed copy
  // P overwritten with the dot products of an assignment: it is computed again when it is needed again
  void P_overwritten() { void_projection(); }
  // k-means++ begins: Cdev holds seeds from here on, and the tile minima are rewritten
  void kmpp_begins() {
    km_proj_k = 0;
    kmpp_track_k = 0;
  }
  // k-means++ kept a complete first assignment for the k seeds it handed out, on the current projection
  void kmpp_kept_first_assignment(int k) {
    kmpp_P_gen = P_gen;
    kmpp_track_k = k;
  }
  // Lloyd in span(U) begins: Cdev and `assign` are its from here on.  Raised in three steps, because the call reads the ledger in between:
  // at entry; when `assign` is about to be written (partition_rewrite_begins); when the route has been chosen from what k-means++ kept
  void lloyd_projected_begins() {
    km_proj_k = 0;
    km_last_space = -1;
  }
  void kmpp_first_assignment_taken() { kmpp_track_k = 0; }  // used (the tile minima become bounds in place) or stale
  // `assign` is about to be rewritten by a loop (both spaces)
  void partition_rewrite_begins() { assign_valid = false; }
  // Lloyd in span(U) ends after at least one iteration: what isle_hip_kmeans_objective reads as the resident state of that space.  (It does
  // not set assign_valid: the catchword stage takes the partition of Lloyd on B or the caller's.)
  void lloyd_projected_done(int space, int k) {
    km_last_space = space;
    km_last_k = k;
    km_proj_k = k;
    km_proj_P_gen = P_gen;
  }
  // word-space centres installed for n columns (lifted, or the caller's)
  void centres_installed(int n) {
    centers_ready = true;
    centers_k = n;
  }
  void centres_lifted(int ld, int k) {
    lift_ld = ld;
    lift_k = k;
    lift_valid = true;
  }
  // centres given by the caller, or about to move: they are no longer U lift_C^T
  void centres_not_lifted() { lift_valid = false; }
  // Lloyd on B begins
  void lloyd_word_begins() { km_last_space = -1; }
  // Lloyd on B ends: the partition stays resident for isle_hip_catchwords; with at least one iteration it is that loop's for the objective
  void lloyd_word_done(int space, int k, bool iterated) {
    assign_valid = true;
    if (iterated) {
      km_last_space = space;
      km_last_k = k;
    }
  }
  void member_lists_built() { members_valid = true; }
  // member lists belong to an earlier assignment, and the caller wants the next reader to know (see members_valid)
  void member_lists_stale() { members_valid = false; }
  // partition handed in by the caller: no loop's
  void partition_given() {
    assign_valid = true;
    members_valid = false;
    km_last_space = -1;
  }
  // catchwords done for k topics: the models are those of earlier catchwords
  void catchwords_done(int k) {
    p_k = k;
    p_catch_ready = true;
    p_model_ready = false;
    p_avg_ready = false;
  }
  void topic_model_done() { p_model_ready = true; }
  void avg_model_begins() { p_avg_ready = false; }
  void avg_model_done() { p_avg_ready = true; }
  void model_loaded() { ml_ready = true; }
  void inference_begins() { inf_valid = false; }
  void inference_done() { inf_valid = true; }

 private:
  void void_projection() {
    P_ready = false;
    Pt_ready = false;
    Pt2 = ISLE_PT2_ABSENT;
  }
  void void_downstream() {  // catchwords and models are read off both matrices
    p_catch_ready = false;
    p_model_ready = false;
    p_avg_ready = false;
  }
};
