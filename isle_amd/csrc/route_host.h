// isle_amd/csrc/route_host.h — every rule that chooses which form of a computation runs for a given shape, device and switch setting: the
// typed values of the "form" and "tuning" switches (RouteEnv, filled from the strings of knobs.h's table by route_env), and one function per
// rule.  These rules fix the roundings, the launch sequence and the speed of every step.  Plain C++ (no HIP type, no isle_ctx, nothing read
// from the environment): a rule takes integers, doubles, the context's validity flags as plain bools and a RouteEnv, so that a threshold is
// checked without a device: ../host/route_host_main.cpp applies the rules to a script, tests/test_route_host_cpu.py states the answers.
// Float and double expressions keep the type, the order and the constants they were measured with: a comparison that flips at a threshold
// changes which kernel runs.  A rule with a side effect is cut in two: the decision from sizes is here; the allocation, the device query or
// the agreement across ranks stays at the call site.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "gl_plan.h"
#include "knobs.h"
#include "ks_host.h"

// ---- the switches -------------------------------------------------------------------------------------------------------------------------
// One field per switch, named after it.  The meanings are not uniform and are kept as they grew: some switches are on when set to ANY value
// ("0" and the empty string included), the ones that default to on are turned off by a value whose atoi is 0 (the empty string included),
// the rest match exact words.
struct RouteEnv {
  bool gram_lds = true;           // off only at atoi == 0
  int gl_g1 = 0, gl_g2 = 0;       // through gl_forced_g; 0: the build's own rule
  bool gl_place = true, gl_fill_buckets = true, gl_rounds = true, gl_columns = true;  // off at atoi == 0
  int gl_panel = 0;               // 10 | 8; 0 (unset, or anything else): the default
  bool gl_wide_grouped = true;    // off at atoi == 0
  bool wide_gather = false, wide_lds = false;  // set at all
  bool ks_rowshard = true;        // off at atoi == 0
  bool ks_sync = false;           // set at all
  int ks_ortho_passes = 2;        // ks_host.h ks_ortho_passes
  bool update_mfma = true;        // off at atoi == 0
  bool evd_jacobi = false, td_chain = false;  // set at all
  int td_bar = 2;                 // the barrier of td_persist_k<B>: 0 "flat", 1 "hier", 2 otherwise (sharded counters)
  bool td_back = false;           // the value begins with 's' (seq)
  bool evd_split = false;         // set and atoi != 0
  bool kmpp_host_dice = false;    // set at all
  int kmpp_sparse = -1;           // -1 unset (by cost), 0, 1 (atoi != 0)
  bool kmpp_track = true;         // off at atoi == 0
  bool no_hamerly = false;        // set at all
  int kmeans_bounds = 0;          // 1 "hamerly", 2 "none", 0 otherwise (Yinyang)
  bool proj_bounds = false;       // "hamerly"
  int proj_full = 0;              // 1 "gemm", 2 "fused", 0 otherwise (by size)
  int first_assign = 0;           // 1 "sparse", 2 "projection", 0 otherwise (by cost)
  bool gemm_bf16x3 = true, gemm_epilogue = true;  // off at atoi == 0
  int gemm_terms = 2;             // 3 at atoi == 3
  bool gemm_dma = true;           // off at atoi == 0
  int yy_mode = -1;               // 0 "doc", 1 "docg", 2 "group", -1 otherwise (by the group count)
  bool yy_fused = true, yy_movers = true, yy_regroup = true;  // off at atoi == 0
  int yy_order = -1;              // -1 unset (by the form), 0 "doc", 1 any other value (member)
  bool pt_sort = true;            // off at atoi == 0
  bool proj_active = true;        // all centres through the assignment product: unset or "gemm"; false: any other value (tiles)
  bool proj_sums = false;         // "fresh"
  bool centers_fresh = false;     // set at all
  uint32_t infer_cap_rows = 0;    // atoi
  uint32_t chunk_cols = 0;        // atoi; 0: the default
  bool comm_timeout_set = false;  // ISLE_COMM_TIMEOUT_S
  double comm_timeout = 0.0;      // its atof
  int comm_selftest = -1;         // -1 unset (the transport's default), 0 at atoi == 0, 1 otherwise
};

// val[id]: the string of switch id, null where it is not set
inline RouteEnv route_env(const char* const* val) {
  const auto set = [&](int id) { return val[id] != nullptr; };
  const auto zero = [&](int id) { return val[id] && atoi(val[id]) == 0; };
  const auto is = [&](int id, const char* word) { return val[id] && !strcmp(val[id], word); };
  const auto num = [&](int id) { return atoi(val[id]); };
  RouteEnv e;
  e.gram_lds = !zero(KN_GRAM_LDS);
  if (set(KN_GL_G1)) e.gl_g1 = gl_forced_g(num(KN_GL_G1));
  if (set(KN_GL_G2)) e.gl_g2 = gl_forced_g(num(KN_GL_G2));
  e.gl_place = !zero(KN_GL_PLACE);
  e.gl_fill_buckets = !zero(KN_GL_FILL_BUCKETS);
  e.gl_rounds = !zero(KN_GL_ROUNDS);
  e.gl_columns = !zero(KN_GL_COLUMNS);
  if (set(KN_GL_PANEL) && (num(KN_GL_PANEL) == 10 || num(KN_GL_PANEL) == 8)) e.gl_panel = num(KN_GL_PANEL);
  e.gl_wide_grouped = !zero(KN_GL_WIDE_GROUPED);
  e.wide_gather = set(KN_WIDE_GATHER);
  e.wide_lds = set(KN_WIDE_LDS);
  e.ks_rowshard = !zero(KN_KS_ROWSHARD);
  e.ks_sync = set(KN_KS_SYNC);
  e.ks_ortho_passes = ks_ortho_passes(val[KN_KS_ORTHO_PASSES]);
  e.update_mfma = !zero(KN_UPDATE_MFMA);
  e.evd_jacobi = set(KN_EVD_JACOBI);
  e.td_chain = set(KN_TD_CHAIN);
  e.td_bar = is(KN_TD_BAR, "flat") ? 0 : is(KN_TD_BAR, "hier") ? 1 : 2;
  e.td_back = set(KN_TD_BACK) && val[KN_TD_BACK][0] == 's';
  e.evd_split = set(KN_EVD_SPLIT) && !zero(KN_EVD_SPLIT);
  e.kmpp_host_dice = set(KN_KMPP_HOST_DICE);
  if (set(KN_KMPP_SPARSE)) e.kmpp_sparse = num(KN_KMPP_SPARSE) != 0;
  e.kmpp_track = !zero(KN_KMPP_TRACK);
  e.no_hamerly = set(KN_NO_HAMERLY);
  e.kmeans_bounds = is(KN_KMEANS_BOUNDS, "hamerly") ? 1 : is(KN_KMEANS_BOUNDS, "none") ? 2 : 0;
  e.proj_bounds = is(KN_PROJ_BOUNDS, "hamerly");
  e.proj_full = is(KN_PROJ_FULL, "gemm") ? 1 : is(KN_PROJ_FULL, "fused") ? 2 : 0;
  e.first_assign = is(KN_FIRST_ASSIGN, "sparse") ? 1 : is(KN_FIRST_ASSIGN, "projection") ? 2 : 0;
  e.gemm_bf16x3 = !zero(KN_GEMM_BF16X3);
  e.gemm_epilogue = !zero(KN_GEMM_EPILOGUE);
  e.gemm_terms = set(KN_GEMM_TERMS) && num(KN_GEMM_TERMS) == 3 ? 3 : 2;
  e.gemm_dma = !zero(KN_GEMM_DMA);
  e.yy_mode = is(KN_YY_MODE, "doc") ? 0 : is(KN_YY_MODE, "docg") ? 1 : is(KN_YY_MODE, "group") ? 2 : -1;
  e.yy_fused = !zero(KN_YY_FUSED);
  e.yy_movers = !zero(KN_YY_MOVERS);
  e.yy_regroup = !zero(KN_YY_REGROUP);
  if (set(KN_YY_ORDER)) e.yy_order = is(KN_YY_ORDER, "doc") ? 0 : 1;
  e.pt_sort = !zero(KN_PT_SORT);
  e.proj_active = !set(KN_PROJ_ACTIVE) || is(KN_PROJ_ACTIVE, "gemm");
  e.proj_sums = is(KN_PROJ_SUMS, "fresh");
  e.centers_fresh = set(KN_CENTERS_FRESH);
  if (set(KN_INFER_CAP_ROWS)) e.infer_cap_rows = (uint32_t)num(KN_INFER_CAP_ROWS);
  if (set(KN_CHUNK_COLS)) e.chunk_cols = (uint32_t)num(KN_CHUNK_COLS);
  e.comm_timeout_set = set(KN_COMM_TIMEOUT);
  if (set(KN_COMM_TIMEOUT)) e.comm_timeout = atof(val[KN_COMM_TIMEOUT]);
  if (set(KN_COMM_SELFTEST)) e.comm_selftest = !zero(KN_COMM_SELFTEST);
  return e;
}

// ---- the device, the communicator (api.cpp) ----------------------------------------------------------------------------------------------
// May an optional scratch of the GEMM routes be taken?  A function of the problem's size and the device's TOTAL memory only — never of what
// happens to be free — so that the route, and with it every rounding of the first assignment, is the same run after run and rank after
// rank: always up to 8 GB; beyond (all of config 3 on one GPU: 40 GB), up to a fifth of the device (57 GB on an MI355X).  total_mem == 0:
// the device has not been asked yet.  Where the answer needs it *ask is set and the answer is no: the caller asks the device once and
// applies the rule again (isle_route_mem, common.h), so the query stays where the decision first needs it.
inline bool route_scratch_ok(double bytes, uint64_t total_mem, bool* ask) {
  if (bytes <= 8e9) return true;
  if (total_mem == 0) {
    *ask = true;
    return false;
  }
  return bytes <= 0.2 * (double)total_mem;
}
// the self-test behind a communicator's creation; dflt: on over RCCL with more than one rank, off for the host-staged test transport
inline bool route_comm_selftest(bool dflt, const RouteEnv& e) { return e.comm_selftest >= 0 ? e.comm_selftest != 0 : dflt; }
// seconds of the watchdog; now: the context's value (300 until a communicator was created with the switch set)
inline double route_comm_timeout(double now, const RouteEnv& e) { return e.comm_timeout_set ? e.comm_timeout : now; }

// ---- block Krylov-Schur (api_ks.cpp) -------------------------------------------------------------------------------------------------------
// every rank orthogonalises its row slice of the Krylov block (multi: the context has a communicator of either transport)
inline bool route_ks_rowshard(bool multi, bool dense_A, const RouteEnv& e) { return multi && !dense_A && e.ks_rowshard; }
inline bool route_ks_pipelined(const RouteEnv& e) { return !e.ks_sync; }

// ---- dense kernels (dense.hip) ---------------------------------------------------------------------------------------------------------
// the orthogonalisation's update F -= V H on the matrix cores; aligned16: both operands start on 16 bytes
inline bool route_update_mfma(int b, int m, uint64_t ld, bool aligned16, const RouteEnv& e) {
  return b <= 16 && m >= 32 && (ld & 3) == 0 && aligned16 && e.update_mfma;
}
inline uint64_t route_gemm_tiles(uint64_t M, int N) { return (M + 255) / 256 * (uint64_t)((N + 255) / 256); }  // tiles of 256 x 256
// the M x K x N product of an assignment step on the bf16 matrix cores, operands split in three terms; false: gemm_f32.h
inline bool route_gemm_bf16x3(uint64_t M, int K, int N, const RouteEnv& e) { return !(!e.gemm_bf16x3 || N < 64 || K < 32 || route_gemm_tiles(M, N) < 512); }
// may the fused route be taken?  (the bf16 product with 256 x 256 tiles; small products keep the two-kernel route)
inline bool route_gemm_assign_fused_ok(uint64_t M, int K, int N, const RouteEnv& e) {
  return e.gemm_bf16x3 && e.gemm_epilogue && N >= 64 && K >= 32 && route_gemm_tiles(M, N) >= 512 && M < (1ull << 32);
}
// an assignment product runs with two bf16 terms first (and the rows that leaves open again with three); has_rows: the row-major operand is there
inline bool route_gemm_two_terms(bool has_rows, const RouteEnv& e) { return !(e.gemm_terms == 3) && has_rows; }
// its two-term pass reads the pre-split copy of A by LDS-DMA
inline bool route_gemm_dma(bool has_split, const RouteEnv& e) { return has_split && e.gemm_dma; }
// the small symmetric EVD by tridiagonalisation; false: block Jacobi
inline bool route_evd_tridiag(int n, const RouteEnv& e) { return n >= 16 && !e.evd_jacobi; }

// ---- the projection and k-means++ (api_kmeans.cpp ensure_P, isle_hip_kmeanspp_projected; kmeans.hip k_kmpp_update) -------------------------
// the projection also writes its two bf16 terms in the layout the LDS-DMA product stages
inline bool route_want_a2(uint64_t D, int k, const RouteEnv& e) { return D && route_gemm_assign_fused_ok(D, k, k, e) && e.gemm_dma && !(e.gemm_terms == 3); }

struct KmppPlan {
  // k > 224 (Lloyd in span(U) keeps tile bounds): the rounds also keep every document's nearest seed and tile minima, so that Lloyd's
  // first assignment — a D x k x k pass against exactly these seeds — need not be computed again (kmeans.hip kmpp_min_dots_track_k)
  bool track;
  int maxdraw;
  // one rank, seeds not injected: the device throws the dice of a round itself while they fit its 40 slots (kmpp_draw_on_device); the
  // switch is for the test that holds both forms to the same seeds
  bool device_dice;
};
inline KmppPlan route_kmpp_plan(int k, bool multi, bool injected, const RouteEnv& e) {
  KmppPlan plan;
  plan.track = k > 224 && (k + 31) / 32 <= 32 && e.kmpp_track;
  plan.maxdraw = 2 + (int)std::ceil(std::sqrt((double)k));
  plan.device_dice = !multi && !injected && !e.kmpp_host_dice;
  return plan;
}
// The k-means++ round against nc new seeds through thin products of B instead of on the materialised projection.  The rule compares
// measured rates: a pass of the pass-1 stream costs ~2.8 ps per nonzero (= 15.4 bytes of streaming at 5.5 TB/s), the materialised
// projection streams at 5.5 TB/s for <= 16 new seeds (kmpp_min_pt_k) and 2.3x slower through the matrix-core tile beyond.
// can: the LDS-banded operator is built for this B and U has k columns; PW: route_gl_panel_width
inline bool route_kmpp_sparse(bool can, uint64_t nnz, uint64_t D, int ldk, int nc, int PW, const RouteEnv& e) {
  const int passes = (nc + PW - 1) / PW;  // columns per pass of the pass-1 stream
  bool sparse = can && 15.4 * (double)nnz * passes < 4.0 * (double)ldk * (double)D * (nc <= 16 ? 1.0 : 2.3);
  if (e.kmpp_sparse >= 0) sparse = e.kmpp_sparse != 0 && can;
  return sparse;
}

// ---- Lloyd in span(U) (api_kmeans.cpp, kmeans.hip) -----------------------------------------------------------------------------------------
// The route decisions of one call, taken once behind ensure_P (the switches are read at isle_enter only) and read everywhere below.
struct ProjPlan {
  bool hamerly;  // Hamerly bounds (exact skip of documents whose closest centre provably did not change), as in the sparse Lloyd
  // k > 224 (more than 7 tiles of 32 centres): one lower bound per tile instead of Hamerly's single one, which prunes nothing at
  // k = 1000 (kmeans.hip PR_TILES, spmm.hip pt_filter_k).  ISLE_PROJ_BOUNDS=hamerly keeps the single bound.
  bool tiles;
  int T, TL;
  bool from_kmpp;   // the first assignment is the one the k-means++ rounds kept
  bool pt_sorted;   // the active documents are ordered by the tiles they need: the filter walks the documents in their own order
  bool delta_sums;  // the centroid sums are kept up to date by the documents that changed centre
  bool movers;      // tile bounds may leave centres that jumped out of their tiles' movements (where the thin product exists: proj_reassign_tiles)
};
struct ProjFacts {
  uint64_t D;
  bool Pt_ready, Pt2_ready, P_ready;
  int kmpp_track_k;  // the k of the k-means++ rounds that kept their nearest seeds
  bool kmpp_same_P;  // ... on the projection that is there now
  bool seeds_kept;   // the centres of this call equal the seeds those rounds returned
};
inline ProjPlan route_proj_plan(const ProjFacts& f, int k, const RouteEnv& e) {
  ProjPlan p;
  p.hamerly = !e.no_hamerly && (f.Pt_ready || f.Pt2_ready);
  p.T = (k + 31) / 32;
  p.TL = (p.T + 3) & ~3;
  p.tiles = p.hamerly && k > 224 && p.T <= 32 && !e.proj_bounds;
  p.from_kmpp = p.tiles && f.kmpp_track_k == k && f.kmpp_same_P && f.P_ready && e.kmpp_track && f.seeds_kept;
  p.pt_sorted = e.pt_sort;
  p.delta_sums = !e.proj_sums && f.D < (1ull << 31);
  p.movers = e.yy_movers && f.D > 0;
  return p;
}
// the n active documents are ordered by the tiles they ask for (has_need: their tile masks are there)
inline bool route_pt_sort(bool has_need, uint32_t n, const RouteEnv& e) { return has_need && n > 256 && e.pt_sort; }
// The full pass with tile bounds through the assignment product: 2 D k^2 flop of plain matrix product, above ~20 GFLOP, where the product's
// epilogue runs inside it or its D x k scratch may be taken (route_scratch_ok).  ISLE_PROJ_FULL=gemm|fused forces a route.
inline bool route_proj_full_by_gemm(bool Pt_ready, bool Pt2_ready, uint64_t D, int k, const RouteEnv& e, uint64_t total_mem, bool* ask) {
  return (Pt_ready || Pt2_ready) && D > 0 && k >= 64 &&
         (route_gemm_assign_fused_ok(D, k, k, e) || route_scratch_ok((double)D * k * sizeof(float), total_mem, ask)) &&
         ((2.0 * (double)D * k * k >= 2e10 && !(e.proj_full == 2)) || e.proj_full == 1);
}
// the n active documents against all centres through the assignment product on their gathered rows; false: only the tiles their bounds name
inline bool route_proj_active_by_gemm(uint64_t n, int k, const RouteEnv& e) { return e.proj_active && route_gemm_assign_fused_ok(n, k, k, e); }

// ---- Lloyd on B (api_kmeans.cpp, spmm.hip) ---------------------------------------------------------------------------------------------
struct SparsePlan {
  // Default: Yinyang group bounds (groups of 8 centres); ISLE_KMEANS_BOUNDS=hamerly|none selects the others.
  bool hamerly /*any bound-based mode*/, yinyang;
  int G;
  // form of the Yinyang iteration: 0 = by document over the row-major centres, 1 = by document over the group-major copy, 2 = by group.
  // The forms that visit documents in member order (docg, group) hold a document's group bounds four per lane: at most 256 groups
  // (k <= 2048); beyond, by document over the row-major centres, whatever ISLE_YY_MODE asks for
  int yy_mode;
  // by group: the bounds are lowered and the active documents tightened in one launch (the D x G bounds read once), ISLE_YY_FUSED=0: in two
  bool fused;
  // Visiting order of the assignment step: the member lists of the previous iteration, which are then made every iteration (the
  // Hamerly and plain forms: cache locality of the centre rows; results are order-independent).  The fused by-group launch takes the
  // documents in their own order since the end of round 5 (its first phase then streams the bounds as one run per workgroup; once that
  // phase kept sixteen loads in flight the member order's gain in the second phase — neighbours share the own group's table — no longer
  // paid for its scattered rows: sparse_assign 177 -> 170 ms at config 3): nothing reads the lists then, and they are not made (a sort
  // of D keys per iteration).  ISLE_YY_ORDER = doc | member forces either.
  bool by_members;
  bool fused_first;     // the product's epilogue forms the first assignment: no D x k scratch
  bool via_projection;  // the first assignment is the dense product on the projection (where its scratch is had: first_scratch_had)
  bool regroup;         // the Yinyang groups are formed from the centres in the order of their squared norms (sparse_regroup_tables)
  bool movers;          // centres that jumped may be left out of their groups' movements (where the thin product exists: sparse_reassign_yinyang)
};
struct SparseFacts {
  uint64_t D, nnz;
  bool lift_valid;  // the centres came from isle_hip_lift_centers
  int lift_k, U_k, ldk;
  bool P_ready, Pt_ready, Pt2_ready;
};
inline SparsePlan route_sparse_plan(const SparseFacts& f, int k, int ld, const RouteEnv& e, uint64_t total_mem, bool* ask) {
  const uint64_t D = f.D;
  SparsePlan p;
  p.hamerly = !e.no_hamerly && !(e.kmeans_bounds == 2);
  p.yinyang = p.hamerly && !(e.kmeans_bounds == 1);
  p.G = (k + 7) / 8;
  p.yy_mode = !p.yinyang ? 0 : p.G > 256 ? 0 : e.yy_mode >= 0 ? e.yy_mode : (p.G >= 32 ? 2 : 0);
  p.fused = p.yy_mode == 2 && e.yy_fused;
  p.by_members = !p.yinyang || !p.yy_mode || (e.yy_order >= 0 ? e.yy_order != 0 : !p.fused);
  p.movers = p.fused && e.yy_movers;
  // first assignment through the projection: only for centres that came from isle_hip_lift_centers (lift_valid) with the current U and P, and
  // while the dense product is cheaper than the sparse one: always up to k = 384; beyond, by the measured rates — the D x k x k
  // product runs at ~130 TFLOP/s (rocBLAS), a panel pass of the sparse product takes ~2.8 ps per nonzero (C3 shard, k = 1000: 19 against
  // 44 ms) — and while its D x k scratch can be had (route_scratch_ok; first_scratch_had at run time) (ISLE_FIRST_ASSIGN=sparse|projection forces)
  const double t_dense = 2.0 * (double)D * k * k / 130e12, t_sparse = (double)((k + 7) / 8) * (double)f.nnz * 2.8e-12;
  p.fused_first = p.yinyang && route_gemm_assign_fused_ok(D, k, k, e);
  const bool dense_pays = k <= 384 || (t_dense < t_sparse && (p.fused_first || route_scratch_ok((double)D * k * sizeof(float), total_mem, ask)));
  p.via_projection = f.lift_valid && f.lift_k == k && f.U_k == k && f.P_ready && (f.Pt_ready || f.Pt2_ready) && f.ldk == ld && D > 0 &&
                     (dense_pays || e.first_assign == 2) && !(e.first_assign == 1);
  // Regrouping (round 5).  A Yinyang group's bound is the distance to its CLOSEST member, so one centre every document is near spoils the
  // bound of its whole group — and the centres of small squared norm (the large, diffuse clusters) are near every document that lies
  // far from everything else: with groups of eight consecutive labels those few centres sit in as many groups and an undecided document
  // scans them all (config 3: 10 - 15 groups per active document in the first iterations).  The groups are therefore formed from the
  // centres in the order of their squared norms at the loop's entry (stable: equal norms keep their labels' order), through slot
  // tables (YyMap); labels, ties and everything outside the by-group kernels stay in the centres' own numbering.  Config 3 on one GPU:
  // 137 M -> 39 M (document, group) pairs per step, Lloyd on B 296 -> 199 ms, same partition (tools/yy_probe.py, profiles/r05_d_*).
  // Taken with the by-group form behind the product's first assignment; ISLE_YY_REGROUP=0 keeps groups of consecutive labels.
  p.regroup = p.yinyang && p.yy_mode == 2 && p.via_projection && p.fused_first && e.yy_regroup;
  return p;
}
// iteration `it` makes the member lists: the visiting order of the next assignment, and what the FRESH counting centroid update walks
inline bool route_member_lists(int it, bool by_members, int gl_mode, const RouteEnv& e) { return it == 0 || by_members || gl_mode != 1 || e.centers_fresh; }
// the centroid update recounts from the member lists; false: it moves the documents that changed centre
inline bool route_counts_fresh(bool first_of_run, const RouteEnv& e) { return first_of_run || e.centers_fresh; }

// ---- k-wide products (spmm.hip) -----------------------------------------------------------------------------------------------------------
// The k-wide products as ceil(k / 12) passes of the LDS-banded pass-1 stream pay one staging of every word band per pass: a
// win while the vocabulary spans few bands (C2: 15 bands, 5.8 vs 7.0 ms), a loss at 30 bands (C3 shard: 68 vs 52 ms).
// ISLE_WIDE_GATHER=1 / ISLE_WIDE_LDS=1 force either form.
inline bool route_wide_through_lds(uint64_t V, const RouteEnv& e) {
  if (e.wide_gather) return false;
  if (e.wide_lds) return true;
  return V <= 32 * 3412;  // 8-column panels (route_gl_panel_width): measured 46.7 against 51.7 ms at 30 word bands (V = 100k, k = 1000)
}
// float4 per lane of the row-gather kernel (spmm_wide_k<NIT>) at leading dimension ldk; 0: refused (k > 2048)
inline int route_wide_nit(int ldk) {
  const int nit = (ldk / 4 + 63) / 64;
  return nit <= 1 ? 1 : nit <= 2 ? 2 : nit <= 4 ? 4 : nit <= 8 ? 8 : 0;
}

// ---- LDS-banded Gram operator (gram_lds.hip) -------------------------------------------------------------------------------------------
// this rank's shard may take the LDS-banded form (then its rows are checked for a single value, and the ranks agree)
inline bool route_gl_eligible(uint64_t nnz, uint64_t D, uint64_t V, const RouteEnv& e) {
  return e.gram_lds && nnz > 0 && D > 0 && V > 0 && D < 0xfffffff0ull && V < 0xfffffff0ull;
}
// every switch the plan depends on (the test hook ISLE_GL_TEST_CUS is the caller's)
inline GlPlanOpts route_gl_options(const RouteEnv& e) {
  GlPlanOpts o;
  o.g1 = e.gl_g1;
  o.g2 = e.gl_g2;
  o.rounds = e.gl_rounds;
  o.columns = e.gl_columns;
  return o;
}
// the pass-2 id stream is filled by buckets of word positions (positions in 20 bits); false: by one scatter
inline bool route_gl_fill_bucketed(uint32_t n_out, uint64_t nnz, const RouteEnv& e) { return n_out <= (1u << 20) && nnz && e.gl_fill_buckets; }
// Columns per pass of the k-wide / thin products through the pass-1 stream: 10, the widest panel a planar band holds (40-byte rows); 8 at
// 8 output items per lane (the 10-column form spills 8 registers there).  A pass costs what its slots cost, hardly more for more columns
// (2.20 ms per 8-column pass against 2.29 per 10-column one at config 3 on one GPU): k = 1000 is walked in 100 passes.  Steps of 10 columns
// leave the panels 8-byte aligned inside the output rows: they are stored as float2.  (Up to round 3's 48-byte row-major bands 12-column
// passes were used up to 6 items per lane: 33.0 ms per C3-shard projection against 38.9 in 8-column passes.)  ISLE_GL_PANEL = 8 | 10.
inline int route_gl_panel_width(int gl1_G /*items per lane of pass 1*/, const RouteEnv& e) {
  if (e.gl_panel) return e.gl_panel;
  return gl1_G <= 7 ? 10 : 8;
}
// The grouped k-wide form: asked for together with the norms (the projection), a wide operand on a large shard, 10-column panels (groups
// of wg_panels = 16 then start on multiples of 160 columns), and while the slabs fit (7.7 GB at 10 M documents)
inline bool route_gl_wide_grouped(bool with_norms, int PW, int k, uint64_t D, int wg_panels, const RouteEnv& e, uint64_t total_mem, bool* ask) {
  const int ngroups = (k + PW * wg_panels - 1) / (PW * wg_panels);
  const size_t slab = (size_t)D * 12;
  return with_norms && PW == 10 && k >= 160 && D >= 16384 && e.gl_wide_grouped &&
         route_scratch_ok((double)(slab * wg_panels + (size_t)ngroups * D) * sizeof(float), total_mem, ask);
}

// ---- the stage downstream of the path (api_stages.cpp, post.hip) -------------------------------------------------------------------------
// The r-th largest value of every segment (catchword thresholds, rank thresholds of the document-topic sums).  One rank holds every
// segment whole: one workgroup per segment (post_select_k, behind post_qualify_k's slots).  Several ranks: a segment's values lie on
// different ranks, the digits are picked from histograms summed over the ranks (post_select_hist_k / post_select_step_k, behind slots
// numbered in pair order).  A communicator of one rank takes the first form: it issues the launches of a context without one.
enum PostSelect { POST_SELECT_ONE_WORKGROUP = 0, POST_SELECT_HISTOGRAM = 1 };
inline PostSelect route_post_select(int world) { return world > 1 ? POST_SELECT_HISTOGRAM : POST_SELECT_ONE_WORKGROUP; }

// The k-means objective's exact accumulation (objective.hip ob_acc_k): 2 k accumulator words and k sizes, 64-bit each, privatised per
// workgroup in LDS while they fit in 24 KB, global atomics beyond.  The sums are integer sums: the form cannot reach the result.
enum ObjAcc { OBJ_ACC_LDS = 0, OBJ_ACC_GLOBAL = 1 };
constexpr int ROUTE_OBJ_LDS_MAX_K = 1024;
inline ObjAcc route_objective_acc(int k) { return k <= ROUTE_OBJ_LDS_MAX_K ? OBJ_ACC_LDS : OBJ_ACC_GLOBAL; }
inline size_t route_objective_lds_bytes(int k) { return route_objective_acc(k) == OBJ_ACC_LDS ? 3 * (size_t)k * 8 : 0; }

// DocTopicCatchwordSums.tsv (isle_hip_doc_report_text, ISLE_DOCREPORT_TOPIC_SUMS) is one order over all documents' sums.  One rank sorts its
// range's entries and finds a line's document by a search (doc_report.hip DrSrc).  Several ranks: the keys travel with their global document,
// every rank sorts all of them and formats its slice (DrGatherSrc; stage_host.h topic_sums_slice).  A communicator of one rank takes the first.
enum TopicSums { TOPIC_SUMS_LOCAL = 0, TOPIC_SUMS_GATHERED = 1 };
inline TopicSums route_topic_sums(int world) { return world > 1 ? TOPIC_SUMS_GATHERED : TOPIC_SUMS_LOCAL; }

// ---- small EVD by tridiagonalisation (evd_tridiag.hip) -------------------------------------------------------------------------------
// workgroups of the persistent form: each holds its columns plus v and w in lds_bytes of LDS; at least gsmall (more only add barrier latency)
inline int route_td_workgroups(int n, size_t lds_bytes, int gsmall) {
  int pG = gsmall;
  const int ncl_max = (int)(lds_bytes / sizeof(double) / (size_t)n) - 2;
  if (ncl_max >= 1) pG = std::max(pG, (n + ncl_max - 1) / ncl_max);  // what the LDS needs
  else pG = 1 << 30;
  return pG;
}
// One workgroup per CU at most: all must be resident.  A time-out at the grid barrier (the GPU is shared with other work) is remembered
// (failed): later solves of the context go straight to the launch chain.  This rank's wish; several ranks agree on it.
inline bool route_td_persist(int pG, int n, int nmax_back, int num_cus, bool failed, const RouteEnv& e) {
  return pG <= num_cus && n <= nmax_back && !e.td_chain && !failed;
}
// ISLE_EVD_SPLIT=1 with several ranks: rank r computes the eigenvectors [v0, v1) = [r kc, (r + 1) kc) and the columns are all-gathered;
// kc == 0: every rank computes all of them (also where the gathered block would not fit the caller's n x n array)
struct TdSplit {
  int v0, v1, kc;
};
inline TdSplit route_td_split(bool multi, int world, int rank, int nvec, int n, const RouteEnv& e) {
  TdSplit s = {0, nvec, 0};
  if (multi && e.evd_split) {
    s.kc = ((nvec + world - 1) / world + 7) & ~7;
    if ((size_t)s.kc * world <= (size_t)n) {
      s.v0 = std::min(nvec, rank * s.kc);
      s.v1 = std::min(nvec, s.v0 + s.kc);
    } else {
      s.kc = 0;
    }
  }
  return s;
}
// the eigenvectors' back-transformation: blocks of four reflectors in compact WY form, or (ISLE_TD_BACK=seq) reflector by reflector with
// eight eigenvectors per workgroup, four where there are few (twice the workgroups, half the rows per thread)
enum TdBack { TD_BACK_WY, TD_BACK_SEQ8, TD_BACK_SEQ4 };
inline TdBack route_td_back(int nvec, int num_cus, int kc, const RouteEnv& e) {
  if (!e.td_back) return TD_BACK_WY;
  return (nvec + 7) / 8 > num_cus / 2 && !kc ? TD_BACK_SEQ8 : TD_BACK_SEQ4;
}

// ---- the vocabulary pruned by document frequency (api_stages.cpp, vocab.hip) ------------------------------------------------------------
// The document frequencies of A (vocab.hip, isle_hip_word_doc_freq / isle_hip_prune_vocab): 32-bit counters private to a workgroup in LDS
// over vocabulary parts, flushed with one global atomic per (workgroup, word), or one global atomic per entry.  Integer sums: the form
// cannot reach the result.  asked: the context's setting (isle_hip_vocab_hist_form: 0 this rule's choice, 1 LDS, 2 global atomics).  The LDS
// form is the choice: 0.54 ms against 4.9 ms of device time on the 108 M entries of config 2 (V = 50 k: four parts; medians of 5, the two
// forms alternating; tools/vocab_prune_probe.py, profiles/vocab_prune_c2.jsonl).  Not measured: a vocabulary of many more parts.
enum VocabHist { VOCAB_FORM_LDS = 0, VOCAB_FORM_GLOBAL = 1 };
inline VocabHist route_vocab_hist(int asked) { return asked == 2 ? VOCAB_FORM_GLOBAL : VOCAB_FORM_LDS; }

// ---- documents pruned by length and as exact duplicates (api_stages.cpp, docs.hip) -------------------------------------------------------
// The key the documents are sorted by before their contents are compared run by run (docs_host.h): the 64-bit hash, or the same hash cut
// to DOCS_NARROW_BITS bits so that every run holds many unequal documents.  Equality of content decides either way: the form cannot reach
// the result, only the number of rounds.  asked: the context's setting (isle_hip_doc_hash_form: 0 this rule's choice, 1 full, 2 narrow).
// The full hash is the choice: one round where no two unequal documents collide.  On the first 20 000 documents of config 2 0.35 ms
// against 754 ms of wall time (medians of 5; tools/docs_prune_probe.py, profiles/docs_prune_c2.jsonl); the narrow form exists for the tests.
enum DocHash { DOC_FORM_FULL = 0, DOC_FORM_NARROW = 1 };
inline DocHash route_doc_hash(int asked) { return asked == 2 ? DOC_FORM_NARROW : DOC_FORM_FULL; }

// ---- two topic models compared (api_stages.cpp, model_compare.hip) --------------------------------------------------------------------------
#include "match_host.h"  // MC_TILE, MC_CHUNK, mc_slices (included here: tests cite lines above by number)
// The word slices of mc_dist_k (match_host.h states the arithmetic, mc_slices): ceil(ka / MC_TILE) ceil(kb / MC_TILE) pair tiles are 256
// workgroups at k = 1000 and 16 at k = 200, so the words are cut into enough slices, each a multiple of MC_CHUNK words, that every compute
// unit gets MC_SLICE_WAVES workgroups; the slices' partial matrices are added in ascending slice order by mc_reduce_k, and with one slice
// none is written.  asked: the context's setting (isle_hip_model_dist_slices: 0 this rule's choice, >= 1 forced).  The slices fix the order
// of summation and nothing else: where every sum is exactly representable the bits are the same for every count.  README for what was
// measured.
inline uint32_t route_model_dist_slices(uint64_t V, int ka, int kb, int num_cus, int asked = 0) { return mc_slices(V, ka, kb, num_cus, asked); }

// ---- the documents most similar to a query document (api_stages.cpp, similar_docs.hip) -----------------------------------------------------
// The home of the query table of isle_hip_similar_docs (num_topics x Qp fp32, Qp = Q rounded up to a power of two; simdocs_host.h): LDS,
// copied once per workgroup, while the table fits in SIMDOCS_LDS_TABLE_BYTES, else global memory (256 KiB at num_topics = 1024, Q = 64: it
// stays in L2).  64 KiB is TOPDOCS_LDS_BINS_BYTES's budget and reasoning: two workgroups in the 160 KiB of a CU.  Both homes hold the same
// words and give the same bits.  asked: the context's setting (isle_hip_simdocs_table_form: 0 this rule's choice, 1 LDS, 2 global); LDS
// where the table does not fit the budget is global all the same.  THE THRESHOLD IS A CHOICE THAT THE ONE MEASUREMENT DOES NOT SUPPORT: at
// Q = 64, num_topics = 200 (a 51 KiB table, config 2, 1 M rows, cosine, the two homes alternating, medians of 5; tools/similar_docs_probe.py,
// profiles/similar_docs_c2.jsonl) the GLOBAL home was the faster one, 6.65 ms against 8.68 ms of device time on the 27.3 M catchword sums
// and 1.04 ms against 1.84 ms on the 1.31 M inference entries.  A 51 KiB table leaves three workgroups of four waves on a compute unit and
// the LDS launch is capped at two workgroups per unit, where the global form runs eight; whether a smaller table (fewer queries, fewer
// topics) turns the order round, and whether the LDS form with larger workgroups catches up, IS NOT MEASURED.  The rule stays as stated.
enum SimdocsTable { SIMDOCS_HOME_LDS = 0, SIMDOCS_HOME_GLOBAL = 1 };
constexpr uint64_t SIMDOCS_LDS_TABLE_BYTES = 64 * 1024;
inline SimdocsTable route_simdocs_table(int Q, uint64_t num_topics, int asked) {
  uint64_t qp = 1;
  while (qp < (uint64_t)Q) qp <<= 1;
  if (asked == 2) return SIMDOCS_HOME_GLOBAL;
  return num_topics * qp * 4 <= SIMDOCS_LDS_TABLE_BYTES ? SIMDOCS_HOME_LDS : SIMDOCS_HOME_GLOBAL;
}

// ---- near-duplicate documents by MinHash (api_stages.cpp, near_dups.hip) ---------------------------------------------------------------------
// The key the live documents of a band are sorted by before the exact Jaccard test runs inside every run of equal keys (neardup_host.h):
// the band's 64-bit key, or the same key cut to DOCS_NARROW_BITS bits so that every run holds many dissimilar documents.  Unlike the exact
// duplicates' hash the form CAN reach the result where num < den: it decides which pairs become candidates, and each form is held to the
// rule's statement of that form; with num == den both give "equal word sets".  asked: the context's setting (isle_hip_neardup_key_form: 0
// this rule's choice, 1 full, 2 narrow).  The full key is the choice: it is what banding means, and a run then holds candidates alone;
// the narrow form exists for the tests.  Not measured: the narrow form at size.
enum NdKey { ND_FORM_FULL = 0, ND_FORM_NARROW = 1 };
inline NdKey route_neardup_key(int asked) { return asked == 2 ? ND_FORM_NARROW : ND_FORM_FULL; }
