// isle_amd/csrc/api_kmeans.cpp — k-means++ in span(U), Lloyd in span(U), the lift and Lloyd on B behind the C ABI
// (kmeanspp_on_projected_space src/sparseMatrix.cpp:2133-2209, run_lloyds_on_projected_space :2016-2072, left_multiply_by_U_Spectra
// :1438-1450, run_lloyds :1690-1746): the reference's draw schedule, stop rules and iteration structure on the host, the arithmetic in
// kmeans.hip / spmm.hip / dense.hip / gram_lds.hip.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdlib>
#include <cstring>
#include <numeric>

#include "api_internal.h"

#ifndef ISLE_PROJ_FULL_NUM
// Lloyd in span(U): a full pass instead of the active rows' products when more than NUM / DEN of the documents are active.  A third since round 5
// (a half before): at config 3 the loop takes 187 ms with 1/2, 166 with 1/3 and 1/4, 199 with 1/6, 214 with 1/10 (the full product costs
// 5.5 ns a document, the compaction + tile products of the active rows 15 - 20 ns an active document, and a full pass refreshes every bound)
#define ISLE_PROJ_FULL_NUM 1
#define ISLE_PROJ_FULL_DEN 3
#endif
// ------------------------------------------------------------------------------------------
// k-means in the projected space
// ------------------------------------------------------------------------------------------
// The movers of an iteration (YyMovers): up to ten centres whose movement stands out — more than twice the eleventh largest — and the
// groups' (Yinyang: 8 centres) or tiles' (projected loop: 32) largest movements WITHOUT them.  The same on every rank (replicated inputs).
static void choose_movers(const std::vector<float>& delta, int k, int group, int G, YyMovers* mv, std::vector<float>* gmax_excl,
                          const std::vector<uint32_t>* slot_of_id = nullptr /*regrouped Yinyang groups: centre i sits in group slot_of_id[i] / group*/) {
  mv->n = 0;
  if ((int)delta.size() != k || k <= 16) return;
  std::vector<int> ord(k);
  std::iota(ord.begin(), ord.end(), 0);
  std::partial_sort(ord.begin(), ord.begin() + 11, ord.end(), [&](int a, int b) { return delta[a] > delta[b] || (delta[a] == delta[b] && a < b); });
  const float ref = delta[ord[10]];
  for (int j = 0; j < 10; ++j)
    if (delta[ord[j]] > 2.0f * ref && delta[ord[j]] > 1e-4f) mv->id[mv->n++] = (uint32_t)ord[j];
  if (!mv->n) return;
  mv->ld = 4 * ((mv->n + 3) / 4);
  gmax_excl->assign(G, 0.f);
  for (int i = 0; i < k; ++i) {
    bool is_mover = false;
    for (int j = 0; j < mv->n; ++j) is_mover = is_mover || mv->id[j] == (uint32_t)i;
    const int gi = (int)(slot_of_id ? (*slot_of_id)[i] : (uint32_t)i) / group;
    if (!is_mover) (*gmax_excl)[gi] = std::max((*gmax_excl)[gi], delta[i]);
  }
}

static int trace_objective(isle_ctx* c, int space, int k);  // isle_hip_lloyds_trace: below, with the objective

static int ensure_P(isle_ctx* c, int k) {
  if (c->res.U_k != k) return isle_fail(c, ISLE_E_ARG, "U has %d columns, k = %d (run isle_hip_block_ks / set_U first)", c->res.U_k, k);
  if (c->res.P_ready) return 0;
  const size_t D = c->D ? c->D : 1;
  HIPCHK(c, c->P.reserve(D * c->ldk));
  HIPCHK(c, c->pnorm.reserve(D));
  c->res.projection_begins();
  // Where the assignment products run with their epilogues inside (a large shard) they read the projection's two bf16 terms in the layout
  // the LDS-DMA product stages (gemm_bf16x2_dma_k).  The grouped projection writes that copy on its way, by POSITION (the products map their
  // rows to documents through dperm): no transposition and no split pass behind the projection (round 5: 15 + 15 ms at config 3).
  const bool want_a2 = route_want_a2(c->D, k, c->route);
  bool a2_done = false;
  if (want_a2) HIPCHK(c, c->Pt2.reserve(k_gemm_split_a_bytes(c->D, k) / sizeof(uint4)));
  ISLECHK(k_spmm_wide_project(c, c->Urm.p, k, c->ldk, c->P.p, c->pnorm.p, want_a2 ? c->Pt2.p : nullptr, &a2_done));
  c->res.projection_made(a2_done);
  if (!a2_done && c->D) {  // (with the split copy by position, the f32 coordinate-major copy is made when a route asks for it: k_ensure_pt)
    TimeScope ts(c, ISLE_T_PROJECT);
    ISLECHK(k_ensure_pt(c));
    if (want_a2) {  // the projection took another route than the grouped one: split the transposed copy
      ISLECHK(k_gemm_split_a(c, c->Pt.p, c->D, k, c->Pt2.p));
      c->res.split_copy_made();
    }
  }
  return 0;
}

// dst (n x ldk, device) <- P rows of the given GLOBAL doc ids (owner contributes, others zero, then all-reduce)
static int fetch_rows(isle_ctx* c, const uint64_t* ids, int n, float* dst) {
  if (n == 0) return 0;
  const bool multi = c->multi();
  std::vector<uint64_t> local(n);
  for (int i = 0; i < n; ++i) {
    const uint64_t g = ids[i];
    if (g >= c->doc_offset && g < c->doc_offset + c->D) local[i] = g - c->doc_offset;
    else if (multi) local[i] = ~0ull;  // another rank's document: zeros here, the all-reduce brings the row
    else return isle_fail(c, ISLE_E_ARG, "seed doc id %llu out of range", (unsigned long long)g);
  }
  ISLECHK(k_fetch_rows(c, c->P.p, c->ldk, local.data(), n, dst));  // one kernel (the ids travel as arguments), not one copy per row
  if (multi) ISLECHK(allreduce_sum<float>(c, dst, (size_t)n * c->ldk));
  return 0;
}

// the k x k centres of the C ABI <-> the k x ldk rows the device keeps, through the page-locked staging
static void centres_pack(float* Ch, const float* C_lowd, int k, int ldk) {
  if (ldk != k) memset(Ch, 0, (size_t)k * ldk * sizeof(float));
  for (int cc = 0; cc < k; ++cc) memcpy(Ch + (size_t)cc * ldk, C_lowd + (size_t)cc * k, (size_t)k * sizeof(float));
}
static void centres_unpack(float* C_lowd, const float* Ch, int k, int ldk) {
  for (int cc = 0; cc < k; ++cc) memcpy(C_lowd + (size_t)cc * k, Ch + (size_t)cc * ldk, (size_t)k * sizeof(float));
}

namespace {
// page-locked staging for the per-round scalars (IslePinSmall::kmpp_stage): [my 2 | tot 2 * world | local maxdraw] doubles, then drawn
// maxdraw u64, then the 42 words of the device's search
struct KmppStage {
  double *my, *tot, *local;
  uint64_t *drawn, *res;
};
// device scalars of the rounds, carved out of c->gram (1024 doubles)
struct KmppScalars {
  double* gather;   // [0, 2 * world]: the ranks' totals, then this rank's own (allgather_host)
  double* dice;     // 64: the dice of a round beyond 16
  uint64_t* found;  // 128: the positions found
  double* totals;   // 200: this rank's {sum of the distances, last distance}
};
}  // namespace
static KmppScalars kmpp_scalars(isle_ctx* c) { return {c->gram.p, c->gram.p + 64, (uint64_t*)(c->gram.p + 128), c->gram.p + 200}; }

// one rank: the dice are products of the total with host-drawn fractions, so the device can throw them itself — the totals, the
// dice and their search come back in one copy (search_frac_k), one host round trip per round
static int kmpp_draw_on_device(isle_ctx* c, HostRng& rng, int ndraw, std::vector<double>& dice, const KmppStage& st, double* grand, double* last_md) {
  const uint64_t D = c->D;
  for (int i = 0; i < ndraw; ++i) dice[i] = rng.fraction();  // :2184
  // the kernel writes its 42 words straight into the page-locked area (host memory mapped into the device's address space): no
  // copy kernel, and one gap less, between the search and the host's wake-up
  ISLECHK(k_search_frac(c, c->cum.p, D, D > 0 ? c->min_dist.p + (D - 1) : nullptr, dice.data(), ndraw, st.res));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  memcpy(st.my, st.res + 40, 2 * sizeof(double));
  *grand = st.my[0];
  *last_md = st.my[1];
  for (int i = 0; i < ndraw; ++i) st.drawn[i] = std::min<uint64_t>(st.res[i], D - 1) + c->doc_offset;
  return 0;
}

// several ranks (or injected seeds, or the switch): the ranks' totals are gathered, all ranks draw the same dice and the owner of a die's
// interval searches its local prefix sums
static int kmpp_draw_by_ranks(isle_ctx* c, HostRng& rng, int ndraw, bool injected, std::vector<double>& dice, const KmppStage& st, double* grand,
                              double* last_md) {
  const uint64_t D = c->D;
  const KmppScalars sc = kmpp_scalars(c);
  // totals (per rank) -> offsets
  st.my[0] = st.my[1] = 0.0;
  // the second scalar is the last distance of the CORPUS: only the rank that holds its last document reports one (the ranks behind it
  // hold no document at all and report 0, as do the ranks before it)
  const bool holds_last = D > 0 && c->doc_offset + D == c->D_global;
  ISLECHK(k_pack2(c, c->cum.p + D, holds_last ? c->min_dist.p + (D - 1) : nullptr, sc.totals));
  HIPCHK(c, hipMemcpyAsync(st.my, sc.totals, 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));  // one copy, one round trip for both scalars
  for (int r = 0; r < 2 * c->world; ++r) st.tot[r] = 0.0;
  ISLECHK(allgather_host<double>(c, st.my, 2, sc.gather, st.tot));
  *grand = 0.0;
  double my_off = 0.0;
  for (int r = 0; r < c->world; ++r) {
    if (r == c->rank) my_off = *grand;
    *grand += st.tot[2 * r];
  }
  *last_md = 0.0;
  for (int r = 0; r < c->world; ++r) *last_md += st.tot[2 * r + 1];  // one rank's, whichever holds the last document (not rank world - 1 when its shard is empty)
  if (injected) return 0;
  // all ranks draw the same dice; the owner of the interval searches its local prefix sums
  for (int i = 0; i < ndraw; ++i) {
    dice[i] = *grand * rng.fraction();  // :2184
    const double x = dice[i] - my_off;
    // a die that no interval holds (the total is zero, or the fraction rounded to 1) is the last document's, as the search's clamp
    // makes it on one rank: the rank that holds that document answers
    const bool mine = (x >= 0.0 && x < st.my[0]) || (c->world == 1) || (holds_last && dice[i] >= *grand);
    st.local[i] = mine ? std::min(std::max(x, 0.0), st.my[0]) : -1.0;
  }
  if (ndraw <= 16) {
    ISLECHK(k_search_args(c, c->cum.p, D, st.local, ndraw, sc.found));  // dice as kernel arguments
  } else {
    HIPCHK(c, hipMemcpyAsync(sc.dice, st.local, ndraw * sizeof(double), hipMemcpyHostToDevice, c->stream));  // `local` outlives the sync below
    ISLECHK(k_search(c, c->cum.p, D, sc.dice, ndraw, sc.found));
  }
  HIPCHK(c, hipMemcpyAsync(st.drawn, sc.found, ndraw * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < ndraw; ++i) {
    if (st.local[i] < 0.0 || D == 0) st.drawn[i] = 0;
    else st.drawn[i] = std::min<uint64_t>(st.drawn[i], D - 1) + c->doc_offset + 1;  // +1: zero means "not mine"
  }
  ISLECHK(allreduce_host<uint64_t>(c, st.drawn, ndraw, sc.found));
  for (int i = 0; i < ndraw; ++i) st.drawn[i] = st.drawn[i] ? st.drawn[i] - 1 : 0;
  return 0;
}

extern "C" int isle_hip_kmeanspp_projected(isle_ctx* c, int k, const uint64_t* inject, uint64_t rng_seed, uint64_t* seeds_out,
                                           float* C_lowd, float* residual, int* rounds_out) {
  if (!c || !seeds_out || !C_lowd || k < 1) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  if ((uint64_t)k > c->D_global) return isle_fail(c, ISLE_E_ARG, "k > number of documents");
  const KmppPlan plan = route_kmpp_plan(k, c->multi(), inject != nullptr, c->route);
  isle_host_mark("kmeanspp: entry");
  ISLECHK(ensure_P(c, k));  // compute_projected_docs_l2sq :2144
  isle_host_mark("kmeanspp: projection enqueued");
  const uint64_t D = c->D, Dg = c->D_global;
  const int ldk = c->ldk;
  HIPCHK(c, c->min_dist.reserve(D ? D : 1));
  HIPCHK(c, c->cum.reserve(D + 1));
  HIPCHK(c, c->Cdev.reserve((size_t)k * ldk));
  HIPCHK(c, c->gram.reserve(1024));
  HIPCHK(c, c->small.reserve(4096));
  ISLECHK(k_fill_f32(c, c->min_dist.p, D, 3.402823466e+38f));  // FP_MAX :2148
  HostRng rng(rng_seed);
  std::vector<uint64_t> centers;
  const uint64_t first = inject ? inject[0] : (uint64_t)(((size_t)rng.next31() * (size_t)84619573) % (size_t)Dg);  // :2150
  centers.push_back(first);
  c->res.kmpp_begins();  // Cdev holds seeds from here on
  ISLECHK(fetch_rows(c, &first, 1, c->Cdev.p));
  int new_added = 1, rounds = 0;
  double grand = 0.0, last_md = 0.0;
  std::vector<double> dice(plan.maxdraw);
  IslePinSmall* pin = c->pin_small();
  if ((size_t)(2 + 2 * c->world + 2 * plan.maxdraw + 42) * 8 > sizeof(pin->kmpp_stage)) return isle_fail(c, ISLE_E_ARG, "k-means++: staging area too small");
  KmppStage st;
  st.my = pin->kmpp_stage;
  st.tot = st.my + 2;
  st.local = st.tot + 2 * c->world;
  st.drawn = reinterpret_cast<uint64_t*>(st.local + plan.maxdraw);
  st.res = st.drawn + plan.maxdraw;  // 42 entries
  while ((int)centers.size() < k) {
    rounds++;
    ISLECHK(k_kmpp_update(c, c->P.p, c->pnorm.p, D, k, ldk, c->Cdev.p + (centers.size() - new_added) * (size_t)ldk, new_added,
                          c->min_dist.p, (int)(centers.size() - new_added), plan.track));
    ISLECHK(k_scan_f2d(c, c->min_dist.p, D, c->cum.p));  // :2170-2172 (double, parallel; the reference's is fp32 sequential)
    const int s = (int)centers.size();
    int ndraw = 0;
    for (int cc = 0; cc < 1 + std::sqrt((double)(s - 5 > 0 ? s - 5 : 0)); ++cc) ndraw++;  // :2183 (upper bound on draws)
    ndraw = std::min(ndraw, plan.maxdraw);
    if (plan.device_dice && ndraw <= 40) ISLECHK(kmpp_draw_on_device(c, rng, ndraw, dice, st, &grand, &last_md));
    else ISLECHK(kmpp_draw_by_ranks(c, rng, ndraw, inject != nullptr, dice, st, &grand, &last_md));
    new_added = 0;
    std::vector<uint64_t> fresh;
    for (int cc = 0; cc < ndraw && (int)centers.size() < k; ++cc) {
      const uint64_t nc = inject ? inject[centers.size()] : st.drawn[cc];
      if (std::find(centers.begin(), centers.end(), nc) == centers.end()) {  // duplicates skipped, not redrawn :2189
        centers.push_back(nc);
        fresh.push_back(nc);
        new_added++;
      }
    }
    if (new_added) ISLECHK(fetch_rows(c, fresh.data(), new_added, c->Cdev.p + (centers.size() - new_added) * (size_t)ldk));
    if (inject && new_added == 0) return isle_fail(c, ISLE_E_ARG, "injected seeds contain duplicates");
    if (rounds > 100 * k) return isle_fail(c, ISLE_E_NUMERIC, "k-means++ cannot find %d distinct seeds", k);
  }
  isle_host_mark("kmeanspp: rounds done");
  // the last batch of seeds is never folded into min_dist (the loop ends when the k-th seed is drawn, :2163-2207); for Lloyd's first
  // assignment it is folded into a COPY of the distances
  if (plan.track && c->kmpp_track && new_added > 0 && c->kmpp_track_seeds == k - new_added && D > 0) {
    HIPCHK(c, c->kmpp_best.reserve(D));
    HIPCHK(c, hipMemcpyAsync(c->kmpp_best.p, c->min_dist.p, D * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    ISLECHK(k_kmpp_update(c, c->P.p, c->pnorm.p, D, k, ldk, c->Cdev.p + (size_t)(k - new_added) * ldk, new_added, c->kmpp_best.p, k - new_added, true));
  }
  // best_centers_coords[c] = U^T b_seed[c]  (:2232-2234)
  const size_t ch_bytes = (size_t)k * ldk * sizeof(float);
  HIPCHK(c, c->pin_stage.reserve(ch_bytes));
  HIPCHK(c, hipMemcpyAsync(c->pin_stage.p, c->Cdev.p, ch_bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::copy(centers.begin(), centers.end(), seeds_out);
  centres_unpack(C_lowd, reinterpret_cast<const float*>(c->pin_stage.p), k, ldk);
  if (residual) *residual = (float)(grand - last_md);  // dist_cumul[num_docs - 1]  (:2208; App. C #9)
  if (rounds_out) *rounds_out = rounds;
  if (plan.track && c->kmpp_track && c->kmpp_track_seeds == k) {  // complete: Lloyd may start from it if it is handed exactly these centres
    c->kmpp_C_host.assign(C_lowd, C_lowd + (size_t)k * k);
    c->res.kmpp_kept_first_assignment(k);
  }
  isle_host_mark("kmeanspp: exit");
  return 0;
}

extern "C" int isle_hip_get_min_dist(isle_ctx* c, float* out) {
  if (!c || !out) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  if (c->D) HIPCHK(c, hipMemcpy(out, c->min_dist.p, c->D * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

// The reference's stop rule (src/sparseMatrix.cpp:2044-2064 / :1718-1738): converged when the cluster
// sizes equal the previous iteration's AND the partition equals the last partition stored on an
// iteration whose sizes matched.
namespace {
struct StopRule {
  isle_ctx* c;
  int k;
  std::vector<long long> prev_sizes;
  bool have_prev = false;
  StopRule(isle_ctx* c_, int k_) : c(c_), k(k_), prev_sizes(k_, 0) {}
  // sizes: GLOBAL cluster sizes of this iteration.  assign: device, local docs.
  int converged(const std::vector<long long>& sizes, const uint32_t* assign, bool* out) {
    bool changed = false;
    for (int i = 0; i < k; ++i)
      if (prev_sizes[i] != sizes[i]) changed = true;
    prev_sizes = sizes;
    if (!changed) {
      if (!have_prev) {
        changed = c->D_global > 0;  // prev_closest_docs are k empty lists
      } else {
        HIPCHK(c, c->flags.reserve(16));
        ISLECHK(k_compare_u32(c, assign, c->assign_prev.p, c->D, c->flags.p));
        ISLECHK(allreduce_sum<int>(c, c->flags.p, 1));
        uint32_t differ = 0;
        ISLECHK(isle_fetch_u32(c, reinterpret_cast<const uint32_t*>(c->flags.p), &c->pin_small()->stop_flag, &differ));
        changed = differ != 0;
      }
      HIPCHK(c, c->assign_prev.reserve(c->D ? c->D : 1));
      if (c->D) HIPCHK(c, hipMemcpyAsync(c->assign_prev.p, assign, c->D * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
      have_prev = true;
    }
    *out = !changed;
    return 0;
  }
};
}  // namespace

static int fetch_sizes(isle_ctx* c, int k, std::vector<long long>& sizes) {
  ISLECHK(allreduce_sum<int>(c, c->counts.p, k));
  std::vector<int> hv;
  int* h = c->pin_small()->cluster_sizes;  // page-locked, 64 KB
  if ((size_t)k * sizeof(int) > sizeof(c->pin_small()->cluster_sizes)) {
    hv.resize(k);
    h = hv.data();
  }
  HIPCHK(c, hipMemcpyAsync(h, c->counts.p, (size_t)k * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  sizes.assign(h, h + k);
  return 0;
}

// The k centre movements of the last update, on the host for choose_movers: through the page-locked area and behind a stream
// synchronisation of its own (the stop rule synchronises only when the cluster sizes stayed the same)
static int fetch_delta(isle_ctx* c, const float* delta_dev, int k, std::vector<float>& out) {
  out.resize(k);
  float* h = c->pin_small()->movements;  // page-locked, 32 KB
  if ((size_t)k * sizeof(float) > sizeof(c->pin_small()->movements)) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out.data(), delta_dev, (size_t)k * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
  }
  HIPCHK(c, hipMemcpyAsync(h, delta_dev, (size_t)k * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  memcpy(out.data(), h, (size_t)k * sizeof(float));
  return 0;
}

// The movers of the coming re-examination, chosen from the last update's movements, and the groups' largest movements without them on
// their way to c->yy_gmax2 (mv->n > 0).  `excl` is the caller's: it synchronises the stream before the vector dies.
static int prepare_movers(isle_ctx* c, const std::vector<float>& delta, int k, int group, int G, const std::vector<uint32_t>* slot_of_id, YyMovers* mv,
                          std::vector<float>* excl) {
  choose_movers(delta, k, group, G, mv, excl, slot_of_id);
  if (!mv->n) return 0;
  HIPCHK(c, c->yy_gmax2.reserve(std::max(G, 64)));
  HIPCHK(c, hipMemcpyAsync(c->yy_gmax2.p, excl->data(), (size_t)G * sizeof(float), hipMemcpyHostToDevice, c->stream));
  return 0;
}

// ------------------------------------------------------------------------------------------
// Lloyd in span(U)
// ------------------------------------------------------------------------------------------
namespace {
// device scalars of the loop, behind the previous centres in c->Cold and in c->small
struct ProjScalars {
  float* delta;  // k movements (Cold + k * ldk)
  HamTop* top;   // their top two (behind the movements, 16-byte aligned)
  float* tmove;  // T tile maxima (small)
};
}  // namespace

// the route decisions of one call (route_host.h ProjPlan), taken once behind ensure_P: the switches are read at isle_enter only
static ProjPlan proj_plan(isle_ctx* c, int k, const float* C_lowd) {
  const bool seeds_kept = c->kmpp_C_host.size() == (size_t)k * k && memcmp(c->kmpp_C_host.data(), C_lowd, (size_t)k * k * sizeof(float)) == 0;
  const ProjFacts f = {c->D, c->res.Pt_ready, c->res.Pt2_ready(), c->res.P_ready, c->res.kmpp_track_k, c->res.kmpp_same_P(), seeds_kept};
  return route_proj_plan(f, k, c->route);
}

static int proj_reserve(isle_ctx* c, const ProjPlan& p, int k, ProjScalars* sc) {
  const uint64_t D = c->D;
  const int ldk = c->ldk;
  if (p.hamerly) {
    HIPCHK(c, c->hub.reserve(D ? D : 1));
    HIPCHK(c, c->hlb.reserve(D ? D : 1));
    HIPCHK(c, c->active.reserve(D + 1));
    HIPCHK(c, c->Pa.reserve((size_t)(D ? D : 1) * ldk));
    HIPCHK(c, c->pna.reserve(D ? D : 1));
    HIPCHK(c, c->Cold.reserve((size_t)k * ldk + k + 8));
  }
  if (p.tiles) {
    HIPCHK(c, c->ptlb.reserve((size_t)(D ? D : 1) * p.TL));
    HIPCHK(c, c->pneed.reserve(D ? D : 1));
    HIPCHK(c, c->pcand.reserve(D + 1));
    HIPCHK(c, c->small.reserve(4096));
  }
  if (p.delta_sums) HIPCHK(c, c->proj_counted.reserve(D ? D : 1));
  if (c->multi()) HIPCHK(c, c->Csum_local.reserve((size_t)k * ldk));
  sc->delta = p.hamerly ? c->Cold.p + (size_t)k * ldk : nullptr;
  sc->top = p.hamerly ? reinterpret_cast<HamTop*>(c->Cold.p + (size_t)k * ldk + round4(k)) : nullptr;
  sc->tmove = p.tiles ? c->small.p : nullptr;
  return 0;
}

// every document against every centre: the first iteration, and every iteration of the loop without bounds
static int proj_assign_first(isle_ctx* c, const ProjPlan& p, int k) {
  const uint64_t D = c->D;
  const int ldk = c->ldk;
  // the centres are the k-means++ seeds and the rounds kept every document's nearest seed, its tile's runner-up and the minimum of
  // every other tile: exactly this assignment (up to the rounding of the two distance evaluations, inside the bounds' slack)
  if (p.from_kmpp) return k_kmpp_to_tiles(c, D, k, c->pnorm.p, c->cnorm.p, c->kmpp_best.p, c->assign.p, c->hub.p, p.TL);
  if (p.tiles)
    return k_proj_assign_tiles(c, c->P.p, c->pnorm.p, D, k, ldk, c->Cdev.p, c->cnorm.p, c->assign.p, c->hub.p, c->ptlb.p, p.TL, nullptr, 0, nullptr, nullptr,
                               nullptr);  // :1947
  return k_proj_assign(c, c->P.p, c->pnorm.p, D, k, ldk, c->Cdev.p, c->cnorm.p, c->assign.p, p.hamerly ? c->hub.p : nullptr,
                       p.hamerly ? c->hlb.p : nullptr);  // :1947
}

// ISLE_DEBUG_HAMERLY: how many tiles the active documents ask for
static int debug_tile_stats(isle_ctx* c, int it, uint32_t na, int T) {
  const uint64_t D = c->D;
  std::vector<uint32_t> act(na), need(D);
  if (na) HIPCHK(c, hipMemcpy(act.data(), c->active.p, na * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (D) HIPCHK(c, hipMemcpy(need.data(), c->pneed.p, D * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (route_pt_sort(true, na, c->route))  // the order k_proj_assign_tiles gives the list
    std::stable_sort(act.begin(), act.end(), [&](uint32_t a, uint32_t b) { return need[a] < need[b]; });
  double tiles_sum = 0, union_sum = 0;
  for (uint32_t i = 0; i < na; i += 128) {
    uint32_t u = 0;
    for (uint32_t j = i; j < std::min(na, i + 128); ++j) {
      tiles_sum += __builtin_popcount(need[act[j]]);
      u |= need[act[j]];
    }
    union_sum += __builtin_popcount(u);
  }
  fprintf(stderr, "[tile bounds, projected] iter %d active %u of %llu, tiles per document %.1f, per workgroup (union) %.1f of %d\n", it, na,
          (unsigned long long)D, na ? tiles_sum / na : 0.0, na ? union_sum / ((na + 127) / 128) : 0.0, T);
  return 0;
}

// Tile bounds: candidates by the grown upper bounds, then the exact distance to the own centre for those (pt_tighten_k), then the
// active documents against the tiles they need — or all documents against all centres where most are active.  Documents are taken
// grouped by their centre (member lists of the previous iteration): a workgroup of the re-examination then holds neighbours, whose
// needed tiles coincide.
static int proj_reassign_tiles(isle_ctx* c, const ProjPlan& p, const ProjScalars& sc, int k, int it, const std::vector<float>& pdelta_host) {
  const uint64_t D = c->D;
  const int ldk = c->ldk, T = p.T, TL = p.TL;
  uint32_t* nact = c->active.p + D;
  uint32_t* ncand = c->pcand.p + D;
  // movers (see Lloyd on B below): a tile of 32 centres loses its bound to ONE centre that jumped; up to ten such centres are left out
  // of their tiles' movements and bounded by their exact new distances  P_d . c = b_d^T (U c): a thin product of B with U C_m^T
  // (the k-means++ rounds' route), one pass of the pass-1 stream
  YyMovers mv;
  const float* tmove_use = sc.tmove;
  if (p.movers && c->res.thin_product_possible(k)) {
    std::vector<float> tm;
    ISLECHK(prepare_movers(c, pdelta_host, k, 32, T, nullptr, &mv, &tm));
    if (mv.n) {
      HIPCHK(c, c->Tmp.reserve((size_t)c->V * 32 + (size_t)16 * ldk));
      float* Cm = c->Tmp.p + (size_t)c->V * 32;  // the movers' centres, one row each
      for (int j = 0; j < mv.n; ++j)
        HIPCHK(c, hipMemcpyAsync(Cm + (size_t)j * ldk, c->Cdev.p + (size_t)mv.id[j] * ldk, (size_t)ldk * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));  // tm is stack-owned
      HIPCHK(c, c->yy_mdots.reserve((size_t)D * mv.ld));
      ISLECHK(k_gemm_nn(c, c->Ucm.p, c->V, k, Cm, ldk, mv.n, c->Tmp.p, ISLE_T_LLOYD_PROJ));  // W = U C_m^T  (V x n col-major)
      {
        TimeScope ts(c, ISLE_T_LLOYD_PROJ);
        ISLECHK(k_gl_thin(c, c->Tmp.p, mv.n, mv.ld, c->yy_mdots.p, true));  // rows by position: pt_filter_k reads them through dpos
      }
      tmove_use = c->yy_gmax2.p;
    }
  }
  ISLECHK(k_pt_filter(c, p.pt_sorted ? nullptr : (c->res.members_valid ? c->members.p : nullptr), c->assign.p, c->hub.p, c->ptlb.p, T, TL, sc.delta, tmove_use,
                      c->pneed.p, c->pcand.p, ncand, mv, c->yy_mdots.p, c->cnorm.p, c->pnorm.p));
  ISLECHK(k_pt_tighten(c, c->P.p, c->pnorm.p, ldk, c->Cdev.p, c->cnorm.p, c->assign.p, c->pcand.p, ncand, c->hub.p, c->ptlb.p, T, TL, c->pneed.p,
                       c->active.p, nact));
  uint32_t na = 0;
  ISLECHK(isle_fetch_u32(c, nact, &c->pin_small()->active_count, &na));
  if (c->knob_on(KN_DEBUG_HAMERLY)) ISLECHK(debug_tile_stats(c, it, na, T));
  // (measured with the product on the gathered rows of the active documents: handing the full pass over only beyond 3/4 of the documents
  // is slower, 222 against 187 ms at config 3 — gathering 5.4 M rows costs what the product saves, and the full pass refreshes every bound)
  if ((uint64_t)na * ISLE_PROJ_FULL_DEN > (uint64_t)D * ISLE_PROJ_FULL_NUM && k_proj_full_by_gemm(c, D, k))  // most documents are up for re-examination: the full GEMM pass costs less than
    return k_proj_assign_tiles(c, c->P.p, c->pnorm.p, D, k, ldk, c->Cdev.p, c->cnorm.p, c->assign.p, c->hub.p, c->ptlb.p, TL, nullptr, 0, nullptr, nullptr,
                               nullptr);  // compacting them and walking their tiles, and refreshes every bound
  return k_proj_assign_tiles(c, c->P.p, c->pnorm.p, D, k, ldk, c->Cdev.p, c->cnorm.p, c->assign.p, c->hub.p, c->ptlb.p, TL, c->active.p, na, c->pneed.p, c->Pa.p,
                             c->pna.p);
}

static int proj_reassign_hamerly(isle_ctx* c, const ProjScalars& sc, int k, int it) {
  uint32_t* nact = c->active.p + c->D;
  ISLECHK(k_hamerly_filter(c, nullptr, c->assign.p, c->hub.p, c->hlb.p, sc.delta, sc.top, c->active.p, nact, ISLE_T_LLOYD_PROJ));
  uint32_t na = 0;
  ISLECHK(isle_fetch_u32(c, nact, &c->pin_small()->active_count, &na));
  if (c->knob_on(KN_DEBUG_HAMERLY)) fprintf(stderr, "[hamerly, projected] iter %d active %u of %llu\n", it, na, (unsigned long long)c->D);
  return k_proj_assign_active(c, c->P.p, c->pnorm.p, k, c->ldk, c->Cdev.p, c->cnorm.p, c->active.p, na, c->Pa.p, c->pna.p, c->assign.p, c->hub.p, c->hlb.p);
}

// the centres of the next iteration from the cluster sizes in c->counts: sums of the members' rows (:1957-1984; afresh in the first
// iteration, afterwards from the documents that changed centre), over the ranks, divided (:1988-1992); the global sizes for the stop rule
static int proj_update_centres(isle_ctx* c, const ProjPlan& p, int k, int it, std::vector<long long>& sizes) {
  const uint64_t D = c->D;
  const int ldk = c->ldk;
  float* sums = c->multi() ? c->Csum_local.p : c->Csum.p;  // this rank's sums
  bool updated = false;
  if (p.delta_sums && it > 0) ISLECHK(k_proj_accumulate_delta(c, c->P.p, D, k, ldk, c->assign.p, c->proj_counted.p, sums, c->counts.p, &updated));
  if (!updated) {
    ISLECHK(k_proj_accumulate(c, c->P.p, D, k, ldk, c->assign.p, sums, c->counts.p));
    if (p.delta_sums && D) HIPCHK(c, hipMemcpyAsync(c->proj_counted.p, c->assign.p, D * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
  } else {
    c->res.member_lists_stale();
  }
  if (c->multi()) HIPCHK(c, hipMemcpyAsync(c->Csum.p, sums, (size_t)k * ldk * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  ISLECHK(allreduce_sum<float>(c, c->Csum.p, (size_t)k * ldk));
  ISLECHK(fetch_sizes(c, k, sizes));
  if (p.hamerly) HIPCHK(c, hipMemcpyAsync(c->Cold.p, c->Cdev.p, (size_t)k * ldk * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  return k_proj_finalize(c, c->Csum.p, c->counts.p, k, ldk, c->Cdev.p);
}

// centre movements for the next filter
static int proj_movements(isle_ctx* c, const ProjPlan& p, const ProjScalars& sc, int k, std::vector<float>& pdelta_host) {
  ISLECHK(k_rownorms_diff(c, c->Cdev.p, c->Cold.p, k, k, c->ldk, sc.delta));
  if (!p.tiles) return k_ham_delta(c, sc.delta, k, sc.top);  // rounded-up movements and their top two, on the device
  ISLECHK(k_yy_delta(c, sc.delta, k, p.T, 32, sc.tmove));    // rounded-up movements and their maxima per tile
  return fetch_delta(c, sc.delta, k, pdelta_host);           // ... and a copy for the choice of the movers
}

extern "C" int isle_hip_lloyds_projected(isle_ctx* c, int k, float* C_lowd, int max_reps, int* iters_run, uint32_t* assign_out) {
  if (!c || !C_lowd || k < 1) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  isle_host_mark("lloyds_projected: entry");
  c->lloyd_trace_v[ISLE_SPACE_PROJECTED].clear();
  c->res.lloyd_projected_begins();
  ISLECHK(ensure_P(c, k));  // compute_projected_docs_l2sq :2032
  const ProjPlan plan = proj_plan(c, k, C_lowd);
  const uint64_t D = c->D;
  const int ldk = c->ldk;
  HIPCHK(c, c->Cdev.reserve((size_t)k * ldk));
  HIPCHK(c, c->Csum.reserve((size_t)k * ldk));
  HIPCHK(c, c->cnorm.reserve(k));
  HIPCHK(c, c->counts.reserve(k));
  HIPCHK(c, c->assign.reserve(D ? D : 1));
  c->res.partition_rewrite_begins();
  const size_t ch_bytes = (size_t)k * ldk * sizeof(float);
  HIPCHK(c, c->pin_stage.reserve(ch_bytes));
  float* Ch = reinterpret_cast<float*>(c->pin_stage.p);
  centres_pack(Ch, C_lowd, k, ldk);
  HIPCHK(c, hipMemcpyAsync(c->Cdev.p, Ch, ch_bytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));  // the staging buffer is written again at the end of this call
  isle_host_mark("lloyds_projected: centres uploaded");
  ProjScalars sc;
  ISLECHK(proj_reserve(c, plan, k, &sc));
  c->res.kmpp_first_assignment_taken();
  if (c->knob_on(KN_DEBUG_HAMERLY)) fprintf(stderr, "[projected Lloyd] first assignment %s\n", plan.from_kmpp ? "taken from the k-means++ rounds" : "computed");
  StopRule stop(c, k);
  int it = 0;
  std::vector<float> pdelta_host;  // the k centre movements of the last update (tile bounds: choice of the movers)
  isle_host_mark("lloyds_projected: loop starts");
  for (; it < max_reps; ++it) {
    ISLECHK(k_rownorms(c, c->Cdev.p, k, k, ldk, c->cnorm.p));  // :1938
    if (it == 0 || !plan.hamerly) ISLECHK(proj_assign_first(c, plan, k));
    else if (plan.tiles) ISLECHK(proj_reassign_tiles(c, plan, sc, k, it, pdelta_host));
    else ISLECHK(proj_reassign_hamerly(c, sc, k, it));
    ISLECHK(k_count_sizes(c, c->assign.p, D, k, c->counts.p));
    std::vector<long long> sizes;
    ISLECHK(proj_update_centres(c, plan, k, it, sizes));
    if (c->lloyd_trace) ISLECHK(trace_objective(c, ISLE_SPACE_PROJECTED, k));
    if (plan.hamerly && it + 1 < max_reps) ISLECHK(proj_movements(c, plan, sc, k, pdelta_host));
    bool conv = false;
    ISLECHK(stop.converged(sizes, c->assign.p, &conv));
    if (conv) {
      ++it;
      break;
    }
  }
  isle_host_mark("lloyds_projected: loop done");
  HIPCHK(c, hipMemcpyAsync(Ch, c->Cdev.p, ch_bytes, hipMemcpyDeviceToHost, c->stream));
  if (assign_out && D) HIPCHK(c, hipMemcpyAsync(assign_out, c->assign.p, D * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  centres_unpack(C_lowd, Ch, k, ldk);
  if (iters_run) *iters_run = it;
  if (max_reps > 0) {  // what isle_hip_kmeans_objective reads as the resident state of this space
    c->res.lloyd_projected_done(ISLE_SPACE_PROJECTED, k);
  }
  isle_host_mark("lloyds_projected: exit");
  return 0;
}

// ------------------------------------------------------------------------------------------
// lift + Lloyd on the sparse matrix
// ------------------------------------------------------------------------------------------
static int install_centers(isle_ctx* c, int ncols) {  // centers_cm (V x ncols) -> centers_rm (V x ld), zero padded
  const int ld = round4(ncols);
  HIPCHK(c, c->centers_rm.reserve((size_t)c->V * ld));
  HIPCHK(c, hipMemsetAsync(c->centers_rm.p, 0, (size_t)c->V * ld * sizeof(float), c->stream));
  ISLECHK(k_transpose(c, c->centers_cm.p, c->V, ncols, c->V, c->centers_rm.p, ld));
  c->res.centres_installed(ncols);
  return 0;
}

extern "C" int isle_hip_lift_centers(isle_ctx* c, const float* in, int ld_in, int ncols, float* centers) {
  if (!c || !in || ncols < 1) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  if (c->res.U_k == 0 || ld_in < c->res.U_k) return isle_fail(c, ISLE_E_ARG, "lift: need U and ld_in >= k");
  isle_host_mark("lift: entry");
  HIPCHK(c, c->Csum.reserve((size_t)ld_in * ncols));
  {
    const size_t in_bytes = (size_t)ld_in * ncols * sizeof(float);
    HIPCHK(c, c->pin_stage.reserve(in_bytes));
    memcpy(c->pin_stage.p, in, in_bytes);
    HIPCHK(c, hipMemcpyAsync(c->Csum.p, c->pin_stage.p, in_bytes, hipMemcpyHostToDevice, c->stream));  // the call synchronises before it returns
  }
  HIPCHK(c, c->centers_cm.reserve((size_t)c->V * ncols));
  ISLECHK(k_gemm_nn(c, c->Ucm.p, c->V, c->res.U_k, c->Csum.p, ld_in, ncols, c->centers_cm.p, ISLE_T_LIFT));
  ISLECHK(install_centers(c, ncols));
  // the centres lie in span(U): Lloyd on B can take its first assignment from the projection (isle_hip_lloyds_sparse)
  HIPCHK(c, c->lift_C.reserve((size_t)ld_in * ncols));
  HIPCHK(c, hipMemcpyAsync(c->lift_C.p, c->Csum.p, (size_t)ld_in * ncols * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  c->res.centres_lifted(ld_in, ncols);
  if (centers) HIPCHK(c, hipMemcpyAsync(centers, c->centers_cm.p, (size_t)c->V * ncols * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  isle_host_mark("lift: exit");
  return 0;
}

namespace {
// device scalars of the loop in c->Csum (2 k + 16 + G floats)
struct SparseScalars {
  float* delta;   // k movements
  float* cn_max;  // 2 k + 8: the largest centre norm
  HamTop* top;    // 2 k + 12: the top two movements (Hamerly)
  float* gmax;    // 2 k + 16: G group maxima of the movements (Yinyang)
};
// the regrouping of a run: slot tables on the device and the host's copy of slot_of_id (identity: null / empty)
struct SparseGroups {
  YyMap ymap;
  std::vector<uint32_t> slot_of_id_host;
};
}  // namespace
static SparseScalars sparse_scalars(isle_ctx* c, int k) {
  return {c->Csum.p, c->Csum.p + 2 * k + 8, reinterpret_cast<HamTop*>(c->Csum.p + 2 * k + 12), c->Csum.p + 2 * k + 16};
}

// The D x k scratch of the first assignment's product.  The route is chosen from sizes alone (route_scratch_ok), but on a device shared with
// other work the scratch may still not be had: the sparse product gives the same assignment up to dot-product rounding, so take it
// instead of failing the call
static bool first_scratch_had(isle_ctx* c, int k) {
  if (c->dotsT.reserve((size_t)c->D * k) == hipSuccess) return true;
  (void)hipGetLastError();
  fprintf(stderr, "[isle_hip] lloyds_sparse: no memory for the %.1f GB product of the first assignment; taking the sparse route\n",
          (double)c->D * k * sizeof(float) / 1e9);
  return false;
}

// the route decisions of one call (route_host.h SparsePlan)
static SparsePlan sparse_plan(isle_ctx* c, int k, int ld) {
  const SparseFacts f = {c->D, c->nnz, c->res.lift_valid, c->res.lift_k, c->res.U_k, c->ldk, c->res.P_ready, c->res.Pt_ready, c->res.Pt2_ready()};
  return isle_route_mem(c, [&](uint64_t total_mem, bool* ask) { return route_sparse_plan(f, k, ld, c->route, total_mem, ask); });
}

// the slot tables, from the norms just computed (the same on every rank: the centres are replicated)
static int sparse_regroup_tables(isle_ctx* c, int k, int G, SparseGroups* g) {
  TimeScope ts(c, ISLE_T_SPARSE_ASSIGN);
  float* cn_pin = c->pin_small()->centre_norms;  // page-locked, 32 KB (regrouping is the by-group form's: k <= 2048)
  HIPCHK(c, hipMemcpyAsync(cn_pin, c->cnorm.p, (size_t)k * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::vector<float> cnh(cn_pin, cn_pin + k);
  std::vector<uint32_t> id_of_slot((size_t)8 * G, 0xffffffffu);
  std::iota(id_of_slot.begin(), id_of_slot.begin() + k, 0u);
  std::stable_sort(id_of_slot.begin(), id_of_slot.begin() + k, [&](uint32_t a, uint32_t b) { return cnh[a] < cnh[b]; });
  g->slot_of_id_host.assign(k, 0u);
  for (int s2 = 0; s2 < k; ++s2) g->slot_of_id_host[id_of_slot[s2]] = (uint32_t)s2;
  ISLECHK(k_yy_map_upload(c, id_of_slot.data(), g->slot_of_id_host.data(), k, G, &g->ymap));
  HIPCHK(c, c->yy_cns.reserve((size_t)8 * G));
  return 0;
}

// B^T (U C^T) = (U^T B)^T C^T: the k-wide sparse product of the first assignment (distsq_docs_to_centers, :1494-1550) is a dense
// D x k x k product on the projection that k-means++ / Lloyd in span(U) left on the device — one MFMA GEMM, a transposition into
// the doc-major layout and the same distance / bound epilogue (norms of centres and documents are the word-space ones)
static int sparse_assign_first_via_projection(isle_ctx* c, const SparsePlan& p, const SparseScalars& sc, int k, int ld, const YyMap& ymap, const float* cn_grp) {
  const uint64_t D = c->D;
  TimeScope ts(c, ISLE_T_SPARSE_ASSIGN);
  if (p.yinyang && p.fused_first) {  // distances, group bounds and candidates formed inside the product: no D x k matrix in memory
    ISLECHK(k_max_f32(c, c->cnorm.p, k, sc.cn_max));
    const float* liftC = c->lift_C.p;
    if (p.regroup) {  // the product's columns in slot order: its groups of eight columns are the regrouped groups
      HIPCHK(c, c->yy_liftC.reserve((size_t)k * c->res.lift_ld));
      ISLECHK(k_yy_rows_by_slot(c, ymap, k, c->lift_C.p, c->res.lift_ld, c->yy_liftC.p));
      liftC = c->yy_liftC.p;
    }
    ISLECHK(k_gemm_assign_yy(c, c->res.Pt_ready ? c->Pt.p : nullptr, c->P.p, c->ldk, c->pnorm.p, D, k, liftC, c->res.lift_ld, k, p.G, cn_grp, c->dnorm.p, sc.cn_max,
                             c->assign.p, c->hub.p, c->yglb.p, ISLE_T_SPARSE_ASSIGN, c->res.Pt2_ready() ? c->Pt2.p : nullptr,
                             c->res.Pt2_ready() && c->res.Pt2_by_position() ? c->dperm.p : nullptr));
    if (p.regroup) ISLECHK(k_yy_labels_to_ids(c, ymap, c->assign.p, D));  // columns (slots) -> centres
    return 0;
  }
  HIPCHK(c, c->dotsT.reserve((size_t)D * k));
  ISLECHK(k_ensure_pt(c));
  ISLECHK(k_gemm_nn_assign(c, c->Pt.p, D, k, c->lift_C.p, c->res.lift_ld, k, c->dotsT.p, ISLE_T_SPARSE_ASSIGN));
  if (p.yinyang) {  // assignment and group bounds straight from the column-major product (the projection stays valid)
    ISLECHK(k_max_f32(c, c->cnorm.p, k, sc.cn_max));
    return k_dots_assign_cm(c, c->dotsT.p, k, p.G, c->cnorm.p, c->dnorm.p, sc.cn_max, c->assign.p, c->hub.p, c->yglb.p);
  }
  c->res.P_overwritten();  // P now holds the dot products (as with the LDS-banded wide product)
  if (ld != k) HIPCHK(c, hipMemsetAsync(c->P.p, 0, (size_t)D * ld * sizeof(float), c->stream));
  ISLECHK(k_transpose(c, c->dotsT.p, D, (uint64_t)k, D, c->P.p, (uint64_t)ld));
  return k_dots_assign(c, k, ld, c->cnorm.p, c->dnorm.p, c->assign.p, c->hub.p, c->hlb.p, 0);
}

// ISLE_DEBUG_HAMERLY: which bound the active documents reach, and by how much
static int debug_yy_margins(isle_ctx* c, int it, int G, const YyMap& ymap) {
  unsigned long long hh[16];
  ISLECHK(k_yy_dbg_margins(c, c->active.p, c->active.p + c->D, c->assign.p, c->hub.p, c->yglb.p, G, ymap, hh));
  fprintf(stderr, "[yinyang] iter %d active by (ub - smallest group bound) < 1e-6 | 1e-5 | 1e-4 | 1e-3 | 1e-2 | 1e-1 | 1 | more:  own group", it);
  for (int b = 0; b < 8; ++b) fprintf(stderr, " %llu", hh[b]);
  fprintf(stderr, ";  another group");
  for (int b = 0; b < 8; ++b) fprintf(stderr, " %llu", hh[8 + b]);
  fprintf(stderr, "\n");
  return 0;
}

// ISLE_DEBUG_HAMERLY: movements, norms and sizes behind a Yinyang re-examination; its group scans (done: the by-group form's pairs)
static int debug_yy_iteration(isle_ctx* c, const SparseScalars& sc, int k, int G, int it, bool done, unsigned long long npairs) {
  const uint64_t D = c->D;
  uint32_t na = 0;
  unsigned long long cnt[2] = {0, 0};
  HIPCHK(c, hipMemcpy(&na, c->active.p + D, 4, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(cnt, c->dbg_cnt.p, 16, hipMemcpyDeviceToHost));
  std::vector<float> sd(k), gs(G), sc2(k);
  float cm = 0.f;
  HIPCHK(c, hipMemcpy(sd.data(), sc.delta, k * sizeof(float), hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(gs.data(), sc.gmax, G * sizeof(float), hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(sc2.data(), c->cnorm.p, k * sizeof(float), hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(&cm, sc.cn_max, sizeof(float), hipMemcpyDeviceToHost));
  std::sort(sd.begin(), sd.end());
  std::sort(sc2.begin(), sc2.end());
  std::vector<long long> szs;
  ISLECHK(fetch_sizes(c, k, szs));
  long long smin = szs[0], smax = szs[0], empty = 0;
  for (auto v : szs) { smin = std::min(smin, v); smax = std::max(smax, v); empty += v == 0; }
  int n1 = 0, n2 = 0, n3 = 0, g1 = 0, g2 = 0;
  for (float v : sd) {
    n1 += v > 0.3f;
    n2 += v > 0.1f;
    n3 += v > 0.03f;
  }
  for (float v : gs) {
    g1 += v > 0.1f;
    g2 += v > 0.03f;
  }
  fprintf(stderr, "[yinyang] iter %d: centres that moved more than 0.3 / 0.1 / 0.03: %d / %d / %d of %d; groups whose largest movement exceeds 0.1 / 0.03: %d / %d of %d\n", it, n1,
          n2, n3, k, g1, g2, G);
  fprintf(stderr, "[yinyang] iter %d: movement median %.3g max %.3g; |c|^2 median %.3g max %.3g (cn_max %.3g); cluster sizes %lld..%lld, %lld empty\n", it,
          sd[k / 2], sd[k - 1], sc2[k / 2], sc2[k - 1], cm, smin, smax, empty);
  if (done)
    fprintf(stderr, "[yinyang] iter %d active %u of %llu; by group: %llu pairs beside the own-group scans (%.1f per active document, of %d)\n", it, na,
            (unsigned long long)D, npairs, na ? (double)npairs / na : 0.0, G);
  else
    fprintf(stderr, "[yinyang] iter %d active %u of %llu; group scans %llu (%.1f per active document, of %d), gathered nonzeros %llu\n", it, na,
            (unsigned long long)D, cnt[0], na ? (double)cnt[0] / na : 0.0, G, cnt[1]);
  return 0;
}

// A Yinyang re-examination.  All its bookkeeping stays on the device (largest centre norm, movements, group maxima, member offsets): the
// only host round trip of an iteration is the one the stop rule needs
static int sparse_reassign_yinyang(isle_ctx* c, const SparsePlan& p, const SparseScalars& sc, int k, int ld, int it, const SparseGroups& g, const float* cn_grp,
                                   const std::vector<float>& delta_host) {
  const int G = p.G;
  const YyMap& ymap = g.ymap;
  {
    TimeScope ts(c, ISLE_T_SPARSE_ASSIGN);
    ISLECHK(k_max_f32(c, c->cnorm.p, k, sc.cn_max));
  }
  uint32_t* nact = c->active.p + c->D;
  // large k: the centres also group-major (one 32-byte-row table per group) and the active documents grouped by their own group
  // (the member lists), so that waves running together gather from one table in L2; ISLE_YY_MODE = doc | docg | group picks the form
  // (measured, Lloyd on B per step: C3 shard 176 ms by document -> 112 ms by group, all of config 3 on one GPU 825 -> 588 ms; at C2,
  // G = 25 and a 40 MB table, the three forms are within 10 % of each other and the plain one stays)
  const uint32_t* order = p.yy_mode && c->res.members_valid && p.by_members ? c->members.p : nullptr;
  if (p.yy_mode) ISLECHK(k_yy_pack_groups(c, c->centers_rm.p, ld, G, ymap));
  // Movers.  A group's bound falls by the LARGEST movement among its eight centres, for every document: one centre that jumped (a
  // cluster of a handful of documents that gained or lost one) takes a whole group's bound away and makes nearly every document
  // active (config 3: 98 % in iterations 3 - 5, because of 1 - 3 centres).  Up to ten centres whose movement stands out (more than
  // twice the eleventh largest) are therefore left out of their groups' maxima and bounded by their exact new distances — one thin
  // pass of the pass-1 stream for b_d . c over all documents (k_yy_filter_tighten).  Exact: min(bound lowered by the other members'
  // movement, distance to the mover) is a lower bound of the group as before.  Same movements on every rank (the centres are all-reduced).
  YyMovers mv;
  const float* gmax_use = sc.gmax;
  // (the movers' distances are a thin product through the pass-1 stream: LDS-banded form only — the gather form, ISLE_GRAM_LDS=0 or a
  // matrix whose rows are not single-valued, keeps every centre inside its group's movement)
  if (p.movers) ISLECHK(k_band_build(c));
  if (p.movers && c->res.gl_mode == 1) {
    std::vector<float> gm;
    ISLECHK(prepare_movers(c, delta_host, k, 8, G, p.regroup ? &g.slot_of_id_host : nullptr, &mv, &gm));
    if (mv.n) {
      HIPCHK(c, hipStreamSynchronize(c->stream));  // gm is stack-owned
      gmax_use = c->yy_gmax2.p;
    }
  }
  if (p.fused)
    ISLECHK(k_yy_filter_tighten(c, order, c->assign.p, c->hub.p, c->yglb.p, G, sc.delta, gmax_use, c->active.p, nact, c->yy_cg.p, k, ld, cn_grp, c->dnorm.p, sc.cn_max,
                                mv, c->centers_rm.p, ymap, c->cnorm.p));
  else
    ISLECHK(k_yy_filter(c, order, c->assign.p, c->hub.p, c->yglb.p, G, sc.delta, sc.gmax, c->active.p, nact));
  const bool dbg = c->knob_on(KN_DEBUG_HAMERLY);
  unsigned long long* dbg_dev = nullptr;
  if (dbg && p.fused) ISLECHK(debug_yy_margins(c, it, G, ymap));
  if (dbg) {  // diagnostic only: group scans and gathered nonzeros of this iteration
    HIPCHK(c, c->dbg_cnt.reserve(18));
    HIPCHK(c, hipMemsetAsync(c->dbg_cnt.p, 0, 16, c->stream));
    dbg_dev = c->dbg_cnt.p;
  }
  bool done = false;
  unsigned long long npairs = 0;
  if (p.yy_mode == 2)
    ISLECHK(k_yy2_assign(c, c->yy_cg.p, k, ld, G, cn_grp, c->dnorm.p, sc.cn_max, c->active.p, nact, c->assign.p, c->hub.p, c->yglb.p, &done, &npairs, p.fused, ymap));
  if (!done)
    ISLECHK(k_yy_scan(c, c->centers_rm.p, p.yy_mode ? c->yy_cg.p : nullptr, k, ld, G, cn_grp, c->dnorm.p, sc.cn_max, c->active.p, nact, c->assign.p, c->hub.p,
                      c->yglb.p, dbg_dev, ymap));
  if (dbg) ISLECHK(debug_yy_iteration(c, sc, k, G, it, done, npairs));
  return 0;
}

static int sparse_reassign_hamerly(isle_ctx* c, const SparseScalars& sc, int k, int ld, int it) {
  uint32_t* nact = c->active.p + c->D;
  ISLECHK(k_hamerly_filter(c, c->res.members_valid ? c->members.p : nullptr, c->assign.p, c->hub.p, c->hlb.p, sc.delta, sc.top, c->active.p, nact));
  ISLECHK(k_spmm_wide_assign(c, c->centers_rm.p, k, ld, c->cnorm.p, c->dnorm.p, c->assign.p, c->active.p, nact, c->hub.p, c->hlb.p));
  if (c->knob_on(KN_DEBUG_HAMERLY)) {
    uint32_t na = 0;
    HIPCHK(c, hipMemcpy(&na, nact, 4, hipMemcpyDeviceToHost));
    fprintf(stderr, "[hamerly] iter %d active %u of %llu\n", it, na, (unsigned long long)c->D);
  }
  return 0;
}

// the centres of the next iteration from the cluster sizes in c->counts (:1613-1646), and the global sizes for the stop rule
static int sparse_update_centres(isle_ctx* c, const SparsePlan& p, int k, int ld, int it, std::vector<long long>& sizes) {
  const uint64_t D = c->D, V = c->V;
  // documents grouped by centre: visiting order of the next assignment (SparsePlan::by_members), and what the FRESH counting centroid
  // update walks (the first of a run; later ones go by the documents that changed centre)
  if (route_member_lists(it, p.by_members, c->res.gl_mode, c->route)) {
    TimeScope ts(c, ISLE_T_SPARSE_ASSIGN);
    ISLECHK(k_member_lists_dev(c, c->assign.p, D, k, c->counts.p));
  } else {
    c->res.member_lists_stale();
  }
  if (p.hamerly) HIPCHK(c, hipMemcpyAsync(c->centers_old.p, c->centers_rm.p, (size_t)V * ld * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  ISLECHK(k_centers_from_rows(c, c->assign.p, k, ld, c->centers_rm.p, it == 0));  // :1613-1638
  ISLECHK(allreduce_sum<float>(c, c->centers_rm.p, (size_t)V * ld));
  ISLECHK(fetch_sizes(c, k, sizes));
  return k_scale_centers(c, c->centers_rm.p, V, k, ld, c->counts.p);  // :1641-1646
}

// centre movements for the next filter
static int sparse_movements(isle_ctx* c, const SparsePlan& p, const SparseScalars& sc, int k, int ld, const YyMap& ymap, std::vector<float>& delta_host) {
  TimeScope ts(c, ISLE_T_SPARSE_ASSIGN);
  ISLECHK(k_colnorms_rm(c, c->centers_rm.p, c->V, k, ld, sc.delta, c->centers_old.p));
  if (!p.yinyang) return k_ham_delta(c, sc.delta, k, sc.top);
  ISLECHK(k_yy_delta(c, sc.delta, k, p.G, 8, sc.gmax, ymap.id_of_slot));  // movements and group maxima stay on the device
  return fetch_delta(c, sc.delta, k, delta_host);                        // ... and a copy of the k movements for the choice of the movers
}

extern "C" int isle_hip_lloyds_sparse(isle_ctx* c, int k, const float* centers_in, float* centers_out, uint32_t* assign, int max_reps,
                                      int* iters_run) {
  if (!c || k < 1) return ISLE_E_ARG;
  if (c->V == 0) return isle_fail(c, ISLE_E_ARG, "no matrix uploaded");
  ISLECHK(isle_enter(c));
  isle_host_mark("lloyds_sparse: entry");
  c->lloyd_trace_v[ISLE_SPACE_WORD].clear();
  c->res.lloyd_word_begins();
  const uint64_t D = c->D, V = c->V;
  const int ld = round4(k), G = (k + 7) / 8;
  if (centers_in) {
    HIPCHK(c, c->centers_cm.reserve((size_t)V * k));
    HIPCHK(c, hipMemcpy(c->centers_cm.p, centers_in, (size_t)V * k * sizeof(float), hipMemcpyHostToDevice));
    ISLECHK(install_centers(c, k));
    c->res.centres_not_lifted();
  } else if (!c->res.centers_ready || c->res.centers_k != k) {
    return isle_fail(c, ISLE_E_ARG, "lloyds_sparse: no device-resident centres for k = %d (call isle_hip_lift_centers)", k);
  }
  const SparsePlan plan = sparse_plan(c, k, ld);
  HIPCHK(c, c->dnorm.reserve(D ? D : 1));
  HIPCHK(c, c->cnorm.reserve(k));
  HIPCHK(c, c->counts.reserve(k));
  HIPCHK(c, c->assign.reserve(D ? D : 1));
  c->res.partition_rewrite_begins();
  {
    TimeScope ts(c, ISLE_T_SPARSE_ASSIGN);  // the plain pass over B: the floor of every other pass over it (tools/objective_probe.py)
    ISLECHK(k_doc_norms(c, c->dnorm.p));  // :1680-1687
  }
  if (plan.yinyang) HIPCHK(c, c->yglb.reserve((size_t)(D ? D : 1) * G + 64));
  HIPCHK(c, c->hub.reserve(D ? D : 1));
  HIPCHK(c, c->hlb.reserve(D ? D : 1));
  HIPCHK(c, c->active.reserve(D + 1));
  HIPCHK(c, c->centers_old.reserve((size_t)V * ld));
  HIPCHK(c, c->Csum.reserve((size_t)2 * k + 16 + G));
  const SparseScalars sc = sparse_scalars(c, k);
  StopRule stop(c, k);
  const bool dense_first = plan.via_projection && (plan.fused_first || first_scratch_had(c, k));
  c->res.centres_not_lifted();  // the centres move below
  int it = 0;
  SparseGroups groups;
  std::vector<float> delta_host;  // the k centre movements of the last update (Yinyang: choice of the movers)
  isle_host_mark("lloyds_sparse: loop starts");
  for (; it < max_reps; ++it) {
    {
      TimeScope ts(c, ISLE_T_SPARSE_ASSIGN);
      ISLECHK(k_colnorms_rm(c, c->centers_rm.p, V, k, ld, c->cnorm.p));  // :1604
    }
    if (it == 0 && plan.regroup) ISLECHK(sparse_regroup_tables(c, k, G, &groups));
    if (plan.regroup) {
      TimeScope ts(c, ISLE_T_SPARSE_ASSIGN);
      ISLECHK(k_yy_gather_by_slot(c, groups.ymap, k, G, c->cnorm.p, c->yy_cns.p));
    }
    const float* cn_grp = plan.regroup ? c->yy_cns.p : c->cnorm.p;  // the norms as the by-group kernels index them
    if (it == 0 && dense_first)
      ISLECHK(sparse_assign_first_via_projection(c, plan, sc, k, ld, groups.ymap, cn_grp));
    else if (it == 0 || !plan.hamerly)
      // documents are visited grouped by their previous centre (cache locality of the centre rows); results are order-independent
      ISLECHK(k_spmm_wide_assign(c, c->centers_rm.p, k, ld, c->cnorm.p, c->dnorm.p, c->assign.p, c->res.members_valid ? c->members.p : nullptr, nullptr, c->hub.p,
                                 plan.yinyang ? c->yglb.p : c->hlb.p, plan.yinyang ? G : 0));  // :1606
    else if (plan.yinyang)
      ISLECHK(sparse_reassign_yinyang(c, plan, sc, k, ld, it, groups, cn_grp, delta_host));
    else
      ISLECHK(sparse_reassign_hamerly(c, sc, k, ld, it));
    ISLECHK(k_count_sizes(c, c->assign.p, D, k, c->counts.p));
    std::vector<long long> sizes;
    ISLECHK(sparse_update_centres(c, plan, k, ld, it, sizes));
    if (c->lloyd_trace) ISLECHK(trace_objective(c, ISLE_SPACE_WORD, k));
    if (plan.hamerly && it + 1 < max_reps) ISLECHK(sparse_movements(c, plan, sc, k, ld, groups.ymap, delta_host));
    bool conv = false;
    ISLECHK(stop.converged(sizes, c->assign.p, &conv));
    if (conv) {
      ++it;
      break;
    }
  }
  isle_host_mark("lloyds_sparse: loop done");
  c->res.lloyd_word_done(ISLE_SPACE_WORD, k, max_reps > 0);  // the partition stays resident for isle_hip_catchwords
  if (assign && D) HIPCHK(c, hipMemcpyAsync(assign, c->assign.p, D * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  if (centers_out) {
    HIPCHK(c, c->centers_cm.reserve((size_t)V * k));
    // row-major (V x ld) -> col-major (V x k): view as a k x V col-major matrix with ld_in = ld
    ISLECHK(k_transpose(c, c->centers_rm.p, k, V, ld, c->centers_cm.p, V));
    HIPCHK(c, hipMemcpyAsync(centers_out, c->centers_cm.p, (size_t)V * k * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  isle_host_mark("lloyds_sparse: exit");
  if (iters_run) *iters_run = it;
  return 0;
}

// ------------------------------------------------------------------------------------------
// the k-means objective (objective.hip)
// ------------------------------------------------------------------------------------------
// The visiting order of the word-space pass: the resident member lists where they stand, lists of the given partition otherwise.  The
// lists reach the speed alone, never the result; where they were not valid they are left marked so (c->members is then nobody's).
static int objective_order(isle_ctx* c, int k, const uint32_t* assign_dev, const uint32_t** order) {
  *order = nullptr;
  if (c->D == 0) return 0;
  if (!c->res.members_valid) {
    TimeScope ts(c, ISLE_T_SPARSE_ASSIGN);
    HIPCHK(c, c->ob_cnt.reserve(k));
    ISLECHK(k_count_sizes(c, assign_dev, c->D, k, c->ob_cnt.p));
    ISLECHK(k_member_lists_dev(c, assign_dev, c->D, k, c->ob_cnt.p));
    c->res.member_lists_stale();
  }
  *order = c->members.p;
  return 0;
}

// the objective of the resident state of a loop in `space`: c->assign with centers_rm / Cdev
static int objective_resident(isle_ctx* c, int space, int k) {
  if (space == ISLE_SPACE_WORD) {
    const uint32_t* order = nullptr;
    ISLECHK(objective_order(c, k, c->assign.p, &order));
    return k_objective(c, space, k, c->assign.p, c->centers_rm.p, round4(k), order, ISLE_T_SPARSE_ASSIGN);
  }
  return k_objective(c, space, k, c->assign.p, c->Cdev.p, c->ldk, nullptr, ISLE_T_LLOYD_PROJ);
}

// c->ob_sums on the host and their sum, t ascending
static int objective_fetch_sums(isle_ctx* c, int k, std::vector<double>& sums, double* total) {
  sums.resize(k);
  HIPCHK(c, hipMemcpyAsync(sums.data(), c->ob_sums.p, (size_t)k * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  double s = 0.0;
  for (int t = 0; t < k; ++t) s += sums[t];
  *total = s;
  return 0;
}

// isle_hip_lloyds_trace: the total objective of the centres just updated with the partition they were averaged from (the reference's
// `residual`, src/sparseMatrix.cpp:1649-1663)
static int trace_objective(isle_ctx* c, int space, int k) {
  ISLECHK(objective_resident(c, space, k));
  std::vector<double> sums;
  double total = 0.0;
  ISLECHK(objective_fetch_sums(c, k, sums, &total));
  c->lloyd_trace_v[space].push_back(total);
  return 0;
}

extern "C" int isle_hip_kmeans_objective(isle_ctx* c, int space, int k, const uint32_t* assign, const float* centers, double* cluster_sums,
                                         uint64_t* cluster_sizes, double* total, double* doc_dist) {
  if (!c) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  if (space != ISLE_SPACE_WORD && space != ISLE_SPACE_PROJECTED) return isle_fail(c, ISLE_E_ARG, "kmeans_objective: unknown space %d", space);
  if (k < 1) return isle_fail(c, ISLE_E_ARG, "kmeans_objective: k < 1");
  if (c->V == 0) return isle_fail(c, ISLE_E_ARG, "kmeans_objective: no matrix uploaded");
  const bool word = space == ISLE_SPACE_WORD;
  const char* sname = word ? "word" : "projected";
  const uint64_t D = c->D, V = c->V;
  if (!word && c->res.U_k != k)
    return isle_fail(c, ISLE_E_ARG, "kmeans_objective: projected space needs U of k = %d columns, U has %d (run isle_hip_block_ks / set_U first)", k, c->res.U_k);
  if (!assign) {
    if (!c->res.loop_partition_resident(space, k, word))
      return isle_fail(c, ISLE_E_ARG, "kmeans_objective: no resident partition for the %s space and k = %d (run the loop of that space or pass assign)", sname, k);
    if (!word && !c->res.loop_projection_resident())
      return isle_fail(c, ISLE_E_ARG, "kmeans_objective: the projection P of the resident partition was released (run isle_hip_lloyds_projected again or pass assign)");
  } else {
    for (uint64_t j = 0; j < D; ++j)
      if (assign[j] >= (uint32_t)k) return isle_fail(c, ISLE_E_ARG, "kmeans_objective: assign[%llu] = %u out of range (k = %d)", (unsigned long long)j, assign[j], k);
  }
  if (!centers && !c->res.loop_centres_resident(word, k))
    return isle_fail(c, ISLE_E_ARG, "kmeans_objective: no resident centres for the %s space and k = %d (run the loop of that space or pass centers)", sname, k);
  ISLECHK(agree_i32(c, 2 * k + space, "the space and k of kmeans_objective"));
  if (!word) ISLECHK(ensure_P(c, k));  // local to the shard: no collective
  const int ld = word ? round4(k) : c->ldk;
  const uint32_t* assign_dev = c->assign.p;
  if (assign) {
    HIPCHK(c, c->ob_assign.reserve(D ? D : 1));
    if (D) HIPCHK(c, hipMemcpyAsync(c->ob_assign.p, assign, D * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    assign_dev = c->ob_assign.p;
  }
  const float* centres_dev = word ? c->centers_rm.p : c->Cdev.p;
  std::vector<float> packed;  // outlives the stream work: every path below synchronises
  if (centers && word) {
    HIPCHK(c, c->ob_cm.reserve((size_t)V * k));
    HIPCHK(c, c->ob_centres.reserve((size_t)V * ld));
    HIPCHK(c, hipMemcpyAsync(c->ob_cm.p, centers, (size_t)V * k * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(c->ob_centres.p, 0, (size_t)V * ld * sizeof(float), c->stream));
    ISLECHK(k_transpose(c, c->ob_cm.p, V, k, V, c->ob_centres.p, ld));
    centres_dev = c->ob_centres.p;
  } else if (centers) {
    packed.resize((size_t)k * ld);
    centres_pack(packed.data(), centers, k, ld);
    HIPCHK(c, c->ob_centres.reserve((size_t)k * ld));
    HIPCHK(c, hipMemcpyAsync(c->ob_centres.p, packed.data(), (size_t)k * ld * sizeof(float), hipMemcpyHostToDevice, c->stream));
    centres_dev = c->ob_centres.p;
  }
  const uint32_t* order = nullptr;
  if (word) ISLECHK(objective_order(c, k, assign_dev, &order));
  ISLECHK(k_objective(c, space, k, assign_dev, centres_dev, ld, order, word ? ISLE_T_SPARSE_ASSIGN : ISLE_T_LLOYD_PROJ));
  std::vector<double> sums;
  double tot = 0.0;
  ISLECHK(objective_fetch_sums(c, k, sums, &tot));
  if (cluster_sums) std::copy(sums.begin(), sums.end(), cluster_sums);
  if (total) *total = tot;
  if (cluster_sizes) HIPCHK(c, hipMemcpy(cluster_sizes, c->ob_acc.p + 2 * (size_t)k, (size_t)k * sizeof(uint64_t), hipMemcpyDeviceToHost));
  if (doc_dist && D) HIPCHK(c, hipMemcpy(doc_dist, c->ob_dd.p, D * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int isle_hip_get_projection(isle_ctx* c, int k, float* P) {
  if (!c || !P || k < 1) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  ISLECHK(ensure_P(c, k));
  if (c->D)
    HIPCHK(c, hipMemcpy2DAsync(P, (size_t)k * sizeof(float), c->P.p, (size_t)c->ldk * sizeof(float), (size_t)k * sizeof(float), c->D, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int isle_hip_lloyds_trace(isle_ctx* c, int on) {
  if (!c) return ISLE_E_ARG;
  c->lloyd_trace = on != 0;
  return 0;
}

extern "C" int isle_hip_lloyds_trace_get(isle_ctx* c, int space, double* objective, int cap, int* n) {
  if (!c) return ISLE_E_ARG;
  if (space != ISLE_SPACE_WORD && space != ISLE_SPACE_PROJECTED) return isle_fail(c, ISLE_E_ARG, "lloyds_trace_get: unknown space %d", space);
  const std::vector<double>& v = c->lloyd_trace_v[space];
  if (n) *n = (int)v.size();
  if (objective && cap > 0) std::copy(v.begin(), v.begin() + std::min<size_t>(v.size(), (size_t)cap), objective);
  return 0;
}
