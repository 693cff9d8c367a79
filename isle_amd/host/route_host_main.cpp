// isle_amd/host/route_host_main.cpp — the rules that choose a kernel form (../csrc/route_host.h) applied to a script on stdin, one JSON
// object per command on stdout: no library, no GPU (tests/test_route_host_cpu.py builds it with the address and undefined-behaviour
// sanitizers and states every expected value itself).  Booleans go in and out as 0 / 1; a double goes in as its 64 bits, as an unsigned
// decimal integer.  Every rule reads the switches of the last `env` command (none set before the first one).
//   env <n (id hex)>                      route_env: switch number id (the order of knobs.h) holds the string with these bytes in hex,
//                                         '-' for the empty string; every other switch is not set.  Answers every field of RouteEnv
//   scratch <bytes> total_mem             route_scratch_ok, and whether it asked for the device
//   comm dflt <now>                       route_comm_selftest, route_comm_timeout
//   ks multi dense_A                      route_ks_rowshard, route_ks_pipelined
//   update b m ld aligned16               route_update_mfma
//   gemm M K N has_rows has_split         route_gemm_tiles, route_gemm_bf16x3, route_gemm_assign_fused_ok, route_gemm_two_terms, route_gemm_dma
//   evd n                                 route_evd_tridiag
//   a2 D k                                route_want_a2
//   kmpp k multi injected                 route_kmpp_plan
//   kmpp_sparse can nnz D ldk nc PW       route_kmpp_sparse
//   proj D Pt Pt2 P track_k same_P seeds_kept k                route_proj_plan
//   pt_sort has_need n                    route_pt_sort
//   full Pt Pt2 D k total_mem             route_proj_full_by_gemm
//   active n k                            route_proj_active_by_gemm
//   sparse D nnz lift_valid lift_k U_k ldk P Pt Pt2 k ld total_mem   route_sparse_plan
//   centres it by_members gl_mode first   route_member_lists, route_counts_fresh
//   wide V ldk                            route_wide_through_lds, route_wide_nit
//   gl nnz D V n_out gl1_G                route_gl_eligible, route_gl_options, route_gl_fill_bucketed, route_gl_panel_width
//   grouped with_norms PW k D wg_panels total_mem              route_gl_wide_grouped
//   td n lds_bytes gsmall nmax_back num_cus failed             route_td_workgroups, route_td_persist
//   td_split multi world rank nvec n      route_td_split
//   td_back nvec num_cus kc               route_td_back
//   objective k                           route_objective_acc, route_objective_lds_bytes
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "../csrc/route_host.h"

namespace {

template <class T>
T take() {
  T v = T();
  std::cin >> v;
  return v;
}
bool flag() { return take<int>() != 0; }
double take_double() {
  const unsigned long long b = take<unsigned long long>();
  double v;
  std::memcpy(&v, &b, 8);
  return v;
}
unsigned long long bits(double v) {
  unsigned long long b;
  std::memcpy(&b, &v, 8);
  return b;
}
bool first_field;
void put(const char* name, long long v) {
  std::printf("%s\"%s\": %lld", first_field ? "" : ", ", name, v);
  first_field = false;
}
void put_u(const char* name, unsigned long long v) {
  std::printf("%s\"%s\": %llu", first_field ? "" : ", ", name, v);
  first_field = false;
}

RouteEnv read_env() {
  // every string in storage of exactly its length + 1: a read past the terminator is the sanitizer's to find
  std::vector<std::vector<char>> store(KN_COUNT);
  const char* val[KN_COUNT] = {};
  for (size_t n = take<size_t>(); n > 0 && std::cin; --n) {
    const int id = take<int>();
    const std::string hex = take<std::string>();
    if (id < 0 || id >= KN_COUNT) continue;
    store[id].clear();
    for (size_t i = 0; hex != "-" && i + 1 < hex.size(); i += 2) store[id].push_back((char)std::stoi(hex.substr(i, 2), nullptr, 16));
    store[id].push_back('\0');
    val[id] = store[id].data();
  }
  return route_env(val);
}
void put_env(const RouteEnv& e) {
  put("gram_lds", e.gram_lds), put("gl_g1", e.gl_g1), put("gl_g2", e.gl_g2), put("gl_place", e.gl_place), put("gl_fill_buckets", e.gl_fill_buckets);
  put("gl_rounds", e.gl_rounds), put("gl_columns", e.gl_columns), put("gl_panel", e.gl_panel), put("gl_wide_grouped", e.gl_wide_grouped);
  put("wide_gather", e.wide_gather), put("wide_lds", e.wide_lds), put("ks_rowshard", e.ks_rowshard), put("ks_sync", e.ks_sync);
  put("ks_ortho_passes", e.ks_ortho_passes), put("update_mfma", e.update_mfma), put("evd_jacobi", e.evd_jacobi), put("td_chain", e.td_chain);
  put("td_bar", e.td_bar), put("td_back", e.td_back), put("evd_split", e.evd_split), put("kmpp_host_dice", e.kmpp_host_dice);
  put("kmpp_sparse", e.kmpp_sparse), put("kmpp_track", e.kmpp_track), put("no_hamerly", e.no_hamerly), put("kmeans_bounds", e.kmeans_bounds);
  put("proj_bounds", e.proj_bounds), put("proj_full", e.proj_full), put("first_assign", e.first_assign), put("gemm_bf16x3", e.gemm_bf16x3);
  put("gemm_epilogue", e.gemm_epilogue), put("gemm_terms", e.gemm_terms), put("gemm_dma", e.gemm_dma), put("yy_mode", e.yy_mode);
  put("yy_fused", e.yy_fused), put("yy_movers", e.yy_movers), put("yy_regroup", e.yy_regroup), put("yy_order", e.yy_order), put("pt_sort", e.pt_sort);
  put("proj_active", e.proj_active), put("proj_sums", e.proj_sums), put("centers_fresh", e.centers_fresh), put_u("infer_cap_rows", e.infer_cap_rows);
  put_u("chunk_cols", e.chunk_cols), put("comm_timeout_set", e.comm_timeout_set), put_u("comm_timeout", bits(e.comm_timeout));
  put("comm_selftest", e.comm_selftest);
}

}  // namespace

int main() {
  RouteEnv e;
  std::string cmd;
  while (std::cin >> cmd) {
    std::printf("{\"cmd\": \"%s\", ", cmd.c_str());
    first_field = true;
    bool ask = false;
    if (cmd == "env") {
      e = read_env();
      put_env(e);
    } else if (cmd == "scratch") {
      const double bytes = take_double();
      const uint64_t total = take<uint64_t>();
      put("ok", route_scratch_ok(bytes, total, &ask)), put("ask", ask);
    } else if (cmd == "comm") {
      const bool dflt = flag();
      const double now = take_double();
      put("selftest", route_comm_selftest(dflt, e)), put_u("timeout", bits(route_comm_timeout(now, e)));
    } else if (cmd == "ks") {
      const bool multi = flag(), dense_A = flag();
      put("shard", route_ks_rowshard(multi, dense_A, e)), put("pipelined", route_ks_pipelined(e));
    } else if (cmd == "update") {
      const int b = take<int>(), m = take<int>();
      const uint64_t ld = take<uint64_t>();
      const bool aligned = flag();
      put("mfma", route_update_mfma(b, m, ld, aligned, e));
    } else if (cmd == "gemm") {
      const uint64_t M = take<uint64_t>();
      const int K = take<int>(), N = take<int>();
      const bool has_rows = flag(), has_split = flag();
      put_u("tiles", route_gemm_tiles(M, N)), put("bf16x3", route_gemm_bf16x3(M, K, N, e)), put("fused_ok", route_gemm_assign_fused_ok(M, K, N, e));
      put("two_terms", route_gemm_two_terms(has_rows, e)), put("dma", route_gemm_dma(has_split, e));
    } else if (cmd == "evd") {
      put("tridiag", route_evd_tridiag(take<int>(), e));
    } else if (cmd == "a2") {
      const uint64_t D = take<uint64_t>();
      put("want_a2", route_want_a2(D, take<int>(), e));
    } else if (cmd == "kmpp") {
      const int k = take<int>();
      const bool multi = flag(), injected = flag();
      const KmppPlan p = route_kmpp_plan(k, multi, injected, e);
      put("track", p.track), put("maxdraw", p.maxdraw), put("device_dice", p.device_dice);
    } else if (cmd == "kmpp_sparse") {
      const bool can = flag();
      const uint64_t nnz = take<uint64_t>(), D = take<uint64_t>();
      const int ldk = take<int>(), nc = take<int>(), PW = take<int>();
      put("sparse", route_kmpp_sparse(can, nnz, D, ldk, nc, PW, e));
    } else if (cmd == "proj") {
      ProjFacts f;
      f.D = take<uint64_t>();
      f.Pt_ready = flag(), f.Pt2_ready = flag(), f.P_ready = flag();
      f.kmpp_track_k = take<int>();
      f.kmpp_same_P = flag(), f.seeds_kept = flag();
      const ProjPlan p = route_proj_plan(f, take<int>(), e);
      put("hamerly", p.hamerly), put("tiles", p.tiles), put("T", p.T), put("TL", p.TL), put("from_kmpp", p.from_kmpp), put("pt_sorted", p.pt_sorted);
      put("delta_sums", p.delta_sums), put("movers", p.movers);
    } else if (cmd == "pt_sort") {
      const bool has_need = flag();
      put("sort", route_pt_sort(has_need, take<uint32_t>(), e));
    } else if (cmd == "full") {
      const bool Pt = flag(), Pt2 = flag();
      const uint64_t D = take<uint64_t>();
      const int k = take<int>();
      const uint64_t total = take<uint64_t>();
      put("by_gemm", route_proj_full_by_gemm(Pt, Pt2, D, k, e, total, &ask)), put("ask", ask);
    } else if (cmd == "active") {
      const uint64_t n = take<uint64_t>();
      put("by_gemm", route_proj_active_by_gemm(n, take<int>(), e));
    } else if (cmd == "sparse") {
      SparseFacts f;
      f.D = take<uint64_t>(), f.nnz = take<uint64_t>();
      f.lift_valid = flag();
      f.lift_k = take<int>(), f.U_k = take<int>(), f.ldk = take<int>();
      f.P_ready = flag(), f.Pt_ready = flag(), f.Pt2_ready = flag();
      const int k = take<int>(), ld = take<int>();
      const uint64_t total = take<uint64_t>();
      const SparsePlan p = route_sparse_plan(f, k, ld, e, total, &ask);
      put("hamerly", p.hamerly), put("yinyang", p.yinyang), put("G", p.G), put("yy_mode", p.yy_mode), put("fused", p.fused), put("by_members", p.by_members);
      put("fused_first", p.fused_first), put("via_projection", p.via_projection), put("regroup", p.regroup), put("movers", p.movers), put("ask", ask);
    } else if (cmd == "centres") {
      const int it = take<int>();
      const bool by_members = flag();
      const int gl_mode = take<int>();
      const bool first = flag();
      put("lists", route_member_lists(it, by_members, gl_mode, e)), put("fresh", route_counts_fresh(first, e));
    } else if (cmd == "wide") {
      const uint64_t V = take<uint64_t>();
      put("lds", route_wide_through_lds(V, e)), put("nit", route_wide_nit(take<int>()));
    } else if (cmd == "gl") {
      const uint64_t nnz = take<uint64_t>(), D = take<uint64_t>(), V = take<uint64_t>();
      const uint32_t n_out = take<uint32_t>();
      const int G = take<int>();
      const GlPlanOpts o = route_gl_options(e);
      put("eligible", route_gl_eligible(nnz, D, V, e)), put("g1", o.g1), put("g2", o.g2), put("rounds", o.rounds), put("columns", o.columns);
      put_u("test_cus", o.test_cus), put("bucketed", route_gl_fill_bucketed(n_out, nnz, e)), put("panel", route_gl_panel_width(G, e));
    } else if (cmd == "grouped") {
      const bool with_norms = flag();
      const int PW = take<int>(), k = take<int>();
      const uint64_t D = take<uint64_t>();
      const int wg = take<int>();
      const uint64_t total = take<uint64_t>();
      put("grouped", route_gl_wide_grouped(with_norms, PW, k, D, wg, e, total, &ask)), put("ask", ask);
    } else if (cmd == "td") {
      const int n = take<int>();
      const size_t lds = take<size_t>();
      const int gsmall = take<int>(), nmax = take<int>(), cus = take<int>();
      const bool failed = flag();
      const int pG = route_td_workgroups(n, lds, gsmall);
      put("pG", pG), put("persist", route_td_persist(pG, n, nmax, cus, failed, e));
    } else if (cmd == "td_split") {
      const bool multi = flag();
      const int world = take<int>(), rank = take<int>(), nvec = take<int>(), n = take<int>();
      const TdSplit s = route_td_split(multi, world, rank, nvec, n, e);
      put("v0", s.v0), put("v1", s.v1), put("kc", s.kc);
    } else if (cmd == "td_back") {
      const int nvec = take<int>(), cus = take<int>(), kc = take<int>();
      const TdBack b = route_td_back(nvec, cus, kc, e);
      put("back", b == TD_BACK_WY ? 0 : b == TD_BACK_SEQ8 ? 8 : 4);
    } else if (cmd == "objective") {
      const int k = take<int>();
      put("lds", route_objective_acc(k) == OBJ_ACC_LDS), put_u("lds_bytes", route_objective_lds_bytes(k));
    } else {
      std::fprintf(stderr, "route_host_main: unknown command %s\n", cmd.c_str());
      return 2;
    }
    std::printf("}\n");
    if (!std::cin) {
      std::fprintf(stderr, "route_host_main: %s: input ended or did not parse\n", cmd.c_str());
      return 2;
    }
  }
  return 0;
}
