// isle_amd/host/edge_select_main.cpp — the yardstick of the edge-topic pair selection: the host rule
// (fpsparse_detail::select_edge_pairs_host, fpsparse_hip.h) against the device entry (isle_hip_select_edge_pairs) on drawn documents.
//   edge_select_main <n_docs> <num_topics> <max_edge_topics> <seed> [--min-docs m] [--time] [--host-only] [--input file] [--triples file]
// n_docs (top1, top2) pairs are drawn from the seed, skewed (topic = floor(k u^3)) so that a few pairs are hot and many counts tie, one id
// in sixteen is -1; --input: top1[n_docs] then top2[n_docs] as raw int32 instead.  Prints "identical: <n> documents, <c> candidates,
// <s> selected" and exits 0 only if the triples, the candidate count and the threshold agree entry for entry; --time: one warm-up, then
// the wall time of each side.  --host-only: the host rule alone, no device (prints "host: ..."); --triples: its triples as text lines.
#include <chrono>
#include <fstream>

#include "fpsparse_hip.h"

using namespace ISLE;

static uint64_t splitmix(uint64_t& s) {
  uint64_t z = (s += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
static int32_t draw_topic(uint64_t& s, int k) {
  const uint64_t r = splitmix(s);
  if ((r & 15u) == 0) return -1;
  const double u = (double)(r >> 11) * (1.0 / 9007199254740992.0);
  const int t = (int)((double)k * u * u * u);
  return t < k ? t : k - 1;
}
static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int main(int argc, char** argv) {
  if (argc < 5) {
    std::cerr << "usage: edge_select_main <n_docs> <num_topics> <max_edge_topics> <seed> [--min-docs m] [--time] [--host-only] [--input file] [--triples file]\n";
    return 2;
  }
  const uint64_t n_docs = std::strtoull(argv[1], nullptr, 10);
  const int k = std::atoi(argv[2]);
  const int64_t max_edge = std::atoll(argv[3]);
  uint64_t seed = std::strtoull(argv[4], nullptr, 10), min_docs = ISLE_EDGE_TOPIC_MIN_DOCS;
  bool timed = false, host_only = false;
  std::string input, triples_out;
  for (int i = 5; i < argc; ++i) {
    const std::string a = argv[i];
    if (a == "--time") timed = true;
    else if (a == "--host-only") host_only = true;
    else if (a == "--min-docs" && i + 1 < argc) min_docs = std::strtoull(argv[++i], nullptr, 10);
    else if (a == "--input" && i + 1 < argc) input = argv[++i];
    else if (a == "--triples" && i + 1 < argc) triples_out = argv[++i];
    else {
      std::cerr << "unknown argument " << a << "\n";
      return 2;
    }
  }
  if (k < 1) {
    std::cerr << "num_topics < 1\n";
    return 2;
  }
  std::vector<int32_t> t1(n_docs), t2(n_docs);
  if (!input.empty()) {
    std::ifstream in(input, std::ios::binary);
    in.read((char*)t1.data(), (std::streamsize)(n_docs * sizeof(int32_t)));
    in.read((char*)t2.data(), (std::streamsize)(n_docs * sizeof(int32_t)));
    if (!in) {
      std::cerr << "cannot read " << n_docs << " pairs from " << input << "\n";
      return 2;
    }
  } else {
    for (uint64_t d = 0; d < n_docs; ++d) {
      t1[d] = draw_topic(seed, k);
      t2[d] = draw_topic(seed, k);
    }
  }
  std::vector<std::tuple<int, int, uint64_t>> host_sel;
  uint64_t h_cand = 0, h_thr = 0;
  double host_ms = 0.0;
  for (int rep = 0; rep < (timed ? 2 : 1); ++rep) {
    const double t0 = now_ms();
    fpsparse_detail::select_edge_pairs_host(t1.data(), t2.data(), n_docs, max_edge, min_docs, host_sel, &h_cand, &h_thr);
    host_ms = now_ms() - t0;
  }
  if (!triples_out.empty()) {
    std::ofstream o(triples_out);
    for (const auto& p : host_sel) o << std::get<0>(p) << ' ' << std::get<1>(p) << ' ' << std::get<2>(p) << '\n';
    o << "candidates " << h_cand << " threshold " << h_thr << '\n';
  }
  if (host_only) {
    std::cout << "host: " << n_docs << " documents, " << h_cand << " candidates, " << host_sel.size() << " selected" << std::endl;
    return 0;
  }
  isle_ctx* ctx = isle_hip_create(0);
  if (!ctx) {
    std::cerr << "isle_hip_create failed: no device\n";
    return 1;
  }
  const uint64_t cap = std::min<uint64_t>(std::min<uint64_t>((uint64_t)std::max<int64_t>(max_edge, 0), (uint64_t)k * (uint64_t)k), n_docs);
  std::vector<int64_t> dev(3 * cap + 1);
  uint64_t d_sel = 0, d_cand = 0, d_thr = 0;
  double dev_ms = 0.0;
  int rc = 0;
  for (int rep = 0; rep < (timed ? 2 : 1) && rc == 0; ++rep) {
    const double t0 = now_ms();
    rc = isle_hip_select_edge_pairs(ctx, t1.data(), t2.data(), n_docs, k, max_edge, min_docs, dev.data(), cap, &d_sel, &d_cand, &d_thr);
    dev_ms = now_ms() - t0;
  }
  if (rc != 0) {
    std::cerr << "isle_hip_select_edge_pairs: " << isle_hip_last_error(ctx) << "\n";
    isle_hip_destroy(ctx);
    return 1;
  }
  isle_hip_destroy(ctx);
  bool same = d_sel == host_sel.size() && d_cand == h_cand && d_thr == h_thr;
  for (uint64_t e = 0; same && e < d_sel; ++e)
    same = dev[3 * e] == std::get<0>(host_sel[e]) && dev[3 * e + 1] == std::get<1>(host_sel[e]) && (uint64_t)dev[3 * e + 2] == std::get<2>(host_sel[e]);
  if (timed) std::cout << "host " << host_ms << " ms, device (upload included) " << dev_ms << " ms" << std::endl;
  if (!same) {
    std::cout << "DIFFERENT: host " << h_cand << " candidates, " << host_sel.size() << " selected, threshold " << h_thr << "; device " << d_cand << ", " << d_sel
              << ", " << d_thr << std::endl;
    return 1;
  }
  std::cout << "identical: " << n_docs << " documents, " << h_cand << " candidates, " << host_sel.size() << " selected" << std::endl;
  return 0;
}
