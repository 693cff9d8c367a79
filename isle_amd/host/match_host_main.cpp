// isle_amd/host/match_host_main.cpp — the rule of isle_hip_compare_models / isle_hip_match_topics (../csrc/match_host.h) applied to a script on
// stdin, one JSON object per command on stdout: no library, no GPU (tests/test_match_rule_cpu.py builds it with the address and
// undefined-behaviour sanitizers and states every expected value itself).  A float goes in as its 32 bits and a double in and out as its 64
// bits, as unsigned decimal integers; <k ...> is a count followed by that many values.
//   consts                                                        MC_TILE, MC_CHUNK and the other constants
//   compare vocab  which host_given cols resident res_vocab res_cols  (side a, then the same six for side b)
//                                                                 mc_check_compare: the refusal's text, empty = accepted
//   matchargs dist_given na nb                                    mc_check_match
//   slicesargs slices                                             mc_check_slices
//   slices V ka kb num_cus asked                                  mc_slices and the slices' bounds
//   dist V ka kb <a bits> <b bits>                                model_dist_plain
//   match na nb <dist bits>                                       match_greedy
#include <cstring>
#include <iostream>

#include "../csrc/match_host.h"

namespace {

template <class T>
T take() {
  T v = T();
  std::cin >> v;
  return v;
}
template <class T>
std::vector<T> take_list() {
  std::vector<T> v(take<size_t>());
  for (T& x : v) std::cin >> x;
  return v;
}
template <class T>
void put_list(const char* name, const std::vector<T>& v, bool last = false) {
  std::cout << "\"" << name << "\": [";
  for (size_t i = 0; i < v.size(); ++i) std::cout << (i ? ", " : "") << (long long)v[i];
  std::cout << "]" << (last ? "" : ", ");
}
uint64_t bits_of(double d) {
  uint64_t u;
  std::memcpy(&u, &d, sizeof(u));
  return u;
}
void put_bits(const char* name, const std::vector<double>& v, bool last = false) {
  std::cout << "\"" << name << "\": [";
  for (size_t i = 0; i < v.size(); ++i) std::cout << (i ? ", " : "") << (unsigned long long)bits_of(v[i]);
  std::cout << "]" << (last ? "" : ", ");
}
McSide take_side() {
  McSide m;
  m.which = take<int>();
  m.host_given = take<int>() != 0;
  m.cols = take<int>();
  m.resident = take<int>() != 0;
  m.res_vocab = take<uint64_t>();
  m.res_cols = take<int>();
  return m;
}

}  // namespace

int main() {
  std::string cmd;
  while (std::cin >> cmd) {
    if (cmd == "consts") {
      std::cout << "{\"cmd\": \"consts\", \"tile\": " << MC_TILE << ", \"chunk\": " << MC_CHUNK << ", \"max_topics\": " << MC_MAX_TOPICS
                << ", \"max_vocab\": " << (unsigned long long)MC_MAX_VOCAB << ", \"partial_bytes\": " << (unsigned long long)MC_PARTIAL_BYTES
                << ", \"slice_waves\": " << MC_SLICE_WAVES << ", \"models\": [" << MC_MODEL_CATCH << ", " << MC_MODEL_AVG << ", " << MC_MODEL_HOST << ", "
                << MC_MODEL_LOADED << "]}\n";
    } else if (cmd == "compare") {
      const uint64_t vocab = take<uint64_t>();
      const McSide a = take_side(), b = take_side();
      std::cout << "{\"cmd\": \"compare\", \"text\": \"" << mc_check_compare(a, b, vocab) << "\"}\n";
    } else if (cmd == "matchargs") {
      const int given = take<int>(), na = take<int>(), nb = take<int>();
      std::cout << "{\"cmd\": \"matchargs\", \"text\": \"" << mc_check_match(given != 0, na, nb) << "\"}\n";
    } else if (cmd == "slicesargs") {
      std::cout << "{\"cmd\": \"slicesargs\", \"text\": \"" << mc_check_slices(take<int>()) << "\"}\n";
    } else if (cmd == "slices") {
      const uint64_t V = take<uint64_t>();
      const int ka = take<int>(), kb = take<int>(), cus = take<int>(), asked = take<int>();
      const uint32_t s = mc_slices(V, ka, kb, cus, asked);
      std::vector<uint64_t> bounds;
      for (uint32_t t = 0; t <= s; ++t) bounds.push_back(mc_slice_begin(V, s, t));
      std::cout << "{\"cmd\": \"slices\", \"slices\": " << s << ", \"words\": " << (unsigned long long)mc_slice_words(V, s) << ", ";
      put_list("bounds", bounds, true);
      std::cout << "}\n";
    } else if (cmd == "dist") {
      const uint64_t V = take<uint64_t>();
      const int ka = take<int>(), kb = take<int>();
      const std::vector<uint32_t> ab = take_list<uint32_t>(), bb = take_list<uint32_t>();
      if (ab.size() != V * (uint64_t)ka || bb.size() != V * (uint64_t)kb) return 2;
      std::vector<float> a(ab.size()), b(bb.size());
      if (!ab.empty()) std::memcpy(a.data(), ab.data(), ab.size() * sizeof(float));
      if (!bb.empty()) std::memcpy(b.data(), bb.data(), bb.size() * sizeof(float));
      std::vector<double> dist;
      model_dist_plain(a.data(), ka, b.data(), kb, V, dist);
      std::cout << "{\"cmd\": \"dist\", ";
      put_bits("dist", dist, true);
      std::cout << "}\n";
    } else if (cmd == "match") {
      const int na = take<int>(), nb = take<int>();
      const std::vector<uint64_t> db = take_list<uint64_t>();
      if (na < 1 || nb < 1 || db.size() != (size_t)na * nb) return 2;
      std::vector<double> d(db.size());
      std::memcpy(d.data(), db.data(), db.size() * sizeof(double));
      const McMatch m = match_greedy(d.data(), na, nb);
      std::cout << "{\"cmd\": \"match\", \"n_matched\": " << (unsigned long long)m.n_matched << ", \"mean_dist\": " << (unsigned long long)bits_of(m.mean_dist) << ", ";
      put_list("match_a", m.match_a);
      put_list("match_b", m.match_b);
      put_bits("match_dist", m.match_dist, true);
      std::cout << "}\n";
    } else {
      std::cerr << "unknown command " << cmd << "\n";
      return 2;
    }
  }
  return 0;
}
