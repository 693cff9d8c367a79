// isle_amd/csrc/match_host.h — the rule of isle_hip_compare_models / isle_hip_match_topics (model_compare.hip, api_stages.cpp): the L1
// distance of every topic of one model to every topic of another, and the greedy matching of the topics by it.  Plain C++ (no HIP type, no
// isle_ctx): the tile constants the kernel compiles, the argument checks with the refusals' texts, a plain triple loop for the distances
// and the sort-and-sweep statement of the matching.  ../host/match_host_main.cpp applies all of it to a script,
// tests/test_match_rule_cpu.py checks the answers.
//
// Distance.  Models a (V x ka) and b (V x kb), column-major fp32, the same V:
//   dist[i][j] = sum over w of | (double)a[w, i] - (double)b[w, j] |            (row-major ka x kb doubles)
// Every term is formed in double: the subtraction rounds at most once, the absolute value is exact.  The terms are summed in double in an
// order that is a function of (V, ka, kb, slices) only: no floating-point atomics, two calls give the same bits.  A column with any
// non-finite entry makes its whole row (a) or column (b) of dist NaN.  Nothing asks the columns to be L1-normalised.  Guaranteed:
// |dist - exact| <= V 2^-53 exact (1 + O(V 2^-53)).  Where every entry is an integer multiple of 2^-12 and V <= 2^20 every partial sum is
// exact in double and the result is the exact value whatever the order: most tests compare with ==.
// That the terms are formed and summed in fp64 is a choice for the sake of a clean rule; an fp32 difference would be another rule, not a
// faster form of this one, and is not built.
//
// Matching, on an na x nb matrix of doubles.  An edge (i, j) exists where dist[i][j] is finite (NaN, +inf and -inf are no edge).  The edges
// are ordered by (dist, i, j): < on doubles (so -0 equals +0), then i, then j.  They are walked in that order and (i, j) is matched when
// both are still free.  match_a[i] = the matched j or -1, match_b[j] = the matched i or -1, match_dist[i] = the matched distance (its own
// bits) or NaN, n_matched, and mean_dist = the matched distances summed in double in ascending i on the host, over n_matched (NaN where
// nothing matched).  THE OPTIMAL (HUNGARIAN) ASSIGNMENT IS OUT OF SCOPE: greedy is the stated rule, its mean an upper bound of the
// optimal one's.
// On the device the same matching is the fixed point of rounds of mutually best pairs: every free row takes its least free finite column
// (ties: the smaller j), every free column its least free finite row over ALL free rows (ties: the smaller i), a pair that chose each
// other is matched.  The least edge among the free ones is always mutual, so a round matches at least one pair while an edge between two
// free sides is left.  rounds = the rounds that matched a pair (min(na, nb) at most; dist[i][j] = i + j takes exactly that many).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

constexpr int MC_TILE = 64;   // topics of each side per workgroup of mc_dist_k
constexpr int MC_CHUNK = 64;  // words staged in LDS at once; slice bounds are multiples of it
constexpr int MC_MAX_TOPICS = 8192;                 // a side's columns: the matrix is cols_a cols_b 8 bytes, 512 MB at the limit
constexpr uint64_t MC_MAX_VOCAB = 0xfffffff0ull;
constexpr uint64_t MC_PARTIAL_BYTES = 1ull << 30;   // the slices' partial matrices together never take more
constexpr int MC_SLICE_WAVES = 4;                   // the slice rule aims at this many workgroups per compute unit
constexpr int MC_MODEL_CATCH = 0, MC_MODEL_AVG = 1, MC_MODEL_HOST = 2, MC_MODEL_LOADED = 3;  // include/isle_hip.h: ISLE_MODEL_*

// ---- the slice rule's arithmetic (route_host.h: route_model_dist_slices) -------------------------------------------------------------------
// asked >= 1: that many; asked == 0: enough slices that the pair tiles times the slices give every compute unit MC_SLICE_WAVES workgroups.
// Either way at most ceil(V / MC_CHUNK) and at most what keeps the partial matrices within MC_PARTIAL_BYTES; at least 1.
inline uint32_t mc_slices(uint64_t V, int ka, int kb, int num_cus, int asked) {
  const uint64_t tiles = (uint64_t)((ka + MC_TILE - 1) / MC_TILE) * (uint64_t)((kb + MC_TILE - 1) / MC_TILE);
  const uint64_t chunks = std::max<uint64_t>(1, (V + MC_CHUNK - 1) / MC_CHUNK);
  uint64_t s = asked >= 1 ? (uint64_t)asked : ((uint64_t)MC_SLICE_WAVES * (uint64_t)std::max(1, num_cus) + tiles - 1) / std::max<uint64_t>(1, tiles);
  s = std::min(s, chunks);
  s = std::min(s, std::max<uint64_t>(1, MC_PARTIAL_BYTES / ((uint64_t)ka * (uint64_t)kb * 8)));
  return (uint32_t)std::max<uint64_t>(1, s);
}
// the words of a slice: a multiple of MC_CHUNK; slice s holds the words [min(V, s per), min(V, (s + 1) per))
inline uint64_t mc_slice_words(uint64_t V, uint32_t slices) {
  const uint64_t chunks = std::max<uint64_t>(1, (V + MC_CHUNK - 1) / MC_CHUNK);
  return (chunks + slices - 1) / slices * MC_CHUNK;
}
inline uint64_t mc_slice_begin(uint64_t V, uint32_t slices, uint32_t s) { return std::min<uint64_t>(V, (uint64_t)s * mc_slice_words(V, slices)); }

// ---- the argument checks: empty = accepted, else the refusal's text ------------------------------------------------------------------------
struct McSide {
  int which;           // MC_MODEL_*
  bool host_given;     // HOST: the caller's pointer is not null
  int cols;            // the caller's
  bool resident;       // a resident side exists ...
  uint64_t res_vocab;  // ... with this vocabulary
  int res_cols;        // ... and these columns
};
inline const char* mc_model_name(int which) {
  return which == MC_MODEL_CATCH ? "catch" : which == MC_MODEL_AVG ? "average" : which == MC_MODEL_LOADED ? "loaded" : which == MC_MODEL_HOST ? "host" : "?";
}
inline std::string mc_check_side(const char* side, const McSide& m, uint64_t vocab) {
  char t[240];
  t[0] = 0;
  if (m.which != MC_MODEL_CATCH && m.which != MC_MODEL_AVG && m.which != MC_MODEL_HOST && m.which != MC_MODEL_LOADED)
    snprintf(t, sizeof(t), "compare_models: side %s: unknown model %d", side, m.which);
  else if (m.cols < 1 || m.cols > MC_MAX_TOPICS) snprintf(t, sizeof(t), "compare_models: side %s: %d columns outside 1 .. %d", side, m.cols, MC_MAX_TOPICS);
  else if (m.which == MC_MODEL_HOST && !m.host_given) snprintf(t, sizeof(t), "compare_models: side %s: null host model", side);
  else if (m.which != MC_MODEL_HOST && !m.resident) snprintf(t, sizeof(t), "compare_models: side %s: no %s model is resident", side, mc_model_name(m.which));
  else if (m.which != MC_MODEL_HOST && vocab != m.res_vocab)
    snprintf(t, sizeof(t), "compare_models: side %s: vocab = %llu, the %s model's is %llu", side, (unsigned long long)vocab, mc_model_name(m.which),
             (unsigned long long)m.res_vocab);
  else if (m.which != MC_MODEL_HOST && m.cols != m.res_cols)
    snprintf(t, sizeof(t), "compare_models: side %s: %d columns, the %s model has %d", side, m.cols, mc_model_name(m.which), m.res_cols);
  return t;
}
inline std::string mc_check_compare(const McSide& a, const McSide& b, uint64_t vocab) {
  char t[240];
  if (vocab == 0 || vocab > MC_MAX_VOCAB) {
    snprintf(t, sizeof(t), "compare_models: vocab = %llu outside 1 .. %llu", (unsigned long long)vocab, (unsigned long long)MC_MAX_VOCAB);
    return t;
  }
  const std::string why = mc_check_side("a", a, vocab);
  return why.empty() ? mc_check_side("b", b, vocab) : why;
}
inline std::string mc_check_match(bool dist_given, int na, int nb) {
  char t[240];
  t[0] = 0;
  if (na < 1 || na > MC_MAX_TOPICS || nb < 1 || nb > MC_MAX_TOPICS) snprintf(t, sizeof(t), "match_topics: %d x %d outside 1 .. %d on each side", na, nb, MC_MAX_TOPICS);
  else if (!dist_given) snprintf(t, sizeof(t), "match_topics: null dist_host");
  return t;
}
inline std::string mc_check_slices(int slices) {
  char t[240];
  t[0] = 0;
  if (slices < 0) snprintf(t, sizeof(t), "model_dist_slices: slices = %d is negative", slices);
  return t;
}

// ---- the statement of the distances: a plain triple loop, words ascending ------------------------------------------------------------------
inline void model_dist_plain(const float* a, int ka, const float* b, int kb, uint64_t V, std::vector<double>& dist) {
  dist.assign((size_t)ka * kb, 0.0);
  std::vector<char> bad_a((size_t)ka, 0), bad_b((size_t)kb, 0);
  for (int i = 0; i < ka; ++i)
    for (uint64_t w = 0; w < V; ++w) bad_a[i] |= !std::isfinite(a[(size_t)i * V + w]);
  for (int j = 0; j < kb; ++j)
    for (uint64_t w = 0; w < V; ++w) bad_b[j] |= !std::isfinite(b[(size_t)j * V + w]);
  for (int i = 0; i < ka; ++i)
    for (int j = 0; j < kb; ++j) {
      double s = 0.0;
      for (uint64_t w = 0; w < V; ++w) s += std::fabs((double)a[(size_t)i * V + w] - (double)b[(size_t)j * V + w]);
      dist[(size_t)i * kb + j] = (bad_a[i] || bad_b[j]) ? std::numeric_limits<double>::quiet_NaN() : s;
    }
}

// ---- the statement of the matching: sort the edges, sweep them -----------------------------------------------------------------------------
struct McMatch {
  std::vector<int32_t> match_a, match_b;
  std::vector<double> match_dist;
  uint64_t n_matched = 0;
  double mean_dist = std::numeric_limits<double>::quiet_NaN();
};
// mean_dist of what is matched: ascending i, in double (what the library's host side does with the fetched match_dist)
inline double mc_mean(const std::vector<int32_t>& match_a, const std::vector<double>& match_dist, uint64_t* n_matched) {
  double s = 0.0;
  uint64_t n = 0;
  for (size_t i = 0; i < match_a.size(); ++i)
    if (match_a[i] >= 0) s += match_dist[i], ++n;
  if (n_matched) *n_matched = n;
  return n ? s / (double)n : std::numeric_limits<double>::quiet_NaN();
}
inline McMatch match_greedy(const double* dist, int na, int nb) {
  McMatch m;
  m.match_a.assign((size_t)na, -1);
  m.match_b.assign((size_t)nb, -1);
  m.match_dist.assign((size_t)na, std::numeric_limits<double>::quiet_NaN());
  std::vector<uint64_t> edge;  // i * nb + j: ascending is (i, j)
  for (int i = 0; i < na; ++i)
    for (int j = 0; j < nb; ++j)
      if (std::isfinite(dist[(size_t)i * nb + j])) edge.push_back((uint64_t)i * nb + j);
  std::stable_sort(edge.begin(), edge.end(), [&](uint64_t x, uint64_t y) { return dist[x] < dist[y]; });
  for (uint64_t e : edge) {
    const int i = (int)(e / nb), j = (int)(e % nb);
    if (m.match_a[i] >= 0 || m.match_b[j] >= 0) continue;
    m.match_a[i] = j;
    m.match_b[j] = i;
    m.match_dist[i] = dist[e];
  }
  m.mean_dist = mc_mean(m.match_a, m.match_dist, &m.n_matched);
  return m;
}
