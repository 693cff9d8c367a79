// isle_amd/csrc/prevalence_host.h — the rule of isle_hip_topic_prevalence (topic_prevalence.hip, api_stages.cpp): how much of the corpus each
// topic is, by group of documents, from sparse topic weights that are stored by document.  Plain C++ (no HIP type, no isle_ctx): the weight
// domain, the terms, the dominant topic, the order of summation, the topic tile, the home of the counters, the argument checks with the
// refusal texts and a plain loop that is the statement of the result.  ../host/prevalence_host_main.cpp applies it to a script,
// tests/test_prevalence_rule_cpu.py checks the answers.
//
// A row is a document's entries (topic, weight), topics ascending strictly.  Every weight is finite, >= 0 and < 2^31; -0.0 counts as 0: its
// term is +0.0.  groups: one uint32 label per row, or none (every row has label 0 and num_groups is 1); PREV_GROUP_NONE: the row belongs to
// no group, it is counted in `unlabelled` and nowhere else (its entries are checked all the same); any other label >= num_groups is refused.
// Per row r:   rs_r = 0.0, then rs_r = rs_r + (double)w over the row's entries in stored order
//              x_r(t) = (double)w for a stored topic, (double)w / rs_r (one IEEE division) with normalise, +0.0 where rs_r == 0 or w == 0;
//              +0.0 for a topic the row does not store
//              the dominant topic: the entry with the largest weight, the smaller topic among equal weights (-0 = +0); none without entries
// Per group g < G and topic t < k, G x k tables group-major:
//   docs[g]        the rows labelled g, rows without entries included
//   count[g,t]     the rows of g that store t, whatever the weight
//   dominant[g,t]  the rows of g whose dominant topic is t
//   sum[g,t]       r_0 < r_1 < .. < r_{n-1} the rows of g ascending: v0_i = x_{r_i}(t);
//                  v(j+1)_i = (((0.0 + vj_{64i}) + vj_{64i+1}) + .. + vj_{64i+63}) over the indices that exist, every + one IEEE double
//                  addition; repeated until one value is left, at least once (n = 1: 0.0 + v0_0); n = 0 gives 0.0.
// The fan-in PREV_FAN = 64 is part of the rule: every level is parallel, and host and device agree bit for bit.  All terms are >= +0.0, so
// adding +0.0 never changes bits: absent terms, empty partials and further levels of one value may be skipped.
// Against the exact rational sum, without normalise, |sum - exact| / exact <= c u / (1 - c u), c = count[g,t], u = 2^-53 (Higham, Accuracy
// and Stability of Numerical Algorithms, 2nd ed., section 4.2: the bound holds for ANY order of summation; absent terms cost no rounding).
// The caller forms mean[g,t] = sum[g,t] / (double)docs[g], NaN where docs[g] == 0.
//
// Device memory of a call, derived (not measured), rows R, entries E, groups G, topics k, tile w = prev_tile(k, form), B = R / 64 + G an
// upper bound of the level-1 blocks: the tables 8 G (1 + 3 k) bytes; per row 8 bytes of row sum (normalise), and with labels 4 (labels)
// + 2 (8 + 4) (sort keys and rows, twice), and the sort's histogram and its offsets, 1.5 R, in the context's scratch, which stays; the
// level bases 8 (L + 1) (G + 1), L <= 6 levels; the partials 8 w (B + B / 64 + G) bytes, reused tile after tile.  A HOST source adds its
// upload, 8 (R + 1) + 8 E.
#pragma once
#include <cmath>
#include <cstring>

#include "topdocs_host.h"  // the sources, the row form, ISLE_STAGE_HD

constexpr uint32_t PREV_FAN = 64;
constexpr uint32_t PREV_GROUP_NONE = 0xffffffffu;       // include/isle_hip.h: ISLE_GROUP_NONE
constexpr uint64_t PREV_MAX_CELLS = 1ull << 24;         // ISLE_PREVALENCE_MAX_CELLS
constexpr int PREV_MAX_TOPICS = 8192;
constexpr uint64_t PREV_MAX_ROWS = 0xffffffffull;       // a row is a 32-bit number in the sorted list
constexpr int PREV_TILE_AUTO = 0, PREV_TILE_WIDE_FORM = 1, PREV_TILE_NARROW_FORM = 2;  // ISLE_PREVALENCE_TILE_*
constexpr uint32_t PREV_TILE_WIDE = 1024, PREV_TILE_NARROW = 64;  // topics per private table: 8 KiB / 512 B of doubles per owner
// what the row pass names through its atomicMin: (entry << 2) | what; 1 and 2 are topdocs_entry_fault's
constexpr unsigned PREV_BAD_WEIGHT = 3;
// The row pass counts in LDS, private per workgroup, while docs, count and dominant (G (2 k + 1) u32) fit in this many bytes, else with
// global atomics: with few cells every entry of a wave hits the same few addresses.  Integer sums: the same numbers either way.  No
// measurement stands behind the number.
constexpr uint64_t PREV_LDS_HIST_BYTES = 32 * 1024;

ISLE_STAGE_HD inline bool prev_weight_ok(float w) { return w >= 0.0f && w < 2147483648.0f; }  // NaN fails both, -0.0 passes
// the topics of one private table: asked is the context's setting (isle_hip_prevalence_tile_form)
ISLE_STAGE_HD inline uint32_t prev_tile(uint32_t num_topics, int asked) {
  const uint32_t tile = asked == PREV_TILE_NARROW_FORM ? PREV_TILE_NARROW : PREV_TILE_WIDE;
  return num_topics < tile ? num_topics : tile;
}
ISLE_STAGE_HD inline bool prev_hist_in_lds(uint64_t num_groups, uint64_t num_topics) {
  return num_groups * (2 * num_topics + 1) * sizeof(uint32_t) <= PREV_LDS_HIST_BYTES;
}
// rs: the row's sum (read with normalise only)
ISLE_STAGE_HD inline double prev_term(float w, int normalise, double rs) {
  if (w == 0.0f) return 0.0;  // -0.0 included
  const double x = (double)w;
  if (!normalise) return x;
  if (rs == 0.0) return 0.0;
  const double q = x / rs;
  return q;
}
// does an entry (topic, w) take the place of the best so far?  Entries come in stored order: topics ascend, so ties keep the earlier one.
ISLE_STAGE_HD inline bool prev_heavier(float w, float best) { return w > best; }
// the levels of the tree above n values: the smallest L >= 1 with ceil(n / 64^L) <= 1 (n = 0: none)
inline int prev_levels(uint64_t n) {
  if (!n) return 0;
  int L = 1;
  for (uint64_t m = (n + PREV_FAN - 1) / PREV_FAN; m > 1; m = (m + PREV_FAN - 1) / PREV_FAN) ++L;
  return L;
}

// the argument checks that need no entry: empty = accepted, else the refusal's text
inline std::string prevalence_check_args(int source, int num_topics, uint64_t num_groups, int normalise, bool has_groups, int world, uint64_t rows) {
  char t[200];
  t[0] = 0;
  if (source != TOPDOCS_INFER && source != TOPDOCS_SUMS && source != TOPDOCS_HOST) snprintf(t, sizeof(t), "topic_prevalence: unknown source %d", source);
  else if (normalise != 0 && normalise != 1) snprintf(t, sizeof(t), "topic_prevalence: normalise = %d, not 0 or 1", normalise);
  else if (num_topics < 1 || num_topics > PREV_MAX_TOPICS) snprintf(t, sizeof(t), "topic_prevalence: num_topics = %d not in [1, %d]", num_topics, PREV_MAX_TOPICS);
  else if (num_groups < 1) snprintf(t, sizeof(t), "topic_prevalence: num_groups = 0 < 1");
  else if (num_groups * (uint64_t)num_topics > PREV_MAX_CELLS)
    snprintf(t, sizeof(t), "topic_prevalence: %llu groups x %d topics are more than %llu cells", (unsigned long long)num_groups, num_topics,
             (unsigned long long)PREV_MAX_CELLS);
  else if (!has_groups && num_groups != 1)
    snprintf(t, sizeof(t), "topic_prevalence: null groups with num_groups = %llu: without labels every row has label 0", (unsigned long long)num_groups);
  else if (world > 1)
    snprintf(t, sizeof(t), "topic_prevalence: %d ranks: a bit-equal sum across ranks needs the list order exchanged, which is not built", world);
  else if (rows > PREV_MAX_ROWS) snprintf(t, sizeof(t), "topic_prevalence: %llu rows, 2^32 or more", (unsigned long long)rows);
  return t;
}
inline std::string prevalence_check_form(int form) {
  char t[80];
  t[0] = 0;
  if (form != PREV_TILE_AUTO && form != PREV_TILE_WIDE_FORM && form != PREV_TILE_NARROW_FORM) snprintf(t, sizeof(t), "prevalence_tile_form: unknown form %d", form);
  return t;
}
inline std::string prevalence_label_text(uint64_t row, uint32_t label, uint32_t num_groups) {
  char t[200];
  snprintf(t, sizeof(t), "topic_prevalence: row %llu has label %u >= num_groups %u (0xffffffff: no group)", (unsigned long long)row, label, num_groups);
  return t;
}
inline std::string prevalence_weight_text(uint64_t entry, uint64_t row, float w) {
  char t[200];
  snprintf(t, sizeof(t), "topic_prevalence: entry %llu (row %llu) has weight %g: a weight is finite, >= 0 and < 2^31", (unsigned long long)entry,
           (unsigned long long)row, (double)w);
  return t;
}
// an entry's fault in the form of its row (what 1, 2: topdocs_entry_fault) or its weight (PREV_BAD_WEIGHT)
inline std::string prevalence_entry_text(unsigned what, uint64_t entry, uint64_t row, uint32_t topic, float w, uint32_t num_topics) {
  if (what == PREV_BAD_WEIGHT) return prevalence_weight_text(entry, row, w);
  return "topic_prevalence: " + topdocs_fault_text(what, entry, row, topic, num_topics).substr(sizeof("topic_top_docs: ") - 1);
}
// The first offenders as the device names them.  *bad_row: the first row with a label that is neither a group nor PREV_GROUP_NONE, else
// ~0; *bad_entry: the smallest (entry << 2) | what, else ~0.  A bad label is reported before a bad entry.
inline void prevalence_first_faults(uint32_t num_topics, uint64_t rows, const int64_t* off, const uint32_t* topic, const float* weight, const uint32_t* groups,
                                    uint32_t num_groups, uint64_t* bad_row, uint64_t* bad_entry) {
  *bad_row = ~0ull;
  *bad_entry = ~0ull;
  for (uint64_t r = 0; r < rows; ++r) {
    if (groups && groups[r] != PREV_GROUP_NONE && groups[r] >= num_groups && *bad_row == ~0ull) *bad_row = r;
    for (int64_t e = off[r]; e < off[r + 1] && *bad_entry == ~0ull; ++e) {
      unsigned what = topdocs_entry_fault(topic[e], num_topics, e == off[r], e == off[r] ? 0u : topic[e - 1]);
      if (!what && !prev_weight_ok(weight[e])) what = PREV_BAD_WEIGHT;
      if (what) *bad_entry = ((uint64_t)e << 2) | what;
    }
  }
}

// ---- the statement of the rule: a plain loop -------------------------------------------------------------------------------------------------
// off: rows + 1; groups: rows labels or null; docs: G; count / dominant / sum: G x k group-major.  The inputs are taken as valid.
inline void prevalence_host(uint32_t num_topics, uint64_t rows, const int64_t* off, const uint32_t* topic, const float* weight, const uint32_t* groups,
                            uint32_t num_groups, int normalise, uint64_t* docs, uint64_t* unlabelled, uint64_t* count, uint64_t* dominant, double* sum) {
  const size_t k = num_topics, G = num_groups;
  std::fill(docs, docs + G, 0ull);
  std::fill(count, count + G * k, 0ull);
  std::fill(dominant, dominant + G * k, 0ull);
  std::fill(sum, sum + G * k, 0.0);
  uint64_t none = 0;
  std::vector<std::vector<uint64_t>> list(G);  // the rows of every group, ascending
  for (uint64_t r = 0; r < rows; ++r) {
    const uint32_t g = groups ? groups[r] : 0u;
    if (g == PREV_GROUP_NONE) {
      ++none;
      continue;
    }
    list[g].push_back(r);
    docs[g]++;
    if (off[r + 1] == off[r]) continue;
    int64_t best = off[r];
    for (int64_t e = off[r]; e < off[r + 1]; ++e) {
      count[g * k + topic[e]]++;
      if (prev_heavier(weight[e], weight[best])) best = e;
    }
    dominant[g * k + topic[best]]++;
  }
  if (unlabelled) *unlabelled = none;
  std::vector<double> cur, next;
  for (size_t g = 0; g < G; ++g) {
    const std::vector<uint64_t>& rs_of = list[g];
    uint64_t n = rs_of.size();
    if (!n) continue;
    // level 1 from the rows: a dense partial per block of 64 rows, the rows in list order, absent terms skipped
    uint64_t m = (n + PREV_FAN - 1) / PREV_FAN;
    cur.assign(m * k, 0.0);
    for (uint64_t i = 0; i < n; ++i) {
      const uint64_t r = rs_of[i];
      double rs = 0.0;
      for (int64_t e = off[r]; e < off[r + 1]; ++e) rs = rs + (double)weight[e];
      double* part = &cur[(i / PREV_FAN) * k];
      for (int64_t e = off[r]; e < off[r + 1]; ++e) part[topic[e]] = part[topic[e]] + prev_term(weight[e], normalise, rs);
    }
    // the levels above: 64 children in order
    for (n = m; n > 1; n = m) {
      m = (n + PREV_FAN - 1) / PREV_FAN;
      next.assign(m * k, 0.0);
      for (uint64_t i = 0; i < n; ++i)
        for (size_t t = 0; t < k; ++t) next[(i / PREV_FAN) * k + t] = next[(i / PREV_FAN) * k + t] + cur[i * k + t];
      cur.swap(next);
    }
    std::copy(cur.begin(), cur.begin() + k, sum + g * k);
  }
}
