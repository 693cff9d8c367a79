// isle_amd/csrc/score_host.h — the rule of isle_hip_score_docs (score_docs.hip, api_stages.cpp): how well given topic weights predict the
// entries of a sparse matrix of counts, per document.  Plain C++ (no HIP type, no isle_ctx): the weight domain, the product at an entry, which
// entries are scored, the measures, the order of a document's sum, the corpus total, the held-out split, the argument checks with the
// refusal texts and a plain loop that is the statement of the result.  ../host/score_host_main.cpp applies it to a script,
// tests/test_score_rule_cpu.py checks the answers.
//
// The model M is vocab x ncols; document d has a weight row (t_0 < t_1 < .., th_j), topics ascending strictly, every weight finite, >= 0 and
// < 2^31 (prevalence_host.h's domain), and entries (w, c), w < vocab, c finite and >= 0.
//   th'_j = (double)th_j, or with normalise (double)th_j / s_d (one IEEE division), s_d = ((0.0 + (double)th_0) + (double)th_1) + ..; a row
//           with s_d == 0 has no weights under normalise (every z is 0)
//   z     = fma((double)M[w,t_j], th'_j, z) for j = 0, 1, .. from z = 0.0: FUSED, one rounding per stored topic, in double.  Without
//           normalise the product of two fp32 values is exact in double, so fused and unfused give the same bits; with normalise they do
//           not, and fused is the rule (std::fma here, fma() in the kernel).
//   class   z NaN, infinite or negative: unscored.  Else z < floor (z == 0 included; floor > 0): scored at floor and counted in `floored`.
//           Else z == 0: unscored.  Else scored at z.  An unscored entry adds +0.0 to score and tokens at its place, and 1 / (double)c to
//           unscored_entries / unscored_tokens.
//   term    SCORE_LOG: (double)c * log(z), the product rounded once (never fused into the sum); SCORE_PROB: (double)c * z, likewise
//   sums    a document of n entries: lane i < 64 adds the terms of its entries i, i + 64, .. in ascending order from 0.0; then
//           p[i] = p[i] + p[i + s] for s = 32, 16, .., 1, i < s; the sum is p[0].  score, tokens (the (double)c of scored entries) and
//           unscored_tokens are summed so; unscored_entries and floored are integers.  The order depends on n alone.
//   total   score_total: the ascending sequential sum from 0.0, on the host; perplexity = exp(-total score / total tokens) for SCORE_LOG.
// SCORE_PROB without normalise: device and host agree bit for bit (every operation above is one IEEE operation in a stated order).
// SCORE_LOG: the device's log is not the host's; two device calls give the same bits, and against the exact value
//   |score - exact| <= g / (1 - g) sum c |ln z|,  g = (2 K + 1 + m) 2^-53,  m = ceil(n / 64) + 6,  K the ulp error of the device's log
// (profiles/score_certificate.md has the derivation).
// The held-out split: entry (doc, word) is held out when docs_mix(seed ^ ((doc << 32) | word)) % den < num, doc the global document.
#pragma once
#include <cmath>
#include <cstring>

#include "docs_host.h"      // docs_mix
#include "prevalence_host.h"  // prev_weight_ok; topdocs_host.h: the sources, the row form, ISLE_STAGE_HD

constexpr int SCORE_RESIDENT = 0, SCORE_HOST = 1;  // include/isle_hip.h: ISLE_SCORE_RESIDENT / _HOST
constexpr int SCORE_LOG = 0, SCORE_PROB = 1;       // ISLE_SCORE_LOG / _PROB
constexpr uint32_t SCORE_LANES = 64;
constexpr uint32_t SCORE_TILE = 256;  // weight entries staged at a time (score_docs.hip); no result depends on it, no measurement stands behind it
constexpr int SCORE_MAX_COLS = 1024;
constexpr unsigned SCORE_BAD_WEIGHT = 3;               // beside topdocs_entry_fault's 1 and 2: (entry << 2) | what
constexpr unsigned SCORE_BAD_WORD = 0, SCORE_BAD_COUNT = 1;  // an entry of the matrix: (entry << 1) | what
constexpr int SCORE_SCORED = 0, SCORE_FLOORED = 1, SCORE_UNSCORED = 2;

ISLE_STAGE_HD inline bool score_count_ok(float c) { return c >= 0.0f && c <= 3.402823466e+38f; }  // NaN fails, -0.0 passes
ISLE_STAGE_HD inline double score_theta(float w, bool normalise, double s) { return normalise ? (double)w / s : (double)w; }
ISLE_STAGE_HD inline double score_step(double z, float m, double th) { return fma((double)m, th, z); }
// the class of an entry and the value it is scored at
ISLE_STAGE_HD inline int score_class(double z, double floor, double* at) {
  *at = 0.0;
  if (!(z >= 0.0) || z > 1.7976931348623157e308) return SCORE_UNSCORED;  // NaN, negative, infinite
  if (z < floor) {
    *at = floor;
    return SCORE_FLOORED;
  }
  if (z == 0.0) return SCORE_UNSCORED;
  *at = z;
  return SCORE_SCORED;
}
// a * b rounded once, whatever the compiler may contract (hipcc's __dmul_rn is a plain product that it may still fuse into an addition)
ISLE_STAGE_HD inline double score_mul(double a, double b) {
#if defined(__clang__)
#pragma clang fp contract(off)
  return a * b;
#else
  volatile double p = a * b;
  return p;
#endif
}
// the term of an entry scored at `at` (the logarithm is the caller's: log() of the side that runs)
ISLE_STAGE_HD inline double score_term(int measure, float c, double at, double log_at) { return score_mul((double)c, measure == SCORE_LOG ? log_at : at); }
ISLE_STAGE_HD inline bool score_held_out(uint64_t seed, uint64_t doc, uint32_t word, uint64_t num, uint64_t den) {
  return docs_mix(seed ^ ((doc << 32) | (uint64_t)word)) % den < num;
}
inline double score_total(const double* v, uint64_t n) {
  double s = 0.0;
  for (uint64_t i = 0; i < n; ++i) s = s + v[i];
  return s;
}
// the fold of the 64 lane sums
inline double score_fold(double* p) {
  for (uint32_t s = SCORE_LANES / 2; s; s >>= 1)
    for (uint32_t i = 0; i < s; ++i) p[i] = p[i] + p[i + s];
  return p[0];
}

// ---- the argument checks that need no entry: empty = accepted, else the refusal's text ------------------------------------------------------
inline std::string score_check_args(int weights_source, int entries_source, int measure, int normalise, double floor, int ncols) {
  char t[200];
  t[0] = 0;
  if (weights_source != TOPDOCS_INFER && weights_source != TOPDOCS_HOST)
    snprintf(t, sizeof(t), "score_docs: unknown weights source %d (ISLE_TOPDOCS_INFER or ISLE_TOPDOCS_HOST)", weights_source);
  else if (entries_source != SCORE_RESIDENT && entries_source != SCORE_HOST) snprintf(t, sizeof(t), "score_docs: unknown entries source %d", entries_source);
  else if (measure != SCORE_LOG && measure != SCORE_PROB) snprintf(t, sizeof(t), "score_docs: unknown measure %d", measure);
  else if (normalise != 0 && normalise != 1) snprintf(t, sizeof(t), "score_docs: normalise = %d, not 0 or 1", normalise);
  else if (!(floor >= 0.0) || floor > 1.7976931348623157e308) snprintf(t, sizeof(t), "score_docs: floor = %g, not finite and >= 0", floor);
  else if (ncols < 1 || ncols > SCORE_MAX_COLS) snprintf(t, sizeof(t), "score_docs: ncols = %d not in [1, %d]", ncols, SCORE_MAX_COLS);
  return t;
}
inline std::string score_rows_text(uint64_t num_rows, uint64_t have, const char* of_what) {
  char t[200];
  snprintf(t, sizeof(t), "score_docs: num_rows = %llu, %s has %llu rows", (unsigned long long)num_rows, of_what, (unsigned long long)have);
  return t;
}
inline std::string score_range_text(uint64_t doc_begin, uint64_t num_rows, uint64_t docs) {
  char t[200];
  snprintf(t, sizeof(t), "score_docs: documents [%llu, %llu + %llu) of %llu", (unsigned long long)doc_begin, (unsigned long long)doc_begin,
           (unsigned long long)num_rows, (unsigned long long)docs);
  return t;
}
inline std::string score_begin_text(uint64_t doc_begin, uint64_t inf_begin) {
  char t[200];
  snprintf(t, sizeof(t), "score_docs: doc_begin = %llu, the resident inference result begins at document %llu", (unsigned long long)doc_begin,
           (unsigned long long)inf_begin);
  return t;
}
inline std::string score_vocab_text(uint64_t vocab, uint64_t have) {
  char t[200];
  snprintf(t, sizeof(t), "score_docs: the model has %llu words, the count matrix %llu", (unsigned long long)vocab, (unsigned long long)have);
  return t;
}
// the caller's offsets (what: "w_offsets" or "offsets"): rows + 1 ascending values from 0
inline std::string score_check_offsets(const char* what, const int64_t* off, uint64_t rows) {
  char t[200];
  t[0] = 0;
  if (off[0] != 0) snprintf(t, sizeof(t), "score_docs: %s[0] = %lld, not 0", what, (long long)off[0]);
  for (uint64_t r = 0; r < rows && !t[0]; ++r)
    if (off[r + 1] < off[r]) snprintf(t, sizeof(t), "score_docs: %s descend at row %llu", what, (unsigned long long)r);
  return t;
}
// a weight entry's fault (what 1, 2: topdocs_entry_fault; SCORE_BAD_WEIGHT)
inline std::string score_weight_text(unsigned what, uint64_t entry, uint64_t row, uint32_t topic, float w, uint32_t ncols) {
  if (what == SCORE_BAD_WEIGHT) {
    char t[200];
    snprintf(t, sizeof(t), "score_docs: weight entry %llu (row %llu) has weight %g: a weight is finite, >= 0 and < 2^31", (unsigned long long)entry,
             (unsigned long long)row, (double)w);
    return t;
  }
  return "score_docs: weight " + topdocs_fault_text(what, entry, row, topic, ncols).substr(sizeof("topic_top_docs: ") - 1);
}
// an entry's fault (SCORE_BAD_WORD, SCORE_BAD_COUNT)
inline std::string score_entry_text(unsigned what, uint64_t entry, uint64_t row, uint32_t word, float c, uint64_t vocab) {
  char t[200];
  if (what == SCORE_BAD_WORD)
    snprintf(t, sizeof(t), "score_docs: entry %llu (document %llu) has word %u >= vocab %llu", (unsigned long long)entry, (unsigned long long)row, word,
             (unsigned long long)vocab);
  else
    snprintf(t, sizeof(t), "score_docs: entry %llu (document %llu) has count %g: a count is finite and >= 0", (unsigned long long)entry,
             (unsigned long long)row, (double)c);
  return t;
}
// The first offenders as the device names them: *bad_weight the smallest (entry << 2) | what over the weight rows, *bad_entry the smallest
// (entry << 1) | what over the entries, ~0 = none.  A bad weight entry is reported before a bad entry.
inline void score_first_faults(uint32_t ncols, uint64_t vocab, uint64_t rows, const int64_t* w_off, const uint32_t* w_topic, const float* w_weight,
                               const float* cnt, const uint32_t* word, const int64_t* off, uint64_t* bad_weight, uint64_t* bad_entry) {
  *bad_weight = *bad_entry = ~0ull;
  for (uint64_t r = 0; r < rows; ++r) {
    for (int64_t e = w_off[r]; e < w_off[r + 1] && *bad_weight == ~0ull; ++e) {
      unsigned what = topdocs_entry_fault(w_topic[e], ncols, e == w_off[r], e == w_off[r] ? 0u : w_topic[e - 1]);
      if (!what && !prev_weight_ok(w_weight[e])) what = SCORE_BAD_WEIGHT;
      if (what) *bad_weight = ((uint64_t)e << 2) | what;
    }
    for (int64_t e = off[r]; e < off[r + 1] && *bad_entry == ~0ull; ++e) {
      if (word[e] >= vocab) *bad_entry = ((uint64_t)e << 1) | SCORE_BAD_WORD;
      else if (!score_count_ok(cnt[e])) *bad_entry = ((uint64_t)e << 1) | SCORE_BAD_COUNT;
    }
  }
}

// ---- the statement of the rule: a plain loop -------------------------------------------------------------------------------------------------
// model: vocab x ncols column-major (the C ABI's layout).  w_off / off: rows + 1 (off may begin above 0: positions in cnt / word).  The five
// outputs: rows each.  z_out: null, or z of entry e at z_out[e - off[0]].  The inputs are taken as valid.
inline void score_docs_host(uint32_t ncols, uint64_t vocab, const float* model, uint64_t rows, const int64_t* w_off, const uint32_t* w_topic,
                            const float* w_weight, const float* cnt, const uint32_t* word, const int64_t* off, int measure, int normalise, double floor,
                            double* score, double* tokens, uint32_t* unscored_entries, double* unscored_tokens, uint32_t* floored, double* z_out) {
  (void)ncols;
  for (uint64_t r = 0; r < rows; ++r) {
    double s = 0.0;
    for (int64_t j = w_off[r]; j < w_off[r + 1]; ++j) s = s + (double)w_weight[j];
    const bool none = normalise && s == 0.0;
    double ps[SCORE_LANES], pt[SCORE_LANES], pu[SCORE_LANES];
    for (uint32_t i = 0; i < SCORE_LANES; ++i) ps[i] = pt[i] = pu[i] = 0.0;
    uint32_t ue = 0, fl = 0;
    for (int64_t e = off[r]; e < off[r + 1]; ++e) {
      const uint32_t lane = (uint32_t)((e - off[r]) % SCORE_LANES);
      double z = 0.0;
      if (!none)
        for (int64_t j = w_off[r]; j < w_off[r + 1]; ++j)
          z = score_step(z, model[(size_t)w_topic[j] * vocab + word[e]], score_theta(w_weight[j], normalise != 0, s));
      if (z_out) z_out[e - off[0]] = z;
      double at;
      const int cls = score_class(z, floor, &at);
      if (cls == SCORE_UNSCORED) {
        ++ue;
        pu[lane] = pu[lane] + (double)cnt[e];
        continue;  // (a lane sum begins at +0.0 and so is never -0.0: adding +0.0 changes no bits and may be skipped)
      }
      if (cls == SCORE_FLOORED) ++fl;
      ps[lane] = ps[lane] + score_term(measure, cnt[e], at, measure == SCORE_LOG ? std::log(at) : 0.0);
      pt[lane] = pt[lane] + (double)cnt[e];
    }
    score[r] = score_fold(ps);
    tokens[r] = score_fold(pt);
    unscored_tokens[r] = score_fold(pu);
    unscored_entries[r] = ue;
    floored[r] = fl;
  }
}
