// isle_amd/csrc/simdocs_host.h — the rule of isle_hip_similar_docs (similar_docs.hip, api_stages.cpp): the n documents most similar to each of
// Q query documents, from sparse topic weights that are stored by document.  Plain C++ (no HIP type, no isle_ctx): the weight domain, the
// terms and the scores (ISLE_STAGE_HD: the kernels compile the same functions), the argument checks with the refusal texts, the hash the
// ranks agree the queries by and a plain loop that is the statement of the result.  ../host/simdocs_host_main.cpp applies it to a script,
// tests/test_simdocs_rule_cpu.py checks the answers.
//
// A row is a document's entries (topic, weight), topics ascending strictly; the row's document is doc = doc_base + row.  A query is the same
// kind of list.  Every weight is finite, >= 0 and < 2^31 (-0.0 counts as 0).
// Candidates are structural: row r is a candidate of query q when some topic is STORED in both, whatever the weights, unless
// doc_base + r == exclude[q] (0xffffffff: nothing is excluded).  candidates[q] counts them over all ranks.
// The score of a candidate pair, a the row's and b the query's weight at a common topic, common topics ascending:
//   DOT            s = sum (double)a (double)b                                  score = (float)s
//   COSINE         s likewise; nr = sum over ALL the row's entries (double)a (double)a, nq likewise over the query;
//                  den = sqrtf((float)nr) * sqrtf((float)nq) in fp32            score = den == 0 ? 0 : (float)s / den, the division in fp32
//   BHATTACHARYYA  s = sum (double)sqrtf(a * b), product and root in fp32       score = (float)s    (for distributions: 1 - Hellinger^2)
// A product of two fp32 values is exact in double, so s + a b rounds once with or without an fma; everything else is one IEEE operation.
// The result is topdocs_host.h's with the query in the place of the topic: key = ord(bits(score)) << 32 | ~doc, the larger key wins.
// NOT CERTIFIED: fp32 products a * b that are subnormal (BHATTACHARYYA with weights below 2^-60); the tests keep their weights above.
#pragma once
#include <cmath>

#include "topdocs_host.h"

constexpr int SIM_DOT = 0, SIM_COSINE = 1, SIM_BHATTACHARYYA = 2;  // include/isle_hip.h: ISLE_SIM_*
constexpr int SIMDOCS_MAX_QUERIES = 64;
constexpr uint32_t SIMDOCS_NO_DOC = 0xffffffffu;  // exclude[q]: nothing
constexpr float SIMDOCS_ABSENT = -1.0f;           // the query table's mark: every valid weight is >= 0
constexpr int SIMDOCS_TABLE_AUTO = 0, SIMDOCS_TABLE_LDS = 1, SIMDOCS_TABLE_GLOBAL = 2;  // ISLE_SIMDOCS_TABLE_*
// what sd_count_k names through its atomicMin: (entry << 2) | what; 1 and 2 are topdocs_entry_fault's
constexpr unsigned SIMDOCS_BAD_WEIGHT = 3;

ISLE_STAGE_HD inline bool simdocs_weight_ok(float w) { return w >= 0.0f && w < 2147483648.0f; }  // NaN fails both, -0.0 passes
ISLE_STAGE_HD inline uint32_t simdocs_qp(uint32_t Q) {
  uint32_t p = 1;
  while (p < Q) p <<= 1;
  return p;
}
// one common topic's term of s
ISLE_STAGE_HD inline double simdocs_term(int measure, float a, float b) {
  if (measure == SIM_BHATTACHARYYA) {
    const float p = a * b;
    const float r = sqrtf(p);
    return (double)r;
  }
  return (double)a * (double)b;
}
ISLE_STAGE_HD inline double simdocs_square(float a) { return (double)a * (double)a; }
ISLE_STAGE_HD inline float simdocs_score(int measure, double s, double nr, double nq) {
  const float num = (float)s;
  if (measure != SIM_COSINE) return num;
  const float fr = (float)nr, fq = (float)nq;
  const float rr = sqrtf(fr), rq = sqrtf(fq);
  const float den = rr * rq;
  if (den == 0.0f) return 0.0f;
  const float q = num / den;
  return q;
}

// the argument checks that need no entry: empty = accepted, else the refusal's text
inline std::string simdocs_check_args(int source, int measure, int num_topics, int n, int num_queries, int world, uint64_t doc_base, uint64_t rows) {
  char t[200];
  t[0] = 0;
  if (source != TOPDOCS_INFER && source != TOPDOCS_SUMS && source != TOPDOCS_HOST) snprintf(t, sizeof(t), "similar_docs: unknown source %d", source);
  else if (measure != SIM_DOT && measure != SIM_COSINE && measure != SIM_BHATTACHARYYA) snprintf(t, sizeof(t), "similar_docs: unknown measure %d", measure);
  else if (num_topics < 1) snprintf(t, sizeof(t), "similar_docs: num_topics = %d < 1", num_topics);
  else if (num_queries < 1 || num_queries > SIMDOCS_MAX_QUERIES)
    snprintf(t, sizeof(t), "similar_docs: num_queries = %d not in [1, %d]", num_queries, SIMDOCS_MAX_QUERIES);
  else if (n < 1 || n > TOPDOCS_MAX_N) snprintf(t, sizeof(t), "similar_docs: n = %d not in [1, %d]", n, TOPDOCS_MAX_N);
  else if ((uint64_t)world * (uint64_t)n > TOPDOCS_SORT_KEYS)
    snprintf(t, sizeof(t), "similar_docs: %d ranks x n = %d are more than %llu keys per query", world, n, (unsigned long long)TOPDOCS_SORT_KEYS);
  else if (doc_base > TOPDOCS_DOC_END || rows > TOPDOCS_DOC_END - doc_base)
    snprintf(t, sizeof(t), "similar_docs: doc_base %llu + %llu rows exceed %llu: a document is a 32-bit number <= 0xfffffff0", (unsigned long long)doc_base,
             (unsigned long long)rows, (unsigned long long)TOPDOCS_DOC_END);
  return t;
}
inline std::string simdocs_check_form(int form) {
  char t[80];
  t[0] = 0;
  if (form != SIMDOCS_TABLE_AUTO && form != SIMDOCS_TABLE_LDS && form != SIMDOCS_TABLE_GLOBAL) snprintf(t, sizeof(t), "simdocs_table_form: unknown form %d", form);
  return t;
}
inline std::string simdocs_check_query_rows(const uint64_t* query_rows, int num_queries, uint64_t rows) {
  char t[160];
  t[0] = 0;
  for (int q = 0; q < num_queries && !t[0]; ++q)
    if (query_rows[q] >= rows)
      snprintf(t, sizeof(t), "similar_docs: query_rows[%d] = %llu is not below the %llu rows", q, (unsigned long long)query_rows[q], (unsigned long long)rows);
  return t;
}
inline std::string simdocs_weight_text(const char* whose, uint64_t entry, uint64_t row, float w) {
  char t[200];
  snprintf(t, sizeof(t), "similar_docs: entry %llu (%s %llu) has weight %g: a weight is finite, >= 0 and < 2^31", (unsigned long long)entry, whose,
           (unsigned long long)row, (double)w);
  return t;
}
// the caller's queries, in this order, each condition over all queries before the next: the offsets ascend from 0; every topic < num_topics;
// the topics of a query ascend strictly; the weight domain.  The first offender of the first failing condition is named.
inline std::string simdocs_check_queries(int num_queries, uint32_t num_topics, const int64_t* q_off, const uint32_t* q_topic, const float* q_weight) {
  char t[200];
  t[0] = 0;
  if (q_off[0] != 0) {
    snprintf(t, sizeof(t), "similar_docs: q_offsets[0] = %lld, not 0", (long long)q_off[0]);
    return t;
  }
  for (int q = 0; q < num_queries; ++q)
    if (q_off[q + 1] < q_off[q]) {
      snprintf(t, sizeof(t), "similar_docs: q_offsets descend at query %d", q);
      return t;
    }
  for (int q = 0; q < num_queries; ++q)
    for (int64_t e = q_off[q]; e < q_off[q + 1]; ++e)
      if (q_topic[e] >= num_topics) {
        snprintf(t, sizeof(t), "similar_docs: query entry %lld (query %d) has topic %u >= num_topics %u", (long long)e, q, q_topic[e], num_topics);
        return t;
      }
  for (int q = 0; q < num_queries; ++q)
    for (int64_t e = q_off[q] + 1; e < q_off[q + 1]; ++e)
      if (q_topic[e - 1] >= q_topic[e]) {
        snprintf(t, sizeof(t), "similar_docs: query entry %lld (query %d), topic %u: the topics of a query must ascend strictly", (long long)e, q, q_topic[e]);
        return t;
      }
  for (int q = 0; q < num_queries; ++q)
    for (int64_t e = q_off[q]; e < q_off[q + 1]; ++e)
      if (!simdocs_weight_ok(q_weight[e])) return simdocs_weight_text("query", (uint64_t)e, (uint64_t)q, q_weight[e]);
  return t;
}
// 64-bit FNV-1a over what the ranks of a collective call must share: the queries and the excluded documents
inline uint64_t simdocs_hash_bytes(uint64_t h, const void* p, size_t n) {
  const unsigned char* b = (const unsigned char*)p;
  for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001b3ull;
  return h;
}
inline uint64_t simdocs_query_hash(int num_queries, const int64_t* q_off, const uint32_t* q_topic, const float* q_weight, const uint32_t* exclude) {
  uint64_t h = 0xcbf29ce484222325ull;
  const uint64_t nq = (uint64_t)q_off[num_queries];
  h = simdocs_hash_bytes(h, q_off, ((size_t)num_queries + 1) * sizeof(int64_t));
  h = simdocs_hash_bytes(h, q_topic, nq * sizeof(uint32_t));
  h = simdocs_hash_bytes(h, q_weight, nq * sizeof(float));
  const unsigned char has = exclude ? 1 : 0;
  h = simdocs_hash_bytes(h, &has, 1);
  if (exclude) h = simdocs_hash_bytes(h, exclude, (size_t)num_queries * sizeof(uint32_t));
  return h;
}

// ---- the statement of the rule: a plain loop -------------------------------------------------------------------------------------------------
// off: rows + 1; q_off: Q + 1; exclude: Q documents or null; docs / score_bits: Q x n query-major, unused slots 0xffffffff / bits of 0.0f;
// counts: min(n, candidates[q]).  The inputs are taken as valid (the checks above).
inline void simdocs_select_host(int measure, uint32_t n, uint64_t doc_base, uint64_t rows, const int64_t* off, const uint32_t* topic, const float* weight,
                                uint32_t Q, const int64_t* q_off, const uint32_t* q_topic, const float* q_weight, const uint32_t* exclude, uint32_t* docs,
                                uint32_t* score_bits, uint32_t* counts, uint64_t* candidates) {
  for (uint32_t q = 0; q < Q; ++q) {
    double nq = 0.0;
    for (int64_t f = q_off[q]; f < q_off[q + 1]; ++f) nq += simdocs_square(q_weight[f]);
    std::vector<uint64_t> keys;
    for (uint64_t r = 0; r < rows; ++r) {
      const uint32_t doc = (uint32_t)(doc_base + r);
      if (exclude && exclude[q] != SIMDOCS_NO_DOC && exclude[q] == doc) continue;
      double s = 0.0, nr = 0.0;
      bool common = false;
      int64_t f = q_off[q];
      for (int64_t e = off[r]; e < off[r + 1]; ++e) {
        nr += simdocs_square(weight[e]);
        while (f < q_off[q + 1] && q_topic[f] < topic[e]) ++f;
        if (f < q_off[q + 1] && q_topic[f] == topic[e]) {
          common = true;
          s += simdocs_term(measure, weight[e], q_weight[f]);
        }
      }
      if (!common) continue;
      const float score = simdocs_score(measure, s, nr, nq);
      uint32_t bits;
      static_assert(sizeof(bits) == sizeof(score), "fp32");
      std::copy((const unsigned char*)&score, (const unsigned char*)&score + 4, (unsigned char*)&bits);
      keys.push_back(topdocs_key(bits, doc));
    }
    std::sort(keys.begin(), keys.end(), [](uint64_t a, uint64_t b) { return a > b; });
    const uint32_t m = (uint32_t)std::min<uint64_t>(n, keys.size());
    for (uint32_t i = 0; i < n; ++i) {
      docs[(uint64_t)q * n + i] = i < m ? topdocs_key_doc(keys[i]) : 0xffffffffu;
      score_bits[(uint64_t)q * n + i] = i < m ? topdocs_key_bits(keys[i]) : 0u;
    }
    counts[q] = m;
    candidates[q] = keys.size();
  }
}
