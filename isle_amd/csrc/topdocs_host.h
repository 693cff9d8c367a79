// isle_amd/csrc/topdocs_host.h — the rule of isle_hip_topic_top_docs (topic_docs.hip, api_stages.cpp): the n heaviest documents of every topic,
// selected from (row, topic, value) entries that are stored by document.  Plain C++ (no HIP type, no isle_ctx): the order on value bits, the
// key that carries the document, the way back, the argument checks, the home of the select's bins and a plain loop that is the statement of
// the result.  ../host/topdocs_host_main.cpp applies all of it to a script, tests/test_topdocs_rule_cpu.py checks the answers.
//
// An entry is (row, topic, value): value is fp32 with bits b, the row's document is doc = doc_base + row, a 32-bit number in the corpus.
//   ord(b) = b ^ (b >> 31 ? 0xffffffff : 0x80000000)      the usual order-preserving map: for positive finite values the numeric order
//   key    = (uint64)ord(b) << 32 | (uint32)~doc
// The larger key wins: the heavier value first, the smaller document among bit-equal values (the tie rule ISLE_DOCREPORT_TOPIC_SUMS states).
// Within a topic the keys are distinct (a (row, topic) pair occurs once), and a real key is never 0: doc <= 0xfffffff0, so ~doc >= 0xf.
// The result for topic t: its min(n, cnt_t) largest keys in descending order, cnt_t the topic's entry count over all ranks.
// Values that are not positive finite go by ord as well: -0.0 below +0.0, negatives below both (the more negative the lower), +inf above
// every finite value, a NaN with the sign bit clear above +inf, one with the sign bit set below -inf.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "stage_host.h"  // select_digit, ISLE_STAGE_HD

constexpr int TOPDOCS_INFER = 0, TOPDOCS_SUMS = 1, TOPDOCS_HOST = 2;  // include/isle_hip.h: ISLE_TOPDOCS_*
constexpr int TOPDOCS_MAX_N = 256;
constexpr uint64_t TOPDOCS_SORT_KEYS = 8192;      // world x n keys of a topic sorted in LDS: 64 KiB of keys
constexpr uint64_t TOPDOCS_DOC_END = 0xfffffff1;  // doc_base + rows may not exceed it: doc <= 0xfffffff0
// The select's bins (num_topics x 256 u32) live in LDS, private per workgroup, while they fit in this many bytes: with few topics every
// entry of a wave hits the same few addresses.  64 KiB leaves room for two workgroups in the 160 KiB of a CU.  No measurement stands behind
// the number: the two homes have been timed at different topic counts only (profiles/top_docs_c2.jsonl), never one against the other.
constexpr uint64_t TOPDOCS_LDS_BINS_BYTES = 64 * 1024;

ISLE_STAGE_HD inline uint32_t topdocs_ord(uint32_t b) { return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u); }
ISLE_STAGE_HD inline uint32_t topdocs_unord(uint32_t o) { return o ^ ((o >> 31) ? 0x80000000u : 0xffffffffu); }
ISLE_STAGE_HD inline uint64_t topdocs_key(uint32_t bits, uint32_t doc) { return ((uint64_t)topdocs_ord(bits) << 32) | (uint64_t)(uint32_t)~doc; }
ISLE_STAGE_HD inline uint32_t topdocs_key_doc(uint64_t key) { return ~(uint32_t)key; }
ISLE_STAGE_HD inline uint32_t topdocs_key_bits(uint64_t key) { return topdocs_unord((uint32_t)(key >> 32)); }
// the eight rounds read the byte at shift = 56, 48, .., 0; an entry takes part in a round while its key carries the prefix found so far
ISLE_STAGE_HD inline uint32_t topdocs_key_byte(uint64_t key, int shift) { return (uint32_t)(key >> shift) & 0xffu; }
ISLE_STAGE_HD inline bool topdocs_under_prefix(uint64_t key, uint64_t prefix, int shift) { return shift >= 56 || ((key ^ prefix) >> (shift + 8)) == 0; }
ISLE_STAGE_HD inline bool topdocs_bins_in_lds(uint64_t num_topics) { return num_topics * 256 * sizeof(uint32_t) <= TOPDOCS_LDS_BINS_BYTES; }

// the argument checks that need no entry: empty = accepted, else the refusal's text
inline std::string topdocs_check_args(int source, int num_topics, int n, int world, uint64_t doc_base, uint64_t rows) {
  char t[160];
  t[0] = 0;
  if (source != TOPDOCS_INFER && source != TOPDOCS_SUMS && source != TOPDOCS_HOST) snprintf(t, sizeof(t), "topic_top_docs: unknown source %d", source);
  else if (num_topics < 1) snprintf(t, sizeof(t), "topic_top_docs: num_topics = %d < 1", num_topics);
  else if (n < 1 || n > TOPDOCS_MAX_N) snprintf(t, sizeof(t), "topic_top_docs: n = %d not in [1, %d]", n, TOPDOCS_MAX_N);
  else if ((uint64_t)world * (uint64_t)n > TOPDOCS_SORT_KEYS)
    snprintf(t, sizeof(t), "topic_top_docs: %d ranks x n = %d are more than %llu keys per topic", world, n, (unsigned long long)TOPDOCS_SORT_KEYS);
  else if (doc_base > TOPDOCS_DOC_END || rows > TOPDOCS_DOC_END - doc_base)
    snprintf(t, sizeof(t), "topic_top_docs: doc_base %llu + %llu rows exceed %llu: a document is a 32-bit number <= 0xfffffff0", (unsigned long long)doc_base,
             (unsigned long long)rows, (unsigned long long)TOPDOCS_DOC_END);
  return t;
}
// the caller's offsets: rows + 1 ascending values from 0
inline std::string topdocs_check_offsets(const int64_t* off, uint64_t rows) {
  char t[160];
  t[0] = 0;
  if (off[0] != 0) snprintf(t, sizeof(t), "topic_top_docs: doc_offsets[0] = %lld, not 0", (long long)off[0]);
  for (uint64_t r = 0; r < rows && !t[0]; ++r)
    if (off[r + 1] < off[r]) snprintf(t, sizeof(t), "topic_top_docs: doc_offsets descend at row %llu", (unsigned long long)r);
  return t;
}
// the first entry that breaks a row's form, as the device names it: 0 = none, else (entry << 2) | what, what 1: topic >= num_topics,
// 2: the topics of the row do not ascend strictly at this entry
constexpr unsigned TOPDOCS_BAD_TOPIC = 1, TOPDOCS_BAD_ORDER = 2;
ISLE_STAGE_HD inline unsigned topdocs_entry_fault(uint32_t topic, uint32_t num_topics, bool first_of_row, uint32_t topic_before) {
  if (topic >= num_topics) return TOPDOCS_BAD_TOPIC;
  if (!first_of_row && topic_before >= topic) return TOPDOCS_BAD_ORDER;
  return 0;
}
inline std::string topdocs_fault_text(unsigned what, uint64_t entry, uint64_t row, uint32_t topic, uint32_t num_topics) {
  char t[200];
  if (what == TOPDOCS_BAD_TOPIC)
    snprintf(t, sizeof(t), "topic_top_docs: entry %llu (row %llu) has topic %u >= num_topics %u", (unsigned long long)entry, (unsigned long long)row, topic, num_topics);
  else
    snprintf(t, sizeof(t), "topic_top_docs: entry %llu (row %llu), topic %u: the topics of a row must ascend strictly", (unsigned long long)entry,
             (unsigned long long)row, topic);
  return t;
}

// ---- the statement of the rule: a plain loop -------------------------------------------------------------------------------------------------
// off: rows + 1; docs / values: num_topics x n topic-major, unused slots 0xffffffff / bits of 0.0f; counts: min(n, cnt_t); entries: cnt_t
inline void topdocs_select_host(uint32_t num_topics, uint32_t n, uint64_t doc_base, uint64_t rows, const int64_t* off, const uint32_t* topic,
                                const uint32_t* value_bits, uint32_t* docs, uint32_t* values_bits, uint32_t* counts, uint64_t* entries) {
  std::vector<std::vector<uint64_t>> keys(num_topics);
  for (uint64_t r = 0; r < rows; ++r)
    for (int64_t e = off[r]; e < off[r + 1]; ++e) keys[topic[e]].push_back(topdocs_key(value_bits[e], (uint32_t)(doc_base + r)));
  for (uint32_t t = 0; t < num_topics; ++t) {
    std::sort(keys[t].begin(), keys[t].end(), [](uint64_t a, uint64_t b) { return a > b; });
    const uint32_t m = (uint32_t)std::min<uint64_t>(n, keys[t].size());
    for (uint32_t i = 0; i < n; ++i) {
      docs[(uint64_t)t * n + i] = i < m ? topdocs_key_doc(keys[t][i]) : 0xffffffffu;
      values_bits[(uint64_t)t * n + i] = i < m ? topdocs_key_bits(keys[t][i]) : 0u;
    }
    counts[t] = m;
    entries[t] = keys[t].size();
  }
}

// ---- the device's procedure on the host, over W simulated ranks: what topic_docs.hip and the collectives between its kernels do ------------------
// share q holds rows [cut[q], cut[q + 1]) of the triples.  Per round: every rank's bins, summed; select_digit; after the eighth round the
// prefix is the smallest selected key.  Then every rank collects its keys >= that key into its table, the tables side by side are sorted.
inline void topdocs_rounds_host(uint32_t num_topics, uint32_t n, uint64_t doc_base, uint64_t rows, const int64_t* off, const uint32_t* topic,
                                const uint32_t* value_bits, const std::vector<uint64_t>& cut, uint32_t* docs, uint32_t* values_bits, uint32_t* counts,
                                uint64_t* entries) {
  const size_t W = cut.size() - 1;
  std::vector<std::vector<uint64_t>> key(W);
  std::vector<std::vector<uint32_t>> top(W);
  std::vector<uint64_t> cnt(num_topics, 0);
  for (size_t q = 0; q < W; ++q)
    for (uint64_t r = cut[q]; r < cut[q + 1]; ++r)
      for (int64_t e = off[r]; e < off[r + 1]; ++e) {
        key[q].push_back(topdocs_key(value_bits[e], (uint32_t)(doc_base + r)));
        top[q].push_back(topic[e]);
        cnt[topic[e]]++;
      }
  std::vector<uint64_t> prefix(num_topics, 0);
  std::vector<uint32_t> rem(num_topics), bins((size_t)num_topics * 256);
  for (uint32_t t = 0; t < num_topics; ++t) rem[t] = (uint32_t)std::min<uint64_t>(n, cnt[t]);
  for (int shift = 56; shift >= 0; shift -= 8) {
    std::fill(bins.begin(), bins.end(), 0u);
    for (size_t q = 0; q < W; ++q)  // (the sum over the ranks)
      for (size_t i = 0; i < key[q].size(); ++i)
        if (topdocs_under_prefix(key[q][i], prefix[top[q][i]], shift)) bins[(size_t)top[q][i] * 256 + topdocs_key_byte(key[q][i], shift)]++;
    for (uint32_t t = 0; t < num_topics; ++t) {
      if (!cnt[t]) continue;
      const SelectPick p = select_digit(&bins[(size_t)t * 256], rem[t]);
      prefix[t] |= (uint64_t)p.digit << shift;
      rem[t] = p.remaining;
    }
  }
  std::vector<uint64_t> table(W * (size_t)num_topics * n, 0);
  for (size_t q = 0; q < W; ++q) {
    std::vector<uint32_t> fill(num_topics, 0);
    for (size_t i = 0; i < key[q].size(); ++i) {
      const uint32_t t = top[q][i];
      if (key[q][i] >= prefix[t]) {
        const uint32_t slot = fill[t]++;
        if (slot < n) table[(q * num_topics + t) * n + slot] = key[q][i];
      }
    }
  }
  for (uint32_t t = 0; t < num_topics; ++t) {
    std::vector<uint64_t> k;
    for (size_t q = 0; q < W; ++q)
      for (uint32_t i = 0; i < n; ++i)
        if (table[(q * num_topics + t) * n + i]) k.push_back(table[(q * num_topics + t) * n + i]);
    std::sort(k.begin(), k.end(), [](uint64_t a, uint64_t b) { return a > b; });
    const uint32_t m = (uint32_t)std::min<uint64_t>(n, cnt[t]);
    for (uint32_t i = 0; i < n; ++i) {
      docs[(uint64_t)t * n + i] = i < m && i < k.size() ? topdocs_key_doc(k[i]) : 0xffffffffu;
      values_bits[(uint64_t)t * n + i] = i < m && i < k.size() ? topdocs_key_bits(k[i]) : 0u;
    }
    counts[t] = (uint32_t)std::min<uint64_t>(m, k.size());
    entries[t] = cnt[t];
  }
}
