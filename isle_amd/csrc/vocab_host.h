// isle_amd/csrc/vocab_host.h — the rule of isle_hip_word_doc_freq / isle_hip_prune_vocab (vocab.hip, api_stages.cpp): which words of the count
// matrix A stay, by the number of documents that hold them, and what A becomes.  Plain C++ (no HIP type, no isle_ctx): the key of the keep_n
// cut, the argument checks, the rule on a table of document frequencies and a plain loop that builds the pruned CSC from a CSC.
// ../host/vocab_host_main.cpp applies all of it to a script, tests/test_vocab_rule_cpu.py checks the answers.
//
//   df[w]     the documents of the whole corpus (all ranks) whose column of A holds word w; a column holds a word at most once: its entries
//   max_df'   max_df, or the corpus's document count where max_df == 0
//   passes    min_df <= df[w] <= max_df'
//   keep_n    > 0 and more than keep_n words pass: only the keep_n passers with the largest key (uint64)df[w] << 32 | (uint32)~w stay:
//             the larger df wins, the smaller word id among equal df
//   new ids   the kept words are numbered 0 .. newV - 1 in ascending old id, kept_words[new] = old: every column stays sorted
//   new A     every document keeps its entries of kept words in their order, counts bit for bit, rows renumbered; D, the document offset
//             and the corpus's document count stay; a document may become empty
//   emptied   the documents that had entries and have none afterwards
// Refused before anything is rewritten: no count matrix, min_df > max_df', keep_n >= 2^32, no word kept.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <string>
#include <vector>

constexpr uint32_t VOCAB_DROPPED = 0xffffffffu;  // remap[w] of a word that goes (a kept word's is its new id < newV <= 0xfffffff0)
constexpr int VOCAB_HIST_AUTO = 0, VOCAB_HIST_LDS = 1, VOCAB_HIST_GLOBAL = 2;  // include/isle_hip.h: ISLE_VOCAB_HIST_*
// Words per vocabulary part of the document-frequency kernel's workgroup-private counters (vocab.hip vocab_df_lds_k): 16384 32-bit counters
// are 64 KiB of LDS, what a kernel gets without asking for more, and leave room for two workgroups in the 160 KiB of a CU.  A workgroup
// walks its run of entries once per part (the run stays in L2), so a vocabulary of 100 k words costs seven walks.  No measurement stands
// behind the number: tools/vocab_prune_probe.py times the two forms of the kernel against each other, not part sizes.
constexpr uint32_t VOCAB_DF_PART = 16384;

inline uint64_t vocab_key(uint32_t df, uint32_t w) { return ((uint64_t)df << 32) | (uint64_t)(uint32_t)~w; }
inline uint64_t vocab_max_df(uint64_t max_df, uint64_t docs_global) { return max_df ? max_df : docs_global; }
inline uint32_t vocab_df_parts(uint64_t V) { return (uint32_t)((V + VOCAB_DF_PART - 1) / VOCAB_DF_PART); }

// the argument checks that need no table: empty = accepted, else the refusal's text
inline std::string vocab_check_args(bool has_A, uint64_t min_df, uint64_t max_df, uint64_t keep_n, uint64_t docs_global) {
  char t[200];
  t[0] = 0;
  const uint64_t top = vocab_max_df(max_df, docs_global);
  if (!has_A) snprintf(t, sizeof(t), "prune_vocab: no count matrix");
  else if (min_df > top)
    snprintf(t, sizeof(t), "prune_vocab: min_df = %llu > max_df = %llu%s", (unsigned long long)min_df, (unsigned long long)top,
             max_df ? "" : " (the corpus's document count)");
  else if (keep_n >= (1ull << 32)) snprintf(t, sizeof(t), "prune_vocab: keep_n = %llu, 2^32 or more", (unsigned long long)keep_n);
  return t;
}

// df of one CSC (added to df: the shards of a corpus one after the other)
inline void vocab_df_host(uint64_t D, const int64_t* offs, const uint32_t* rows, uint32_t* df) {
  for (int64_t e = offs[0]; e < offs[D]; ++e) df[rows[e]]++;
}

// The rule on the table: remap (V entries: the new id, or VOCAB_DROPPED) and kept_words (newV entries).  Empty = accepted, else the
// refusal's text (no word kept); the arguments have passed vocab_check_args.
inline std::string vocab_rule(const uint32_t* df, uint64_t V, uint64_t min_df, uint64_t max_df, uint64_t keep_n, uint64_t docs_global,
                              std::vector<uint32_t>& remap, std::vector<uint32_t>& kept_words) {
  const uint64_t top = vocab_max_df(max_df, docs_global);
  std::vector<uint64_t> keys;
  for (uint64_t w = 0; w < V; ++w)
    if (df[w] >= min_df && df[w] <= top) keys.push_back(vocab_key(df[w], (uint32_t)w));
  if (keep_n && keys.size() > keep_n) {
    std::nth_element(keys.begin(), keys.begin() + (size_t)keep_n, keys.end(), std::greater<uint64_t>());  // the keys are distinct: the cut is one set
    keys.resize((size_t)keep_n);
  }
  remap.assign((size_t)V, VOCAB_DROPPED);
  kept_words.clear();
  for (uint64_t key : keys) remap[~(uint32_t)key] = 0;
  for (uint64_t w = 0; w < V; ++w)
    if (remap[w] != VOCAB_DROPPED) {
      remap[w] = (uint32_t)kept_words.size();
      kept_words.push_back((uint32_t)w);
    }
  char t[200];
  t[0] = 0;
  if (kept_words.empty())
    snprintf(t, sizeof(t), "prune_vocab: no word kept (min_df = %llu, max_df = %llu, keep_n = %llu)", (unsigned long long)min_df, (unsigned long long)top,
             (unsigned long long)keep_n);
  return t;
}

// ---- the statement of the result: a plain loop ---------------------------------------------------------------------------------------------
// offs: D + 1 from 0; counts as their 32 bits.  new_offs: D + 1; new_counts / new_rows: new_offs[D] entries.  -> the documents emptied
inline uint64_t vocab_prune_csc_host(uint64_t D, const int64_t* offs, const uint32_t* count_bits, const uint32_t* rows, const uint32_t* remap,
                                     std::vector<int64_t>& new_offs, std::vector<uint32_t>& new_count_bits, std::vector<uint32_t>& new_rows) {
  uint64_t emptied = 0;
  new_offs.assign(1, 0);
  new_count_bits.clear();
  new_rows.clear();
  for (uint64_t d = 0; d < D; ++d) {
    for (int64_t e = offs[d]; e < offs[d + 1]; ++e)
      if (remap[rows[e]] != VOCAB_DROPPED) {
        new_count_bits.push_back(count_bits[e]);
        new_rows.push_back(remap[rows[e]]);
      }
    new_offs.push_back((int64_t)new_rows.size());
    if (offs[d + 1] > offs[d] && new_offs[d + 1] == new_offs[d]) ++emptied;
  }
  return emptied;
}
