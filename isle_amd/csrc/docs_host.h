// isle_amd/csrc/docs_host.h — the rule of isle_hip_doc_lengths / isle_hip_doc_duplicates / isle_hip_prune_docs (docs.hip, api_stages.cpp):
// which documents of the count matrix A stay, by their length and by being the first of their kind, and what A becomes.  Plain C++ (no HIP
// type, no isle_ctx): the hash the device sorts by, the argument checks, the lengths, the first-of-its-kind table, the rule and a plain
// loop that builds the pruned CSC from a CSC.  ../host/docs_host_main.cpp applies all of it to a script, tests/test_docs_rule_cpu.py
// checks the answers.
//
// For a local document d of the resident A (its entries are offs[d] .. offs[d + 1]):
//   words[d]    offs[d + 1] - offs[d]: its distinct words (u32)
//   tokens[d]   the sum over its entries of (uint64)count: the truncation th_stats_k applies; exact and order-independent (u64)
//   max_words'  max_words, or no bound where max_words == 0 (likewise max_tokens')
//   passes      min_words <= words[d] <= max_words'  and  min_tokens <= tokens[d] <= max_tokens'
//   equal       two documents are equal when they have the same number of entries, the same rows and the same count BITS, entry by entry
//               (1.0f and the next float up are different documents; all empty documents are equal to each other)
//   first_of[d] with drop_duplicates: the smallest document equal to d (d itself where d is the first of its kind); without it: d
//   kept        passes  and  first_of[d] == d
//   new ids     the kept documents numbered 0 .. new_docs - 1 in ascending old id; kept_docs[new] = the old number IN THE CORPUS
//               (doc_offset + d)
//   new A       the kept documents' columns, entries in order, rows unchanged, counts bit for bit; the vocabulary stays
// Equal documents have equal lengths: either both pass or neither does.  So it does not matter whether duplicates are sought among all
// documents or among the passers, and an implementation may hash only the passers (docs.hip seeks among all: one path for
// isle_hip_doc_duplicates and the prune).
// What is reported: first_of[d] = DOCS_DROPPED for a document dropped by length; a document dropped as a duplicate reports its
// representative's old local number.  dropped[3] counts the documents below the bounds, above them, and the duplicates among the passers;
// the tests run in the order words-min, tokens-min, words-max, tokens-max and the FIRST failing one decides: a document too short in words
// and too long in tokens counts as below.
// Refused before anything is rewritten: no count matrix; min_words > max_words' or min_tokens > max_tokens'; drop_duplicates outside
// {0, 1}; drop_duplicates with several ranks (equality across ranks needs the contents exchanged: out of scope); no document kept in the
// corpus.
//
// The hash is mechanism, equality of content is the rule: the device sorts the documents by docs_hash_cut(hash) and compares contents
// inside every run of equal keys, so the result is the same whatever the hash gives.  DOC_HASH_NARROW cuts it to DOCS_NARROW_BITS bits so
// that every run holds many unequal documents (the tests, the probe).  No measurement stands behind that width: two bits are the fewest
// that still give more than two runs, and the rounds of the resolution grow with the distinct contents per run, so a test corpus of a few
// hundred contents stays at a few hundred rounds.
// How the device deals documents to lanes (docs.hip): a document belongs to one wave, in the hash pass, in the comparisons and in the
// copy; its lanes stride over its entries.  Document lengths are Zipf-like with a long tail, and a one-word document leaves 63 lanes
// idle; a lane per document or a run of entries per workgroup are the alternatives.  No measurement stands behind the choice:
// tools/docs_prune_probe.py times this dealing alone, not the alternatives (README).
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

constexpr uint32_t DOCS_DROPPED = 0xffffffffu;  // first_of[d] of a document dropped by length (a document's number is < 0xfffffff0)
constexpr int DOC_HASH_AUTO = 0, DOC_HASH_FULL = 1, DOC_HASH_NARROW = 2;  // include/isle_hip.h: ISLE_DOC_HASH_*
constexpr int DOCS_NARROW_BITS = 2;

// the 64-bit mix of one entry (the finaliser of splitmix64: a bijection of the 64-bit words) ...
#if defined(__HIPCC__)
#define DOCS_HD __host__ __device__
#else
#define DOCS_HD
#endif
DOCS_HD inline uint64_t docs_mix(uint64_t x) {
  x += 0x9e3779b97f4a7c15ull;
  x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
  x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
  return x ^ (x >> 31);
}
DOCS_HD inline uint64_t docs_entry_hash(uint32_t row, uint32_t count_bits) { return docs_mix(((uint64_t)row << 32) | count_bits); }
// ... the key a document is sorted by, and its width for the radix sort
DOCS_HD inline uint64_t docs_hash_cut(uint64_t h, bool narrow) { return narrow ? h & ((1ull << DOCS_NARROW_BITS) - 1) : h; }
inline int docs_key_bits(bool narrow) { return narrow ? DOCS_NARROW_BITS : 64; }

// a document's hash: the COMMUTATIVE sum (mod 2^64) of its entries' mixes; rows ascend strictly, so the multiset is the content
inline uint64_t docs_hash_host(const uint32_t* rows, const uint32_t* count_bits, int64_t b, int64_t e) {
  uint64_t h = 0;
  for (int64_t i = b; i < e; ++i) h += docs_entry_hash(rows[i], count_bits[i]);
  return h;
}

inline uint64_t docs_token_of(uint32_t count_bits) {
  float f;
  std::memcpy(&f, &count_bits, sizeof(f));
  return (uint64_t)f;  // counts are positive and below 2^32: the truncation is defined
}

struct DocsBounds {
  uint64_t min_words, max_words, min_tokens, max_tokens;  // a maximum of 0: no bound
};
// 0 passes, 1 below, 2 above: the first failing test in the order words-min, tokens-min, words-max, tokens-max
DOCS_HD inline int docs_fails(uint64_t words, uint64_t tokens, uint64_t min_words, uint64_t max_words, uint64_t min_tokens, uint64_t max_tokens) {
  if (words < min_words) return 1;
  if (tokens < min_tokens) return 1;
  if (max_words && words > max_words) return 2;
  if (max_tokens && tokens > max_tokens) return 2;
  return 0;
}

// the argument checks that need no table: empty = accepted, else the refusal's text.  who: "prune_docs" or "doc_duplicates"
inline std::string docs_check_args(const char* who, bool has_A, const DocsBounds& b, int drop_duplicates, int world) {
  char t[240];
  t[0] = 0;
  if (!has_A) snprintf(t, sizeof(t), "%s: no count matrix", who);
  else if (drop_duplicates != 0 && drop_duplicates != 1) snprintf(t, sizeof(t), "%s: drop_duplicates = %d, neither 0 nor 1", who, drop_duplicates);
  else if (drop_duplicates && world > 1)
    snprintf(t, sizeof(t), "%s: duplicates with %d ranks: equality across ranks needs the contents exchanged", who, world);
  else if (b.max_words && b.min_words > b.max_words)
    snprintf(t, sizeof(t), "%s: min_words = %llu > max_words = %llu", who, (unsigned long long)b.min_words, (unsigned long long)b.max_words);
  else if (b.max_tokens && b.min_tokens > b.max_tokens)
    snprintf(t, sizeof(t), "%s: min_tokens = %llu > max_tokens = %llu", who, (unsigned long long)b.min_tokens, (unsigned long long)b.max_tokens);
  return t;
}
inline std::string docs_none_kept(const DocsBounds& b, int drop_duplicates) {
  char t[240];
  snprintf(t, sizeof(t), "prune_docs: no document kept (min_words = %llu, max_words = %llu, min_tokens = %llu, max_tokens = %llu, drop_duplicates = %d)",
           (unsigned long long)b.min_words, (unsigned long long)b.max_words, (unsigned long long)b.min_tokens, (unsigned long long)b.max_tokens, drop_duplicates);
  return t;
}

// offs: D + 1 from 0; counts as their 32 bits
inline void docs_lengths_host(uint64_t D, const int64_t* offs, const uint32_t* count_bits, std::vector<uint32_t>& words, std::vector<uint64_t>& tokens) {
  words.assign((size_t)D, 0);
  tokens.assign((size_t)D, 0);
  for (uint64_t d = 0; d < D; ++d) {
    words[d] = (uint32_t)(offs[d + 1] - offs[d]);
    for (int64_t e = offs[d]; e < offs[d + 1]; ++e) tokens[d] += docs_token_of(count_bits[e]);
  }
}

// first_of[d] = the smallest document equal to d, by content and nothing else (an ordered map of the contents: no hash).  -> the documents
// that are not the first of their kind
inline uint64_t docs_first_of_host(uint64_t D, const int64_t* offs, const uint32_t* count_bits, const uint32_t* rows, std::vector<uint32_t>& first_of) {
  std::map<std::vector<uint64_t>, uint32_t> seen;
  uint64_t dup = 0;
  first_of.assign((size_t)D, 0);
  for (uint64_t d = 0; d < D; ++d) {
    std::vector<uint64_t> content;
    for (int64_t e = offs[d]; e < offs[d + 1]; ++e) content.push_back(((uint64_t)rows[e] << 32) | count_bits[e]);
    const auto at = seen.insert(std::make_pair(std::move(content), (uint32_t)d));
    first_of[d] = at.first->second;
    dup += !at.second;
  }
  return dup;
}

// The rule on one rank's documents: keep (D flags), first_of as reported (D), dropped[3] and the kept documents' number, all this rank's
// own (several ranks: dropped and the kept numbers are summed by the caller, and "no document kept" is decided on the sums).
inline uint64_t docs_rule(uint64_t D, const int64_t* offs, const uint32_t* count_bits, const uint32_t* rows, const DocsBounds& b, int drop_duplicates,
                          std::vector<uint32_t>& keep, std::vector<uint32_t>& first_of, uint64_t dropped[3]) {
  std::vector<uint32_t> words;
  std::vector<uint64_t> tokens;
  docs_lengths_host(D, offs, count_bits, words, tokens);
  if (drop_duplicates) docs_first_of_host(D, offs, count_bits, rows, first_of);
  else {
    first_of.resize((size_t)D);
    for (uint64_t d = 0; d < D; ++d) first_of[d] = (uint32_t)d;
  }
  keep.assign((size_t)D, 0);
  dropped[0] = dropped[1] = dropped[2] = 0;
  uint64_t kept = 0;
  for (uint64_t d = 0; d < D; ++d) {
    const int fails = docs_fails(words[d], tokens[d], b.min_words, b.max_words, b.min_tokens, b.max_tokens);
    if (fails) {
      first_of[d] = DOCS_DROPPED;
      ++dropped[fails - 1];
    } else if (first_of[d] != d) {
      ++dropped[2];
    } else {
      keep[d] = 1;
      ++kept;
    }
  }
  return kept;
}

// ---- the statement of the result: a plain loop ---------------------------------------------------------------------------------------------
// new_offs: kept + 1; new_counts / new_rows: new_offs[kept] entries; kept_docs[new] = doc_offset + old
inline void docs_prune_csc_host(uint64_t D, const int64_t* offs, const uint32_t* count_bits, const uint32_t* rows, const uint32_t* keep, uint64_t doc_offset,
                                std::vector<uint32_t>& kept_docs, std::vector<int64_t>& new_offs, std::vector<uint32_t>& new_count_bits,
                                std::vector<uint32_t>& new_rows) {
  kept_docs.clear();
  new_offs.assign(1, 0);
  new_count_bits.clear();
  new_rows.clear();
  for (uint64_t d = 0; d < D; ++d) {
    if (!keep[d]) continue;
    kept_docs.push_back((uint32_t)(doc_offset + d));
    for (int64_t e = offs[d]; e < offs[d + 1]; ++e) {
      new_count_bits.push_back(count_bits[e]);
      new_rows.push_back(rows[e]);
    }
    new_offs.push_back((int64_t)new_rows.size());
  }
}
