// isle_amd/csrc/neardup_host.h — the rule of isle_hip_doc_signatures / isle_hip_doc_jaccard / isle_hip_doc_near_duplicates /
// isle_hip_prune_near_docs (near_dups.hip, api_stages.cpp): which documents of the count matrix A are near copies of an earlier one, by
// MinHash signatures, banding and an exact Jaccard test on the candidates, and what A becomes.  Plain C++ (no HIP type, no isle_ctx): the
// hashes, the argument checks, the signatures, the band keys, the exact set sizes, the resolution across bands and the roots.
// ../host/neardup_host_main.cpp applies all of it to a script, tests/test_neardup_rule_cpu.py checks the answers.  Every quantity is an
// integer; nothing here or on the device is floating point.
//
// For a local document d of the resident A (its entries are offs[d] .. offs[d + 1]):
//   S_d         the rows of its entries (counts are ignored; rows ascend strictly within a column), n_d = |S_d|
//   inter, uni  of two documents: |S_a ∩ S_b| and n_a + n_b - inter
//   similar     inter den >= num uni in 64-bit integers, the threshold the rational num/den with 1 <= num <= den <= 65535.  Two empty
//               documents are similar (0 >= 0), an empty and a non-empty one never (0 >= num n, n >= 1); no special case is written.
//   nd_hash     nd_hash(i, w) = docs_mix(((uint64)(i + 1) << 32) | w), i = 0 .. H - 1, H = bands rows_per_band <= 128
//   sig[d][i]   the minimum over w in S_d of nd_hash(i, w); ~0 in every slot of an empty document
//   key[b][d]   k = 0; for j = 0 .. rows_per_band - 1: k = docs_mix(k ^ sig[d][b rows_per_band + j]).  The NARROW form cuts the key to
//               its DOCS_NARROW_BITS low bits (docs_hash_cut), so that every group holds many dissimilar documents: for the tests.
//   resolution  parent[d] = d.  For b = 0 .. bands - 1 in order: the live documents (parent[d] == d) are grouped by key[b] as the form
//               cuts it; inside a group, in ascending document order, leader clustering: the first document is a leader, every later one
//               is tested against the group's leaders in the order they became leaders, the first similar leader l becomes parent[d] = l,
//               a document similar to none becomes a leader.  A document attached in band b is not live in later bands.
//   parent[d]   the verified neighbour: parent[d] < d and similar(d, parent[d]) for every attached document (P1)
//   first_of[d] the root of the parent chain (chains descend, so they end); kept <=> first_of[d] == d; n_dropped the others
//   pairs_tested  the (document, leader) tests, those the length filter decides included
//   rounds      the largest number of leaders in any group, summed over the bands
//   new A       docs_prune_csc_host of the kept flags: kept documents in ascending old id, kept_docs[new] = doc_offset + old
// The length filter is mechanism and changes no answer: where min(n_a, n_b) den < num max(n_a, n_b) the pair is not similar.  Proof:
// inter <= min(n_a, n_b) and uni >= max(n_a, n_b) (the union holds the larger set), so inter den <= min den < num max <= num uni.
// (P2) Documents with the same word set always share first_of: equal sets have equal signatures, so they fall into the same group in band
// 0 in either form; there they have the same similarities to every leader, so the later one either attaches to the same leader as the
// earlier one, or the earlier one became a leader, to which the later one is similar (inter = uni) unless an earlier leader took it — and
// an earlier leader similar to the later one would have taken the earlier one too.
// (P3) With num == den similar means inter == uni, equal word sets; by P2 the partition is "equal word sets" and first_of[d] the smallest
// document with d's set, in both forms, for every bands / rows_per_band.
// The forms differ in which pairs become candidates, so first_of may differ between FULL and NARROW where num < den: that is the rule.
// Refused before anything is launched or rewritten (texts below): no count matrix; several ranks (similarity across ranks needs the
// contents exchanged: out of scope); num, den, bands, rows_per_band out of range; a pair's document >= the documents there are.
#pragma once
#include <algorithm>
#include <map>

#include "docs_host.h"  // docs_mix, docs_hash_cut, docs_key_bits, docs_prune_csc_host

constexpr int ND_KEY_AUTO = 0, ND_KEY_FULL = 1, ND_KEY_NARROW = 2;  // include/isle_hip.h: ISLE_NEARDUP_KEY_*
constexpr int ND_MAX_BANDS = 64, ND_MAX_ROWS = 8, ND_MAX_H = 128;
constexpr uint32_t ND_MAX_DEN = 65535;
constexpr uint64_t ND_EMPTY_SIG = ~0ull;

DOCS_HD inline uint64_t nd_hash(uint32_t i, uint32_t w) { return docs_mix(((uint64_t)(i + 1) << 32) | w); }
// one step of a band key's fold
DOCS_HD inline uint64_t nd_key_step(uint64_t k, uint64_t sig) { return docs_mix(k ^ sig); }
// the length filter: false = not similar whatever the contents (the proof is above)
DOCS_HD inline bool nd_lengths_allow(uint64_t na, uint64_t nb, uint64_t num, uint64_t den) {
  const uint64_t lo = na < nb ? na : nb, hi = na < nb ? nb : na;
  return lo * den >= num * hi;
}
DOCS_HD inline bool nd_similar(uint64_t inter, uint64_t na, uint64_t nb, uint64_t num, uint64_t den) { return inter * den >= num * (na + nb - inter); }

// the argument checks: empty = accepted, else the refusal's text.  who: "doc_signatures", "doc_jaccard", "doc_near_duplicates" or
// "prune_near_docs" (the first two pass num = den = 1; doc_jaccard bands = rows_per_band = 1 too)
inline std::string nd_check_args(const char* who, bool has_A, uint64_t num, uint64_t den, long long bands, long long rows_per_band, int world) {
  char t[240];
  t[0] = 0;
  if (!has_A) snprintf(t, sizeof(t), "%s: no count matrix", who);
  else if (world > 1)
    snprintf(t, sizeof(t), "%s: near duplicates with %d ranks: similarity across ranks needs the contents exchanged: out of scope", who, world);
  else if (num < 1 || num > den || den > ND_MAX_DEN)
    snprintf(t, sizeof(t), "%s: threshold %llu/%llu, not 1 <= num <= den <= %u", who, (unsigned long long)num, (unsigned long long)den, ND_MAX_DEN);
  else if (bands < 1 || bands > ND_MAX_BANDS || rows_per_band < 1 || rows_per_band > ND_MAX_ROWS || bands * rows_per_band > ND_MAX_H)
    snprintf(t, sizeof(t), "%s: bands = %lld, rows_per_band = %lld, not 1 <= bands <= %d, 1 <= rows_per_band <= %d, bands rows_per_band <= %d", who, bands,
             rows_per_band, ND_MAX_BANDS, ND_MAX_ROWS, ND_MAX_H);
  return t;
}
inline std::string nd_bad_pair(uint64_t at, uint32_t a, uint32_t b, uint64_t D) {
  char t[240];
  snprintf(t, sizeof(t), "doc_jaccard: pair %llu names documents %u and %u of %llu", (unsigned long long)at, a, b, (unsigned long long)D);
  return t;
}
// the first pair that names a document >= D, n_pairs where none does
inline uint64_t nd_first_bad_pair(uint64_t n_pairs, const uint32_t* a, const uint32_t* b, uint64_t D) {
  for (uint64_t i = 0; i < n_pairs; ++i)
    if (a[i] >= D || b[i] >= D) return i;
  return n_pairs;
}

// sig: D x H row-major
inline void nd_signatures_host(uint64_t D, const int64_t* offs, const uint32_t* rows, int H, std::vector<uint64_t>& sig) {
  sig.assign((size_t)D * H, ND_EMPTY_SIG);
  for (uint64_t d = 0; d < D; ++d)
    for (int64_t e = offs[d]; e < offs[d + 1]; ++e)
      for (int i = 0; i < H; ++i) sig[d * H + i] = std::min(sig[d * H + i], nd_hash((uint32_t)i, rows[e]));
}
// keys: bands x D band-major, not cut
inline void nd_keys_host(uint64_t D, const uint64_t* sig, int bands, int rows_per_band, std::vector<uint64_t>& keys) {
  const int H = bands * rows_per_band;
  keys.assign((size_t)bands * D, 0);
  for (int b = 0; b < bands; ++b)
    for (uint64_t d = 0; d < D; ++d) {
      uint64_t k = 0;
      for (int j = 0; j < rows_per_band; ++j) k = nd_key_step(k, sig[d * H + b * rows_per_band + j]);
      keys[(size_t)b * D + d] = k;
    }
}
// |S_a ∩ S_b| by a merge of the two ascending row lists
inline uint32_t nd_inter_host(const int64_t* offs, const uint32_t* rows, uint32_t a, uint32_t b) {
  int64_t i = offs[a], j = offs[b];
  uint32_t n = 0;
  while (i < offs[a + 1] && j < offs[b + 1]) {
    if (rows[i] < rows[j]) ++i;
    else if (rows[j] < rows[i]) ++j;
    else ++n, ++i, ++j;
  }
  return n;
}
inline void nd_jaccard_host(const int64_t* offs, const uint32_t* rows, uint32_t a, uint32_t b, uint32_t* inter, uint32_t* uni) {
  *inter = nd_inter_host(offs, rows, a, b);
  *uni = (uint32_t)((offs[a + 1] - offs[a]) + (offs[b + 1] - offs[b]) - *inter);
}

struct NdResult {
  std::vector<uint32_t> parent, first_of, keep;
  uint64_t n_dropped = 0, pairs_tested = 0, rounds = 0;
};
// The rule on one rank's documents; keys as nd_keys_host gives them.
inline void nd_rule(uint64_t D, const int64_t* offs, const uint32_t* rows, const uint64_t* keys, int bands, bool narrow, uint64_t num, uint64_t den, NdResult& r) {
  r = NdResult();
  r.parent.resize((size_t)D);
  for (uint64_t d = 0; d < D; ++d) r.parent[d] = (uint32_t)d;
  for (int b = 0; b < bands; ++b) {
    std::map<uint64_t, std::vector<uint32_t>> leaders;  // per group, in the order they became leaders
    uint64_t most = 0;
    for (uint64_t d = 0; d < D; ++d) {
      if (r.parent[d] != d) continue;
      std::vector<uint32_t>& ls = leaders[docs_hash_cut(keys[(size_t)b * D + d], narrow)];
      const uint64_t nd = (uint64_t)(offs[d + 1] - offs[d]);
      bool attached = false;
      for (size_t i = 0; i < ls.size() && !attached; ++i) {
        const uint64_t nl = (uint64_t)(offs[ls[i] + 1] - offs[ls[i]]);
        ++r.pairs_tested;
        if (nd_lengths_allow(nd, nl, num, den) && nd_similar(nd_inter_host(offs, rows, (uint32_t)d, ls[i]), nd, nl, num, den)) {
          r.parent[d] = ls[i];
          attached = true;
        }
      }
      if (!attached) {  // (a document attached in this band has parent < d and is passed over by the later documents: they ask parent[x] == x of themselves only)
        ls.push_back((uint32_t)d);
        most = std::max<uint64_t>(most, ls.size());
      }
    }
    r.rounds += most;
  }
  r.first_of.resize((size_t)D);
  r.keep.assign((size_t)D, 0);
  for (uint64_t d = 0; d < D; ++d) {  // parents are smaller: their roots are known
    r.first_of[d] = r.parent[d] == d ? (uint32_t)d : r.first_of[r.parent[d]];
    r.keep[d] = r.first_of[d] == d;
    r.n_dropped += !r.keep[d];
  }
}
