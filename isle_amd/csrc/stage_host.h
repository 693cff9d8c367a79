// isle_amd/csrc/stage_host.h — what the stages either side of the hot path (api_stages.cpp) decide on the host: the corpus average and its
// limit, the two thresholding counts, the sampling keys, their pivot over all ranks and the drop mask, a shard's place in B's columns, the
// plan and the sums of the UMass coherence, the digit pick and the chunk plan of the distributed select, the slices of the gathered topic sums, the top-five count rule, the diversity average and the line of a byte.  Plain C++ (no HIP type,
// no isle_ctx, nothing read from the environment), so that rules whose mistakes do not fault but keep other documents run without a device
// and without a transport: ../host/stage_host_main.cpp applies them to a script, tests/test_stage_host_cpu.py checks the answers.  Operand
// types, casts and the order of every float and double operation are the reference's, as cited: no build of it takes -ffast-math.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <string>
#include <vector>

// ---- corpus statistics (src/sparseMatrix.cpp:92-99) ------------------------------------------------------------------------------------------
inline float corpus_avg(uint64_t tokens, uint64_t nz_docs) { return (float)(tokens / std::max<uint64_t>(nz_docs, 1)); }  // :98, integer division
// the largest rounded value the per-word histogram counts; false: the average is refused (the histogram's values are 16 bits wide)
inline bool hist_maxv(float avg, uint32_t* maxv) {
  const uint64_t maxv64 = (uint64_t)avg + 2;
  if (maxv64 > 65535) return false;
  *maxv = (uint32_t)maxv64;
  return true;
}

// ---- thresholds (src/sparseMatrix.cpp:367-368): float operands, double arithmetic ---------------------------------------------------------------
struct ThresholdCounts {
  uint64_t gr, eq;
};
inline ThresholdCounts threshold_counts(uint64_t nz_docs, uint64_t num_topics) {
  uint64_t count_gr = (uint64_t)(1.0 * (float)nz_docs / (2.0 * (float)num_topics));
  uint64_t count_eq = (uint64_t)std::ceil(3.0 * (1.0 / 60.0) * 1.0 * (float)nz_docs / (float)num_topics);
  if (count_gr == 0) count_gr = 1;
  if (count_eq == 0) count_eq = 1;
  return {count_gr, count_eq};
}

// ---- sampled_threshold_and_copy, src/sparseMatrix.cpp:1383-1415 (keys on the host, like the reference) ---------------------------------------
// Several ranks: a document's key depends on its GLOBAL number only, the pivot is the (rate x D_global)-th largest key of the whole corpus —
// every rank gathers all keys (padded to the largest shard) and selects the same pivot; what a shard keeps is what the single-rank run
// keeps of those documents.
inline float sample_key(uint64_t seed, uint64_t d /*the document's number in the corpus*/, float weight) {
  uint64_t z = (seed + 1) * 0x9E3779B97F4A7C15ull ^ (d * 0xD1342543DE82EF95ull);
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z = z ^ (z >> 31);
  const double u = (double)(z >> 11) * (1.0 / 9007199254740992.0);
  return (weight == 0.f) ? 0.f : (float)std::pow(u, 1.0 / (double)weight);
}
// the keys of a shard whose first document is number doc_offset of the corpus
inline std::vector<float> sample_keys(uint64_t seed, uint64_t doc_offset, const std::vector<float>& weight) {
  std::vector<float> key(weight.size());
  for (uint64_t dl = 0; dl < key.size(); ++dl) key[dl] = sample_key(seed, doc_offset + dl, weight[dl]);
  return key;
}
// a shard's keys as it sends them to the all-gather: padded with -1 to the largest shard's count (one slot where every shard is empty)
inline std::vector<float> sample_pad(const std::vector<float>& keys, uint64_t dmax) {
  if (dmax == 0) dmax = 1;
  std::vector<float> mine(dmax, -1.f);
  std::copy(keys.begin(), keys.end(), mine.begin());
  return mine;
}
// dice: every key of the corpus, with or without padding (stripped and reordered here)
inline float sample_pivot(double rate, std::vector<float>& dice) {
  dice.erase(std::remove_if(dice.begin(), dice.end(), [](float v) { return !(v >= 0.f); }), dice.end());
  const size_t Dg = dice.size();
  float pivot = 2.f;  // (an empty corpus keeps nothing)
  if (Dg) {
    const size_t nth = std::min<size_t>((size_t)((float)rate * (float)Dg), Dg - 1);
    std::nth_element(dice.begin(), dice.begin() + nth, dice.end(), std::greater<float>());
    pivot = dice[nth];
  }
  return pivot;
}
inline std::vector<uint8_t> drop_mask(const std::vector<float>& key, float pivot) {  // one slot at least: it sizes a device buffer
  std::vector<uint8_t> drop(key.empty() ? 1 : key.size());
  for (size_t d = 0; d < key.size(); ++d) drop[d] = !(key[d] >= pivot);
  return drop;
}

// ---- placement of a shard in B's global column numbering: kept[r] columns on rank r ---------------------------------------------------------------
struct ShardPlace {
  uint64_t b_off, b_glob;
};
inline ShardPlace shard_placement(int rank, const std::vector<uint64_t>& kept) {
  ShardPlace s = {0, 0};
  for (int r = 0; r < (int)kept.size(); ++r) {
    if (r == rank) s.b_off = s.b_glob;
    s.b_glob += kept[r];
  }
  return s;
}

// ---- UMass coherence (src/sparseMatrix.cpp:841-1016): what is counted, and the sums over the counts ---------------------------------------------
struct CoherencePlan {
  size_t n = 0, m = 0, npt = 0;  // topics, top words per topic, pairs per topic
  std::string refused;           // why there is no plan, in the caller's words; empty: there is one
  // U: distinct words ascending, local id = rank; P: distinct (lo, hi) pairs of local ids, sorted, as a CSR keyed by lo
  std::vector<uint32_t> U, loc, part_off, part_hi;
  std::vector<uint64_t> keys, P;
  CoherencePlan(const uint32_t* top_words, size_t num_topics, size_t M, uint64_t vocab) : n(num_topics), m(M), npt(M * (M - 1) / 2) {
    char text[128];
    for (size_t t = 0; t < n; ++t) {
      const uint32_t* w = top_words + t * m;
      for (size_t i = 0; i < m; ++i) {
        if (w[i] >= vocab) {
          snprintf(text, sizeof(text), "topic_coherence: word %u of topic %zu >= vocab %llu", w[i], t, (unsigned long long)vocab);
          refused = text;
          return;
        }
        for (size_t j = 0; j < i; ++j)
          if (w[j] == w[i]) {
            snprintf(text, sizeof(text), "topic_coherence: word %u repeats in topic %zu", w[i], t);
            refused = text;
            return;
          }
      }
    }
    U.assign(top_words, top_words + n * m);
    std::sort(U.begin(), U.end());
    U.erase(std::unique(U.begin(), U.end()), U.end());
    loc.resize(n * m);
    for (size_t i = 0; i < n * m; ++i) loc[i] = (uint32_t)(std::lower_bound(U.begin(), U.end(), top_words[i]) - U.begin());
    keys.reserve(n * npt);
    for (size_t t = 0; t < n; ++t)
      for (size_t i = 1; i < m; ++i)
        for (size_t j = 0; j < i; ++j) {
          const uint64_t a = loc[t * m + i], b = loc[t * m + j];
          keys.push_back(a < b ? (a << 32 | b) : (b << 32 | a));
        }
    P = keys;
    std::sort(P.begin(), P.end());
    P.erase(std::unique(P.begin(), P.end()), P.end());
    part_off.assign(U.size() + 1, 0u);
    part_hi.resize(P.size());
    for (size_t p = 0; p < P.size(); ++p) {
      part_off[(P[p] >> 32) + 1]++;
      part_hi[p] = (uint32_t)P[p];
    }
    for (size_t u = 0; u < U.size(); ++u) part_off[u + 1] += part_off[u];
  }
};
// cnt: the document frequencies of U, then of P (|U| + |P| entries).  coherence: n; doc_freq: n x m or null; co_doc_freq: n x npt or null
inline void coherence_sums(const CoherencePlan& pl, const uint32_t* cnt, double eps, double* coherence, uint64_t* doc_freq, uint64_t* co_doc_freq) {
  const size_t n = pl.n, m = pl.m, npt = pl.npt;
  const uint32_t* du = cnt;
  const uint32_t* dp = cnt + pl.U.size();
  for (size_t t = 0; t < n; ++t) {
    double sum = 0.0;
    bool undefined = false;
    for (size_t i = 1; i < m; ++i)
      for (size_t j = 0; j < i; ++j) {
        const uint64_t key = pl.keys[t * npt + i * (i - 1) / 2 + j];
        const uint32_t dij = dp[std::lower_bound(pl.P.begin(), pl.P.end(), key) - pl.P.begin()], dj = du[pl.loc[t * m + j]];
        if (dj == 0) undefined = true;
        sum += std::log((double)dij + eps) - std::log((double)dj);
        if (co_doc_freq) co_doc_freq[t * npt + i * (i - 1) / 2 + j] = dij;
      }
    coherence[t] = undefined ? std::nan("") : sum;
    if (doc_freq)
      for (size_t i = 0; i < m; ++i) doc_freq[t * m + i] = du[pl.loc[t * m + i]];
  }
}

// ---- the distributed radix select of the stage downstream (post.hip post_select_hist_k / post_select_step_k) ---------------------------------
// With several ranks the values of a segment (the normalised counts of a word over the documents of a cluster; the sums of a topic) lie on
// different ranks.  The r-th largest is found from the float bits, eight at a time from the top (all values are positive: unsigned order is
// float order): every rank counts its own values under the prefix found so far into 256 bins, the bins are summed over the ranks, and every
// rank picks the next digit from the same integers by the rule post_select_k's thread 0 applies within one workgroup.
#if defined(__HIPCC__)
#define ISLE_STAGE_HD __host__ __device__
#else
#define ISLE_STAGE_HD
#endif
struct SelectPick {
  uint32_t digit, remaining;
};
// bins: the counts of the 256 values of a digit; remaining >= 1: the rank (1-based, from the largest) still to go among them.  The digit
// is the largest d whose values together with all above reach the rank; what remains is the rank among the values of digit d.  A rank
// past all the values (which no caller asks for) ends in digit 0.
ISLE_STAGE_HD inline SelectPick select_digit(const uint32_t* bins, uint32_t remaining) {
  uint32_t cum = 0;
  int d = 255;
  for (; d > 0; --d) {
    if (cum + bins[d] >= remaining) break;
    cum += bins[d];
  }
  SelectPick p = {(uint32_t)d, remaining - cum};
  return p;
}
// the bits already fixed ahead of the pass that reads the digit at `shift` (24, 16, 8, 0)
ISLE_STAGE_HD inline uint32_t select_mask(int shift) { return shift >= 24 ? 0u : 0xffffffffu << (shift + 8); }
// The slots (segments) are walked in chunks, one all-reduce of chunk x 256 bins per chunk and pass, so that the table of bins stays bounded.
// The size is a number nobody has measured: 64 MiB of bins per all-reduce, 65 536 slots, to begin with.
constexpr uint64_t SELECT_BINS_BYTES = 64ull << 20;
constexpr uint64_t SELECT_CHUNK_SLOTS = SELECT_BINS_BYTES / (256 * sizeof(uint32_t));
struct SlotChunk {
  uint64_t first, count;
};
inline uint64_t select_chunks(uint64_t nslots, uint64_t chunk_slots) { return (nslots + chunk_slots - 1) / chunk_slots; }
inline SlotChunk select_chunk(uint64_t nslots, uint64_t chunk_slots, uint64_t i) {
  const uint64_t first = std::min(nslots, i * chunk_slots);
  SlotChunk s = {first, std::min(chunk_slots, nslots - first)};
  return s;
}

// ---- document bounds of `parts` shards balanced by weight (isle_hip_plan_shards: entries; the tdf counting stream, tdf_plan_k: lines) ----------
// offs: num_docs + 1 ascending offsets of the weights, offs[0] = 0, offs[num_docs] = total.  Bound p (0 < p < parts) is the first document d
// with offs[d] >= floor(total * p / parts), never above num_docs and never below `before`, the bound p - 1.  The target is formed without
// 128-bit arithmetic: total = q * parts + r gives q * p + floor(r * p / parts), and r * p < parts * p < 2^62.  Targets ascend with p, so the
// chain of `before` equals max(bound p - 1 found alone, bound p found alone): a thread per bound computes both.
ISLE_STAGE_HD inline int64_t plan_target(int64_t total, int p, int parts) {
  const int64_t q = total / parts, r = total % parts;
  return q * p + (r * p) / parts;
}
ISLE_STAGE_HD inline uint64_t plan_bound(const int64_t* offs, uint64_t num_docs, int p, int parts, uint64_t before) {
  const int64_t target = plan_target(offs[num_docs], p, parts);
  uint64_t lo = 0, hi = num_docs + 1;  // the first d in [0, num_docs] with offs[d] >= target, num_docs + 1 if none
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (offs[mid] < target) lo = mid + 1;
    else hi = mid;
  }
  uint64_t d = lo > num_docs ? num_docs : lo;
  if (d < before) d = before;
  return d;
}

// ---- DocTopicCatchwordSums.tsv over document shards: the first line of rank q's part of the corpus's L lines, W ranks (q <= W) ---------------
// slice(q) = q floor(L / W) + min(q, L mod W): slice(0) = 0, slice(W) = L, the first L mod W ranks take one line more.  No product wraps:
// q floor(L / W) <= L.
ISLE_STAGE_HD inline uint64_t topic_sums_slice(uint64_t L, uint64_t W, uint64_t q) { return q * (L / W) + std::min(q, L % W); }

// ---- corpus diagnostics and what reads a model ------------------------------------------------------------------------------------------------
// The loop of src/sparseMatrix.cpp:198-208 moves its mark from p to p + max(rem(p), m), rem(p) = distance from p to the end of
// its run, and counts every move that lands before n.  r: the run holding p, rb: the run's first position.  Runs are not empty, m >= 2.
inline uint64_t top_five_count(const uint64_t* run_lengths, uint64_t n_runs, int32_t m) {
  uint64_t n = 0;
  for (uint64_t r = 0; r < n_runs; ++r) n += run_lengths[r];
  uint64_t num = 0, p = 0, r = 0, rb = 0;
  while (n_runs) {
    const uint64_t next = std::max(rb + run_lengths[r], p + (uint64_t)m);
    if (next >= n) break;
    ++num;
    p = next;
    while (rb + run_lengths[r] <= p) rb += run_lengths[r++];
  }
  return num;
}
// src/trainer.cpp:750-774: the finite distances summed in topic order over the kp topics the device found to have one; none: NaN
inline double diversity_average(const double* dist, uint32_t k, uint32_t kp) {
  double s = 0.0;
  for (uint32_t t = 0; t < k; ++t)
    if (std::isfinite(dist[t])) s += dist[t];
  return kp ? s / (double)kp : std::nan("");
}
// the 1-based line of byte `pos` of a text; a position at or past the end belongs to the last byte's line
inline uint64_t line_of_byte(const char* text, uint64_t nbytes, uint64_t pos) {
  const uint64_t upto = std::min<uint64_t>(pos, nbytes ? nbytes - 1 : 0);
  uint64_t line = 1;
  for (uint64_t i = 0; i < upto; ++i) line += text[i] == '\n';
  return line;
}
