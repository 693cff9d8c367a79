// isle_amd/csrc/similar_docs.hip — the documents most similar to a query document (isle_hip_similar_docs): a product of sparse rows with a
// small dense table of queries that writes its result as a CSR by row, which the selection of topic_docs.hip then reads with the query in the
// place of the topic.  The rule (the weight domain, the terms, the scores, what a candidate is) is simdocs_host.h's, and the kernels compile
// its functions; the collectives and the selection between and behind the steps below are api_stages.cpp's.
//   sd_gather_off_k / sd_gather_k   only where the queries are rows of the source: those rows' entries copied into the query CSR
//   sd_table_k    the queries densified into table[topic][query] (num_topics x Qp fp32, Qp = Q rounded up to a power of two), SIMDOCS_ABSENT
//                 (negative: every valid weight is >= 0) where the query does not store the topic, the padded queries included; and nq, the
//                 query's sum of squares in double, ascending
//   sd_walk_k     a wave takes 64 / Qp rows at a time; lane (row in group, query) holds one double accumulator (COSINE: and the row's sum of
//                 squares).  The group reads Qp entries of its row at once, one per lane, and hands them round by shuffles; the trip count
//                 is the wave's longest row, so the walk is wave-uniform and every lane takes part in every shuffle.  It covers ALL entries of
//                 the row: the norm and the checks come with it.
//                 COUNT form (the step "sd_count"): per row the number of candidate lanes (a ballot's popcount); the first entry with a topic >= num_topics, topics
//                 that do not ascend, or a weight outside the domain is named through one 64-bit atomicMin (as td_doc_k names its entry).
//                 SCORE form (the step "sd_score"), behind a 64-bit exclusive scan of the counts: the same walk, every candidate lane writes (query, score) at
//                 off[row] + its rank among the row's candidate lanes; queries ascend within a row because lanes do.
// The walk is done twice.  The alternative, a dense rows x Qp block of scores written once and compacted, costs 4 Qp bytes per row of
// traffic against a second read of the entries; NEITHER IS MEASURED against the other.
// The table's home is LDS (copied once per workgroup) or global memory: route_host.h route_simdocs_table; the same words, the same bits.
// Everything is written with plain stores, there is no floating-point atomic, and nothing resident is written: every buffer is the call's.
#include <algorithm>

#include "common.h"
#include "scan.h"
#include "simdocs_host.h"

namespace {

constexpr int SD_T = 256;
constexpr int SD_WAVES = SD_T / 64;

__global__ __launch_bounds__(64) void sd_gather_off_k(const int64_t* __restrict__ off, const unsigned long long* __restrict__ qrows, uint32_t Q,
                                                      int64_t* __restrict__ q_off) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int64_t at = 0;
  q_off[0] = 0;
  for (uint32_t q = 0; q < Q; ++q) {
    at += off[qrows[q] + 1] - off[qrows[q]];
    q_off[q + 1] = at;
  }
}

__global__ __launch_bounds__(SD_T) void sd_gather_k(const int64_t* __restrict__ off, const uint32_t* __restrict__ topic, const float* __restrict__ weight,
                                                    const unsigned long long* __restrict__ qrows, const int64_t* __restrict__ q_off,
                                                    uint32_t* __restrict__ q_topic, float* __restrict__ q_weight) {
  const uint32_t q = blockIdx.x;
  const int64_t src = off[qrows[q]], dst = q_off[q], len = q_off[q + 1] - dst;
  for (int64_t i = threadIdx.x; i < len; i += SD_T) {
    q_topic[dst + i] = topic[src + i];
    q_weight[dst + i] = weight[src + i];
  }
}

// table: filled with SIMDOCS_ABSENT before; nq: Qp doubles, zeroed before
__global__ __launch_bounds__(SD_T) void sd_table_k(const int64_t* __restrict__ q_off, const uint32_t* __restrict__ q_topic, const float* __restrict__ q_weight,
                                                   uint32_t num_topics, uint32_t Qp, float* __restrict__ table, double* __restrict__ nq) {
  const uint32_t q = blockIdx.x;
  const int64_t b = q_off[q], e = q_off[q + 1];
  for (int64_t f = b + threadIdx.x; f < e; f += SD_T) {
    const uint32_t t = q_topic[f];
    if (t < num_topics) table[(uint64_t)t * Qp + q] = q_weight[f];  // (a gathered row with a bad topic: sd_walk_k names it, nothing is written)
  }
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int64_t f = b; f < e; ++f) s += simdocs_square(q_weight[f]);
    nq[q] = s;
  }
}

// lq = log2(Qp).  SCORE = false: cnt[row] and *err; SCORE = true: qid / score at pair_off[row] + rank.  exclude, nq: Qp elements.
template <int MEASURE, bool SCORE, bool LDS>
__global__ __launch_bounds__(SD_T) void sd_walk_k(const int64_t* __restrict__ off, const uint32_t* __restrict__ topic, const float* __restrict__ weight,
                                                  uint64_t rows, uint32_t num_topics, uint64_t doc_base, const float* __restrict__ table, uint32_t lq,
                                                  const uint32_t* __restrict__ exclude, const double* __restrict__ nq, uint32_t* __restrict__ cnt,
                                                  unsigned long long* __restrict__ err, const int64_t* __restrict__ pair_off, uint32_t* __restrict__ qid,
                                                  float* __restrict__ score) {
  extern __shared__ float sd_tab[];
  const uint32_t Qp = 1u << lq;
  if (LDS) {
    const uint32_t words = num_topics * Qp;  // <= 16384: route_simdocs_table
    for (uint32_t i = threadIdx.x; i < words; i += SD_T) sd_tab[i] = table[i];
    __syncthreads();
  }
  const float* __restrict__ tab = LDS ? sd_tab : table;
  const uint32_t lane = threadIdx.x & 63u, g = lane >> lq, j = lane & (Qp - 1u), G = 64u >> lq;
  const uint32_t first_lane = g << lq;
  const unsigned long long gmask = (Qp == 64u ? ~0ull : ((1ull << Qp) - 1ull)) << first_lane;
  const uint32_t ex = exclude[j];
  const uint64_t nwaves = (uint64_t)gridDim.x * SD_WAVES;
  for (uint64_t row0 = ((uint64_t)blockIdx.x * SD_WAVES + (threadIdx.x >> 6)) * G; row0 < rows; row0 += nwaves * G) {  // wave-uniform
    const uint64_t r = row0 + g;
    const bool live = r < rows;
    const int64_t b = live ? off[r] : 0;
    const unsigned long long len = live ? (unsigned long long)(off[r + 1] - b) : 0ull;
    unsigned long long maxlen = len;
    for (int d = 32; d > 0; d >>= 1) {
      const unsigned long long o = __shfl_xor(maxlen, d);
      maxlen = o > maxlen ? o : maxlen;
    }
    double s = 0.0, nr = 0.0;
    bool hit = false;
    for (unsigned long long c0 = 0; c0 < maxlen; c0 += Qp) {
      const bool have = c0 + j < len;
      const int64_t idx = b + (int64_t)(c0 + j);
      const uint32_t t = have ? topic[idx] : 0xffffffffu;
      const float a = have ? weight[idx] : 0.0f;
      if (!SCORE && have) {
        const bool first = c0 + j == 0;
        unsigned what = topdocs_entry_fault(t, num_topics, first, first ? 0u : topic[idx - 1]);
        if (!what && !simdocs_weight_ok(a)) what = SIMDOCS_BAD_WEIGHT;
        if (what) atomicMin(err, ((unsigned long long)idx << 2) | (unsigned long long)what);
      }
      const uint32_t m = (uint32_t)min((unsigned long long)Qp, maxlen - c0);
      for (uint32_t i = 0; i < m; ++i) {
        const uint32_t ti = __shfl(t, (int)(first_lane + i));
        const float ai = __shfl(a, (int)(first_lane + i));
        if (ti < num_topics) {  // (an entry of the row, with a topic the table has)
          if (SCORE && MEASURE == SIM_COSINE) nr += simdocs_square(ai);
          const float bq = tab[(uint64_t)ti * Qp + j];
          if (bq >= 0.0f) {  // stored in the query (-0.0 included)
            hit = true;
            if (SCORE) s += simdocs_term(MEASURE, ai, bq);
          }
        }
      }
    }
    const bool cand = live && hit && (ex == SIMDOCS_NO_DOC || ex != (uint32_t)(doc_base + r));
    const unsigned long long mine = __ballot(cand) & gmask;
    if (!SCORE) {
      if (live && j == 0) cnt[r] = (uint32_t)__popcll(mine);
    } else if (cand) {
      const int64_t pos = pair_off[r] + (int64_t)__popcll(mine & ((1ull << lane) - 1ull));
      qid[pos] = j;
      score[pos] = simdocs_score(MEASURE, s, nr, nq[j]);
    }
  }
}

template <int MEASURE, bool SCORE>
int sd_launch(isle_ctx* c, const TdView& v, bool lds, uint32_t Qp, const float* table, const uint32_t* exclude, const double* nq, uint32_t* cnt,
              uint64_t* err, const int64_t* pair_off, uint32_t* qid, float* score) {
  uint32_t lq = 0;
  while ((1u << lq) < Qp) ++lq;
  const uint64_t G = 64u >> lq, blocks = (v.rows + G * SD_WAVES - 1) / (G * SD_WAVES);
  if (lds) {
    const size_t bytes = (size_t)v.num_topics * Qp * sizeof(float);
    ISLECHK(isle_max_lds(c, (const void*)sd_walk_k<MEASURE, SCORE, true>, (int)SIMDOCS_LDS_TABLE_BYTES));
    hipLaunchKernelGGL((sd_walk_k<MEASURE, SCORE, true>), dim3((unsigned)std::min<uint64_t>(blocks, (uint64_t)c->num_cus * 2)), dim3(SD_T), bytes, c->stream, v.off,
                       v.topic, v.value, v.rows, v.num_topics, v.doc_base, table, lq, exclude, nq, cnt, (unsigned long long*)err, pair_off, qid, score);
  } else {
    hipLaunchKernelGGL((sd_walk_k<MEASURE, SCORE, false>), dim3((unsigned)std::min<uint64_t>(blocks, (uint64_t)c->num_cus * 8)), dim3(SD_T), 0, c->stream, v.off,
                       v.topic, v.value, v.rows, v.num_topics, v.doc_base, table, lq, exclude, nq, cnt, (unsigned long long*)err, pair_off, qid, score);
  }
  HIPCHK(c, hipGetLastError());
  return 0;
}

}  // namespace

// the queries are rows of the source: q_off (device and host, Q + 1) from those rows' lengths
int k_sd_gather_offsets(isle_ctx* c, const TdView& v, const uint64_t* qrows_dev, uint32_t Q, int64_t* q_off_dev, int64_t* q_off_host) {
  TimeScope ts(c, v.fam);
  hipLaunchKernelGGL(sd_gather_off_k, dim3(1), dim3(64), 0, c->stream, v.off, (const unsigned long long*)qrows_dev, Q, q_off_dev);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(q_off_host, q_off_dev, ((size_t)Q + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

// ... and their entries into the query CSR
int k_sd_gather(isle_ctx* c, const TdView& v, const uint64_t* qrows_dev, uint32_t Q, const int64_t* q_off_dev, uint32_t* q_topic, float* q_weight) {
  TimeScope ts(c, v.fam);
  hipLaunchKernelGGL(sd_gather_k, dim3(Q), dim3(SD_T), 0, c->stream, v.off, v.topic, v.value, (const unsigned long long*)qrows_dev, q_off_dev, q_topic, q_weight);
  HIPCHK(c, hipGetLastError());
  return 0;
}

// table (num_topics x Qp) and nq (Qp) from the query CSR on the device
int k_sd_table(isle_ctx* c, int fam, uint32_t Q, uint32_t num_topics, const int64_t* q_off, const uint32_t* q_topic, const float* q_weight, float* table,
               double* nq) {
  TimeScope ts(c, fam);
  const uint32_t Qp = simdocs_qp(Q);
  uint32_t absent;
  const float mark = SIMDOCS_ABSENT;
  memcpy(&absent, &mark, sizeof(absent));
  HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)table, (int)absent, (size_t)num_topics * Qp, c->stream));
  HIPCHK(c, hipMemsetAsync(nq, 0, (size_t)Qp * sizeof(double), c->stream));
  hipLaunchKernelGGL(sd_table_k, dim3(Q), dim3(SD_T), 0, c->stream, q_off, q_topic, q_weight, num_topics, Qp, table, nq);
  HIPCHK(c, hipGetLastError());
  return 0;
}

// v: the source's rows (num_topics: the table's).  cnt (rows), pair_off (rows + 1; blk: its scan's scratch), *bad: ~0 = none, else
// (entry << 2) | what; *pairs: the candidate pairs of this rank
int k_sd_count(isle_ctx* c, const TdView& v, bool lds, uint32_t Q, const float* table, const uint32_t* exclude, uint32_t* cnt, int64_t* pair_off, int64_t* blk,
               uint64_t* err_dev, uint64_t* bad, uint64_t* pairs) {
  TimeScope ts(c, v.fam);
  *bad = ~0ull;
  *pairs = 0;
  HIPCHK(c, hipMemsetAsync(err_dev, 0xff, sizeof(uint64_t), c->stream));
  if (!v.rows) {
    HIPCHK(c, hipMemsetAsync(pair_off, 0, sizeof(int64_t), c->stream));
    return 0;
  }
  ISLECHK((sd_launch<SIM_DOT, false>(c, v, lds, simdocs_qp(Q), table, exclude, nullptr, cnt, err_dev, nullptr, nullptr, nullptr)));
  HIPCHK(c, (isle_scan::exclusive_scan<uint32_t, int64_t>(c->stream, cnt, v.rows, pair_off, blk)));
  int64_t total = 0;
  HIPCHK(c, hipMemcpyAsync(bad, err_dev, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(&total, pair_off + v.rows, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *pairs = (uint64_t)total;
  return 0;
}

// the pairs' (query, score) at pair_off
int k_sd_score(isle_ctx* c, const TdView& v, int measure, bool lds, uint32_t Q, const float* table, const uint32_t* exclude, const double* nq,
               const int64_t* pair_off, uint32_t* qid, float* score) {
  TimeScope ts(c, v.fam);
  if (!v.rows) return 0;
  const uint32_t Qp = simdocs_qp(Q);
  if (measure == SIM_DOT) return sd_launch<SIM_DOT, true>(c, v, lds, Qp, table, exclude, nq, nullptr, nullptr, pair_off, qid, score);
  if (measure == SIM_COSINE) return sd_launch<SIM_COSINE, true>(c, v, lds, Qp, table, exclude, nq, nullptr, nullptr, pair_off, qid, score);
  return sd_launch<SIM_BHATTACHARYYA, true>(c, v, lds, Qp, table, exclude, nq, nullptr, nullptr, pair_off, qid, score);
}
