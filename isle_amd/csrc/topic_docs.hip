// isle_amd/csrc/topic_docs.hip — the n heaviest documents of every topic (isle_hip_topic_top_docs), selected where the entries lie: the
// inference entries inf_* and the document-topic catchword sums p_dts_* are stored by document, and nothing gathers them per topic.  The rule
// (the order on value bits, the key that carries the document, the tie rule, the result) is topdocs_host.h's; the kernels below are the device
// steps, the collectives between them are api_stages.cpp's.
//   td_doc_k      tiles of MT_TILE entries: the row of every entry from the offsets window of doc_text.h (shared with the text formatters),
//                 doc[e] = doc_base + row as u32, cnt_t counted, and the form of the rows checked in the same pass (topic < num_topics, topics
//                 ascending strictly within a row); the first bad entry is named through one 64-bit atomicMin.  The later passes read (topic,
//                 value, doc), 12 bytes per entry, coalesced.  This costs 4 bytes per entry; recomputing the row in every pass instead is the
//                 alternative, and NEITHER IS MEASURED.
//   td_hist_k     one of eight rounds, most significant byte first: the entries whose key carries its topic's prefix so far, counted by the byte
//                 at `shift` into bins[topic][256] (u32, integer atomics: the result does not depend on order).  The bins live in LDS, private
//                 per workgroup and flushed once, while topdocs_bins_in_lds(num_topics) (<= 64 topics), else in global memory; both forms give
//                 the same integers.
//   td_step_k     select_digit(bins_t, remaining_t) (stage_host.h) extends the prefix; remaining_t starts at min(n, cnt_t).  After the eighth
//                 round the prefix is the smallest selected key of the topic.  Topics without entries are skipped.
//   td_collect_k  the entries with key >= that key take a slot by atomicAdd on fill[t] in a zeroed num_topics x n table of keys: exactly
//                 min(n, cnt_t) per topic over all ranks.
//   td_sort_k     one workgroup per topic: up to world x n keys into LDS (zero = an unused slot; they sink to the end), a bitonic sort in
//                 descending order, and for the first min(n, cnt_t) keys docs[t n + i] and values[t n + i]; unused slots 0xffffffff / 0.0f.
// Everything is written with plain stores.  Nothing resident is written: every buffer is the call's.
#include <algorithm>

#include "common.h"
#include "doc_text.h"
#include "topdocs_host.h"

namespace {

constexpr int TD_LCNT = 1024;  // td_doc_k counts the topics in LDS up to this many (4 KiB); a choice, not a measurement

__global__ __launch_bounds__(MT) void td_doc_k(const int64_t* __restrict__ off, const uint32_t* __restrict__ topic, uint64_t rows, uint64_t nnz, uint64_t ntiles,
                                               uint32_t num_topics, uint64_t doc_base, uint32_t* __restrict__ doc, unsigned long long* __restrict__ cnt,
                                               unsigned long long* __restrict__ err) {
  __shared__ uint32_t win[IT_WIN];
  __shared__ uint64_t row0;
  __shared__ uint32_t lcnt[TD_LCNT];
  const bool local = num_topics <= (uint32_t)TD_LCNT;
  if (local)
    for (uint32_t i = threadIdx.x; i < num_topics; i += MT) lcnt[i] = 0;  // (it_stage_window's first barrier precedes the first add)
  for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint64_t e0 = tile * MT_TILE;
    const uint32_t nl = (uint32_t)min((uint64_t)MT_TILE, nnz - e0);
    it_stage_window(off, 0, rows, e0, win, &row0);
    for (uint32_t l = threadIdx.x; l < nl; l += MT) {
      const uint64_t e = e0 + l;
      const uint64_t row = it_window_row(off, rows, e, l, nl, win, row0);
      const uint32_t t = topic[e];
      doc[e] = (uint32_t)(doc_base + row);
      const bool first = e == (uint64_t)off[row];
      const unsigned what = topdocs_entry_fault(t, num_topics, first, first ? 0u : topic[e - 1]);
      if (what) atomicMin(err, ((unsigned long long)e << 2) | (unsigned long long)what);
      if (t < num_topics) {
        if (local) atomicAdd(&lcnt[t], 1u);
        else atomicAdd(&cnt[t], 1ull);
      }
    }
  }
  __syncthreads();
  if (local)
    for (uint32_t i = threadIdx.x; i < num_topics; i += MT)
      if (lcnt[i]) atomicAdd(&cnt[i], (unsigned long long)lcnt[i]);
}

__global__ __launch_bounds__(MT) void td_init_k(const unsigned long long* __restrict__ cnt, uint32_t num_topics, uint32_t n, unsigned long long* __restrict__ prefix,
                                                uint32_t* __restrict__ rem) {
  const uint32_t t = blockIdx.x * MT + threadIdx.x;
  if (t >= num_topics) return;
  prefix[t] = 0;
  rem[t] = (uint32_t)min((unsigned long long)n, cnt[t]);
}

template <bool LDS>
__global__ __launch_bounds__(MT) void td_hist_k(const uint32_t* __restrict__ topic, const float* __restrict__ value, const uint32_t* __restrict__ doc, uint64_t nnz,
                                                uint32_t num_topics, const unsigned long long* __restrict__ prefix, int shift, uint32_t* __restrict__ bins) {
  extern __shared__ uint32_t td_lbins[];
  const uint32_t nb = num_topics * 256u;
  if (LDS) {
    for (uint32_t i = threadIdx.x; i < nb; i += MT) td_lbins[i] = 0;
    __syncthreads();
  }
  for (uint64_t e = (uint64_t)blockIdx.x * MT + threadIdx.x; e < nnz; e += (uint64_t)gridDim.x * MT) {
    const uint32_t t = topic[e];  // < num_topics: td_doc_k has checked
    const uint64_t key = topdocs_key(__float_as_uint(value[e]), doc[e]);
    if (topdocs_under_prefix(key, prefix[t], shift)) {
      const uint64_t b = (uint64_t)t * 256u + topdocs_key_byte(key, shift);
      if (LDS) atomicAdd(&td_lbins[b], 1u);
      else atomicAdd(&bins[b], 1u);
    }
  }
  if (LDS) {
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < nb; i += MT)
      if (td_lbins[i]) atomicAdd(&bins[i], td_lbins[i]);
  }
}

__global__ __launch_bounds__(MT) void td_step_k(const uint32_t* __restrict__ bins, const unsigned long long* __restrict__ cnt, uint32_t num_topics, int shift,
                                                unsigned long long* __restrict__ prefix, uint32_t* __restrict__ rem) {
  const uint32_t t = blockIdx.x * MT + threadIdx.x;
  if (t >= num_topics || cnt[t] == 0) return;
  const SelectPick p = select_digit(bins + (uint64_t)t * 256, rem[t]);
  prefix[t] |= (unsigned long long)p.digit << shift;
  rem[t] = p.remaining;
}

__global__ __launch_bounds__(MT) void td_collect_k(const uint32_t* __restrict__ topic, const float* __restrict__ value, const uint32_t* __restrict__ doc, uint64_t nnz,
                                                   uint32_t n, const unsigned long long* __restrict__ tau, uint32_t* __restrict__ fill,
                                                   unsigned long long* __restrict__ table) {
  for (uint64_t e = (uint64_t)blockIdx.x * MT + threadIdx.x; e < nnz; e += (uint64_t)gridDim.x * MT) {
    const uint32_t t = topic[e];
    const uint64_t key = topdocs_key(__float_as_uint(value[e]), doc[e]);
    if (key >= tau[t]) {
      const uint32_t slot = atomicAdd(&fill[t], 1u);
      if (slot < n) table[(uint64_t)t * n + slot] = key;  // (never beyond: exactly min(n, cnt_t) keys reach the smallest selected one)
    }
  }
}

// tables: world blocks of num_topics x n keys; P: the power of two >= world n, the keys sorted in LDS
__global__ __launch_bounds__(MT) void td_sort_k(const unsigned long long* __restrict__ tables, uint32_t world, uint32_t num_topics, uint32_t n, uint32_t P,
                                                const unsigned long long* __restrict__ cnt, uint32_t* __restrict__ docs, float* __restrict__ values,
                                                uint32_t* __restrict__ counts) {
  extern __shared__ unsigned long long td_keys[];
  const uint32_t t = blockIdx.x, total = world * n;
  for (uint32_t i = threadIdx.x; i < P; i += MT) {
    unsigned long long k = 0;
    if (i < total) {
      const uint32_t q = i / n, j = i - q * n;
      k = tables[((uint64_t)q * num_topics + t) * n + j];
    }
    td_keys[i] = k;
  }
  __syncthreads();
  for (uint32_t k = 2; k <= P; k <<= 1)
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t i = threadIdx.x; i < P; i += MT) {
        const uint32_t x = i ^ j;
        if (x > i) {
          const unsigned long long a = td_keys[i], b = td_keys[x];
          if ((i & k) == 0 ? a < b : a > b) {
            td_keys[i] = b;
            td_keys[x] = a;
          }
        }
      }
      __syncthreads();
    }
  const uint32_t m = (uint32_t)min((unsigned long long)n, cnt[t]);
  for (uint32_t i = threadIdx.x; i < n; i += MT) {
    const unsigned long long k = i < m ? td_keys[i] : 0ull;
    docs[(uint64_t)t * n + i] = k ? topdocs_key_doc(k) : 0xffffffffu;
    values[(uint64_t)t * n + i] = k ? __uint_as_float(topdocs_key_bits(k)) : 0.0f;
  }
  if (threadIdx.x == 0) counts[t] = m;
}

}  // namespace

#define LAUNCH_CHECK(c) HIPCHK(c, hipGetLastError())

// doc[e], cnt_t (zeroed here, this rank's entries) and the first bad entry (*bad: ~0 = none, else (entry << 2) | what); nnz >= 1
int k_td_docs(isle_ctx* c, const TdView& v, uint32_t* doc, uint64_t* cnt, uint64_t* err_dev, uint64_t* bad) {
  TimeScope ts(c, v.fam);
  HIPCHK(c, hipMemsetAsync(cnt, 0, (size_t)v.num_topics * sizeof(uint64_t), c->stream));
  HIPCHK(c, hipMemsetAsync(err_dev, 0xff, sizeof(uint64_t), c->stream));
  *bad = ~0ull;
  if (v.nnz) {
    const uint64_t ntiles = (v.nnz + MT_TILE - 1) / MT_TILE;
    hipLaunchKernelGGL(td_doc_k, dim3((unsigned)std::min<uint64_t>(ntiles, (uint64_t)c->num_cus * 8)), dim3(MT), 0, c->stream, v.off, v.topic, v.rows, v.nnz,
                       ntiles, v.num_topics, v.doc_base, doc, (unsigned long long*)cnt, (unsigned long long*)err_dev);
    LAUNCH_CHECK(c);
    HIPCHK(c, hipMemcpyAsync(bad, err_dev, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return 0;
}

// cnt: the corpus's counts -> prefix = 0, remaining = min(n, cnt_t)
int k_td_init(isle_ctx* c, const TdView& v, const uint64_t* cnt, uint64_t* prefix, uint32_t* rem) {
  TimeScope ts(c, v.fam);
  hipLaunchKernelGGL(td_init_k, dim3(cdiv(v.num_topics, MT)), dim3(MT), 0, c->stream, (const unsigned long long*)cnt, v.num_topics, v.n,
                     (unsigned long long*)prefix, rem);
  LAUNCH_CHECK(c);
  return 0;
}

// this rank's bins of the round at `shift` (zeroed here)
int k_td_hist(isle_ctx* c, const TdView& v, const uint32_t* doc, const uint64_t* prefix, int shift, uint32_t* bins) {
  TimeScope ts(c, v.fam);
  const size_t bytes = (size_t)v.num_topics * 256 * sizeof(uint32_t);
  HIPCHK(c, hipMemsetAsync(bins, 0, bytes, c->stream));
  if (!v.nnz) return 0;
  if (topdocs_bins_in_lds(v.num_topics)) {
    ISLECHK(isle_max_lds(c, (const void*)td_hist_k<true>, (int)TOPDOCS_LDS_BINS_BYTES));
    const unsigned g = (unsigned)std::min<uint64_t>((v.nnz + 4 * MT_TILE - 1) / (4 * MT_TILE), (uint64_t)c->num_cus * 2);
    hipLaunchKernelGGL(td_hist_k<true>, dim3(g), dim3(MT), bytes, c->stream, v.topic, v.value, doc, v.nnz, v.num_topics, (const unsigned long long*)prefix, shift,
                       bins);
  } else {
    const unsigned g = (unsigned)std::min<uint64_t>((v.nnz + MT - 1) / MT, (uint64_t)c->num_cus * 16);
    hipLaunchKernelGGL(td_hist_k<false>, dim3(g), dim3(MT), 0, c->stream, v.topic, v.value, doc, v.nnz, v.num_topics, (const unsigned long long*)prefix, shift, bins);
  }
  LAUNCH_CHECK(c);
  return 0;
}

// bins: the corpus's -> the prefix extended by the byte at `shift`
int k_td_step(isle_ctx* c, const TdView& v, const uint32_t* bins, const uint64_t* cnt, int shift, uint64_t* prefix, uint32_t* rem) {
  TimeScope ts(c, v.fam);
  hipLaunchKernelGGL(td_step_k, dim3(cdiv(v.num_topics, MT)), dim3(MT), 0, c->stream, bins, (const unsigned long long*)cnt, v.num_topics, shift,
                     (unsigned long long*)prefix, rem);
  LAUNCH_CHECK(c);
  return 0;
}

// this rank's winners into its num_topics x n table (zeroed here; fill: num_topics words of the call)
int k_td_collect(isle_ctx* c, const TdView& v, const uint32_t* doc, const uint64_t* tau, uint32_t* fill, uint64_t* table) {
  TimeScope ts(c, v.fam);
  HIPCHK(c, hipMemsetAsync(fill, 0, (size_t)v.num_topics * sizeof(uint32_t), c->stream));
  HIPCHK(c, hipMemsetAsync(table, 0, (size_t)v.num_topics * v.n * sizeof(uint64_t), c->stream));
  if (!v.nnz) return 0;
  const unsigned g = (unsigned)std::min<uint64_t>((v.nnz + MT - 1) / MT, (uint64_t)c->num_cus * 16);
  hipLaunchKernelGGL(td_collect_k, dim3(g), dim3(MT), 0, c->stream, v.topic, v.value, doc, v.nnz, v.n, (const unsigned long long*)tau, fill,
                     (unsigned long long*)table);
  LAUNCH_CHECK(c);
  return 0;
}

// tables: `world` tables side by side -> the lists (device arrays of num_topics x n, num_topics)
int k_td_sort(isle_ctx* c, const TdView& v, const uint64_t* tables, uint32_t world, const uint64_t* cnt, uint32_t* docs, float* values, uint32_t* counts) {
  TimeScope ts(c, v.fam);
  uint32_t P = 1;
  while (P < world * v.n) P <<= 1;  // <= TOPDOCS_SORT_KEYS: topdocs_check_args
  ISLECHK(isle_max_lds(c, (const void*)td_sort_k, (int)(TOPDOCS_SORT_KEYS * sizeof(uint64_t))));
  hipLaunchKernelGGL(td_sort_k, dim3(v.num_topics), dim3(MT), (size_t)P * sizeof(uint64_t), c->stream, (const unsigned long long*)tables, world, v.num_topics, v.n, P,
                     (const unsigned long long*)cnt, docs, values, counts);
  LAUNCH_CHECK(c);
  return 0;
}
