// isle_amd/csrc/edge_select.hip — the pair selection of ISLETrainer::construct_edge_topics_v2 (src/trainer.cpp:1120-1145) on the
// documents' device-resident (top topic, second topic).  The rule is the one hot_path.select_edge_pairs and
// fpsparse_detail::select_edge_pairs_host state: documents with top1 >= 0 and top2 >= 0 are counted per ordered pair, pairs with
// count >= min_docs are candidates, candidates are ordered by count descending and (primary, secondary) ascending among equal counts,
// the first max_edge_topics are kept; the threshold is the count of the first candidate cut off.
//
//   ep_count_k      grid-stride over documents, one integer atomicAdd on table[top1 * k + top2]: integer sums do not depend on the
//                   order of arrival.  An id >= k or < -1 is never used as an index: the first such document is reported through
//                   one 64-bit atomicMin (as feed_key_k reports its first bad entry)
//   (all-reduce)    several ranks: every rank counted its own documents; the table is summed, everything below runs replicated
//   ep_flag_k       flag[bin] = count >= min_docs, the largest count and the smallest candidate count
//   (isle_scan)     exclusive scan of the flags: the candidates' positions in ascending bin order
//   ep_compact_k    candidates -> (key = max_count - count, value = bin) in ascending bin order
//   (k_sort_pairs_u64, ingest.hip)  stable LSD radix sort on the bit length of the largest key: count descending, and the stability on
//                   the bin-ascending input is the tie rule
//   ep_out_k        the first min(max_edge_topics, candidates) entries as (primary, secondary, count) int64 triples, and the threshold
//
// The table form: k * k counters, used for k <= ISLE_EDGE_TABLE_MAX_TOPICS = 8192 (256 MB of counters); beyond that the entry refuses and the
// C++ mirror keeps its host loop.  Counting by sorting the documents' keys top1 * k + top2 and taking run lengths would lift the limit;
// whether it would also be faster at k = 1000 with hot bins (many documents adding to one counter) is unmeasured.
#include <algorithm>

#include "common.h"
#include "scan.h"

namespace {

constexpr int ET = 256;
constexpr unsigned long long EP_NONE = ~0ull;

__global__ __launch_bounds__(ET) void ep_count_k(const int32_t* __restrict__ top1, const int32_t* __restrict__ top2, uint64_t D, int32_t k,
                                                  uint32_t* __restrict__ table, unsigned long long* __restrict__ err) {
  for (uint64_t d = (uint64_t)blockIdx.x * ET + threadIdx.x; d < D; d += (uint64_t)gridDim.x * ET) {
    const int32_t p = top1[d], s = top2[d];
    if (p >= k || p < -1 || s >= k || s < -1) {
      atomicMin(err, (unsigned long long)d);
      continue;
    }
    if (p >= 0 && s >= 0) atomicAdd(&table[(size_t)p * (size_t)k + (size_t)s], 1u);
  }
}

// mm[0] = the largest count, mm[1] = the smallest count among the candidates (0xffffffff: none)
__global__ __launch_bounds__(ET) void ep_flag_k(const uint32_t* __restrict__ table, uint64_t nb, uint32_t min_docs, uint32_t* __restrict__ flag,
                                                 uint32_t* __restrict__ mm) {
  __shared__ uint32_t smax[ET], smin[ET];
  const uint64_t i = (uint64_t)blockIdx.x * ET + threadIdx.x;
  const uint32_t x = i < nb ? table[i] : 0u;
  const bool cand = i < nb && x >= min_docs;
  if (i < nb) flag[i] = cand ? 1u : 0u;
  smax[threadIdx.x] = x;
  smin[threadIdx.x] = cand ? x : 0xffffffffu;
  __syncthreads();
  for (int o = ET / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      smax[threadIdx.x] = max(smax[threadIdx.x], smax[threadIdx.x + o]);
      smin[threadIdx.x] = min(smin[threadIdx.x], smin[threadIdx.x + o]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (smax[0]) atomicMax(&mm[0], smax[0]);
    if (smin[0] != 0xffffffffu) atomicMin(&mm[1], smin[0]);
  }
}

__global__ __launch_bounds__(ET) void ep_compact_k(const uint32_t* __restrict__ table, const uint32_t* __restrict__ flag, const int64_t* __restrict__ at,
                                                    uint64_t nb, const uint32_t* __restrict__ mm, uint64_t* __restrict__ key, uint32_t* __restrict__ bin) {
  const uint64_t i = (uint64_t)blockIdx.x * ET + threadIdx.x;
  if (i >= nb || !flag[i]) return;
  const int64_t q = at[i];  // < the number of candidates = the size of key / bin
  key[q] = (uint64_t)(mm[0] - table[i]);
  bin[q] = (uint32_t)i;
}

// out: nsel triples, then one word: the count of candidate nsel (the first one cut off) when ncand > nsel
__global__ __launch_bounds__(ET) void ep_out_k(const uint64_t* __restrict__ key, const uint32_t* __restrict__ bin, uint64_t nsel, uint64_t ncand, uint32_t k,
                                                const uint32_t* __restrict__ mm, int64_t* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * ET + threadIdx.x;
  if (i > nsel || i >= ncand) return;
  const int64_t cnt = (int64_t)((uint64_t)mm[0] - key[i]);
  if (i == nsel) {
    out[3 * nsel] = cnt;
    return;
  }
  const uint32_t b = bin[i];
  out[3 * i] = (int64_t)(b / k);
  out[3 * i + 1] = (int64_t)(b % k);
  out[3 * i + 2] = cnt;
}

}  // namespace

#define LAUNCH_CHECK(c) HIPCHK(c, hipGetLastError())

int k_edge_select(isle_ctx* c, const int32_t* top1_dev, const int32_t* top2_dev, uint64_t D, uint32_t k, uint64_t max_edge_topics, uint64_t min_docs,
                  int64_t* pairs_host, uint64_t cap, uint64_t* n_selected, uint64_t* n_candidates, uint64_t* threshold, uint64_t* bad_doc) {
  *n_selected = *n_candidates = *threshold = 0;
  *bad_doc = EP_NONE;
  const uint64_t nb = (uint64_t)k * k;  // <= 2^26
  // every buffer is local: freed on return, behind the synchronisations below
  DevBuf<uint32_t> table, flag, bin_a, bin_b;
  DevBuf<uint64_t> key_a, key_b, small;  // small: [first bad document | (largest count, smallest candidate count) as two u32]
  DevBuf<int64_t> at, scratch, out;
  HIPCHK(c, table.reserve(nb));
  HIPCHK(c, flag.reserve(nb));
  HIPCHK(c, at.reserve(nb + 1));
  HIPCHK(c, scratch.reserve(isle_scan_scratch(nb) + 8));
  HIPCHK(c, small.reserve(2));
  uint32_t* mm = (uint32_t*)(small.p + 1);
  // a count is at most D < 2^32 (the entry checks it); min_docs = 0 selects what 1 selects: a pair no document has is no candidate
  const uint32_t md = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(min_docs, 1), 0xffffffffull);
  uint64_t ncand = 0;
  uint32_t h_mm[2] = {0u, 0xffffffffu};
  {
    TimeScope ts(c, ISLE_T_POST);
    const uint64_t init[2] = {EP_NONE, (uint64_t)0xffffffffu << 32};  // mm[0] = 0, mm[1] = 0xffffffff (little endian, as the device reads them)
    HIPCHK(c, hipMemcpyAsync(small.p, init, sizeof(init), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(table.p, 0, nb * sizeof(uint32_t), c->stream));
    if (D) {
      const unsigned g = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((D + ET - 1) / ET, (uint64_t)c->num_cus * 8));
      hipLaunchKernelGGL(ep_count_k, dim3(g), dim3(ET), 0, c->stream, top1_dev, top2_dev, D, (int32_t)k, table.p, (unsigned long long*)small.p);
      LAUNCH_CHECK(c);
    }
  }
  if (c->multi()) {  // the documents are this rank's: the counters summed over the ranks, the rest of the selection replicated on every rank
    TimeScope ts(c, ISLE_T_COMM);
    ISLECHK(isle_allreduce(c, table.p, nb, ISLE_DT_U32));
  }
  {
    TimeScope ts(c, ISLE_T_POST);
    hipLaunchKernelGGL(ep_flag_k, dim3(cdiv((long)nb, ET)), dim3(ET), 0, c->stream, table.p, nb, md, flag.p, mm);
    LAUNCH_CHECK(c);
    HIPCHK(c, (isle_scan::exclusive_scan<uint32_t, int64_t>(c->stream, flag.p, nb, at.p, scratch.p)));
  }
  {
    uint64_t h_small[2];
    int64_t h_n = 0;
    HIPCHK(c, hipMemcpyAsync(h_small, small.p, sizeof(h_small), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&h_n, at.p + nb, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (h_small[0] != EP_NONE) {
      *bad_doc = h_small[0];
      return 0;
    }
    ncand = (uint64_t)h_n;
    h_mm[0] = (uint32_t)(h_small[1] & 0xffffffffu);
    h_mm[1] = (uint32_t)(h_small[1] >> 32);
  }
  const uint64_t nsel = std::min<uint64_t>(max_edge_topics, ncand);
  *n_candidates = ncand;
  *n_selected = nsel;
  if (ncand == 0 || nsel > cap) return 0;  // (the entry turns nsel > cap into its error)
  int key_bits = 0;
  for (uint32_t span = h_mm[0] - h_mm[1]; span; span >>= 1) ++key_bits;  // the largest key = largest count - smallest candidate count
  HIPCHK(c, key_a.reserve(ncand));
  HIPCHK(c, key_b.reserve(ncand));
  HIPCHK(c, bin_a.reserve(ncand));
  HIPCHK(c, bin_b.reserve(ncand));
  HIPCHK(c, out.reserve(3 * nsel + 1));
  {
    TimeScope ts(c, ISLE_T_POST);
    hipLaunchKernelGGL(ep_compact_k, dim3(cdiv((long)nb, ET)), dim3(ET), 0, c->stream, table.p, flag.p, at.p, nb, mm, key_a.p, bin_a.p);
    LAUNCH_CHECK(c);
    bool in_a = true;
    ISLECHK(k_sort_pairs_u64(c, key_a.p, bin_a.p, key_b.p, bin_b.p, ncand, key_bits, &in_a));
    hipLaunchKernelGGL(ep_out_k, dim3(cdiv((long)(nsel + 1), ET)), dim3(ET), 0, c->stream, in_a ? key_a.p : key_b.p, in_a ? bin_a.p : bin_b.p, nsel, ncand, k, mm,
                       out.p);
    LAUNCH_CHECK(c);
  }
  int64_t thr = 0;
  if (nsel) HIPCHK(c, hipMemcpyAsync(pairs_host, out.p, 3 * nsel * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  if (ncand > nsel) HIPCHK(c, hipMemcpyAsync(&thr, out.p + 3 * nsel, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *threshold = (uint64_t)thr;
  return 0;
}
