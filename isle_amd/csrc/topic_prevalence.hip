// isle_amd/csrc/topic_prevalence.hip — topic prevalence by document group (isle_hip_topic_prevalence): a keyed (group x topic) reduction of
// sparse rows with a stated order of summation, so that the sums are the same bits on every call and on the host.  The rule (the weight
// domain, the terms, the dominant topic, the radix-64 tree, the tile) is prevalence_host.h's, and the kernels compile its functions; the
// refusals and the order of the steps are api_stages.cpp's.
//   tp_rows_k    one thread per row: the label and every entry checked (the first bad row and the first bad entry each named through one
//                64-bit atomicMin), the row sum rs_r in stored order (normalise), the dominant topic, and docs / count / dominant bumped with
//                integer atomics, which no order can change: in LDS, private per workgroup and flushed once, while the tables fit
//                (prev_hist_in_lds), else in global memory.  With labels it also writes the sort's (label, row) pairs.
//   (the list)   with labels: the stable radix sort k_sort_pairs_u64 on the label alone, rows ascending within a label because the sort is
//                stable; rows of no group sort behind every group.  Without labels the list is the identity and nothing is sorted.
//   tp_next_k    the counts of the next level, ceil(n / 64) per group; the 64-bit exclusive_scan of scan.h makes each level's bases (level 0:
//                the scan of docs, the list's group bases; level 1: the block bases)
//   tp_level0_k  a wave owns a block of 64 consecutive list positions and a private table of one topic tile of doubles in LDS.  It fetches
//                its 64 row numbers, their offsets and row sums with coalesced loads up front and hands them round by shuffles, then walks
//                the rows in list order, its lanes taking the entries of a row: topics are distinct within a row, so a plain
//                read-modify-write is enough.  The block's group comes from an upper-bound search in the block bases.  The partial is
//                written dense, block x tile.
//   tp_fold_k    levels >= 1: one thread per (parent, topic), sequential over at most 64 children, coalesced along the topic.
// The last level writes `sum`.  Topics beyond one tile are taken tile after tile, the partials reused.  There is no floating-point atomic
// anywhere, and nothing resident is written: every buffer is the call's.
// NOT MEASURED: a part of a wave as a block's owner (rows of few entries leave most lanes of the wave idle), tiles other than 1024.
// Compiler's report for gfx950 (hipcc -O3 -Rpass-analysis=kernel-resource-usage); no kernel of this file uses scratch or spills:
//   tp_rows_k<false>     VGPRs 25, SGPRs 67, scratch 0 bytes, LDS 0, occupancy 8 waves/SIMD
//   tp_rows_k<true>      VGPRs 25, SGPRs 76, scratch 0 bytes, LDS dynamic: 4 (G (2 k + 1) + 1) bytes <= 32 KiB + 4, occupancy 8 waves/SIMD
//   tp_level0_k<false>   VGPRs 36, SGPRs 56, scratch 0 bytes, LDS dynamic: 4 waves x 8 tile bytes <= 32 KiB, occupancy 8 waves/SIMD
//   tp_level0_k<true>    VGPRs 48, SGPRs 64, scratch 0 bytes, LDS as above, occupancy 8 waves/SIMD
//   tp_fold_k            VGPRs 22, SGPRs 43, scratch 0 bytes, LDS 0, occupancy 8 waves/SIMD
//   tp_next_k            VGPRs 6, SGPRs 12, scratch 0 bytes, LDS 0, occupancy 8 waves/SIMD
#include <algorithm>

#include "common.h"
#include "prevalence_host.h"
#include "scan.h"

namespace {

constexpr int TP_T = 256;
constexpr int TP_WAVES = TP_T / 64;

// the last index i of base[0 .. n] (ascending, base[0] = 0 <= x < base[n]) with base[i] <= x: empty groups share their base with the next
__device__ inline uint32_t tp_group_of(const unsigned long long* __restrict__ base, uint32_t n, unsigned long long x) {
  uint32_t lo = 0, hi = n;  // base[lo] <= x < base[hi]
  while (hi - lo > 1) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (base[mid] <= x) lo = mid;
    else hi = mid;
  }
  return lo;
}

template <bool LDS>
__device__ inline void tp_bump(uint32_t* hist, unsigned long long* table, uint64_t at, uint64_t lds_at) {
  if (LDS) atomicAdd(hist + lds_at, 1u);
  else atomicAdd(table + at, 1ull);
}

// docs: G + 1 counters, the last one the rows of no group.  err[0]: the first row with a bad label; err[1]: the first bad entry.
// rs (rows, nullable), label / rowid (rows, nullable: the sort's pairs).  LDS: G + 1 | G k | G k words.
template <bool LDS>
__global__ __launch_bounds__(TP_T) void tp_rows_k(const int64_t* __restrict__ off, const uint32_t* __restrict__ topic, const float* __restrict__ weight,
                                                  uint64_t rows, uint32_t k, const uint32_t* __restrict__ groups, uint32_t G,
                                                  unsigned long long* __restrict__ docs, unsigned long long* __restrict__ count,
                                                  unsigned long long* __restrict__ dominant, double* __restrict__ rs, unsigned long long* __restrict__ label,
                                                  uint32_t* __restrict__ rowid, unsigned long long* __restrict__ err) {
  extern __shared__ uint32_t tp_hist[];
  const uint32_t cells = G * k, words = 2u * cells + G + 1u;  // (LDS: <= 8193 words)
  if (LDS) {
    for (uint32_t i = threadIdx.x; i < words; i += TP_T) tp_hist[i] = 0u;
    __syncthreads();
  }
  const uint32_t c0 = G + 1u, d0 = G + 1u + cells;
  for (uint64_t r = (uint64_t)blockIdx.x * TP_T + threadIdx.x; r < rows; r += (uint64_t)gridDim.x * TP_T) {
    const uint32_t lab = groups ? groups[r] : 0u;
    const bool none = lab == PREV_GROUP_NONE, bad = !none && lab >= G, in = !none && !bad;
    if (bad) atomicMin(err, (unsigned long long)r);
    if (label) {
      label[r] = in ? lab : G;
      rowid[r] = (uint32_t)r;
    }
    const int64_t b = off[r], e = off[r + 1];
    double s = 0.0;
    float best = 0.0f;
    uint32_t best_t = 0xffffffffu, before = 0u;
    for (int64_t i = b; i < e; ++i) {
      const uint32_t t = topic[i];
      const float w = weight[i];
      unsigned what = topdocs_entry_fault(t, k, i == b, before);
      if (!what && !prev_weight_ok(w)) what = PREV_BAD_WEIGHT;
      if (what) atomicMin(err + 1, ((unsigned long long)i << 2) | (unsigned long long)what);
      before = t;
      s = s + (double)w;
      if (i == b || prev_heavier(w, best)) {
        best = w;
        best_t = t;
      }
      if (in && t < k) tp_bump<LDS>(tp_hist, count, (uint64_t)lab * k + t, c0 + lab * k + t);
    }
    if (rs) rs[r] = s;
    if (!bad) tp_bump<LDS>(tp_hist, docs, in ? lab : G, in ? lab : G);
    if (in && best_t < k) tp_bump<LDS>(tp_hist, dominant, (uint64_t)lab * k + best_t, d0 + lab * k + best_t);
  }
  if (LDS) {
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < words; i += TP_T) {
      const uint32_t n = tp_hist[i];
      if (!n) continue;
      if (i < c0) atomicAdd(docs + i, (unsigned long long)n);
      else if (i < d0) atomicAdd(count + (i - c0), (unsigned long long)n);
      else atomicAdd(dominant + (i - d0), (unsigned long long)n);
    }
  }
}

// cnt[g] = ceil((base[g + 1] - base[g]) / 64): the next level's values of every group
__global__ __launch_bounds__(TP_T) void tp_next_k(const unsigned long long* __restrict__ base, uint32_t G, unsigned long long* __restrict__ cnt) {
  const uint32_t g = blockIdx.x * TP_T + threadIdx.x;
  if (g < G) cnt[g] = (base[g + 1] - base[g] + (PREV_FAN - 1)) / PREV_FAN;
}

// base0 / base1: the bases of the list and of the blocks (G + 1 each); total1 = base1[G] blocks.  Topics [t0, t0 + tw) of k.
// out: total1 x tw partials, or, where this level is the last (every group has at most one block), sum (G x k).  LDS: TP_WAVES x tw doubles.
template <bool NORM>
__global__ __launch_bounds__(TP_T) void tp_level0_k(const int64_t* __restrict__ off, const uint32_t* __restrict__ topic, const float* __restrict__ weight,
                                                    const uint32_t* __restrict__ list, const double* __restrict__ rs, uint32_t G,
                                                    const unsigned long long* __restrict__ base0, const unsigned long long* __restrict__ base1,
                                                    unsigned long long total1, uint32_t t0, uint32_t tw, uint32_t k, double* __restrict__ out, bool last) {
  extern __shared__ double tp_tab[];
  const uint32_t lane = threadIdx.x & 63u;
  double* const tab = tp_tab + (size_t)(threadIdx.x >> 6) * tw;
  for (unsigned long long blk = (unsigned long long)blockIdx.x * TP_WAVES + (threadIdx.x >> 6); blk < total1;
       blk += (unsigned long long)gridDim.x * TP_WAVES) {  // wave-uniform
    const uint32_t g = tp_group_of(base1, G, blk);
    const unsigned long long first = base0[g] + (blk - base1[g]) * PREV_FAN, left = base0[g + 1] - first;
    const uint32_t n = left < PREV_FAN ? (uint32_t)left : PREV_FAN;
    for (uint32_t t = lane; t < tw; t += 64u) tab[t] = 0.0;
    const bool have = lane < n;
    const uint64_t r = have ? (list ? (uint64_t)list[first + lane] : (uint64_t)(first + lane)) : 0ull;
    const int64_t mb = have ? off[r] : 0, me = have ? off[r + 1] : 0;
    const double mrs = (NORM && have) ? rs[r] : 0.0;
    for (uint32_t j = 0; j < n; ++j) {
      // (a row's stores are in LDS before the next row's loads: the wave's LDS operations complete in order; the fence holds the compiler)
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      const int64_t b = __shfl(mb, (int)j), e = __shfl(me, (int)j);
      const double rj = NORM ? __shfl(mrs, (int)j) : 0.0;
      for (int64_t p = b + lane; p < e; p += 64) {
        const uint32_t t = topic[p] - t0;  // (below t0: wraps above tw)
        if (t < tw) tab[t] = tab[t] + prev_term(weight[p], NORM ? 1 : 0, rj);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    double* const dst = last ? out + (size_t)g * k + t0 : out + (size_t)blk * tw;
    for (uint32_t t = lane; t < tw; t += 64u) dst[t] = tab[t];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  }
}

// in: the values of level j (base_in), tw wide; out: those of level j + 1 (base_out, total_out values), or sum where that level is the last
__global__ __launch_bounds__(TP_T) void tp_fold_k(const double* __restrict__ in, const unsigned long long* __restrict__ base_in,
                                                  const unsigned long long* __restrict__ base_out, uint32_t G, unsigned long long total_out, uint32_t t0,
                                                  uint32_t tw, uint32_t k, double* __restrict__ out, bool last) {
  const unsigned long long cells = total_out * tw;
  for (unsigned long long idx = (unsigned long long)blockIdx.x * TP_T + threadIdx.x; idx < cells; idx += (unsigned long long)gridDim.x * TP_T) {
    const unsigned long long p = idx / tw;
    const uint32_t t = (uint32_t)(idx - p * tw);
    const uint32_t g = tp_group_of(base_out, G, p);
    const unsigned long long first = base_in[g] + (p - base_out[g]) * PREV_FAN, left = base_in[g + 1] - first;
    const uint32_t n = left < PREV_FAN ? (uint32_t)left : PREV_FAN;
    double s = 0.0;
    for (uint32_t j = 0; j < n; ++j) s = s + in[(first + j) * tw + t];
    if (last) out[(size_t)g * k + t0 + t] = s;
    else out[p * tw + t] = s;
  }
}

}  // namespace

// v: the source's rows, its num_topics k.  groups_dev: rows labels or null.  docs (G + 1, the last the rows of no group), count, dominant
// (G x k): zeroed here.  rs: rows doubles or null; label / rowid: rows each or null.  *bad_row / *bad_entry: ~0 = none.  Drained on return.
int k_tp_rows(isle_ctx* c, const TdView& v, const uint32_t* groups_dev, uint32_t G, uint64_t* docs, uint64_t* count, uint64_t* dominant, double* rs,
              uint64_t* label, uint32_t* rowid, uint64_t* err_dev, uint64_t* bad_row, uint64_t* bad_entry) {
  TimeScope ts(c, v.fam);
  const size_t cells = (size_t)G * v.num_topics;
  *bad_row = *bad_entry = ~0ull;
  HIPCHK(c, hipMemsetAsync(err_dev, 0xff, 2 * sizeof(uint64_t), c->stream));
  HIPCHK(c, hipMemsetAsync(docs, 0, ((size_t)G + 1) * sizeof(uint64_t), c->stream));
  HIPCHK(c, hipMemsetAsync(count, 0, cells * sizeof(uint64_t), c->stream));
  HIPCHK(c, hipMemsetAsync(dominant, 0, cells * sizeof(uint64_t), c->stream));
  const unsigned blocks = (unsigned)std::min<uint64_t>((v.rows + TP_T - 1) / TP_T, (uint64_t)c->num_cus * 8);
  if (!v.rows) {  // (the zeroed tables are the result)
  } else if (prev_hist_in_lds(G, v.num_topics)) {
    const size_t bytes = (2 * cells + G + 1) * sizeof(uint32_t);
    hipLaunchKernelGGL((tp_rows_k<true>), dim3(blocks), dim3(TP_T), bytes, c->stream, v.off, v.topic, v.value, v.rows, v.num_topics, groups_dev, G,
                       (unsigned long long*)docs, (unsigned long long*)count, (unsigned long long*)dominant, rs, (unsigned long long*)label, rowid,
                       (unsigned long long*)err_dev);
  } else {
    hipLaunchKernelGGL((tp_rows_k<false>), dim3(blocks), dim3(TP_T), 0, c->stream, v.off, v.topic, v.value, v.rows, v.num_topics, groups_dev, G,
                       (unsigned long long*)docs, (unsigned long long*)count, (unsigned long long*)dominant, rs, (unsigned long long*)label, rowid,
                       (unsigned long long*)err_dev);
  }
  HIPCHK(c, hipGetLastError());
  uint64_t err[2] = {~0ull, ~0ull};
  HIPCHK(c, hipMemcpyAsync(err, err_dev, sizeof(err), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *bad_row = err[0];
  *bad_entry = err[1];
  return 0;
}

// bases: (levels + 1) x (G + 1); level 0 = the exclusive scan of docs, level j + 1 that of ceil(n / 64).  cnt: G words; blk: scan scratch of G.
int k_tp_bases(isle_ctx* c, int fam, const uint64_t* docs, uint32_t G, int levels, uint64_t* bases, uint64_t* cnt, uint64_t* blk) {
  TimeScope ts(c, fam);
  HIPCHK(c, (isle_scan::exclusive_scan<uint64_t, uint64_t>(c->stream, docs, G, bases, blk)));
  for (int j = 0; j < levels; ++j) {
    uint64_t* const base = bases + (size_t)j * (G + 1);
    hipLaunchKernelGGL(tp_next_k, dim3((G + TP_T - 1) / TP_T), dim3(TP_T), 0, c->stream, (const unsigned long long*)base, G, (unsigned long long*)cnt);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, (isle_scan::exclusive_scan<uint64_t, uint64_t>(c->stream, cnt, G, base + (G + 1), blk)));
  }
  return 0;
}

// One tile of topics [t0, t0 + tw) through every level.  list: the rows by group (null: the identity); totals[j] = the values of level j
// over all groups (host; totals[levels] = the groups that have rows); part_a / part_b: totals[1] x tw and totals[2] x tw doubles.
// sum (G x k) was zeroed by the caller: a group without rows keeps 0.0.
int k_tp_tile(isle_ctx* c, const TdView& v, const uint32_t* list, const double* rs, uint32_t G, const uint64_t* bases, int levels, const uint64_t* totals,
              uint32_t t0, uint32_t tw, double* part_a, double* part_b, double* sum) {
  TimeScope ts(c, v.fam);
  if (!levels) return 0;
  const uint64_t* const base0 = bases;
  const uint64_t* const base1 = bases + (G + 1);
  {
    const bool last = levels == 1;
    const unsigned blocks = (unsigned)std::min<uint64_t>((totals[1] + TP_WAVES - 1) / TP_WAVES, (uint64_t)c->num_cus * 8);
    const size_t bytes = (size_t)TP_WAVES * tw * sizeof(double);  // <= 32 KiB
    if (rs)
      hipLaunchKernelGGL((tp_level0_k<true>), dim3(blocks), dim3(TP_T), bytes, c->stream, v.off, v.topic, v.value, list, rs, G, (const unsigned long long*)base0,
                         (const unsigned long long*)base1, (unsigned long long)totals[1], t0, tw, v.num_topics, last ? sum : part_a, last);
    else
      hipLaunchKernelGGL((tp_level0_k<false>), dim3(blocks), dim3(TP_T), bytes, c->stream, v.off, v.topic, v.value, list, rs, G, (const unsigned long long*)base0,
                         (const unsigned long long*)base1, (unsigned long long)totals[1], t0, tw, v.num_topics, last ? sum : part_a, last);
    HIPCHK(c, hipGetLastError());
  }
  double *in = part_a, *out = part_b;
  for (int j = 1; j < levels; ++j) {
    const bool last = j + 1 == levels;
    const uint64_t cells = totals[j + 1] * tw;
    const unsigned blocks = (unsigned)std::min<uint64_t>((cells + TP_T - 1) / TP_T, (uint64_t)c->num_cus * 16);
    hipLaunchKernelGGL(tp_fold_k, dim3(blocks), dim3(TP_T), 0, c->stream, in, (const unsigned long long*)(bases + (size_t)j * (G + 1)),
                       (const unsigned long long*)(bases + (size_t)(j + 1) * (G + 1)), G, (unsigned long long)totals[j + 1], t0, tw, v.num_topics,
                       last ? sum : out, last);
    HIPCHK(c, hipGetLastError());
    std::swap(in, out);
  }
  return 0;
}
