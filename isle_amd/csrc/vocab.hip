// isle_amd/csrc/vocab.hip — the device steps of isle_hip_word_doc_freq / isle_hip_prune_vocab on the resident count matrix A (the rule:
// vocab_host.h; the collectives, the rule's run on the host and the swap: api_stages.cpp).  Pure bandwidth work on integers: every result
// is exact and independent of the visiting order.
//   vocab_df_lds_k     df[w] += entries of word w, summed on chip first: a workgroup owns a run of consecutive entries and walks it once per
//                      vocabulary part of VOCAB_DF_PART words, counting into 32-bit counters in LDS (a Zipf corpus has a head word in nearly
//                      every document: its adds meet in LDS, not on one line of HBM), then flushes the non-zero counters with one global
//                      atomic per (workgroup, word).  The run is read from HBM once; the later walks find it in L2.
//   vocab_df_global_k  the same table by one global atomic per entry: the second form (route_vocab_hist), kept for the probe and the tests.
//   vocab_flag_k       flag[e] = remap[rows[e]] is kept, for the scan (scan.h, 64-bit positions)
//   vocab_pack_k       the kept entries to the twin buffers at the scanned positions: counts bit for bit, rows renumbered
//   vocab_offsets_k    new_offs[d] = pos[old_offs[d]] (pos[nnz] = the total, so d = D needs no case of its own), and the documents that
//                      had entries and have none afterwards counted
// Index spaces of nnz are walked in 64 bits by grid-stride loops from grids of bounded size.  rows are read 16 bytes per lane where a whole
// group of four lies inside the range (the buffers are 256-byte aligned, the runs start on multiples of four).
#include <algorithm>

#include "api_internal.h"  // StreamDrain
#include "scan.h"
#include "vocab_host.h"

namespace {

constexpr int VT = 256;
constexpr uint64_t VOCAB_RUN_STEP = 4 * VT;  // a run is a multiple of this: every lane's group of four starts 16-byte aligned

__global__ __launch_bounds__(VT) void vocab_df_lds_k(const uint32_t* __restrict__ rows, uint64_t nnz, uint64_t run, uint32_t V, uint32_t* __restrict__ df) {
  __shared__ uint32_t cnt[VOCAB_DF_PART];
  const uint64_t e0 = (uint64_t)blockIdx.x * run, e1 = min(nnz, e0 + run);
  for (uint32_t w0 = 0; w0 < V; w0 += VOCAB_DF_PART) {
    const uint32_t nw = min(VOCAB_DF_PART, V - w0);
    for (uint32_t j = threadIdx.x; j < nw; j += VT) cnt[j] = 0;
    __syncthreads();
    for (uint64_t e = e0 + 4ull * threadIdx.x; e < e1; e += VOCAB_RUN_STEP) {
      if (e + 4 <= e1) {
        const uint4 r = *reinterpret_cast<const uint4*>(rows + e);
        // (r - w0 wraps below the part: one compare covers both ends)
        if (r.x - w0 < nw) atomicAdd(&cnt[r.x - w0], 1u);
        if (r.y - w0 < nw) atomicAdd(&cnt[r.y - w0], 1u);
        if (r.z - w0 < nw) atomicAdd(&cnt[r.z - w0], 1u);
        if (r.w - w0 < nw) atomicAdd(&cnt[r.w - w0], 1u);
      } else {
        for (uint64_t i = e; i < e1; ++i) {
          const uint32_t l = rows[i] - w0;
          if (l < nw) atomicAdd(&cnt[l], 1u);
        }
      }
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < nw; j += VT)
      if (cnt[j]) atomicAdd(&df[w0 + j], cnt[j]);
    __syncthreads();
  }
}

__global__ __launch_bounds__(VT) void vocab_df_global_k(const uint32_t* __restrict__ rows, uint64_t nnz, uint32_t V, uint32_t* __restrict__ df) {
  const uint64_t stride = (uint64_t)gridDim.x * VOCAB_RUN_STEP;
  for (uint64_t e = (uint64_t)blockIdx.x * VOCAB_RUN_STEP + 4ull * threadIdx.x; e < nnz; e += stride) {
    if (e + 4 <= nnz) {
      const uint4 r = *reinterpret_cast<const uint4*>(rows + e);
      if (r.x < V) atomicAdd(&df[r.x], 1u);
      if (r.y < V) atomicAdd(&df[r.y], 1u);
      if (r.z < V) atomicAdd(&df[r.z], 1u);
      if (r.w < V) atomicAdd(&df[r.w], 1u);
    } else {
      for (uint64_t i = e; i < nnz; ++i)
        if (rows[i] < V) atomicAdd(&df[rows[i]], 1u);
    }
  }
}

__device__ inline uint32_t vocab_kept(const uint32_t* __restrict__ remap, uint32_t V, uint32_t w) { return w < V && remap[w] != VOCAB_DROPPED ? 1u : 0u; }

__global__ __launch_bounds__(VT) void vocab_flag_k(const uint32_t* __restrict__ rows, uint64_t nnz, const uint32_t* __restrict__ remap, uint32_t V,
                                                   uint32_t* __restrict__ flag) {
  const uint64_t stride = (uint64_t)gridDim.x * VOCAB_RUN_STEP;
  for (uint64_t e = (uint64_t)blockIdx.x * VOCAB_RUN_STEP + 4ull * threadIdx.x; e < nnz; e += stride) {
    if (e + 4 <= nnz) {
      const uint4 r = *reinterpret_cast<const uint4*>(rows + e);
      *reinterpret_cast<uint4*>(flag + e) = make_uint4(vocab_kept(remap, V, r.x), vocab_kept(remap, V, r.y), vocab_kept(remap, V, r.z), vocab_kept(remap, V, r.w));
    } else {
      for (uint64_t i = e; i < nnz; ++i) flag[i] = vocab_kept(remap, V, rows[i]);
    }
  }
}

__global__ __launch_bounds__(VT) void vocab_pack_k(const float* __restrict__ cnt, const uint32_t* __restrict__ rows, uint64_t nnz, const uint32_t* __restrict__ remap,
                                                   uint32_t V, const int64_t* __restrict__ pos, uint64_t total, float* __restrict__ new_cnt,
                                                   uint32_t* __restrict__ new_rows) {
  const uint64_t stride = (uint64_t)gridDim.x * VT;
  for (uint64_t e = (uint64_t)blockIdx.x * VT + threadIdx.x; e < nnz; e += stride) {
    const uint32_t w = rows[e];
    const uint32_t nw = w < V ? remap[w] : VOCAB_DROPPED;
    if (nw == VOCAB_DROPPED) continue;
    const uint64_t j = (uint64_t)pos[e];
    if (j < total) {  // (always: pos is the scan of the same flags; the compare keeps a store inside the twin buffers whatever pos holds)
      new_cnt[j] = cnt[e];
      new_rows[j] = nw;
    }
  }
}

__global__ __launch_bounds__(VT) void vocab_offsets_k(const int64_t* __restrict__ offs, uint64_t D, uint64_t nnz, const int64_t* __restrict__ pos,
                                                      int64_t* __restrict__ new_offs, unsigned long long* __restrict__ emptied) {
  const uint64_t stride = (uint64_t)gridDim.x * VT;
  for (uint64_t d = (uint64_t)blockIdx.x * VT + threadIdx.x; d <= D; d += stride) {
    const uint64_t o = min((uint64_t)offs[d], nnz);
    const int64_t n = pos[o];
    new_offs[d] = n;
    if (d < D) {
      const uint64_t o1 = min((uint64_t)offs[d + 1], nnz);
      if (o1 > o && pos[o1] == n) atomicAdd(emptied, 1ull);
    }
  }
}

}  // namespace

#define LAUNCH_CHECK(c) HIPCHK(c, hipGetLastError())

// grid of a grid-stride walk over n items, `per` items per workgroup and step: enough workgroups to fill the device, never 2^32 threads
static unsigned vocab_grid(const isle_ctx* c, uint64_t n, uint64_t per) {
  return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + per - 1) / per, (uint64_t)c->num_cus * 16));
}

// df_dev (a_V words, zeroed here) = this rank's entries per word, in the form asked for (route_vocab_hist)
int k_vocab_df(isle_ctx* c, VocabHist form, uint32_t* df_dev) {
  TimeScope ts(c, ISLE_T_INGEST);
  HIPCHK(c, hipMemsetAsync(df_dev, 0, (size_t)c->a_V * sizeof(uint32_t), c->stream));
  const uint64_t nnz = c->a_nnz;
  if (!nnz) return 0;
  if (form == VOCAB_FORM_LDS) {
    // a run per workgroup: at least four steps (the flush costs up to VOCAB_DF_PART atomics per part), eight workgroups per CU on a large A
    uint64_t run = (nnz + (uint64_t)c->num_cus * 8 - 1) / ((uint64_t)c->num_cus * 8);
    run = std::max<uint64_t>(4 * VOCAB_RUN_STEP, (run + VOCAB_RUN_STEP - 1) / VOCAB_RUN_STEP * VOCAB_RUN_STEP);
    hipLaunchKernelGGL(vocab_df_lds_k, dim3((unsigned)((nnz + run - 1) / run)), dim3(VT), 0, c->stream, c->a_rows.p, nnz, run, (uint32_t)c->a_V, df_dev);
  } else {
    hipLaunchKernelGGL(vocab_df_global_k, dim3(vocab_grid(c, nnz, VOCAB_RUN_STEP)), dim3(VT), 0, c->stream, c->a_rows.p, nnz, (uint32_t)c->a_V, df_dev);
  }
  LAUNCH_CHECK(c);
  return 0;
}

// The resident A compacted out of place under remap_dev (a_V words: the new id, or VOCAB_DROPPED) into the caller's twin buffers, which
// are sized here: *total entries, D + 1 offsets.  *emptied: this rank's documents that lost all of their entries.  Nothing resident is written.
int k_vocab_compact(isle_ctx* c, const uint32_t* remap_dev, DevBuf<float>& new_cnt, DevBuf<uint32_t>& new_rows, DevBuf<int64_t>& new_offs, uint64_t* total,
                    uint64_t* emptied) {
  TimeScope ts(c, ISLE_T_INGEST);
  const uint64_t nnz = c->a_nnz, D = c->a_D;
  const uint32_t V = (uint32_t)c->a_V;
  DevBuf<uint32_t> flag;
  DevBuf<int64_t> pos, scratch;
  DevBuf<unsigned long long> gone;
  StreamDrain drain(c);
  HIPCHK(c, flag.reserve(nnz ? nnz : 1));
  HIPCHK(c, pos.reserve(nnz + 1));
  HIPCHK(c, scratch.reserve(isle_scan_scratch(nnz) + 8));
  HIPCHK(c, gone.reserve(1));
  HIPCHK(c, hipMemsetAsync(gone.p, 0, sizeof(unsigned long long), c->stream));
  if (nnz) hipLaunchKernelGGL(vocab_flag_k, dim3(vocab_grid(c, nnz, VOCAB_RUN_STEP)), dim3(VT), 0, c->stream, c->a_rows.p, nnz, remap_dev, V, flag.p);
  LAUNCH_CHECK(c);
  HIPCHK(c, (isle_scan::exclusive_scan<uint32_t, int64_t>(c->stream, flag.p, nnz, pos.p, scratch.p)));
  int64_t m = 0;
  HIPCHK(c, hipMemcpyAsync(&m, pos.p + nnz, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (m < 0 || (uint64_t)m > nnz) return isle_fail(c, ISLE_E_HIP, "prune_vocab: the scan counts %lld kept entries of %llu", (long long)m, (unsigned long long)nnz);
  HIPCHK(c, new_cnt.reserve(m ? m : 1));
  HIPCHK(c, new_rows.reserve(m ? m : 1));
  HIPCHK(c, new_offs.reserve(D + 1));
  if (nnz && m)
    hipLaunchKernelGGL(vocab_pack_k, dim3(vocab_grid(c, nnz, VT)), dim3(VT), 0, c->stream, c->a_cnt.p, c->a_rows.p, nnz, remap_dev, V, pos.p, (uint64_t)m, new_cnt.p,
                       new_rows.p);
  LAUNCH_CHECK(c);
  hipLaunchKernelGGL(vocab_offsets_k, dim3(vocab_grid(c, D + 1, VT)), dim3(VT), 0, c->stream, c->a_offs.p, D, nnz, pos.p, new_offs.p, gone.p);
  LAUNCH_CHECK(c);
  unsigned long long g = 0;
  HIPCHK(c, hipMemcpyAsync(&g, gone.p, sizeof(g), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *total = (uint64_t)m;
  *emptied = g;
  return 0;
}
