// isle_amd/csrc/coherence.hip — document frequencies behind UMass topic coherence (SparseMatrix::topic_coherence,
// compute_doc_frequency, compute_joint_doc_frequency, src/sparseMatrix.cpp:841-1016) on the count matrix A in HBM.
//
//   coh_count_k      one pass over A per counter tile: D(w) for the distinct top words U and D(w_lo, w_hi) for the distinct
//                    word pairs P, as u32 counters in LDS, flushed once per workgroup by contiguous global adds
//   coh_lut_fill_k   word -> local id table in HBM, for vocabularies whose membership bitmap does not fit in LDS
//
// The counter space is [0, |U|) for the words and |U| + pair id for the pairs (pair ids: P sorted by (lo, hi), local ids = rank of
// the word in U).  A tile is a contiguous range of it; tiles are walked one pass over A each.  A wave takes one document at a time:
// lanes load 64 row ids, look each up (bitmap + per-word prefix count in LDS, or the HBM table), and the hits are compacted by ballot
// into the wave's hit list in LDS.  Rows ascend within a column and local ids follow word order, so the list is sorted: each hit then
// walks its partners (pair CSR keyed by lo) and binary-searches each partner's local id in the rest of the list.  A document with more
// hits than the list holds searches the partner's WORD in the document's own rows in HBM instead (same result, slower).
// All counts are integer adds: the result does not depend on the order of documents, waves or workgroups.
#include "common.h"

namespace {

constexpr int CT = 1024;               // threads per workgroup: 16 waves share one copy of the bitmap and of the counters
constexpr int CW = CT / ISLE_WAVE;
constexpr uint32_t HCAP = 256;         // hit-list entries per wave (config 3 documents hold about 110 entries in all)
constexpr size_t COH_LDS = 160 * 1024 - 512;
constexpr uint32_t NONE32 = 0xffffffffu;
constexpr uint64_t COH_BITMAP_MAX_V = 131072;  // bitmap + prefix counts: 32 KB of LDS; above it the word -> local id table in HBM

__device__ inline void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// first index in [lo, hi) of the ascending array a with a[i] >= x
template <class P>
__device__ inline uint64_t lower_bound_u32(P a, uint64_t lo, uint64_t hi, uint32_t x) {
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

template <bool LUT>
__device__ inline uint32_t lookup(uint32_t w, const uint32_t* s_bits, const uint32_t* s_pref, const uint32_t* __restrict__ lut) {
  if (LUT) return lut[w];
  const uint32_t b = s_bits[w >> 5], bit = 1u << (w & 31u);
  return (b & bit) ? s_pref[w >> 5] + (uint32_t)__popc(b & (bit - 1u)) : NONE32;
}

// Counter tile [c0, c0 + nc) of the space described above.  nwords: 32-bit words of the bitmap (0 on the LUT path).
template <bool LUT>
__global__ __launch_bounds__(CT) void coh_count_k(const uint32_t* __restrict__ rows, const int64_t* __restrict__ offs, uint64_t D,
                                                  const uint32_t* __restrict__ bits, const uint32_t* __restrict__ pref, uint32_t nwords,
                                                  const uint32_t* __restrict__ lut, const uint32_t* __restrict__ uword,
                                                  const uint32_t* __restrict__ part_off, const uint32_t* __restrict__ part_hi, uint32_t nU,
                                                  uint32_t c0, uint32_t nc, uint32_t* __restrict__ gcnt) {
  extern __shared__ uint32_t sm[];
  uint32_t* s_bits = sm;
  uint32_t* s_pref = sm + nwords;
  uint32_t* s_hits = sm + 2 * (size_t)nwords;
  uint32_t* s_cnt = s_hits + (size_t)CW * HCAP;
  for (uint32_t i = threadIdx.x; i < nwords; i += CT) {
    s_bits[i] = bits[i];
    s_pref[i] = pref[i];
  }
  for (uint32_t i = threadIdx.x; i < nc; i += CT) s_cnt[i] = 0u;
  __syncthreads();

  const int lane = threadIdx.x & 63;
  const uint32_t wv = threadIdx.x >> 6;
  uint32_t* hl = s_hits + wv * HCAP;
  const uint64_t c1 = (uint64_t)c0 + nc;
  const bool pairs_in_tile = c1 > nU;
  for (uint64_t d = (uint64_t)blockIdx.x * CW + wv; d < D; d += (uint64_t)gridDim.x * CW) {
    const int64_t s = offs[d], e = offs[d + 1];
    uint32_t h = 0;  // hits so far (wave-uniform)
    for (int64_t base = s; base < e; base += 64) {
      const int64_t i = base + lane;
      const uint32_t loc = i < e ? lookup<LUT>(rows[i], s_bits, s_pref, lut) : NONE32;
      const uint64_t m = __ballot(loc != NONE32);
      if (loc != NONE32) {
        const uint32_t pos = h + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        if (pos < HCAP) hl[pos] = loc;
        if (loc >= c0 && (uint64_t)loc < c1) atomicAdd(&s_cnt[loc - c0], 1u);
      }
      h += (uint32_t)__popcll(m);
    }
    if (h < 2 || !pairs_in_tile) continue;
    wave_sync();
    if (h <= HCAP) {
      for (uint32_t k = lane; k < h; k += 64) {
        const uint32_t a = hl[k];
        const uint64_t pb = (uint64_t)nU + part_off[a], pe = (uint64_t)nU + part_off[a + 1];
        const uint64_t cb = pb > c0 ? pb : (uint64_t)c0, ce = pe < c1 ? pe : c1;
        for (uint64_t cc = cb; cc < ce; ++cc) {
          const uint32_t hi = part_hi[cc - nU];
          const uint64_t at = lower_bound_u32(hl, k + 1, h, hi);
          if (at < h && hl[at] == hi) atomicAdd(&s_cnt[cc - c0], 1u);
        }
      }
    } else {  // more hits than the list holds: search the partner's word in the document's rows
      for (int64_t i = s + lane; i < e; i += 64) {
        const uint32_t a = lookup<LUT>(rows[i], s_bits, s_pref, lut);
        if (a == NONE32) continue;
        const uint64_t pb = (uint64_t)nU + part_off[a], pe = (uint64_t)nU + part_off[a + 1];
        const uint64_t cb = pb > c0 ? pb : (uint64_t)c0, ce = pe < c1 ? pe : c1;
        for (uint64_t cc = cb; cc < ce; ++cc) {
          const uint32_t w = uword[part_hi[cc - nU]];
          const int64_t at = (int64_t)lower_bound_u32(rows, (uint64_t)(i + 1), (uint64_t)e, w);
          if (at < e && rows[at] == w) atomicAdd(&s_cnt[cc - c0], 1u);
        }
      }
    }
    wave_sync();  // every lane is done with the list before the next document overwrites it
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < nc; i += CT) {
    const uint32_t v = s_cnt[i];
    if (v) atomicAdd(&gcnt[(uint64_t)c0 + i], v);
  }
}

__global__ __launch_bounds__(256) void coh_lut_fill_k(uint32_t* __restrict__ lut, uint64_t V) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < V) lut[i] = NONE32;
}
__global__ __launch_bounds__(256) void coh_lut_scatter_k(uint32_t* __restrict__ lut, const uint32_t* __restrict__ uword, uint32_t nU) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < nU) lut[uword[i]] = i;
}

}  // namespace

#define LAUNCH_CHECK(c) HIPCHK(c, hipGetLastError())

// U: ascending distinct words; part_off (|U| + 1) / part_hi (|P|): the pairs (lo, hi) of local ids, sorted, as a CSR keyed by lo.
// counts (out, host): |U| + |P| entries, D(w) then D(pair).  passes (out): tiles, i.e. passes over A.
int k_coherence_counts(isle_ctx* c, const std::vector<uint32_t>& U, const std::vector<uint32_t>& part_off, const std::vector<uint32_t>& part_hi,
                       std::vector<uint32_t>& counts, int* passes) {
  TimeScope ts(c, ISLE_T_POST);
  const uint64_t V = c->a_V, D = c->a_D;
  const uint32_t nU = (uint32_t)U.size();
  const uint64_t N = (uint64_t)nU + part_hi.size();
  if (N >= 0xffffffffull) return isle_fail(c, ISLE_E_ARG, "topic_coherence: %llu counters exceed 32-bit ids", (unsigned long long)N);
  const bool use_lut = V > COH_BITMAP_MAX_V;
  const uint32_t nwords = use_lut ? 0u : (uint32_t)((V + 31) / 32);
  const size_t fixed = (2 * (size_t)nwords + (size_t)CW * HCAP) * sizeof(uint32_t);
  const uint64_t tile = (COH_LDS - fixed) / sizeof(uint32_t);

  std::vector<uint32_t> bits(nwords ? nwords : 1, 0u), pref(nwords ? nwords : 1, 0u);
  if (!use_lut) {
    for (uint32_t w : U) bits[w >> 5] |= 1u << (w & 31u);
    uint32_t run = 0;
    for (uint32_t i = 0; i < nwords; ++i) {
      pref[i] = run;
      run += (uint32_t)__builtin_popcount(bits[i]);
    }
  }
  DevBuf<uint32_t> d_bits, d_pref, d_lut, d_uword, d_off, d_hi, d_cnt;
  HIPCHK(c, d_bits.reserve(bits.size()));
  HIPCHK(c, d_pref.reserve(pref.size()));
  HIPCHK(c, d_lut.reserve(use_lut ? V : 1));
  HIPCHK(c, d_uword.reserve(nU ? nU : 1));
  HIPCHK(c, d_off.reserve(part_off.size()));
  HIPCHK(c, d_hi.reserve(part_hi.empty() ? 1 : part_hi.size()));
  HIPCHK(c, d_cnt.reserve(N ? N : 1));
  HIPCHK(c, hipMemcpyAsync(d_bits.p, bits.data(), bits.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_pref.p, pref.data(), pref.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  if (nU) HIPCHK(c, hipMemcpyAsync(d_uword.p, U.data(), nU * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_off.p, part_off.data(), part_off.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  if (!part_hi.empty()) HIPCHK(c, hipMemcpyAsync(d_hi.p, part_hi.data(), part_hi.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(d_cnt.p, 0, (N ? N : 1) * sizeof(uint32_t), c->stream));
  if (use_lut) {
    hipLaunchKernelGGL(coh_lut_fill_k, dim3(cdiv((long)V, 256)), dim3(256), 0, c->stream, d_lut.p, V);
    if (nU) hipLaunchKernelGGL(coh_lut_scatter_k, dim3(cdiv((long)nU, 256)), dim3(256), 0, c->stream, d_lut.p, d_uword.p, nU);
    LAUNCH_CHECK(c);
  }

  int np = 0;
  if (D && N) {
    const size_t lds_max = fixed + (size_t)std::min<uint64_t>(tile, N) * sizeof(uint32_t);
    const void* fn = use_lut ? (const void*)coh_count_k<true> : (const void*)coh_count_k<false>;
    ISLECHK(isle_max_lds(c, fn, (int)lds_max));
    for (uint64_t c0 = 0; c0 < N; c0 += tile) {
      const uint32_t nc = (uint32_t)std::min<uint64_t>(tile, N - c0);
      const size_t lds = fixed + (size_t)nc * sizeof(uint32_t);
      const uint64_t per_cu = std::max<uint64_t>(1, (COH_LDS + 512) / lds);
      const unsigned g = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((D + CW - 1) / CW, (uint64_t)c->num_cus * std::min<uint64_t>(per_cu, 2)));
      if (use_lut)
        hipLaunchKernelGGL(coh_count_k<true>, dim3(g), dim3(CT), lds, c->stream, c->a_rows.p, c->a_offs.p, D, d_bits.p, d_pref.p, 0u, d_lut.p,
                           d_uword.p, d_off.p, d_hi.p, nU, (uint32_t)c0, nc, d_cnt.p);
      else
        hipLaunchKernelGGL(coh_count_k<false>, dim3(g), dim3(CT), lds, c->stream, c->a_rows.p, c->a_offs.p, D, d_bits.p, d_pref.p, nwords,
                           d_lut.p, d_uword.p, d_off.p, d_hi.p, nU, (uint32_t)c0, nc, d_cnt.p);
      LAUNCH_CHECK(c);
      ++np;
    }
  }
  counts.assign(N, 0u);
  if (N) HIPCHK(c, hipMemcpyAsync(counts.data(), d_cnt.p, N * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (passes) *passes = np;
  return 0;
}
