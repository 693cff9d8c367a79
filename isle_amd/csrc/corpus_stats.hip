// isle_amd/csrc/corpus_stats.hip — the two corpus diagnostics of the reference trainer on the count matrix A in HBM
// (ISLETrainer::print_log_combinatorial / print_distinct_top_five_sets, src/trainer.cpp:373-403).
//
//   cs_doc_words_k   N_d = sum of (int)count over document d, a wave per document (integer adds: any order),   src/sparseMatrix.cpp:1020-1030
//                    and the corpus maximum
//   cs_log_comb_k    0 - log_fact[(int)c_0] - log_fact[(int)c_1] - ... + log_fact[N_d] in fp32, one lane per   :1036-1042
//                    document walking its entries in CSC order (the reference's order: bit-equal); the table
//                    (built on the host as the reference builds it) from LDS when it fits, else from HBM
//   cs_top5_k        the 5 largest normalised values of every document with >= 5 entries, with multiplicity: a  src/sparseMatrix.cpp:174-183
//                    wave per document, a sorted top 5 per lane, merged by 5 wave-wide arg-max rounds
//   cs_key_k         sort keys for the three stable LSD passes (k_sort_pairs_u64, ingest.hip) that order the    :184-195
//                    tuples lexicographically: (q4, q5), then (q2, q3), then q1, the tuple index as payload
//   cs_flag_k        run starts of equal tuples in sorted order, compacted to positions by a scan            :198-208 (the count rule
//                                                                                                              on the run lengths: host)
// The normalised values are non-negative floats, so their u32 bit patterns order as the floats do and equality is bit equality.
#include <climits>
#include <cmath>
#include <utility>

#include "common.h"
#include "scan.h"

namespace {

constexpr int CT = 256;
constexpr int CW = CT / ISLE_WAVE;
constexpr uint32_t LF_LDS_MAX = 16384;  // table entries read from LDS (64 KB); larger tables are read from HBM through the caches

inline unsigned grid_for(isle_ctx* c, uint64_t items, uint64_t per_block) {
  const uint64_t want = (items + per_block - 1) / per_block;
  return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(want, (uint64_t)c->num_cus * 32));
}

// (int)count as the reference takes it; counts at or above 2^31 (undefined there) map above INT_MAX so that N_d is refused
__device__ inline uint64_t int_count(float x) { return x < 2147483648.f ? (uint64_t)(int)x : 0x80000000ull; }

__global__ __launch_bounds__(CT) void cs_doc_words_k(const float* __restrict__ cnt, const int64_t* __restrict__ offs, uint64_t D,
                                                     uint32_t* __restrict__ nd, unsigned long long* __restrict__ maxn) {
  const int lane = threadIdx.x & 63;
  unsigned long long mx = 0;
  for (uint64_t d = (uint64_t)blockIdx.x * CW + (threadIdx.x >> 6); d < D; d += (uint64_t)gridDim.x * CW) {
    const int64_t s = offs[d], e = offs[d + 1];
    unsigned long long n = 0;
    for (int64_t i = s + lane; i < e; i += 64) n += int_count(cnt[i]);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) n += __shfl_xor(n, o);
    if (lane == 0) nd[d] = n > 0xffffffffull ? 0xffffffffu : (uint32_t)n;
    mx = n > mx ? n : mx;
  }
  if (lane == 0 && mx) atomicMax(maxn, mx);
}

// every N_d <= INT_MAX and the table has max N_d + 1 entries, so every index below is in range
template <bool LDS>
__global__ __launch_bounds__(CT) void cs_log_comb_k(const float* __restrict__ cnt, const int64_t* __restrict__ offs, uint64_t D,
                                                    const uint32_t* __restrict__ nd, const float* __restrict__ lf, uint32_t nlf,
                                                    float* __restrict__ out) {
  extern __shared__ float s_lf[];
  if (LDS) {
    for (uint32_t i = threadIdx.x; i < nlf; i += CT) s_lf[i] = lf[i];
    __syncthreads();
  }
  const float* T = LDS ? s_lf : lf;
  for (uint64_t d = (uint64_t)blockIdx.x * CT + threadIdx.x; d < D; d += (uint64_t)gridDim.x * CT) {
    const int64_t s = offs[d], e = offs[d + 1];
    float acc = 0.f;
    for (int64_t i = s; i < e; ++i) acc -= T[(int)cnt[i]];
    acc += T[nd[d]];
    out[d] = acc;
  }
}

__global__ __launch_bounds__(CT) void cs_five_flag_k(const int64_t* __restrict__ offs, uint64_t D, uint32_t* __restrict__ flag) {
  const uint64_t d = (uint64_t)blockIdx.x * CT + threadIdx.x;
  if (d < D) flag[d] = offs[d + 1] - offs[d] >= 5 ? 1u : 0u;
}

// insert v into the descending a[0..4] (the smallest is dropped)
__device__ inline void top5_insert(uint32_t (&a)[5], uint32_t v) {
  if (v <= a[4]) return;
  a[4] = v;
#pragma unroll
  for (int j = 4; j > 0; --j)
    if (a[j] > a[j - 1]) {
      const uint32_t t = a[j];
      a[j] = a[j - 1];
      a[j - 1] = t;
    }
}

// q: 5 x n, q[j * n + p] = the (j+1)-th largest value of the p-th qualifying document; pos: exclusive scan of cs_five_flag_k.
// Lanes start from 0 (the smallest possible value): a lane with fewer than 5 entries contributes zeros, which can only be chosen
// where the document itself holds zeros, so the tuple is the same.
__global__ __launch_bounds__(CT) void cs_top5_k(const uint32_t* __restrict__ nv, const int64_t* __restrict__ offs, uint64_t D,
                                                const int64_t* __restrict__ pos, uint64_t n, uint32_t* __restrict__ q) {
  const int lane = threadIdx.x & 63;
  for (uint64_t d = (uint64_t)blockIdx.x * CW + (threadIdx.x >> 6); d < D; d += (uint64_t)gridDim.x * CW) {
    const int64_t s = offs[d], e = offs[d + 1];
    if (e - s < 5) continue;
    uint32_t a[5] = {0u, 0u, 0u, 0u, 0u};
    for (int64_t i = s + lane; i < e; i += 64) top5_insert(a, nv[i]);
    uint32_t r[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      uint32_t m = a[0];
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) {
        const uint32_t x = __shfl_xor(m, o);
        m = x > m ? x : m;
      }
      const uint64_t holders = __ballot(a[0] == m);
      if (lane == __ffsll((unsigned long long)holders) - 1) {  // one holder pops its head
        a[0] = a[1];
        a[1] = a[2];
        a[2] = a[3];
        a[3] = a[4];
        a[4] = 0u;
      }
      r[k] = m;
    }
    if (lane < 5) {
      const uint64_t p = (uint64_t)pos[d];
      uint32_t v = r[0];
#pragma unroll
      for (int k = 1; k < 5; ++k) v = lane == k ? r[k] : v;
      q[(uint64_t)lane * n + p] = v;
    }
  }
}

// key = q[hi][t] << 32 | q[lo][t] (lo < 0: q[hi][t] alone), payload t, t = perm[i] (perm == nullptr: t = i)
__global__ __launch_bounds__(CT) void cs_key_k(const uint32_t* __restrict__ q, uint64_t n, const uint32_t* __restrict__ perm, int hi, int lo,
                                               uint64_t* __restrict__ key, uint32_t* __restrict__ val) {
  const uint64_t i = (uint64_t)blockIdx.x * CT + threadIdx.x;
  if (i >= n) return;
  const uint32_t t = perm ? perm[i] : (uint32_t)i;
  const uint64_t h = q[(uint64_t)hi * n + t];
  key[i] = lo < 0 ? h : (h << 32 | q[(uint64_t)lo * n + t]);
  val[i] = t;
}

__global__ __launch_bounds__(CT) void cs_flag_k(const uint32_t* __restrict__ q, uint64_t n, const uint32_t* __restrict__ perm, uint32_t* __restrict__ flag) {
  const uint64_t i = (uint64_t)blockIdx.x * CT + threadIdx.x;
  if (i >= n) return;
  uint32_t f = 1u;
  if (i > 0) {
    const uint32_t a = perm[i], b = perm[i - 1];
    f = 0u;
#pragma unroll
    for (int j = 0; j < 5; ++j) f |= q[(uint64_t)j * n + a] != q[(uint64_t)j * n + b];
  }
  flag[i] = f;
}

__global__ __launch_bounds__(CT) void cs_starts_k(const uint32_t* __restrict__ flag, const int64_t* __restrict__ at, uint64_t n, uint64_t* __restrict__ starts) {
  const uint64_t i = (uint64_t)blockIdx.x * CT + threadIdx.x;
  if (i < n && flag[i]) starts[at[i]] = i;
}

// out (n x 5, row-major): the tuples in sorted order, as floats
__global__ __launch_bounds__(CT) void cs_gather_k(const uint32_t* __restrict__ q, uint64_t n, const uint32_t* __restrict__ perm, uint32_t* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * CT + threadIdx.x;
  if (i >= n) return;
  const uint32_t t = perm[i];
#pragma unroll
  for (int j = 0; j < 5; ++j) out[i * 5 + j] = q[(uint64_t)j * n + t];
}

}  // namespace

#define LAUNCH_CHECK(c) HIPCHK(c, hipGetLastError())

// out (host, a_D floats): every document's log multinomial coefficient; max_words (nullable): the largest N_d.
int k_log_combinatorial(isle_ctx* c, float* out, uint64_t* max_words) {
  TimeScope ts(c, ISLE_T_POST);
  const uint64_t D = c->a_D;
  DevBuf<uint32_t> nd;
  DevBuf<unsigned long long> mx;
  DevBuf<float> lf, res;
  HIPCHK(c, nd.reserve(D ? D : 1));
  HIPCHK(c, mx.reserve(1));
  HIPCHK(c, hipMemsetAsync(mx.p, 0, sizeof(unsigned long long), c->stream));
  if (D) hipLaunchKernelGGL(cs_doc_words_k, dim3(grid_for(c, D, CW)), dim3(CT), 0, c->stream, c->a_cnt.p, c->a_offs.p, D, nd.p, mx.p);
  LAUNCH_CHECK(c);
  unsigned long long maxn = 0;
  HIPCHK(c, hipMemcpyAsync(&maxn, mx.p, sizeof(maxn), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (max_words) *max_words = maxn;
  if (maxn > (unsigned long long)INT_MAX)
    return isle_fail(c, ISLE_E_ARG, "log_combinatorial: a document holds %llu words, more than the reference's int table index", maxn);
  // src/sparseMatrix.cpp:1032-1034: log_fact[i + 1] = log_fact[i] + std::log(i + 1), the sum in double, stored as float
  const uint32_t nlf = (uint32_t)maxn + 1;
  std::vector<float> h_lf(nlf);
  h_lf[0] = 0.f;
  for (uint32_t i = 0; i + 1 < nlf; ++i) h_lf[i + 1] = (float)((double)h_lf[i] + std::log((double)(i + 1)));
  HIPCHK(c, lf.reserve(nlf));
  HIPCHK(c, res.reserve(D ? D : 1));
  HIPCHK(c, hipMemcpyAsync(lf.p, h_lf.data(), (size_t)nlf * sizeof(float), hipMemcpyHostToDevice, c->stream));
  if (D) {
    const unsigned g = grid_for(c, D, CT);
    if (nlf <= LF_LDS_MAX) {
      ISLECHK(isle_max_lds(c, (const void*)cs_log_comb_k<true>, (int)(nlf * sizeof(float))));
      hipLaunchKernelGGL(cs_log_comb_k<true>, dim3(g), dim3(CT), (size_t)nlf * sizeof(float), c->stream, c->a_cnt.p, c->a_offs.p, D, nd.p, lf.p, nlf,
                         res.p);
    } else {
      hipLaunchKernelGGL(cs_log_comb_k<false>, dim3(g), dim3(CT), 0, c->stream, c->a_cnt.p, c->a_offs.p, D, nd.p, lf.p, nlf, res.p);
    }
    LAUNCH_CHECK(c);
    HIPCHK(c, hipMemcpyAsync(out, res.p, D * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

// Needs c->a_nv (k_post_normalize).  n_out: tuples (documents with >= 5 entries); runs: lengths of the runs of equal tuples in
// ascending lexicographic order; tuples (nullable, host, n x 5 floats row-major): the sorted tuples.
int k_top_five_runs(isle_ctx* c, uint64_t* n_out, std::vector<uint64_t>& runs, float* tuples) {
  TimeScope ts(c, ISLE_T_POST);
  const uint64_t D = c->a_D;
  runs.clear();
  *n_out = 0;
  if (D == 0) return 0;
  DevBuf<uint32_t> flag, q, va, vb;
  DevBuf<int64_t> pos, scratch;
  DevBuf<uint64_t> ka, kb;
  HIPCHK(c, flag.reserve(D));
  HIPCHK(c, pos.reserve(D + 1));
  HIPCHK(c, scratch.reserve(isle_scan_scratch(D) + 8));
  hipLaunchKernelGGL(cs_five_flag_k, dim3(cdiv((long)D, CT)), dim3(CT), 0, c->stream, c->a_offs.p, D, flag.p);
  LAUNCH_CHECK(c);
  HIPCHK(c, (isle_scan::exclusive_scan<uint32_t, int64_t>(c->stream, flag.p, D, pos.p, scratch.p)));
  int64_t nn = 0;
  HIPCHK(c, hipMemcpyAsync(&nn, pos.p + D, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const uint64_t n = (uint64_t)nn;
  *n_out = n;
  if (n == 0) return 0;
  HIPCHK(c, q.reserve(5 * n));
  hipLaunchKernelGGL(cs_top5_k, dim3(grid_for(c, D, CW)), dim3(CT), 0, c->stream, (const uint32_t*)c->a_nv.p, c->a_offs.p, D, pos.p, n, q.p);
  LAUNCH_CHECK(c);

  // lexicographic order by three stable passes, least significant columns first
  HIPCHK(c, ka.reserve(n));
  HIPCHK(c, kb.reserve(n));
  HIPCHK(c, va.reserve(n));
  HIPCHK(c, vb.reserve(n));
  static const int cols[3][2] = {{3, 4}, {1, 2}, {0, -1}};
  const unsigned g = (unsigned)cdiv((long)n, CT);
  uint64_t *kx = ka.p, *ky = kb.p;
  uint32_t *vx = va.p, *vy = vb.p;
  const uint32_t* perm = nullptr;
  for (int pass = 0; pass < 3; ++pass) {
    hipLaunchKernelGGL(cs_key_k, dim3(g), dim3(CT), 0, c->stream, q.p, n, perm, cols[pass][0], cols[pass][1], kx, vx);
    LAUNCH_CHECK(c);
    bool in_x = true;
    ISLECHK(k_sort_pairs_u64(c, kx, vx, ky, vy, n, cols[pass][1] < 0 ? 32 : 64, &in_x));
    if (!in_x) {
      std::swap(kx, ky);
      std::swap(vx, vy);
    }
    perm = vx;  // sorted payload; the next pass writes its keys into the other pair
    std::swap(kx, ky);
    std::swap(vx, vy);
  }

  // runs of equal tuples: their starts, compacted in order
  DevBuf<uint64_t> starts;
  HIPCHK(c, flag.reserve(n));
  HIPCHK(c, pos.reserve(n + 1));
  HIPCHK(c, scratch.reserve(isle_scan_scratch(n) + 8));
  hipLaunchKernelGGL(cs_flag_k, dim3(g), dim3(CT), 0, c->stream, q.p, n, perm, flag.p);
  LAUNCH_CHECK(c);
  HIPCHK(c, (isle_scan::exclusive_scan<uint32_t, int64_t>(c->stream, flag.p, n, pos.p, scratch.p)));
  int64_t nr = 0;
  HIPCHK(c, hipMemcpyAsync(&nr, pos.p + n, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, starts.reserve((size_t)nr));
  hipLaunchKernelGGL(cs_starts_k, dim3(g), dim3(CT), 0, c->stream, flag.p, pos.p, n, starts.p);
  LAUNCH_CHECK(c);
  runs.resize((size_t)nr);
  HIPCHK(c, hipMemcpyAsync(runs.data(), starts.p, (size_t)nr * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  if (tuples) {
    DevBuf<uint32_t> out;
    HIPCHK(c, out.reserve(5 * n));
    hipLaunchKernelGGL(cs_gather_k, dim3(g), dim3(CT), 0, c->stream, q.p, n, perm, out.p);
    LAUNCH_CHECK(c);
    HIPCHK(c, hipMemcpyAsync(tuples, out.p, 5 * n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (size_t r = 0; r < runs.size(); ++r) runs[r] = (r + 1 < runs.size() ? runs[r + 1] : n) - runs[r];
  return 0;
}
