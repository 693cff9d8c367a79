// isle_amd/csrc/avg_model.hip — the cluster-average topic model (ISLETrainer::output_avg_topic_coherence, src/trainer.cpp:705-745),
// exact top-word selection of a V x ncols model and topic diversity (output_topic_diversity, :750-774).
//
//   am_minmax_k     smallest and largest normalised value of A (positive floats: unsigned order == float order)
//   am_acc_k        s_t[w] += nv[w, d] for every entry of a clustered document, one wave per document.  Every value is an
//                   integer multiple of ulp(smallest value), so v * 2^e (e = -exponent of that ulp) is an exact integer below
//                   2^64; it is split into 32-bit halves added by 64-bit integer atomics into a (lo, hi) pair.  Integer sums are
//                   exact, so the result does not depend on the order of arrival: bitwise reproducible.
//   am_finalize_k   s = hi * 2^32 + lo in double, the column's L1 norm by a fixed-shape reduction, model = (float)(s / norm);
//                   an empty cluster gives 0 / 0 = NaN
//   tw_select_k     n heaviest words of a column: 4-pass radix select of the n-th largest key on the float bits, then the keys
//                   above it and the first ties in id order, ranked (weight descending, id ascending, NaN last).  The column is a
//                   stored one (TwPlain) or an edge topic formed from the model's two columns as it is read (TwEdge)
//   dv_*_k          diversity in double: finite columns, the mean topic over them (topics ascending), squared distances
#include <cmath>
#include <cstring>

#include "common.h"

namespace {

constexpr int AT = 256;
constexpr int AW = AT / ISLE_WAVE;

__global__ __launch_bounds__(AT) void am_minmax_k(const float* __restrict__ nv, uint64_t n, uint32_t* __restrict__ mm) {
  __shared__ uint32_t smin[AT], smax[AT];
  uint32_t lo = 0xffffffffu, hi = 0u;
  for (uint64_t i = (uint64_t)blockIdx.x * AT + threadIdx.x; i < n; i += (uint64_t)gridDim.x * AT) {
    const uint32_t b = __float_as_uint(nv[i]);
    lo = min(lo, b);
    hi = max(hi, b);
  }
  smin[threadIdx.x] = lo;
  smax[threadIdx.x] = hi;
  __syncthreads();
  for (int o = AT / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      smin[threadIdx.x] = min(smin[threadIdx.x], smin[threadIdx.x + o]);
      smax[threadIdx.x] = max(smax[threadIdx.x], smax[threadIdx.x + o]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    atomicMin(&mm[0], smin[0]);
    atomicMax(&mm[1], smax[0]);
  }
}

__global__ __launch_bounds__(AT) void am_acc_k(const uint32_t* __restrict__ rows, const int64_t* __restrict__ offs, const float* __restrict__ nv,
                                                const int32_t* __restrict__ cluster_of, uint64_t D, uint64_t V, int e,
                                                unsigned long long* __restrict__ acc /*V x k pairs (lo, hi), col-major*/) {
  const int lane = threadIdx.x & 63;
  const uint64_t nw = (uint64_t)gridDim.x * AW;
  for (uint64_t d = (uint64_t)blockIdx.x * AW + (threadIdx.x >> 6); d < D; d += nw) {
    const int32_t t = cluster_of[d];
    if (t < 0) continue;
    unsigned long long* col = acc + 2 * (size_t)t * V;
    const int64_t s = offs[d], end = offs[d + 1];
    for (int64_t i = s + lane; i < end; i += 64) {
      const double q = ldexp((double)nv[i], e);  // exact integer < 2^64
      const double qh = floor(ldexp(q, -32));
      const double ql = q - ldexp(qh, 32);       // exact, < 2^32
      unsigned long long* p = col + 2 * (size_t)rows[i];
      atomicAdd(&p[0], (unsigned long long)ql);
      if (qh != 0.0) atomicAdd(&p[1], (unsigned long long)qh);
    }
  }
}

__device__ inline double am_value(const unsigned long long* p) { return ldexp((double)p[1], 32) + (double)p[0]; }

__global__ __launch_bounds__(AT) void am_finalize_k(const unsigned long long* __restrict__ acc, uint64_t V, float* __restrict__ model) {
  __shared__ double sh[AT];
  const unsigned long long* col = acc + 2 * (size_t)blockIdx.x * V;
  float* out = model + (size_t)blockIdx.x * V;
  double s = 0.0;
  for (uint64_t w = threadIdx.x; w < V; w += AT) s += am_value(col + 2 * w);
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int o = AT / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  const double norm = sh[0];
  for (uint64_t w = threadIdx.x; w < V; w += AT) out[w] = (float)(am_value(col + 2 * w) / norm);
}

// larger weight -> larger key; -0 == +0; NaN and -inf -> 0 (hot_path.top_words maps NaN to -inf)
__device__ inline uint32_t tw_key(float x) {
  if (x != x || x == -INFINITY) return 0u;
  const uint32_t u = __float_as_uint(x == 0.f ? 0.f : x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Where tw_select_k reads column blockIdx.x from.  TwPlain: a stored column of a V x ncols model.  TwEdge: the edge topic
// a * model[:, p] + b * model[:, q] formed as it is read, entry for entry as post_edge_k and model_text.hip form it (the product rounded,
// then one fused multiply-add), so that no V x n_edge matrix is stored.
struct TwPlain {
  const float* col;
  __device__ TwPlain(const float* model, const int64_t*, float, float, uint64_t V) : col(model + (size_t)blockIdx.x * V) {}
  __device__ inline float operator[](uint64_t w) const { return col[w]; }
};
struct TwEdge {
  const float *mp, *mq;
  float a, b;
  __device__ TwEdge(const float* model, const int64_t* pairs, float a_, float b_, uint64_t V)
      : mp(model + (size_t)pairs[2 * blockIdx.x] * V), mq(model + (size_t)pairs[2 * blockIdx.x + 1] * V), a(a_), b(b_) {}
  __device__ inline float operator[](uint64_t w) const {
    const float y = a * mp[w];  // FPaxpy into a zeroed column (src/trainer.cpp:1154-1156)
    return fmaf(b, mq[w], y);   // second FPaxpy (:1157-1159)
  }
};

// One workgroup per column; n <= 32 <= AT.
template <class Src>
__global__ __launch_bounds__(AT) void tw_select_k(const float* __restrict__ model, const int64_t* __restrict__ pairs, float ea, float eb, uint64_t V,
                                                   int n, uint32_t* __restrict__ ids, float* __restrict__ weights) {
  __shared__ uint32_t hist[256];
  __shared__ uint32_t sh_digit, sh_remaining, n_gt;
  __shared__ uint32_t sel_id[32];
  __shared__ uint32_t tie_id[AW][32];
  __shared__ uint32_t tie_n[AW];
  const Src col(model, pairs, ea, eb, V);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint32_t prefix = 0, mask = 0, remaining = (uint32_t)n;
  for (int shift = 24; shift >= 0; shift -= 8) {
    hist[threadIdx.x] = 0;
    __syncthreads();
    for (uint64_t w = threadIdx.x; w < V; w += AT) {
      const uint32_t key = tw_key(col[w]);
      if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t cum = 0;
      int dg = 255;
      for (; dg > 0; --dg) {
        if (cum + hist[dg] >= remaining) break;
        cum += hist[dg];
      }
      sh_digit = (uint32_t)dg;
      sh_remaining = remaining - cum;
    }
    __syncthreads();
    prefix |= sh_digit << shift;
    mask |= 255u << shift;
    remaining = sh_remaining;
    __syncthreads();
  }
  // prefix = K, the n-th largest key; `remaining` ties at K are taken (the lowest ids), n - remaining keys lie above K
  const uint32_t K = prefix, r = remaining;
  if (threadIdx.x == 0) n_gt = 0;
  if (lane == 0) tie_n[wv] = 0;
  __syncthreads();
  const uint64_t per = (V + AW - 1) / AW;
  const uint64_t b = (uint64_t)wv * per, e = b + per < V ? b + per : V;
  uint32_t taken = 0;
  for (uint64_t base = b; base < e; base += 64) {
    const uint64_t w = base + lane;
    const uint32_t key = w < e ? tw_key(col[w]) : 0u;
    const bool gt = w < e && key > K, tie = w < e && key == K;
    if (gt) sel_id[atomicAdd(&n_gt, 1u)] = (uint32_t)w;
    const unsigned long long m = __ballot(tie);
    if (tie) {
      const uint32_t pos = taken + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
      if (pos < r) tie_id[wv][pos] = (uint32_t)w;
    }
    taken += (uint32_t)__popcll(m);
  }
  if (lane == 0) tie_n[wv] = taken < r ? taken : r;
  __syncthreads();
  if (threadIdx.x == 0) {  // ties in id order: the waves' ranges are consecutive
    uint32_t at = (uint32_t)n - r;
    for (int q = 0; q < AW && at < (uint32_t)n; ++q)
      for (uint32_t j = 0; j < tie_n[q] && at < (uint32_t)n; ++j) sel_id[at++] = tie_id[q][j];
  }
  __syncthreads();
  if ((int)threadIdx.x < n) {
    const uint32_t id = sel_id[threadIdx.x];
    const float x = col[id];
    const uint64_t me = ((uint64_t)tw_key(x) << 32) | (0xffffffffu - id);
    int rank = 0;
    for (int j = 0; j < n; ++j) {
      const uint32_t oj = sel_id[j];
      const uint64_t other = ((uint64_t)tw_key(col[oj]) << 32) | (0xffffffffu - oj);
      rank += other > me;
    }
    ids[(size_t)blockIdx.x * n + rank] = id;
    if (weights) weights[(size_t)blockIdx.x * n + rank] = x;
  }
}

__global__ __launch_bounds__(AT) void dv_finite_k(const float* __restrict__ model, uint64_t V, int32_t* __restrict__ finite) {
  __shared__ int bad;
  if (threadIdx.x == 0) bad = 0;
  __syncthreads();
  const float* col = model + (size_t)blockIdx.x * V;
  int b = 0;
  for (uint64_t w = threadIdx.x; w < V; w += AT) b |= !isfinite(col[w]);
  if (b) bad = 1;
  __syncthreads();
  if (threadIdx.x == 0) finite[blockIdx.x] = !bad;
}

// abar[w] = (1/k') sum over finite topics, t ascending
__global__ __launch_bounds__(AT) void dv_mean_k(const float* __restrict__ model, uint64_t V, int k, const int32_t* __restrict__ finite, double kp,
                                                 double* __restrict__ abar) {
  const uint64_t w = (uint64_t)blockIdx.x * AT + threadIdx.x;
  if (w >= V) return;
  double s = 0.0;
  for (int t = 0; t < k; ++t)
    if (finite[t]) s += (double)model[(size_t)t * V + w];
  abar[w] = s / kp;  // k' = 0: NaN
}

__global__ __launch_bounds__(AT) void dv_dist_k(const float* __restrict__ model, uint64_t V, const double* __restrict__ abar,
                                                 const int32_t* __restrict__ finite, double* __restrict__ dist) {
  __shared__ double sh[AT];
  const float* col = model + (size_t)blockIdx.x * V;
  double s = 0.0;
  for (uint64_t w = threadIdx.x; w < V; w += AT) {
    const double x = (double)col[w] - abar[w];
    s += x * x;
  }
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int o = AT / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) dist[blockIdx.x] = finite[blockIdx.x] ? sh[0] : (double)NAN;
}

inline unsigned am_doc_grid(isle_ctx* c, uint64_t D) {
  const uint64_t want = (D + AW - 1) / AW;
  return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(want, (uint64_t)c->num_cus * 32));
}

}  // namespace

#define LAUNCH_CHECK(c) HIPCHK(c, hipGetLastError())

// c->p_avg_model = the cluster-average model over c->p_cluster_of and c->a_nv
int k_avg_model(isle_ctx* c, uint32_t k) {
  TimeScope ts(c, ISLE_T_POST);
  const uint64_t V = c->a_V, D = c->a_D, nnz = c->a_nnz;
  int e = 0;
  if (nnz) {
    HIPCHK(c, c->p_counters.reserve(4));
    uint32_t* mm = (uint32_t*)c->p_counters.p;
    const uint32_t init[2] = {0xffffffffu, 0u};
    HIPCHK(c, hipMemcpyAsync(mm, init, sizeof(init), hipMemcpyHostToDevice, c->stream));
    const unsigned g = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((nnz + AT - 1) / AT, (uint64_t)c->num_cus * 8));
    hipLaunchKernelGGL(am_minmax_k, dim3(g), dim3(AT), 0, c->stream, c->a_nv.p, nnz, mm);
    LAUNCH_CHECK(c);
    uint32_t h[2];
    HIPCHK(c, hipMemcpyAsync(h, mm, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    float vmin, vmax;
    std::memcpy(&vmin, &h[0], 4);
    std::memcpy(&vmax, &h[1], 4);
    if (!(vmin > 0.f) || !std::isfinite(vmax))
      return isle_fail(c, ISLE_E_NUMERIC, "avg_topic_model: normalised values outside (0, inf): %g .. %g", (double)vmin, (double)vmax);
    int ex;
    std::frexp(vmin, &ex);  // vmin = m * 2^ex, 0.5 <= m < 1: every value >= vmin is a multiple of 2^(ex - 24)
    e = 24 - ex;
    if (std::ldexp((double)vmax, e) >= 18446744073709551616.0)
      return isle_fail(c, ISLE_E_NUMERIC, "avg_topic_model: normalised values span %g .. %g, beyond the exact accumulator's 2^64 range",
                       (double)vmin, (double)vmax);
  }
  HIPCHK(c, c->p_avg_acc.reserve(2 * V * k));
  HIPCHK(c, c->p_avg_model.reserve(V * k));
  HIPCHK(c, hipMemsetAsync(c->p_avg_acc.p, 0, 2 * V * k * sizeof(uint64_t), c->stream));
  if (D && nnz)
    hipLaunchKernelGGL(am_acc_k, dim3(am_doc_grid(c, D)), dim3(AT), 0, c->stream, c->a_rows.p, c->a_offs.p, c->a_nv.p, c->p_cluster_of.p, D, V, e,
                       (unsigned long long*)c->p_avg_acc.p);
  LAUNCH_CHECK(c);
  hipLaunchKernelGGL(am_finalize_k, dim3(k), dim3(AT), 0, c->stream, (const unsigned long long*)c->p_avg_acc.p, V, c->p_avg_model.p);
  LAUNCH_CHECK(c);
  return 0;
}

int k_model_top_words(isle_ctx* c, const float* model_dev, uint64_t V, uint32_t ncols, int n, uint32_t* ids_dev, float* weights_dev) {
  TimeScope ts(c, ISLE_T_POST);
  if (ncols == 0) return 0;
  hipLaunchKernelGGL(tw_select_k<TwPlain>, dim3(ncols), dim3(AT), 0, c->stream, model_dev, (const int64_t*)nullptr, 0.f, 0.f, V, n, ids_dev,
                     weights_dev);
  LAUNCH_CHECK(c);
  return 0;
}

int k_edge_top_words(isle_ctx* c, const float* model_dev, uint64_t V, const int64_t* pairs_dev, uint32_t n_edge, float a, float b, int n,
                     uint32_t* ids_dev, float* weights_dev) {
  TimeScope ts(c, ISLE_T_POST);
  if (n_edge == 0) return 0;
  hipLaunchKernelGGL(tw_select_k<TwEdge>, dim3(n_edge), dim3(AT), 0, c->stream, model_dev, pairs_dev, a, b, V, n, ids_dev, weights_dev);
  LAUNCH_CHECK(c);
  return 0;
}

// dist (device, k doubles); k' = the number of finite columns (host)
int k_topic_diversity(isle_ctx* c, const float* model_dev, uint64_t V, uint32_t k, double* dist_dev, double* abar_dev, int32_t* finite_dev,
                      uint32_t* kprime) {
  TimeScope ts(c, ISLE_T_POST);
  hipLaunchKernelGGL(dv_finite_k, dim3(k), dim3(AT), 0, c->stream, model_dev, V, finite_dev);
  LAUNCH_CHECK(c);
  std::vector<int32_t> fin(k);
  HIPCHK(c, hipMemcpyAsync(fin.data(), finite_dev, k * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  uint32_t kp = 0;
  for (uint32_t t = 0; t < k; ++t) kp += fin[t] != 0;
  *kprime = kp;
  hipLaunchKernelGGL(dv_mean_k, dim3(cdiv((long)V, AT)), dim3(AT), 0, c->stream, model_dev, V, (int)k, finite_dev, (double)kp,
                     abar_dev);
  hipLaunchKernelGGL(dv_dist_k, dim3(k), dim3(AT), 0, c->stream, model_dev, V, abar_dev, finite_dev, dist_dev);
  LAUNCH_CHECK(c);
  return 0;
}
