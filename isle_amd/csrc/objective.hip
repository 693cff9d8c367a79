// isle_amd/csrc/objective.hip — the k-means objective of a partition, per cluster, in word space and in span(U)
// (the residual of FPSparseMatrix::lloyds_iter, src/sparseMatrix.cpp:1649-1663; its projected twin is unwritten there, :1995-1998).
//
//   ob_cnorm_k      |c_t|^2 in fp64 over the V rows of the row-major centres: 64 columns x 16 row slices per workgroup, each slice summed
//                   in row order, the slices by a fixed tree
//   ob_word_k       a wave per document: lanes stride its entries, v^2 - 2 v C[w, t] per entry in fp64 (both products exact), a fixed
//                   xor tree over the lanes, + |c_t|^2, clamped at 0.  The value depends on the document and its centre alone: not on the
//                   workgroup, the rank or the visiting order (documents are visited grouped by centre for the centre column's sake)
//   ob_proj_k       a wave per row of P: (p_dj - c_tj)^2 in fp64, lanes stride the coordinates, the same tree
//   (both)          the largest distance's high word by an integer atomicMax: with its exponent ex (all ranks': an all-reduce(MAX) of one
//                   word) and q = 2^(ex - 53) every rint(dist / q) is an integer below 2^53
//   ob_acc_k        those integers split into 32-bit halves and added by 64-bit integer atomics into a (lo, hi) pair per cluster, sizes
//                   beside them; per workgroup in LDS first where k allows (route_objective_acc).  Integer sums are exact: the result
//                   does not depend on the order of arrival, the shard layout or the form (the idiom of am_acc_k, avg_model.hip)
//   ob_finalize_k   (hi 2^32 + lo) q in double, after the all-reduce of the 3 k words
#include <cmath>

#include "common.h"

namespace {

constexpr int OT = 256;
constexpr int OW = OT / ISLE_WAVE;

__global__ __launch_bounds__(1024) void ob_cnorm_k(const float* __restrict__ C, uint64_t V, int k, int ld, double* __restrict__ cn) {
  __shared__ double sh[16][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int t = blockIdx.x * 64 + tx;
  double s = 0.0;
  if (t < k)
    for (uint64_t w = ty; w < V; w += 16) {
      const double x = (double)C[(size_t)w * ld + t];
      s += x * x;
    }
  sh[ty][tx] = s;
  __syncthreads();
  for (int o = 8; o > 0; o >>= 1) {
    if (ty < o) sh[ty][tx] += sh[ty + o][tx];
    __syncthreads();
  }
  if (ty == 0 && t < k) cn[t] = sh[0][tx];
}

__device__ inline double ob_wave_sum(double a) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off);  // both partners form the same sum: every lane ends with the same bits
  return a;
}

__global__ __launch_bounds__(OT) void ob_word_k(const float* __restrict__ vals, const uint32_t* __restrict__ rows, const int64_t* __restrict__ offs,
                                                 const uint32_t* __restrict__ assign, const uint32_t* __restrict__ order, uint64_t D,
                                                 const float* __restrict__ C, int ld, const double* __restrict__ cn, double* __restrict__ dd,
                                                 uint32_t* __restrict__ maxhi) {
  const int lane = threadIdx.x & 63;
  const uint64_t nw = (uint64_t)gridDim.x * OW;
  uint32_t mx = 0;
  for (uint64_t slot = (uint64_t)blockIdx.x * OW + (threadIdx.x >> 6); slot < D; slot += nw) {
    const uint64_t d = order ? (uint64_t)order[slot] : slot;
    const uint32_t t = assign[d];
    const int64_t s = offs[d], e = offs[d + 1];
    double a = 0.0;
    for (int64_t i = s + lane; i < e; i += 64) {
      const double v = (double)vals[i];
      const double cw = (double)C[(size_t)rows[i] * ld + t];
      a += fma(v, v, -2.0 * v * cw);  // v^2 and 2 v c are exact in fp64: one rounding per entry
    }
    a = ob_wave_sum(a) + cn[t];
    a = a > 0.0 ? a : 0.0;
    if (lane == 0) dd[d] = a;
    mx = max(mx, (uint32_t)__double2hiint(a));  // non-negative doubles: the order of the high words is the order of the values
  }
  if (lane == 0 && mx) atomicMax(maxhi, mx);
}

__global__ __launch_bounds__(OT) void ob_proj_k(const float* __restrict__ P, const uint32_t* __restrict__ assign, uint64_t D, int k, int ldk,
                                                 const float* __restrict__ C, double* __restrict__ dd, uint32_t* __restrict__ maxhi) {
  const int lane = threadIdx.x & 63;
  const uint64_t nw = (uint64_t)gridDim.x * OW;
  uint32_t mx = 0;
  for (uint64_t d = (uint64_t)blockIdx.x * OW + (threadIdx.x >> 6); d < D; d += nw) {
    const float* p = P + (size_t)d * ldk;
    const float* ct = C + (size_t)assign[d] * ldk;
    double a = 0.0;
    for (int j = lane; j < k; j += 64) {
      const double x = (double)p[j] - (double)ct[j];
      a += x * x;
    }
    a = ob_wave_sum(a);
    a = a > 0.0 ? a : 0.0;
    if (lane == 0) dd[d] = a;
    mx = max(mx, (uint32_t)__double2hiint(a));
  }
  if (lane == 0 && mx) atomicMax(maxhi, mx);
}

// q = 2^qe with qe = ex - 53, ex the exponent of the largest distance as frexp gives it (biased field - 1022); never below the smallest
// subnormal, whose multiples all doubles are
__device__ inline int ob_qe(uint32_t maxhi) { return max((int)((maxhi >> 20) & 0x7ffu) - 1075, -1074); }

template <bool LDS>
__global__ __launch_bounds__(OT) void ob_acc_k(const double* __restrict__ dd, const uint32_t* __restrict__ assign, uint64_t D, int k,
                                                const uint32_t* __restrict__ maxhi, unsigned long long* __restrict__ acc) {
  extern __shared__ unsigned long long ob_sh[];
  unsigned long long* A = LDS ? ob_sh : acc;
  if (LDS) {
    for (int i = threadIdx.x; i < 3 * k; i += OT) ob_sh[i] = 0ull;
    __syncthreads();
  }
  const int qe = ob_qe(*maxhi);
  for (uint64_t d = (uint64_t)blockIdx.x * OT + threadIdx.x; d < D; d += (uint64_t)gridDim.x * OT) {
    const unsigned long long qv = (unsigned long long)rint(ldexp(dd[d], -qe));  // an integer below 2^53
    const size_t t = assign[d];
    atomicAdd(&A[2 * t], qv & 0xffffffffull);
    if (qv >> 32) atomicAdd(&A[2 * t + 1], qv >> 32);
    atomicAdd(&A[2 * (size_t)k + t], 1ull);
  }
  if (LDS) {
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * k; i += OT)
      if (ob_sh[i]) atomicAdd(&acc[i], ob_sh[i]);
  }
}

__global__ void ob_finalize_k(const unsigned long long* __restrict__ acc, int k, const uint32_t* __restrict__ maxhi, double* __restrict__ sums) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= k) return;
  const unsigned long long lo = acc[2 * (size_t)t], hi = acc[2 * (size_t)t + 1] + (lo >> 32);  // the carry of the low halves' sum
  sums[t] = ldexp(ldexp((double)hi, 32) + (double)(lo & 0xffffffffull), ob_qe(*maxhi));
}

inline unsigned ob_grid(isle_ctx* c, uint64_t items, int per_block) {
  const uint64_t want = (items + per_block - 1) / per_block;
  return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(want, (uint64_t)c->num_cus * 32));
}

}  // namespace

#define LAUNCH_CHECK(c) HIPCHK(c, hipGetLastError())

int k_objective(isle_ctx* c, int space, int k, const uint32_t* assign, const float* centres, int ld, const uint32_t* order, int fam) {
  const uint64_t D = c->D, V = c->V;
  HIPCHK(c, c->ob_dd.reserve(D ? D : 1));
  HIPCHK(c, c->ob_cn.reserve(k));
  HIPCHK(c, c->ob_sums.reserve(k));
  HIPCHK(c, c->ob_acc.reserve(3 * (size_t)k + 1));
  unsigned long long* acc = c->ob_acc.p;
  uint32_t* maxhi = reinterpret_cast<uint32_t*>(acc + 3 * (size_t)k);
  HIPCHK(c, hipMemsetAsync(acc, 0, (3 * (size_t)k + 1) * sizeof(unsigned long long), c->stream));
  {
    TimeScope ts(c, fam);
    if (space == ISLE_SPACE_WORD) {
      hipLaunchKernelGGL(ob_cnorm_k, dim3(cdiv(k, 64)), dim3(1024), 0, c->stream, centres, V, k, ld, c->ob_cn.p);
      if (D)
        hipLaunchKernelGGL(ob_word_k, dim3(ob_grid(c, D, OW)), dim3(OT), 0, c->stream, c->vals.p, c->rows.p, c->offs.p, assign, order, D, centres, ld,
                           c->ob_cn.p, c->ob_dd.p, maxhi);
    } else if (D) {
      hipLaunchKernelGGL(ob_proj_k, dim3(ob_grid(c, D, OW)), dim3(OT), 0, c->stream, c->P.p, assign, D, k, ld, centres, c->ob_dd.p, maxhi);
    }
    LAUNCH_CHECK(c);
  }
  if (c->multi()) {
    TimeScope ts(c, ISLE_T_COMM);
    ISLECHK(isle_allreduce(c, maxhi, 1, ISLE_DT_U32, true));
  }
  if (D) {
    TimeScope ts(c, fam);
    const unsigned g = ob_grid(c, D, OT);
    if (route_objective_acc(k) == OBJ_ACC_LDS)
      hipLaunchKernelGGL(ob_acc_k<true>, dim3(g), dim3(OT), route_objective_lds_bytes(k), c->stream, c->ob_dd.p, assign, D, k, maxhi, acc);
    else
      hipLaunchKernelGGL(ob_acc_k<false>, dim3(g), dim3(OT), 0, c->stream, c->ob_dd.p, assign, D, k, maxhi, acc);
    LAUNCH_CHECK(c);
  }
  if (c->multi()) {
    TimeScope ts(c, ISLE_T_COMM);
    ISLECHK(isle_allreduce(c, acc, 3 * (size_t)k, ISLE_DT_U64));
  }
  {
    TimeScope ts(c, fam);
    hipLaunchKernelGGL(ob_finalize_k, dim3(cdiv(k, 256)), dim3(256), 0, c->stream, acc, k, maxhi, c->ob_sums.p);
    LAUNCH_CHECK(c);
  }
  return 0;
}
