// isle_amd/csrc/model_compare.hip — the device steps of isle_hip_compare_models / isle_hip_match_topics (the rule: match_host.h; the checks,
// the uploads and the fetches: api_stages.cpp).  Two V x k models, column-major fp32, give the ka x kb matrix of L1 distances of their
// columns in fp64; a matrix of doubles gives the greedy matching of its rows and columns.
//   mc_finite_k     bad[col] = the column holds a non-finite entry (a wave per column): the rule's NaN rows and columns are set from it, so
//                   that "any non-finite entry -> NaN" holds for inf too (a finite column against an inf column would sum to inf)
//   mc_dist_k       a workgroup owns MC_TILE x MC_TILE pairs and one word slice; a thread owns 4 x 4 pair sums in double.  The slice is
//                   walked in chunks of MC_CHUNK words: both models' chunk is read along the word axis (columns are contiguous there; 16
//                   bytes at once where the address allows, else guarded 4-byte loads: a column starts 16-byte aligned only where
//                   vocab % 4 == 0, and the tail of the slice is never read past), kept in registers while the chunk before is summed,
//                   and staged in LDS as [word][topic], rows padded to MC_TILE + 4 floats: a word's 4 consecutive topics are one
//                   16-byte read, 16 distinct ones per wave for the b side (256 contiguous bytes) and 4 for the a side.  A value is
//                   converted to double once per word and thread (8 conversions for 16 terms); a term is one v_add_f64 with a negated
//                   operand and one with the |x| modifier.  Words beyond the slice and topics beyond the model are staged as 0: |0 - 0|
//                   adds +0, which changes no sum.  Each thread adds its words in ascending order: the order of summation is a function
//                   of (V, ka, kb, slices) alone.
//   mc_reduce_k     the slices' partial matrices added in ascending slice order, the NaN rows and columns set
//   mc_init_k       match_a = match_b = -1, match_dist = NaN
//   mc_transpose_k  the matrix transposed once (tiles through LDS), so that the column step reads along rows too
//   mc_row_k        every free row's least free finite column, ties to the smaller j (a wave per row; lanes stride over the columns)
//   mc_col_k        every free column's least free finite row over ALL free rows, ties to the smaller i: the same walk on the transpose
//   mc_pair_k       a pair that chose each other is matched; one counter per round is read back
// Not the hot path of anything the benchmark runs.
#include <algorithm>
#include <climits>

#include "api_internal.h"  // StreamDrain
#include "match_host.h"

namespace {

constexpr int MT = 256;
constexpr int MC_LD = MC_TILE + 4;  // floats per staged word: rows stay 16-byte aligned, the stores of a quarter wave spread over 16 banks
constexpr int MC_Q = MC_CHUNK / 16;  // 16-byte loads per thread, side and chunk
static_assert(MC_TILE == 64 && MC_CHUNK % 16 == 0, "mc_dist_k deals 64 columns to 256 threads, four words to a load");

__global__ __launch_bounds__(MT) void mc_finite_k(const float* __restrict__ m, int k, uint64_t V, uint32_t* __restrict__ bad) {
  const int lane = threadIdx.x & 63;
  const int nw = gridDim.x * (MT / ISLE_WAVE);
  for (int col = blockIdx.x * (MT / ISLE_WAVE) + (threadIdx.x >> 6); col < k; col += nw) {
    const float* __restrict__ p = m + (uint64_t)col * V;
    bool b = false;
    for (uint64_t w = lane; w < V; w += 64) b |= !isfinite(p[w]);
    const bool any = __any(b);
    if (lane == 0) bad[col] = any ? 1u : 0u;
  }
}

// the thread's MC_Q loads of one side's chunk: column c0 + tid / 4, words w0 + 4 ((tid & 3) + 4 q) .. + 3
__device__ inline void mc_load(const float* __restrict__ m, int k, int c0, uint64_t V, uint64_t w0, uint64_t w_end, int tid, float4 (&r)[MC_Q]) {
  const int col = c0 + (tid >> 2);
#pragma unroll
  for (int q = 0; q < MC_Q; ++q) {
    const uint64_t w = w0 + 4 * (uint64_t)((tid & 3) + 4 * q);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (col < k && w < w_end) {
      const float* __restrict__ p = m + (uint64_t)col * V + w;
      if (w + 4 <= w_end && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        v = *reinterpret_cast<const float4*>(p);
      } else {
        v.x = p[0];
        if (w + 1 < w_end) v.y = p[1];
        if (w + 2 < w_end) v.z = p[2];
        if (w + 3 < w_end) v.w = p[3];
      }
    }
    r[q] = v;
  }
}
__device__ inline void mc_store(float (*s)[MC_LD], int tid, const float4 (&r)[MC_Q]) {
  const int col = tid >> 2;
#pragma unroll
  for (int q = 0; q < MC_Q; ++q) {
    const int w = 4 * ((tid & 3) + 4 * q);
    s[w + 0][col] = r[q].x;
    s[w + 1][col] = r[q].y;
    s[w + 2][col] = r[q].z;
    s[w + 3][col] = r[q].w;
  }
}

// out: the distances (one slice; bad_a / bad_b set the NaN rows and columns) or the slice's partial matrix at out + blockIdx.z * ka * kb
__global__ __launch_bounds__(MT) void mc_dist_k(const float* __restrict__ a, int ka, const float* __restrict__ b, int kb, uint64_t V, uint64_t slice_words,
                                                double* __restrict__ out, bool partial, const uint32_t* __restrict__ bad_a, const uint32_t* __restrict__ bad_b) {
  __shared__ __attribute__((aligned(16))) float sa[MC_CHUNK][MC_LD];
  __shared__ __attribute__((aligned(16))) float sb[MC_CHUNK][MC_LD];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int i0 = blockIdx.y * MC_TILE, j0 = blockIdx.x * MC_TILE;
  const uint64_t w_begin = min(V, (uint64_t)blockIdx.z * slice_words), w_end = min(V, w_begin + slice_words);
  double acc[4][4];
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[p][q] = 0.0;
  float4 ra[MC_Q], rb[MC_Q];
  if (w_begin < w_end) {
    mc_load(a, ka, i0, V, w_begin, w_end, tid, ra);
    mc_load(b, kb, j0, V, w_begin, w_end, tid, rb);
  }
  for (uint64_t w0 = w_begin; w0 < w_end; w0 += MC_CHUNK) {
    mc_store(sa, tid, ra);
    mc_store(sb, tid, rb);
    __syncthreads();
    if (w0 + MC_CHUNK < w_end) {  // the next chunk travels while this one is summed
      mc_load(a, ka, i0, V, w0 + MC_CHUNK, w_end, tid, ra);
      mc_load(b, kb, j0, V, w0 + MC_CHUNK, w_end, tid, rb);
    }
#pragma unroll 4
    for (int w = 0; w < MC_CHUNK; ++w) {
      const float4 fa = *reinterpret_cast<const float4*>(&sa[w][4 * ty]);
      const float4 fb = *reinterpret_cast<const float4*>(&sb[w][4 * tx]);
      const double da[4] = {(double)fa.x, (double)fa.y, (double)fa.z, (double)fa.w};
      const double db[4] = {(double)fb.x, (double)fb.y, (double)fb.z, (double)fb.w};
#pragma unroll
      for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[p][q] += fabs(da[p] - db[q]);
    }
    __syncthreads();
  }
  double* __restrict__ o = out + (partial ? (uint64_t)blockIdx.z * (uint64_t)ka * (uint64_t)kb : 0);
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int i = i0 + 4 * ty + p;
    if (i >= ka) continue;
    const bool bi = !partial && bad_a[i];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = j0 + 4 * tx + q;
      if (j < kb) o[(uint64_t)i * kb + j] = (bi || (!partial && bad_b[j])) ? __longlong_as_double(0x7ff8000000000000ll) : acc[p][q];
    }
  }
}

__global__ __launch_bounds__(MT) void mc_reduce_k(const double* __restrict__ part, uint32_t slices, int ka, int kb, const uint32_t* __restrict__ bad_a,
                                                  const uint32_t* __restrict__ bad_b, double* __restrict__ dist) {
  const uint64_t n = (uint64_t)ka * kb, stride = (uint64_t)gridDim.x * MT;
  for (uint64_t e = (uint64_t)blockIdx.x * MT + threadIdx.x; e < n; e += stride) {
    double s = part[e];
    for (uint32_t t = 1; t < slices; ++t) s += part[(uint64_t)t * n + e];
    dist[e] = (bad_a[e / kb] || bad_b[e % kb]) ? __longlong_as_double(0x7ff8000000000000ll) : s;
  }
}

__global__ __launch_bounds__(MT) void mc_init_k(int32_t* __restrict__ match_a, int na, int32_t* __restrict__ match_b, int nb, double* __restrict__ match_dist) {
  const int stride = gridDim.x * MT;
  for (int i = blockIdx.x * MT + threadIdx.x; i < max(na, nb); i += stride) {
    if (i < na) match_a[i] = -1, match_dist[i] = __longlong_as_double(0x7ff8000000000000ll);
    if (i < nb) match_b[i] = -1;
  }
}

// t (nb x na) = d (na x nb) transposed: 32 x 32 tiles, grid (ceil(nb / 32), ceil(na / 32))
__global__ __launch_bounds__(MT) void mc_transpose_k(const double* __restrict__ d, int na, int nb, double* __restrict__ t) {
  __shared__ double tile[32][33];
  const int x = threadIdx.x & 31, y = threadIdx.x >> 5;
  const int i0 = blockIdx.y * 32, j0 = blockIdx.x * 32;
  for (int r = y; r < 32; r += 8)
    if (i0 + r < na && j0 + x < nb) tile[r][x] = d[(uint64_t)(i0 + r) * nb + j0 + x];
  __syncthreads();
  for (int r = y; r < 32; r += 8)
    if (j0 + r < nb && i0 + x < na) t[(uint64_t)(j0 + r) * na + i0 + x] = tile[x][r];
}

// best[r] = the least free finite entry of row r of d (n x m), ties to the smaller index; -1 where r is matched or has none
__device__ inline void mc_best(const double* __restrict__ d, int n, int m, const int32_t* __restrict__ self_match, const int32_t* __restrict__ other_match,
                               int32_t* __restrict__ best) {
  const int lane = threadIdx.x & 63;
  const int nw = gridDim.x * (MT / ISLE_WAVE);
  for (int r = blockIdx.x * (MT / ISLE_WAVE) + (threadIdx.x >> 6); r < n; r += nw) {
    if (self_match[r] >= 0) {  // (the same for the whole wave)
      if (lane == 0) best[r] = -1;
      continue;
    }
    const double* __restrict__ row = d + (uint64_t)r * m;
    double bd = 0.0;
    int bj = INT_MAX;
    for (int j = lane; j < m; j += 64) {
      const double v = row[j];
      if (other_match[j] < 0 && isfinite(v) && (bj == INT_MAX || v < bd)) bd = v, bj = j;  // ascending j: < keeps the smaller one of a tie
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const double od = __shfl_xor(bd, o);
      const int oj = __shfl_xor(bj, o);
      if (oj != INT_MAX && (bj == INT_MAX || od < bd || (od == bd && oj < bj))) bd = od, bj = oj;
    }
    if (lane == 0) best[r] = bj == INT_MAX ? -1 : bj;
  }
}
__global__ __launch_bounds__(MT) void mc_row_k(const double* __restrict__ d, int na, int nb, const int32_t* __restrict__ match_a, const int32_t* __restrict__ match_b,
                                               int32_t* __restrict__ row_best) {
  mc_best(d, na, nb, match_a, match_b, row_best);
}
__global__ __launch_bounds__(MT) void mc_col_k(const double* __restrict__ dt, int na, int nb, const int32_t* __restrict__ match_a, const int32_t* __restrict__ match_b,
                                               int32_t* __restrict__ col_best) {
  mc_best(dt, nb, na, match_b, match_a, col_best);
}

__global__ __launch_bounds__(MT) void mc_pair_k(const double* __restrict__ d, int na, int nb, const int32_t* __restrict__ row_best, const int32_t* __restrict__ col_best,
                                                int32_t* __restrict__ match_a, int32_t* __restrict__ match_b, double* __restrict__ match_dist,
                                                unsigned int* __restrict__ matched) {
  const int stride = gridDim.x * MT;
  for (int i = blockIdx.x * MT + threadIdx.x; i < na; i += stride) {
    const int j = row_best[i];
    if (j < 0 || j >= nb || col_best[j] != i) continue;  // (a column chose one row: no two rows write one j)
    match_a[i] = j;
    match_b[j] = i;
    match_dist[i] = d[(uint64_t)i * nb + j];
    atomicAdd(matched, 1u);
  }
}

}  // namespace

#define LAUNCH_CHECK(c) HIPCHK(c, hipGetLastError())

static unsigned mc_grid(const isle_ctx* c, uint64_t n, uint64_t per) {
  return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + per - 1) / per, (uint64_t)c->num_cus * 16));
}

int k_mc_dist(isle_ctx* c, const float* a, int ka, const float* b, int kb, uint64_t V, uint32_t slices, double* dist) {
  TimeScope ts(c, ISLE_T_POST);
  DevBuf<uint32_t> bad;
  DevBuf<double> part;
  StreamDrain drain(c);
  HIPCHK(c, bad.reserve((size_t)ka + kb));
  uint32_t *bad_a = bad.p, *bad_b = bad.p + ka;
  hipLaunchKernelGGL(mc_finite_k, dim3(mc_grid(c, ka, MT / ISLE_WAVE)), dim3(MT), 0, c->stream, a, ka, V, bad_a);
  LAUNCH_CHECK(c);
  hipLaunchKernelGGL(mc_finite_k, dim3(mc_grid(c, kb, MT / ISLE_WAVE)), dim3(MT), 0, c->stream, b, kb, V, bad_b);
  LAUNCH_CHECK(c);
  const uint64_t chunks = (V + MC_CHUNK - 1) / MC_CHUNK;
  slices = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(slices, chunks));
  const uint64_t per = mc_slice_words(V, slices);
  const dim3 grid((kb + MC_TILE - 1) / MC_TILE, (ka + MC_TILE - 1) / MC_TILE, slices);
  if (slices == 1) {
    hipLaunchKernelGGL(mc_dist_k, grid, dim3(MT), 0, c->stream, a, ka, b, kb, V, per, dist, false, bad_a, bad_b);
    LAUNCH_CHECK(c);
    return 0;
  }
  const uint64_t n = (uint64_t)ka * kb;
  HIPCHK(c, part.reserve((size_t)(n * slices)));
  hipLaunchKernelGGL(mc_dist_k, grid, dim3(MT), 0, c->stream, a, ka, b, kb, V, per, part.p, true, bad_a, bad_b);
  LAUNCH_CHECK(c);
  hipLaunchKernelGGL(mc_reduce_k, dim3(mc_grid(c, n, MT)), dim3(MT), 0, c->stream, part.p, slices, ka, kb, bad_a, bad_b, dist);
  LAUNCH_CHECK(c);
  return 0;
}

int k_mc_match(isle_ctx* c, const double* dist, int na, int nb, int32_t* match_a, int32_t* match_b, double* match_dist, uint64_t* n_matched, uint32_t* rounds) {
  TimeScope ts(c, ISLE_T_POST);
  *n_matched = 0;
  *rounds = 0;
  DevBuf<double> dt;
  DevBuf<int32_t> best;
  DevBuf<unsigned int> counter;
  StreamDrain drain(c);
  HIPCHK(c, dt.reserve((size_t)na * nb));
  HIPCHK(c, best.reserve((size_t)na + nb));
  HIPCHK(c, counter.reserve(1));
  int32_t *row_best = best.p, *col_best = best.p + na;
  hipLaunchKernelGGL(mc_init_k, dim3(mc_grid(c, std::max(na, nb), MT)), dim3(MT), 0, c->stream, match_a, na, match_b, nb, match_dist);
  LAUNCH_CHECK(c);
  hipLaunchKernelGGL(mc_transpose_k, dim3((nb + 31) / 32, (na + 31) / 32), dim3(MT), 0, c->stream, dist, na, nb, dt.p);
  LAUNCH_CHECK(c);
  const uint64_t most = (uint64_t)std::min(na, nb);
  uint64_t matched = 0;
  while (matched < most) {
    HIPCHK(c, hipMemsetAsync(counter.p, 0, sizeof(unsigned int), c->stream));
    hipLaunchKernelGGL(mc_row_k, dim3(mc_grid(c, na, MT / ISLE_WAVE)), dim3(MT), 0, c->stream, dist, na, nb, match_a, match_b, row_best);
    LAUNCH_CHECK(c);
    hipLaunchKernelGGL(mc_col_k, dim3(mc_grid(c, nb, MT / ISLE_WAVE)), dim3(MT), 0, c->stream, dt.p, na, nb, match_a, match_b, col_best);
    LAUNCH_CHECK(c);
    hipLaunchKernelGGL(mc_pair_k, dim3(mc_grid(c, na, MT)), dim3(MT), 0, c->stream, dist, na, nb, row_best, col_best, match_a, match_b, match_dist, counter.p);
    LAUNCH_CHECK(c);
    unsigned int got = 0;
    HIPCHK(c, hipMemcpyAsync(&got, counter.p, sizeof(got), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (got > most - matched)
      return isle_fail(c, ISLE_E_HIP, "match_topics: a round matches %u pairs where %llu are left", got, (unsigned long long)(most - matched));
    if (!got) break;  // no edge between two free sides is left
    matched += got;
    ++*rounds;
  }
  *n_matched = matched;
  return 0;
}
