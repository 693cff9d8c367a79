// isle_amd/csrc/infer_resident.hip — document-topic inference on what is resident: documents [doc_begin, doc_end) of the count matrix A
// under a V x k column-major device model (the catch model, the average model, or a caller's model uploaded once), the weights returned
// as CSR entries above a threshold instead of the dense docs x k matrix (40 GB at 10 M documents, k = 1000).
//
// The iterations are infer.hip's: k_infer_rowok / k_infer_docs, the launches isle_hip_infer makes, on the resident buffers.  New here:
//   inf_pack_k     the model, column-major V x k -> row-major V x ld (ld = round4(k), padding columns exact zeros), the layout the
//                  iteration kernels read as float4: a 64 x 64 tiled transpose through LDS
//   inf_count_k    per document of a chunk, the number of topics above the threshold (one wave per document, ballot + popcount)
//   inf_write_k    the same ballots again, every entry placed at its document's offset + the popcount of the lanes before it
// with the 64-bit scan of scan.h between the two.  No atomics: the entries are in (document, topic) order and reproducible bit for bit.
// The five heaviest topics of every document stay resident beside the entries (c->inf_top_topic / inf_top_weight, under the same
// validity flag): infer_text.hip prints both from where they are.
// The documents go in chunks so that the device never holds more than ISLE_INFER_CHUNK_BYTES of dense weights; a document is computed
// by one workgroup from its own words alone, so the chunk size does not enter any result.
#include <algorithm>
#include <cstdint>
#include <vector>

#include "common.h"
#include "scan.h"

namespace {

// The dense weights of one chunk of documents stay within this budget: 1 GiB (chunk = budget / (4 k) documents by default).
constexpr uint64_t ISLE_INFER_CHUNK_BYTES = 1ull << 30;
// ... and a chunk is at most this many documents: the iteration kernels run one workgroup of 256 threads per document, and a launch of
// 2^32 threads or more does not run (common.h, the launch guard)
constexpr uint64_t ISLE_INFER_CHUNK_MAX_DOCS = 1ull << 22;

constexpr int PK = 64;  // tile edge: 64 words x 64 topics

// in: V x k column-major, out: V x ld row-major.  Block (bx, by) moves words [64 bx, +64) x topics [64 by, +64).
// Read: thread (tx = tid & 63, ty = tid >> 6) loads in[(t0 + ty + 4 i) V + w0 + tx], i < 16: a wave reads 256 contiguous bytes of one
// column.  LDS tile[topic][word] with rows of 65 floats: the write of a 32-lane half (ds_write_b32, 32 banks) has tx consecutive ->
// 32 different banks.  Write: a thread owns four consecutive topics (quad q) of one word and stores them as one float4; a 32-lane half
// holds quads q0 .. q0 + 7 of words wl .. wl + 3, whose LDS reads tile[4 q + j][wl] sit at dword 65 (4 q + j) + wl = 4 q + wl + j
// (mod 32): 4 q + wl runs through 0 .. 31, no two lanes of the half share a bank.  A wave stores 256 contiguous bytes of each of four rows.
__global__ __launch_bounds__(256) void inf_pack_k(const float* __restrict__ in, uint64_t V, int k, int ld, float* __restrict__ out) {
  __shared__ float tile[PK][PK + 1];
  const int tid = threadIdx.x;
  const uint64_t w0 = (uint64_t)blockIdx.x * PK;
  const int t0 = blockIdx.y * PK;
  {
    const int tx = tid & 63, ty = tid >> 6;
    const uint64_t w = w0 + tx;
#pragma unroll 4
    for (int i = 0; i < PK / 4; ++i) {
      const int tl = ty + 4 * i, t = t0 + tl;
      tile[tl][tx] = (w < V && t < k) ? in[(size_t)t * V + w] : 0.f;
    }
  }
  __syncthreads();
  const int lane = tid & 63, wave = tid >> 6;
  const int q = (lane & 7) | ((lane >> 5) << 3);  // quad of topics, 0 .. 15
  const int sub = (lane >> 3) & 3;
  const int t = t0 + 4 * q;
  if (t >= ld) return;  // ld is a multiple of 4: a quad lies inside the row or outside it
#pragma unroll
  for (int pass = 0; pass < 4; ++pass) {
    const int wl = 16 * pass + 4 * wave + sub;
    const uint64_t w = w0 + wl;
    if (w < V) {
      const float4 v = make_float4(tile[4 * q][wl], tile[4 * q + 1][wl], tile[4 * q + 2][wl], tile[4 * q + 3][wl]);
      *reinterpret_cast<float4*>(out + (size_t)w * ld + t) = v;  // 16-byte aligned: ld and t are multiples of 4
    }
  }
}

// bo[i] = offs[min(i chunk, R)], i <= nch: where the chunks' entries begin in A
__global__ __launch_bounds__(256) void inf_bounds_k(const int64_t* __restrict__ offs, uint64_t R, uint64_t chunk, uint64_t nch, int64_t* __restrict__ bo) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i <= nch) bo[i] = offs[i * chunk < R ? i * chunk : R];
}

// The rule of an entry: the document converged (llh.first != 0, as isle_hip_infer counts nconverged) and W[d, t] > min_weight, compared
// in float (NaN on either side: no entry).
__device__ inline bool inf_entry(bool good, float v, float minw) { return good && v > minw; }

__global__ __launch_bounds__(256) void inf_count_k(const float* __restrict__ W, const float* __restrict__ llh, uint64_t n, int k, float minw,
                                                    uint32_t* __restrict__ cnt) {
  const int lane = threadIdx.x & 63;
  const uint64_t d = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (d >= n) return;
  const bool good = llh[2 * d] != 0.0f;
  const float* row = W + (size_t)d * k;
  uint32_t c = 0;
  for (int t0 = 0; t0 < k; t0 += 64) {
    const int t = t0 + lane;
    const bool in = t < k && inf_entry(good, row[t < k ? t : 0], minw);
    c += (uint32_t)__popcll(__ballot(in));
  }
  if (lane == 0) cnt[d] = c;
}

// co: the exclusive scan of cnt over the chunk (n + 1 values); base: entries of the chunks before.  off: the call's offsets at this chunk.
__global__ __launch_bounds__(256) void inf_write_k(const float* __restrict__ W, const float* __restrict__ llh, uint64_t n, int k, float minw,
                                                    const int64_t* __restrict__ co, int64_t base, int64_t* __restrict__ off,
                                                    uint32_t* __restrict__ topic, float* __restrict__ weight) {
  const int lane = threadIdx.x & 63;
  const uint64_t d = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (d >= n) return;
  const bool good = llh[2 * d] != 0.0f;
  const float* row = W + (size_t)d * k;
  int64_t at = base + co[d];
  if (lane == 0) {
    off[d] = at;
    if (d + 1 == n) off[n] = base + co[n];
  }
  for (int t0 = 0; t0 < k; t0 += 64) {
    const int t = t0 + lane;
    const float v = row[t < k ? t : 0];
    const bool in = t < k && inf_entry(good, v, minw);
    const unsigned long long m = __ballot(in);
    if (in) {
      const int64_t p = at + __popcll(m & ((1ull << lane) - 1ull));
      topic[p] = (uint32_t)t;
      weight[p] = v;
    }
    at += __popcll(m);
  }
}

// capacity for `need` elements with the first `keep` preserved (DevBuf::reserve drops the contents)
template <class T>
int grow_keep(isle_ctx* c, DevBuf<T>& b, size_t keep, size_t need) {
  if (need <= b.cap) return 0;
  const size_t cap = std::max(need, 2 * b.cap);
  T* p = nullptr;
  HIPCHK(c, hipMalloc((void**)&p, cap * sizeof(T)));
  hipError_t e = hipSuccess;
  if (keep) e = hipMemcpyAsync(p, b.p, keep * sizeof(T), hipMemcpyDeviceToDevice, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) {
    (void)hipFree(p);
    HIPCHK(c, e);
  }
  if (b.p) (void)hipFree(b.p);
  b.p = p;
  b.cap = cap;
  return 0;
}

template <class T>
T* shifted(T* p, int64_t elems) {  // p - elems as an address: the kernels add positions >= elems back before they dereference
  return reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(p) - (uintptr_t)elems * sizeof(T));
}

}  // namespace

int k_inf_pack(isle_ctx* c, const float* model_cm_dev, uint64_t V, int k, float* out) {
  const int ld = (k + 3) & ~3;
  TimeScope ts(c, ISLE_T_INFER);
  hipLaunchKernelGGL(inf_pack_k, dim3((unsigned)((V + PK - 1) / PK), (unsigned)((ld + PK - 1) / PK)), dim3(256), 0, c->stream, model_cm_dev, V, k, ld, out);
  HIPCHK(c, hipGetLastError());
  return 0;
}

int k_infer_resident(isle_ctx* c, const float* model_cm_dev, int k, uint64_t doc_begin, uint64_t doc_end, int iters, float Lfguess,
                     float avg_doc_sz, float min_weight, uint64_t chunk_docs, int32_t* top_topic, float* top_weight, float* llh,
                     uint64_t* nconverged, uint64_t* nentries) {
  const uint64_t V = c->a_V, R = doc_end - doc_begin;
  const int ld = (k + 3) & ~3;
  const float minw = min_weight < 0.f ? 1.0f / (float)k : min_weight;
  uint64_t chunk = chunk_docs ? chunk_docs : std::max<uint64_t>(1, ISLE_INFER_CHUNK_BYTES / (sizeof(float) * (uint64_t)k));
  chunk = std::min(chunk, ISLE_INFER_CHUNK_MAX_DOCS);
  chunk = std::max<uint64_t>(1, std::min(chunk, R));
  const uint64_t nch = (R + chunk - 1) / chunk;
  c->res.inference_begins();

  DevBuf<float> dM, dfa, dW, dllh;
  DevBuf<uint32_t> dfw, dnk, dcnt;
  DevBuf<int64_t> dbo, dco, dblk;
  DevBuf<unsigned char> dok;
  DevBuf<unsigned int> dnc;
  HIPCHK(c, dM.reserve((size_t)V * ld));
  HIPCHK(c, dok.reserve(V));
  HIPCHK(c, dnc.reserve(1));
  HIPCHK(c, hipMemsetAsync(dnc.p, 0, sizeof(unsigned int), c->stream));
  {
    TimeScope ts(c, ISLE_T_INFER);
    hipLaunchKernelGGL(inf_pack_k, dim3((unsigned)((V + PK - 1) / PK), (unsigned)((ld + PK - 1) / PK)), dim3(256), 0, c->stream, model_cm_dev, V, k, ld,
                       dM.p);
    HIPCHK(c, hipGetLastError());
    ISLECHK(k_infer_rowok(c, dM.p, V, k, dok.p));
  }
  HIPCHK(c, c->inf_off.reserve(R + 1));
  int64_t running = 0;
  if (R == 0) {
    HIPCHK(c, hipMemsetAsync(c->inf_off.p, 0, sizeof(int64_t), c->stream));
  } else {
    // where the chunks' entries begin in A: sizes the compaction scratch of a chunk and places it
    std::vector<int64_t> bo(nch + 1);
    HIPCHK(c, dbo.reserve(nch + 1));
    hipLaunchKernelGGL(inf_bounds_k, dim3(cdiv((long)(nch + 1), 256)), dim3(256), 0, c->stream, c->a_offs.p + doc_begin, R, chunk, nch, dbo.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(bo.data(), dbo.p, (nch + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int64_t max_nnz = 1;
    for (uint64_t i = 0; i < nch; ++i) max_nnz = std::max(max_nnz, bo[i + 1] - bo[i]);
    HIPCHK(c, dfw.reserve((size_t)max_nnz));
    HIPCHK(c, dfa.reserve((size_t)max_nnz));
    HIPCHK(c, dnk.reserve(chunk));
    HIPCHK(c, dcnt.reserve(chunk));
    HIPCHK(c, dco.reserve(chunk + 1));
    HIPCHK(c, dblk.reserve(isle_scan::scan_scratch_elems(chunk)));
    HIPCHK(c, dW.reserve(chunk * (size_t)k));
    HIPCHK(c, c->inf_top_topic.reserve(5 * R));
    HIPCHK(c, c->inf_top_weight.reserve(5 * R));
    HIPCHK(c, dllh.reserve(2 * R));
    for (uint64_t i = 0; i < nch; ++i) {
      const uint64_t r0 = i * chunk, n = std::min(chunk, R - r0);
      const int64_t* offs = c->a_offs.p + doc_begin + r0;
      ISLECHK(k_infer_docs(c, dM.p, k, n, c->a_cnt.p, c->a_rows.p, offs, dok.p, shifted(dfw.p, bo[i]), shifted(dfa.p, bo[i]), dnk.p, iters, Lfguess,
                           avg_doc_sz, dW.p, c->inf_top_topic.p + 5 * r0, c->inf_top_weight.p + 5 * r0, dllh.p + 2 * r0, dnc.p));
      int64_t total = 0;
      {
        TimeScope ts(c, ISLE_T_INFER);
        hipLaunchKernelGGL(inf_count_k, dim3(cdiv((long)n, 4)), dim3(256), 0, c->stream, dW.p, dllh.p + 2 * r0, n, k, minw, dcnt.p);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, (isle_scan::exclusive_scan<uint32_t, int64_t>(c->stream, dcnt.p, n, dco.p, dblk.p)));
      }
      HIPCHK(c, hipMemcpyAsync(&total, dco.p + n, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
      const size_t need = (size_t)(running + total);
      ISLECHK(grow_keep(c, c->inf_topic, (size_t)running, std::max<size_t>(need, 1)));
      ISLECHK(grow_keep(c, c->inf_weight, (size_t)running, std::max<size_t>(need, 1)));
      {
        TimeScope ts(c, ISLE_T_INFER);
        hipLaunchKernelGGL(inf_write_k, dim3(cdiv((long)n, 4)), dim3(256), 0, c->stream, dW.p, dllh.p + 2 * r0, n, k, minw, dco.p, running,
                           c->inf_off.p + r0, c->inf_topic.p, c->inf_weight.p);
        HIPCHK(c, hipGetLastError());
      }
      running += total;
    }
  }
  unsigned int nc = 0;
  HIPCHK(c, hipMemcpyAsync(&nc, dnc.p, sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
  if (R) {
    if (top_topic) HIPCHK(c, hipMemcpyAsync(top_topic, c->inf_top_topic.p, 5 * R * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (top_weight) HIPCHK(c, hipMemcpyAsync(top_weight, c->inf_top_weight.p, 5 * R * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (llh) HIPCHK(c, hipMemcpyAsync(llh, dllh.p, 2 * R * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->inf_docs = R;
  c->inf_doc_begin = doc_begin;
  c->inf_n = (uint64_t)running;
  c->inf_cols = k;
  c->res.inference_done();
  if (nconverged) *nconverged = nc;
  if (nentries) *nentries = (uint64_t)running;
  return 0;
}
