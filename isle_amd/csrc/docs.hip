// isle_amd/csrc/docs.hip — the device steps of isle_hip_doc_lengths / isle_hip_doc_duplicates / isle_hip_prune_docs on the resident count
// matrix A (the rule: docs_host.h; the collectives, the refusals and the swap: api_stages.cpp).  Integer and bit-pattern work: every result
// is exact and independent of the visiting order.
//   docs_len_hash_k   words, tokens ((uint64)count summed in 64 bits) and the 64-bit hash of every document: a commutative sum of
//                     docs_entry_hash(row, count bits) over its entries, a per-document wave reduction like th_round_k's
//   docs_key_k        the sort's pairs: (the hash as the form cuts it, the document)
//   docs_head_flag_k  flag[p] = sorted position p opens a run of equal keys; the scan (scan.h) numbers the runs
//   docs_heads_k      every run's first document is its first head, and the first of its kind
//   docs_round_k      every unresolved document compares its content with its run's current head, the number of entries first, then rows
//                     and count bits: equal -> first_of = the head; else its sorted position competes (atomicMin) for the run's slot
//   docs_advance_k    the smallest unequal position of every run is the next head and the first of its kind.  The sort is stable, so
//                     documents ascend within a run and a head is always the smallest document of its content.
//   docs_keep_k       the rule's flags from the four bounds and first_of, and the counters kept / below / above / duplicate
//   docs_len_kept_k   the kept documents' lengths, for the 64-bit scan that gives the new offsets
//   docs_offsets_k    new_offs and kept_docs at the scanned new ids
//   docs_copy_k       the kept columns to the twin buffers, every store guarded by the total
// A document belongs to one wave wherever its entries are walked (hash pass, comparison, copy): its 64 lanes stride over the entries, so
// loads and stores are coalesced 4-byte accesses and no access leaves the document's own range (documents do not start 16-byte aligned:
// no wide loads).  No measurement stands behind that dealing (docs_host.h).  Index spaces are walked in 64 bits from grids of bounded size.
#include <algorithm>

#include "api_internal.h"  // StreamDrain
#include "docs_host.h"
#include "scan.h"

namespace {

constexpr int DT = 256;
constexpr int DW = DT / ISLE_WAVE;  // documents per workgroup and step where a document belongs to a wave
constexpr uint32_t DOCS_NONE = 0xffffffffu;

__device__ inline uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const uint32_t lo = __shfl_xor((uint32_t)v, o), hi = __shfl_xor((uint32_t)(v >> 32), o);
    v += ((uint64_t)hi << 32) | lo;
  }
  return v;
}

// document d's entries [s, e), clamped into the nnz entries there are
__device__ inline void doc_range(const int64_t* __restrict__ offs, uint64_t d, uint64_t nnz, uint64_t* s, uint64_t* e) {
  const uint64_t a = min((uint64_t)offs[d], nnz), b = min((uint64_t)offs[d + 1], nnz);
  *s = a;
  *e = max(a, b);
}

__global__ __launch_bounds__(DT) void docs_len_hash_k(const uint32_t* __restrict__ cnt_bits, const uint32_t* __restrict__ rows, const int64_t* __restrict__ offs,
                                                      uint64_t D, uint64_t nnz, uint32_t* __restrict__ words, uint64_t* __restrict__ tokens,
                                                      uint64_t* __restrict__ hash) {
  const int lane = threadIdx.x & 63;
  const uint64_t nw = (uint64_t)gridDim.x * DW;
  for (uint64_t d = (uint64_t)blockIdx.x * DW + (threadIdx.x >> 6); d < D; d += nw) {
    uint64_t s, e;
    doc_range(offs, d, nnz, &s, &e);
    uint64_t t = 0, h = 0;
    for (uint64_t i = s + lane; i < e; i += 64) {
      const uint32_t b = cnt_bits[i];
      t += (unsigned long long)__uint_as_float(b);
      h += docs_entry_hash(rows[i], b);
    }
    t = wave_sum_u64(t);
    h = wave_sum_u64(h);
    if (lane == 0) {
      words[d] = (uint32_t)(e - s);
      tokens[d] = t;
      if (hash) hash[d] = h;
    }
  }
}

__global__ __launch_bounds__(DT) void docs_key_k(uint64_t* __restrict__ key /*in: the hashes*/, uint32_t* __restrict__ val, uint64_t D, bool narrow) {
  const uint64_t stride = (uint64_t)gridDim.x * DT;
  for (uint64_t d = (uint64_t)blockIdx.x * DT + threadIdx.x; d < D; d += stride) {
    key[d] = docs_hash_cut(key[d], narrow);
    val[d] = (uint32_t)d;
  }
}

__global__ __launch_bounds__(DT) void docs_head_flag_k(const uint64_t* __restrict__ key, uint64_t D, uint32_t* __restrict__ flag) {
  const uint64_t stride = (uint64_t)gridDim.x * DT;
  for (uint64_t p = (uint64_t)blockIdx.x * DT + threadIdx.x; p < D; p += stride) flag[p] = (p == 0 || key[p] != key[p - 1]) ? 1u : 0u;
}

__global__ __launch_bounds__(DT) void docs_heads_k(const uint32_t* __restrict__ flag, const int64_t* __restrict__ run_of, const uint32_t* __restrict__ doc, uint64_t D,
                                                   uint64_t R, uint32_t* __restrict__ cur_head, uint32_t* __restrict__ first_of) {
  const uint64_t stride = (uint64_t)gridDim.x * DT;
  for (uint64_t p = (uint64_t)blockIdx.x * DT + threadIdx.x; p < D; p += stride) {
    if (!flag[p]) continue;
    const uint64_t r = (uint64_t)run_of[p];  // the exclusive scan of the flags: the heads before p
    const uint32_t d = doc[p];
    if (r < R && d < D) {
      cur_head[r] = (uint32_t)p;
      first_of[d] = d;
    }
  }
}

__global__ __launch_bounds__(DT) void docs_round_k(const uint32_t* __restrict__ cnt_bits, const uint32_t* __restrict__ rows, const int64_t* __restrict__ offs, uint64_t D,
                                                   uint64_t nnz, const uint32_t* __restrict__ words, const int64_t* __restrict__ run_of,
                                                   const uint32_t* __restrict__ doc, uint64_t R, const uint32_t* __restrict__ cur_head,
                                                   uint32_t* __restrict__ next_head, uint32_t* __restrict__ first_of, unsigned long long* __restrict__ unequal) {
  const int lane = threadIdx.x & 63;
  const uint64_t nw = (uint64_t)gridDim.x * DW;
  for (uint64_t p = (uint64_t)blockIdx.x * DW + (threadIdx.x >> 6); p < D; p += nw) {
    const uint32_t d = doc[p];
    if (d >= D || first_of[d] != DOCS_NONE) continue;  // (the same for the whole wave)
    const uint64_t r = (uint64_t)run_of[p] - 1;        // not a run's first position: the heads before p include its run's
    if (r >= R) continue;
    const uint32_t hp = cur_head[r];
    if (hp >= D) continue;
    const uint32_t hd = doc[hp];
    if (hd >= D) continue;
    bool equal = words[d] == words[hd];
    if (equal) {
      uint64_t s1, e1, s2, e2;
      doc_range(offs, d, nnz, &s1, &e1);
      doc_range(offs, hd, nnz, &s2, &e2);
      const uint64_t n = e1 - s1;
      equal = n == e2 - s2;  // (always where the lengths agree: the bound of both walks below)
      for (uint64_t base = 0; equal && base < n; base += 64) {
        const uint64_t i = base + lane;
        const bool differs = i < n && (rows[s1 + i] != rows[s2 + i] || cnt_bits[s1 + i] != cnt_bits[s2 + i]);
        if (__any(differs)) equal = false;
      }
    }
    if (lane == 0) {
      if (equal) {
        first_of[d] = hd;
      } else {
        atomicMin(&next_head[r], (uint32_t)p);
        atomicAdd(unequal, 1ull);
      }
    }
  }
}

__global__ __launch_bounds__(DT) void docs_advance_k(const uint32_t* __restrict__ doc, uint64_t D, uint64_t R, uint32_t* __restrict__ cur_head,
                                                     uint32_t* __restrict__ next_head, uint32_t* __restrict__ first_of, unsigned long long* __restrict__ heads) {
  const uint64_t stride = (uint64_t)gridDim.x * DT;
  for (uint64_t r = (uint64_t)blockIdx.x * DT + threadIdx.x; r < R; r += stride) {
    const uint32_t p = next_head[r];
    if (p == DOCS_NONE || p >= D) continue;
    const uint32_t d = doc[p];
    if (d >= D) continue;
    cur_head[r] = p;
    next_head[r] = DOCS_NONE;
    first_of[d] = d;
    atomicAdd(heads, 1ull);
  }
}

__global__ __launch_bounds__(DT) void docs_keep_k(const uint32_t* __restrict__ words, const uint64_t* __restrict__ tokens, uint64_t D, uint64_t min_words,
                                                  uint64_t max_words, uint64_t min_tokens, uint64_t max_tokens, bool dups, uint32_t* __restrict__ first_of,
                                                  uint32_t* __restrict__ keep, unsigned long long* __restrict__ out /*kept, below, above, duplicate*/) {
  __shared__ unsigned int sh[4];
  if (threadIdx.x < 4) sh[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t stride = (uint64_t)gridDim.x * DT;
  for (uint64_t d = (uint64_t)blockIdx.x * DT + threadIdx.x; d < D; d += stride) {
    const int fails = docs_fails(words[d], tokens[d], min_words, max_words, min_tokens, max_tokens);
    uint32_t first = dups ? first_of[d] : (uint32_t)d;
    int kind = 0;
    if (fails) kind = fails, first = DOCS_DROPPED;
    else if (first != d) kind = 3;
    first_of[d] = first;
    keep[d] = kind == 0 ? 1u : 0u;
    atomicAdd(&sh[kind], 1u);  // (a thread visits fewer than 2^32 documents, a workgroup's DT threads fewer than 2^32 together: D < 2^32)
  }
  __syncthreads();
  if (threadIdx.x < 4 && sh[threadIdx.x]) atomicAdd(&out[threadIdx.x], (unsigned long long)sh[threadIdx.x]);
}

__global__ __launch_bounds__(DT) void docs_len_kept_k(const uint32_t* __restrict__ keep, const uint32_t* __restrict__ words, uint64_t D, uint32_t* __restrict__ len) {
  const uint64_t stride = (uint64_t)gridDim.x * DT;
  for (uint64_t d = (uint64_t)blockIdx.x * DT + threadIdx.x; d < D; d += stride) len[d] = keep[d] ? words[d] : 0u;
}

__global__ __launch_bounds__(DT) void docs_offsets_k(const uint32_t* __restrict__ keep, const int64_t* __restrict__ new_id, const int64_t* __restrict__ at, uint64_t D,
                                                     uint64_t new_docs, uint64_t doc_offset, int64_t* __restrict__ new_offs, uint32_t* __restrict__ kept_docs) {
  const uint64_t stride = (uint64_t)gridDim.x * DT;
  for (uint64_t d = (uint64_t)blockIdx.x * DT + threadIdx.x; d <= D; d += stride) {
    if (d == D) {
      new_offs[new_docs] = at[D];  // the total
    } else if (keep[d]) {
      const uint64_t j = (uint64_t)new_id[d];
      if (j < new_docs) {  // (always: new_id is the scan of the same flags; the compare keeps the stores inside the buffers whatever it holds)
        new_offs[j] = at[d];
        kept_docs[j] = (uint32_t)(doc_offset + d);
      }
    }
  }
}

__global__ __launch_bounds__(DT) void docs_copy_k(const float* __restrict__ cnt, const uint32_t* __restrict__ rows, const int64_t* __restrict__ offs, uint64_t D,
                                                  uint64_t nnz, const uint32_t* __restrict__ keep, const int64_t* __restrict__ at, uint64_t total,
                                                  float* __restrict__ new_cnt, uint32_t* __restrict__ new_rows) {
  const int lane = threadIdx.x & 63;
  const uint64_t nw = (uint64_t)gridDim.x * DW;
  for (uint64_t d = (uint64_t)blockIdx.x * DW + (threadIdx.x >> 6); d < D; d += nw) {
    if (!keep[d]) continue;
    uint64_t s, e;
    doc_range(offs, d, nnz, &s, &e);
    const uint64_t o = (uint64_t)at[d];
    for (uint64_t i = s + lane; i < e; i += 64) {
      const uint64_t j = o + (i - s);
      if (j < total) {  // (always: at is the scan of the kept lengths)
        new_cnt[j] = cnt[i];
        new_rows[j] = rows[i];
      }
    }
  }
}

}  // namespace

#define LAUNCH_CHECK(c) HIPCHK(c, hipGetLastError())

// grid of a grid-stride walk over n items, `per` items per workgroup and step: enough workgroups to fill the device, never 2^32 threads
static unsigned docs_grid(const isle_ctx* c, uint64_t n, uint64_t per) {
  return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + per - 1) / per, (uint64_t)c->num_cus * 16));
}

int k_docs_len_hash(isle_ctx* c, uint32_t* words, uint64_t* tokens, uint64_t* hash) {
  TimeScope ts(c, ISLE_T_INGEST);
  const uint64_t D = c->a_D;
  if (!D) return 0;
  hipLaunchKernelGGL(docs_len_hash_k, dim3(docs_grid(c, D, DW)), dim3(DT), 0, c->stream, reinterpret_cast<const uint32_t*>(c->a_cnt.p), c->a_rows.p, c->a_offs.p, D,
                     c->a_nnz, words, tokens, hash);
  LAUNCH_CHECK(c);
  return 0;
}

int k_docs_first_of(isle_ctx* c, DocHash form, const uint32_t* words, uint64_t* hash, uint32_t* first_of, uint64_t* dups, uint64_t* rounds) {
  TimeScope ts(c, ISLE_T_INGEST);
  const uint64_t D = c->a_D, nnz = c->a_nnz;
  *dups = 0;
  *rounds = 0;
  if (!D) return 0;
  const bool narrow = form == DOC_FORM_NARROW;
  DevBuf<uint64_t> key_b;
  DevBuf<uint32_t> val_a, val_b, flag, cur_head, next_head;
  DevBuf<int64_t> run_of, scratch;
  DevBuf<unsigned long long> counters;
  StreamDrain drain(c);
  HIPCHK(c, key_b.reserve(D));
  HIPCHK(c, val_a.reserve(D));
  HIPCHK(c, val_b.reserve(D));
  HIPCHK(c, flag.reserve(D));
  HIPCHK(c, run_of.reserve(D + 1));
  HIPCHK(c, scratch.reserve(isle_scan_scratch(D) + 8));
  HIPCHK(c, counters.reserve(2));
  // ---- sorted by key: stable, so the documents ascend within a run
  hipLaunchKernelGGL(docs_key_k, dim3(docs_grid(c, D, DT)), dim3(DT), 0, c->stream, hash, val_a.p, D, narrow);
  LAUNCH_CHECK(c);
  bool in_a = true;
  ISLECHK(k_sort_pairs_u64(c, hash, val_a.p, key_b.p, val_b.p, D, docs_key_bits(narrow), &in_a));
  const uint64_t* key = in_a ? hash : key_b.p;
  const uint32_t* doc = in_a ? val_a.p : val_b.p;
  // ---- the runs numbered, their first documents the first heads
  hipLaunchKernelGGL(docs_head_flag_k, dim3(docs_grid(c, D, DT)), dim3(DT), 0, c->stream, key, D, flag.p);
  LAUNCH_CHECK(c);
  HIPCHK(c, (isle_scan::exclusive_scan<uint32_t, int64_t>(c->stream, flag.p, D, run_of.p, scratch.p)));
  int64_t runs = 0;
  HIPCHK(c, hipMemcpyAsync(&runs, run_of.p + D, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (runs < 1 || (uint64_t)runs > D) return isle_fail(c, ISLE_E_HIP, "doc_duplicates: the scan counts %lld runs of %llu documents", (long long)runs, (unsigned long long)D);
  const uint64_t R = (uint64_t)runs;
  HIPCHK(c, cur_head.reserve(R));
  HIPCHK(c, next_head.reserve(R));
  HIPCHK(c, hipMemsetAsync(first_of, 0xff, D * sizeof(uint32_t), c->stream));  // DOCS_NONE: unresolved
  HIPCHK(c, hipMemsetAsync(cur_head.p, 0xff, R * sizeof(uint32_t), c->stream));
  HIPCHK(c, hipMemsetAsync(next_head.p, 0xff, R * sizeof(uint32_t), c->stream));
  hipLaunchKernelGGL(docs_heads_k, dim3(docs_grid(c, D, DT)), dim3(DT), 0, c->stream, flag.p, run_of.p, doc, D, R, cur_head.p, first_of);
  LAUNCH_CHECK(c);
  // ---- rounds: every round resolves at least one document (the new head) of every run that still has unresolved ones
  uint64_t left = D - R, heads = R;
  while (left) {
    HIPCHK(c, hipMemsetAsync(counters.p, 0, 2 * sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(docs_round_k, dim3(docs_grid(c, D, DW)), dim3(DT), 0, c->stream, reinterpret_cast<const uint32_t*>(c->a_cnt.p), c->a_rows.p, c->a_offs.p, D, nnz,
                       words, run_of.p, doc, R, cur_head.p, next_head.p, first_of, counters.p);
    LAUNCH_CHECK(c);
    hipLaunchKernelGGL(docs_advance_k, dim3(docs_grid(c, R, DT)), dim3(DT), 0, c->stream, doc, D, R, cur_head.p, next_head.p, first_of, counters.p + 1);
    LAUNCH_CHECK(c);
    unsigned long long got[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(got, counters.p, sizeof(got), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    ++*rounds;
    if (got[0] > left || got[1] > got[0] || (got[0] && !got[1]))
      return isle_fail(c, ISLE_E_HIP, "doc_duplicates: round %llu leaves %llu of %llu documents unequal to their heads and makes %llu new heads",
                       (unsigned long long)*rounds, got[0], (unsigned long long)left, got[1]);
    heads += got[1];
    left = got[0] - got[1];
  }
  *dups = D - heads;
  return 0;
}

int k_docs_keep(isle_ctx* c, const uint32_t* words, const uint64_t* tokens, const uint64_t bounds[4], bool dups, uint32_t* first_of, uint32_t* keep,
                uint64_t dropped[3], uint64_t* kept) {
  TimeScope ts(c, ISLE_T_INGEST);
  const uint64_t D = c->a_D;
  dropped[0] = dropped[1] = dropped[2] = 0;
  *kept = 0;
  if (!D) return 0;
  DevBuf<unsigned long long> out;
  StreamDrain drain(c);
  HIPCHK(c, out.reserve(4));
  HIPCHK(c, hipMemsetAsync(out.p, 0, 4 * sizeof(unsigned long long), c->stream));
  hipLaunchKernelGGL(docs_keep_k, dim3(docs_grid(c, D, DT)), dim3(DT), 0, c->stream, words, tokens, D, bounds[0], bounds[1], bounds[2], bounds[3], dups, first_of, keep,
                     out.p);
  LAUNCH_CHECK(c);
  unsigned long long got[4] = {0, 0, 0, 0};
  HIPCHK(c, hipMemcpyAsync(got, out.p, sizeof(got), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (got[0] + got[1] + got[2] + got[3] != D)
    return isle_fail(c, ISLE_E_HIP, "prune_docs: %llu documents counted of %llu", got[0] + got[1] + got[2] + got[3], (unsigned long long)D);
  *kept = got[0];
  dropped[0] = got[1], dropped[1] = got[2], dropped[2] = got[3];
  return 0;
}

int k_docs_compact(isle_ctx* c, const uint32_t* keep, const uint32_t* words, uint64_t new_docs, DevBuf<float>& new_cnt, DevBuf<uint32_t>& new_rows,
                   DevBuf<int64_t>& new_offs, uint32_t* kept_docs, uint64_t* total) {
  TimeScope ts(c, ISLE_T_INGEST);
  const uint64_t D = c->a_D, nnz = c->a_nnz;
  DevBuf<uint32_t> len;
  DevBuf<int64_t> new_id, at, scratch;
  StreamDrain drain(c);
  HIPCHK(c, len.reserve(D ? D : 1));
  HIPCHK(c, new_id.reserve(D + 1));
  HIPCHK(c, at.reserve(D + 1));
  HIPCHK(c, scratch.reserve(isle_scan_scratch(D) + 8));
  if (D) hipLaunchKernelGGL(docs_len_kept_k, dim3(docs_grid(c, D, DT)), dim3(DT), 0, c->stream, keep, words, D, len.p);
  LAUNCH_CHECK(c);
  HIPCHK(c, (isle_scan::exclusive_scan<uint32_t, int64_t>(c->stream, keep, D, new_id.p, scratch.p)));
  HIPCHK(c, (isle_scan::exclusive_scan<uint32_t, int64_t>(c->stream, len.p, D, at.p, scratch.p)));
  int64_t got[2] = {0, 0};
  HIPCHK(c, hipMemcpyAsync(&got[0], new_id.p + D, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(&got[1], at.p + D, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if ((uint64_t)got[0] != new_docs || got[1] < 0 || (uint64_t)got[1] > nnz)
    return isle_fail(c, ISLE_E_HIP, "prune_docs: the scans count %lld kept documents (the flags: %llu) and %lld entries of %llu", (long long)got[0],
                     (unsigned long long)new_docs, (long long)got[1], (unsigned long long)nnz);
  const uint64_t m = (uint64_t)got[1];
  HIPCHK(c, new_cnt.reserve(m ? m : 1));
  HIPCHK(c, new_rows.reserve(m ? m : 1));
  HIPCHK(c, new_offs.reserve(new_docs + 1));
  hipLaunchKernelGGL(docs_offsets_k, dim3(docs_grid(c, D + 1, DT)), dim3(DT), 0, c->stream, keep, new_id.p, at.p, D, new_docs, c->a_doc_offset, new_offs.p, kept_docs);
  LAUNCH_CHECK(c);
  if (D && m)
    hipLaunchKernelGGL(docs_copy_k, dim3(docs_grid(c, D, DW)), dim3(DT), 0, c->stream, c->a_cnt.p, c->a_rows.p, c->a_offs.p, D, nnz, keep, at.p, m, new_cnt.p, new_rows.p);
  LAUNCH_CHECK(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *total = m;
  return 0;
}
