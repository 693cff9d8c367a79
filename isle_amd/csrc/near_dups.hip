// isle_amd/csrc/near_dups.hip — the device steps of isle_hip_doc_signatures / isle_hip_doc_jaccard / isle_hip_doc_near_duplicates /
// isle_hip_prune_near_docs on the resident count matrix A (the rule: neardup_host.h; the refusals and the swap: api_stages.cpp; the
// compaction: docs.hip's k_docs_compact).  Integer work only: every result is exact and independent of the visiting order, two calls give
// the same bits.
//   nd_sig_k        MinHash signatures and band keys.  A document belongs to a wave; lane i owns hash function i (and i + 64 where
//                   H > 64).  The wave loads 64 row ids with one coalesced load and hands them round lane by lane (a shuffle from a
//                   wave-uniform lane), every lane folds nd_hash(i, row) into its running minimum: no reduction across lanes, all lanes
//                   busy however short the document.  Signatures go out coalesced (sig[d H + lane]) only when asked for; the band keys are
//                   folded by lane b from the rows_per_band neighbouring lanes' minima (shuffles) and stored band-major, so that a band's
//                   sort reads one contiguous array and the prune never holds D H signatures in memory.
//   nd_live_flag_k  flag[d] = d is live (parent[d] == d); the 64-bit scan (scan.h) gives its place in the ascending live list
//   nd_live_k       the sort's pairs of the live documents: (key[b][d] as the form cuts it, d)
//   nd_head_flag_k / nd_heads_k   the runs of equal sorted keys numbered by the scan; a run's first document is its first leader
//   nd_round_k      docs_round_k's scheme with similar in the place of equal: every unresolved document is tested against its run's current
//                   leader.  The length filter first (no content read); then the wave's lanes stride over the SHORTER document's rows and
//                   search each by bisection in the LONGER document's ascending rows, inter is a wave sum, the test is in 64-bit integers.
//                   similar -> parent = the leader; else its sorted position competes (atomicMin) to be the run's next leader.
//   nd_advance_k    the smallest dissimilar position of every run is the next leader.  The sort is stable, so documents ascend within a
//                   run and the leaders appear in the order the rule's sequential clustering makes them.
//   nd_roots_k      pointer jumping over parent until a pass changes nothing: first_of = the root
//   nd_keep_k       keep[d] = first_of[d] == d, and the number kept
//   nd_jaccard_k    the same intersection for the caller's pairs: a wave per pair
// Every round has a counter pair of its own; the pairs of ND_BATCH rounds are read back together (one synchronisation per batch, not per
// round), and pairs_tested is summed on the host in 64 bits from the rounds' unresolved counts.
// Measured on the config-2 corpus (tools/near_dups_probe.py, 2 600 rounds): 165 ms of device time against 229 ms with a read-back per round.
// Bisection per row was chosen for the intersection (no state carried between lanes, a lane's accesses stay inside the longer document's
// range by construction); a wave-cooperative merge was NOT measured.  The alternative dealing of the signature pass (a lane per entry, H
// minima in registers or LDS, a reduction across lanes per hash) was NOT measured either.
// Compiler's report for gfx950 (hipcc -O3 -Rpass-analysis=kernel-resource-usage); no kernel of this file uses scratch (LDS: nd_keep_k's one counter):
//   nd_sig_k<false>  VGPRs 32, SGPRs 46, scratch 0 bytes, occupancy 8 waves/SIMD
//   nd_sig_k<true>   VGPRs 40, SGPRs 49, scratch 0 bytes, occupancy 8 waves/SIMD
//   nd_round_k       VGPRs 36, SGPRs 60, scratch 0 bytes, occupancy 8 waves/SIMD
//   nd_jaccard_k     VGPRs 29, SGPRs 46, scratch 0 bytes, occupancy 8 waves/SIMD
#include <algorithm>

#include "api_internal.h"  // StreamDrain
#include "neardup_host.h"
#include "scan.h"

namespace {

constexpr int NT = 256;
constexpr int NW = NT / ISLE_WAVE;  // documents per workgroup and step where a document belongs to a wave
constexpr uint32_t ND_NONE = 0xffffffffu;
constexpr int ND_BATCH = 8;  // rounds queued per read-back of their counters (k_nd_resolve)

__device__ inline uint64_t shfl_u64(uint64_t v, int src) {
  const uint32_t lo = __shfl((uint32_t)v, src), hi = __shfl((uint32_t)(v >> 32), src);
  return ((uint64_t)hi << 32) | lo;
}
__device__ inline uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// document d's entries [s, e), clamped into the nnz entries there are
__device__ inline void nd_range(const int64_t* __restrict__ offs, uint64_t d, uint64_t nnz, uint64_t* s, uint64_t* e) {
  const uint64_t a = min((uint64_t)offs[d], nnz), b = min((uint64_t)offs[d + 1], nnz);
  *s = a;
  *e = max(a, b);
}

template <bool TWO>  // TWO: H > 64, a lane owns hash functions lane and lane + 64
__global__ __launch_bounds__(NT) void nd_sig_k(const uint32_t* __restrict__ rows, const int64_t* __restrict__ offs, uint64_t D, uint64_t nnz, int H, int bands,
                                               int rows_per_band, uint64_t* __restrict__ sig, uint64_t* __restrict__ keys) {
  const int lane = threadIdx.x & 63;
  const uint64_t nw = (uint64_t)gridDim.x * NW;
  for (uint64_t d = (uint64_t)blockIdx.x * NW + (threadIdx.x >> 6); d < D; d += nw) {
    uint64_t s, e;
    nd_range(offs, d, nnz, &s, &e);
    uint64_t m0 = ND_EMPTY_SIG, m1 = ND_EMPTY_SIG;
    for (uint64_t base = s; base < e; base += 64) {
      const uint64_t i = base + lane;
      const uint32_t mine = i < e ? rows[i] : 0u;
      const int cnt = (int)min((uint64_t)64, e - base);  // (the same for the whole wave)
      for (int j = 0; j < cnt; ++j) {
        const uint32_t r = __shfl(mine, j);
        m0 = min(m0, nd_hash((uint32_t)lane, r));
        if (TWO) m1 = min(m1, nd_hash((uint32_t)lane + 64u, r));
      }
    }
    if (sig) {
      if (lane < H) sig[d * (uint64_t)H + lane] = m0;
      if (TWO && lane + 64 < H) sig[d * (uint64_t)H + 64 + lane] = m1;
    }
    if (keys) {  // lane b folds band b: signature h = b rows_per_band + j lies in lane h & 63, in m1 where h >= 64
      uint64_t k = 0;
      for (int j = 0; j < rows_per_band; ++j) {
        const int h = lane * rows_per_band + j;  // (every lane shuffles; the lanes >= bands fold values nobody stores)
        const uint64_t v0 = shfl_u64(m0, h & 63);
        const uint64_t v1 = TWO ? shfl_u64(m1, h & 63) : v0;
        k = nd_key_step(k, (h & 64) ? v1 : v0);
      }
      if (lane < bands) keys[(uint64_t)lane * D + d] = k;
    }
  }
}

// |S_a ∩ S_b| by the whole wave: [s1, e1) the shorter document's entries, [s2, e2) the longer one's
__device__ inline uint32_t nd_inter_wave(const uint32_t* __restrict__ rows, uint64_t s1, uint64_t e1, uint64_t s2, uint64_t e2, int lane) {
  uint32_t hit = 0;
  for (uint64_t i = s1 + lane; i < e1; i += 64) {
    const uint32_t r = rows[i];
    uint64_t lo = s2, hi = e2;
    while (lo < hi) {  // s2 <= lo <= mid < hi <= e2: no access leaves the longer document
      const uint64_t mid = lo + ((hi - lo) >> 1);
      if (rows[mid] < r) lo = mid + 1;
      else hi = mid;
    }
    hit += (lo < e2 && rows[lo] == r) ? 1u : 0u;
  }
  return wave_sum_u32(hit);
}
__device__ inline uint32_t nd_inter_docs(const uint32_t* __restrict__ rows, const int64_t* __restrict__ offs, uint64_t nnz, uint32_t a, uint32_t b, int lane,
                                         uint64_t* na, uint64_t* nb) {
  uint64_t s1, e1, s2, e2;
  nd_range(offs, a, nnz, &s1, &e1);
  nd_range(offs, b, nnz, &s2, &e2);
  *na = e1 - s1;
  *nb = e2 - s2;
  return *na <= *nb ? nd_inter_wave(rows, s1, e1, s2, e2, lane) : nd_inter_wave(rows, s2, e2, s1, e1, lane);
}

__global__ __launch_bounds__(NT) void nd_iota_k(uint32_t* __restrict__ parent, uint64_t D) {
  const uint64_t stride = (uint64_t)gridDim.x * NT;
  for (uint64_t d = (uint64_t)blockIdx.x * NT + threadIdx.x; d < D; d += stride) parent[d] = (uint32_t)d;
}

__global__ __launch_bounds__(NT) void nd_live_flag_k(const uint32_t* __restrict__ parent, uint64_t D, uint32_t* __restrict__ flag) {
  const uint64_t stride = (uint64_t)gridDim.x * NT;
  for (uint64_t d = (uint64_t)blockIdx.x * NT + threadIdx.x; d < D; d += stride) flag[d] = parent[d] == d ? 1u : 0u;
}

__global__ __launch_bounds__(NT) void nd_live_k(const uint32_t* __restrict__ flag, const int64_t* __restrict__ place, const uint64_t* __restrict__ band_keys, uint64_t D,
                                                uint64_t n, bool narrow, uint64_t* __restrict__ key, uint32_t* __restrict__ val) {
  const uint64_t stride = (uint64_t)gridDim.x * NT;
  for (uint64_t d = (uint64_t)blockIdx.x * NT + threadIdx.x; d < D; d += stride) {
    if (!flag[d]) continue;
    const uint64_t p = (uint64_t)place[d];
    if (p < n) {  // (always: n is the number of live documents, place the scan of their flags)
      key[p] = docs_hash_cut(band_keys[d], narrow);
      val[p] = (uint32_t)d;
    }
  }
}

__global__ __launch_bounds__(NT) void nd_head_flag_k(const uint64_t* __restrict__ key, uint64_t n, uint32_t* __restrict__ flag) {
  const uint64_t stride = (uint64_t)gridDim.x * NT;
  for (uint64_t p = (uint64_t)blockIdx.x * NT + threadIdx.x; p < n; p += stride) flag[p] = (p == 0 || key[p] != key[p - 1]) ? 1u : 0u;
}

__global__ __launch_bounds__(NT) void nd_heads_k(const uint32_t* __restrict__ flag, const int64_t* __restrict__ run_of, uint64_t n, uint64_t R,
                                                 uint32_t* __restrict__ cur_head, uint32_t* __restrict__ done) {
  const uint64_t stride = (uint64_t)gridDim.x * NT;
  for (uint64_t p = (uint64_t)blockIdx.x * NT + threadIdx.x; p < n; p += stride) {
    const uint64_t r = (uint64_t)run_of[p];  // the exclusive scan of the flags: the heads before p
    const bool head = flag[p] && r < R;
    if (head) cur_head[r] = (uint32_t)p;
    done[p] = head ? 1u : 0u;
  }
}

__global__ __launch_bounds__(NT) void nd_round_k(const uint32_t* __restrict__ rows, const int64_t* __restrict__ offs, uint64_t D, uint64_t nnz, uint64_t n,
                                                 const int64_t* __restrict__ run_of, const uint32_t* __restrict__ doc, uint64_t R,
                                                 const uint32_t* __restrict__ cur_head, uint32_t* __restrict__ next_head, uint32_t* __restrict__ done,
                                                 uint32_t* __restrict__ parent, uint64_t num, uint64_t den, unsigned long long* __restrict__ dissimilar) {
  const int lane = threadIdx.x & 63;
  const uint64_t nw = (uint64_t)gridDim.x * NW;
  for (uint64_t p = (uint64_t)blockIdx.x * NW + (threadIdx.x >> 6); p < n; p += nw) {
    if (done[p]) continue;  // (the same for the whole wave)
    const uint32_t d = doc[p];
    const uint64_t r = (uint64_t)run_of[p] - 1;  // not a run's first position: the heads before p include its run's
    if (d >= D || r >= R) continue;
    const uint32_t hp = cur_head[r];
    if (hp >= n) continue;
    const uint32_t hd = doc[hp];
    if (hd >= D) continue;
    uint64_t s1, e1, s2, e2;
    nd_range(offs, d, nnz, &s1, &e1);
    nd_range(offs, hd, nnz, &s2, &e2);
    bool sim = nd_lengths_allow(e1 - s1, e2 - s2, num, den);  // the length filter: no content is read where it decides
    if (sim) {
      uint64_t a_n, b_n;
      const uint32_t inter = nd_inter_docs(rows, offs, nnz, d, hd, lane, &a_n, &b_n);
      sim = nd_similar(inter, a_n, b_n, num, den);
    }
    if (lane == 0) {
      if (sim) {
        parent[d] = hd;
        done[p] = 1u;
      } else {
        atomicMin(&next_head[r], (uint32_t)p);
        atomicAdd(dissimilar, 1ull);
      }
    }
  }
}

__global__ __launch_bounds__(NT) void nd_advance_k(uint64_t n, uint64_t R, uint32_t* __restrict__ cur_head, uint32_t* __restrict__ next_head, uint32_t* __restrict__ done,
                                                   unsigned long long* __restrict__ heads) {
  const uint64_t stride = (uint64_t)gridDim.x * NT;
  for (uint64_t r = (uint64_t)blockIdx.x * NT + threadIdx.x; r < R; r += stride) {
    const uint32_t p = next_head[r];
    if (p == ND_NONE || p >= n) continue;
    cur_head[r] = p;
    next_head[r] = ND_NONE;
    done[p] = 1u;
    atomicAdd(heads, 1ull);
  }
}

// one pass of pointer jumping; the racing reads see a value of this pass or of the one before, both on the document's own chain
__global__ __launch_bounds__(NT) void nd_roots_k(uint32_t* __restrict__ first_of, uint64_t D, unsigned long long* __restrict__ changed) {
  const uint64_t stride = (uint64_t)gridDim.x * NT;
  for (uint64_t d = (uint64_t)blockIdx.x * NT + threadIdx.x; d < D; d += stride) {
    const uint32_t f = first_of[d];
    if (f >= D) continue;
    const uint32_t g = first_of[f];
    if (g != f && g < D) {
      first_of[d] = g;
      atomicAdd(changed, 1ull);
    }
  }
}

__global__ __launch_bounds__(NT) void nd_keep_k(const uint32_t* __restrict__ first_of, uint64_t D, uint32_t* __restrict__ keep, unsigned long long* __restrict__ kept) {
  __shared__ unsigned int sh;
  if (threadIdx.x == 0) sh = 0;
  __syncthreads();
  const uint64_t stride = (uint64_t)gridDim.x * NT;
  for (uint64_t d = (uint64_t)blockIdx.x * NT + threadIdx.x; d < D; d += stride) {
    const bool k = first_of[d] == d;
    keep[d] = k ? 1u : 0u;
    if (k) atomicAdd(&sh, 1u);  // (a workgroup visits fewer than 2^32 documents: D < 2^32)
  }
  __syncthreads();
  if (threadIdx.x == 0 && sh) atomicAdd(kept, (unsigned long long)sh);
}

__global__ __launch_bounds__(NT) void nd_jaccard_k(const uint32_t* __restrict__ rows, const int64_t* __restrict__ offs, uint64_t D, uint64_t nnz, uint64_t n_pairs,
                                                   const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint32_t* __restrict__ inter,
                                                   uint32_t* __restrict__ uni) {
  const int lane = threadIdx.x & 63;
  const uint64_t nw = (uint64_t)gridDim.x * NW;
  for (uint64_t i = (uint64_t)blockIdx.x * NW + (threadIdx.x >> 6); i < n_pairs; i += nw) {
    const uint32_t x = a[i], y = b[i];
    if (x >= D || y >= D) continue;  // (never: the host refuses such a pair before the launch)
    uint64_t na, nb;
    const uint32_t got = nd_inter_docs(rows, offs, nnz, x, y, lane, &na, &nb);
    if (lane == 0) {
      inter[i] = got;
      uni[i] = (uint32_t)(na + nb - got);
    }
  }
}

}  // namespace

#define LAUNCH_CHECK(c) HIPCHK(c, hipGetLastError())

// grid of a grid-stride walk over n items, `per` items per workgroup and step: enough workgroups to fill the device, never 2^32 threads
static unsigned nd_grid(const isle_ctx* c, uint64_t n, uint64_t per) {
  return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + per - 1) / per, (uint64_t)c->num_cus * 16));
}

int k_nd_signatures(isle_ctx* c, int bands, int rows_per_band, uint64_t* sig, uint64_t* keys) {
  TimeScope ts(c, ISLE_T_INGEST);
  const uint64_t D = c->a_D;
  if (!D || (!sig && !keys)) return 0;
  const int H = bands * rows_per_band;
  if (H > 64)
    hipLaunchKernelGGL(nd_sig_k<true>, dim3(nd_grid(c, D, NW)), dim3(NT), 0, c->stream, c->a_rows.p, c->a_offs.p, D, c->a_nnz, H, bands, rows_per_band, sig, keys);
  else
    hipLaunchKernelGGL(nd_sig_k<false>, dim3(nd_grid(c, D, NW)), dim3(NT), 0, c->stream, c->a_rows.p, c->a_offs.p, D, c->a_nnz, H, bands, rows_per_band, sig, keys);
  LAUNCH_CHECK(c);
  return 0;
}

int k_nd_jaccard(isle_ctx* c, uint64_t n_pairs, const uint32_t* a, const uint32_t* b, uint32_t* inter, uint32_t* uni) {
  TimeScope ts(c, ISLE_T_INGEST);
  if (!n_pairs) return 0;
  hipLaunchKernelGGL(nd_jaccard_k, dim3(nd_grid(c, n_pairs, NW)), dim3(NT), 0, c->stream, c->a_rows.p, c->a_offs.p, c->a_D, c->a_nnz, n_pairs, a, b, inter, uni);
  LAUNCH_CHECK(c);
  return 0;
}

int k_nd_resolve(isle_ctx* c, NdKey form, uint64_t num, uint64_t den, int bands, const uint64_t* keys, uint32_t* parent, uint32_t* first_of, uint32_t* keep,
                 uint64_t* kept, uint64_t* pairs_tested, uint64_t* rounds) {
  TimeScope ts(c, ISLE_T_INGEST);
  const uint64_t D = c->a_D, nnz = c->a_nnz;
  *kept = *pairs_tested = *rounds = 0;
  if (!D) return 0;
  const bool narrow = form == ND_FORM_NARROW;
  DevBuf<uint64_t> key_a, key_b;
  DevBuf<uint32_t> val_a, val_b, flag, cur_head, next_head, done;
  DevBuf<int64_t> place, run_of, scratch;
  DevBuf<unsigned long long> counters;
  StreamDrain drain(c);
  HIPCHK(c, key_a.reserve(D));
  HIPCHK(c, key_b.reserve(D));
  HIPCHK(c, val_a.reserve(D));
  HIPCHK(c, val_b.reserve(D));
  HIPCHK(c, flag.reserve(D));
  HIPCHK(c, cur_head.reserve(D));
  HIPCHK(c, next_head.reserve(D));
  HIPCHK(c, done.reserve(D));
  HIPCHK(c, place.reserve(D + 1));
  HIPCHK(c, run_of.reserve(D + 1));
  HIPCHK(c, scratch.reserve(isle_scan_scratch(D) + 8));
  HIPCHK(c, counters.reserve(2 * ND_BATCH));
  hipLaunchKernelGGL(nd_iota_k, dim3(nd_grid(c, D, NT)), dim3(NT), 0, c->stream, parent, D);
  LAUNCH_CHECK(c);
  uint64_t n = D;  // the live documents: every leader of the band before
  for (int b = 0; b < bands; ++b) {
    // ---- the live list, ascending, and its pairs sorted by key: stable, so the documents ascend within a run
    hipLaunchKernelGGL(nd_live_flag_k, dim3(nd_grid(c, D, NT)), dim3(NT), 0, c->stream, parent, D, flag.p);
    LAUNCH_CHECK(c);
    HIPCHK(c, (isle_scan::exclusive_scan<uint32_t, int64_t>(c->stream, flag.p, D, place.p, scratch.p)));
    hipLaunchKernelGGL(nd_live_k, dim3(nd_grid(c, D, NT)), dim3(NT), 0, c->stream, flag.p, place.p, keys + (uint64_t)b * D, D, n, narrow, key_a.p, val_a.p);
    LAUNCH_CHECK(c);
    bool in_a = true;
    ISLECHK(k_sort_pairs_u64(c, key_a.p, val_a.p, key_b.p, val_b.p, n, docs_key_bits(narrow), &in_a));
    const uint64_t* key = in_a ? key_a.p : key_b.p;
    const uint32_t* doc = in_a ? val_a.p : val_b.p;
    // ---- the runs numbered, their first documents the first leaders
    hipLaunchKernelGGL(nd_head_flag_k, dim3(nd_grid(c, n, NT)), dim3(NT), 0, c->stream, key, n, flag.p);
    LAUNCH_CHECK(c);
    HIPCHK(c, (isle_scan::exclusive_scan<uint32_t, int64_t>(c->stream, flag.p, n, run_of.p, scratch.p)));
    int64_t got_n[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(&got_n[0], place.p + D, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&got_n[1], run_of.p + n, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if ((uint64_t)got_n[0] != n || got_n[1] < 1 || (uint64_t)got_n[1] > n)
      return isle_fail(c, ISLE_E_HIP, "doc_near_duplicates: band %d: the scans count %lld live documents (the rounds: %llu) in %lld runs", b, (long long)got_n[0],
                       (unsigned long long)n, (long long)got_n[1]);
    const uint64_t R = (uint64_t)got_n[1];
    HIPCHK(c, hipMemsetAsync(cur_head.p, 0xff, R * sizeof(uint32_t), c->stream));
    HIPCHK(c, hipMemsetAsync(next_head.p, 0xff, R * sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL(nd_heads_k, dim3(nd_grid(c, n, NT)), dim3(NT), 0, c->stream, flag.p, run_of.p, n, R, cur_head.p, done.p);
    LAUNCH_CHECK(c);
    // ---- rounds: round k tests every unresolved document against its run's k-th leader.  ND_BATCH rounds are queued behind each other, each
    // with its own counter pair, and their counters read back together: a round that finds nothing unresolved does nothing
    uint64_t left = n - R, heads = R, band_rounds = 1;  // every run has one leader at least
    while (left) {
      HIPCHK(c, hipMemsetAsync(counters.p, 0, 2 * ND_BATCH * sizeof(unsigned long long), c->stream));
      for (int i = 0; i < ND_BATCH; ++i) {
        hipLaunchKernelGGL(nd_round_k, dim3(nd_grid(c, n, NW)), dim3(NT), 0, c->stream, c->a_rows.p, c->a_offs.p, D, nnz, n, run_of.p, doc, R, cur_head.p, next_head.p,
                           done.p, parent, num, den, counters.p + 2 * i);
        LAUNCH_CHECK(c);
        hipLaunchKernelGGL(nd_advance_k, dim3(nd_grid(c, R, NT)), dim3(NT), 0, c->stream, n, R, cur_head.p, next_head.p, done.p, counters.p + 2 * i + 1);
        LAUNCH_CHECK(c);
      }
      unsigned long long got[2 * ND_BATCH] = {0};
      HIPCHK(c, hipMemcpyAsync(got, counters.p, sizeof(got), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
      for (int i = 0; i < ND_BATCH && left; ++i) {
        const unsigned long long far = got[2 * i], made = got[2 * i + 1];
        *pairs_tested += left;
        if (far > left || made > far || (far && !made))
          return isle_fail(c, ISLE_E_HIP, "doc_near_duplicates: band %d: a round leaves %llu of %llu documents dissimilar to their leaders and makes %llu new leaders", b,
                           far, (unsigned long long)left, made);
        if (made) ++band_rounds;  // some run got its next leader: the largest number of leaders in a run grew by one
        heads += made;
        left = far - made;
      }
    }
    *rounds += band_rounds;
    n = heads;
  }
  // ---- the roots of the parent chains, the kept flags
  HIPCHK(c, hipMemcpyAsync(first_of, parent, D * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
  for (int pass = 0;; ++pass) {
    HIPCHK(c, hipMemsetAsync(counters.p, 0, 2 * sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(nd_roots_k, dim3(nd_grid(c, D, NT)), dim3(NT), 0, c->stream, first_of, D, counters.p);
    LAUNCH_CHECK(c);
    unsigned long long changed = 0;
    HIPCHK(c, hipMemcpyAsync(&changed, counters.p, sizeof(changed), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (!changed) break;
    if (pass > bands) return isle_fail(c, ISLE_E_HIP, "doc_near_duplicates: the parent chains are longer than the %d bands", bands);
  }
  HIPCHK(c, hipMemsetAsync(counters.p, 0, 2 * sizeof(unsigned long long), c->stream));
  hipLaunchKernelGGL(nd_keep_k, dim3(nd_grid(c, D, NT)), dim3(NT), 0, c->stream, first_of, D, keep, counters.p);
  LAUNCH_CHECK(c);
  unsigned long long got_kept = 0;
  HIPCHK(c, hipMemcpyAsync(&got_kept, counters.p, sizeof(got_kept), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (got_kept != n) return isle_fail(c, ISLE_E_HIP, "doc_near_duplicates: %llu roots counted, %llu documents live after the last band", got_kept, (unsigned long long)n);
  *kept = got_kept;
  return 0;
}
