// isle_amd/csrc/score_docs.hip — held-out scores per document (isle_hip_score_docs): a sampled dense-sparse product, z = M[w, :] . theta[:, d]
// at every stored entry (w, c) of a sparse matrix, and a sum per document in a stated order.  The rule (the weight domain, the fused step,
// the classes, the terms, the order of the sum) is score_host.h's, and the kernels compile its functions; the refusals and the order of the
// steps are api_stages.cpp's.  The model is read in inf_pack_k's layout (vocab x round4(k) row-major, infer_resident.hip): the topics of
// one document are ascending addresses inside one model row.
//   sc_rows_k   one thread per weight row: every entry checked (the first bad one named through one 64-bit atomicMin) and the row sum s_d
//               in stored order.
//   sc_walk_k   a wave owns a document.  It stages the weight row in LDS as (topic, theta'), at most SCORE_TILE = 256 entries at a time
//               (3 KiB per wave whatever k is; a row of more is staged tile after tile, again for every 64 entries of the document); lane i
//               takes the entries i, i + 64, ..; every lane walks the staged row (the LDS reads are broadcasts) and gathers
//               M[w ld + t], keeping its z in a double across tiles; it classes its entry, forms the term and keeps its lane sums; the
//               lanes are folded by shuffles, p[i] += p[i + s], s = 32 .. 1; lane 0 stores the document's five numbers.  z_out is
//               written on the way where asked for.  A word >= vocab or a bad count is named through one 64-bit atomicMin and not read.
// Plain stores only, no floating-point atomic, nothing resident is written.
// NOT MEASURED, and not presented as tuned: a wave per document (documents of few entries leave lanes idle; a part of a wave per document is
// the alternative); the sparse walk for dense weight rows (a dense form that reads whole model rows as float4 would be another rule where
// the model holds NaN, and is not built); the 256-entry LDS tile; the grid of 8 workgroups per CU.
// Compiler's report for gfx950 (hipcc -O3 -Rpass-analysis=kernel-resource-usage); no kernel of this file uses scratch or spills:
//   sc_rows_k   VGPRs 18, SGPRs 42, scratch 0 bytes, LDS 0, occupancy 8 waves/SIMD
//   sc_walk_k   VGPRs 84, SGPRs 104, scratch 0 bytes, LDS 12288 bytes (4 waves x 256 x (8 + 4)), occupancy 5 waves/SIMD (the inlined fp64 log)
#include <algorithm>

#include "common.h"
#include "score_host.h"

namespace {

constexpr int SC_T = 256;
constexpr int SC_WAVES = SC_T / 64;

__global__ __launch_bounds__(SC_T) void sc_rows_k(const int64_t* __restrict__ off, const uint32_t* __restrict__ topic, const float* __restrict__ weight,
                                                  uint64_t rows, uint32_t k, double* __restrict__ rs, unsigned long long* __restrict__ err) {
  for (uint64_t r = (uint64_t)blockIdx.x * SC_T + threadIdx.x; r < rows; r += (uint64_t)gridDim.x * SC_T) {
    const int64_t b = off[r], e = off[r + 1];
    double s = 0.0;
    uint32_t before = 0u;
    for (int64_t i = b; i < e; ++i) {
      const uint32_t t = topic[i];
      const float w = weight[i];
      unsigned what = topdocs_entry_fault(t, k, i == b, before);
      if (!what && !prev_weight_ok(w)) what = SCORE_BAD_WEIGHT;
      if (what) atomicMin(err, ((unsigned long long)i << 2) | (unsigned long long)what);
      before = t;
      s = s + (double)w;
    }
    rs[r] = s;
  }
}

// The weight rows have passed sc_rows_k: every topic is < k <= ld.  rs: null without normalise.  z_out: null, or indexed by the entry.
__global__ __launch_bounds__(SC_T) void sc_walk_k(const int64_t* __restrict__ w_off, const uint32_t* __restrict__ w_topic, const float* __restrict__ w_weight,
                                                  uint64_t rows, const float* __restrict__ M, uint32_t ld, uint64_t vocab, const float* __restrict__ cnt,
                                                  const uint32_t* __restrict__ word, const int64_t* __restrict__ off, const double* __restrict__ rs,
                                                  int measure, double floor, double* __restrict__ score, double* __restrict__ tokens,
                                                  uint32_t* __restrict__ unscored_entries, double* __restrict__ unscored_tokens,
                                                  uint32_t* __restrict__ floored, double* __restrict__ z_out, unsigned long long* __restrict__ err) {
#pragma clang fp contract(off)
  __shared__ double sc_th[SC_WAVES][SCORE_TILE];
  __shared__ uint32_t sc_tp[SC_WAVES][SCORE_TILE];
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  double* const th = sc_th[wv];
  uint32_t* const tp = sc_tp[wv];
  const bool norm = rs != nullptr;
  for (uint64_t r = (uint64_t)blockIdx.x * SC_WAVES + wv; r < rows; r += (uint64_t)gridDim.x * SC_WAVES) {  // wave-uniform
    const int64_t wb = w_off[r], eb = off[r], ee = off[r + 1];
    const double s = norm ? rs[r] : 0.0;
    const int64_t nw = (norm && s == 0.0) ? 0 : w_off[r + 1] - wb;  // a row whose sum is 0 has no weights
    bool staged = false;
    double ps = 0.0, pt = 0.0, pu = 0.0;
    uint32_t ue = 0u, fl = 0u;
    for (int64_t e0 = eb; e0 < ee; e0 += 64) {
      const int64_t e = e0 + lane;
      const bool have = e < ee;
      uint32_t w = have ? word[e] : 0u;
      const float c = have ? cnt[e] : 0.0f;
      bool ok = have;
      if (have && w >= vocab) {
        atomicMin(err, ((unsigned long long)e << 1) | (unsigned long long)SCORE_BAD_WORD);
        ok = false;
      } else if (have && !score_count_ok(c)) {
        atomicMin(err, ((unsigned long long)e << 1) | (unsigned long long)SCORE_BAD_COUNT);
        ok = false;
      }
      if (!ok) w = 0u;  // (row 0 exists: vocab >= 1; the lane's z is not used)
      const float* const mrow = M + (size_t)w * ld;
      double z = 0.0;
      for (int64_t t0 = 0; t0 < nw; t0 += SCORE_TILE) {
        const uint32_t tn = nw - t0 < (int64_t)SCORE_TILE ? (uint32_t)(nw - t0) : SCORE_TILE;
        if (!staged || nw > (int64_t)SCORE_TILE) {
          // (the walk's loads are done before the tile is overwritten, and the stores before the next walk: the wave's LDS operations
          // complete in order; the fences hold the compiler)
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          for (uint32_t j = lane; j < tn; j += 64u) {
            tp[j] = w_topic[wb + t0 + j];
            th[j] = score_theta(w_weight[wb + t0 + j], norm, s);
          }
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          staged = true;
        }
        for (uint32_t j = 0; j < tn; ++j) z = score_step(z, mrow[tp[j]], th[j]);
      }
      if (z_out && have) z_out[e] = z;
      if (ok) {
        double at;
        const int cls = score_class(z, floor, &at);
        if (cls == SCORE_UNSCORED) {
          ++ue;
          pu = pu + (double)c;
        } else {
          if (cls == SCORE_FLOORED) ++fl;
          ps = ps + score_term(measure, c, at, measure == SCORE_LOG ? log(at) : 0.0);
          pt = pt + (double)c;
        }
      }
    }
    for (int sft = 32; sft; sft >>= 1) {  // lanes >= sft hold values no later step reads
      ps = ps + __shfl_down(ps, sft);
      pt = pt + __shfl_down(pt, sft);
      pu = pu + __shfl_down(pu, sft);
      ue += __shfl_down(ue, sft);
      fl += __shfl_down(fl, sft);
    }
    if (lane == 0u) {
      score[r] = ps;
      tokens[r] = pt;
      unscored_tokens[r] = pu;
      unscored_entries[r] = ue;
      floored[r] = fl;
    }
  }
}

}  // namespace

int k_sc_rows(isle_ctx* c, const TdView& w, double* rs, uint64_t* err_dev, uint64_t* bad) {
  TimeScope ts(c, ISLE_T_INFER);
  *bad = ~0ull;
  if (!w.rows) return 0;
  HIPCHK(c, hipMemsetAsync(err_dev, 0xff, sizeof(uint64_t), c->stream));
  const unsigned blocks = (unsigned)std::min<uint64_t>((w.rows + SC_T - 1) / SC_T, (uint64_t)c->num_cus * 8);
  hipLaunchKernelGGL(sc_rows_k, dim3(blocks), dim3(SC_T), 0, c->stream, w.off, w.topic, w.value, w.rows, w.num_topics, rs, (unsigned long long*)err_dev);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(bad, err_dev, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

int k_sc_walk(isle_ctx* c, const TdView& w, const float* M, int ld, uint64_t vocab, const float* cnt, const uint32_t* word, const int64_t* off,
              const double* rs, int measure, double floor, double* score, double* tokens, uint32_t* unscored_entries, double* unscored_tokens,
              uint32_t* floored, double* z_out, uint64_t* err_dev, uint64_t* bad) {
  TimeScope ts(c, ISLE_T_INFER);
  *bad = ~0ull;
  if (!w.rows) return 0;
  HIPCHK(c, hipMemsetAsync(err_dev, 0xff, sizeof(uint64_t), c->stream));
  const unsigned blocks = (unsigned)std::min<uint64_t>((w.rows + SC_WAVES - 1) / SC_WAVES, (uint64_t)c->num_cus * 8);
  hipLaunchKernelGGL(sc_walk_k, dim3(blocks), dim3(SC_T), 0, c->stream, w.off, w.topic, w.value, w.rows, M, (uint32_t)ld, vocab, cnt, word, off, rs, measure,
                     floor, score, tokens, unscored_entries, unscored_tokens, floored, z_out, (unsigned long long*)err_dev);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(bad, err_dev, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}
