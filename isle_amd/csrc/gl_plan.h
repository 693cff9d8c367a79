// isle_amd/csrc/gl_plan.h — the host plan of the LDS-banded operator build (gram_lds.hip k_gl_build): which slices a wave owns, which waves and
// source bands a workgroup of gl_apply_k takes, and which slab it writes.  Plain C++ (no HIP type, no isle_ctx, nothing read from the
// environment: every switch arrives in GlPlanOpts), so that the arithmetic that decides every workgroup descriptor runs without a device:
// gl_plan_main.cpp prints a plan, tests/test_gl_plan_cpu.py checks it.  The double arithmetic decides ties: it is written as measured, and no
// build of it takes -ffast-math, -march or an FMA-enabling flag.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

struct GlDesc {  // one workgroup: 16 waves wave0 + i*wstride (i < nw), source bands [b0, b1), output slab
  uint32_t wave0, wstride, nw, b0, b1, slab, pos_base, pad;
};

constexpr int GL_WAVES = 16;
constexpr int GL_GMAX = 8;  // groups (output items per lane) of a wave: 4 ... 8, GlSide::G; count records are GL_GMAX wide
#ifndef GL_RB_V
#define GL_RB_V 4078
#endif
#ifndef GL_APPLY_WAVES_V
#define GL_APPLY_WAVES_V 16
#endif
constexpr uint32_t GL_RB = GL_RB_V;  // source rows per band (even: the half plane is whole float4)
constexpr uint32_t GL_APPLY_WAVES = GL_APPLY_WAVES_V;  // most waves of a workgroup of gl_apply_k (experiment builds: 8 with bands of half the height, two workgroups per CU)
constexpr uint32_t GL_NONE = 0xffffffffu;
constexpr double GL_BAND_COST = 256.0;  // cost of staging one 160 KB band from HBM in pass 2, in super-rounds (measured by sweep at C2)

struct GlPlanOpts {
  int g1 = 0, g2 = 0;     // ISLE_GL_G1 / ISLE_GL_G2 through gl_forced_g: items per lane of pass 1 / pass 2; 0: the build's own rule
  bool rounds = true;     // ISLE_GL_ROUNDS=0 clears it: pass 1 stays strided
  bool columns = true;    // ISLE_GL_COLUMNS=0 clears it: per-block chunking only
  uint32_t test_cus = 0;  // ISLE_GL_TEST_CUS (>= 1): pass 1 is laid out for that many CUs — the geometry of a larger problem on a small one; 0: the device's
};
inline int gl_forced_g(int asked) { return std::max(4, std::min(GL_GMAX, asked)); }

// what both passes hand to the stream build (gram_lds.hip GlStream): the geometry of a side and the slices of its waves
struct GlGeom {
  uint32_t NB = 0, nslice = 0, nwv = 0;
  uint32_t wpg = GL_APPLY_WAVES;    // waves per workgroup of gl_apply_k (pass 2: per word block)
  int G = 4;                        // output items per lane
  std::vector<uint32_t> slice_of;   // nwv x G: the slice of (wave, group), GL_NONE where there is none
};
struct GlPlan1 : GlGeom {
  bool adjacent = false;            // a workgroup takes adjacent waves (whole rounds of the CUs), else waves strided over the length order
  std::vector<GlDesc> desc;
};
struct GlGeom2 : GlGeom {
  uint32_t nblk = 0, bitems = 0;    // word blocks of wpg waves; words per block
};
struct GlSched2 {
  const char* error = nullptr;      // the band-column cut failed (k_gl_build: "operator build: <error>")
  bool columns = false;
  std::vector<uint32_t> cut;        // band-column form: column cc = bands [cut[cc], cut[cc + 1]); NC = cut.size() - 1
  std::vector<GlDesc> desc;
  std::vector<uint32_t> slab0, nch;  // per word block: first partial slab, number of slabs
  uint32_t nslab = 0;
};

// ---- pass 1: outputs = documents (position order), sources = words
inline GlPlan1 gl_plan_pass1(uint64_t nnz, uint32_t D, uint32_t V, uint32_t num_cus, const GlPlanOpts& o) {
  GlPlan1 s1;
  s1.NB = (V + GL_RB - 1) / GL_RB;
  s1.nslice = (D + 63) / 64;
  // items per lane G and waves per workgroup: the makespan model  rounds x (waves x G x LDS time of a slice + staging of all bands)
  // over G = 4..8 and 1..16 waves.  Every workgroup stages every word band, so a shard whose documents need more than one round of
  // workgroups at G = 4 (a C3 shard: 306 workgroups on 256 CUs, 0.44 ms per pass) runs one fuller round at G = 5 (245 workgroups,
  // 0.31 ms), and all of config 3 on one GPU five rounds at G = 8 instead of ten (2.69 -> 2.34 ms); small matrices keep G = 4 and
  // take fewer waves per workgroup so that all CUs stay busy.  The model's figures against the measured ones, pass 1 with 10 columns:
  // C3 shard G = 5: 312 / 313 us; config 3 on one GPU G = 4 / 6 / 8: 2610 / 2530 / 2310 against 2690 / 2490 / 2336 us.
  // ISLE_GL_G1 = 4..8 forces G.
  const uint32_t maxw = GL_APPLY_WAVES;
  uint32_t wpw = maxw;
  const uint32_t cus = o.test_cus ? o.test_cus : num_cus;
  {
    const double t_slice = 0.05 * 2.5 * (double)nnz / 256.0 / std::max<uint32_t>(1u, s1.nslice);  // us: ~50 ns per super-round, ~2.5x padded
    const double t_stage = 2.0 * s1.NB;                                                            // us: ~2 us per band from L2
    const int g_lo = o.g1 ? o.g1 : 4, g_hi = o.g1 ? g_lo : GL_GMAX - 1;  // 8: the 10-column kernel spills there
    double best = 1e300;
    for (int G = g_lo; G <= g_hi; ++G) {
      const uint32_t nwv = (s1.nslice + G - 1) / G;
      for (uint32_t cand = maxw; cand >= 1; --cand) {
        const uint32_t wgs = (nwv + cand - 1) / cand;
        const double fewer = 1.0 + 0.25 * (double)(GL_WAVES - cand) / GL_WAVES;  // fewer waves hide less of the id-stream latency
        const uint32_t rounds = (wgs + cus - 1) / cus;
        // more than one round: the workgroups are spread over WHOLE rounds (below), a wave then owns nslice / (rounds x CUs x waves) slices
        const double per_wave = rounds > 1 ? (double)s1.nslice / ((double)rounds * cus * cand) : (double)G;
        const double cost = (double)rounds * (cand * per_wave * t_slice * fewer + t_stage);
        if (cost < best * 0.97) {  // prefer fewer items per lane and more waves per workgroup unless clearly worse
          best = cost;
          wpw = cand;
          s1.G = G;
        }
      }
    }
  }
  s1.nwv = (s1.nslice + s1.G - 1) / s1.G;
  s1.wpg = wpw;
  // More than one round of workgroups: their number is rounded up to whole rounds of the CUs — the waves of the last quantile range
  // then own one slice less — and a workgroup takes ADJACENT waves (slices of neighbouring lengths: its waves reach the barrier of a band
  // together; the workgroups differ by the length of their documents, the longest are launched first).  5.45 rounds of 7 slices per wave
  // ran like 6 (all of config 3 on one GPU, pass 1); 6 rounds of 6.36 do the same work with the CUs busy to the end.  One round (a C3
  // shard: 244 workgroups): the workgroups must finish together, so they take waves strided over the whole length order as before.
  {
    const uint32_t nwg0 = (s1.nwv + wpw - 1) / wpw;
    if (nwg0 > cus && o.rounds) {
      const uint32_t nwg_r = (nwg0 + cus - 1) / cus * cus;
      s1.nwv = nwg_r * wpw;
      s1.adjacent = true;
    }
  }
  // serpentine over G quantile ranges of the length-ordered slices: every wave gets long, middle and short slices alike
  const int G = s1.G;
  s1.slice_of.resize((size_t)s1.nwv * G);
  const uint64_t n = s1.nwv;
  for (uint64_t wv = 0; wv < n; ++wv)
    for (int g = 0; g < G; ++g) {
      const uint64_t cand = (g & 1) ? (uint64_t)(g + 1) * n - 1 - wv : (uint64_t)g * n + wv;
      s1.slice_of[wv * G + g] = cand < s1.nslice ? (uint32_t)cand : GL_NONE;
    }
  // workgroup j = waves j, j + nwg, j + 2 nwg, ... : equal totals, one slab (Y itself)
  const uint32_t nwg = (s1.nwv + wpw - 1) / wpw;
  s1.desc.resize(nwg);
  for (uint32_t j = 0; j < nwg; ++j) {
    uint32_t nw = 0;
    while (nw < wpw && (uint64_t)j + (uint64_t)nw * nwg < s1.nwv) ++nw;
    s1.desc[j] = s1.adjacent ? GlDesc{j * wpw, 1u, (uint32_t)std::min<uint64_t>(wpw, s1.nwv - (uint64_t)j * wpw), 0u, s1.NB, 0u, 0u, 0u} : GlDesc{j, nwg, nw, 0u, s1.NB, 0u, 0u, 0u};
  }
  return s1;
}

// ---- pass 2: outputs = words (position order), sources = documents (position order)
inline GlGeom2 gl_plan_pass2_geometry(uint32_t D, uint32_t V, uint32_t num_cus, const GlPlanOpts& o) {
  GlGeom2 s2;
  s2.NB = (D + GL_RB - 1) / GL_RB;
  s2.nslice = (V + 63) / 64;
  // items per lane in pass 2 (4 ... 8):
  // 4; 6 beyond 1024 document bands (more than 4 M documents): fewer word blocks, and every block stages every band of its columns.
  // Measured with the final kernels, pass 2: config 3 on one GPU (2452 bands) 2.41 / 2.40 / 2.26 / 3.07 ms at 4 / 5 / 6 / 8; a C3 shard
  // (307 bands) 0.309 / 0.334 / 0.314 at 4 / 5 / 6
  s2.G = o.g2 ? o.g2 : (s2.NB > 1024 ? 6 : 4);
  const uint32_t G2 = (uint32_t)s2.G;
  // a word block = wpb waves = G2 wpb consecutive slices; 16 waves unless the vocabulary is so small that blocks x bands would
  // leave CUs idle
  uint32_t wpb = GL_APPLY_WAVES;
  while (wpb > 1 && (uint64_t)((s2.nslice + G2 * wpb - 1) / (G2 * wpb)) * s2.NB < 2ull * num_cus) wpb /= 2;
  const uint32_t bslices = G2 * wpb;
  s2.bitems = 64 * bslices;
  s2.nblk = (s2.nslice + bslices - 1) / bslices;
  s2.nwv = s2.nblk * wpb;
  s2.wpg = wpb;
  // serpentine inside the block keeps its waves level
  s2.slice_of.resize((size_t)s2.nwv * G2);
  for (uint32_t ob = 0; ob < s2.nblk; ++ob)
    for (uint32_t w = 0; w < wpb; ++w)
      for (uint32_t g = 0; g < G2; ++g) {
        const uint32_t cand = (g & 1u) ? (g + 1) * wpb - 1 - w : g * wpb + w;
        const uint64_t sl = (uint64_t)ob * bslices + cand;
        s2.slice_of[((size_t)ob * wpb + w) * G2 + g] = sl < s2.nslice ? (uint32_t)sl : GL_NONE;
      }
  return s2;
}

// the band-column form needs 16 document bands; its totals are per (block, band), the per-block form's per block (gl_blocktot_k)
inline bool gl_use_columns(uint32_t NB, const GlPlanOpts& o) { return o.columns && NB >= 16; }

constexpr double GL_WGS_PER_CU = 2.0;  // measured by sweeps at C2, like GL_BAND_COST

// NC columns of equal total cost over the NB document bands (bcost per band, `all` their sum): column cc = bands [cut[cc], cut[cc + 1])
inline std::vector<uint32_t> gl_cut_columns(const std::vector<double>& bcost, double all, uint32_t NB, uint32_t NC) {
  std::vector<uint32_t> cut(NC + 1, 0);
  double pre = 0;
  uint32_t cc = 1;
  for (uint32_t bnd = 0; bnd < NB && cc < NC; ++bnd) {
    pre += bcost[bnd];
    // close column cc - 1 behind this band once its share of the cost is reached, leaving at least one band per later column
    while (cc < NC && (pre >= all * cc / NC || NB - (bnd + 1) <= NC - cc) && bnd + 1 > cut[cc - 1]) cut[cc++] = bnd + 1;
  }
  while (cc <= NC) cut[cc++] = NB;
  cut[NC] = NB;
  return cut;
}

// Band columns shared through L2.  Every word block walks every document band, so Y (48 MB at C2) is staged from HBM once
// per word block (13 x 48 MB = 0.62 GB of the 1.2 GB pass 2 moves; 25 x 60 MB = 1.5 of 2.6 GB at a C3 shard, where pass 2 runs
// at the HBM rate).  Here the document bands are cut into NC "columns" of equal total cost — at most colbands bands, 1.3 MB
// of Y — the SAME cut for all word blocks, and all workgroups of a column are queued back to back on ONE XCD (workgroup i
// runs on XCD i % 8), so the column's bands are fetched from HBM once and found in that XCD's 4 MB L2 by the other word
// blocks (measured with one workgroup per (block, column): FETCH_SIZE of pass 2 1.11 -> 0.66 GB).  Inside a column a word
// block is cut into sub-chunks of about the same cost as everybody else's (the word blocks differ 5x in cost; with whole
// columns per workgroup the heavy ones set the makespan: 0.301 -> 0.349 ms at C2).
// tot[ob * NB + band] = super-rounds of (word block, document band).
inline void gl_sched2_columns(GlSched2& s, const std::vector<unsigned long long>& tot, uint32_t nblk, uint32_t NB, uint32_t wpb, uint32_t bitems,
                              uint32_t num_cus) {
  const double bc = GL_BAND_COST, wgs_per_cu = GL_WGS_PER_CU;
  std::vector<double> bcost(NB, 0.0);
  double all = 0;
  for (uint32_t bnd = 0; bnd < NB; ++bnd) {
    for (uint32_t ob = 0; ob < nblk; ++ob) bcost[bnd] += (double)tot[(size_t)ob * NB + bnd] + bc;
    all += bcost[bnd];
  }
  // <= 12 bands (1.9 MB of Y) per column: measured at C2 / C3 shard, pass 2 in ms — per-block chunks 0.291 / 0.474, columns of
  // <= 8 bands 0.294 / 0.459, <= 12 bands 0.283 / 0.436, <= 16 bands 0.282 / 0.464
  // with the planar bands and the final kernels (round 3), all of config 3 on one GPU (2452 bands): 8 / 12 / 16 / 24 / 32 / 48 / 64 bands
  // 2.42 / 2.28 / 2.20 / 2.15 / 2.16 / 2.26 / 2.43 ms; a C3 shard and C2 do not depend on it (their column count is set by the other term)
  const uint32_t colbands = 24u;
  const double W = wgs_per_cu * num_cus;
  uint32_t NC = 8u * (uint32_t)std::ceil(std::max(W / (1.25 * nblk), (double)NB / colbands) / 8.0);
  NC = std::max(8u, std::min(NC, (NB / 8u) * 8u));
  const std::vector<uint32_t>& cut = s.cut = gl_cut_columns(bcost, all, NB, NC);
  for (uint32_t cc = 0; cc < NC; ++cc)
    if (cut[cc + 1] <= cut[cc]) {
      s.error = "empty band column";
      return;
    }
  const double target = std::max(1.0, all / W);
  // sub-chunks per (block, column), then the blocks' slab ranges, then the descriptors in XCD queues
  std::vector<uint32_t> nsub((size_t)nblk * NC);
  for (uint32_t ob = 0; ob < nblk; ++ob) {
    s.slab0[ob] = s.nslab;
    for (uint32_t cc = 0; cc < NC; ++cc) {
      double cost = 0;
      for (uint32_t bnd = cut[cc]; bnd < cut[cc + 1]; ++bnd) cost += (double)tot[(size_t)ob * NB + bnd] + bc;
      const uint32_t nb = cut[cc + 1] - cut[cc];
      const uint32_t n = (uint32_t)std::min<double>((double)nb, std::max(1.0, std::floor(cost / target + 0.5)));
      nsub[(size_t)ob * NC + cc] = n;
      s.nch[ob] += n;
      s.nslab += n;
    }
  }
  std::vector<std::vector<GlDesc>> xq(8);
  std::vector<std::pair<double, uint32_t>> order(nblk);
  std::vector<uint32_t> next(nblk);
  for (uint32_t ob = 0; ob < nblk; ++ob) next[ob] = s.slab0[ob];
  for (uint32_t cc = 0; cc < NC; ++cc) {
    const uint32_t b0 = cut[cc], b1 = cut[cc + 1], nb = b1 - b0;
    for (uint32_t ob = 0; ob < nblk; ++ob) {
      double t = 0;
      for (uint32_t bnd = b0; bnd < b1; ++bnd) t += (double)tot[(size_t)ob * NB + bnd];
      order[ob] = {-t / nsub[(size_t)ob * NC + cc], ob};
    }
    std::sort(order.begin(), order.end());  // heaviest workgroups of the column first
    for (auto& od : order) {
      const uint32_t ob = od.second, n = nsub[(size_t)ob * NC + cc];
      for (uint32_t q = 0; q < n; ++q)
        xq[cc % 8].push_back(GlDesc{ob * wpb, 1u, wpb, b0 + (uint32_t)((uint64_t)q * nb / n), b0 + (uint32_t)((uint64_t)(q + 1) * nb / n), next[ob]++,
                                    ob * bitems, 0u});
    }
  }
  size_t qmax = 0;
  for (auto& q : xq) qmax = std::max(qmax, q.size());
  s.desc.reserve(qmax * 8);
  for (size_t j = 0; j < qmax; ++j)
    for (uint32_t x = 0; x < 8; ++x) s.desc.push_back(j < xq[x].size() ? xq[x][j] : GlDesc{0u, 1u, 0u, 0u, 0u, 0u, 0u, 0u});  // empty: no wave is valid
}

// per word block: band chunks in proportion to the block's cost (round 1's form; small matrices, or ISLE_GL_COLUMNS=0).
// Cost = super-rounds (LDS-bound, ~50 ns of CU time each) + GL_BAND_COST per band staged; without the second term a block
// of rare words would walk all bands in a single workgroup.  tot[ob] = super-rounds of the word block.
inline void gl_sched2_blocks(GlSched2& s, const std::vector<unsigned long long>& tot, uint32_t nblk, uint32_t NB, uint32_t wpb, uint32_t bitems,
                             uint32_t num_cus) {
  const double bc = GL_BAND_COST, wgs_per_cu = GL_WGS_PER_CU;
  double all = 0;
  for (auto t : tot) all += (double)t;
  all += bc * (double)NB * nblk;
  const double target = std::max(1.0, all / (wgs_per_cu * num_cus));
  for (uint32_t ob = 0; ob < nblk; ++ob) {
    s.slab0[ob] = s.nslab;
    const uint32_t nzb = NB;
    const double cost = (double)tot[ob] + bc * nzb;
    const uint32_t n = (uint32_t)std::min<double>((double)nzb, std::max(1.0, std::ceil(cost / target)));
    for (uint32_t ch = 0; ch < n; ++ch) {
      const uint32_t b0 = (uint32_t)((uint64_t)ch * nzb / n), b1 = (uint32_t)((uint64_t)(ch + 1) * nzb / n);
      s.desc.push_back(GlDesc{ob * wpb, 1u, wpb, b0, b1, s.nslab, ob * bitems, 0u});
      ++s.nslab;
      ++s.nch[ob];
    }
  }
}

// the workgroups of pass 2 from the super-round totals gl_blocktot_k read back: nblk x NB of them with columns, nblk without
inline GlSched2 gl_plan_pass2_schedule(const std::vector<unsigned long long>& tot, uint32_t nblk, uint32_t NB, uint32_t wpb, uint32_t bitems,
                                       uint32_t num_cus, bool columns) {
  GlSched2 s;
  s.columns = columns;
  s.slab0.assign(nblk, 0);
  s.nch.assign(nblk, 0);
  if (columns) gl_sched2_columns(s, tot, nblk, NB, wpb, bitems, num_cus);
  else gl_sched2_blocks(s, tot, nblk, NB, wpb, bitems, num_cus);
  return s;
}
