// isle_amd/csrc/text_tiles.h — the one count / scan / write skeleton of the per-document text formatters (infer_text.hip,
// doc_report.hip; model_text.hip keeps kernels of its own and says why).  A text is a sequence of candidate lines cut into tiles of at
// most MT_TILE consecutive candidates, MT_ITEMS per thread:
//   text_count_k  one read of the source: bytes per tile, lines printed (64-bit), and the least key of a candidate that would be printed
//                 but lies outside the host writers' domain
//   the exclusive scan of the tile sizes into 64-bit offsets (scan.h); offs[ntiles] is the size of the text
//   text_write_k  per tile: tiles of size 0 are skipped before anything is read; else the candidates again (those outside the domain
//                 dropped here too, not on the count pass's word), a block scan of their lengths, every line's characters into LDS at the
//                 tile's own alignment modulo 16, then the tile leaves as whole aligned 16-byte lines (mt_store_tile, text_format.h)
//   k_text_tiles  the host side: scratch, count, scan, the refusal, the two counters, and the write launches handed to k_text_pump
// What a line is, is the source's business.  A source is a plain struct passed by value with
//   static constexpr int kWindow           offsets the block stages per tile in LDS (0: none, and the kernels declare no window)
//   static constexpr bool kSkipEmpty       the count pass probes a tile before it stages, and a tile that prints nothing
//                                          gets the size 0 and stages no offsets (worth a block sum where candidates can be absent)
//   struct Tile { uint32_t n; ... }        what every thread knows of a tile; n = its candidates
//   struct Line { bool present; ... }      a candidate's numbers; present = it is printed
//   Tile open(tile)
//   Line probe(t, l)                       candidate l < t.n: printed or not, and what of its line needs no window
//   void stage(t, win, row0)               kWindow only; every thread of the block calls it (it holds barriers)
//   void place(t, l, win, row0, x)         the rest of a printed line
//   bool in_domain(x)                      after place
//   uint32_t len(t, l, x)
//   char* put(t, l, x, p)
//   char extra(t)                          the one byte that ends the tile after its lines, or 0 for none (a dense column's '\n')
//   uint64_t key(t, l)                     what stat[1] reports for an offending candidate
// Every early `continue` of the tile loops is the same for all threads of the block: stage, mt_block_sum, block_exclusive and
// mt_store_tile hold barriers.
#pragma once
#include <algorithm>

#include "common.h"
#include "scan.h"
#include "text_format.h"

#pragma clang fp contract(off)

// stat[0] += lines printed; stat[1] = min over the offending printed candidates of their key
template <class Src>
__global__ __launch_bounds__(MT) void text_count_k(Src src, uint64_t ntiles, uint32_t* __restrict__ sizes, unsigned long long* __restrict__ stat) {
  __shared__ uint32_t shb[MT / ISLE_WAVE], shc[MT / ISLE_WAVE];
  uint32_t* win = nullptr;
  uint64_t* row0 = nullptr;
  if constexpr (Src::kWindow > 0) {
    __shared__ uint32_t win_lds[Src::kWindow];
    __shared__ uint64_t row0_lds;
    win = win_lds;
    row0 = &row0_lds;
  }
  for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const typename Src::Tile t = src.open(tile);
    if constexpr (Src::kWindow > 0 && !Src::kSkipEmpty) src.stage(t, win, row0);
    typename Src::Line x[MT_ITEMS];
    uint32_t cand = 0;
#pragma unroll
    for (int i = 0; i < MT_ITEMS; ++i) {
      const uint32_t l = threadIdx.x * MT_ITEMS + i;
      x[i].present = false;
      if (l < t.n) x[i] = src.probe(t, l);
      cand += x[i].present ? 1u : 0u;
    }
    if constexpr (Src::kWindow > 0 && Src::kSkipEmpty) {
      if (mt_block_sum(cand, shc) == 0) {  // nothing to place, nothing to store
        if (threadIdx.x == 0) sizes[tile] = 0;
        continue;
      }
      src.stage(t, win, row0);
    }
    uint32_t bytes = 0, cnt = 0;
    unsigned long long bad = ~0ull;
#pragma unroll
    for (int i = 0; i < MT_ITEMS; ++i) {
      if (!x[i].present) continue;
      const uint32_t l = threadIdx.x * MT_ITEMS + i;
      src.place(t, l, win, row0, x[i]);
      if (!src.in_domain(x[i])) {
        bad = min(bad, (unsigned long long)src.key(t, l));
      } else {
        ++cnt;
        bytes += src.len(t, l, x[i]);
      }
    }
    if (bad != ~0ull) atomicMin(&stat[1], bad);
    const uint32_t tb = mt_block_sum(bytes, shb), tc = mt_block_sum(cnt, shc);
    if (threadIdx.x == 0) {
      sizes[tile] = tb + (src.extra(t) ? 1u : 0u);
      if (tc) atomicAdd(&stat[0], (unsigned long long)tc);
    }
  }
}

// tiles [tile0, tile0 + n) -> out[offs[tile] - offs[tile0] ...); out is 16-byte aligned
template <class Src>
__global__ __launch_bounds__(MT) void text_write_k(Src src, uint64_t tile0, uint64_t n, const uint64_t* __restrict__ offs, unsigned char* __restrict__ out) {
  __shared__ uint4 lines[MT_LDS_LINES];
  __shared__ uint32_t sh[MT];
  uint32_t* win = nullptr;
  uint64_t* row0 = nullptr;
  if constexpr (Src::kWindow > 0) {
    __shared__ uint32_t win_lds[Src::kWindow];
    __shared__ uint64_t row0_lds;
    win = win_lds;
    row0 = &row0_lds;
  }
  char* const text = reinterpret_cast<char*>(lines);
  const uint64_t base = offs[tile0];
  for (uint64_t tile = tile0 + blockIdx.x; tile < tile0 + n; tile += gridDim.x) {
    const uint64_t dst0 = offs[tile] - base;
    const uint32_t nbytes = (uint32_t)(offs[tile + 1] - offs[tile]);
    if (nbytes == 0) continue;
    const uint32_t shift = (uint32_t)(dst0 & 15u);  // LDS position == position in out, modulo 16
    const typename Src::Tile t = src.open(tile);
    if constexpr (Src::kWindow > 0) src.stage(t, win, row0);
    typename Src::Line x[MT_ITEMS];
    uint32_t mine = 0;
#pragma unroll
    for (int i = 0; i < MT_ITEMS; ++i) {
      const uint32_t l = threadIdx.x * MT_ITEMS + i;
      x[i].present = false;
      if (l < t.n) {
        x[i] = src.probe(t, l);
        if (x[i].present) {
          src.place(t, l, win, row0, x[i]);
          if (!src.in_domain(x[i])) x[i].present = false;  // (the counting pass has refused such a call)
        }
      }
      if (x[i].present) mine += src.len(t, l, x[i]);
    }
    uint32_t total;
    const uint32_t at = isle_scan::block_exclusive<uint32_t>(mine, sh, &total);
    char* p = text + shift + at;
#pragma unroll
    for (int i = 0; i < MT_ITEMS; ++i) {
      if (x[i].present) p = src.put(t, threadIdx.x * MT_ITEMS + i, x[i], p);
    }
    const char end = src.extra(t);
    if (threadIdx.x == 0 && end && total < nbytes) text[shift + total] = end;  // before mt_store_tile's first barrier
    mt_store_tile(lines, shift, nbytes, out, dst0);
  }
}

// The host side of a formatter `who` whose kernels are timed as `family`: the sizes and offsets of src's ntiles tiles, then either
// refuse(key) — the formatter's isle_fail for the offending candidate of the least key — or *nbytes / *nlines and, with a sink and a
// text that is not empty, its delivery through k_text_pump in chunks cut at multiples of `group` tiles.
template <class Src, class Refuse>
int k_text_tiles(isle_ctx* c, const char* who, int family, const Src& src, uint64_t ntiles, uint64_t group, isle_text_sink_fn sink, void* user,
                 uint64_t* nbytes, uint64_t* nlines, Refuse refuse) {
  const unsigned cap = (unsigned)c->num_cus * 16u;
  HIPCHK(c, c->mt_sizes.reserve(ntiles));
  HIPCHK(c, c->mt_offs.reserve(ntiles + 1));
  HIPCHK(c, c->mt_blk.reserve(isle_scan::scan_scratch_elems(ntiles)));
  HIPCHK(c, c->mt_stat.reserve(2));
  unsigned long long* stat = (unsigned long long*)c->mt_stat.p;
  const uint64_t init[2] = {0, ~0ull};
  uint64_t h[3] = {0, ~0ull, 0};
  {
    TimeScope ts(c, family);
    HIPCHK(c, hipMemcpyAsync(stat, init, sizeof(init), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(text_count_k<Src>, dim3((unsigned)std::min<uint64_t>(ntiles, cap)), dim3(MT), 0, c->stream, src, ntiles, c->mt_sizes.p, stat);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, (isle_scan::exclusive_scan<uint32_t, uint64_t>(c->stream, c->mt_sizes.p, ntiles, c->mt_offs.p, c->mt_blk.p)));
  }
  HIPCHK(c, hipMemcpyAsync(h, stat, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(h + 2, c->mt_offs.p + ntiles, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (h[1] != ~0ull) return refuse(h[1]);
  const uint64_t total = h[2];
  if (nbytes) *nbytes = total;
  if (nlines) *nlines = h[0];
  if (!sink || total == 0) return 0;
  return k_text_pump(c, who, c->mt_offs.p, ntiles, total, group, sink, user, [&](uint64_t t0, uint64_t n, unsigned char* out) -> int {
    TimeScope ts(c, family);
    hipLaunchKernelGGL(text_write_k<Src>, dim3((unsigned)std::min<uint64_t>(n, cap)), dim3(MT), 0, c->stream, src, t0, n, c->mt_offs.p, out);
    HIPCHK(c, hipGetLastError());
    return 0;
  });
}
