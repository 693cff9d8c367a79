// isle_amd/csrc/infer_text.hip — the per-document topic files formatted on the device: the lines "<doc>\t<topic>\t<weight>\n" of
// ISLEInfer's top_topics_* files (drivers/ISLEInfer.cpp:100-112) and of ISLETrainer::output_doc_topic_weights' DocTopicWeights.tsv, as
// trainer_detail::doc_line_text / write_doc_topic_lines (isle_amd/host/trainer_hip.h) restate them, from the result of the last
// isle_hip_infer_resident where it lies.  The two integers are MMappedOutput::concat_int's plain decimals, the weight is mt_weight
// (text_format.h), the library's one copy of the digit rule.
//
// A line is a candidate index L of the call, cut into tiles of MT_TILE = 1024 consecutive candidates:
//   ISLE_DOCTEXT_ENTRIES  L = an entry of [off[row_begin], off[row_end]); every candidate is printed
//   ISLE_DOCTEXT_TOP      L = 5 (row - row_begin) + slot; slot i of a row is printed while slots 0 .. i hold a topic >= 0, else its
//                         length is 0
// An entry does not store its row (doc_text.h, shared with doc_report.hip).  Per tile, thread 0 finds the row of the tile's first entry by an upper-bound search in the
// offsets, the block stages the IT_WIN offsets that follow it in LDS (relative to the tile's first entry, clamped), and every line
// finds its row by a search in that window.  A tile of 1024 entries spans at most 1024 non-empty rows, but any number of empty ones:
// where the window's last offset does not lie beyond the tile (a run of empty documents longer than the window), the lines of that
// tile search the global offsets instead.  IT_WIN = 1024 (4 KiB of LDS) is a choice, not a measurement: it covers every tile whose rows
// hold on average one entry or more.
//   it_count_k   bytes per tile, lines printed (64-bit), the first candidate outside the writers' domain (a number >= 0x7fffffff,
//                concat_int's assert; a weight that is negative, NaN, infinite or >= 2^31)
//   the 64-bit exclusive scan of scan.h
//   it_write_k   mt_write_k's scheme: lengths, a block scan, the characters into LDS at the tile's alignment modulo 16, whole aligned
//                uint4 lines out (mt_store_tile)
// and the text leaves through k_text_pump (model_text.hip), the pump of the model files.  Nothing resident is written.
#include <algorithm>
#include <vector>

#include "common.h"
#include "doc_text.h"
#include "scan.h"
#include "text_format.h"

#pragma clang fp contract(off)

namespace {

// Where the lines come from.  Other per-document files of the reference (two integers and a weight per line) fit the same descriptor:
// a CSR of (column, value) over the rows, or a fixed number of slots per row.
struct ItSrc {
  int what;
  const int64_t* off;       // ENTRIES: offsets of the resident rows (rows + 1), off[0] = 0
  const uint32_t* topic;    // ENTRIES: per entry
  const int32_t* slot;      // TOP: five per row, < 0 = no further topic
  const float* weight;      // ENTRIES: per entry; TOP: five per row
  uint64_t row_begin, row_end;
  uint64_t first;           // ENTRIES: off[row_begin]; TOP: 5 row_begin — candidate L is element first + L
  uint64_t ncand;           // candidates of the call
  uint64_t base;
};
struct ItLine {
  uint64_t number, topic1;  // as printed
  float w;
  bool present;
};

// ENTRIES: the tile's first row and the offsets that follow it, staged (doc_text.h).  Every thread of the block calls it.
__device__ inline void it_stage(const ItSrc& s, uint64_t tile, uint32_t* win, uint64_t* row0) {
  if (s.what != ISLE_DOCTEXT_ENTRIES) return;
  it_stage_window(s.off, s.row_begin, s.row_end, s.first + tile * MT_TILE, win, row0);
}

// candidate l < nl of the tile (nl = the tile's candidates)
__device__ inline ItLine it_line(const ItSrc& s, uint64_t tile, uint32_t l, uint32_t nl, const uint32_t* win, uint64_t row0) {
  ItLine x;
  const uint64_t at = s.first + tile * MT_TILE + l;
  if (s.what == ISLE_DOCTEXT_ENTRIES) {
    const uint64_t row = it_window_row(s.off, s.row_end, at, l, nl, win, row0);
    x.number = row + s.base;
    x.topic1 = (uint64_t)s.topic[at] + 1u;
    x.w = s.weight[at];
    x.present = true;
  } else {
    const uint64_t row = at / 5u;
    const int i = (int)(at % 5u);
    x.present = true;
    for (int j = 0; j <= i; ++j) x.present = x.present && s.slot[5u * row + j] >= 0;
    x.number = row + s.base;
    x.topic1 = x.present ? (uint64_t)s.slot[at] + 1u : 1u;
    x.w = x.present ? s.weight[at] : 0.f;
  }
  return x;
}
__device__ inline bool it_in_domain(const ItSrc& s, const ItLine& x) {
  return s.base < IT_NUM_END && x.number < IT_NUM_END && x.topic1 < IT_NUM_END && mt_weight_in_domain(x.w);
}
__device__ inline uint32_t it_len(const ItLine& x) {
  return it_line_len((uint32_t)x.number, (uint32_t)x.topic1, x.w);
}

// stat[0] += lines printed; stat[1] = min over the offending printed candidates of L
__global__ __launch_bounds__(MT) void it_count_k(ItSrc src, uint64_t ntiles, uint32_t* __restrict__ sizes, unsigned long long* __restrict__ stat) {
  __shared__ uint32_t win[IT_WIN];
  __shared__ uint64_t row0;
  __shared__ uint32_t shb[MT / ISLE_WAVE], shc[MT / ISLE_WAVE];
  for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint32_t nl = (uint32_t)min((uint64_t)MT_TILE, src.ncand - tile * MT_TILE);
    it_stage(src, tile, win, &row0);
    uint32_t bytes = 0, cnt = 0;
    unsigned long long bad = ~0ull;
#pragma unroll
    for (int i = 0; i < MT_ITEMS; ++i) {
      const uint32_t l = threadIdx.x * MT_ITEMS + i;
      if (l >= nl) break;
      const ItLine x = it_line(src, tile, l, nl, win, row0);
      if (!x.present) continue;
      if (!it_in_domain(src, x)) {
        bad = min(bad, (unsigned long long)(tile * MT_TILE + l));
      } else {
        ++cnt;
        bytes += it_len(x);
      }
    }
    if (bad != ~0ull) atomicMin(&stat[1], bad);
    const uint32_t tb = mt_block_sum(bytes, shb), tc = mt_block_sum(cnt, shc);
    if (threadIdx.x == 0) {
      sizes[tile] = tb;
      if (tc) atomicAdd(&stat[0], (unsigned long long)tc);
    }
  }
}

// tiles [tile0, tile0 + n) -> out[offs[tile] - offs[tile0] ...); out is 16-byte aligned
__global__ __launch_bounds__(MT) void it_write_k(ItSrc src, uint64_t tile0, uint64_t n, const uint64_t* __restrict__ offs, unsigned char* __restrict__ out) {
  __shared__ uint4 lines[MT_LDS_LINES];
  __shared__ uint32_t sh[MT];
  __shared__ uint32_t win[IT_WIN];
  __shared__ uint64_t row0;
  char* const text = reinterpret_cast<char*>(lines);
  const uint64_t base = offs[tile0];
  for (uint64_t tile = tile0 + blockIdx.x; tile < tile0 + n; tile += gridDim.x) {
    const uint64_t dst0 = offs[tile] - base;
    const uint32_t nbytes = (uint32_t)(offs[tile + 1] - offs[tile]);
    if (nbytes == 0) continue;  // the same for every thread of the block
    const uint32_t shift = (uint32_t)(dst0 & 15u);  // LDS position == position in out, modulo 16
    const uint32_t nl = (uint32_t)min((uint64_t)MT_TILE, src.ncand - tile * MT_TILE);
    it_stage(src, tile, win, &row0);
    ItLine x[MT_ITEMS];
    uint32_t mine = 0;
#pragma unroll
    for (int i = 0; i < MT_ITEMS; ++i) {
      const uint32_t l = threadIdx.x * MT_ITEMS + i;
      x[i].present = false;
      if (l < nl) {
        x[i] = it_line(src, tile, l, nl, win, row0);
        if (x[i].present && !it_in_domain(src, x[i])) x[i].present = false;  // (the counting pass has refused such a call)
      }
      if (x[i].present) mine += it_len(x[i]);
    }
    uint32_t total;
    const uint32_t at = isle_scan::block_exclusive<uint32_t>(mine, sh, &total);
    char* p = text + shift + at;
#pragma unroll
    for (int i = 0; i < MT_ITEMS; ++i) {
      if (!x[i].present) continue;
      p = it_put_line(p, (uint32_t)x[i].number, (uint32_t)x[i].topic1, x[i].w);
    }
    mt_store_tile(lines, shift, nbytes, out, dst0);
  }
}

}  // namespace

#define LAUNCH_CHECK(c) HIPCHK(c, hipGetLastError())

int k_infer_text(isle_ctx* c, int what, uint64_t row_begin, uint64_t row_end, uint64_t base, isle_text_sink_fn sink, void* user, uint64_t* nbytes,
                 uint64_t* nlines) {
  if (nbytes) *nbytes = 0;
  if (nlines) *nlines = 0;
  if (row_begin == row_end) return 0;
  ItSrc src{what, c->inf_off.p, c->inf_topic.p, c->inf_top_topic.p, nullptr, row_begin, row_end, 0, 0, base};
  if (what == ISLE_DOCTEXT_ENTRIES) {
    int64_t ends[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(&ends[0], c->inf_off.p + row_begin, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&ends[1], c->inf_off.p + row_end, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    src.weight = c->inf_weight.p;
    src.first = (uint64_t)ends[0];
    src.ncand = (uint64_t)(ends[1] - ends[0]);
  } else {
    src.weight = c->inf_top_weight.p;
    src.first = 5 * row_begin;
    src.ncand = 5 * (row_end - row_begin);
  }
  if (src.ncand == 0) return 0;
  const uint64_t ntiles = (src.ncand + MT_TILE - 1) / MT_TILE;
  if (ntiles >= (1ull << 31)) return isle_fail(c, ISLE_E_ARG, "infer_text: %llu lines are more than 2^31 tiles", (unsigned long long)src.ncand);
  const unsigned cap = (unsigned)c->num_cus * 16u;
  HIPCHK(c, c->mt_sizes.reserve(ntiles));
  HIPCHK(c, c->mt_offs.reserve(ntiles + 1));
  HIPCHK(c, c->mt_blk.reserve(isle_scan::scan_scratch_elems(ntiles)));
  HIPCHK(c, c->mt_stat.reserve(2));
  unsigned long long* stat = (unsigned long long*)c->mt_stat.p;
  const uint64_t init[2] = {0, ~0ull};
  uint64_t h[3] = {0, ~0ull, 0};
  {
    TimeScope ts(c, ISLE_T_INFER);
    HIPCHK(c, hipMemcpyAsync(stat, init, sizeof(init), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(it_count_k, dim3((unsigned)std::min<uint64_t>(ntiles, cap)), dim3(MT), 0, c->stream, src, ntiles, c->mt_sizes.p, stat);
    LAUNCH_CHECK(c);
    HIPCHK(c, (isle_scan::exclusive_scan<uint32_t, uint64_t>(c->stream, c->mt_sizes.p, ntiles, c->mt_offs.p, c->mt_blk.p)));
  }
  HIPCHK(c, hipMemcpyAsync(h, stat, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(h + 2, c->mt_offs.p + ntiles, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (h[1] != ~0ull) {
    // name the line: its row (ENTRIES: a search in the offsets, fetched for this message only), topic and weight
    const uint64_t at = src.first + h[1];
    uint64_t row = at / 5;
    int64_t topic = 0;
    float w = 0.f;
    if (what == ISLE_DOCTEXT_ENTRIES) {
      std::vector<int64_t> off(row_end - row_begin + 1);
      uint32_t t = 0;
      HIPCHK(c, hipMemcpy(off.data(), c->inf_off.p + row_begin, off.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
      HIPCHK(c, hipMemcpy(&t, c->inf_topic.p + at, sizeof(t), hipMemcpyDeviceToHost));
      row = row_begin + (uint64_t)(std::upper_bound(off.begin(), off.end(), (int64_t)at) - off.begin()) - 1;
      topic = t;
    } else {
      int32_t t = 0;
      HIPCHK(c, hipMemcpy(&t, c->inf_top_topic.p + at, sizeof(t), hipMemcpyDeviceToHost));
      topic = t;
    }
    HIPCHK(c, hipMemcpy(&w, src.weight + at, sizeof(w), hipMemcpyDeviceToHost));
    return isle_fail(c, ISLE_E_ARG,
                     "infer_text: the line of row %llu (number %llu), topic %lld (0-based), weight %g is outside the writers' domain: a number >= "
                     "0x7fffffff, or a weight that is negative, infinite or >= 2^31",
                     (unsigned long long)row, (unsigned long long)(row + base), (long long)topic, (double)w);
  }
  const uint64_t total = h[2];
  if (nbytes) *nbytes = total;
  if (nlines) *nlines = h[0];
  if (!sink || total == 0) return 0;
  return k_text_pump(c, "infer_text", c->mt_offs.p, ntiles, total, 1, sink, user, [&](uint64_t t0, uint64_t n, unsigned char* out) -> int {
    TimeScope ts(c, ISLE_T_INFER);
    hipLaunchKernelGGL(it_write_k, dim3((unsigned)std::min<uint64_t>(n, cap)), dim3(MT), 0, c->stream, src, t0, n, c->mt_offs.p, out);
    LAUNCH_CHECK(c);
    return 0;
  });
}

extern "C" int isle_hip_doc_line_text(uint64_t doc_number, uint64_t topic_number, float w, char* out40) {
  if (!out40) return -1;
  out40[0] = 0;
  if (doc_number >= IT_NUM_END || topic_number >= IT_NUM_END || !mt_weight_in_domain(w)) return -1;
  char* p = it_put_line(out40, (uint32_t)doc_number, (uint32_t)topic_number, w);
  *p = 0;
  return (int)(p - out40);
}
