// isle_amd/csrc/doc_report.hip — the three per-document report files of the trainer formatted on the device, from what
// isle_hip_catchwords / isle_hip_topic_model left resident: ISLETrainer::output_doc_topic's DocCatchword.tsv and
// DocTopicCatchwordSums.tsv (src/trainer.cpp:874-991) and ISLETrainer::print_top_two_topics' TopTwoTopicsPerDoc.txt (:1008-1040), as
// trainer_detail::doc_catchword_text / doc_topic_sums_text / top_two_text (isle_amd/host/trainer_hip.h) restate them.  The lines are
// those of doc_text.h: two integers and a weight (isle_hip_doc_line_text), or three integers (isle_hip_top_two_line_text); every number is
// printed 1-based.
//
// A line is a candidate index L of the call, cut into tiles of MT_TILE = 1024 consecutive candidates (infer_text.hip's scheme):
//   ISLE_DOCREPORT_CATCHWORDS         L = an entry of A in [a_offs[doc_begin], a_offs[doc_end]); printed iff p_catch[a_rows] >= 0 (the
//                                     reference's merge walk beside the column, :946-964: a word is a catchword of at most one topic)
//   ISLE_DOCREPORT_TOPIC_SUMS_BY_DOC  L = an entry of the (document, topic) sums p_dts_* of the documents; every candidate is printed
//   ISLE_DOCREPORT_TOPIC_SUMS         L = a position of those entries' order by topic ascending, then value descending
//                                     (src/sparseMatrix.cpp:715-718); candidate L prints entry perm[L]
//   ISLE_DOCREPORT_TOP_TWO            L = a document; printed iff p_top1 >= 0 and p_top2 >= 0
// The order of TOPIC_SUMS: dr_key_k makes the key (topic << 32) | ~bits(value) of every entry of the range (a value is positive and
// finite, so its bit pattern is monotone) with the entry's index in the range as payload, and k_sort_pairs_u64 (ingest.hip) sorts them
// on 32 + bitlen(k - 1) bits.  The entries lie (document, topic) ascending and the sort is stable, so equal (topic, value) pairs go by
// document ascending; the reference's parallel_sort leaves them in no stated order.  That is the one deviation.
// The document of a CATCHWORDS / TOPIC_SUMS_BY_DOC line comes from the offsets window of doc_text.h.  The document of a TOPIC_SUMS line
// comes from a search of its entry in the global offsets (it_row_of), about log2(documents) dependent loads per line; the alternative, a
// second payload carried through the sort, is NOT measured against it.
// Whether p_catch should be staged in LDS is not measured either (400 KB at 100 k words: it lives in L2); it is read where it lies.
//   dr_count_k   which candidates print (a tile that prints nothing gets the size 0 here and stages no offsets), then bytes per tile,
//                lines printed (64-bit) and the first printed candidate outside the writers' domain (a number >= 0x7fffffff; a weight
//                that is negative, NaN, infinite or >= 2^31)
//   the 64-bit exclusive scan of scan.h
//   dr_write_k   tiles of size 0 are skipped before anything is read; else it_write_k's scheme (lengths, a block scan, the characters
//                into LDS at the tile's alignment modulo 16, mt_store_tile)
// and the text leaves through k_text_pump (model_text.hip).  Nothing resident is written: the sort works in buffers of the call.
#include <algorithm>
#include <vector>

#include "common.h"
#include "doc_text.h"
#include "scan.h"
#include "text_format.h"

#pragma clang fp contract(off)

namespace {

struct DrSrc {
  int what;
  const int64_t* off;      // CATCHWORDS: a_offs; the sums: p_dts_off (documents + 1)
  const uint32_t* col;     // CATCHWORDS: a_rows; the sums: p_dts_topic
  const float* val;        // CATCHWORDS: a_nv; the sums: p_dts_val
  const int32_t* catchw;   // CATCHWORDS: p_catch
  const uint32_t* perm;    // TOPIC_SUMS: candidate L is entry first + perm[L]
  const int32_t *top1, *top2;  // TOP_TWO
  uint64_t row_begin, row_end;
  uint64_t first;          // off[row_begin]; TOP_TWO: row_begin — candidate L is element first + L
  uint64_t ncand;
};
struct DrLine {
  uint64_t a, b, c;  // as printed; c: TOP_TWO only
  float w;
  bool present;
};

__device__ inline bool dr_windowed(const DrSrc& s) { return s.what == ISLE_DOCREPORT_CATCHWORDS || s.what == ISLE_DOCREPORT_TOPIC_SUMS_BY_DOC; }

// candidate L of the call: whether it prints, and everything of its line that needs no row search
__device__ inline DrLine dr_probe(const DrSrc& s, uint64_t L) {
  DrLine x;
  x.a = x.b = x.c = 1u;
  x.w = 0.f;
  if (s.what == ISLE_DOCREPORT_TOP_TWO) {
    const uint64_t row = s.first + L;
    const int32_t t1 = s.top1[row], t2 = s.top2[row];
    x.present = t1 >= 0 && t2 >= 0;
    if (x.present) {
      x.a = row + 1u;
      x.b = (uint64_t)t1 + 1u;
      x.c = (uint64_t)t2 + 1u;
    }
    return x;
  }
  const uint64_t at = s.first + (s.what == ISLE_DOCREPORT_TOPIC_SUMS ? (uint64_t)s.perm[L] : L);
  const uint32_t col = s.col[at];
  x.present = s.what != ISLE_DOCREPORT_CATCHWORDS || s.catchw[col] >= 0;
  if (x.present) {
    x.b = (uint64_t)col + 1u;
    x.w = s.val[at];
  }
  return x;
}
// ... and the document of a printed entry: candidate l < nl of the tile
__device__ inline void dr_place(const DrSrc& s, uint64_t tile, uint32_t l, uint32_t nl, const uint32_t* win, uint64_t row0, DrLine& x) {
  if (dr_windowed(s)) {
    x.a = it_window_row(s.off, s.row_end, s.first + tile * MT_TILE + l, l, nl, win, row0) + 1u;
  } else if (s.what == ISLE_DOCREPORT_TOPIC_SUMS) {
    x.a = it_row_of(s.off, s.row_begin, s.row_end, s.first + (uint64_t)s.perm[tile * MT_TILE + l]) + 1u;
  }
}
__device__ inline bool dr_in_domain(const DrSrc& s, const DrLine& x) {
  return x.a < IT_NUM_END && x.b < IT_NUM_END && x.c < IT_NUM_END && mt_weight_in_domain(x.w);
}
__device__ inline uint32_t dr_len(const DrSrc& s, const DrLine& x) {
  return s.what == ISLE_DOCREPORT_TOP_TWO ? it_line3_len((uint32_t)x.a, (uint32_t)x.b, (uint32_t)x.c) : it_line_len((uint32_t)x.a, (uint32_t)x.b, x.w);
}

// key[i] = (topic << 32) | ~bits(value) of entry first + i, payload i
__global__ __launch_bounds__(MT) void dr_key_k(const uint32_t* __restrict__ topic, const float* __restrict__ val, uint64_t first, uint64_t n,
                                               uint64_t* __restrict__ key, uint32_t* __restrict__ idx) {
  for (uint64_t i = (uint64_t)blockIdx.x * MT + threadIdx.x; i < n; i += (uint64_t)gridDim.x * MT) {
    key[i] = ((uint64_t)topic[first + i] << 32) | (uint64_t)(~__float_as_uint(val[first + i]));
    idx[i] = (uint32_t)i;
  }
}

// stat[0] += lines printed; stat[1] = min over the offending printed candidates of L
__global__ __launch_bounds__(MT) void dr_count_k(DrSrc src, uint64_t ntiles, uint32_t* __restrict__ sizes, unsigned long long* __restrict__ stat) {
  __shared__ uint32_t win[IT_WIN];
  __shared__ uint64_t row0;
  __shared__ uint32_t shb[MT / ISLE_WAVE], shc[MT / ISLE_WAVE];
  for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint32_t nl = (uint32_t)min((uint64_t)MT_TILE, src.ncand - tile * MT_TILE);
    DrLine x[MT_ITEMS];
    uint32_t cand = 0;
#pragma unroll
    for (int i = 0; i < MT_ITEMS; ++i) {
      const uint32_t l = threadIdx.x * MT_ITEMS + i;
      x[i].present = false;
      if (l < nl) x[i] = dr_probe(src, tile * MT_TILE + l);
      cand += x[i].present ? 1u : 0u;
    }
    if (mt_block_sum(cand, shc) == 0) {  // the same for every thread of the block: nothing to place, nothing to store
      if (threadIdx.x == 0) sizes[tile] = 0;
      continue;
    }
    if (dr_windowed(src)) it_stage_window(src.off, src.row_begin, src.row_end, src.first + tile * MT_TILE, win, &row0);
    uint32_t bytes = 0, cnt = 0;
    unsigned long long bad = ~0ull;
#pragma unroll
    for (int i = 0; i < MT_ITEMS; ++i) {
      if (!x[i].present) continue;
      const uint32_t l = threadIdx.x * MT_ITEMS + i;
      dr_place(src, tile, l, nl, win, row0, x[i]);
      if (!dr_in_domain(src, x[i])) {
        bad = min(bad, (unsigned long long)(tile * MT_TILE + l));
      } else {
        ++cnt;
        bytes += dr_len(src, x[i]);
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
__global__ __launch_bounds__(MT) void dr_write_k(DrSrc src, uint64_t tile0, uint64_t n, const uint64_t* __restrict__ offs, unsigned char* __restrict__ out) {
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
    if (dr_windowed(src)) it_stage_window(src.off, src.row_begin, src.row_end, src.first + tile * MT_TILE, win, &row0);
    DrLine x[MT_ITEMS];
    uint32_t mine = 0;
#pragma unroll
    for (int i = 0; i < MT_ITEMS; ++i) {
      const uint32_t l = threadIdx.x * MT_ITEMS + i;
      x[i].present = false;
      if (l < nl) {
        x[i] = dr_probe(src, tile * MT_TILE + l);
        if (x[i].present) {
          dr_place(src, tile, l, nl, win, row0, x[i]);
          if (!dr_in_domain(src, x[i])) x[i].present = false;  // (the counting pass has refused such a call)
        }
      }
      if (x[i].present) mine += dr_len(src, x[i]);
    }
    uint32_t total;
    const uint32_t at = isle_scan::block_exclusive<uint32_t>(mine, sh, &total);
    char* p = text + shift + at;
#pragma unroll
    for (int i = 0; i < MT_ITEMS; ++i) {
      if (!x[i].present) continue;
      p = src.what == ISLE_DOCREPORT_TOP_TWO ? it_put_line3(p, (uint32_t)x[i].a, (uint32_t)x[i].b, (uint32_t)x[i].c)
                                             : it_put_line(p, (uint32_t)x[i].a, (uint32_t)x[i].b, x[i].w);
    }
    mt_store_tile(lines, shift, nbytes, out, dst0);
  }
}

const char* dr_name(int what) {
  switch (what) {
    case ISLE_DOCREPORT_CATCHWORDS: return "catchwords";
    case ISLE_DOCREPORT_TOPIC_SUMS: return "topic_sums";
    case ISLE_DOCREPORT_TOPIC_SUMS_BY_DOC: return "topic_sums_by_doc";
    default: return "top_two";
  }
}

}  // namespace

#define LAUNCH_CHECK(c) HIPCHK(c, hipGetLastError())

int k_doc_report_text(isle_ctx* c, int what, uint64_t doc_begin, uint64_t doc_end, isle_text_sink_fn sink, void* user, uint64_t* nbytes,
                      uint64_t* nlines) {
  if (nbytes) *nbytes = 0;
  if (nlines) *nlines = 0;
  if (doc_begin == doc_end) return 0;
  DrSrc src{what, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, doc_begin, doc_end, 0, 0};
  if (what == ISLE_DOCREPORT_TOP_TWO) {
    src.top1 = c->p_top1.p;
    src.top2 = c->p_top2.p;
    src.first = doc_begin;
    src.ncand = doc_end - doc_begin;
  } else {
    if (what == ISLE_DOCREPORT_CATCHWORDS) {
      src.off = c->a_offs.p;
      src.col = c->a_rows.p;
      src.val = c->a_nv.p;
      src.catchw = c->p_catch.p;
    } else {
      src.off = c->p_dts_off.p;
      src.col = c->p_dts_topic.p;
      src.val = c->p_dts_val.p;
    }
    int64_t ends[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(&ends[0], src.off + doc_begin, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&ends[1], src.off + doc_end, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    src.first = (uint64_t)ends[0];
    src.ncand = (uint64_t)(ends[1] - ends[0]);
  }
  if (src.ncand == 0) return 0;
  const uint64_t ntiles = (src.ncand + MT_TILE - 1) / MT_TILE;
  if (ntiles >= (1ull << 31))
    return isle_fail(c, ISLE_E_ARG, "doc_report_text(%s): %llu candidate lines are more than 2^31 tiles", dr_name(what), (unsigned long long)src.ncand);
  const unsigned cap = (unsigned)c->num_cus * 16u;
  // the order of TOPIC_SUMS, in buffers of this call (freed on return, behind the pump's synchronisation)
  DevBuf<uint64_t> key_a, key_b;
  DevBuf<uint32_t> idx_a, idx_b;
  if (what == ISLE_DOCREPORT_TOPIC_SUMS) {
    if (src.ncand >= (1ull << 32))
      return isle_fail(c, ISLE_E_ARG, "doc_report_text(topic_sums): %llu sums in one range; the order's payload is 32 bits wide — write the range in parts",
                       (unsigned long long)src.ncand);
    int key_bits = 32;
    for (uint32_t t = c->p_k > 1 ? (uint32_t)c->p_k - 1u : 0u; t; t >>= 1) ++key_bits;
    HIPCHK(c, key_a.reserve(src.ncand));
    HIPCHK(c, key_b.reserve(src.ncand));
    HIPCHK(c, idx_a.reserve(src.ncand));
    HIPCHK(c, idx_b.reserve(src.ncand));
    TimeScope ts(c, ISLE_T_POST);
    hipLaunchKernelGGL(dr_key_k, dim3((unsigned)std::min<uint64_t>((src.ncand + MT - 1) / MT, cap)), dim3(MT), 0, c->stream, src.col, src.val, src.first,
                       src.ncand, key_a.p, idx_a.p);
    LAUNCH_CHECK(c);
    bool in_a = true;
    ISLECHK(k_sort_pairs_u64(c, key_a.p, idx_a.p, key_b.p, idx_b.p, src.ncand, key_bits, &in_a));
    src.perm = in_a ? idx_a.p : idx_b.p;
  }
  HIPCHK(c, c->mt_sizes.reserve(ntiles));
  HIPCHK(c, c->mt_offs.reserve(ntiles + 1));
  HIPCHK(c, c->mt_blk.reserve(isle_scan::scan_scratch_elems(ntiles)));
  HIPCHK(c, c->mt_stat.reserve(2));
  unsigned long long* stat = (unsigned long long*)c->mt_stat.p;
  const uint64_t init[2] = {0, ~0ull};
  uint64_t h[3] = {0, ~0ull, 0};
  {
    TimeScope ts(c, ISLE_T_POST);
    HIPCHK(c, hipMemcpyAsync(stat, init, sizeof(init), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(dr_count_k, dim3((unsigned)std::min<uint64_t>(ntiles, cap)), dim3(MT), 0, c->stream, src, ntiles, c->mt_sizes.p, stat);
    LAUNCH_CHECK(c);
    HIPCHK(c, (isle_scan::exclusive_scan<uint32_t, uint64_t>(c->stream, c->mt_sizes.p, ntiles, c->mt_offs.p, c->mt_blk.p)));
  }
  HIPCHK(c, hipMemcpyAsync(h, stat, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(h + 2, c->mt_offs.p + ntiles, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (h[1] != ~0ull) {
    // name the line (its document: a search in the offsets, fetched for this message only)
    uint64_t doc = src.first + h[1];
    if (what == ISLE_DOCREPORT_TOP_TWO) {
      int32_t t[2] = {0, 0};
      HIPCHK(c, hipMemcpy(&t[0], src.top1 + doc, sizeof(int32_t), hipMemcpyDeviceToHost));
      HIPCHK(c, hipMemcpy(&t[1], src.top2 + doc, sizeof(int32_t), hipMemcpyDeviceToHost));
      return isle_fail(c, ISLE_E_ARG, "doc_report_text(top_two): the line of document %llu, topics %d and %d (0-based) is outside the writers' domain: a number >= 0x7fffffff",
                       (unsigned long long)doc, (int)t[0], (int)t[1]);
    }
    uint64_t at = src.first + h[1];
    if (what == ISLE_DOCREPORT_TOPIC_SUMS) {
      uint32_t e = 0;
      HIPCHK(c, hipMemcpy(&e, src.perm + h[1], sizeof(e), hipMemcpyDeviceToHost));
      at = src.first + e;
    }
    std::vector<int64_t> off(doc_end - doc_begin + 1);
    uint32_t col = 0;
    float w = 0.f;
    HIPCHK(c, hipMemcpy(off.data(), src.off + doc_begin, off.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(&col, src.col + at, sizeof(col), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(&w, src.val + at, sizeof(w), hipMemcpyDeviceToHost));
    doc = doc_begin + (uint64_t)(std::upper_bound(off.begin(), off.end(), (int64_t)at) - off.begin()) - 1;
    return isle_fail(c, ISLE_E_ARG,
                     "doc_report_text(%s): the line of document %llu, %s %u (0-based), value %g is outside the writers' domain: a number >= 0x7fffffff, "
                     "or a weight that is negative, NaN, infinite or >= 2^31",
                     dr_name(what), (unsigned long long)doc, what == ISLE_DOCREPORT_CATCHWORDS ? "word" : "topic", col, (double)w);
  }
  const uint64_t total = h[2];
  if (nbytes) *nbytes = total;
  if (nlines) *nlines = h[0];
  if (!sink || total == 0) return 0;
  return k_text_pump(c, "doc_report_text", c->mt_offs.p, ntiles, total, 1, sink, user, [&](uint64_t t0, uint64_t n, unsigned char* out) -> int {
    TimeScope ts(c, ISLE_T_POST);
    hipLaunchKernelGGL(dr_write_k, dim3((unsigned)std::min<uint64_t>(n, cap)), dim3(MT), 0, c->stream, src, t0, n, c->mt_offs.p, out);
    LAUNCH_CHECK(c);
    return 0;
  });
}

extern "C" int isle_hip_top_two_line_text(uint64_t doc_number, uint64_t t1_number, uint64_t t2_number, char* out40) {
  if (!out40) return -1;
  out40[0] = 0;
  if (doc_number >= IT_NUM_END || t1_number >= IT_NUM_END || t2_number >= IT_NUM_END) return -1;
  char* p = it_put_line3(out40, (uint32_t)doc_number, (uint32_t)t1_number, (uint32_t)t2_number);
  *p = 0;
  return (int)(p - out40);
}
