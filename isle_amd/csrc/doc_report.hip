// isle_amd/csrc/doc_report.hip — the three per-document report files of the trainer formatted on the device, from what
// isle_hip_catchwords / isle_hip_topic_model left resident: ISLETrainer::output_doc_topic's DocCatchword.tsv and
// DocTopicCatchwordSums.tsv (src/trainer.cpp:874-991) and ISLETrainer::print_top_two_topics' TopTwoTopicsPerDoc.txt (:1008-1040), as
// trainer_detail::doc_catchword_text / doc_topic_sums_text / top_two_text (isle_amd/host/trainer_hip.h) restate them.  The lines are
// those of doc_text.h: two integers and a weight (isle_hip_doc_line_text), or three integers (isle_hip_top_two_line_text); every number is
// printed 1-based.
//
// A line is a candidate index L of the call, cut into tiles of MT_TILE = 1024 consecutive candidates:
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
// The tiles are counted, placed and written by the skeleton of text_tiles.h, of which DrSrc below is the source: its probe says which
// candidates print, so a tile that prints nothing stages no offsets.  A printed candidate is refused where it lies outside the writers'
// domain (a number >= 0x7fffffff; a weight that is negative, NaN, infinite or >= 2^31).  Nothing resident is written: the sort works in
// buffers of the call.
//
// Document shards (world > 1, stage_host.h / route_host.h): the document printed is doc_base + doc + 1, doc_base = the shard's first document
// in the corpus (DrSrc::doc_base; 0 with one rank, whatever the upload said), and the domain check is on that number.  CATCHWORDS,
// TOPIC_SUMS_BY_DOC and TOP_TWO need nothing of another rank.  TOPIC_SUMS is one order over all ranks' sums (route_topic_sums ==
// TOPIC_SUMS_GATHERED; the collectives are api_stages.cpp's, the steps k_dr_sums_* below): dr_key_doc_k makes the same keys with the GLOBAL
// document as payload, the ranks' counts and then their keys and documents are all-gathered in blocks padded to the largest count and
// compacted in rank order into L pairs, the same stable sort runs replicated (rank order is document order: ties go by document ascending,
// as on one rank), and rank q formats the lines [topic_sums_slice(L, W, q), topic_sums_slice(L, W, q + 1)) through DrGatherSrc: no row
// search, no offsets window.  Every collective of the call precedes its first sink call, and every count that shapes one comes from gathered
// data.  NOT measured: the device memory of this form ((W + 1) nmax 12 bytes and the sort's twin), and any time at N > 1.
#include <algorithm>
#include <cstring>
#include <vector>

#include "common.h"
#include "doc_text.h"
#include "scan.h"
#include "text_format.h"
#include "text_tiles.h"

#pragma clang fp contract(off)

namespace {

struct DrSrc {
  static constexpr int kWindow = IT_WIN;
  static constexpr bool kSkipEmpty = true;  // most entries of A are no catchwords
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
  uint64_t doc_base;       // the shard's first document in the corpus; 0 with one rank
  struct Tile {
    uint32_t n;
    uint64_t L0;  // the tile's first candidate
  };
  struct Line {
    uint64_t a, b, c;  // as printed; c: TOP_TWO only
    float w;
    bool present;
  };
  __device__ bool windowed() const { return what == ISLE_DOCREPORT_CATCHWORDS || what == ISLE_DOCREPORT_TOPIC_SUMS_BY_DOC; }
  __device__ Tile open(uint64_t tile) const { return Tile{(uint32_t)min((uint64_t)MT_TILE, ncand - tile * MT_TILE), tile * MT_TILE}; }
  __device__ void stage(const Tile& t, uint32_t* win, uint64_t* row0) const {
    if (windowed()) it_stage_window(off, row_begin, row_end, first + t.L0, win, row0);
  }
  // whether the candidate prints, and everything of its line that needs no row search
  __device__ Line probe(const Tile& t, uint32_t l) const {
    Line x;
    x.a = x.b = x.c = 1u;
    x.w = 0.f;
    if (what == ISLE_DOCREPORT_TOP_TWO) {
      const uint64_t row = first + t.L0 + l;
      const int32_t t1 = top1[row], t2 = top2[row];
      x.present = t1 >= 0 && t2 >= 0;
      if (x.present) {
        x.a = doc_base + row + 1u;
        x.b = (uint64_t)t1 + 1u;
        x.c = (uint64_t)t2 + 1u;
      }
      return x;
    }
    const uint64_t at = first + (what == ISLE_DOCREPORT_TOPIC_SUMS ? (uint64_t)perm[t.L0 + l] : t.L0 + l);
    const uint32_t cl = col[at];
    x.present = what != ISLE_DOCREPORT_CATCHWORDS || catchw[cl] >= 0;
    if (x.present) {
      x.b = (uint64_t)cl + 1u;
      x.w = val[at];
    }
    return x;
  }
  // ... and the document of a printed entry
  __device__ void place(const Tile& t, uint32_t l, const uint32_t* win, const uint64_t* row0, Line& x) const {
    if (windowed()) {
      x.a = doc_base + it_window_row(off, row_end, first + t.L0 + l, l, t.n, win, *row0) + 1u;
    } else if (what == ISLE_DOCREPORT_TOPIC_SUMS) {
      x.a = doc_base + it_row_of(off, row_begin, row_end, first + (uint64_t)perm[t.L0 + l]) + 1u;
    }
  }
  __device__ bool in_domain(const Line& x) const { return x.a < IT_NUM_END && x.b < IT_NUM_END && x.c < IT_NUM_END && mt_weight_in_domain(x.w); }
  __device__ uint32_t len(const Tile&, uint32_t, const Line& x) const {
    return what == ISLE_DOCREPORT_TOP_TWO ? it_line3_len((uint32_t)x.a, (uint32_t)x.b, (uint32_t)x.c) : it_line_len((uint32_t)x.a, (uint32_t)x.b, x.w);
  }
  __device__ char* put(const Tile&, uint32_t, const Line& x, char* p) const {
    return what == ISLE_DOCREPORT_TOP_TWO ? it_put_line3(p, (uint32_t)x.a, (uint32_t)x.b, (uint32_t)x.c) : it_put_line(p, (uint32_t)x.a, (uint32_t)x.b, x.w);
  }
  __device__ char extra(const Tile&) const { return 0; }
  __device__ uint64_t key(const Tile& t, uint32_t l) const { return t.L0 + l; }
};

// key[i] = (topic << 32) | ~bits(value) of entry first + i, payload i
__global__ __launch_bounds__(MT) void dr_key_k(const uint32_t* __restrict__ topic, const float* __restrict__ val, uint64_t first, uint64_t n,
                                               uint64_t* __restrict__ key, uint32_t* __restrict__ idx) {
  for (uint64_t i = (uint64_t)blockIdx.x * MT + threadIdx.x; i < n; i += (uint64_t)gridDim.x * MT) {
    key[i] = ((uint64_t)topic[first + i] << 32) | (uint64_t)(~__float_as_uint(val[first + i]));
    idx[i] = (uint32_t)i;
  }
}

// The gathered form's keys: the same key, the payload the entry's document in the corpus (saturated at 2^32 - 1, which the writers refuse)
__global__ __launch_bounds__(MT) void dr_key_doc_k(const int64_t* __restrict__ off, const uint32_t* __restrict__ topic, const float* __restrict__ val,
                                                   uint64_t row_begin, uint64_t row_end, uint64_t first, uint64_t n, uint64_t doc_base,
                                                   uint64_t* __restrict__ key, uint32_t* __restrict__ doc) {
  for (uint64_t i = (uint64_t)blockIdx.x * MT + threadIdx.x; i < n; i += (uint64_t)gridDim.x * MT) {
    key[i] = ((uint64_t)topic[first + i] << 32) | (uint64_t)(~__float_as_uint(val[first + i]));
    const uint64_t g = doc_base + it_row_of(off, row_begin, row_end, first + i);
    doc[i] = g > 0xffffffffull ? 0xffffffffu : (uint32_t)g;
  }
}

// The lines of the gathered form: candidate l of the call is pair first + l of the corpus's sorted (key, document) pairs
struct DrGatherSrc {
  static constexpr int kWindow = 0;
  static constexpr bool kSkipEmpty = false;
  const uint64_t* keys;
  const uint32_t* docs;
  uint64_t first, ncand;
  struct Tile {
    uint32_t n;
    uint64_t L0;  // the tile's first candidate
  };
  struct Line {
    uint64_t a, b;
    float w;
    bool present;
  };
  __device__ Tile open(uint64_t tile) const { return Tile{(uint32_t)min((uint64_t)MT_TILE, ncand - tile * MT_TILE), tile * MT_TILE}; }
  __device__ Line probe(const Tile& t, uint32_t l) const {
    const uint64_t kv = keys[first + t.L0 + l];
    return Line{(uint64_t)docs[first + t.L0 + l] + 1u, (kv >> 32) + 1u, __uint_as_float(~(uint32_t)kv), true};
  }
  __device__ void place(const Tile&, uint32_t, const uint32_t*, const uint64_t*, Line&) const {}
  __device__ bool in_domain(const Line& x) const { return x.a < IT_NUM_END && x.b < IT_NUM_END && mt_weight_in_domain(x.w); }
  __device__ uint32_t len(const Tile&, uint32_t, const Line& x) const { return it_line_len((uint32_t)x.a, (uint32_t)x.b, x.w); }
  __device__ char* put(const Tile&, uint32_t, const Line& x, char* p) const { return it_put_line(p, (uint32_t)x.a, (uint32_t)x.b, x.w); }
  __device__ char extra(const Tile&) const { return 0; }
  __device__ uint64_t key(const Tile& t, uint32_t l) const { return t.L0 + l; }
};

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

static int key_bits_of(int k) {
  int key_bits = 32;
  for (uint32_t t = k > 1 ? (uint32_t)k - 1u : 0u; t; t >>= 1) ++key_bits;
  return key_bits;
}

// ---- ISLE_DOCREPORT_TOPIC_SUMS over document shards: the device steps between the collectives of api_stages.cpp (TopicSumsGather) ----
// the sums of documents [doc_begin, doc_end): the first entry and their number
int k_dr_sums_range(isle_ctx* c, uint64_t doc_begin, uint64_t doc_end, uint64_t* first, uint64_t* n) {
  *first = *n = 0;
  if (doc_begin == doc_end) return 0;
  int64_t ends[2] = {0, 0};
  HIPCHK(c, hipMemcpyAsync(&ends[0], c->p_dts_off.p + doc_begin, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(&ends[1], c->p_dts_off.p + doc_end, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *first = (uint64_t)ends[0];
  *n = (uint64_t)(ends[1] - ends[0]);
  return 0;
}

// this rank's block of nmax >= n (key, document) pairs: the n pairs of its sums, then zeros (the padding travels: the same bytes every time)
int k_dr_sums_keys(isle_ctx* c, uint64_t doc_begin, uint64_t doc_end, uint64_t first, uint64_t n, uint64_t nmax, uint64_t* key, uint32_t* doc) {
  TimeScope ts(c, ISLE_T_POST);
  HIPCHK(c, hipMemsetAsync(key, 0, nmax * sizeof(uint64_t), c->stream));
  HIPCHK(c, hipMemsetAsync(doc, 0, nmax * sizeof(uint32_t), c->stream));
  if (n == 0) return 0;
  const unsigned cap = (unsigned)c->num_cus * 16u;
  hipLaunchKernelGGL(dr_key_doc_k, dim3((unsigned)std::min<uint64_t>((n + MT - 1) / MT, cap)), dim3(MT), 0, c->stream, c->p_dts_off.p, c->p_dts_topic.p,
                     c->p_dts_val.p, doc_begin, doc_end, first, n, c->a_doc_offset, key, doc);
  LAUNCH_CHECK(c);
  return 0;
}

// The L pairs of the corpus in rank order (key_a / doc_a; key_b / doc_b: the sort's twin) sorted replicated, then lines [L0, L1) of the
// corpus's file formatted.  No collective from here on: a refusal of this rank's sink or slice leaves no other rank waiting.
int k_dr_sums_gathered_text(isle_ctx* c, uint64_t* key_a, uint32_t* doc_a, uint64_t* key_b, uint32_t* doc_b, uint64_t L, uint64_t L0, uint64_t L1,
                            isle_text_sink_fn sink, void* user, uint64_t* nbytes, uint64_t* nlines) {
  bool in_a = true;
  {
    TimeScope ts(c, ISLE_T_POST);
    ISLECHK(k_sort_pairs_u64(c, key_a, doc_a, key_b, doc_b, L, key_bits_of(c->res.p_k), &in_a));
  }
  if (L1 == L0) return 0;
  const DrGatherSrc src{in_a ? key_a : key_b, in_a ? doc_a : doc_b, L0, L1 - L0};
  const uint64_t ntiles = (src.ncand + MT_TILE - 1) / MT_TILE;  // fewer than 2^22: L < 2^32
  return k_text_tiles(c, "doc_report_text", ISLE_T_POST, src, ntiles, 1, sink, user, nbytes, nlines, [&](uint64_t key) -> int {
    uint64_t kv = 0;
    uint32_t doc = 0;
    HIPCHK(c, hipMemcpy(&kv, src.keys + src.first + key, sizeof(kv), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(&doc, src.docs + src.first + key, sizeof(doc), hipMemcpyDeviceToHost));
    const uint32_t bits = ~(uint32_t)kv;
    float w;
    memcpy(&w, &bits, sizeof(w));
    return isle_fail(c, ISLE_E_ARG,
                     "doc_report_text(topic_sums): line %llu of the corpus's order, document %llu of the corpus (0-based; 4294967295: that or beyond), "
                     "topic %llu (0-based), value %g is outside the writers' domain: a number >= 0x7fffffff, or a weight that is negative, NaN, infinite or >= 2^31",
                     (unsigned long long)(src.first + key), (unsigned long long)doc, (unsigned long long)(kv >> 32), (double)w);
  });
}

int k_doc_report_text(isle_ctx* c, int what, uint64_t doc_begin, uint64_t doc_end, isle_text_sink_fn sink, void* user, uint64_t* nbytes,
                      uint64_t* nlines) {
  if (nbytes) *nbytes = 0;
  if (nlines) *nlines = 0;
  if (doc_begin == doc_end) return 0;
  const uint64_t doc_base = c->world > 1 ? c->a_doc_offset : 0;  // one rank: the bytes of a context without a communicator, whatever the upload said
  DrSrc src{what, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, doc_begin, doc_end, 0, 0, doc_base};
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
    const int key_bits = key_bits_of(c->res.p_k);
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
  return k_text_tiles(c, "doc_report_text", ISLE_T_POST, src, ntiles, 1, sink, user, nbytes, nlines, [&](uint64_t key) -> int {
    // name the line (its document: a search in the offsets, fetched for this message only)
    uint64_t doc = src.first + key;
    if (what == ISLE_DOCREPORT_TOP_TWO) {
      int32_t t[2] = {0, 0};
      HIPCHK(c, hipMemcpy(&t[0], src.top1 + doc, sizeof(int32_t), hipMemcpyDeviceToHost));
      HIPCHK(c, hipMemcpy(&t[1], src.top2 + doc, sizeof(int32_t), hipMemcpyDeviceToHost));
      return isle_fail(c, ISLE_E_ARG,
                       "doc_report_text(top_two): the line of document %llu (document %llu of the corpus), topics %d and %d (0-based) is outside the writers' "
                       "domain: a number >= 0x7fffffff",
                       (unsigned long long)doc, (unsigned long long)(doc_base + doc), (int)t[0], (int)t[1]);
    }
    uint64_t at = src.first + key;
    if (what == ISLE_DOCREPORT_TOPIC_SUMS) {
      uint32_t e = 0;
      HIPCHK(c, hipMemcpy(&e, src.perm + key, sizeof(e), hipMemcpyDeviceToHost));
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
                     "doc_report_text(%s): the line of document %llu (document %llu of the corpus), %s %u (0-based), value %g is outside the writers' domain: a "
                     "number >= 0x7fffffff, or a weight that is negative, NaN, infinite or >= 2^31",
                     dr_name(what), (unsigned long long)doc, (unsigned long long)(doc_base + doc), what == ISLE_DOCREPORT_CATCHWORDS ? "word" : "topic", col, (double)w);
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
