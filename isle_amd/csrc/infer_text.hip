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
// The tiles are counted, placed and written by the skeleton of text_tiles.h, of which ItSrc below is the source.  A candidate is refused
// where it lies outside the writers' domain (a number >= 0x7fffffff, concat_int's assert; a weight that is negative, NaN, infinite or
// >= 2^31).  Nothing resident is written.
#include <algorithm>
#include <vector>

#include "common.h"
#include "doc_text.h"
#include "scan.h"
#include "text_format.h"
#include "text_tiles.h"

#pragma clang fp contract(off)

namespace {

// Where the lines come from.  Other per-document files of the reference (two integers and a weight per line) fit the same descriptor:
// a CSR of (column, value) over the rows, or a fixed number of slots per row.
struct ItSrc {
  static constexpr int kWindow = IT_WIN;
  static constexpr bool kSkipEmpty = false;  // ENTRIES, the windowed kind, prints every candidate
  int what;
  const int64_t* off;       // ENTRIES: offsets of the resident rows (rows + 1), off[0] = 0
  const uint32_t* topic;    // ENTRIES: per entry
  const int32_t* slot;      // TOP: five per row, < 0 = no further topic
  const float* weight;      // ENTRIES: per entry; TOP: five per row
  uint64_t row_begin, row_end;
  uint64_t first;           // ENTRIES: off[row_begin]; TOP: 5 row_begin — candidate L is element first + L
  uint64_t ncand;           // candidates of the call
  uint64_t base;
  struct Tile {
    uint32_t n;
    uint64_t L0;  // the tile's first candidate
  };
  struct Line {
    uint64_t number, topic1;  // as printed; ENTRIES: number is the line's only after place
    float w;
    bool present;
  };
  __device__ Tile open(uint64_t tile) const { return Tile{(uint32_t)min((uint64_t)MT_TILE, ncand - tile * MT_TILE), tile * MT_TILE}; }
  // ENTRIES: the tile's first row and the offsets that follow it, staged (doc_text.h)
  __device__ void stage(const Tile& t, uint32_t* win, uint64_t* row0) const {
    if (what == ISLE_DOCTEXT_ENTRIES) it_stage_window(off, row_begin, row_end, first + t.L0, win, row0);
  }
  __device__ Line probe(const Tile& t, uint32_t l) const {
    Line x;
    const uint64_t at = first + t.L0 + l;
    x.present = true;
    if (what == ISLE_DOCTEXT_ENTRIES) {
      x.number = 0;  // place finds the row
      x.topic1 = (uint64_t)topic[at] + 1u;
      x.w = weight[at];
    } else {
      const uint64_t row = at / 5u;
      const int i = (int)(at % 5u);
      for (int j = 0; j <= i; ++j) x.present = x.present && slot[5u * row + j] >= 0;
      x.number = row + base;
      x.topic1 = x.present ? (uint64_t)slot[at] + 1u : 1u;
      x.w = x.present ? weight[at] : 0.f;
    }
    return x;
  }
  __device__ void place(const Tile& t, uint32_t l, const uint32_t* win, const uint64_t* row0, Line& x) const {
    if (what == ISLE_DOCTEXT_ENTRIES) x.number = it_window_row(off, row_end, first + t.L0 + l, l, t.n, win, *row0) + base;
  }
  __device__ bool in_domain(const Line& x) const {
    return base < IT_NUM_END && x.number < IT_NUM_END && x.topic1 < IT_NUM_END && mt_weight_in_domain(x.w);
  }
  __device__ uint32_t len(const Tile&, uint32_t, const Line& x) const { return it_line_len((uint32_t)x.number, (uint32_t)x.topic1, x.w); }
  __device__ char* put(const Tile&, uint32_t, const Line& x, char* p) const { return it_put_line(p, (uint32_t)x.number, (uint32_t)x.topic1, x.w); }
  __device__ char extra(const Tile&) const { return 0; }
  __device__ uint64_t key(const Tile& t, uint32_t l) const { return t.L0 + l; }
};

}  // namespace

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
  return k_text_tiles(c, "infer_text", ISLE_T_INFER, src, ntiles, 1, sink, user, nbytes, nlines, [&](uint64_t key) -> int {
    // name the line: its row (ENTRIES: a search in the offsets, fetched for this message only), topic and weight
    const uint64_t at = src.first + key;
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
