// isle_amd/csrc/doc_text.h — what the per-document text formatters (infer_text.hip, doc_report.hip) share: the row of a CSR entry that
// does not store it (a search in the global offsets, or in a window of offsets staged per tile), and the two kinds of lines, host and
// device: "<number>\t<number>\t<weight>\n" (isle_hip_doc_line_text) and "<number>\t<number>\t<number>\n" (isle_hip_top_two_line_text).
// The integers are MMappedOutput::concat_int's plain decimals, the weight is mt_weight (text_format.h).
#pragma once
#include "text_format.h"

#pragma clang fp contract(off)

constexpr int IT_WIN = 1024;                    // offsets staged per tile
constexpr uint64_t IT_NUM_END = 0x7fffffffull;  // concat_int: assert(num < 0x7fffffff)
static_assert(10 + 1 + 10 + 1 + 13 + 1 <= MT_MAX_ENTRY, "a line fits the LDS budget of a tile");
static_assert(10 + 1 + 10 + 1 + 10 + 1 <= MT_MAX_ENTRY, "a line of three integers fits it too");

// ---- the lines: lengths and characters for numbers inside the writers' domain ----
__host__ __device__ inline uint32_t it_line_len(uint32_t a, uint32_t b, float w) {
  return (uint32_t)(mt_ndigits(a) + 1 + mt_ndigits(b) + 1 + mt_whole_digits(w) + 7 + 1);
}
__host__ __device__ inline char* it_put_line(char* p, uint32_t a, uint32_t b, float w) {
  p = mt_put_uint(p, a, mt_ndigits(a));
  *p++ = '\t';
  p = mt_put_uint(p, b, mt_ndigits(b));
  *p++ = '\t';
  p = mt_weight(w, p);
  *p++ = '\n';
  return p;
}
__host__ __device__ inline uint32_t it_line3_len(uint32_t a, uint32_t b, uint32_t c) {
  return (uint32_t)(mt_ndigits(a) + 1 + mt_ndigits(b) + 1 + mt_ndigits(c) + 1);
}
__host__ __device__ inline char* it_put_line3(char* p, uint32_t a, uint32_t b, uint32_t c) {
  p = mt_put_uint(p, a, mt_ndigits(a));
  *p++ = '\t';
  p = mt_put_uint(p, b, mt_ndigits(b));
  *p++ = '\t';
  p = mt_put_uint(p, c, mt_ndigits(c));
  *p++ = '\n';
  return p;
}

#if defined(__HIPCC__)
// the row r of [lo, hi) with off[r] <= e < off[r + 1]; the caller knows off[lo] <= e < off[hi]
__device__ inline uint64_t it_row_of(const int64_t* __restrict__ off, uint64_t lo, uint64_t hi, uint64_t e) {
  while (hi - lo > 1) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if ((uint64_t)off[mid] <= e) lo = mid;
    else hi = mid;
  }
  return lo;
}

// A tile of MT_TILE consecutive entries that begins at entry e0 of rows [row_begin, row_end): the tile's first row into *row0 and
// win[j] = min(off[row0 + 1 + j] - e0, MT_TILE), j < IT_WIN (MT_TILE beyond row_end).  Every thread of the block calls it.
__device__ inline void it_stage_window(const int64_t* __restrict__ off, uint64_t row_begin, uint64_t row_end, uint64_t e0, uint32_t* win,
                                       uint64_t* row0) {
  __syncthreads();  // the previous tile's searches are over
  if (threadIdx.x == 0) *row0 = it_row_of(off, row_begin, row_end, e0);
  __syncthreads();
  const uint64_t r0 = *row0;
  for (int j = threadIdx.x; j < IT_WIN; j += MT) {
    const uint64_t r = r0 + 1 + (uint64_t)j;
    win[j] = r <= row_end ? (uint32_t)min((uint64_t)off[r] - e0, (uint64_t)MT_TILE) : (uint32_t)MT_TILE;
  }
  __syncthreads();
}

// the row of entry `at` = e0 + l, l < nl (the tile's entries), after it_stage_window: the rows before the first staged offset > l where
// the window reaches beyond the tile, else (a run of empty rows longer than the window) a search in the global offsets
__device__ inline uint64_t it_window_row(const int64_t* __restrict__ off, uint64_t row_end, uint64_t at, uint32_t l, uint32_t nl, const uint32_t* win,
                                         uint64_t row0) {
  if (win[IT_WIN - 1] >= nl) {
    uint32_t lo = 0, n = IT_WIN;
    while (n) {  // upper bound of l
      const uint32_t h = n >> 1;
      if (win[lo + h] <= l) {
        lo += h + 1;
        n -= h + 1;
      } else {
        n = h;
      }
    }
    return row0 + lo;
  }
  return it_row_of(off, row0, row_end, at);
}
#endif
