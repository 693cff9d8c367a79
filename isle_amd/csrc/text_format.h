// isle_amd/csrc/text_format.h — what the text formatters (model_text.hip, infer_text.hip, doc_report.hip) share below their count and
// write kernels (model_text.hip's own, text_tiles.h for the other two): the library's one copy of the digit rule (mt_weight, host and
// device), the decimal integers of MMappedOutput::concat_int, the tile geometry, the block sum and the way a tile leaves LDS as whole
// 16-byte lines.  The chunk pump they all deliver through is k_text_pump (model_text.hip, common.h).
//
// Floating-point contraction: hipcc contracts a * b - c into an fma by default, which would take the fraction digits from an unrounded
// product, and this toolchain's __fmul_rn / __fsub_rn are plain operators that contract all the same (seen in the ISA).  Contraction is
// therefore switched off from here to the end of every file that includes this header, host and device; the including .hip files say
// so again below their includes.
#pragma once
#include <algorithm>
#include <cstdint>

#include "common.h"
#include "scan.h"

#pragma clang fp contract(off)

constexpr int MT = isle_scan::SCAN_T;  // 256: block_exclusive's width
constexpr int MT_ITEMS = 4;            // consecutive rows (lines) per thread
constexpr int MT_TILE = MT * MT_ITEMS;
constexpr int MT_MAX_ENTRY = 36;       // "<number <= 2^31>\t<number < 2^32>\t<6>.<6>\n" = 10 + 1 + 10 + 1 + 13 + 1
constexpr int MT_LDS_LINES = (MT_TILE * MT_MAX_ENTRY + 15 /*alignment shift*/ + 1 /*dense '\n'*/ + 15) / 16;

__host__ __device__ inline int mt_ndigits(uint32_t v) {
  return 1 + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u) + (v >= 100000000u) +
         (v >= 1000000000u);
}
__host__ __device__ inline char* mt_put_uint(char* out, uint32_t v, int nd) {  // the nd low digits of v
  char* q = out + nd;
  for (int i = 0; i < nd; ++i) {
    *--q = (char)('0' + v % 10u);
    v /= 10u;
  }
  return out + nd;
}
__host__ __device__ inline bool mt_weight_in_domain(float w) { return w >= 0.0f && w < 2147483648.0f; }  // (int)w / (unsigned)w are defined
__host__ __device__ inline int mt_whole_digits(float w) { return std::min(6, mt_ndigits((uint32_t)w)); }  // inside the domain only

// trainer_detail::weight_text for an entry inside the domain: at most the six low digits of (unsigned)w, '.', six fraction digits peeled
// off the fp32 remainder by separately rounded multiply and subtract (no contraction in this file).  Returns the end.
__host__ __device__ inline char* mt_weight(float w, char* out) {
  const uint32_t whole = (uint32_t)w;
  out = mt_put_uint(out, whole % 1000000u, std::min(6, mt_ndigits(whole)));
  *out++ = '.';
  float rest = w - (float)(int)w;
  for (int place = 0; place < 6; ++place) {
    rest = rest * 10.0f;
    const int digit = (int)rest;
    *out++ = (char)('0' + digit);
    rest = rest - (float)digit;
  }
  return out;
}

__device__ inline uint32_t mt_block_sum(uint32_t v, uint32_t* sh /*MT / 64*/) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();  // sh may still be read from the previous use
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t s = 0;
#pragma unroll
  for (int i = 0; i < MT / ISLE_WAVE; ++i) s += sh[i];
  return s;
}

// A tile's nbytes characters, formatted into LDS at text[shift ...) with shift = dst0 % 16, leave for out[dst0 ...): whole aligned
// 16-byte lines (uint4, consecutive lanes consecutive lines), single byte stores only for the < 16 bytes the tile shares with its
// neighbour's line at either end.  out is 16-byte aligned.  Every thread of the block calls it; it ends in a barrier, after which the
// lines may be overwritten.
__device__ inline void mt_store_tile(const uint4* lines, uint32_t shift, uint32_t nbytes, unsigned char* __restrict__ out, uint64_t dst0) {
  const char* const text = reinterpret_cast<const char*>(lines);
  __syncthreads();
  const uint32_t end = shift + nbytes;
  const uint32_t first = shift ? 1u : 0u, last = end >> 4;  // whole lines [first, last)
  uint4* const gl = reinterpret_cast<uint4*>(out + (dst0 - shift));
  for (uint32_t j = first + threadIdx.x; j < last; j += MT) gl[j] = lines[j];
  const uint32_t head_end = shift ? min(16u, end) : 0u;  // [shift, head_end): the line shared with the tile before
  const uint32_t tail = max(last << 4, head_end);        // [tail, end): the line shared with the tile after
  if (threadIdx.x < 16) {
    const uint32_t j = shift + threadIdx.x;
    if (j < head_end) out[dst0 - shift + j] = (unsigned char)text[j];
  } else if (threadIdx.x < 32) {
    const uint32_t j = tail + (threadIdx.x - 16);
    if (j < end) out[dst0 - shift + j] = (unsigned char)text[j];
  }
  __syncthreads();  // the next tile overwrites the lines
}
