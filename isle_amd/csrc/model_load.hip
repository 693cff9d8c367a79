// isle_amd/csrc/model_load.hip — the reference's model files read on the device: the inverse of model_text.hip.  read_sparse_model
// (src/infer.cpp:125-208) and read_model (:8-76) as isle_amd/host/model_read.h restates them; the floats are theirs, bit for bit.
// The text is on the device in one piece; the result is a vocab x ncols column-major model.
//
// The weight rule (ml_push / ml_finish, the library's one copy, exported as isle_hip_parse_weight): <digits>[.<digits>], the digits
// before and after the point accumulated in fp32 as v = v * 10; v = v + d, each operation rounded on its own, the value
// (float)((double)vb + (double)va * P[pos]) with P[n] = the host's std::pow(0.1, n), uploaded as a table (the device calls no pow).
// Contraction is switched off for this whole file, host and device, by the "#pragma clang fp contract(off)" below the includes, as in
// model_text.hip: this toolchain's __fmul_rn / __fadd_rn are plain operators that contract all the same.
//
// No walk is unbounded: a sparse line of more than 4096 bytes and, in the dense form, a run of more than 64 consecutive '\r' are refused
// (as bad characters), so one lane never walks a hostile gigabyte and no thread looks back further than that.
//
// Every byte position is a key: an error is (position << 3) | kind and the smallest key wins (atomicMin), so the first offending line
// of the file is reported whatever the launch order; errors of a whole line (field count, ids, token count) sit at the line's end, where
// the serial host parser meets them.
//
//   ISLE_TEXT_SPARSE  ml_sparse_k: a thread owns the lines that START in its 16 bytes (one uint4 load finds them) and walks each to its
//                     '\n'.  A parsed line leaves (ordinal << 32) | float bits in its cell by a 64-bit atomicMax, ordinal =
//                     (line start >> 2) + 1: a line with three fields is at least 6 bytes long, so the ordinal grows strictly with the
//                     line number and the last line naming a cell wins, deterministically.  ml_resolve_k keeps the low words; a cell
//                     nobody named is +0.  The ordinal's 32 bits bound the text at 2^34 bytes.
//   ISLE_TEXT_DENSE   a line is a column (about 1 MB at 100 k words), so the unit is the token: ml_dense_count_k counts token starts
//                     and '\n' per 4096-byte tile, two 64-bit exclusive scans (scan.h) number them, ml_dense_lines_k notes for every
//                     physical line the tokens before it and where it ends, ml_dense_check_k holds every non-blank line to vocab
//                     tokens and flags it, a third scan numbers the non-blank lines, and ml_dense_parse_k gives every token start a
//                     thread: its line from the '\n' scan, its place in the line from the token scan, its value into model[place, line].
#include <algorithm>
#include <cmath>
#include <cstring>

#include "common.h"
#include "scan.h"

#pragma clang fp contract(off)

namespace {

constexpr int ML = isle_scan::SCAN_T;  // 256: block_exclusive's width
constexpr int ML_CHUNK = 16;           // bytes per thread: one uint4
constexpr int ML_TILE = ML * ML_CHUNK;
constexpr int ML_MAX_TOKEN = 64;       // P holds 0 .. 64
constexpr int ML_MAX_ID_DIGITS = 18;
constexpr int ML_MAX_CR_RUN = 64;        // DENSE: more consecutive '\r' than this are refused, so no walk over them is longer
constexpr int ML_MAX_LINE = 4096;        // SPARSE: bytes of a line, its '\n' excluded, so no lane walks further
constexpr uint32_t ML_NAN_HEAD = (uint32_t)'n' | ((uint32_t)'a' << 8) | ((uint32_t)'n' << 16);
enum { ML_E_CHAR = 1, ML_E_MANY = 2, ML_E_FEW = 3, ML_E_ID = 4, ML_E_LONG = 5, ML_E_TOKENS = 6, ML_E_LINES = 7 };

// a weight token, byte by byte ('\r' never reaches it)
struct MlWeight {
  float vb = 0.f, va = 0.f;
  int pos = 0, nd = 0, len = 0, err = 0;  // fraction digits, digits, bytes, the first error met
  bool dot = false;
  uint32_t head = 0;  // the first three bytes
};
__host__ __device__ inline void ml_push(MlWeight& w, unsigned char ch) {
  if (++w.len > ML_MAX_TOKEN) {
    if (!w.err) w.err = ML_E_LONG;
    return;
  }
  if (w.len <= 3) w.head |= (uint32_t)ch << (8 * (w.len - 1));
  if (ch >= '0' && ch <= '9') {
    const float d = (float)(ch - '0');
    if (!w.dot) {
      w.vb = w.vb * 10.0f;
      w.vb = w.vb + d;
    } else {
      w.va = w.va * 10.0f;
      w.va = w.va + d;
      ++w.pos;
    }
    ++w.nd;
  } else if (ch == '.' && !w.dot) {
    w.dot = true;
  } else if (!w.err) {
    w.err = ML_E_CHAR;
  }
}
// 0 and the value, or the kind of error
__host__ __device__ inline int ml_finish(const MlWeight& w, int format, const double* __restrict__ P, float* out) {
  if (format == ISLE_TEXT_DENSE && w.len == 3 && w.head == ML_NAN_HEAD) {  // what the dense writer prints for NaN
    const uint32_t bits = 0x7fc00000u;
    __builtin_memcpy(out, &bits, sizeof(float));
    return 0;
  }
  if (w.err) return w.err;
  if (w.nd == 0) return ML_E_CHAR;  // "" or "."
  const double after = (double)w.va * P[w.pos];
  *out = (float)((double)w.vb + after);
  return 0;
}

__device__ inline bool ml_blank(unsigned char ch) { return ch == ' ' || ch == '\t'; }

// the thread's 16 bytes at pos (a multiple of 16; hipMalloc aligns the base), zero beyond n
__device__ inline void ml_load16(const unsigned char* __restrict__ text, uint64_t pos, uint64_t n, unsigned char b[ML_CHUNK]) {
  if (pos + ML_CHUNK <= n) {
    const uint4 v = *reinterpret_cast<const uint4*>(text + pos);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < ML_CHUNK; ++i) b[i] = (unsigned char)(w[i >> 2] >> (8 * (i & 3)));
  } else {
#pragma unroll
    for (int i = 0; i < ML_CHUNK; ++i) b[i] = pos + i < n ? text[pos + i] : (unsigned char)0;
  }
}

// ---------------- ISLE_TEXT_SPARSE ----------------------------------------------------------------------------------------------
// the line that starts at s: "<topic> <word> <weight>".  true: a line was parsed (*cell, *val); false: blank, or an error left in *key
__device__ inline bool ml_sparse_line(const unsigned char* __restrict__ text, uint64_t s, uint64_t n, uint64_t V, uint32_t ncols, uint32_t base,
                                      const double* __restrict__ P, uint64_t* cell, float* val, unsigned long long* key) {
  unsigned long long id[2] = {0, 0};
  int digits[2] = {0, 0}, field = 0;
  bool was_ws = false, any = false;
  MlWeight w;
  uint64_t q = s;
  for (; q < n; ++q) {
    const unsigned char ch = text[q];
    if (ch == '\n') break;
    if (q - s >= (uint64_t)ML_MAX_LINE) {
      *key = (q << 3) | ML_E_CHAR;
      return false;
    }
    if (ch == '\r') continue;
    if (ml_blank(ch)) {
      was_ws = true;
      continue;
    }
    if (was_ws && any && ++field > 2) {
      *key = (q << 3) | ML_E_MANY;
      return false;
    }
    was_ws = false;
    any = true;
    if (field < 2) {
      if (ch < '0' || ch > '9') {
        *key = (q << 3) | ML_E_CHAR;
        return false;
      }
      if (++digits[field] > ML_MAX_ID_DIGITS) {
        *key = (q << 3) | ML_E_ID;
        return false;
      }
      id[field] = id[field] * 10ull + (unsigned long long)(ch - '0');
    } else {
      ml_push(w, ch);
      if (w.err) {  // (the sparse form has no "nan": the first error stands)
        *key = (q << 3) | (unsigned)w.err;
        return false;
      }
    }
  }
  if (!any) return false;
  int bad = field != 2 ? ML_E_FEW : ml_finish(w, ISLE_TEXT_SPARSE, P, val);
  if (!bad && (id[0] < base || id[1] < base || id[0] - base >= ncols || id[1] - base >= V)) bad = ML_E_ID;
  if (bad) {
    *key = (q << 3) | (unsigned)bad;  // q: the line's '\n', or n
    return false;
  }
  *cell = (id[0] - base) * V + (id[1] - base);
  return true;
}

// stat[0] = min over the errors of (position << 3) | kind; stat[1] += lines parsed
__global__ __launch_bounds__(ML) void ml_sparse_k(const unsigned char* __restrict__ text, uint64_t n, uint64_t ntiles, uint64_t V, uint32_t ncols, uint32_t base,
                                                   const double* __restrict__ P, unsigned long long* __restrict__ owner,
                                                   unsigned long long* __restrict__ stat) {
  uint32_t parsed = 0;
  for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint64_t pos = tile * ML_TILE + (uint64_t)threadIdx.x * ML_CHUNK;
    if (pos >= n) continue;
    unsigned char b[ML_CHUNK];
    ml_load16(text, pos, n, b);
    uint32_t starts = (pos == 0 || text[pos - 1] == '\n') ? 1u : 0u;  // bit i: a line starts at pos + i
#pragma unroll
    for (int i = 1; i < ML_CHUNK; ++i) starts |= (b[i - 1] == '\n' ? 1u : 0u) << i;
    while (starts) {
      const int i = __ffs((int)starts) - 1;
      starts &= starts - 1;
      const uint64_t s = pos + (uint64_t)i;
      if (s >= n) break;
      uint64_t cell = 0;
      float val = 0.f;
      unsigned long long key = ~0ull;
      if (ml_sparse_line(text, s, n, V, ncols, base, P, &cell, &val, &key)) {
        atomicMax(&owner[cell], (((unsigned long long)(s >> 2) + 1ull) << 32) | (unsigned long long)__float_as_uint(val));
        ++parsed;
      } else if (key != ~0ull) {
        atomicMin(&stat[0], key);
      }
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) parsed += __shfl_xor(parsed, o);
  if ((threadIdx.x & 63) == 0 && parsed) atomicAdd(&stat[1], (unsigned long long)parsed);
}

__global__ __launch_bounds__(ML) void ml_resolve_k(const unsigned long long* __restrict__ owner, uint64_t cells, float* __restrict__ model) {
  for (uint64_t i = (uint64_t)blockIdx.x * ML + threadIdx.x; i < cells; i += (uint64_t)gridDim.x * ML) model[i] = __uint_as_float((uint32_t)owner[i]);
}

// ---------------- ISLE_TEXT_DENSE -----------------------------------------------------------------------------------------------
// Of the thread's 16 bytes: bit i of *starts = a token starts at pos + i (a byte that is no blank, '\n' or '\r', the byte before it,
// '\r' skipped, a blank or '\n' or the start of the text); bit i of *nls = '\n' at pos + i.
__device__ inline void ml_dense_chunk(const unsigned char* __restrict__ text, uint64_t pos, uint64_t n, uint32_t* starts, uint32_t* nls) {
  unsigned char b[ML_CHUNK];
  ml_load16(text, pos, n, b);
  uint64_t q = pos;
  while (q > 0 && pos - q <= (uint64_t)ML_MAX_CR_RUN && text[q - 1] == '\r') --q;  // (a longer run is an error of its own: ml_cr_run)
  bool open = q == 0 || ml_blank(text[q - 1]) || text[q - 1] == '\n';  // the next token byte starts a token
  uint32_t st = 0, nl = 0;
#pragma unroll
  for (int i = 0; i < ML_CHUNK; ++i) {
    if (pos + i >= n) break;
    const unsigned char ch = b[i];
    if (ch == '\r') continue;
    if (ch == '\n') nl |= 1u << i;
    if (ml_blank(ch) || ch == '\n') {
      open = true;
    } else {
      st |= (open ? 1u : 0u) << i;
      open = false;
    }
  }
  *starts = st;
  *nls = nl;
}

// the '\r' at e ends a run ('\r' is not the next byte): true when the run is longer than ML_MAX_CR_RUN.  At most that many steps.
__device__ inline bool ml_cr_run(const unsigned char* __restrict__ text, uint64_t e) {
  int len = 1;
  while (len <= ML_MAX_CR_RUN && e >= (uint64_t)len && text[e - len] == '\r') ++len;
  return len > ML_MAX_CR_RUN;
}

// per thread (newlines << 16) | token starts: a tile holds at most 4096 of either
__device__ inline uint32_t ml_dense_counts(const unsigned char* __restrict__ text, uint64_t pos, uint64_t n, uint32_t* starts, uint32_t* nls) {
  *starts = *nls = 0;
  if (pos < n) ml_dense_chunk(text, pos, n, starts, nls);
  return ((uint32_t)__popc(*nls) << 16) | (uint32_t)__popc(*starts);
}

__global__ __launch_bounds__(ML) void ml_dense_count_k(const unsigned char* __restrict__ text, uint64_t n, uint32_t* __restrict__ tile_tok,
                                                        uint32_t* __restrict__ tile_nl) {
  __shared__ uint32_t sh[ML];
  const uint64_t pos = (uint64_t)blockIdx.x * ML_TILE + (uint64_t)threadIdx.x * ML_CHUNK;
  uint32_t starts, nls, total;
  const uint32_t mine = ml_dense_counts(text, pos, n, &starts, &nls);
  (void)isle_scan::block_exclusive<uint32_t>(mine, sh, &total);
  if (threadIdx.x == 0) {
    tile_tok[blockIdx.x] = total & 0xffffu;
    tile_nl[blockIdx.x] = total >> 16;
  }
}

// physical line L (0-based, ended by the L-th '\n' or by the end of the text) holds the tokens [line_tok[L], line_tok[L + 1]) and ends
// at line_end[L]; line_tok[0] and the last line's entries are the host's
__global__ __launch_bounds__(ML) void ml_dense_lines_k(const unsigned char* __restrict__ text, uint64_t n, const uint64_t* __restrict__ tok_off,
                                                        const uint64_t* __restrict__ nl_off, uint64_t* __restrict__ line_tok,
                                                        uint64_t* __restrict__ line_end) {
  __shared__ uint32_t sh[ML];
  const uint64_t pos = (uint64_t)blockIdx.x * ML_TILE + (uint64_t)threadIdx.x * ML_CHUNK;
  uint32_t starts, nls, total;
  const uint32_t before = isle_scan::block_exclusive<uint32_t>(ml_dense_counts(text, pos, n, &starts, &nls), sh, &total);
  uint64_t L = nl_off[blockIdx.x] + (before >> 16);
  const uint64_t tok = tok_off[blockIdx.x] + (before & 0xffffu);
  while (nls) {
    const int i = __ffs((int)nls) - 1;
    nls &= nls - 1;
    line_tok[L + 1] = tok + (uint64_t)__popc(starts & ((1u << i) - 1u));
    line_end[L] = pos + (uint64_t)i;
    ++L;
  }
}

// flag[L] = line L is not blank; a non-blank line holds exactly V tokens
__global__ __launch_bounds__(ML) void ml_dense_check_k(const uint64_t* __restrict__ line_tok, const uint64_t* __restrict__ line_end, uint64_t nlines, uint64_t V,
                                                        uint32_t* __restrict__ flag, unsigned long long* __restrict__ stat) {
  const uint64_t L = (uint64_t)blockIdx.x * ML + threadIdx.x;
  if (L >= nlines) return;
  const uint64_t cnt = line_tok[L + 1] - line_tok[L];
  flag[L] = cnt ? 1u : 0u;
  if (cnt && cnt != V) atomicMin(&stat[0], (unsigned long long)((line_end[L] << 3) | ML_E_TOKENS));
}

// token j of non-blank line t -> model[j + t * V]
__global__ __launch_bounds__(ML) void ml_dense_parse_k(const unsigned char* __restrict__ text, uint64_t n, const uint64_t* __restrict__ tok_off,
                                                        const uint64_t* __restrict__ nl_off, const uint64_t* __restrict__ line_tok,
                                                        const uint64_t* __restrict__ line_t, uint64_t V, uint32_t ncols, const double* __restrict__ P,
                                                        float* __restrict__ model, unsigned long long* __restrict__ stat) {
  __shared__ uint32_t sh[ML];
  const uint64_t pos = (uint64_t)blockIdx.x * ML_TILE + (uint64_t)threadIdx.x * ML_CHUNK;
  uint32_t starts, nls, total;
  const uint32_t before = isle_scan::block_exclusive<uint32_t>(ml_dense_counts(text, pos, n, &starts, &nls), sh, &total);
  const uint64_t L0 = nl_off[blockIdx.x] + (before >> 16);
  uint64_t g = tok_off[blockIdx.x] + (before & 0xffffu);
  for (int i = 0; i < ML_CHUNK && pos + i < n; ++i) {  // the ends of the '\r' runs in this chunk
    const uint64_t e = pos + (uint64_t)i;
    if (text[e] == '\r' && (e + 1 == n || text[e + 1] != '\r') && ml_cr_run(text, e)) atomicMin(&stat[0], (unsigned long long)((e << 3) | ML_E_CHAR));
  }
  for (; starts; ++g) {
    const int i = __ffs((int)starts) - 1;
    starts &= starts - 1;
    const uint64_t L = L0 + (uint64_t)__popc(nls & ((1u << i) - 1u));
    MlWeight w;
    uint64_t q = pos + (uint64_t)i, epos = 0;
    int cr = 0;
    for (; q < n; ++q) {
      const unsigned char ch = text[q];
      if (ch == '\r') {
        if (++cr > ML_MAX_CR_RUN) break;  // (reported by the thread at the run's end)
        continue;
      }
      cr = 0;
      if (ml_blank(ch) || ch == '\n') break;
      const int had = w.err;
      ml_push(w, ch);
      if (!had && w.err) epos = q;
      if (w.len > ML_MAX_TOKEN) break;
    }
    if (!w.err) epos = q;  // "." is found wanting at its end
    float val = 0.f;
    const int bad = ml_finish(w, ISLE_TEXT_DENSE, P, &val);
    if (bad) {
      atomicMin(&stat[0], (unsigned long long)((epos << 3) | (unsigned)bad));
      continue;
    }
    const uint64_t j = g - line_tok[L], t = line_t[L];
    if (j < V && t < ncols) model[t * V + j] = val;  // (a line or a text of another size is an error of the checks; nothing of it is stored)
  }
}

const double* ml_pow_table() {  // P[n] = std::pow(0.1, n), n = 0 .. 64
  static double P[ML_MAX_TOKEN + 1];
  static const bool made = [] {
    for (int i = 0; i <= ML_MAX_TOKEN; ++i) P[i] = std::pow(0.1, i);
    return true;
  }();
  (void)made;
  return P;
}

}  // namespace

#define LAUNCH_CHECK(c) HIPCHK(c, hipGetLastError())

int k_load_model_text(isle_ctx* c, const unsigned char* text_dev, uint64_t n, uint64_t V, uint32_t ncols, int format, unsigned base, float* model_dev,
                      uint64_t* nentries, uint64_t* err_key) {
  TimeScope ts(c, ISLE_T_INGEST);
  *nentries = 0;
  *err_key = ~0ull;
  const uint64_t cells = V * (uint64_t)ncols, ntiles = (n + ML_TILE - 1) / ML_TILE;
  const unsigned cap = (unsigned)c->num_cus * 16u;
  DevBuf<double> P;
  DevBuf<unsigned long long> stat;
  HIPCHK(c, P.reserve(ML_MAX_TOKEN + 1));
  HIPCHK(c, stat.reserve(2));
  const unsigned long long init[2] = {~0ull, 0ull};
  unsigned long long h[2] = {~0ull, 0ull};
  HIPCHK(c, hipMemcpyAsync(P.p, ml_pow_table(), (ML_MAX_TOKEN + 1) * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(stat.p, init, sizeof(init), hipMemcpyHostToDevice, c->stream));

  if (format == ISLE_TEXT_SPARSE) {
    DevBuf<unsigned long long> owner;
    HIPCHK(c, owner.reserve(cells));
    HIPCHK(c, hipMemsetAsync(owner.p, 0, cells * sizeof(unsigned long long), c->stream));
    if (ntiles) {
      hipLaunchKernelGGL(ml_sparse_k, dim3((unsigned)std::min<uint64_t>(ntiles, cap)), dim3(ML), 0, c->stream, text_dev, n, ntiles, V, ncols, (uint32_t)base,
                         P.p, owner.p, stat.p);
      LAUNCH_CHECK(c);
    }
    hipLaunchKernelGGL(ml_resolve_k, dim3((unsigned)std::min<uint64_t>((cells + ML - 1) / ML, cap)), dim3(ML), 0, c->stream, owner.p, cells, model_dev);
    LAUNCH_CHECK(c);
    HIPCHK(c, hipMemcpyAsync(h, stat.p, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *err_key = h[0];
    *nentries = h[1];
    return 0;
  }

  // ISLE_TEXT_DENSE
  if (ntiles == 0) {
    *err_key = ML_E_LINES;  // position 0
    return 0;
  }
  DevBuf<uint32_t> tile_tok, tile_nl, flag;
  DevBuf<uint64_t> tok_off, nl_off, blk, line_tok, line_end, line_t;
  HIPCHK(c, tile_tok.reserve(ntiles));
  HIPCHK(c, tile_nl.reserve(ntiles));
  HIPCHK(c, tok_off.reserve(ntiles + 1));
  HIPCHK(c, nl_off.reserve(ntiles + 1));
  HIPCHK(c, blk.reserve(isle_scan::scan_scratch_elems(ntiles)));
  hipLaunchKernelGGL(ml_dense_count_k, dim3((unsigned)ntiles), dim3(ML), 0, c->stream, text_dev, n, tile_tok.p, tile_nl.p);
  LAUNCH_CHECK(c);
  HIPCHK(c, (isle_scan::exclusive_scan<uint32_t, uint64_t>(c->stream, tile_tok.p, ntiles, tok_off.p, blk.p)));
  HIPCHK(c, (isle_scan::exclusive_scan<uint32_t, uint64_t>(c->stream, tile_nl.p, ntiles, nl_off.p, blk.p)));
  uint64_t ntok = 0, nnl = 0;
  HIPCHK(c, hipMemcpyAsync(&ntok, tok_off.p + ntiles, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(&nnl, nl_off.p + ntiles, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const uint64_t nlines = nnl + 1;  // the last one may be empty
  HIPCHK(c, line_tok.reserve(nlines + 1));
  HIPCHK(c, line_end.reserve(nlines));
  HIPCHK(c, flag.reserve(nlines));
  HIPCHK(c, line_t.reserve(nlines + 1));
  HIPCHK(c, blk.reserve(isle_scan::scan_scratch_elems(nlines)));
  HIPCHK(c, hipMemsetAsync(line_tok.p, 0, sizeof(uint64_t), c->stream));
  HIPCHK(c, hipMemcpyAsync(line_tok.p + nlines, &ntok, sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(line_end.p + nnl, &n, sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(ml_dense_lines_k, dim3((unsigned)ntiles), dim3(ML), 0, c->stream, text_dev, n, tok_off.p, nl_off.p, line_tok.p, line_end.p);
  LAUNCH_CHECK(c);
  hipLaunchKernelGGL(ml_dense_check_k, dim3((unsigned)((nlines + ML - 1) / ML)), dim3(ML), 0, c->stream, line_tok.p, line_end.p, nlines, V, flag.p, stat.p);
  LAUNCH_CHECK(c);
  HIPCHK(c, (isle_scan::exclusive_scan<uint32_t, uint64_t>(c->stream, flag.p, nlines, line_t.p, blk.p)));
  hipLaunchKernelGGL(ml_dense_parse_k, dim3((unsigned)ntiles), dim3(ML), 0, c->stream, text_dev, n, tok_off.p, nl_off.p, line_tok.p, line_t.p, V, ncols, P.p,
                     model_dev, stat.p);
  LAUNCH_CHECK(c);
  uint64_t filled = 0;
  HIPCHK(c, hipMemcpyAsync(h, stat.p, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(&filled, line_t.p + nlines, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *err_key = h[0];
  if (filled != ncols) *err_key = std::min<uint64_t>(*err_key, (n << 3) | ML_E_LINES);  // met at the end of the text
  *nentries = ntok;
  return 0;
}

extern "C" int isle_hip_parse_weight(const char* token, uint64_t n, int format, float* out) {
  if ((n && !token) || !out || (format != ISLE_TEXT_SPARSE && format != ISLE_TEXT_DENSE)) return -1;
  MlWeight w;
  for (uint64_t i = 0; i < n && w.len <= ML_MAX_TOKEN; ++i) ml_push(w, (unsigned char)token[i]);
  return ml_finish(w, format, ml_pow_table(), out) ? -1 : 0;
}
