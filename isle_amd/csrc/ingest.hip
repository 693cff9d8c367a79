// isle_amd/csrc/ingest.hip — tdf text -> count matrix A (CSC) in HBM.
//
//   ing_nl_count_k / ing_nl_fill_k   line starts (one '\n' scan over the text)
//   ing_parse_k / ing_pack_k         one thread per line: "<doc> <word> <count>", 1-based ids,        include/utils.h:158-228
//                                    blanks / tabs between fields, '\r' ignored; the entries packed   (DocWordEntriesReader)
//   rs_hist_k / rs_scatter_k         stable LSD radix sort of the entries by (doc, word), 8 bits      src/trainer.cpp:236-241
//                                    per pass, hand-written (wave-level multisplit)
//   ing_flag_k / ing_compact_k       drop repeated (doc, word) pairs, first in file order survives    src/trainer.cpp:243-247
//   ing_offsets_k                    column offsets, empty documents included                         src/sparseMatrix.cpp:58-87
//   feed_key_k                       binary (doc, word, count) triples in batches (isle_hip_feed_*) instead of lines
//   tdf_advance_k                    the same text in pieces cut anywhere (isle_hip_tdf_*): the same kernels over the complete lines of
//                                    [carry | piece], the entries packed behind those held; the rest becomes the next carry
//   tdf_window_k                     the windowed stream (isle_hip_tdf_begin_window): every line checked as above, then only the entries of
//                                    documents [doc_begin, doc_end) stay valid, keyed by doc - doc_begin
//   tdf_doc_count_k / tdf_plan_k     the counting stream (isle_hip_tdf_begin_counts): valid lines per document, one atomic add per run of
//                                    equal documents within a wave; then the bounds of `parts` shards balanced by lines (stage_host.h plan_bound)
//
// Deviations from the reference parser, shared with the host parser of isle_amd/host/prestage.h: trailing blanks do not
// leak into the next line (the reference keeps its was_whitespace flag across '\n'), blank lines are skipped, a bad
// character or a line with more than three fields is an error instead of a debug assert, and so are a line with fewer than three
// fields, an id outside 1..D / 1..V, a count of 0 and a count above 4294967295.  A field saturates at 2^32 while it is read (no id or
// count needs more), so no digit string, however long, wraps into range.  Of several bad lines the first in the file is reported.  The
// reference's std::sort + std::unique keeps an unspecified one of several equal (doc, word) lines; here it is the first in the file.
#include <algorithm>
#include <utility>

#include "common.h"
#include "scan.h"
#include "stage_host.h"

namespace {

constexpr int IT = 256;
constexpr int BYTES_PER_THREAD = 16;
constexpr int TILE_BYTES = IT * BYTES_PER_THREAD;  // 4096

__device__ inline int count_nl16(const unsigned char* __restrict__ text, uint64_t pos, uint64_t n) {
  int c = 0;
  if (pos + 16 <= n) {
    const uint4 v = *reinterpret_cast<const uint4*>(text + pos);  // pos is a multiple of 16; hipMalloc aligns the base
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int b = 0; b < 4; ++b) c += ((w[j] >> (8 * b)) & 0xffu) == (uint32_t)'\n';
  } else {
    for (uint64_t p = pos; p < n; ++p) c += text[p] == '\n';
  }
  return c;
}

__global__ __launch_bounds__(IT) void ing_nl_count_k(const unsigned char* __restrict__ text, uint64_t n, uint32_t* __restrict__ tile_cnt) {
  __shared__ uint32_t sh[IT];
  const uint64_t pos = (uint64_t)blockIdx.x * TILE_BYTES + (uint64_t)threadIdx.x * BYTES_PER_THREAD;
  sh[threadIdx.x] = pos < n ? (uint32_t)count_nl16(text, pos, n) : 0u;
  __syncthreads();
  for (int o = IT / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) tile_cnt[blockIdx.x] = sh[0];
}

// line_start[j + 1] = position after the j-th '\n' (line_start[0] = 0 is set by the host)
__global__ __launch_bounds__(IT) void ing_nl_fill_k(const unsigned char* __restrict__ text, uint64_t n, const int64_t* __restrict__ tile_off,
                                                     uint64_t* __restrict__ line_start) {
  __shared__ int64_t sh[isle_scan::SCAN_T];
  const uint64_t pos = (uint64_t)blockIdx.x * TILE_BYTES + (uint64_t)threadIdx.x * BYTES_PER_THREAD;
  const int mine = pos < n ? count_nl16(text, pos, n) : 0;
  int64_t tot;
  int64_t at = tile_off[blockIdx.x] + isle_scan::block_exclusive<int64_t>((int64_t)mine, sh, &tot);
  if (mine) {
    const uint64_t e = pos + 16 < n ? pos + 16 : n;
    for (uint64_t p = pos; p < e; ++p)
      if (text[p] == '\n') line_start[++at] = p + 1;
  }
}

// One line, text[s, e) without its '\n'.  -> 0 with *ok = 1 and its (key, count), 0 with *ok = 0 for a line without a digit, or the kind of
// what is wrong with it: 1 bad character, 2 too many fields, 3 fewer than three fields, 4 doc/word id 0 or out of range, 5 count 0,
// 6 count above 2^32 - 1.
__device__ inline int ing_parse_line(const unsigned char* __restrict__ text, uint64_t s, uint64_t e, uint64_t V, uint64_t D, int wbits, uint64_t* key,
                                     uint32_t* cnt, uint32_t* ok) {
  constexpr unsigned long long FIELD_MAX = 0xffffffffull;
  unsigned long long f[3] = {0, 0, 0};
  int state = 0;
  bool was_ws = false, any = false;
  int bad = 0;
  for (uint64_t p = s; p < e; ++p) {
    const unsigned char ch = text[p];
    if (ch == '\r') continue;
    if (ch == ' ' || ch == '\t') {
      was_ws = true;
      continue;
    }
    if (ch < '0' || ch > '9') {
      bad = 1;
      break;
    }
    if (was_ws && any) ++state;
    was_ws = false;
    any = true;
    if (state > 2) {
      bad = 2;
      break;
    }
    f[state] = f[state] * 10ull + (unsigned long long)(ch - '0');
    if (f[state] > FIELD_MAX) f[state] = FIELD_MAX + 1ull;  // saturated: above every id and every count, and 10 * 2^32 + 9 still fits
  }
  *ok = 0;
  if (!bad && any) {
    if (state != 2) bad = 3;
    else if (f[0] == 0 || f[1] == 0 || f[0] > D || f[1] > V) bad = 4;
    else if (f[2] == 0) bad = 5;  // a document made of zero counts would normalise to 0 / 0 (src/sparseMatrix.cpp:136-167)
    else if (f[2] > FIELD_MAX) bad = 6;
    else {
      *ok = 1;
      *key = ((f[0] - 1) << wbits) | (f[1] - 1);
      *cnt = (uint32_t)f[2];
    }
  }
  return bad;
}

// The lines of text[0, n): the nnl lines that end in '\n', line l being text[line_start[l], line_start[l + 1] - 1), and with `tail` the
// bytes behind the last '\n' as one more line.  nnl is *nnl_dev where the count is on the device only (the stream), else nnl_host.
// valid[] is written for every l < nmax, the host's bound on the lines, so that the scan behind needs no count from the device.
// *err starts as all ones and ends as the smallest (line << 3) | kind over the bad lines: the first bad line, whichever thread gets
// there first.  Lines are numbered from *line0 (the stream: from tdf_begin), from 0 where it is null.
__global__ __launch_bounds__(IT) void ing_parse_k(const unsigned char* __restrict__ text, uint64_t n, const uint64_t* __restrict__ line_start,
                                                   const int64_t* __restrict__ nnl_dev, uint64_t nnl_host, uint64_t nmax, int tail, uint64_t V, uint64_t D,
                                                   int wbits, uint64_t* __restrict__ key, uint32_t* __restrict__ cnt, uint32_t* __restrict__ valid,
                                                   unsigned long long* __restrict__ err, const unsigned long long* __restrict__ line0) {
  const uint64_t l = (uint64_t)blockIdx.x * IT + threadIdx.x;
  if (l >= nmax) return;
  const uint64_t nnl = nnl_dev ? (uint64_t)*nnl_dev : nnl_host;
  if (l >= nnl + (uint64_t)tail) {
    valid[l] = 0;
    return;
  }
  const uint64_t s = l ? line_start[l] : 0;  // (a tail alone, the stream's last line, has no line starts at all)
  const uint64_t e = l < nnl ? line_start[l + 1] - 1 : n;
  uint64_t k = 0;
  uint32_t x = 0, ok = 0;
  const int bad = ing_parse_line(text, s, e, V, D, wbits, &k, &x, &ok);
  if (ok) {
    key[l] = k;
    cnt[l] = x;
  }
  valid[l] = ok;
  if (bad) atomicMin(err, (((line0 ? *line0 : 0ull) + l) << 3) | (unsigned long long)bad);
}

// the valid ones of nlines (key, count) pairs to okey / ocnt, behind the *held entries these hold (none where it is null)
__global__ __launch_bounds__(IT) void ing_pack_k(const uint64_t* __restrict__ key, const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ valid,
                                                  const int64_t* __restrict__ at, uint64_t nlines, uint64_t* __restrict__ okey, uint32_t* __restrict__ ocnt,
                                                  const unsigned long long* __restrict__ held) {
  const uint64_t l = (uint64_t)blockIdx.x * IT + threadIdx.x;
  if (l < nlines && valid[l]) {
    const uint64_t j = (held ? (uint64_t)*held : 0ull) + (uint64_t)at[l];
    okey[j] = key[l];
    ocnt[j] = cnt[l];
  }
}

// ---------------- stable LSD radix sort, 8 bits per pass ------------------------------------------------------------
constexpr int RS_ITEMS = 8;
constexpr int RS_TILE = IT * RS_ITEMS;  // 2048 keys per workgroup
constexpr int RS_WAVES = IT / ISLE_WAVE;

__global__ __launch_bounds__(IT) void rs_hist_k(const uint64_t* __restrict__ key, uint64_t n, int shift, uint32_t nblocks, uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t base = (uint64_t)blockIdx.x * RS_TILE;
#pragma unroll
  for (int r = 0; r < RS_ITEMS; ++r) {
    const uint64_t i = base + (uint64_t)r * IT + threadIdx.x;
    if (i < n) atomicAdd(&h[(key[i] >> shift) & 255u], 1u);
  }
  __syncthreads();
  hist[(size_t)threadIdx.x * nblocks + blockIdx.x] = h[threadIdx.x];  // digit-major: one exclusive scan orders digits first
}

__global__ __launch_bounds__(IT) void rs_scatter_k(const uint64_t* __restrict__ key, const uint32_t* __restrict__ val, uint64_t n, int shift, uint32_t nblocks,
                                                    const int64_t* __restrict__ hist_off, uint64_t* __restrict__ okey, uint32_t* __restrict__ oval) {
  __shared__ int64_t base_of[256];
  __shared__ uint32_t run[256];
  __shared__ uint32_t wcnt[RS_WAVES][256];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  base_of[t] = hist_off[(size_t)t * nblocks + blockIdx.x];
  run[t] = 0;
#pragma unroll
  for (int w = 0; w < RS_WAVES; ++w) wcnt[w][t] = 0;
  __syncthreads();
  const uint64_t base = (uint64_t)blockIdx.x * RS_TILE;
  const unsigned long long lt = (1ull << lane) - 1ull;
  for (int r = 0; r < RS_ITEMS; ++r) {
    const uint64_t i = base + (uint64_t)r * IT + t;
    const bool live = i < n;
    const uint64_t k = live ? key[i] : 0ull;
    const uint32_t v = live ? val[i] : 0u;
    const uint32_t d = (uint32_t)(k >> shift) & 255u;
    // lanes of this wave holding the same digit (dead lanes form their own class)
    unsigned long long peers = __ballot(live);
    if (!live) peers = ~peers;
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const unsigned long long m = __ballot((d >> b) & 1u);
      peers &= ((d >> b) & 1u) ? m : ~m;
    }
    const uint32_t rank = (uint32_t)__popcll(peers & lt);
    if (live && rank == 0) wcnt[wv][d] = (uint32_t)__popcll(peers);
    __syncthreads();
    if (live) {
      uint32_t before = 0;
      for (int w = 0; w < wv; ++w) before += wcnt[w][d];
      const int64_t pos = base_of[d] + run[d] + before + rank;
      okey[pos] = k;
      oval[pos] = v;
    }
    __syncthreads();
    uint32_t tot = 0;
#pragma unroll
    for (int w = 0; w < RS_WAVES; ++w) {
      tot += wcnt[w][t];
      wcnt[w][t] = 0;
    }
    run[t] += tot;
    __syncthreads();
  }
}

__global__ __launch_bounds__(IT) void ing_flag_k(const uint64_t* __restrict__ key, uint64_t n, uint32_t* __restrict__ flag) {
  const uint64_t i = (uint64_t)blockIdx.x * IT + threadIdx.x;
  if (i < n) flag[i] = (i == 0 || key[i] != key[i - 1]) ? 1u : 0u;
}

__global__ __launch_bounds__(IT) void ing_compact_k(const uint64_t* __restrict__ key, const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ flag,
                                                     const int64_t* __restrict__ at, uint64_t n, int wbits, uint32_t* __restrict__ rows,
                                                     float* __restrict__ counts, uint32_t* __restrict__ docs) {
  const uint64_t i = (uint64_t)blockIdx.x * IT + threadIdx.x;
  if (i < n && flag[i]) {
    const int64_t j = at[i];
    rows[j] = (uint32_t)(key[i] & ((1ull << wbits) - 1ull));
    counts[j] = (float)cnt[i];
    docs[j] = (uint32_t)(key[i] >> wbits);
  }
}

// offs[d] = first entry of document d (entries sorted by document); offs[D] = m
__global__ __launch_bounds__(IT) void ing_offsets_k(const uint32_t* __restrict__ docs, uint64_t m, uint64_t D, int64_t* __restrict__ offs) {
  const uint64_t i = (uint64_t)blockIdx.x * IT + threadIdx.x;
  if (i > m) return;
  const uint64_t lo = (i == 0) ? 0 : (uint64_t)docs[i - 1] + 1;  // first document not yet opened
  const uint64_t hi = (i == m) ? D : (uint64_t)docs[i];         // documents lo..hi start at entry i
  for (uint64_t d = lo; d <= hi; ++d) offs[d] = (int64_t)i;
}

}  // namespace

#define LAUNCH_CHECK(c) HIPCHK(c, hipGetLastError())

// Stable LSD radix sort of n (key, payload) pairs on the low key_bits bits of the keys, ping-ponging between the caller's
// two buffer pairs; *in_a tells which pair holds the sorted sequence.  The histogram (256 counters per 2048 keys), its offsets
// and the scan's scratch are the caller's and grow as needed.
static int rs_sort_pairs(isle_ctx* c, DevBuf<uint32_t>& hist, DevBuf<int64_t>& hist_off, DevBuf<int64_t>& scratch, uint64_t* key_a, uint32_t* val_a,
                         uint64_t* key_b, uint32_t* val_b, uint64_t n, int key_bits, bool* in_a) {
  *in_a = true;
  if (n < 2) return 0;
  const uint32_t nblocks = (uint32_t)((n + RS_TILE - 1) / RS_TILE);
  HIPCHK(c, hist.reserve((size_t)256 * nblocks));
  HIPCHK(c, hist_off.reserve((size_t)256 * nblocks + 1));
  HIPCHK(c, scratch.reserve(isle_scan_scratch((uint64_t)256 * nblocks) + 8));
  uint64_t *ka = key_a, *kb = key_b;
  uint32_t *va = val_a, *vb = val_b;
  for (int shift = 0; shift < key_bits; shift += 8) {
    hipLaunchKernelGGL(rs_hist_k, dim3(nblocks), dim3(IT), 0, c->stream, ka, n, shift, nblocks, hist.p);
    LAUNCH_CHECK(c);
    HIPCHK(c, (isle_scan::exclusive_scan<uint32_t, int64_t>(c->stream, hist.p, (uint64_t)256 * nblocks, hist_off.p, scratch.p)));
    hipLaunchKernelGGL(rs_scatter_k, dim3(nblocks), dim3(IT), 0, c->stream, ka, va, n, shift, nblocks, hist_off.p, kb, vb);
    LAUNCH_CHECK(c);
    std::swap(ka, kb);
    std::swap(va, vb);
    *in_a = !*in_a;
  }
  return 0;
}

// The same with the context's scratch, which stays: also used by gram_lds.hip to order documents and words by their number of
// nonzeros, and by spmm.hip, kmeans.hip, corpus_stats.hip, edge_select.hip and doc_report.hip.
int k_sort_pairs_u64(isle_ctx* c, uint64_t* key_a, uint32_t* val_a, uint64_t* key_b, uint32_t* val_b, uint64_t n, int key_bits, bool* in_a) {
  return rs_sort_pairs(c, c->rs_hist, c->rs_hist_off, c->rs_scratch, key_a, val_a, key_b, val_b, n, key_bits, in_a);
}

// The part all front ends share: ne (key, count) pairs in offered order in (key_a, cnt_a), keys (doc << wbits) | word; (key_b, cnt_b) is
// the other half of the sort's ping-pong, ne elements each.  Stable sort by (doc, word), the first of equal pairs kept, offsets with the
// empty documents: the result becomes the context's a_cnt / a_rows / a_offs, a_V, a_D, a_nnz.  The sort's scratch is local: a histogram
// of 256 counters per 2048 entries is not to outlive the ingest.
static int ing_sort_dedup_install(isle_ctx* c, uint64_t V, uint64_t D, int wbits, int dbits, uint64_t* key_a, uint32_t* cnt_a, uint64_t* key_b,
                                  uint32_t* cnt_b, uint64_t ne) {
  DevBuf<uint32_t> flag, docs, hist;
  DevBuf<int64_t> at, hist_off, scratch;
  // ---- sort by (doc, word)
  HIPCHK(c, scratch.reserve(isle_scan_scratch(ne + 16) + 8));
  bool in_a = true;
  ISLECHK(rs_sort_pairs(c, hist, hist_off, scratch, key_a, cnt_a, key_b, cnt_b, ne, wbits + dbits, &in_a));
  const uint64_t* ka = in_a ? key_a : key_b;
  const uint32_t* va = in_a ? cnt_a : cnt_b;
  // ---- drop repeated pairs, build the CSC
  HIPCHK(c, flag.reserve(ne ? ne : 1));
  HIPCHK(c, at.reserve(ne + 1));
  if (ne) hipLaunchKernelGGL(ing_flag_k, dim3(cdiv((long)ne, IT)), dim3(IT), 0, c->stream, ka, ne, flag.p);
  LAUNCH_CHECK(c);
  HIPCHK(c, (isle_scan::exclusive_scan<uint32_t, int64_t>(c->stream, flag.p, ne, at.p, scratch.p)));
  int64_t m = 0;
  HIPCHK(c, hipMemcpyAsync(&m, at.p + ne, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, c->a_cnt.reserve(m ? m : 1));
  HIPCHK(c, c->a_rows.reserve(m ? m : 1));
  HIPCHK(c, c->a_offs.reserve(D + 1));
  HIPCHK(c, docs.reserve(m ? m : 1));
  if (ne) hipLaunchKernelGGL(ing_compact_k, dim3(cdiv((long)ne, IT)), dim3(IT), 0, c->stream, ka, va, flag.p, at.p, ne, wbits, c->a_rows.p, c->a_cnt.p, docs.p);
  LAUNCH_CHECK(c);
  hipLaunchKernelGGL(ing_offsets_k, dim3(cdiv((long)m + 1, IT)), dim3(IT), 0, c->stream, docs.p, (uint64_t)m, D, c->a_offs.p);
  LAUNCH_CHECK(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->a_V = V;
  c->a_D = D;
  c->a_nnz = (uint64_t)m;
  return 0;  // (the local buffers are released by their destructors, on the error returns too)
}

static void ing_key_bits(uint64_t V, uint64_t D, int* wbits, int* dbits) {
  *wbits = 1;
  while ((1ull << *wbits) < V) ++*wbits;
  *dbits = 1;
  while ((1ull << *dbits) < D) ++*dbits;
}

// The line starts of text[0, n): the '\n' of each 4096-byte tile counted and scanned (tile_off[ntiles] is their number, nnl, and stays on
// the device), line_start[0] = 0, line_start[j + 1] = the position behind the j-th '\n'.  With nnl_back the count and the text's last byte
// are read back behind the scan and line_start gets nnl + 2 elements; without, the caller has sized it by a bound and nothing is read back.
static int ing_line_starts(isle_ctx* c, const unsigned char* text, uint64_t n, uint32_t* tile_cnt, int64_t* tile_off, int64_t* scratch,
                           DevBuf<uint64_t>& line_start, int64_t* nnl_back, unsigned char* last_back) {
  const uint64_t ntiles = (n + TILE_BYTES - 1) / TILE_BYTES;
  if (ntiles) hipLaunchKernelGGL(ing_nl_count_k, dim3((unsigned)ntiles), dim3(IT), 0, c->stream, text, n, tile_cnt);
  LAUNCH_CHECK(c);
  HIPCHK(c, (isle_scan::exclusive_scan<uint32_t, int64_t>(c->stream, tile_cnt, ntiles, tile_off, scratch)));
  if (nnl_back) {
    HIPCHK(c, hipMemcpyAsync(nnl_back, tile_off + ntiles, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    if (n) HIPCHK(c, hipMemcpyAsync(last_back, text + n - 1, 1, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, line_start.reserve(*nnl_back + 2));
  }
  HIPCHK(c, hipMemsetAsync(line_start.p, 0, sizeof(uint64_t), c->stream));
  if (ntiles) hipLaunchKernelGGL(ing_nl_fill_k, dim3((unsigned)ntiles), dim3(IT), 0, c->stream, text, n, tile_off, line_start.p);
  LAUNCH_CHECK(c);
  return 0;
}

// text_dev: n bytes on the device.  On success the context's count matrix is set (a_cnt / a_rows / a_offs, a_nnz).  Every buffer is the
// call's own and goes at scope exit, on every return: an open feed or text stream keeps its staging.
int k_ingest_tdf(isle_ctx* c, const unsigned char* text_dev, uint64_t n, uint64_t V, uint64_t D, uint64_t* entries_read, uint64_t* err_out /*2*/) {
  TimeScope ts(c, ISLE_T_INGEST);
  err_out[0] = err_out[1] = 0;
  int wbits, dbits;
  ing_key_bits(V, D, &wbits, &dbits);
  const uint64_t ntiles = (n + TILE_BYTES - 1) / TILE_BYTES;
  DevBuf<uint32_t> tile_cnt, valid, cnt0, cnt1;
  DevBuf<int64_t> tile_off, at, scratch;
  DevBuf<uint64_t> line_start, key0, key1, errd;
  // ---- line starts
  HIPCHK(c, tile_cnt.reserve(ntiles ? ntiles : 1));
  HIPCHK(c, tile_off.reserve(ntiles + 1));
  HIPCHK(c, scratch.reserve(isle_scan_scratch(n + 16) + 8));  // every scan below is over at most n elements
  int64_t nnl = 0;
  unsigned char last = '\n';
  ISLECHK(ing_line_starts(c, text_dev, n, tile_cnt.p, tile_off.p, scratch.p, line_start, &nnl, &last));
  const int tail = (n && last != '\n') ? 1 : 0;  // the last line's end is n - 1 if the text ends in '\n', else n
  const uint64_t nlines = (uint64_t)nnl + tail;
  // ---- parse
  HIPCHK(c, key0.reserve(nlines ? nlines : 1));
  HIPCHK(c, cnt0.reserve(nlines ? nlines : 1));
  HIPCHK(c, valid.reserve(nlines ? nlines : 1));
  HIPCHK(c, at.reserve(nlines + 1));
  HIPCHK(c, errd.reserve(1));
  HIPCHK(c, hipMemsetAsync(errd.p, 0xff, sizeof(uint64_t), c->stream));
  if (nlines)
    hipLaunchKernelGGL(ing_parse_k, dim3(cdiv((long)nlines, IT)), dim3(IT), 0, c->stream, text_dev, n, line_start.p, nullptr, (uint64_t)nnl, nlines,
                       tail, V, D, wbits, key0.p, cnt0.p, valid.p, (unsigned long long*)errd.p, nullptr);
  LAUNCH_CHECK(c);
  HIPCHK(c, (isle_scan::exclusive_scan<uint32_t, int64_t>(c->stream, valid.p, nlines, at.p, scratch.p)));
  int64_t nent = 0;
  HIPCHK(c, hipMemcpyAsync(&nent, at.p + nlines, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  uint64_t first_bad = ~0ull;
  HIPCHK(c, hipMemcpyAsync(&first_bad, errd.p, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *entries_read = (uint64_t)nent;
  if (first_bad != ~0ull) {
    err_out[0] = first_bad & 7ull;  // kind
    err_out[1] = first_bad >> 3;    // 0-based line
    return 0;  // the caller formats the message
  }
  const uint64_t ne = (uint64_t)nent;
  HIPCHK(c, key1.reserve(ne ? ne : 1));
  HIPCHK(c, cnt1.reserve(ne ? ne : 1));
  if (nlines)
    hipLaunchKernelGGL(ing_pack_k, dim3(cdiv((long)nlines, IT)), dim3(IT), 0, c->stream, key0.p, cnt0.p, valid.p, at.p, nlines, key1.p, cnt1.p,
                       nullptr);
  LAUNCH_CHECK(c);
  // ---- sort by (doc, word), drop repeated pairs, build the CSC: keys in key1/cnt1, ping-pong with key0/cnt0
  return ing_sort_dedup_install(c, V, D, wbits, dbits, key1.p, cnt1.p, key0.p, cnt0.p, ne);
}

// ---------------- binary (doc, word, count) triples in batches (isle_hip_feed_*) --------------------------------------------------------
namespace {

// kinds: 1 document out of range, 2 word out of range.  *err as in ing_parse_k: the smallest (ordinal << 3) | kind, the ordinal counted
// over every entry offered since the feed was opened.  An entry with count 0 is in range or an error like any other, and is then skipped.
__global__ __launch_bounds__(IT) void feed_key_k(const uint32_t* __restrict__ docs, const uint32_t* __restrict__ words, const uint32_t* __restrict__ counts,
                                                  uint64_t n, uint64_t ordinal0, uint64_t V, uint64_t D, int wbits, uint64_t* __restrict__ key,
                                                  uint32_t* __restrict__ cnt, uint32_t* __restrict__ valid, unsigned long long* __restrict__ err) {
  const uint64_t i = (uint64_t)blockIdx.x * IT + threadIdx.x;
  if (i >= n) return;
  const uint32_t d = docs[i], w = words[i], x = counts[i];
  const int bad = d >= D ? 1 : (w >= V ? 2 : 0);
  key[i] = ((uint64_t)d << wbits) | (uint64_t)w;
  cnt[i] = x;
  valid[i] = (!bad && x != 0u) ? 1u : 0u;
  if (bad) atomicMin(err, ((unsigned long long)(ordinal0 + i) << 3) | (unsigned long long)bad);
}

// a buffer of at least `need` elements whose first `keep` elements are those it held; where it grows, to at least twice what it was
template <class T>
hipError_t grow_keeping(hipStream_t st, DevBuf<T>& b, size_t keep, size_t need) {
  if (need <= b.cap) return hipSuccess;
  const size_t want = std::max(need, 2 * b.cap);
  if (!keep) return b.reserve(want);
  T* q = nullptr;
  hipError_t e = hipMalloc((void**)&q, want * sizeof(T));
  if (e != hipSuccess) return e;
  e = hipMemcpyAsync(q, b.p, keep * sizeof(T), hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    (void)hipFree(q);
    return e;
  }
  if (b.p) (void)hipFree(b.p);
  b.p = q;
  b.cap = want;
  return hipSuccess;
}

// room for m more entries behind the `held` entries of the feed's store
hipError_t feed_room(hipStream_t st, IsleFeed& f, uint64_t held, uint64_t m) {
  const hipError_t e = grow_keeping(st, f.key, (size_t)held, (size_t)(held + m));
  return e != hipSuccess ? e : grow_keeping(st, f.cnt, (size_t)held, (size_t)(held + m));
}

// the staging of m lines or entries ahead of their compaction, with scratch for a scan over scan_n inputs
hipError_t feed_stage(IsleFeed& f, uint64_t m, uint64_t scan_n) {
  hipError_t e = f.t_key.reserve(m);
  if (e == hipSuccess) e = f.t_cnt.reserve(m);
  if (e == hipSuccess) e = f.t_valid.reserve(m);
  if (e == hipSuccess) e = f.t_at.reserve(m + 1);
  if (e == hipSuccess) e = f.t_scratch.reserve(isle_scan_scratch(scan_n) + 8);
  return e;
}

}  // namespace

void IsleFeed::release() {
  open = text = acquired = in_flight = counting = windowed = false;
  n = offered = piece = pieces = w_begin = w_end = 0;
  known = {0, 0, 0, ~0ull, 0};
  if (t_done) (void)hipEventDestroy(t_done);
  t_done = nullptr;
  t_text[0].release(); t_text[1].release(); t_state.release(); t_tile_cnt.release(); t_tile_off.release(); t_line_start.release();
  t_pin[0].release(); t_pin[1].release(); t_back.release(); t_doc_cnt.release(); t_seen.release();
  key.release(); cnt.release(); in_docs.release(); in_words.release(); in_cnt.release(); t_key.release(); t_cnt.release(); t_valid.release();
  t_at.release(); t_scratch.release(); t_err.release();
}

// n <= ISLE_FEED_CHUNK entries from host memory behind what the feed holds.  *bad: ~0, or (ordinal << 3) | kind of the first entry out of
// range, in which case nothing was appended.
int k_feed_chunk(isle_ctx* c, const uint32_t* docs, const uint32_t* words, const uint32_t* counts, uint64_t n, uint64_t* bad) {
  IsleFeed& f = c->feed;
  *bad = ~0ull;
  if (n == 0) return 0;
  int wbits, dbits;
  ing_key_bits(f.V, f.D, &wbits, &dbits);
  HIPCHK(c, f.in_docs.reserve(n));
  HIPCHK(c, f.in_words.reserve(n));
  HIPCHK(c, f.in_cnt.reserve(n));
  HIPCHK(c, feed_stage(f, n, n));
  HIPCHK(c, f.t_err.reserve(1));
  HIPCHK(c, hipMemcpyAsync(f.in_docs.p, docs, n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(f.in_words.p, words, n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(f.in_cnt.p, counts, n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  int64_t nvalid = 0;
  {
    TimeScope ts(c, ISLE_T_INGEST);
    HIPCHK(c, hipMemsetAsync(f.t_err.p, 0xff, sizeof(uint64_t), c->stream));
    hipLaunchKernelGGL(feed_key_k, dim3(cdiv((long)n, IT)), dim3(IT), 0, c->stream, f.in_docs.p, f.in_words.p, f.in_cnt.p, n, f.offered, f.V, f.D, wbits,
                       f.t_key.p, f.t_cnt.p, f.t_valid.p, (unsigned long long*)f.t_err.p);
    LAUNCH_CHECK(c);
    HIPCHK(c, (isle_scan::exclusive_scan<uint32_t, int64_t>(c->stream, f.t_valid.p, n, f.t_at.p, f.t_scratch.p)));
  }
  HIPCHK(c, hipMemcpyAsync(&nvalid, f.t_at.p + n, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(bad, f.t_err.p, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));  // (the host arrays are the caller's again from here)
  if (*bad != ~0ull) return 0;
  HIPCHK(c, feed_room(c->stream, f, f.n, (uint64_t)nvalid));
  if (nvalid) {
    TimeScope ts(c, ISLE_T_INGEST);
    hipLaunchKernelGGL(ing_pack_k, dim3(cdiv((long)n, IT)), dim3(IT), 0, c->stream, f.t_key.p, f.t_cnt.p, f.t_valid.p, f.t_at.p, n, f.key.p + f.n, f.cnt.p + f.n,
                       nullptr);
    LAUNCH_CHECK(c);
  }
  f.n += (uint64_t)nvalid;
  f.offered += n;
  return 0;
}

// the entries held -> the context's count matrix (a_cnt / a_rows / a_offs, a_V, a_D, a_nnz)
int k_feed_finalize(isle_ctx* c) {
  IsleFeed& f = c->feed;
  TimeScope ts(c, ISLE_T_INGEST);
  const uint64_t D = f.windowed ? f.w_end - f.w_begin : f.D;  // a windowed stream's keys are doc - w_begin: fewer document bits to sort
  int wbits, dbits;
  ing_key_bits(f.V, D, &wbits, &dbits);
  f.in_docs.release(); f.in_words.release(); f.in_cnt.release(); f.t_valid.release(); f.t_at.release(); f.t_scratch.release();
  HIPCHK(c, f.key.reserve(1));  // (a feed without entries: the kernels below still take pointers)
  HIPCHK(c, f.cnt.reserve(1));
  HIPCHK(c, f.t_key.reserve(f.n ? f.n : 1));
  HIPCHK(c, f.t_cnt.reserve(f.n ? f.n : 1));
  return ing_sort_dedup_install(c, f.V, D, wbits, dbits, f.key.p, f.cnt.p, f.t_key.p, f.t_cnt.p, f.n);
}

// ---------------- tdf text in pieces cut anywhere (isle_hip_tdf_*) ----------------------------------------------------------------------
// The complete lines of text[0, L) = [carry | piece] go through ing_parse_k / ing_pack_k with the stream's state: lines numbered from
// tdf_begin, entries packed behind those the store holds.  last_line: the text is the carry behind the last piece, one line without a '\n'.
namespace {

// What stands behind the last '\n' of text[0, L) goes to the front of the other text buffer, and the stream's state moves on: the last
// kernel of a piece, the only one that writes the state's counts (no other thread of it reads them).  nvalid: the entries the piece added to
// the store (null: none); nseen: its valid lines where they are not the same number (the windowed and the counting stream), else null.
__global__ __launch_bounds__(IT) void tdf_advance_k(const unsigned char* __restrict__ text, uint64_t L, const uint64_t* __restrict__ line_start,
                                                     const int64_t* __restrict__ nnl, const int64_t* __restrict__ nvalid,
                                                     const unsigned long long* __restrict__ nseen, int last_line, unsigned char* __restrict__ next,
                                                     IsleTdfState* __restrict__ st) {
  const uint64_t from = last_line ? L : line_start[*nnl];
  const uint64_t len = L - from;
  for (uint64_t i = (uint64_t)blockIdx.x * IT + threadIdx.x; i < len; i += (uint64_t)gridDim.x * IT) next[i] = text[from + i];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    st->lines += last_line ? 1ull : (unsigned long long)*nnl;
    const unsigned long long held = nvalid ? (unsigned long long)*nvalid : 0ull;  // (a counting stream holds nothing)
    st->entries += held;
    st->seen += nseen ? *nseen : held;  // an ordinary stream holds every valid line
    st->carry = len;
  }
}

// The windowed stream, between ing_parse_k and the scan: valid[l] is ok(l) on entry and ok(l) && doc in [doc_begin, doc_end) on exit, the
// key of a line that stays rebased to doc - doc_begin.  *nseen (zeroed per piece) receives the number of ok lines, one add per workgroup.
__global__ __launch_bounds__(IT) void tdf_window_k(uint64_t* __restrict__ key, uint32_t* __restrict__ valid, uint64_t nmax, int wbits, uint64_t doc_begin,
                                                    uint64_t doc_end, unsigned long long* __restrict__ nseen) {
  const uint64_t l = (uint64_t)blockIdx.x * IT + threadIdx.x;
  const bool ok = l < nmax && valid[l] != 0u;
  if (ok) {
    const uint64_t k = key[l], doc = k >> wbits;
    if (doc >= doc_begin && doc < doc_end) key[l] = ((doc - doc_begin) << wbits) | (k & ((1ull << wbits) - 1ull));
    else valid[l] = 0u;
  }
  const int n = __syncthreads_count(ok ? 1 : 0);
  if (threadIdx.x == 0 && n) atomicAdd(nseen, (unsigned long long)n);
}

// The counting stream, in place of the scan and ing_pack_k: one line per lane.  Among the valid lanes of a wave a run is a maximal sequence
// of lanes, consecutive among the valid ones, that share a document; an invalid or blank line in between belongs to no run and ends none.
// The head of a run (no valid lane before it in the wave, or another document there) adds the run's length to the document's counter: one
// 32-bit atomic per run instead of one per line on the same address (document-major text puts about a hundred lines of a document in a
// row).  The wave as the unit of aggregation is a choice no measurement stands behind.  *nseen as in tdf_window_k.
__global__ __launch_bounds__(IT) void tdf_doc_count_k(const uint64_t* __restrict__ key, const uint32_t* __restrict__ valid, uint64_t nmax, int wbits,
                                                       uint32_t* __restrict__ doc_cnt, unsigned long long* __restrict__ nseen) {
  const uint64_t l = (uint64_t)blockIdx.x * IT + threadIdx.x;
  const int lane = threadIdx.x & (ISLE_WAVE - 1);
  const bool ok = l < nmax && valid[l] != 0u;
  const uint32_t doc = ok ? (uint32_t)(key[l] >> wbits) : 0u;  // < D <= 0xfffffff0 (ing_parse_line)
  const unsigned long long vmask = __ballot(ok);
  const unsigned long long below = (1ull << lane) - 1ull;
  const unsigned long long before = vmask & below;
  const int prev = before ? 63 - __clzll((long long)before) : lane;  // the valid lane before this one
  const uint32_t prev_doc = (uint32_t)__shfl((int)doc, prev);
  const bool head = ok && (!before || prev_doc != doc);
  const unsigned long long hmask = __ballot(head);
  if (head) {
    const unsigned long long above = hmask & ~((2ull << lane) - 1ull);  // (lane 63: 2 << 63 wraps to 0, no lane is above)
    const unsigned long long upto = above ? (1ull << (__ffsll((long long)above) - 1)) - 1ull : ~0ull;  // the lanes below the next head
    atomicAdd(&doc_cnt[doc], (uint32_t)__popcll(vmask & upto & ~below));
  }
  const int n = __syncthreads_count(ok ? 1 : 0);
  if (threadIdx.x == 0 && n) atomicAdd(nseen, (unsigned long long)n);
}

// bounds[p], 0 < p < parts: one thread per inner bound (stage_host.h plan_bound on the offsets of the line counts); bounds[0] = 0,
// bounds[parts] = D.  offs[D] is the number of lines of the whole text.
__global__ __launch_bounds__(IT) void tdf_plan_k(const int64_t* __restrict__ offs, uint64_t D, int parts, unsigned long long* __restrict__ bounds) {
  const int p = (int)(blockIdx.x * IT + threadIdx.x);
  if (p > parts) return;
  if (p == 0 || p == parts) {
    bounds[p] = p ? D : 0ull;
    return;
  }
  const uint64_t before = p > 1 ? plan_bound(offs, D, p - 1, parts, 0) : 0;
  bounds[p] = plan_bound(offs, D, p, parts, before);
}

}  // namespace

int k_tdf_open(isle_ctx* c) {
  IsleFeed& f = c->feed;
  HIPCHK(c, f.t_state.reserve(1));
  HIPCHK(c, f.t_back.reserve(sizeof(IsleTdfState)));
  HIPCHK(c, f.t_seen.reserve(1));
  HIPCHK(c, hipEventCreateWithFlags(&f.t_done, hipEventDisableTiming));
  f.known = {0, 0, 0, ~0ull, 0};
  HIPCHK(c, hipMemcpyAsync(f.t_state.p, &f.known, sizeof(IsleTdfState), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

int k_tdf_wait(isle_ctx* c) {
  IsleFeed& f = c->feed;
  if (!f.in_flight) return 0;
  HIPCHK(c, hipEventSynchronize(f.t_done));
  f.known = *reinterpret_cast<const IsleTdfState*>(f.t_back.p);
  f.in_flight = false;
  return 0;
}

void k_tdf_release_text(isle_ctx* c) {
  IsleFeed& f = c->feed;
  f.t_text[0].release(); f.t_text[1].release(); f.t_tile_cnt.release(); f.t_tile_off.release(); f.t_line_start.release();
}

// Queues one piece: n bytes from page-locked memory behind the carry, the kernels over [carry | piece], the copy of the state to t_back,
// the event.  No piece is in flight (k_tdf_wait), so f.known is exact and every size below is either known or bounded by n: a piece of n
// bytes ends at most n lines (the carry holds no '\n') and holds at most n / 6 + 1 entries ("1 1 1\n", the first may begin in the carry).
int k_tdf_piece(isle_ctx* c, const char* bytes, uint64_t n, bool last_line) {
  IsleFeed& f = c->feed;
  int wbits, dbits;
  ing_key_bits(f.V, f.D, &wbits, &dbits);
  const int s = (int)(f.pieces & 1);
  const uint64_t carry = f.known.carry, L = carry + n;
  const uint64_t nmax = last_line ? 1 : n, ntiles = (L + TILE_BYTES - 1) / TILE_BYTES;
  HIPCHK(c, grow_keeping(c->stream, f.t_text[s], carry, L + 16));  // (fits unless a line outgrows its pieces)
  HIPCHK(c, grow_keeping(c->stream, f.t_text[s ^ 1], 0, L + 16));  // the next carry: at most all of this text
  if (!f.counting) HIPCHK(c, feed_room(c->stream, f, f.known.entries, n / 6 + 1));
  HIPCHK(c, f.t_tile_cnt.reserve(ntiles));
  HIPCHK(c, f.t_tile_off.reserve(ntiles + 1));
  HIPCHK(c, f.t_line_start.reserve(n + 2));
  HIPCHK(c, feed_stage(f, nmax, L + 16));
  unsigned char* text = f.t_text[s].p;
  if (n) HIPCHK(c, hipMemcpyAsync(text + carry, bytes, n, hipMemcpyHostToDevice, c->stream));
  {
    TimeScope ts(c, ISLE_T_INGEST);
    const int64_t* nnl = f.t_tile_off.p + ntiles;  // on the device only; the last line is the carry, a tail without line starts
    if (!last_line) ISLECHK(ing_line_starts(c, text, L, f.t_tile_cnt.p, f.t_tile_off.p, f.t_scratch.p, f.t_line_start, nullptr, nullptr));
    hipLaunchKernelGGL(ing_parse_k, dim3(cdiv((long)nmax, IT)), dim3(IT), 0, c->stream, text, L, f.t_line_start.p, last_line ? nullptr : nnl, (uint64_t)0, nmax,
                       (int)last_line, f.V, f.D, wbits, f.t_key.p, f.t_cnt.p, f.t_valid.p, &f.t_state.p->err, &f.t_state.p->lines);
    LAUNCH_CHECK(c);
    const bool own_seen = f.counting || f.windowed;  // the piece's valid lines are not the entries it adds to the store
    if (own_seen) HIPCHK(c, hipMemsetAsync(f.t_seen.p, 0, sizeof(unsigned long long), c->stream));
    if (f.counting) {
      hipLaunchKernelGGL(tdf_doc_count_k, dim3(cdiv((long)nmax, IT)), dim3(IT), 0, c->stream, f.t_key.p, f.t_valid.p, nmax, wbits, f.t_doc_cnt.p, f.t_seen.p);
      LAUNCH_CHECK(c);
    } else {
      if (f.windowed) {
        hipLaunchKernelGGL(tdf_window_k, dim3(cdiv((long)nmax, IT)), dim3(IT), 0, c->stream, f.t_key.p, f.t_valid.p, nmax, wbits, f.w_begin, f.w_end, f.t_seen.p);
        LAUNCH_CHECK(c);
      }
      HIPCHK(c, (isle_scan::exclusive_scan<uint32_t, int64_t>(c->stream, f.t_valid.p, nmax, f.t_at.p, f.t_scratch.p)));
      hipLaunchKernelGGL(ing_pack_k, dim3(cdiv((long)nmax, IT)), dim3(IT), 0, c->stream, f.t_key.p, f.t_cnt.p, f.t_valid.p, f.t_at.p, nmax, f.key.p, f.cnt.p,
                         &f.t_state.p->entries);
      LAUNCH_CHECK(c);
    }
    const unsigned nb = (unsigned)std::min<uint64_t>((L + IT - 1) / IT, 1024);
    hipLaunchKernelGGL(tdf_advance_k, dim3(nb), dim3(IT), 0, c->stream, text, L, f.t_line_start.p, nnl, f.counting ? nullptr : f.t_at.p + nmax,
                       own_seen ? f.t_seen.p : nullptr, (int)last_line, f.t_text[s ^ 1].p, f.t_state.p);
    LAUNCH_CHECK(c);
  }
  HIPCHK(c, hipMemcpyAsync(f.t_back.p, f.t_state.p, sizeof(IsleTdfState), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipEventRecord(f.t_done, c->stream));
  f.in_flight = true;
  ++f.pieces;
  return 0;
}

// ---------------- the counting stream's table and the plan from it ------------------------------------------------------------------------
int k_tdf_open_counts(isle_ctx* c) {
  IsleFeed& f = c->feed;
  HIPCHK(c, f.t_doc_cnt.reserve(f.D));
  HIPCHK(c, hipMemsetAsync(f.t_doc_cnt.p, 0, f.D * sizeof(uint32_t), c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

// t_doc_cnt holds the lines per document of the whole text (summed over the ranks).  Their exclusive scan and tdf_plan_k on the device;
// parts + 1 bounds travel to the host.  offs[D], the scan's total, is lines_global: the caller has checked that it fits 32 bits, so no
// counter of the table has wrapped.
int k_tdf_plan(isle_ctx* c, uint64_t lines_global, int parts, uint64_t* bounds) {
  IsleFeed& f = c->feed;
  TimeScope ts(c, ISLE_T_INGEST);
  DevBuf<int64_t> offs, scratch;
  DevBuf<unsigned long long> bd;
  HIPCHK(c, offs.reserve(f.D + 1));
  HIPCHK(c, scratch.reserve(isle_scan_scratch(f.D + 16) + 8));
  HIPCHK(c, bd.reserve((size_t)parts + 1));
  HIPCHK(c, (isle_scan::exclusive_scan<uint32_t, int64_t>(c->stream, f.t_doc_cnt.p, f.D, offs.p, scratch.p)));
  hipLaunchKernelGGL(tdf_plan_k, dim3(cdiv((long)parts + 1, IT)), dim3(IT), 0, c->stream, offs.p, f.D, parts, bd.p);
  LAUNCH_CHECK(c);
  int64_t total = 0;
  std::vector<unsigned long long> h((size_t)parts + 1);
  HIPCHK(c, hipMemcpyAsync(h.data(), bd.p, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(&total, offs.p + f.D, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if ((uint64_t)total != lines_global)
    return isle_fail(c, ISLE_E_NUMERIC, "tdf_finalize_counts: the table sums to %lld lines, the streams counted %llu", (long long)total, (unsigned long long)lines_global);
  for (int p = 0; p <= parts; ++p) bounds[p] = (uint64_t)h[p];
  return 0;
}
