// isle_amd/csrc/model_text.hip — the reference's text form of a topic or edge model, formatted on the device: MMappedOutput
// (include/utils.h:383-478) under DenseMatrix::write_to_file_as_sparse / write_to_file (src/denseMatrix.cpp:124-186), as
// trainer_detail::weight_text / dense_entry_text / write_dense_as_sparse / write_dense (isle_amd/host/trainer_hip.h) restate them.
// The bytes are theirs, one for one.
//
// The V x ncols column-major model is cut into tiles of MT_TILE consecutive rows of one column (a column's last tile is short).
//   mt_count_k   one read of the model: bytes per tile, entries emitted (64-bit), and the column-major first entry that would be
//                printed but lies outside the host writer's domain (negative, infinite, >= 2^31: its (int)w / (unsigned)w are undefined)
//   exclusive scan of the tile sizes into 64-bit offsets (scan.h); offs[ntiles] is the size of the file
//   mt_write_k   per tile: entry lengths again, a block scan, every entry's characters into LDS at the tile's own alignment modulo 16,
//                then the tile leaves as whole aligned 16-byte lines (uint4, consecutive lanes consecutive lines); only the < 16 bytes
//                a tile shares with its neighbour's line at either end are single byte stores
// The text leaves in chunks of at most ISLE_TEXT_CHUNK_BYTES = 16 MiB: whole columns, a column longer than that split between tiles.
// Two device buffers and two pinned host buffers of that size (kept in the context, sized to the text when it is smaller): chunk i + 1
// is formatted on the context's stream while chunk i is copied on the copy stream and consumed by the sink on the calling thread.
// 16 MiB keeps a copy (about 0.3 ms) far above the launch and synchronisation cost of a chunk and the four buffers at 64 MiB.
//
// Edge models (construct_edge_topics_v2's FPaxpy pair, src/trainer.cpp:1152-1159) are never stored: both kernels form an entry as
// post_edge_k (post.hip) does, y = a * m_p rounded, then fmaf(b, m_q, y), while they read the two topic columns, so a V x n edge
// model costs two reads of two columns per pass and no scratch.
//
// Floating-point contraction is switched off for this whole file, host and device (text_format.h gives the reason); mt_weight there is
// the one copy of the digit rule for both sides.  The only fused operation left is the explicit fmaf of the edge entries.
//
// mt_count_k / mt_write_k and the driver below are this file's own copy of the count / scan / write scheme that text_tiles.h holds for
// the per-document formatters: on that skeleton the sparse file-sink case measured above the largest repetition of these kernels
// (profiles/model_text_c2_*.jsonl), so this formatter keeps them.  k_text_pump below is the delivery every text formatter shares.
#include <algorithm>
#include <cstring>
#include <functional>

#include "common.h"
#include "scan.h"
#include "text_format.h"

#pragma clang fp contract(off)

namespace {

// what the writer does with an entry: 0 skipped (SPARSE), 1 "0.0", 2 "nan", 3 <weight>, -1 printed but outside the writer's domain
__host__ __device__ inline int mt_class(float w, int format) {
  if (format == ISLE_TEXT_SPARSE) {
    if (!(w > 0.00000001f)) return 0;
  } else {
    if (w != w) return 2;
    if (w == 0.0f) return 1;
  }
  if (!mt_weight_in_domain(w)) return -1;
  return 3;
}
__host__ __device__ inline int mt_entry_len(int cls, float w) { return cls == 3 ? mt_whole_digits(w) + 7 : cls ? 3 : 0; }

__host__ __device__ inline char* mt_entry(int cls, float w, char* out) {
  if (cls == 3) return mt_weight(w, out);
  out[0] = cls == 1 ? '0' : 'n';
  out[1] = cls == 1 ? '.' : 'a';
  out[2] = cls == 1 ? '0' : 'n';
  return out + 3;
}

struct MtSrc {
  const float* model;
  uint64_t V;
  const int64_t* pairs;  // null: the model's own columns
  float a, b;
};
struct MtCol {
  const float* p;
  const float* q;
};
__device__ inline MtCol mt_column(const MtSrc& s, uint64_t col) {
  if (!s.pairs) return MtCol{s.model + col * s.V, nullptr};
  return MtCol{s.model + (uint64_t)s.pairs[2 * col] * s.V, s.model + (uint64_t)s.pairs[2 * col + 1] * s.V};
}
__device__ inline float mt_load(const MtSrc& s, const MtCol& c, uint64_t row) {
  if (!c.q) return c.p[row];
  const float y = s.a * c.p[row];
  return fmaf(s.b, c.q[row], y);  // post_edge_k's two FPaxpy steps
}

// stat[0] += entries emitted; stat[1] = min over offending entries of col * V + row
__global__ __launch_bounds__(MT) void mt_count_k(MtSrc src, int format, uint64_t tpc, uint64_t ntiles, uint32_t* __restrict__ sizes,
                                                  unsigned long long* __restrict__ stat) {
  __shared__ uint32_t shb[MT / ISLE_WAVE], shc[MT / ISLE_WAVE];
  for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint64_t col = tile / tpc, r0 = (tile % tpc) * MT_TILE + (uint64_t)threadIdx.x * MT_ITEMS;
    const MtCol cp = mt_column(src, col);
    const int fixed = format == ISLE_TEXT_SPARSE ? mt_ndigits((uint32_t)(col + 1)) + 3 : 1;  // col, two tabs, '\n' | the tab
    uint32_t bytes = 0, cnt = 0;
    unsigned long long bad = ~0ull;
#pragma unroll
    for (int i = 0; i < MT_ITEMS; ++i) {
      const uint64_t row = r0 + i;
      if (row >= src.V) break;
      const float w = mt_load(src, cp, row);
      const int cls = mt_class(w, format);
      if (cls < 0) {
        bad = min(bad, (unsigned long long)(col * src.V + row));
      } else if (cls) {
        ++cnt;
        bytes += (uint32_t)(mt_entry_len(cls, w) + fixed + (format == ISLE_TEXT_SPARSE ? mt_ndigits((uint32_t)(row + 1)) : 0));
      }
    }
    if (bad != ~0ull) atomicMin(&stat[1], bad);
    const uint32_t tb = mt_block_sum(bytes, shb), tc = mt_block_sum(cnt, shc);
    if (threadIdx.x == 0) {
      const bool line_end = format == ISLE_TEXT_DENSE && tile % tpc == tpc - 1;  // the column's '\n'
      sizes[tile] = tb + (line_end ? 1u : 0u);
      if (tc) atomicAdd(&stat[0], (unsigned long long)tc);
    }
  }
}

// tiles [tile0, tile0 + n) -> out[offs[tile] - offs[tile0] ...); out is 16-byte aligned
__global__ __launch_bounds__(MT) void mt_write_k(MtSrc src, int format, uint64_t tpc, uint64_t tile0, uint64_t n, const uint64_t* __restrict__ offs,
                                                  unsigned char* __restrict__ out) {
  __shared__ uint4 lines[MT_LDS_LINES];
  __shared__ uint32_t sh[MT];
  char* const text = reinterpret_cast<char*>(lines);
  const uint64_t base = offs[tile0];
  for (uint64_t tile = tile0 + blockIdx.x; tile < tile0 + n; tile += gridDim.x) {
    const uint64_t dst0 = offs[tile] - base;
    const uint32_t nbytes = (uint32_t)(offs[tile + 1] - offs[tile]);
    if (nbytes == 0) continue;  // the same for every thread of the block
    const uint32_t shift = (uint32_t)(dst0 & 15u);  // LDS position == position in out, modulo 16
    const uint64_t col = tile / tpc, r0 = (tile % tpc) * MT_TILE + (uint64_t)threadIdx.x * MT_ITEMS;
    const MtCol cp = mt_column(src, col);
    const int cd = mt_ndigits((uint32_t)(col + 1));
    const int fixed = format == ISLE_TEXT_SPARSE ? cd + 3 : 1;
    float w[MT_ITEMS];
    int cls[MT_ITEMS];
    uint32_t mine = 0;
#pragma unroll
    for (int i = 0; i < MT_ITEMS; ++i) {
      const uint64_t row = r0 + i;
      cls[i] = 0;
      w[i] = 0.f;
      if (row < src.V) {
        w[i] = mt_load(src, cp, row);
        cls[i] = mt_class(w[i], format);
        if (cls[i] < 0) cls[i] = 0;  // (the counting pass has refused such a model)
      }
      if (cls[i]) mine += (uint32_t)(mt_entry_len(cls[i], w[i]) + fixed + (format == ISLE_TEXT_SPARSE ? mt_ndigits((uint32_t)(r0 + i + 1)) : 0));
    }
    uint32_t total;
    const uint32_t at = isle_scan::block_exclusive<uint32_t>(mine, sh, &total);
    char* p = text + shift + at;
#pragma unroll
    for (int i = 0; i < MT_ITEMS; ++i) {
      if (!cls[i]) continue;
      if (format == ISLE_TEXT_SPARSE) {
        p = mt_put_uint(p, (uint32_t)(col + 1), cd);
        *p++ = '\t';
        const uint32_t r1 = (uint32_t)(r0 + i + 1);
        p = mt_put_uint(p, r1, mt_ndigits(r1));
        *p++ = '\t';
        p = mt_weight(w[i], p);
        *p++ = '\n';
      } else {
        p = mt_entry(cls[i], w[i], p);
        *p++ = '\t';
      }
    }
    if (threadIdx.x == 0 && total < nbytes) text[shift + total] = '\n';  // DENSE: the column ends in this tile
    mt_store_tile(lines, shift, nbytes, out, dst0);
  }
}

// what must be undone however the chunk loop ends: nothing of it may still run when the call returns
struct MtPipe {
  isle_ctx* c;
  hipEvent_t formatted[2] = {nullptr, nullptr}, landed[2] = {nullptr, nullptr};
  explicit MtPipe(isle_ctx* c_) : c(c_) {}
  ~MtPipe() {
    (void)hipStreamSynchronize(c->stream);
    if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
    for (int i = 0; i < 2; ++i) {
      if (formatted[i]) (void)hipEventDestroy(formatted[i]);
      if (landed[i]) (void)hipEventDestroy(landed[i]);
    }
  }
};

}  // namespace

#define LAUNCH_CHECK(c) HIPCHK(c, hipGetLastError())

// The delivery of a text whose tiles are placed by offs_dev (ntiles + 1 exclusive 64-bit offsets on the device, offs[ntiles] = total > 0):
// chunks of at most ISLE_TEXT_CHUNK_BYTES, cut between tiles, at a multiple of `group` tiles where one lies inside the chunk (whole
// columns; group = 1: any tile); write(t0, n, out) launches on the context's stream what formats tiles [t0, t0 + n) into out (16-byte
// aligned, position offs[tile] - offs[t0]).  Two device and two pinned buffers: chunk i + 1 is formatted while chunk i is copied on the
// copy stream and consumed by the sink on the calling thread.
int k_text_pump(isle_ctx* c, const char* who, const uint64_t* offs_dev, uint64_t ntiles, uint64_t total, uint64_t group, isle_text_sink_fn sink,
                void* user, const std::function<int(uint64_t, uint64_t, unsigned char*)>& write) {
  std::vector<uint64_t> cut{0};
  std::vector<uint64_t> ho;
  if (total <= ISLE_TEXT_CHUNK_BYTES) {
    ho = {0, total};
    cut.push_back(ntiles);
  } else {
    ho.resize(ntiles + 1);
    HIPCHK(c, hipMemcpy(ho.data(), offs_dev, (ntiles + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
    for (uint64_t t0 = 0; t0 < ntiles;) {
      uint64_t t1 = (uint64_t)(std::upper_bound(ho.begin() + t0 + 1, ho.end(), ho[t0] + ISLE_TEXT_CHUNK_BYTES) - ho.begin()) - 1;  // > t0: a tile is < 37 KB
      if (t1 < ntiles && (t1 / group) * group > t0) t1 = (t1 / group) * group;
      cut.push_back(t1);
      t0 = t1;
    }
  }
  auto off_at = [&](uint64_t t) { return ho.size() == 2 ? (t ? total : 0) : ho[t]; };
  std::vector<std::pair<uint64_t, uint64_t>> chunks;  // (first tile, tiles), the empty ones dropped
  for (size_t i = 0; i + 1 < cut.size(); ++i)
    if (off_at(cut[i + 1]) > off_at(cut[i])) chunks.push_back({cut[i], cut[i + 1] - cut[i]});

  const size_t buf = (size_t)std::min<uint64_t>(total, ISLE_TEXT_CHUNK_BYTES) + 16;
  const int nbuf = chunks.size() > 1 ? 2 : 1;
  for (int i = 0; i < nbuf; ++i) {
    HIPCHK(c, c->mt_text[i].reserve(buf));
    HIPCHK(c, c->mt_pin[i].reserve(buf));
  }
  if (!c->copy_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
  MtPipe pipe(c);
  for (int i = 0; i < nbuf; ++i) {
    HIPCHK(c, hipEventCreateWithFlags(&pipe.formatted[i], hipEventDisableTiming));
    HIPCHK(c, hipEventCreateWithFlags(&pipe.landed[i], hipEventDisableTiming));
  }
  auto issue = [&](size_t i) -> int {
    const int s = (int)(i & 1);
    const uint64_t t0 = chunks[i].first, n = chunks[i].second, len = off_at(t0 + n) - off_at(t0);
    ISLECHK(write(t0, n, c->mt_text[s].p));
    HIPCHK(c, hipEventRecord(pipe.formatted[s], c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->copy_stream, pipe.formatted[s], 0));
    HIPCHK(c, hipMemcpyAsync(c->mt_pin[s].p, c->mt_text[s].p, len, hipMemcpyDeviceToHost, c->copy_stream));
    HIPCHK(c, hipEventRecord(pipe.landed[s], c->copy_stream));
    return 0;
  };
  ISLECHK(issue(0));
  for (size_t i = 0; i < chunks.size(); ++i) {
    // chunk i + 1 goes into the buffers chunk i - 1 used: its copy was waited for and its sink has returned
    if (i + 1 < chunks.size()) ISLECHK(issue(i + 1));
    HIPCHK(c, hipEventSynchronize(pipe.landed[i & 1]));
    const uint64_t len = off_at(chunks[i].first + chunks[i].second) - off_at(chunks[i].first);
    if (sink(c->mt_pin[i & 1].p, len, user) != 0)
      return isle_fail(c, ISLE_E_ARG, "%s: the sink refused piece %zu (%llu bytes)", who, i, (unsigned long long)len);
  }
  return 0;
}

int k_model_text(isle_ctx* c, const float* model_dev, uint64_t V, uint64_t ncols, const int64_t* pairs_dev, float a, float b, int format,
                 isle_text_sink_fn sink, void* user, uint64_t* nbytes, uint64_t* nentries) {
  if (nbytes) *nbytes = 0;
  if (nentries) *nentries = 0;
  if (ncols == 0) return 0;
  const uint64_t tpc = (V + MT_TILE - 1) / MT_TILE, ntiles = tpc * ncols;
  if (ntiles >= (1ull << 31)) return isle_fail(c, ISLE_E_ARG, "model_text: %llu x %llu entries are more than 2^31 tiles", (unsigned long long)V, (unsigned long long)ncols);
  const MtSrc src{model_dev, V, pairs_dev, a, b};
  const unsigned cap = (unsigned)c->num_cus * 16u;
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
    hipLaunchKernelGGL(mt_count_k, dim3((unsigned)std::min<uint64_t>(ntiles, cap)), dim3(MT), 0, c->stream, src, format, tpc, ntiles, c->mt_sizes.p, stat);
    LAUNCH_CHECK(c);
    HIPCHK(c, (isle_scan::exclusive_scan<uint32_t, uint64_t>(c->stream, c->mt_sizes.p, ntiles, c->mt_offs.p, c->mt_blk.p)));
  }
  HIPCHK(c, hipMemcpyAsync(h, stat, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(h + 2, c->mt_offs.p + ntiles, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (h[1] != ~0ull)
    return isle_fail(c, ISLE_E_ARG, "model_text: the entry at column %llu, row %llu (0-based) is negative, infinite or >= 2^31: the reference's writer is undefined for it",
                     (unsigned long long)(h[1] / V), (unsigned long long)(h[1] % V));
  const uint64_t total = h[2];
  if (nbytes) *nbytes = total;
  if (nentries) *nentries = h[0];
  if (!sink || total == 0) return 0;

  return k_text_pump(c, "model_text", c->mt_offs.p, ntiles, total, tpc, sink, user, [&](uint64_t t0, uint64_t n, unsigned char* out) -> int {
    TimeScope ts(c, ISLE_T_POST);
    hipLaunchKernelGGL(mt_write_k, dim3((unsigned)std::min<uint64_t>(n, cap)), dim3(MT), 0, c->stream, src, format, tpc, t0, n, c->mt_offs.p, out);
    LAUNCH_CHECK(c);
    return 0;
  });
}

extern "C" int isle_hip_entry_text(float w, int format, char* out16) {
  if (!out16 || (format != ISLE_TEXT_SPARSE && format != ISLE_TEXT_DENSE)) return -1;
  out16[0] = 0;
  const int cls = mt_class(w, format);
  if (cls <= 0) return cls;
  char* end = mt_entry(cls, w, out16);
  *end = 0;
  return (int)(end - out16);
}
