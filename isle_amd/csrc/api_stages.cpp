// isle_amd/csrc/api_stages.cpp — the stages either side of the hot path behind the C ABI: count matrix upload and tdf
// ingest, thresholding A -> B, catchwords / topic model / edge topics, inference.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdlib>
#include <cstring>
#include <numeric>

#include "api_internal.h"
#include "stage_host.h"
#include "topdocs_host.h"
#include "simdocs_host.h"
#include "prevalence_host.h"
#include "vocab_host.h"
#include "docs_host.h"
#include "match_host.h"

// ------------------------------------------------------------------------------------------
// upstream stage: A -> B on the device
// ------------------------------------------------------------------------------------------
// ---- what the four ways to a count matrix share (upload_counts, ingest_tdf, the feed, the text stream)
// who: the call's prefix of the message, colon included; upload_counts has none and takes a matrix without documents
static int shape_ok(isle_ctx* c, const char* who, uint64_t V, uint64_t D, bool no_docs_ok) {
  if (V == 0 || V > 0xfffffff0ull || (D == 0 && !no_docs_ok) || D > 0xfffffff0ull) return isle_fail(c, ISLE_E_ARG, "%svocab/doc count out of range", who);
  return 0;
}

static int entries_ok(isle_ctx* c, const char* who, uint64_t nread, uint64_t max_entries) {
  if (max_entries && nread != max_entries)  // include/utils.h:227
    return isle_fail(c, ISLE_E_ARG, "%s: file has %llu entries, <max_entries> says %llu", who, (unsigned long long)nread, (unsigned long long)max_entries);
  return 0;
}

// a_cnt / a_rows / a_offs and a_V / a_D / a_nnz are written: they become A, and what was derived from the A before is void
static int install_A(isle_ctx* c, uint64_t doc_offset, uint64_t docs_global, uint64_t entries, uint64_t* entries_out, uint64_t* nnz_out) {
  c->a_doc_offset = doc_offset;
  c->a_D_global = docs_global ? docs_global : c->a_D;
  c->res.A_installed();
  if (entries_out) *entries_out = entries;
  if (nnz_out) *nnz_out = c->a_nnz;
  return 0;
}

// The open feed or text stream goes, with rc: a device or allocation failure inside it, or its end.  Nothing of the caller's is in a
// queue any more when it does.
static int feed_discard(isle_ctx* c, int rc) {
  (void)hipStreamSynchronize(c->stream);
  c->feed.release();
  return rc;
}

// the entry of every call on an open feed (is_text false) or an open text stream (true): each refuses the other's
#define FEED_OPEN(who, is_text)                                                                                     \
  if (!c) return ISLE_E_ARG;                                                                                        \
  ISLECHK(isle_enter(c));                                                                                           \
  IsleFeed& f = c->feed;                                                                                            \
  if (!f.open || f.text != (is_text))                                                                               \
    return isle_fail(c, ISLE_E_ARG, "%s: no open %s", who, (is_text) ? "text stream (isle_hip_tdf_begin)" : "feed (isle_hip_feed_begin)")

extern "C" int isle_hip_upload_counts_u32(isle_ctx* c, uint64_t V, uint64_t D, uint64_t nnz, const float* counts, const uint32_t* rows,
                                          const int64_t* offs, uint64_t doc_offset, uint64_t docs_global) {
  if (!c) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  ISLECHK(shape_ok(c, "", V, D, true));
  if (offs[0] != 0 || (uint64_t)offs[D] != nnz) return isle_fail(c, ISLE_E_ARG, "offsets[0] != 0 or offsets[D] != nnz");
  for (uint64_t d = 0; d < D; ++d) {
    if (offs[d + 1] < offs[d]) return isle_fail(c, ISLE_E_ARG, "offsets not monotone at column %llu", (unsigned long long)d);
    for (int64_t i = offs[d]; i < offs[d + 1]; ++i) {
      if (rows[i] >= V) return isle_fail(c, ISLE_E_ARG, "row index out of range at %lld", (long long)i);
      if (i > offs[d] && rows[i] <= rows[i - 1])
        return isle_fail(c, ISLE_E_ARG, "rows not strictly ascending in column %llu", (unsigned long long)d);
      if (!(counts[i] > 0.f)) return isle_fail(c, ISLE_E_ARG, "count not positive at %lld", (long long)i);
    }
  }
  c->res.A_rewrite_begins();  // a_V / a_D / a_nnz and the buffers are rewritten from here: a failed allocation leaves no A
  c->a_V = V;
  c->a_D = D;
  c->a_nnz = nnz;
  HIPCHK(c, c->a_cnt.reserve(nnz ? nnz : 1));
  HIPCHK(c, c->a_rows.reserve(nnz ? nnz : 1));
  HIPCHK(c, c->a_offs.reserve(D + 1));
  if (nnz) {
    HIPCHK(c, hipMemcpy(c->a_cnt.p, counts, nnz * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->a_rows.p, rows, nnz * sizeof(uint32_t), hipMemcpyHostToDevice));
  }
  HIPCHK(c, hipMemcpy(c->a_offs.p, offs, (D + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
  return install_A(c, doc_offset, docs_global, nnz, nullptr, nullptr);
}

// what is wrong with a line of tdf text, by the kind ing_parse_line returns (ingest.hip)
static const char* const kTdfKind[] = {"", "bad character", "more than three fields", "fewer than three fields", "doc/word id is 0 or exceeds <num_docs>/<vocab_size>",
                                       "count is 0", "count exceeds 4294967295"};

extern "C" int isle_hip_ingest_tdf(isle_ctx* c, const char* text, uint64_t nbytes, uint64_t V, uint64_t D, uint64_t max_entries,
                                   uint64_t* entries_read, uint64_t* nnz) {
  if (!c) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  if (c->world > 1) return isle_fail(c, ISLE_E_ARG, "ingest_tdf: single-rank only");
  ISLECHK(shape_ok(c, "ingest_tdf: ", V, D, false));
  if (nbytes && !text) return isle_fail(c, ISLE_E_ARG, "ingest_tdf: null text");
  c->res.A_rewrite_begins();
  DevBuf<unsigned char> td;
  StreamDrain drain(c);
  HIPCHK(c, td.reserve(nbytes + 16));
  if (nbytes) HIPCHK(c, hipMemcpy(td.p, text, nbytes, hipMemcpyHostToDevice));
  uint64_t nread = 0, err[2] = {0, 0};
  ISLECHK(k_ingest_tdf(c, td.p, nbytes, V, D, &nread, err));
  if (err[0]) {
    return isle_fail(c, ISLE_E_ARG, "ingest_tdf: %s on line %llu", kTdfKind[err[0] < 7 ? err[0] : 0], (unsigned long long)(err[1] + 1));
  }
  ISLECHK(entries_ok(c, "ingest_tdf", nread, max_entries));
  return install_A(c, 0, 0, nread, entries_read, nnz);
}

// ---- (doc, word, count) triples in batches -> A (ingest.hip: feed_key_k, then the tail tdf ingest runs)
extern "C" int isle_hip_feed_begin(isle_ctx* c, uint64_t V, uint64_t D, uint64_t reserve_entries) {
  if (!c) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  c->feed.release();  // an open feed, or an open text stream, is discarded
  ISLECHK(shape_ok(c, "feed_begin: ", V, D, false));
  if (reserve_entries) {
    hipError_t e = c->feed.key.reserve(reserve_entries);
    if (e == hipSuccess) e = c->feed.cnt.reserve(reserve_entries);
    if (e != hipSuccess) c->feed.release();
    HIPCHK(c, e);
  }
  c->feed.V = V;
  c->feed.D = D;
  c->feed.open = true;
  return 0;
}

extern "C" int isle_hip_feed_entries(isle_ctx* c, uint64_t n, const uint32_t* docs, const uint32_t* words, const uint32_t* counts) {
  return isle_hip_feed_entries_pieces(c, n, docs, words, counts, 0);
}

extern "C" int isle_hip_feed_entries_pieces(isle_ctx* c, uint64_t n, const uint32_t* docs, const uint32_t* words, const uint32_t* counts,
                                            uint64_t piece_entries) {
  FEED_OPEN("feed_entries", false);
  if (n == 0) return 0;
  if (!docs || !words || !counts) return isle_fail(c, ISLE_E_ARG, "feed_entries: null array");
  const uint64_t piece = (piece_entries && piece_entries < ISLE_FEED_CHUNK) ? piece_entries : ISLE_FEED_CHUNK;
  const uint64_t n0 = f.n, offered0 = f.offered;  // a batch is taken whole or not at all
  for (uint64_t at = 0; at < n; at += piece) {
    uint64_t bad = ~0ull;
    const int rc = k_feed_chunk(c, docs + at, words + at, counts + at, std::min<uint64_t>(piece, n - at), &bad);
    if (rc) return feed_discard(c, rc);  // once no copy from the caller's arrays is queued any more
    if (bad != ~0ull) {
      f.n = n0;
      f.offered = offered0;
      return isle_fail(c, ISLE_E_ARG, "feed_entries: %s id out of range at entry %llu (0-based, counted from feed_begin)",
                       (bad & 7ull) == 1 ? "document" : "word", (unsigned long long)(bad >> 3));
    }
  }
  return 0;
}

extern "C" int isle_hip_feed_finalize(isle_ctx* c, uint64_t doc_offset, uint64_t docs_global, uint64_t* entries_fed, uint64_t* nnz) {
  FEED_OPEN("feed_finalize", false);
  c->res.A_rewrite_begins();  // a_cnt / a_rows / a_offs are rewritten from here
  const uint64_t fed = f.n;
  ISLECHK(feed_discard(c, k_feed_finalize(c)));
  return install_A(c, doc_offset, docs_global, fed, entries_fed, nnz);
}

// ---- tdf text in pieces cut anywhere -> A (ingest.hip: the whole text's kernels and tdf_advance_k per piece, then the feed's tail)
// Waits for the piece in flight; ISLE_E_ARG naming the first bad line of the text so far, if there is one (the stream is discarded).
static int tdf_settle(isle_ctx* c, const char* who) {
  const int rc = k_tdf_wait(c);
  if (rc) return feed_discard(c, rc);
  const uint64_t bad = c->feed.known.err;
  if (bad == ~0ull || c->feed.counting) return 0;  // (a counting stream refuses no line: the windowed pass names the first bad line of the file)
  c->feed.release();
  return isle_fail(c, ISLE_E_ARG, "%s: %s on line %llu", who, kTdfKind[(bad & 7ull) < 7 ? (bad & 7ull) : 0], (unsigned long long)((bad >> 3) + 1));
}

// what the three ways to open a text stream share: the shape, the piece size, the store's reservation (none: a counting stream), the
// page-locked buffers, the device state.  The stream is not yet open when this returns.
static int tdf_open_stream(isle_ctx* c, const char* who, uint64_t V, uint64_t D, uint64_t reserve_entries, uint64_t piece_bytes) {
  IsleFeed& f = c->feed;
  ISLECHK(shape_ok(c, who, V, D, false));
  f.V = V;
  f.D = D;
  f.piece = (piece_bytes && piece_bytes < ISLE_TDF_PIECE) ? piece_bytes : ISLE_TDF_PIECE;
  hipError_t e = hipSuccess;
  if (reserve_entries) {  // with the headroom of one piece's bound (k_tdf_piece): a hint that is exact never makes the store grow
    const uint64_t room = reserve_entries + f.piece / 6 + 1;
    e = f.key.reserve(room);
    if (e == hipSuccess) e = f.cnt.reserve(room);
  }
  for (int i = 0; i < 2 && e == hipSuccess; ++i) e = f.t_pin[i].reserve(f.piece);
  int rc = 0;
  if (e == hipSuccess) rc = k_tdf_open(c);
  if (e != hipSuccess || rc) f.release();
  HIPCHK(c, e);
  return rc;
}

extern "C" int isle_hip_tdf_begin(isle_ctx* c, uint64_t V, uint64_t D, uint64_t reserve_entries, uint64_t piece_bytes) {
  if (!c) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  IsleFeed& f = c->feed;
  f.release();  // an open text stream, or an open feed, is discarded
  if (c->world > 1) return isle_fail(c, ISLE_E_ARG, "tdf_begin: single-rank only");
  ISLECHK(tdf_open_stream(c, "tdf_begin: ", V, D, reserve_entries, piece_bytes));
  f.open = f.text = true;
  return 0;
}

// ---- one tdf file onto document shards: the counting stream and its plan (pass 1), the windowed stream (pass 2)
extern "C" int isle_hip_tdf_begin_counts(isle_ctx* c, uint64_t V, uint64_t D, uint64_t piece_bytes) {
  if (!c) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  IsleFeed& f = c->feed;
  f.release();
  ISLECHK(tdf_open_stream(c, "tdf_begin_counts: ", V, D, 0, piece_bytes));
  f.counting = true;
  const int rc = k_tdf_open_counts(c);
  if (rc) return feed_discard(c, rc);
  f.open = f.text = true;
  return 0;
}

extern "C" int isle_hip_tdf_begin_window(isle_ctx* c, uint64_t V, uint64_t D, uint64_t doc_begin, uint64_t doc_end, uint64_t reserve_entries,
                                         uint64_t piece_bytes) {
  if (!c) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  IsleFeed& f = c->feed;
  f.release();
  if (doc_begin > doc_end || doc_end > D)
    return isle_fail(c, ISLE_E_ARG, "tdf_begin_window: documents [%llu, %llu) of %llu", (unsigned long long)doc_begin, (unsigned long long)doc_end, (unsigned long long)D);
  ISLECHK(tdf_open_stream(c, "tdf_begin_window: ", V, D, reserve_entries, piece_bytes));
  f.windowed = true;
  f.w_begin = doc_begin;
  f.w_end = doc_end;
  f.open = f.text = true;
  return 0;
}

// The end of a counting stream.  Collective with several ranks: every collective below is issued by all ranks or by none (ranks that
// disagree on agree_tag all leave behind the first).
extern "C" int isle_hip_tdf_finalize_counts(isle_ctx* c, int parts, uint64_t agree_tag, uint64_t* bounds, uint32_t* doc_lines, uint64_t* lines_local,
                                            uint64_t* lines_global) {
  if (!c) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  IsleFeed& f = c->feed;
  if (!f.open || !f.text || !f.counting) return isle_fail(c, ISLE_E_ARG, "tdf_finalize_counts: no open counting stream (isle_hip_tdf_begin_counts)");
  if (parts < 1 || !bounds) {
    f.release();
    return isle_fail(c, ISLE_E_ARG, "tdf_finalize_counts: parts < 1 or null bounds");
  }
  ISLECHK(tdf_settle(c, "tdf_finalize_counts"));
  if (f.known.carry) {  // the bytes behind the last '\n': the last line
    const int rc = k_tdf_piece(c, nullptr, 0, true);
    if (rc) return feed_discard(c, rc);
    ISLECHK(tdf_settle(c, "tdf_finalize_counts"));
  }
  const uint64_t local = f.known.seen;
  uint64_t global = local;
  k_tdf_release_text(c);
  if (c->multi()) {
    DevBuf<uint64_t> word;
    StreamDrain drain(c);
    hipError_t e = word.reserve(2);
    if (e != hipSuccess) f.release();
    HIPCHK(c, e);
    uint64_t tag[2] = {agree_tag, ~agree_tag};  // max over (v, ~v): the largest and the complement of the smallest
    int rc = allreduce_host<uint64_t>(c, tag, 2, word.p, true);
    if (rc) return feed_discard(c, rc);
    if (tag[0] != ~tag[1]) {
      f.release();
      return isle_fail(c, ISLE_E_COMM, "tdf_finalize_counts: ranks disagree on agree_tag (min %llu, max %llu): not the same file", (unsigned long long)~tag[1],
                       (unsigned long long)tag[0]);
    }
    rc = allreduce_sum<uint32_t>(c, f.t_doc_cnt.p, (size_t)f.D);
    if (rc == 0) rc = allreduce_host<uint64_t>(c, &global, 1, word.p);
    if (rc) return feed_discard(c, rc);
  }
  if (lines_local) *lines_local = local;
  if (lines_global) *lines_global = global;
  if (global > 0xffffffffull) {  // a summed 32-bit counter may have wrapped
    f.release();
    return isle_fail(c, ISLE_E_ARG, "tdf_finalize_counts: %llu lines, more than 4294967295: the per-document counters are 32 bits wide", (unsigned long long)global);
  }
  int rc = k_tdf_plan(c, global, parts, bounds);
  if (rc == 0 && doc_lines) {
    const hipError_t e = hipMemcpy(doc_lines, f.t_doc_cnt.p, (size_t)f.D * sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = isle_fail(c, ISLE_E_HIP, "tdf_finalize_counts: %s", hipGetErrorString(e));
  }
  return feed_discard(c, rc);
}

extern "C" int isle_hip_tdf_acquire(isle_ctx* c, char** buf, uint64_t* cap) {
  FEED_OPEN("tdf_acquire", true);
  if (!buf || !cap) return isle_fail(c, ISLE_E_ARG, "tdf_acquire: null argument");
  if (f.acquired) return isle_fail(c, ISLE_E_ARG, "tdf_acquire: the buffer handed out before has not been committed");
  // t_pin[pieces & 1] was the source of piece `pieces - 2`, which the commit of piece `pieces - 1` waited for: free by now
  f.acquired = true;
  *buf = f.t_pin[f.pieces & 1].p;
  *cap = f.piece;
  return 0;
}

extern "C" int isle_hip_tdf_commit(isle_ctx* c, uint64_t nbytes) {
  FEED_OPEN("tdf_commit", true);
  if (!f.acquired) return isle_fail(c, ISLE_E_ARG, "tdf_commit: no buffer acquired (isle_hip_tdf_acquire)");
  if (nbytes > f.piece) return isle_fail(c, ISLE_E_ARG, "tdf_commit: %llu bytes in a buffer of %llu", (unsigned long long)nbytes, (unsigned long long)f.piece);
  f.acquired = false;
  if (nbytes == 0) return 0;
  ISLECHK(tdf_settle(c, "tdf_commit"));  // the piece before: its counts size this one, its carry says where this one lands
  const int rc = k_tdf_piece(c, f.t_pin[f.pieces & 1].p, nbytes, false);
  return rc ? feed_discard(c, rc) : 0;
}

extern "C" int isle_hip_tdf_write(isle_ctx* c, const char* bytes, uint64_t nbytes) {
  FEED_OPEN("tdf_write", true);
  if (nbytes && !bytes) return isle_fail(c, ISLE_E_ARG, "tdf_write: null text");
  if (f.acquired) return isle_fail(c, ISLE_E_ARG, "tdf_write: a buffer is acquired and not committed");
  for (uint64_t at = 0; at < nbytes;) {
    char* buf = nullptr;
    uint64_t cap = 0;
    ISLECHK(isle_hip_tdf_acquire(c, &buf, &cap));
    const uint64_t n = std::min<uint64_t>(cap, nbytes - at);
    memcpy(buf, bytes + at, n);
    ISLECHK(isle_hip_tdf_commit(c, n));
    at += n;
  }
  return 0;
}

extern "C" int isle_hip_tdf_finalize(isle_ctx* c, uint64_t max_entries, uint64_t* entries_read, uint64_t* nnz) {
  FEED_OPEN("tdf_finalize", true);
  if (f.counting) return isle_fail(c, ISLE_E_ARG, "tdf_finalize: the open stream counts lines (isle_hip_tdf_finalize_counts ends it)");
  ISLECHK(tdf_settle(c, "tdf_finalize"));
  if (f.known.carry) {  // the text does not end in '\n': what is left is its last line
    const int rc = k_tdf_piece(c, nullptr, 0, true);
    if (rc) return feed_discard(c, rc);
    ISLECHK(tdf_settle(c, "tdf_finalize"));
  }
  const uint64_t nread = f.known.seen;  // the valid lines of the whole text: on an ordinary stream also the entries held
  const uint64_t doc_offset = f.windowed ? f.w_begin : 0, docs_global = f.windowed ? f.D : 0;
  const int refused = entries_ok(c, "tdf_finalize", nread, max_entries);
  if (refused) {
    f.release();
    return refused;
  }
  c->res.A_rewrite_begins();  // a_cnt / a_rows / a_offs are rewritten from here
  f.n = f.known.entries;
  k_tdf_release_text(c);
  ISLECHK(feed_discard(c, k_feed_finalize(c)));
  return install_A(c, doc_offset, docs_global, nread, entries_read, nnz);
}

extern "C" int isle_hip_get_A(isle_ctx* c, float* counts, uint32_t* rows, int64_t* offs) {
  if (!c) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  if (!c->res.a_ready) return isle_fail(c, ISLE_E_ARG, "get_A: no count matrix");
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (counts && c->a_nnz) HIPCHK(c, hipMemcpy(counts, c->a_cnt.p, c->a_nnz * sizeof(float), hipMemcpyDeviceToHost));
  if (rows && c->a_nnz) HIPCHK(c, hipMemcpy(rows, c->a_rows.p, c->a_nnz * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (offs) HIPCHK(c, hipMemcpy(offs, c->a_offs.p, (c->a_D + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
  return 0;
}

// ---- the vocabulary pruned by document frequency (vocab.hip; the rule: vocab_host.h)
// Several ranks hold the same n <= 6 control values, or all return ISLE_E_COMM: max over (v, ~v) gives the largest and the complement of
// the smallest (in the transport's order of the words, signed or not: equal on all ranks exactly where the two agree)
static const char* const kVocabCtl[4] = {"vocab_size", "min_df", "max_df", "keep_n"};
static int vocab_agree(isle_ctx* c, const char* who, const uint64_t* v, int n, const char* const* name = kVocabCtl) {
  if (!c->multi()) return 0;
  DevBuf<uint64_t> word;
  StreamDrain drain(c);
  HIPCHK(c, word.reserve(12));
  uint64_t tag[12];
  for (int i = 0; i < n; ++i) tag[2 * i] = v[i], tag[2 * i + 1] = ~v[i];
  ISLECHK(allreduce_host<uint64_t>(c, tag, 2 * (size_t)n, word.p, true));
  for (int i = 0; i < n; ++i)
    if (tag[2 * i] != ~tag[2 * i + 1])
      return isle_fail(c, ISLE_E_COMM, "%s: ranks disagree on %s (%llu and %llu)", who, name[i], (unsigned long long)~tag[2 * i + 1], (unsigned long long)tag[2 * i]);
  return 0;
}

// what both calls check of the resident A before any collective: a rank's own refusals
static int vocab_A_ok(isle_ctx* c, const char* who) {
  if (!c->res.a_ready) return isle_fail(c, ISLE_E_ARG, "%s: no count matrix", who);
  if (c->a_D_global > 0xfffffff0ull)
    return isle_fail(c, ISLE_E_ARG, "%s: %llu documents in the corpus, more than 4294967280: the counters are 32 bits wide", who, (unsigned long long)c->a_D_global);
  return 0;
}

// df of the corpus: this rank's histogram, summed over the ranks, on the device (df_dev, a_V words) and on the host
static int vocab_df_corpus(isle_ctx* c, DevBuf<uint32_t>& df_dev, std::vector<uint32_t>& df) {
  HIPCHK(c, df_dev.reserve((size_t)c->a_V));
  ISLECHK(k_vocab_df(c, route_vocab_hist(c->vocab_hist_form), df_dev.p));
  ISLECHK(allreduce_sum<uint32_t>(c, df_dev.p, (size_t)c->a_V));
  df.resize((size_t)c->a_V);
  HIPCHK(c, hipMemcpyAsync(df.data(), df_dev.p, (size_t)c->a_V * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int isle_hip_vocab_hist_form(isle_ctx* c, int form) {
  if (!c) return ISLE_E_ARG;
  if (form != ISLE_VOCAB_HIST_AUTO && form != ISLE_VOCAB_HIST_LDS && form != ISLE_VOCAB_HIST_GLOBAL)
    return isle_fail(c, ISLE_E_ARG, "vocab_hist_form: unknown form %d", form);
  c->vocab_hist_form = form;
  return 0;
}

extern "C" int isle_hip_word_doc_freq(isle_ctx* c, uint32_t* df_out) {
  if (!c) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  ISLECHK(vocab_A_ok(c, "word_doc_freq"));
  DevBuf<uint32_t> df_dev;
  StreamDrain drain(c);
  ISLECHK(vocab_agree(c, "word_doc_freq", &c->a_V, 1));  // (every local refusal lies before this line)
  std::vector<uint32_t> df;
  ISLECHK(vocab_df_corpus(c, df_dev, df));
  if (df_out) std::copy(df.begin(), df.end(), df_out);
  return 0;
}

// For the ledger an ingest of the pruned matrix: A_rewrite_begins is raised once the rule has accepted and the pruned matrix lies complete
// in the twin buffers, right before they are swapped in; install_A ends it.  Every refusal leaves A and everything resident as it was.
extern "C" int isle_hip_prune_vocab(isle_ctx* c, uint64_t min_df, uint64_t max_df, uint64_t keep_n, uint64_t* new_vocab, uint32_t* kept_words, uint32_t* df_out,
                                    uint64_t* nnz_out, uint64_t* docs_emptied) {
  if (!c) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  ISLECHK(vocab_A_ok(c, "prune_vocab"));
  DevBuf<uint32_t> df_dev, remap_dev, new_rows;
  DevBuf<float> new_cnt;
  DevBuf<int64_t> new_offs;
  DevBuf<uint64_t> word;
  StreamDrain drain(c);
  const uint64_t agreed[4] = {c->a_V, min_df, max_df, keep_n};
  ISLECHK(vocab_agree(c, "prune_vocab", agreed, 4));  // (every local refusal lies before this line; the ones below are the same on every rank)
  const std::string why = vocab_check_args(true, min_df, max_df, keep_n, c->a_D_global);
  if (!why.empty()) return isle_fail(c, ISLE_E_ARG, "%s", why.c_str());
  std::vector<uint32_t> df, remap, kept;
  ISLECHK(vocab_df_corpus(c, df_dev, df));
  const std::string none = vocab_rule(df.data(), c->a_V, min_df, max_df, keep_n, c->a_D_global, remap, kept);
  if (!none.empty()) return isle_fail(c, ISLE_E_ARG, "%s", none.c_str());
  // the pruned matrix out of place
  HIPCHK(c, remap_dev.reserve((size_t)c->a_V));
  HIPCHK(c, hipMemcpyAsync(remap_dev.p, remap.data(), (size_t)c->a_V * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  uint64_t total = 0, emptied = 0;
  ISLECHK(k_vocab_compact(c, remap_dev.p, new_cnt, new_rows, new_offs, &total, &emptied));
  if (c->multi()) {
    HIPCHK(c, word.reserve(1));
    ISLECHK(allreduce_host<uint64_t>(c, &emptied, 1, word.p));
  }
  // ... and swapped in: the old buffers go with this call
  c->res.A_rewrite_begins();
  std::swap(c->a_cnt.p, new_cnt.p), std::swap(c->a_cnt.cap, new_cnt.cap);
  std::swap(c->a_rows.p, new_rows.p), std::swap(c->a_rows.cap, new_rows.cap);
  std::swap(c->a_offs.p, new_offs.p), std::swap(c->a_offs.cap, new_offs.cap);
  c->a_V = kept.size();
  c->a_nnz = total;
  if (new_vocab) *new_vocab = kept.size();
  if (kept_words) std::copy(kept.begin(), kept.end(), kept_words);
  if (df_out) std::copy(df.begin(), df.end(), df_out);
  if (docs_emptied) *docs_emptied = emptied;
  return install_A(c, c->a_doc_offset, c->a_D_global, total, nullptr, nnz_out);
}

// ---- documents pruned by length and as exact duplicates (docs.hip; the rule: docs_host.h)
// what the three calls check before any collective: a rank's own refusals (the bounds are checked behind the ranks' agreement on them)
static int docs_A_ok(isle_ctx* c, const char* who, int drop_duplicates) {
  const std::string why = docs_check_args(who, c->res.a_ready, DocsBounds{0, 0, 0, 0}, drop_duplicates, c->world);
  if (!why.empty()) return isle_fail(c, ISLE_E_ARG, "%s", why.c_str());
  return 0;
}

extern "C" int isle_hip_doc_hash_form(isle_ctx* c, int form) {
  if (!c) return ISLE_E_ARG;
  if (form != ISLE_DOC_HASH_AUTO && form != ISLE_DOC_HASH_FULL && form != ISLE_DOC_HASH_NARROW)
    return isle_fail(c, ISLE_E_ARG, "doc_hash_form: unknown form %d", form);
  c->doc_hash_form = form;
  return 0;
}

extern "C" int isle_hip_doc_lengths(isle_ctx* c, uint32_t* words_out, uint64_t* tokens_out) {
  if (!c) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  ISLECHK(docs_A_ok(c, "doc_lengths", 0));
  const uint64_t D = c->a_D;
  DevBuf<uint32_t> words;
  DevBuf<uint64_t> tokens;
  StreamDrain drain(c);
  HIPCHK(c, words.reserve(D ? D : 1));
  HIPCHK(c, tokens.reserve(D ? D : 1));
  ISLECHK(k_docs_len_hash(c, words.p, tokens.p, nullptr));
  if (words_out && D) HIPCHK(c, hipMemcpyAsync(words_out, words.p, D * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  if (tokens_out && D) HIPCHK(c, hipMemcpyAsync(tokens_out, tokens.p, D * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int isle_hip_doc_duplicates(isle_ctx* c, uint32_t* first_of_out, uint64_t* n_duplicates) {
  if (!c) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  ISLECHK(docs_A_ok(c, "doc_duplicates", 1));
  const uint64_t D = c->a_D;
  DevBuf<uint32_t> words, first_of;
  DevBuf<uint64_t> tokens, hash;
  StreamDrain drain(c);
  HIPCHK(c, words.reserve(D ? D : 1));
  HIPCHK(c, tokens.reserve(D ? D : 1));
  HIPCHK(c, hash.reserve(D ? D : 1));
  HIPCHK(c, first_of.reserve(D ? D : 1));
  ISLECHK(k_docs_len_hash(c, words.p, tokens.p, hash.p));
  uint64_t dups = 0, rounds = 0;
  ISLECHK(k_docs_first_of(c, route_doc_hash(c->doc_hash_form), words.p, hash.p, first_of.p, &dups, &rounds));
  if (first_of_out && D) HIPCHK(c, hipMemcpyAsync(first_of_out, first_of.p, D * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (n_duplicates) *n_duplicates = dups;
  return 0;
}

// For the ledger an ingest of the pruned matrix, as isle_hip_prune_vocab: A_rewrite_begins is raised once every refusal is behind and the
// pruned matrix lies complete in the twin buffers, right before they are swapped in; install_A ends it.
extern "C" int isle_hip_prune_docs(isle_ctx* c, uint64_t min_words, uint64_t max_words, uint64_t min_tokens, uint64_t max_tokens, int drop_duplicates,
                                   uint64_t* new_docs_out, uint32_t* kept_docs_out, uint32_t* first_of_out, uint64_t* nnz_out, uint64_t* docs_global_out,
                                   uint64_t dropped_out[3]) {
  if (!c) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  ISLECHK(docs_A_ok(c, "prune_docs", drop_duplicates));
  const uint64_t D = c->a_D;
  const DocsBounds b = {min_words, max_words, min_tokens, max_tokens};
  DevBuf<uint32_t> words, first_of, keep, kept_docs, new_rows;
  DevBuf<uint64_t> tokens, hash, word;
  DevBuf<float> new_cnt;
  DevBuf<int64_t> new_offs;
  StreamDrain drain(c);
  static const char* const kDocsCtl[6] = {"vocab_size", "min_words", "max_words", "min_tokens", "max_tokens", "drop_duplicates"};
  const uint64_t agreed[6] = {c->a_V, min_words, max_words, min_tokens, max_tokens, (uint64_t)drop_duplicates};
  ISLECHK(vocab_agree(c, "prune_docs", agreed, 6, kDocsCtl));  // (every local refusal lies before this line; the ones below are the same on every rank)
  const std::string why = docs_check_args("prune_docs", true, b, drop_duplicates, c->world);
  if (!why.empty()) return isle_fail(c, ISLE_E_ARG, "%s", why.c_str());
  // ---- the rule's flags
  HIPCHK(c, words.reserve(D ? D : 1));
  HIPCHK(c, tokens.reserve(D ? D : 1));
  HIPCHK(c, first_of.reserve(D ? D : 1));
  HIPCHK(c, keep.reserve(D ? D : 1));
  HIPCHK(c, kept_docs.reserve(D ? D : 1));
  if (drop_duplicates) HIPCHK(c, hash.reserve(D ? D : 1));
  ISLECHK(k_docs_len_hash(c, words.p, tokens.p, drop_duplicates ? hash.p : nullptr));
  if (drop_duplicates) {
    uint64_t dups = 0, rounds = 0;
    ISLECHK(k_docs_first_of(c, route_doc_hash(c->doc_hash_form), words.p, hash.p, first_of.p, &dups, &rounds));
  }
  const uint64_t bounds[4] = {min_words, max_words, min_tokens, max_tokens};
  uint64_t dropped[3] = {0, 0, 0}, kept = 0;
  ISLECHK(k_docs_keep(c, words.p, tokens.p, bounds, drop_duplicates != 0, first_of.p, keep.p, dropped, &kept));
  // ---- the corpus's numbers: the ranks' kept counts (the own slot set, summed), then dropped
  const size_t world = (size_t)std::max(1, c->world);
  std::vector<uint64_t> sums(world + 3, 0);
  sums[c->multi() ? (size_t)c->rank : 0] = kept;
  std::copy(dropped, dropped + 3, sums.begin() + world);
  if (c->multi()) {
    HIPCHK(c, word.reserve(world + 3));
    ISLECHK(allreduce_host<uint64_t>(c, sums.data(), world + 3, word.p));
  }
  uint64_t docs_global = 0, doc_offset = 0;
  for (size_t q = 0; q < world; ++q) {
    if (c->multi() && q < (size_t)c->rank) doc_offset += sums[q];
    docs_global += sums[q];
  }
  if (!docs_global) return isle_fail(c, ISLE_E_ARG, "%s", docs_none_kept(b, drop_duplicates).c_str());
  // ---- the pruned matrix out of place
  uint64_t total = 0;
  ISLECHK(k_docs_compact(c, keep.p, words.p, kept, new_cnt, new_rows, new_offs, kept_docs.p, &total));
  if (kept_docs_out && kept) HIPCHK(c, hipMemcpyAsync(kept_docs_out, kept_docs.p, kept * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  if (first_of_out && D) HIPCHK(c, hipMemcpyAsync(first_of_out, first_of.p, D * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  // ... and swapped in: the old buffers go with this call
  c->res.A_rewrite_begins();
  std::swap(c->a_cnt.p, new_cnt.p), std::swap(c->a_cnt.cap, new_cnt.cap);
  std::swap(c->a_rows.p, new_rows.p), std::swap(c->a_rows.cap, new_rows.cap);
  std::swap(c->a_offs.p, new_offs.p), std::swap(c->a_offs.cap, new_offs.cap);
  c->a_D = kept;
  c->a_nnz = total;
  if (new_docs_out) *new_docs_out = kept;
  if (docs_global_out) *docs_global_out = docs_global;
  if (dropped_out) std::copy(sums.begin() + world, sums.end(), dropped_out);
  return install_A(c, doc_offset, docs_global, total, nullptr, nnz_out);
}

// isle_hip_threshold, A -> B: the scalars its steps hand on.  What the host decides between them is stage_host.h.
struct Th {
  isle_ctx* c;
  const uint64_t num_topics;
  const double sample_rate;
  const uint64_t sample_seed;
  const bool sampling;
  const uint64_t V, D;
  uint64_t* st_dev = nullptr;  // two words of a_scan: the statistics, then the scratch of the host values' collectives
  uint64_t nz_docs = 0;
  float avg = 0.f;
  uint32_t maxv = 0;
  uint64_t bnnz = 0, Db = 0, b_off = 0, b_glob = 0;  // nnz(B), columns of B (local), this shard's first column, columns of B (global)

  Th(isle_ctx* c_, uint64_t num_topics_, double rate, uint64_t seed)
      : c(c_), num_topics(num_topics_), sample_rate(rate), sample_seed(seed), sampling(rate > 0.0 && rate < 1.0), V(c_->a_V), D(c_->a_D) {}

  int stats(float* avg_out) {  // corpus statistics (src/sparseMatrix.cpp:92-99), global
    HIPCHK(c, c->a_scan.reserve(isle_scan_scratch(D) + 4));
    st_dev = (uint64_t*)c->a_scan.p;
    ISLECHK(k_th_stats(c, st_dev));
    ISLECHK(allreduce_sum<uint64_t>(c, st_dev, 2));
    uint64_t st[2];
    HIPCHK(c, hipMemcpyAsync(st, st_dev, sizeof(st), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    nz_docs = st[1];
    avg = corpus_avg(st[0], nz_docs);
    if (avg_out) *avg_out = avg;
    c->a_avg = avg;
    c->res.corpus_average_known();
    if (!hist_maxv(avg, &maxv)) return isle_fail(c, ISLE_E_ARG, "threshold: average document size %g too large", (double)avg);
    return 0;
  }

  int round_and_histogram() {  // rounded normalised counts + per-word value histogram, global
    HIPCHK(c, c->a_q.reserve(c->a_nnz ? c->a_nnz : 1));
    HIPCHK(c, c->a_hist.reserve((size_t)V * (maxv + 1)));
    ISLECHK(k_th_round_hist(c, avg, maxv));
    return allreduce_sum<uint32_t>(c, c->a_hist.p, (size_t)V * (maxv + 1));
  }

  int zetas() {
    const ThresholdCounts n = threshold_counts(nz_docs, num_topics);
    HIPCHK(c, c->zetas.reserve(V));
    return k_th_zetas(c, maxv, n.gr, n.eq);
  }

  int count_survivors(uint64_t* entries_above) {  // survivors per document
    HIPCHK(c, c->a_kept.reserve(D ? D : 1));
    if (sampling) HIPCHK(c, c->a_wgt.reserve(D ? D : 1));
    ISLECHK(k_th_count(c, sampling));
    ISLECHK(k_th_scans(c));
    int64_t above_local = 0;
    HIPCHK(c, hipMemcpyAsync(&above_local, c->a_off_all.p + D, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (entries_above) {
      uint64_t g = (uint64_t)above_local;
      ISLECHK(allreduce_host<uint64_t>(c, &g, 1, st_dev));
      *entries_above = g;
    }
    return 0;
  }

  // all keys of the corpus on every rank: shards padded with -1 to the largest one.  dice: this shard's keys in, every shard's block out
  int gather_keys(std::vector<float>& dice) {
    uint64_t dmax = D;
    ISLECHK(allreduce_host<uint64_t>(c, &dmax, 1, st_dev, true, false /*not counted among the collectives' time, as before*/));
    const std::vector<float> mine = sample_pad(dice, dmax);
    const size_t slots = mine.size();
    DevBuf<float> keys_all;
    StreamDrain drain(c);
    HIPCHK(c, keys_all.reserve((size_t)c->world * slots));
    HIPCHK(c, hipMemcpy(keys_all.p + (size_t)c->rank * slots, mine.data(), slots * sizeof(float), hipMemcpyHostToDevice));
    {
      TimeScope ts(c, ISLE_T_COMM);
      ISLECHK(isle_allgather(c, keys_all.p + (size_t)c->rank * slots, keys_all.p, slots, ISLE_DT_F32));
    }
    dice.assign((size_t)c->world * slots, 0.f);
    HIPCHK(c, hipMemcpyAsync(dice.data(), keys_all.p, dice.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
  }

  int sample() {  // sampled_threshold_and_copy, src/sparseMatrix.cpp:1383-1415
    if (!(sampling && (D || c->multi()))) return 0;
    std::vector<float> wgt(D);
    if (D) HIPCHK(c, hipMemcpy(wgt.data(), c->a_wgt.p, D * sizeof(float), hipMemcpyDeviceToHost));
    const std::vector<float> key = sample_keys(sample_seed, c->a_doc_offset, wgt);
    std::vector<float> dice(key);
    if (c->multi()) ISLECHK(gather_keys(dice));
    const std::vector<uint8_t> drop = drop_mask(key, sample_pivot(sample_rate, dice));
    DevBuf<uint8_t> drop_dev;
    StreamDrain drain(c);
    HIPCHK(c, drop_dev.reserve(drop.size()));
    if (D) HIPCHK(c, hipMemcpy(drop_dev.p, drop.data(), D, hipMemcpyHostToDevice));
    if (D) ISLECHK(k_th_drop(c, drop_dev.p));
    return k_th_scans(c);
  }

  int place_shard() {  // placement of this shard in B's global column numbering
    int64_t tail[2];  // nnz(B), columns of B (local)
    HIPCHK(c, hipMemcpyAsync(&tail[0], c->a_off_all.p + D, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&tail[1], c->a_col_of.p + D, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    bnnz = (uint64_t)tail[0];
    Db = b_glob = (uint64_t)tail[1];
    if (c->multi()) {
      DevBuf<uint64_t> all;
      StreamDrain drain(c);
      HIPCHK(c, all.reserve((size_t)c->world + 1));
      std::vector<uint64_t> h(c->world);
      ISLECHK(allgather_host<uint64_t>(c, &Db, 1, all.p, h.data()));
      const ShardPlace s = shard_placement(c->rank, h);
      b_off = s.b_off;
      b_glob = s.b_glob;
    }
    return 0;
  }

  int emit(uint64_t* docs_kept, uint64_t* nnz_kept) {
    isle_trim_derived(c, Db, bnnz);
    c->V = V;
    c->D = Db;
    c->nnz = bnnz;
    c->doc_offset = b_off;
    c->D_global = b_glob;
    HIPCHK(c, c->vals.reserve(bnnz ? bnnz : 1));
    HIPCHK(c, c->rows.reserve(bnnz ? bnnz : 1));
    HIPCHK(c, c->offs.reserve(Db + 1));
    HIPCHK(c, c->original_cols.reserve(Db ? Db : 1));
    if (D == 0) HIPCHK(c, hipMemsetAsync(c->offs.p, 0, sizeof(int64_t), c->stream));
    ISLECHK(k_th_emit(c, c->a_doc_offset));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->res.B_replaced(true);
    if (docs_kept) *docs_kept = Db;
    if (nnz_kept) *nnz_kept = bnnz;
    return 0;
  }
};

extern "C" int isle_hip_threshold(isle_ctx* c, uint64_t num_topics, double sample_rate, uint64_t sample_seed, uint64_t* docs_kept,
                                  uint64_t* nnz_kept, uint64_t* entries_above, float* avg_out) {
  if (!c) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  if (!c->res.a_ready) return isle_fail(c, ISLE_E_ARG, "threshold: no count matrix uploaded");
  if (num_topics == 0) return isle_fail(c, ISLE_E_ARG, "threshold: num_topics == 0");
  Th th(c, num_topics, sample_rate, sample_seed);
  ISLECHK(th.stats(avg_out));
  ISLECHK(th.round_and_histogram());
  ISLECHK(th.zetas());
  ISLECHK(th.count_survivors(entries_above));
  ISLECHK(th.sample());
  ISLECHK(th.place_shard());
  return th.emit(docs_kept, nnz_kept);
}

extern "C" int isle_hip_counts_shape(isle_ctx* c, uint64_t* V, uint64_t* D, uint64_t* nnz, uint64_t* doc_offset, uint64_t* docs_global) {
  if (!c) return ISLE_E_ARG;
  if (!c->res.a_ready) return isle_fail(c, ISLE_E_ARG, "counts_shape: no count matrix");
  if (V) *V = c->a_V;
  if (D) *D = c->a_D;
  if (nnz) *nnz = c->a_nnz;
  if (doc_offset) *doc_offset = c->a_doc_offset;
  if (docs_global) *docs_global = c->a_D_global;
  return 0;
}

extern "C" int isle_hip_shape(isle_ctx* c, uint64_t* V, uint64_t* D, uint64_t* nnz, uint64_t* doc_offset, uint64_t* docs_global) {
  if (!c) return ISLE_E_ARG;
  if (V) *V = c->V;
  if (D) *D = c->D;
  if (nnz) *nnz = c->nnz;
  if (doc_offset) *doc_offset = c->doc_offset;
  if (docs_global) *docs_global = c->D_global;
  return 0;
}

extern "C" int isle_hip_get_B(isle_ctx* c, float* vals, uint32_t* rows, int64_t* offs, uint64_t* original_cols, float* zetas) {
  if (!c) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  if (c->V == 0) return isle_fail(c, ISLE_E_ARG, "get_B: no matrix");
  if ((original_cols || zetas) && !c->res.b_from_threshold)
    return isle_fail(c, ISLE_E_ARG, "get_B: original_cols / zetas exist only after isle_hip_threshold");
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (vals && c->nnz) HIPCHK(c, hipMemcpy(vals, c->vals.p, c->nnz * sizeof(float), hipMemcpyDeviceToHost));
  if (rows && c->nnz) HIPCHK(c, hipMemcpy(rows, c->rows.p, c->nnz * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (offs) HIPCHK(c, hipMemcpy(offs, c->offs.p, (c->D + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
  if (original_cols && c->D) HIPCHK(c, hipMemcpy(original_cols, c->original_cols.p, c->D * sizeof(uint64_t), hipMemcpyDeviceToHost));
  if (zetas) HIPCHK(c, hipMemcpy(zetas, c->zetas.p, c->V * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

// ------------------------------------------------------------------------------------------
// downstream stage: catchwords, topic model, edge topics
// ------------------------------------------------------------------------------------------
// the calls that are collective over document shards (catchwords, topic model) ...
static int post_prepare_sharded(isle_ctx* c, const char* who) {
  if (!c->res.a_ready) return isle_fail(c, ISLE_E_ARG, "%s: no count matrix uploaded (isle_hip_upload_counts_u32)", who);
  return 0;
}
// ... and the ones that read A on one rank only
static int post_prepare(isle_ctx* c, const char* who) {
  ISLECHK(post_prepare_sharded(c, who));
  if (c->world > 1) return isle_fail(c, ISLE_E_ARG, "%s: single-rank only", who);
  return 0;
}
// a reader of a model: with several ranks the catch model is replicated, a host model is the caller's and a loaded model is what each rank
// loaded for itself; each rank reads for itself.  Nothing builds the average model there.
static int model_reader_ok(isle_ctx* c, int which, const char* who) {
  if (c->world > 1 && which != ISLE_MODEL_CATCH && which != ISLE_MODEL_HOST && which != ISLE_MODEL_LOADED)
    return isle_fail(c, ISLE_E_ARG, "%s: single-rank only", who);
  return 0;
}

// a_nv = avg_doc_sz * (count / doc_sum) over A (src/sparseMatrix.cpp:136-167), the values the catchword stage and the top-five
// diagnostic read; avg_doc_sz from the thresholding when it ran, else computed here by the same rule (:92-99), over all ranks
static int ensure_avg_doc_sz(isle_ctx* c) {
  if (!c->res.a_avg_valid) {  // B came from the host: the corpus statistics were never computed here
    HIPCHK(c, c->a_scan.reserve(isle_scan_scratch(c->a_D) + 4));
    ISLECHK(k_th_stats(c, (uint64_t*)c->a_scan.p));
    ISLECHK(allreduce_sum<uint64_t>(c, (uint64_t*)c->a_scan.p, 2));
    uint64_t st[2];
    HIPCHK(c, hipMemcpyAsync(st, c->a_scan.p, sizeof(st), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->a_avg = corpus_avg(st[0], st[1]);
    c->res.corpus_average_known();
  }
  return 0;
}
static int post_normalize_A(isle_ctx* c) {
  ISLECHK(ensure_avg_doc_sz(c));
  return k_post_normalize(c, c->a_avg);
}

// The two order statistics of the stage with several ranks (route_post_select == POST_SELECT_HISTOGRAM): the device steps of post.hip and the
// collectives between them.  Every count that shapes a collective comes from all-reduced data; the slot count still goes through agree_i32,
// so that a rank that disagrees returns ISLE_E_COMM instead of issuing another sequence of collectives.
struct PostShard {
  isle_ctx* c;
  const uint32_t k;

  // four passes of eight bits over the slots' values, the slots in chunks of SELECT_CHUNK_SLOTS (stage_host.h); out[seg_id] = the value
  int select(uint64_t nslots, float* out, const char* what) {
    ISLECHK(agree_i32(c, (int)nslots, what));
    const uint64_t nchunks = select_chunks(nslots, SELECT_CHUNK_SLOTS);
    for (int shift = 24; shift >= 0; shift -= 8)
      for (uint64_t i = 0; i < nchunks; ++i) {
        const SlotChunk ch = select_chunk(nslots, SELECT_CHUNK_SLOTS, i);
        ISLECHK(k_post_select_hist(c, ch.first, ch.count, shift));
        ISLECHK(allreduce_sum<uint32_t>(c, c->p_sel_bins.p, (size_t)ch.count * 256));
        ISLECHK(k_post_select_step(c, ch.first, ch.count, shift, out));
      }
    return 0;
  }

  // catchword thresholds (word-major V x k in p_thr) for rank r; sizes_dev: documents per topic over all ranks
  int catch_thresholds(uint32_t r, const int* sizes_dev) {
    const uint64_t np = c->a_V * k;
    ISLECHK(k_post_pair_counts(c, k));
    ISLECHK(allreduce_sum<uint32_t>(c, c->p_cnt_g.p, np));
    {  // the minima as a maximum of complements: the transport has sum and max only
      TimeScope ts(c, ISLE_T_COMM);
      ISLECHK(isle_allreduce(c, c->p_min.p, np, ISLE_DT_U32, true));
    }
    ISLECHK(k_post_min_restore(c, c->p_min.p, np));
    uint64_t nslots = 0;
    ISLECHK(k_post_number_slots(c, c->p_cnt_g.p, c->p_cnt.p, np, r, r, nullptr, c->p_slot.p, c->p_slot.p, &nslots));
    ISLECHK(k_post_scatter_segments(c, k, nslots));
    ISLECHK(select(nslots, c->p_thr.p, "the number of catchword segments"));
    return k_post_thr_final(c, k, r, sizes_dev);
  }

  // p_mthr: the rank-th largest document sum of a topic over all ranks, 0 where the topic has fewer
  int model_thresholds(uint32_t rank) {
    ISLECHK(k_post_topic_counts(c, k));
    ISLECHK(allreduce_sum<uint32_t>(c, c->p_tcnt_g.p, k));
    uint64_t nslots = 0;
    ISLECHK(k_post_number_slots(c, c->p_tcnt_g.p, c->p_tcnt.p, k, rank - 1, rank, c->p_toff.p, c->p_tcnt_g.p + k, nullptr, &nslots));
    return select(nslots, c->p_mthr.p, "the number of topics with a rank threshold");
  }
};

extern "C" int isle_hip_catchwords(isle_ctx* c, int num_topics, const uint32_t* assign, uint64_t r, double rho, float* thresholds,
                                   int32_t* catch_topic, uint64_t* num_catchwords) {
  if (!c) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  ISLECHK(post_prepare_sharded(c, "catchwords"));
  if (num_topics < 1) return isle_fail(c, ISLE_E_ARG, "catchwords: num_topics < 1");
  if (r < 1 || r > 0xfffffff0ull) return isle_fail(c, ISLE_E_ARG, "catchwords: rank r = %llu out of range (too few documents per topic?)",
                                                    (unsigned long long)r);
  const bool identity = !c->res.b_from_threshold;
  if (identity && c->D != c->a_D) return isle_fail(c, ISLE_E_ARG, "catchwords: B was uploaded separately and its columns do not match A's");
  if (assign) {
    for (uint64_t j = 0; j < c->D; ++j)
      if (assign[j] >= (uint32_t)num_topics) return isle_fail(c, ISLE_E_ARG, "catchwords: assign[%llu] out of range", (unsigned long long)j);
    HIPCHK(c, c->assign.reserve(c->D ? c->D : 1));
    if (c->D) HIPCHK(c, hipMemcpy(c->assign.p, assign, c->D * sizeof(uint32_t), hipMemcpyHostToDevice));
    c->res.partition_given();
  } else if (!c->res.assign_valid) {
    return isle_fail(c, ISLE_E_ARG, "catchwords: no partition resident (run isle_hip_lloyds_sparse or pass assign)");
  }
  ISLECHK(post_normalize_A(c));
  ISLECHK(k_post_cluster_of(c, c->assign.p, identity));
  HIPCHK(c, c->counts.reserve(num_topics));
  ISLECHK(k_count_sizes(c, c->assign.p, c->D, num_topics, c->counts.p));
  ISLECHK(allreduce_sum<int>(c, c->counts.p, (size_t)num_topics));
  if (route_post_select(c->world) == POST_SELECT_HISTOGRAM) {
    PostShard ps = {c, (uint32_t)num_topics};
    ISLECHK(ps.catch_thresholds((uint32_t)r, c->counts.p));
  } else {
    ISLECHK(k_post_catch_thresholds(c, (uint32_t)num_topics, (uint32_t)r, c->counts.p));
  }
  uint64_t nc = 0;
  ISLECHK(k_post_find_catchwords(c, (uint32_t)num_topics, rho, &nc));
  if (num_catchwords) *num_catchwords = nc;
  c->res.catchwords_done(num_topics);
  if (thresholds) {
    HIPCHK(c, c->p_segvals.reserve((size_t)c->a_V * num_topics));
    ISLECHK(k_post_thr_colmajor(c, (uint32_t)num_topics, c->p_segvals.p));
    HIPCHK(c, hipMemcpyAsync(thresholds, c->p_segvals.p, (size_t)c->a_V * num_topics * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  }
  if (catch_topic) HIPCHK(c, hipMemcpyAsync(catch_topic, c->p_catch.p, c->a_V * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int isle_hip_topic_model(isle_ctx* c, int num_topics, uint64_t rank_threshold, float* model, float* model_threshold, int32_t* top1,
                                    int32_t* top2, uint64_t* doc_topic_sums) {
  if (!c) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  ISLECHK(post_prepare_sharded(c, "topic_model"));
  if (!c->res.p_catch_ready || c->res.p_k != num_topics) return isle_fail(c, ISLE_E_ARG, "topic_model: run isle_hip_catchwords(num_topics = %d) first", num_topics);
  if (rank_threshold < 1 || rank_threshold > 0xfffffff0ull) return isle_fail(c, ISLE_E_ARG, "topic_model: rank_threshold out of range");  // :721
  uint64_t n = 0;
  ISLECHK(k_post_doc_topic_sums(c, (uint32_t)num_topics, &n));
  if (route_post_select(c->world) == POST_SELECT_HISTOGRAM) {
    PostShard ps = {c, (uint32_t)num_topics};
    ISLECHK(ps.model_thresholds((uint32_t)rank_threshold));
  } else {
    ISLECHK(k_post_model_thresholds(c, (uint32_t)num_topics, (uint32_t)rank_threshold));
  }
  ISLECHK(k_post_model_accumulate(c, (uint32_t)num_topics));  // this rank's documents ...
  ISLECHK(allreduce_sum<float>(c, c->p_model.p, (size_t)c->a_V * num_topics));  // ... all documents: V x k floats
  ISLECHK(k_post_model_normalize(c, (uint32_t)num_topics));
  c->res.topic_model_done();
  if (doc_topic_sums) *doc_topic_sums = n;
  if (model) HIPCHK(c, hipMemcpyAsync(model, c->p_model.p, (size_t)c->a_V * num_topics * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (model_threshold) HIPCHK(c, hipMemcpyAsync(model_threshold, c->p_mthr.p, num_topics * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (top1 && c->a_D) HIPCHK(c, hipMemcpyAsync(top1, c->p_top1.p, c->a_D * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  if (top2 && c->a_D) HIPCHK(c, hipMemcpyAsync(top2, c->p_top2.p, c->a_D * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int isle_hip_get_doc_topic_sums(isle_ctx* c, int64_t* doc_offsets, uint32_t* topic, float* val) {
  if (!c) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  if (!c->res.p_model_ready) return isle_fail(c, ISLE_E_ARG, "get_doc_topic_sums: run isle_hip_topic_model first");
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (doc_offsets) HIPCHK(c, hipMemcpy(doc_offsets, c->p_dts_off.p, (c->a_D + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
  if (topic && c->p_dts_n) HIPCHK(c, hipMemcpy(topic, c->p_dts_topic.p, c->p_dts_n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (val && c->p_dts_n) HIPCHK(c, hipMemcpy(val, c->p_dts_val.p, c->p_dts_n * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

static int check_topic_pairs(isle_ctx* c, const int64_t* pairs, int n, const char* who) {
  for (int e = 0; e < 2 * n; ++e)
    if (pairs[e] < 0 || pairs[e] >= c->res.p_k) return isle_fail(c, ISLE_E_ARG, "%s: topic id %lld out of range", who, (long long)pairs[e]);
  return 0;
}

extern "C" int isle_hip_edge_topics(isle_ctx* c, const int64_t* pairs, int n, float primary_ratio, float* edge) {
  if (!c) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  if (!c->res.p_model_ready) return isle_fail(c, ISLE_E_ARG, "edge_topics: run isle_hip_topic_model first");
  if (n < 0 || (n && (!pairs || !edge))) return isle_fail(c, ISLE_E_ARG, "edge_topics: bad arguments");
  if (n == 0) return 0;
  ISLECHK(check_topic_pairs(c, pairs, n, "edge_topics"));
  DevBuf<int64_t> pd;
  DevBuf<float> ed;
  StreamDrain drain(c);
  HIPCHK(c, pd.reserve(2 * (size_t)n));
  HIPCHK(c, ed.reserve((size_t)c->a_V * n));
  HIPCHK(c, hipMemcpy(pd.p, pairs, 2 * (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice));
  ISLECHK(k_post_edge(c, pd.p, n, primary_ratio, (float)(1.0 - (double)primary_ratio), ed.p));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(edge, ed.p, (size_t)c->a_V * n * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

// construct_edge_topics_v2's pair selection (src/trainer.cpp:1120-1145) on the device (edge_select.hip), over the resident top-two topics
// of the last topic model or over the caller's arrays
extern "C" int isle_hip_select_edge_pairs(isle_ctx* c, const int32_t* top1, const int32_t* top2, uint64_t n_docs, int num_topics,
                                          int64_t max_edge_topics, uint64_t min_docs, int64_t* pairs, uint64_t cap, uint64_t* n_selected,
                                          uint64_t* n_candidates, uint64_t* threshold) {
  if (!c) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  if (n_selected) *n_selected = 0;
  if (n_candidates) *n_candidates = 0;
  if (threshold) *threshold = 0;
  if (num_topics < 1) return isle_fail(c, ISLE_E_ARG, "select_edge_pairs: num_topics < 1");
  if (num_topics > ISLE_EDGE_TABLE_MAX_TOPICS)
    return isle_fail(c, ISLE_E_ARG, "select_edge_pairs: num_topics = %d, the pairs are counted in a table of num_topics^2 counters and %d is its limit",
                     num_topics, ISLE_EDGE_TABLE_MAX_TOPICS);
  if (max_edge_topics < 0) return isle_fail(c, ISLE_E_ARG, "select_edge_pairs: max_edge_topics < 0");
  if ((top1 == nullptr) != (top2 == nullptr)) return isle_fail(c, ISLE_E_ARG, "select_edge_pairs: one of top1 / top2 is null (both, or neither for the resident pairs)");
  if (n_docs > 0xffffffffull) return isle_fail(c, ISLE_E_ARG, "select_edge_pairs: %llu documents (the counters hold 32 bits)", (unsigned long long)n_docs);
  if (cap && !pairs) return isle_fail(c, ISLE_E_ARG, "select_edge_pairs: null pairs");
  const bool resident = top1 == nullptr;
  const int32_t *t1 = nullptr, *t2 = nullptr;
  DevBuf<int32_t> u1, u2;
  StreamDrain drain(c);
  if (resident) {
    if (!c->res.p_model_ready) return isle_fail(c, ISLE_E_ARG, "select_edge_pairs: no resident top topics (run isle_hip_topic_model, or pass top1 / top2)");
    if (n_docs != c->a_D || num_topics != c->res.p_k)
      return isle_fail(c, ISLE_E_ARG, "select_edge_pairs: n_docs x num_topics = %llu x %d, the resident topic model has %llu x %d", (unsigned long long)n_docs,
                       num_topics, (unsigned long long)c->a_D, c->res.p_k);
    t1 = c->p_top1.p;
    t2 = c->p_top2.p;
  } else {
    HIPCHK(c, u1.reserve(n_docs ? n_docs : 1));
    HIPCHK(c, u2.reserve(n_docs ? n_docs : 1));
    if (n_docs) {
      HIPCHK(c, hipMemcpyAsync(u1.p, top1, n_docs * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
      HIPCHK(c, hipMemcpyAsync(u2.p, top2, n_docs * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    }
    t1 = u1.p;
    t2 = u2.p;
  }
  uint64_t nsel = 0, ncand = 0, thr = 0, bad = ~0ull;
  ISLECHK(k_edge_select(c, t1, t2, n_docs, (uint32_t)num_topics, (uint64_t)max_edge_topics, min_docs, pairs, cap, &nsel, &ncand, &thr, &bad));
  if (bad != ~0ull)
    return isle_fail(c, ISLE_E_ARG, "select_edge_pairs: document %llu: a topic id outside -1 .. %d", (unsigned long long)bad, num_topics - 1);
  if (n_selected) *n_selected = nsel;
  if (n_candidates) *n_candidates = ncand;
  if (nsel > cap)
    return isle_fail(c, ISLE_E_ARG, "select_edge_pairs: %llu pairs selected, room for %llu", (unsigned long long)nsel, (unsigned long long)cap);
  if (threshold) *threshold = thr;
  return 0;
}

// UMass coherence (src/sparseMatrix.cpp:841-1016): the distinct words and word pairs are prepared here, their document frequencies are
// counted on the device in one pass over A per counter tile (coherence.hip), the sums are formed here in double.
extern "C" int isle_hip_topic_coherence(isle_ctx* c, int num_topics, int M, const uint32_t* top_words, double eps, double* coherence,
                                        uint64_t* doc_freq, uint64_t* co_doc_freq) {
  if (!c) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  ISLECHK(post_prepare(c, "topic_coherence"));
  if (num_topics < 1) return isle_fail(c, ISLE_E_ARG, "topic_coherence: num_topics < 1");
  if (M < 1 || M > 32) return isle_fail(c, ISLE_E_ARG, "topic_coherence: M = %d outside 1 .. 32", M);
  if (!top_words || !coherence) return isle_fail(c, ISLE_E_ARG, "topic_coherence: null top_words or coherence");
  const CoherencePlan plan(top_words, (size_t)num_topics, (size_t)M, c->a_V);
  if (!plan.refused.empty()) return isle_fail(c, ISLE_E_ARG, "%s", plan.refused.c_str());
  std::vector<uint32_t> cnt;
  ISLECHK(k_coherence_counts(c, plan.U, plan.part_off, plan.part_hi, cnt, nullptr));
  coherence_sums(plan, cnt.data(), eps, coherence, doc_freq, co_doc_freq);
  return 0;
}

// The cluster-average model (src/trainer.cpp:705-745) and what reads a model: top words (src/denseMatrix.cpp:92-107) and diversity
// (src/trainer.cpp:750-774); avg_model.hip
extern "C" int isle_hip_avg_topic_model(isle_ctx* c, int num_topics, float* model) {
  if (!c) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  ISLECHK(post_prepare(c, "avg_topic_model"));
  if (num_topics < 1 || !c->res.p_catch_ready || c->res.p_k != num_topics)
    return isle_fail(c, ISLE_E_ARG, "avg_topic_model: run isle_hip_catchwords(num_topics = %d) first", num_topics);
  c->res.avg_model_begins();
  ISLECHK(k_avg_model(c, (uint32_t)num_topics));
  c->res.avg_model_done();
  if (model) HIPCHK(c, hipMemcpyAsync(model, c->p_avg_model.p, (size_t)c->a_V * num_topics * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

// the resident model `which` names and its size, or null with the reason in the context
static const float* resident_model(isle_ctx* c, int which, const char* who, uint64_t* V, int* cols) {
  *V = c->a_V;
  *cols = c->res.p_k;
  if (which == ISLE_MODEL_CATCH) {
    if (c->res.p_model_ready) return c->p_model.p;
    isle_fail(c, ISLE_E_ARG, "%s: no catch model (run isle_hip_topic_model)", who);
  } else if (which == ISLE_MODEL_AVG) {
    if (c->res.p_avg_ready) return c->p_avg_model.p;
    isle_fail(c, ISLE_E_ARG, "%s: no average model (run isle_hip_avg_topic_model)", who);
  } else if (which == ISLE_MODEL_LOADED) {
    *V = c->ml_V;
    *cols = c->ml_cols;
    if (c->res.ml_ready) return c->ml_model.p;
    isle_fail(c, ISLE_E_ARG, "%s: no loaded model (run isle_hip_load_model_text)", who);
  } else {
    isle_fail(c, ISLE_E_ARG, "%s: unknown model %d", who, which);
  }
  return nullptr;
}

// the model a call reads: the caller's (uploaded into `up`, which the caller keeps alive until its stream work is done) or a resident one
static int model_source(isle_ctx* c, int which, const float* model_host, uint64_t vocab, int ncols, const char* who, DevBuf<float>* up, const float** dev) {
  if (which == ISLE_MODEL_HOST) {
    if (!model_host && ncols) return isle_fail(c, ISLE_E_ARG, "%s: null model_host", who);
    if (ncols) {
      HIPCHK(c, up->reserve(vocab * (size_t)ncols));
      HIPCHK(c, hipMemcpyAsync(up->p, model_host, vocab * (size_t)ncols * sizeof(float), hipMemcpyHostToDevice, c->stream));
    }
    *dev = up->p;
    return 0;
  }
  uint64_t rV = 0;
  int rcols = 0;
  *dev = resident_model(c, which, who, &rV, &rcols);
  if (!*dev) return ISLE_E_ARG;
  if (vocab != rV || ncols != rcols)
    return isle_fail(c, ISLE_E_ARG, "%s: vocab x ncols = %llu x %d, the resident model is %llu x %d", who, (unsigned long long)vocab, ncols,
                     (unsigned long long)rV, rcols);
  return 0;
}

extern "C" int isle_hip_model_top_words(isle_ctx* c, int which, const float* model_host, uint64_t vocab, int ncols, int n, uint32_t* ids,
                                        float* weights) {
  if (!c) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  ISLECHK(model_reader_ok(c, which, "model_top_words"));
  if (ncols < 0 || vocab == 0 || vocab > 0xfffffff0ull) return isle_fail(c, ISLE_E_ARG, "model_top_words: vocab or ncols out of range");
  if (n < 1 || n > 32 || (uint64_t)n > vocab) return isle_fail(c, ISLE_E_ARG, "model_top_words: n = %d outside 1 .. min(vocab, 32)", n);
  if (!ids) return isle_fail(c, ISLE_E_ARG, "model_top_words: null ids");
  const float* dev = nullptr;
  DevBuf<float> up, w_d;
  DevBuf<uint32_t> id_d;
  StreamDrain drain(c);
  ISLECHK(model_source(c, which, model_host, vocab, ncols, "model_top_words", &up, &dev));
  if (ncols == 0) return 0;
  const size_t m = (size_t)ncols * n;
  HIPCHK(c, id_d.reserve(m));
  HIPCHK(c, w_d.reserve(m));
  ISLECHK(k_model_top_words(c, dev, vocab, (uint32_t)ncols, n, id_d.p, w_d.p));
  HIPCHK(c, hipMemcpyAsync(ids, id_d.p, m * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  if (weights) HIPCHK(c, hipMemcpyAsync(weights, w_d.p, m * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

// ---- two models compared: L1 distances and the greedy matching (model_compare.hip; the rule: match_host.h)
extern "C" int isle_hip_model_dist_slices(isle_ctx* c, int slices) {
  if (!c) return ISLE_E_ARG;
  const std::string why = mc_check_slices(slices);
  if (!why.empty()) return isle_fail(c, ISLE_E_ARG, "%s", why.c_str());
  c->model_dist_slices = slices;
  return 0;
}

// what match_host.h's checks ask about a side, from the ledger alone
static McSide mc_side(const isle_ctx* c, int which, const float* host, int cols) {
  McSide m = {which, host != nullptr, cols, false, c->a_V, c->res.p_k};
  if (which == ISLE_MODEL_CATCH) m.resident = c->res.p_model_ready;
  else if (which == ISLE_MODEL_AVG) m.resident = c->res.p_avg_ready;
  else if (which == ISLE_MODEL_LOADED) m.resident = c->res.ml_ready, m.res_vocab = c->ml_V, m.res_cols = c->ml_cols;
  return m;
}

// the matcher on a device matrix and the fetches of what was asked for (mean_dist: the fetched distances summed in ascending i on the host)
static int mc_match_and_fetch(isle_ctx* c, const double* dist_dev, int na, int nb, int32_t* match_a, int32_t* match_b, double* match_dist, uint64_t* n_matched,
                              double* mean_dist, uint32_t* rounds) {
  DevBuf<int32_t> m_d;
  DevBuf<double> md_d;
  StreamDrain drain(c);
  HIPCHK(c, m_d.reserve((size_t)na + nb));
  HIPCHK(c, md_d.reserve((size_t)na));
  uint64_t n = 0;
  uint32_t r = 0;
  ISLECHK(k_mc_match(c, dist_dev, na, nb, m_d.p, m_d.p + na, md_d.p, &n, &r));
  std::vector<int32_t> ma;
  std::vector<double> md;
  if (mean_dist) {
    ma.resize((size_t)na);
    md.resize((size_t)na);
    HIPCHK(c, hipMemcpyAsync(ma.data(), m_d.p, (size_t)na * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(md.data(), md_d.p, (size_t)na * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  }
  if (match_a) HIPCHK(c, hipMemcpyAsync(match_a, m_d.p, (size_t)na * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  if (match_b) HIPCHK(c, hipMemcpyAsync(match_b, m_d.p + na, (size_t)nb * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  if (match_dist) HIPCHK(c, hipMemcpyAsync(match_dist, md_d.p, (size_t)na * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (mean_dist) {
    uint64_t counted = 0;
    *mean_dist = mc_mean(ma, md, &counted);
    if (counted != n) return isle_fail(c, ISLE_E_HIP, "match_topics: %llu rows are matched where the rounds counted %llu", (unsigned long long)counted, (unsigned long long)n);
  }
  if (n_matched) *n_matched = n;
  if (rounds) *rounds = r;
  return 0;
}

extern "C" int isle_hip_compare_models(isle_ctx* c, int which_a, const float* a_host, int cols_a, int which_b, const float* b_host, int cols_b, uint64_t vocab,
                                       double* dist, int32_t* match_a, int32_t* match_b, double* match_dist, uint64_t* n_matched, double* mean_dist,
                                       uint32_t* rounds) {
  if (!c) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  ISLECHK(model_reader_ok(c, which_a, "compare_models"));
  ISLECHK(model_reader_ok(c, which_b, "compare_models"));
  const std::string why = mc_check_compare(mc_side(c, which_a, a_host, cols_a), mc_side(c, which_b, b_host, cols_b), vocab);
  if (!why.empty()) return isle_fail(c, ISLE_E_ARG, "%s", why.c_str());
  const float *a_dev = nullptr, *b_dev = nullptr;
  DevBuf<float> up_a, up_b;
  DevBuf<double> dist_d;
  StreamDrain drain(c);  // both uploads live until the stream is drained
  ISLECHK(model_source(c, which_a, a_host, vocab, cols_a, "compare_models", &up_a, &a_dev));
  ISLECHK(model_source(c, which_b, b_host, vocab, cols_b, "compare_models", &up_b, &b_dev));
  HIPCHK(c, dist_d.reserve((size_t)cols_a * cols_b));
  ISLECHK(k_mc_dist(c, a_dev, cols_a, b_dev, cols_b, vocab, route_model_dist_slices(vocab, cols_a, cols_b, c->num_cus, c->model_dist_slices), dist_d.p));
  if (dist) HIPCHK(c, hipMemcpyAsync(dist, dist_d.p, (size_t)cols_a * cols_b * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (match_a || match_b || match_dist || n_matched || mean_dist) {
    ISLECHK(mc_match_and_fetch(c, dist_d.p, cols_a, cols_b, match_a, match_b, match_dist, n_matched, mean_dist, rounds));
  } else if (rounds) {
    *rounds = 0;
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int isle_hip_match_topics(isle_ctx* c, const double* dist_host, int na, int nb, int32_t* match_a, int32_t* match_b, double* match_dist,
                                     uint64_t* n_matched, double* mean_dist, uint32_t* rounds) {
  if (!c) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  const std::string why = mc_check_match(dist_host != nullptr, na, nb);
  if (!why.empty()) return isle_fail(c, ISLE_E_ARG, "%s", why.c_str());
  DevBuf<double> dist_d;
  StreamDrain drain(c);
  HIPCHK(c, dist_d.reserve((size_t)na * nb));
  HIPCHK(c, hipMemcpyAsync(dist_d.p, dist_host, (size_t)na * nb * sizeof(double), hipMemcpyHostToDevice, c->stream));
  return mc_match_and_fetch(c, dist_d.p, na, nb, match_a, match_b, match_dist, n_matched, mean_dist, rounds);
}

// ... of the edge topics a * M[:, p] + b * M[:, s] of a model, formed from its two columns while they are read (tw_select_k's edge source)
extern "C" int isle_hip_edge_top_words(isle_ctx* c, int which, const float* model_host, uint64_t vocab, int ncols, const int64_t* pairs, int n_edge,
                                       float primary_ratio, int n, uint32_t* ids, float* weights) {
  if (!c) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  ISLECHK(model_reader_ok(c, which, "edge_top_words"));
  if (ncols < 0 || vocab == 0 || vocab > 0xfffffff0ull) return isle_fail(c, ISLE_E_ARG, "edge_top_words: vocab or ncols out of range");
  if (n < 1 || n > 32 || (uint64_t)n > vocab) return isle_fail(c, ISLE_E_ARG, "edge_top_words: n = %d outside 1 .. min(vocab, 32)", n);
  if (n_edge < 0 || (n_edge && (!pairs || !ids))) return isle_fail(c, ISLE_E_ARG, "edge_top_words: bad arguments");
  for (int e = 0; e < 2 * n_edge; ++e)
    if (pairs[e] < 0 || pairs[e] >= ncols)
      return isle_fail(c, ISLE_E_ARG, "edge_top_words: edge topic %d: topic id %lld outside 0 .. %d", e / 2, (long long)pairs[e], ncols - 1);
  const float* dev = nullptr;
  DevBuf<float> up, w_d;
  DevBuf<int64_t> pd;
  DevBuf<uint32_t> id_d;
  StreamDrain drain(c);
  ISLECHK(model_source(c, which, model_host, vocab, ncols, "edge_top_words", &up, &dev));
  if (n_edge == 0) return 0;
  const size_t m = (size_t)n_edge * n;
  HIPCHK(c, pd.reserve(2 * (size_t)n_edge));
  HIPCHK(c, id_d.reserve(m));
  HIPCHK(c, w_d.reserve(m));
  HIPCHK(c, hipMemcpyAsync(pd.p, pairs, 2 * (size_t)n_edge * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
  ISLECHK(k_edge_top_words(c, dev, vocab, pd.p, (uint32_t)n_edge, primary_ratio, (float)(1.0 - (double)primary_ratio), n, id_d.p, w_d.p));
  HIPCHK(c, hipMemcpyAsync(ids, id_d.p, m * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  if (weights) HIPCHK(c, hipMemcpyAsync(weights, w_d.p, m * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

// The reference's model files formatted on the device (model_text.hip): MMappedOutput, include/utils.h:383-478, under
// DenseMatrix::write_to_file_as_sparse / write_to_file, src/denseMatrix.cpp:124-186
extern "C" int isle_hip_model_text(isle_ctx* c, int which, const float* model_host, uint64_t vocab, int ncols, int format, isle_text_sink_fn sink,
                                   void* user, uint64_t* nbytes, uint64_t* nentries) {
  if (!c) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  if (nbytes) *nbytes = 0;
  if (nentries) *nentries = 0;
  ISLECHK(model_reader_ok(c, which, "model_text"));
  if (format != ISLE_TEXT_SPARSE && format != ISLE_TEXT_DENSE) return isle_fail(c, ISLE_E_ARG, "model_text: unknown format %d", format);
  if (ncols < 0 || vocab == 0 || vocab > 0xfffffff0ull) return isle_fail(c, ISLE_E_ARG, "model_text: vocab or ncols out of range");
  const float* dev = nullptr;
  DevBuf<float> up;
  StreamDrain drain(c);
  ISLECHK(model_source(c, which, model_host, vocab, ncols, "model_text", &up, &dev));
  return k_model_text(c, dev, vocab, (uint64_t)ncols, nullptr, 0.f, 0.f, format, sink, user, nbytes, nentries);
}

// A model file read on the device (model_load.hip) into a resident model of its own: parsed into scratch, swapped in on success
extern "C" int isle_hip_load_model_text(isle_ctx* c, const char* text, uint64_t nbytes, uint64_t vocab, int ncols, int format, unsigned base,
                                        uint64_t* nentries) {
  if (!c) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  if (nentries) *nentries = 0;
  if (format != ISLE_TEXT_SPARSE && format != ISLE_TEXT_DENSE) return isle_fail(c, ISLE_E_ARG, "load_model_text: unknown format %d", format);
  if (base > 1) return isle_fail(c, ISLE_E_ARG, "load_model_text: base = %u (0 or 1)", base);
  if (vocab == 0 || vocab > 0xfffffff0ull || ncols < 1) return isle_fail(c, ISLE_E_ARG, "load_model_text: vocab or ncols out of range");
  if (nbytes && !text) return isle_fail(c, ISLE_E_ARG, "load_model_text: null text");
  if (format == ISLE_TEXT_SPARSE && nbytes > 0x3fffffff0ull)
    return isle_fail(c, ISLE_E_ARG, "load_model_text: a sparse text of %llu bytes (the line order is kept in 32 bits: at most 2^34 - 16)", (unsigned long long)nbytes);
  DevBuf<unsigned char> td;
  DevBuf<float> next;
  StreamDrain drain(c);
  HIPCHK(c, td.reserve(nbytes + 16));
  HIPCHK(c, next.reserve(vocab * (size_t)ncols));
  if (nbytes) HIPCHK(c, hipMemcpy(td.p, text, nbytes, hipMemcpyHostToDevice));
  uint64_t n = 0, key = ~0ull;
  ISLECHK(k_load_model_text(c, td.p, nbytes, vocab, (uint32_t)ncols, format, base, next.p, &n, &key));
  if (key != ~0ull) {
    static const char* what[] = {"", "bad character", "too many fields", "too few fields", "id zero or out of range", "token too long",
                                 "wrong token count", "wrong line count"};
    return isle_fail(c, ISLE_E_ARG, "load_model_text: line %llu: %s", (unsigned long long)line_of_byte(text, nbytes, key >> 3), what[key & 7]);
  }
  std::swap(c->ml_model.p, next.p);  // the previous model leaves with `next`
  std::swap(c->ml_model.cap, next.cap);
  c->ml_V = vocab;
  c->ml_cols = ncols;
  c->res.model_loaded();
  if (nentries) *nentries = n;
  return 0;
}

extern "C" int isle_hip_get_loaded_model(isle_ctx* c, float* model, uint64_t* vocab, int* ncols) {
  if (!c) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  if (!c->res.ml_ready) return isle_fail(c, ISLE_E_ARG, "get_loaded_model: no loaded model (run isle_hip_load_model_text)");
  if (vocab) *vocab = c->ml_V;
  if (ncols) *ncols = c->ml_cols;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (model) HIPCHK(c, hipMemcpy(model, c->ml_model.p, c->ml_V * (size_t)c->ml_cols * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int isle_hip_edge_topics_text(isle_ctx* c, const int64_t* pairs, int n, float primary_ratio, int format, isle_text_sink_fn sink, void* user,
                                         uint64_t* nbytes, uint64_t* nentries) {
  if (!c) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  if (nbytes) *nbytes = 0;
  if (nentries) *nentries = 0;
  if (!c->res.p_model_ready) return isle_fail(c, ISLE_E_ARG, "edge_topics_text: run isle_hip_topic_model first");
  if (format != ISLE_TEXT_SPARSE && format != ISLE_TEXT_DENSE) return isle_fail(c, ISLE_E_ARG, "edge_topics_text: unknown format %d", format);
  if (n < 0 || (n && !pairs)) return isle_fail(c, ISLE_E_ARG, "edge_topics_text: bad arguments");
  if (n == 0) return 0;
  ISLECHK(check_topic_pairs(c, pairs, n, "edge_topics_text"));
  DevBuf<int64_t> pd;
  StreamDrain drain(c);
  HIPCHK(c, pd.reserve(2 * (size_t)n));
  HIPCHK(c, hipMemcpy(pd.p, pairs, 2 * (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice));
  return k_model_text(c, c->p_model.p, c->a_V, (uint64_t)n, pd.p, primary_ratio, (float)(1.0 - (double)primary_ratio), format, sink, user, nbytes,
                      nentries);
}

extern "C" int isle_hip_topic_diversity(isle_ctx* c, int which, int num_topics, double* dist, double* avg) {
  if (!c) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  ISLECHK(model_reader_ok(c, which, "topic_diversity"));
  uint64_t V = 0;
  int cols = 0;
  const float* dev = resident_model(c, which, "topic_diversity", &V, &cols);
  if (!dev) return ISLE_E_ARG;
  if (num_topics != cols) return isle_fail(c, ISLE_E_ARG, "topic_diversity: num_topics = %d, the resident model has %d", num_topics, cols);
  const uint32_t k = (uint32_t)num_topics;
  DevBuf<double> dd, ab;
  DevBuf<int32_t> fin;
  StreamDrain drain(c);
  HIPCHK(c, dd.reserve(k));
  HIPCHK(c, ab.reserve(V));
  HIPCHK(c, fin.reserve(k));
  uint32_t kp = 0;
  ISLECHK(k_topic_diversity(c, dev, V, k, dd.p, ab.p, fin.p, &kp));
  std::vector<double> h(k);
  HIPCHK(c, hipMemcpyAsync(h.data(), dd.p, k * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (dist) std::memcpy(dist, h.data(), k * sizeof(double));
  if (avg) *avg = diversity_average(h.data(), k, kp);
  return 0;
}


// Corpus diagnostics of the trainer (src/trainer.cpp:373-403) on the count matrix A, right after ingest or upload (corpus_stats.hip).
extern "C" int isle_hip_log_combinatorial(isle_ctx* c, float* out, uint64_t* max_words) {
  if (!c) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  ISLECHK(post_prepare(c, "log_combinatorial"));
  if (!out) return isle_fail(c, ISLE_E_ARG, "log_combinatorial: null out");
  return k_log_combinatorial(c, out, max_words);
}

extern "C" int isle_hip_top_five_count_rule(const uint64_t* run_lengths, uint64_t n_runs, int32_t m, uint64_t* out) {
  if (!out || (n_runs && !run_lengths) || m < 2) return ISLE_E_ARG;
  for (uint64_t r = 0; r < n_runs; ++r)
    if (run_lengths[r] == 0) return ISLE_E_ARG;
  *out = top_five_count(run_lengths, n_runs, m);
  return 0;
}

extern "C" int isle_hip_distinct_top_five(isle_ctx* c, int n_m, const int32_t* m, uint64_t* num_distinct, uint64_t* num_quintuples, float* quintuples,
                                          uint64_t* run_lengths, uint64_t* num_runs) {
  if (!c) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  ISLECHK(post_prepare(c, "distinct_top_five"));
  if (n_m < 0 || (n_m && (!m || !num_distinct))) return isle_fail(c, ISLE_E_ARG, "distinct_top_five: n_m < 0, or null m / num_distinct");
  for (int i = 0; i < n_m; ++i)
    if (m[i] < 2) return isle_fail(c, ISLE_E_ARG, "distinct_top_five: m[%d] = %d < 2 (the reference asserts min_distinct >= 2)", i, (int)m[i]);
  ISLECHK(post_normalize_A(c));
  uint64_t n = 0;
  std::vector<uint64_t> runs;
  ISLECHK(k_top_five_runs(c, &n, runs, quintuples));
  for (int i = 0; i < n_m; ++i) (void)isle_hip_top_five_count_rule(runs.data(), runs.size(), m[i], &num_distinct[i]);
  if (num_quintuples) *num_quintuples = n;
  if (num_runs) *num_runs = runs.size();
  if (run_lengths && !runs.empty()) std::memcpy(run_lengths, runs.data(), runs.size() * sizeof(uint64_t));
  return 0;
}

extern "C" int isle_hip_infer(isle_ctx* c, uint64_t V, int k, const float* model_by_word, uint64_t D, uint64_t nnz, const float* counts,
                              const uint32_t* rows, const int64_t* offs, int iters, float Lf, float avg_doc_sz, float* weights,
                              int32_t* top_topic, float* top_weight, float* llh, uint64_t* nconverged) {
  if (!c || !model_by_word || !offs || (nnz && (!counts || !rows))) return ISLE_E_ARG;
  if (iters < 1 || !(Lf > 0.f)) return isle_fail(c, ISLE_E_ARG, "infer: iters = %d, Lf = %g", iters, (double)Lf);
  if (offs[0] != 0 || (uint64_t)offs[D] != nnz) return isle_fail(c, ISLE_E_ARG, "infer: offsets do not span the %llu entries", (unsigned long long)nnz);
  ISLECHK(isle_enter(c));
  return k_infer(c, V, k, model_by_word, D, nnz, counts, rows, offs, iters, Lf, avg_doc_sz, weights, top_topic, top_weight, llh, nconverged);
}


// Document-topic inference on the resident count matrix under a resident or uploaded model (infer_resident.hip).  Every argument is
// checked before any work: a refused call leaves the entries of the previous call as they were.
extern "C" int isle_hip_infer_resident(isle_ctx* c, int which, const float* model_host, uint64_t vocab, int ncols, uint64_t doc_begin,
                                       uint64_t doc_end, int iters, float Lf, float min_weight, uint64_t chunk_docs, int32_t* top_topic,
                                       float* top_weight, float* llh, uint64_t* nconverged, uint64_t* nentries) {
  if (!c) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  ISLECHK(post_prepare_sharded(c, "infer_resident"));
  ISLECHK(model_reader_ok(c, which, "infer_resident"));
  if (doc_begin > doc_end || doc_end > c->a_D)
    return isle_fail(c, ISLE_E_ARG, "infer_resident: documents [%llu, %llu) of %llu", (unsigned long long)doc_begin, (unsigned long long)doc_end,
                     (unsigned long long)c->a_D);
  if (iters < 1 || !(Lf > 0.f)) return isle_fail(c, ISLE_E_ARG, "infer_resident: iters = %d, Lf = %g", iters, (double)Lf);
  if (ncols < 1 || ncols > 1024) return isle_fail(c, ISLE_E_ARG, "infer: num_topics = %d not in [1, 1024]", ncols);
  if (vocab != c->a_V)
    return isle_fail(c, ISLE_E_ARG, "infer_resident: the model has %llu words, the count matrix %llu", (unsigned long long)vocab, (unsigned long long)c->a_V);
  const float* dev = nullptr;
  DevBuf<float> up;
  StreamDrain drain(c);
  ISLECHK(model_source(c, which, model_host, vocab, ncols, "infer_resident", &up, &dev));
  ISLECHK(ensure_avg_doc_sz(c));
  return k_infer_resident(c, dev, ncols, doc_begin, doc_end, iters, Lf, c->a_avg, min_weight, chunk_docs, top_topic, top_weight, llh, nconverged,
                          nentries);
}

extern "C" int isle_hip_get_infer_entries(isle_ctx* c, int64_t* doc_offsets, uint32_t* topic, float* weight) {
  if (!c) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  if (!c->res.inf_valid) return isle_fail(c, ISLE_E_ARG, "get_infer_entries: no entries (run isle_hip_infer_resident; a new count matrix voids them)");
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (doc_offsets) HIPCHK(c, hipMemcpy(doc_offsets, c->inf_off.p, (c->inf_docs + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
  if (topic && c->inf_n) HIPCHK(c, hipMemcpy(topic, c->inf_topic.p, c->inf_n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (weight && c->inf_n) HIPCHK(c, hipMemcpy(weight, c->inf_weight.p, c->inf_n * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

// The per-document topic files formatted on the device (infer_text.hip) from the resident result of the last isle_hip_infer_resident
extern "C" int isle_hip_infer_text(isle_ctx* c, int what, uint64_t row_begin, uint64_t row_end, uint64_t number_base, isle_text_sink_fn sink,
                                   void* user, uint64_t* nbytes, uint64_t* nlines) {
  if (!c) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  if (nbytes) *nbytes = 0;
  if (nlines) *nlines = 0;
  if (what != ISLE_DOCTEXT_ENTRIES && what != ISLE_DOCTEXT_TOP) return isle_fail(c, ISLE_E_ARG, "infer_text: unknown kind %d", what);
  if (!c->res.inf_valid) return isle_fail(c, ISLE_E_ARG, "infer_text: no resident result (run isle_hip_infer_resident; a new count matrix voids it)");
  if (row_begin > row_end || row_end > c->inf_docs)
    return isle_fail(c, ISLE_E_ARG, "infer_text: rows [%llu, %llu) of %llu", (unsigned long long)row_begin, (unsigned long long)row_end,
                     (unsigned long long)c->inf_docs);
  return k_infer_text(c, what, row_begin, row_end, number_base, sink, user, nbytes, nlines);
}

// DocTopicCatchwordSums.tsv over document shards (route_topic_sums == TOPIC_SUMS_GATHERED): the device steps of doc_report.hip and the three
// collectives between them (the counts, the keys, the documents).  Every rank takes every step up to its own slice, a rank without documents
// or without sums included; every count that shapes a collective comes from the gathered counts; no collective follows the first sink call.
static int topic_sums_gathered(isle_ctx* c, uint64_t doc_begin, uint64_t doc_end, isle_text_sink_fn sink, void* user, uint64_t* nbytes, uint64_t* nlines) {
  const size_t W = (size_t)c->world;
  uint64_t first = 0, n_own = 0;
  ISLECHK(k_dr_sums_range(c, doc_begin, doc_end, &first, &n_own));
  DevBuf<uint64_t> cnt_dev, gkey, key_a, key_b;
  DevBuf<uint32_t> gdoc, doc_a, doc_b;
  StreamDrain drain(c);
  std::vector<uint64_t> n_of(W);
  HIPCHK(c, cnt_dev.reserve(W + 1));
  ISLECHK(allgather_host<uint64_t>(c, &n_own, 1, cnt_dev.p, n_of.data()));
  uint64_t L = 0, nmax = 0;
  for (size_t q = 0; q < W; ++q) {
    if (n_of[q] >= (1ull << 32) || (L += n_of[q]) >= (1ull << 32))  // on every rank alike
      return isle_fail(c, ISLE_E_ARG, "doc_report_text(topic_sums): 2^32 sums or more over the ranks' ranges; the order's payload is 32 bits wide — write the ranges in parts");
    nmax = std::max(nmax, n_of[q]);
  }
  if (L == 0) return 0;
  HIPCHK(c, gkey.reserve(W * nmax));
  HIPCHK(c, gdoc.reserve(W * nmax));
  HIPCHK(c, key_a.reserve(L));
  HIPCHK(c, key_b.reserve(L));
  HIPCHK(c, doc_a.reserve(L));
  HIPCHK(c, doc_b.reserve(L));
  uint64_t* const my_key = gkey.p + (size_t)c->rank * nmax;
  uint32_t* const my_doc = gdoc.p + (size_t)c->rank * nmax;
  ISLECHK(k_dr_sums_keys(c, doc_begin, doc_end, first, n_own, nmax, my_key, my_doc));
  {
    TimeScope ts(c, ISLE_T_COMM);
    ISLECHK(isle_allgather(c, my_key, gkey.p, nmax, ISLE_DT_U64));
    ISLECHK(isle_allgather(c, my_doc, gdoc.p, nmax, ISLE_DT_U32));
  }
  uint64_t at = 0;
  for (size_t q = 0; q < W; ++q) {  // the blocks without their padding, in rank order: document order
    if (n_of[q]) {
      HIPCHK(c, hipMemcpyAsync(key_a.p + at, gkey.p + q * nmax, n_of[q] * sizeof(uint64_t), hipMemcpyDeviceToDevice, c->stream));
      HIPCHK(c, hipMemcpyAsync(doc_a.p + at, gdoc.p + q * nmax, n_of[q] * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
    }
    at += n_of[q];
  }
  return k_dr_sums_gathered_text(c, key_a.p, doc_a.p, key_b.p, doc_b.p, L, topic_sums_slice(L, W, (uint64_t)c->rank),
                                 topic_sums_slice(L, W, (uint64_t)c->rank + 1), sink, user, nbytes, nlines);
}

// The trainer's per-document report files formatted on the device (doc_report.hip) from what the catchword and topic-model stages left
// resident.  Several ranks: TOPIC_SUMS is collective, the other kinds are each rank's own business.
extern "C" int isle_hip_doc_report_text(isle_ctx* c, int what, uint64_t doc_begin, uint64_t doc_end, isle_text_sink_fn sink, void* user,
                                        uint64_t* nbytes, uint64_t* nlines) {
  if (!c) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  if (nbytes) *nbytes = 0;
  if (nlines) *nlines = 0;
  ISLECHK(post_prepare_sharded(c, "doc_report_text"));
  if (what != ISLE_DOCREPORT_CATCHWORDS && what != ISLE_DOCREPORT_TOPIC_SUMS && what != ISLE_DOCREPORT_TOPIC_SUMS_BY_DOC && what != ISLE_DOCREPORT_TOP_TWO)
    return isle_fail(c, ISLE_E_ARG, "doc_report_text: unknown kind %d", what);
  if (what == ISLE_DOCREPORT_CATCHWORDS ? !c->res.p_catch_ready : !c->res.p_model_ready)
    return isle_fail(c, ISLE_E_ARG, "doc_report_text: run %s first (a new count matrix voids its result)",
                     what == ISLE_DOCREPORT_CATCHWORDS ? "isle_hip_catchwords" : "isle_hip_topic_model");
  if (doc_begin > doc_end || doc_end > c->a_D)
    return isle_fail(c, ISLE_E_ARG, "doc_report_text: documents [%llu, %llu) of %llu", (unsigned long long)doc_begin, (unsigned long long)doc_end,
                     (unsigned long long)c->a_D);
  if (what == ISLE_DOCREPORT_TOPIC_SUMS && route_topic_sums(c->world) == TOPIC_SUMS_GATHERED)
    return topic_sums_gathered(c, doc_begin, doc_end, sink, user, nbytes, nlines);
  return k_doc_report_text(c, what, doc_begin, doc_end, sink, user, nbytes, nlines);
}

// The selection of topic_docs.hip on a CSR of (topic, value) by row, with the collectives between its steps: the counts' all-reduce with the
// word that says whether any rank found a bad entry, the eight rounds with the bins' all-reduce, the collect, the all-gather, the replicated
// sort and the lists on the host.  name: the call's, for the messages.  isle_hip_topic_top_docs runs it on its source, isle_hip_similar_docs
// on the (query, score) pairs of similar_docs.hip, the query in the place of the topic.
static int td_select(isle_ctx* c, const TdView& v, const char* name, uint32_t* docs, float* values, uint32_t* counts, uint64_t* topic_entries) {
  const size_t T = (size_t)v.num_topics, W = (size_t)c->world, n = (size_t)v.n;
  const uint64_t rows = v.rows, nnz = v.nnz;
  DevBuf<uint32_t> doc, rem, fill, bins, out_docs, out_counts;
  DevBuf<float> out_values;
  DevBuf<uint64_t> cnt, prefix, tables, err;
  StreamDrain drain(c);
  HIPCHK(c, doc.reserve(nnz ? nnz : 1));
  HIPCHK(c, cnt.reserve(T + 1));
  HIPCHK(c, err.reserve(1));
  HIPCHK(c, prefix.reserve(T));
  HIPCHK(c, rem.reserve(T));
  HIPCHK(c, fill.reserve(T));
  HIPCHK(c, bins.reserve(T * 256));
  HIPCHK(c, tables.reserve((W + 1) * T * n));
  HIPCHK(c, out_docs.reserve(T * n));
  HIPCHK(c, out_values.reserve(T * n));
  HIPCHK(c, out_counts.reserve(T));
  // the documents, this rank's counts, the form of the rows; the counts of the corpus travel with the number of ranks that refuse
  uint64_t bad = ~0ull;
  ISLECHK(k_td_docs(c, v, doc.p, cnt.p, err.p, &bad));
  const uint64_t refuses = bad != ~0ull;
  HIPCHK(c, hipMemcpy(cnt.p + T, &refuses, sizeof(uint64_t), hipMemcpyHostToDevice));
  ISLECHK(allreduce_sum<uint64_t>(c, cnt.p, T + 1));
  std::vector<uint64_t> cnt_host(T + 1);
  HIPCHK(c, hipMemcpyAsync(cnt_host.data(), cnt.p, (T + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (refuses) {
    const uint64_t e = bad >> 2;
    std::vector<int64_t> off(rows + 1);
    uint32_t tp = 0;
    HIPCHK(c, hipMemcpy(off.data(), v.off, (rows + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(&tp, v.topic + e, sizeof(tp), hipMemcpyDeviceToHost));
    const uint64_t row = (uint64_t)(std::upper_bound(off.begin(), off.end(), (int64_t)e) - off.begin()) - 1;
    return isle_fail(c, ISLE_E_ARG, "%s", topdocs_fault_text((unsigned)(bad & 3), e, row, tp, v.num_topics).c_str());
  }
  if (cnt_host[T]) return isle_fail(c, ISLE_E_ARG, "%s: another rank refused its entries (a topic >= num_topics, or topics that do not ascend in a row)", name);
  const uint64_t cnt_end = c->multi() ? (1ull << 31) : (1ull << 32);  // the bins are u32; the host-staged transport sums signed words
  for (size_t t = 0; t < T; ++t)
    if (cnt_host[t] >= cnt_end)
      return isle_fail(c, ISLE_E_ARG, "%s: topic %zu has %llu entries, 2^%d or more", name, t, (unsigned long long)cnt_host[t], c->multi() ? 31 : 32);
  // eight rounds, most significant byte first: every rank steps to the same smallest selected key from the same integers
  ISLECHK(k_td_init(c, v, cnt.p, prefix.p, rem.p));
  for (int shift = 56; shift >= 0; shift -= 8) {
    ISLECHK(k_td_hist(c, v, doc.p, prefix.p, shift, bins.p));
    ISLECHK(allreduce_sum<uint32_t>(c, bins.p, T * 256));
    ISLECHK(k_td_step(c, v, bins.p, cnt.p, shift, prefix.p, rem.p));
  }
  // each rank's winners, the tables side by side, the sort replicated
  uint64_t* const mine = c->multi() ? tables.p + W * T * n : tables.p;
  ISLECHK(k_td_collect(c, v, doc.p, prefix.p, fill.p, mine));
  if (c->multi()) {
    TimeScope ts(c, ISLE_T_COMM);
    ISLECHK(isle_allgather(c, mine, tables.p, T * n, ISLE_DT_U64));
  }
  ISLECHK(k_td_sort(c, v, tables.p, c->multi() ? (uint32_t)W : 1u, cnt.p, out_docs.p, out_values.p, out_counts.p));
  HIPCHK(c, hipMemcpyAsync(docs, out_docs.p, T * n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(values, out_values.p, T * n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(counts, out_counts.p, T * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (topic_entries) std::copy(cnt_host.begin(), cnt_host.begin() + T, topic_entries);
  return 0;
}

// the caller's CSR on the device for the call (rows may be 0: one offset)
static int td_upload(isle_ctx* c, uint64_t rows, uint64_t nnz, const int64_t* doc_offsets, const uint32_t* topic, const float* value, DevBuf<int64_t>& up_off,
                     DevBuf<uint32_t>& up_topic, DevBuf<float>& up_value, TdView* v) {
  const int64_t zero = 0;
  HIPCHK(c, up_off.reserve(rows + 1));
  HIPCHK(c, up_topic.reserve(nnz ? nnz : 1));
  HIPCHK(c, up_value.reserve(nnz ? nnz : 1));
  HIPCHK(c, hipMemcpy(up_off.p, rows ? doc_offsets : &zero, (rows + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
  if (nnz) HIPCHK(c, hipMemcpy(up_topic.p, topic, nnz * sizeof(uint32_t), hipMemcpyHostToDevice));
  if (nnz) HIPCHK(c, hipMemcpy(up_value.p, value, nnz * sizeof(float), hipMemcpyHostToDevice));
  v->off = up_off.p;
  v->topic = up_topic.p;
  v->value = up_value.p;
  return 0;
}

// The n heaviest documents of every topic (topic_docs.hip; the rule: topdocs_host.h), selected on entries that lie by document.  Several
// ranks: collective — the control values are agreed, the counts (with a word that says whether any rank found a bad entry) and the bins of
// every round are all-reduced, the ranks' tables of winners all-gathered and sorted replicated (td_select).  Every rank takes every step, a
// rank without rows or without entries included.  Nothing resident is written.
extern "C" int isle_hip_topic_top_docs(isle_ctx* c, int source, int num_topics, int n, uint64_t doc_base, uint64_t num_rows, const int64_t* doc_offsets,
                                       const uint32_t* topic, const float* value, uint32_t* docs, float* values, uint32_t* counts, uint64_t* topic_entries) {
  if (!c) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  const bool infer = source == ISLE_TOPDOCS_INFER, sums = source == ISLE_TOPDOCS_SUMS;
  if (infer && !c->res.inf_valid)
    return isle_fail(c, ISLE_E_ARG, "topic_top_docs: no resident result (run isle_hip_infer_resident; a new count matrix voids it)");
  if (sums && !c->res.p_model_ready) return isle_fail(c, ISLE_E_ARG, "topic_top_docs: run isle_hip_topic_model first (a new count matrix voids its result)");
  const uint64_t rows = infer ? c->inf_docs : (sums ? c->a_D : num_rows);
  const std::string why = topdocs_check_args(source, num_topics, n, c->world, doc_base, rows);
  if (!why.empty()) return isle_fail(c, ISLE_E_ARG, "%s", why.c_str());
  if (sums && num_topics != c->res.p_k)
    return isle_fail(c, ISLE_E_ARG, "topic_top_docs: num_topics = %d, the resident topic model has %d topics", num_topics, c->res.p_k);
  if (!docs || !values || !counts) return isle_fail(c, ISLE_E_ARG, "topic_top_docs: null docs / values / counts");
  uint64_t nnz = infer ? c->inf_n : (sums ? c->p_dts_n : 0);
  if (source == ISLE_TOPDOCS_HOST && rows) {
    if (!doc_offsets) return isle_fail(c, ISLE_E_ARG, "topic_top_docs: null doc_offsets with %llu rows", (unsigned long long)rows);
    const std::string bad_off = topdocs_check_offsets(doc_offsets, rows);
    if (!bad_off.empty()) return isle_fail(c, ISLE_E_ARG, "%s", bad_off.c_str());
    nnz = (uint64_t)doc_offsets[rows];
    if (nnz && (!topic || !value)) return isle_fail(c, ISLE_E_ARG, "topic_top_docs: null topic / value with %llu entries", (unsigned long long)nnz);
  }
  DevBuf<int64_t> up_off;
  DevBuf<uint32_t> up_topic;
  DevBuf<float> up_value;
  StreamDrain drain(c);
  if (c->multi()) {  // (every local refusal lies before this line)
    ISLECHK(agree_i32(c, source, "topic_top_docs: source"));
    ISLECHK(agree_i32(c, num_topics, "topic_top_docs: num_topics"));
    ISLECHK(agree_i32(c, n, "topic_top_docs: n"));
  }
  TdView v = {infer ? c->inf_off.p : c->p_dts_off.p, infer ? c->inf_topic.p : c->p_dts_topic.p, infer ? c->inf_weight.p : c->p_dts_val.p,
              rows,  nnz, doc_base, (uint32_t)num_topics, (uint32_t)n, infer ? ISLE_T_INFER : ISLE_T_POST};
  if (source == ISLE_TOPDOCS_HOST) ISLECHK(td_upload(c, rows, nnz, doc_offsets, topic, value, up_off, up_topic, up_value, &v));
  return td_select(c, v, "topic_top_docs", docs, values, counts, topic_entries);
}

// The context's home of the query table of isle_hip_similar_docs (route_host.h, route_simdocs_table): a setting, not an environment switch.
extern "C" int isle_hip_simdocs_table_form(isle_ctx* c, int form) {
  if (!c) return ISLE_E_ARG;
  const std::string why = simdocs_check_form(form);
  if (!why.empty()) return isle_fail(c, ISLE_E_ARG, "%s", why.c_str());
  c->simdocs_table_form = form;
  return 0;
}

// The n documents most similar to each query (similar_docs.hip; the rule: simdocs_host.h): the queries densified into a table, every row
// scored against every query it shares a stored topic with, the (query, score) pairs written as a CSR by row, and td_select on that CSR with
// the query in the place of the topic.  Several ranks: collective — the control values and a hash of the queries are agreed, one word says
// whether any rank refuses its rows, then td_select's collectives.  Nothing resident is written.
extern "C" int isle_hip_similar_docs(isle_ctx* c, int source, int measure, int num_topics, int n, uint64_t doc_base, uint64_t num_rows,
                                     const int64_t* doc_offsets, const uint32_t* topic, const float* value, int num_queries, const uint64_t* query_rows,
                                     const int64_t* q_offsets, const uint32_t* q_topic, const float* q_weight, const uint32_t* exclude, uint32_t* docs,
                                     float* scores, uint32_t* counts, uint64_t* candidates) {
  if (!c) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  const bool infer = source == ISLE_TOPDOCS_INFER, sums = source == ISLE_TOPDOCS_SUMS;
  if (infer && !c->res.inf_valid)
    return isle_fail(c, ISLE_E_ARG, "similar_docs: no resident result (run isle_hip_infer_resident; a new count matrix voids it)");
  if (sums && !c->res.p_model_ready) return isle_fail(c, ISLE_E_ARG, "similar_docs: run isle_hip_topic_model first (a new count matrix voids its result)");
  const uint64_t rows = infer ? c->inf_docs : (sums ? c->a_D : num_rows);
  const std::string why = simdocs_check_args(source, measure, num_topics, n, num_queries, c->world, doc_base, rows);
  if (!why.empty()) return isle_fail(c, ISLE_E_ARG, "%s", why.c_str());
  if (sums && num_topics != c->res.p_k)
    return isle_fail(c, ISLE_E_ARG, "similar_docs: num_topics = %d, the resident topic model has %d topics", num_topics, c->res.p_k);
  if (infer && num_topics != c->inf_cols)
    return isle_fail(c, ISLE_E_ARG, "similar_docs: num_topics = %d, the resident inference result has %d topics", num_topics, c->inf_cols);
  if (!docs || !scores || !counts) return isle_fail(c, ISLE_E_ARG, "similar_docs: null docs / scores / counts");
  uint64_t nnz = infer ? c->inf_n : (sums ? c->p_dts_n : 0);
  if (source == ISLE_TOPDOCS_HOST && rows) {
    if (!doc_offsets) return isle_fail(c, ISLE_E_ARG, "similar_docs: null doc_offsets with %llu rows", (unsigned long long)rows);
    const std::string bad_off = topdocs_check_offsets(doc_offsets, rows);
    if (!bad_off.empty()) return isle_fail(c, ISLE_E_ARG, "similar_docs: %s", bad_off.c_str() + sizeof("topic_top_docs: ") - 1);
    nnz = (uint64_t)doc_offsets[rows];
    if (nnz && (!topic || !value)) return isle_fail(c, ISLE_E_ARG, "similar_docs: null topic / value with %llu entries", (unsigned long long)nnz);
  }
  const uint32_t Q = (uint32_t)num_queries, Qp = simdocs_qp(Q);
  uint64_t qnnz = 0;
  if (query_rows) {
    if (c->world > 1) return isle_fail(c, ISLE_E_ARG, "similar_docs: query_rows with %d ranks: a row lives on one rank, pass the queries as a CSR", c->world);
    const std::string bad_rows = simdocs_check_query_rows(query_rows, num_queries, rows);
    if (!bad_rows.empty()) return isle_fail(c, ISLE_E_ARG, "%s", bad_rows.c_str());
  } else {
    if (!q_offsets) return isle_fail(c, ISLE_E_ARG, "similar_docs: null q_offsets and no query_rows");
    if (q_offsets[0] == 0 && q_offsets[num_queries] > 0 && (!q_topic || !q_weight)) return isle_fail(c, ISLE_E_ARG, "similar_docs: null q_topic / q_weight");
    const std::string bad_q = simdocs_check_queries(num_queries, (uint32_t)num_topics, q_offsets, q_topic, q_weight);
    if (!bad_q.empty()) return isle_fail(c, ISLE_E_ARG, "%s", bad_q.c_str());
    qnnz = (uint64_t)q_offsets[num_queries];
  }
  std::vector<uint32_t> ex(Qp, SIMDOCS_NO_DOC);
  for (uint32_t q = 0; q < Q; ++q) ex[q] = exclude ? exclude[q] : (query_rows ? (uint32_t)(doc_base + query_rows[q]) : SIMDOCS_NO_DOC);
  DevBuf<int64_t> up_off, dq_off, pair_off, blk;
  DevBuf<uint32_t> up_topic, dq_topic, d_ex, cnt, qid;
  DevBuf<float> up_value, dq_weight, table, score;
  DevBuf<double> nq;
  DevBuf<uint64_t> d_qrows, err, word;
  StreamDrain drain(c);
  if (c->multi()) {  // (every local refusal lies before this line)
    ISLECHK(agree_i32(c, source, "similar_docs: source"));
    ISLECHK(agree_i32(c, measure, "similar_docs: measure"));
    ISLECHK(agree_i32(c, num_topics, "similar_docs: num_topics"));
    ISLECHK(agree_i32(c, n, "similar_docs: n"));
    ISLECHK(agree_i32(c, num_queries, "similar_docs: num_queries"));
    // (query_rows reach this line with a communicator of one rank only: the rows' numbers stand for their entries)
    const uint64_t h = query_rows ? simdocs_hash_bytes(simdocs_hash_bytes(0xcbf29ce484222325ull, query_rows, (size_t)Q * sizeof(uint64_t)), ex.data(), (size_t)Q * sizeof(uint32_t))
                                  : simdocs_query_hash(num_queries, q_offsets, q_topic, q_weight, exclude);
    uint64_t tag[2] = {h, ~h};  // max over (v, ~v): the largest and the complement of the smallest
    HIPCHK(c, word.reserve(2));
    ISLECHK(allreduce_host<uint64_t>(c, tag, 2, word.p, true));
    if (tag[0] != ~tag[1]) return isle_fail(c, ISLE_E_COMM, "similar_docs: ranks disagree on the queries or the excluded documents (a hash of them differs)");
  }
  const int fam = infer ? ISLE_T_INFER : ISLE_T_POST;
  TdView v = {infer ? c->inf_off.p : c->p_dts_off.p, infer ? c->inf_topic.p : c->p_dts_topic.p, infer ? c->inf_weight.p : c->p_dts_val.p,
              rows,  nnz, doc_base, (uint32_t)num_topics, (uint32_t)n, fam};
  if (source == ISLE_TOPDOCS_HOST) ISLECHK(td_upload(c, rows, nnz, doc_offsets, topic, value, up_off, up_topic, up_value, &v));
  // the query CSR on the device: uploaded, or gathered from the source's rows
  HIPCHK(c, dq_off.reserve((size_t)Q + 1));
  if (query_rows) {
    std::vector<int64_t> q_off_host((size_t)Q + 1);
    HIPCHK(c, d_qrows.reserve(Q));
    HIPCHK(c, hipMemcpy(d_qrows.p, query_rows, (size_t)Q * sizeof(uint64_t), hipMemcpyHostToDevice));
    ISLECHK(k_sd_gather_offsets(c, v, d_qrows.p, Q, dq_off.p, q_off_host.data()));
    qnnz = (uint64_t)q_off_host[Q];
    HIPCHK(c, dq_topic.reserve(qnnz ? qnnz : 1));
    HIPCHK(c, dq_weight.reserve(qnnz ? qnnz : 1));
    ISLECHK(k_sd_gather(c, v, d_qrows.p, Q, dq_off.p, dq_topic.p, dq_weight.p));
  } else {
    HIPCHK(c, dq_topic.reserve(qnnz ? qnnz : 1));
    HIPCHK(c, dq_weight.reserve(qnnz ? qnnz : 1));
    HIPCHK(c, hipMemcpy(dq_off.p, q_offsets, ((size_t)Q + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
    if (qnnz) HIPCHK(c, hipMemcpy(dq_topic.p, q_topic, qnnz * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (qnnz) HIPCHK(c, hipMemcpy(dq_weight.p, q_weight, qnnz * sizeof(float), hipMemcpyHostToDevice));
  }
  HIPCHK(c, table.reserve((size_t)num_topics * Qp));
  HIPCHK(c, nq.reserve(Qp));
  HIPCHK(c, d_ex.reserve(Qp));
  HIPCHK(c, hipMemcpy(d_ex.p, ex.data(), (size_t)Qp * sizeof(uint32_t), hipMemcpyHostToDevice));
  ISLECHK(k_sd_table(c, fam, Q, (uint32_t)num_topics, dq_off.p, dq_topic.p, dq_weight.p, table.p, nq.p));
  // the rows' candidate counts and their form; one word through the ranks says whether any of them refuses
  const bool lds = route_simdocs_table(num_queries, (uint64_t)num_topics, c->simdocs_table_form) == SIMDOCS_HOME_LDS;
  HIPCHK(c, cnt.reserve(rows ? rows : 1));
  HIPCHK(c, pair_off.reserve(rows + 1));
  HIPCHK(c, blk.reserve(isle_scan_scratch(rows)));
  HIPCHK(c, err.reserve(1));
  uint64_t bad = ~0ull, pairs = 0;
  ISLECHK(k_sd_count(c, v, lds, Q, table.p, d_ex.p, cnt.p, pair_off.p, blk.p, err.p, &bad, &pairs));
  const bool too_many = pairs >= (1ull << 32);
  uint64_t refusing = (bad != ~0ull || too_many) ? 1 : 0;
  if (c->multi()) {
    HIPCHK(c, word.reserve(2));
    ISLECHK(allreduce_host<uint64_t>(c, &refusing, 1, word.p));
  }
  if (bad != ~0ull) {
    const uint64_t e = bad >> 2;
    const unsigned what = (unsigned)(bad & 3);
    std::vector<int64_t> off(rows + 1);
    uint32_t tp = 0;
    float w = 0.f;
    HIPCHK(c, hipMemcpy(off.data(), v.off, (rows + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(&tp, v.topic + e, sizeof(tp), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(&w, v.value + e, sizeof(w), hipMemcpyDeviceToHost));
    const uint64_t row = (uint64_t)(std::upper_bound(off.begin(), off.end(), (int64_t)e) - off.begin()) - 1;
    if (what == SIMDOCS_BAD_WEIGHT) return isle_fail(c, ISLE_E_ARG, "%s", simdocs_weight_text("row", e, row, w).c_str());
    return isle_fail(c, ISLE_E_ARG, "similar_docs: %s", topdocs_fault_text(what, e, row, tp, (uint32_t)num_topics).c_str() + sizeof("topic_top_docs: ") - 1);
  }
  if (too_many)
    return isle_fail(c, ISLE_E_ARG, "similar_docs: %llu candidate pairs on this rank, 2^32 or more: ask with fewer queries", (unsigned long long)pairs);
  if (refusing) return isle_fail(c, ISLE_E_ARG, "similar_docs: another rank refused its rows (a bad weight or topic, or 2^32 candidate pairs or more)");
  // the pairs' (query, score) by row, and the selection with the query in the place of the topic
  HIPCHK(c, qid.reserve(pairs ? pairs : 1));
  HIPCHK(c, score.reserve(pairs ? pairs : 1));
  ISLECHK(k_sd_score(c, v, measure, lds, Q, table.p, d_ex.p, nq.p, pair_off.p, qid.p, score.p));
  const TdView sel = {pair_off.p, qid.p, score.p, rows, pairs, doc_base, Q, (uint32_t)n, fam};
  return td_select(c, sel, "similar_docs", docs, scores, counts, candidates);
}

// The context's topic tile of isle_hip_topic_prevalence (prevalence_host.h, prev_tile): a setting, not an environment switch.
extern "C" int isle_hip_prevalence_tile_form(isle_ctx* c, int form) {
  if (!c) return ISLE_E_ARG;
  const std::string why = prevalence_check_form(form);
  if (!why.empty()) return isle_fail(c, ISLE_E_ARG, "%s", why.c_str());
  c->prevalence_tile_form = form;
  return 0;
}

// Topic prevalence by document group (topic_prevalence.hip; the rule: prevalence_host.h): the row pass with its checks and integer tables,
// the rows listed by group (a stable sort by label; the identity without labels), the bases of every level, and per topic tile the level-0
// partials and the folds, the last of which writes sum.  One rank only: refused with several, before any collective.  Nothing resident is
// written and nothing is kept.
extern "C" int isle_hip_topic_prevalence(isle_ctx* c, int source, int num_topics, uint64_t num_rows, const int64_t* doc_offsets, const uint32_t* topic,
                                         const float* value, const uint32_t* groups, uint32_t num_groups, int normalise, uint64_t* docs, uint64_t* unlabelled,
                                         uint64_t* count, uint64_t* dominant, double* sum) {
  if (!c) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  const bool infer = source == ISLE_TOPDOCS_INFER, sums = source == ISLE_TOPDOCS_SUMS;
  if (infer && !c->res.inf_valid)
    return isle_fail(c, ISLE_E_ARG, "topic_prevalence: no resident result (run isle_hip_infer_resident; a new count matrix voids it)");
  if (sums && !c->res.p_model_ready) return isle_fail(c, ISLE_E_ARG, "topic_prevalence: run isle_hip_topic_model first (a new count matrix voids its result)");
  const uint64_t rows = infer ? c->inf_docs : (sums ? c->a_D : num_rows);
  const std::string why = prevalence_check_args(source, num_topics, num_groups, normalise, groups != nullptr, c->world, rows);
  if (!why.empty()) return isle_fail(c, ISLE_E_ARG, "%s", why.c_str());
  if (sums && num_topics != c->res.p_k)
    return isle_fail(c, ISLE_E_ARG, "topic_prevalence: num_topics = %d, the resident topic model has %d topics", num_topics, c->res.p_k);
  if (infer && num_topics != c->inf_cols)
    return isle_fail(c, ISLE_E_ARG, "topic_prevalence: num_topics = %d, the resident inference result has %d topics", num_topics, c->inf_cols);
  if (!docs || !count || !dominant || !sum) return isle_fail(c, ISLE_E_ARG, "topic_prevalence: null docs / count / dominant / sum");
  uint64_t nnz = infer ? c->inf_n : (sums ? c->p_dts_n : 0);
  if (source == ISLE_TOPDOCS_HOST && rows) {
    if (!doc_offsets) return isle_fail(c, ISLE_E_ARG, "topic_prevalence: null doc_offsets with %llu rows", (unsigned long long)rows);
    const std::string bad_off = topdocs_check_offsets(doc_offsets, rows);
    if (!bad_off.empty()) return isle_fail(c, ISLE_E_ARG, "topic_prevalence: %s", bad_off.c_str() + sizeof("topic_top_docs: ") - 1);
    nnz = (uint64_t)doc_offsets[rows];
    if (nnz && (!topic || !value)) return isle_fail(c, ISLE_E_ARG, "topic_prevalence: null topic / value with %llu entries", (unsigned long long)nnz);
  }
  const uint32_t G = num_groups;
  const size_t k = (size_t)num_topics, cells = (size_t)G * k;
  DevBuf<int64_t> up_off;
  DevBuf<uint32_t> up_topic, d_groups, row_a, row_b;
  DevBuf<float> up_value;
  DevBuf<uint64_t> d_docs, d_count, d_dom, err, key_a, key_b, bases, cnt, blk;
  DevBuf<double> d_sum, rs, part_a, part_b;
  StreamDrain drain(c);
  TdView v = {infer ? c->inf_off.p : c->p_dts_off.p, infer ? c->inf_topic.p : c->p_dts_topic.p, infer ? c->inf_weight.p : c->p_dts_val.p,
              rows,  nnz, 0, (uint32_t)num_topics, 0, infer ? ISLE_T_INFER : ISLE_T_POST};
  if (source == ISLE_TOPDOCS_HOST) ISLECHK(td_upload(c, rows, nnz, doc_offsets, topic, value, up_off, up_topic, up_value, &v));
  const bool labelled = groups != nullptr && rows > 0;
  if (labelled) {
    HIPCHK(c, d_groups.reserve(rows));
    HIPCHK(c, hipMemcpy(d_groups.p, groups, rows * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIPCHK(c, key_a.reserve(rows));
    HIPCHK(c, key_b.reserve(rows));
    HIPCHK(c, row_a.reserve(rows));
    HIPCHK(c, row_b.reserve(rows));
  }
  HIPCHK(c, d_docs.reserve((size_t)G + 1));
  HIPCHK(c, d_count.reserve(cells));
  HIPCHK(c, d_dom.reserve(cells));
  HIPCHK(c, d_sum.reserve(cells));
  HIPCHK(c, err.reserve(2));
  if (normalise) HIPCHK(c, rs.reserve(rows ? rows : 1));
  // the row pass: the checks, the integer tables, the row sums, the sort's pairs
  uint64_t bad_row = ~0ull, bad_entry = ~0ull;
  ISLECHK(k_tp_rows(c, v, labelled ? d_groups.p : nullptr, G, d_docs.p, d_count.p, d_dom.p, normalise ? rs.p : nullptr, labelled ? key_a.p : nullptr,
                    labelled ? row_a.p : nullptr, err.p, &bad_row, &bad_entry));
  if (bad_row != ~0ull) return isle_fail(c, ISLE_E_ARG, "%s", prevalence_label_text(bad_row, groups[bad_row], G).c_str());
  if (bad_entry != ~0ull) {
    const uint64_t e = bad_entry >> 2;
    std::vector<int64_t> off(rows + 1);
    uint32_t tp = 0;
    float w = 0.f;
    HIPCHK(c, hipMemcpy(off.data(), v.off, (rows + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(&tp, v.topic + e, sizeof(tp), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(&w, v.value + e, sizeof(w), hipMemcpyDeviceToHost));
    const uint64_t row = (uint64_t)(std::upper_bound(off.begin(), off.end(), (int64_t)e) - off.begin()) - 1;
    return isle_fail(c, ISLE_E_ARG, "%s", prevalence_entry_text((unsigned)(bad_entry & 3), e, row, tp, w, (uint32_t)num_topics).c_str());
  }
  std::vector<uint64_t> docs_host((size_t)G + 1);
  HIPCHK(c, hipMemcpy(docs_host.data(), d_docs.p, ((size_t)G + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
  // the levels of the tree: as many as the largest group needs; the values of every level over all groups
  const int levels = prev_levels(*std::max_element(docs_host.begin(), docs_host.begin() + G));
  std::vector<uint64_t> totals((size_t)levels + 2, 0), lvl(docs_host.begin(), docs_host.begin() + G);
  for (int j = 0; j <= levels; ++j)
    for (size_t g = 0; g < G; ++g) {
      totals[j] += lvl[g];
      lvl[g] = (lvl[g] + PREV_FAN - 1) / PREV_FAN;
    }
  HIPCHK(c, hipMemsetAsync(d_sum.p, 0, cells * sizeof(double), c->stream));
  if (levels) {
    // the rows by group: a stable sort by label keeps the rows of a group ascending; the rows of no group sort behind every group
    const uint32_t* list = nullptr;
    if (labelled) {
      int bits = 1;
      while (bits < 32 && (G >> bits)) ++bits;
      bool in_a = true;
      {
        TimeScope ts(c, v.fam);
        ISLECHK(k_sort_pairs_u64(c, key_a.p, row_a.p, key_b.p, row_b.p, rows, bits, &in_a));
      }
      list = in_a ? row_a.p : row_b.p;
    }
    HIPCHK(c, bases.reserve(((size_t)levels + 1) * ((size_t)G + 1)));
    HIPCHK(c, cnt.reserve(G));
    HIPCHK(c, blk.reserve(isle_scan_scratch(G)));
    ISLECHK(k_tp_bases(c, v.fam, d_docs.p, G, levels, bases.p, cnt.p, blk.p));
    const uint32_t tile = prev_tile((uint32_t)num_topics, c->prevalence_tile_form);
    HIPCHK(c, part_a.reserve(levels > 1 ? (size_t)totals[1] * tile : 1));
    HIPCHK(c, part_b.reserve(levels > 2 ? (size_t)totals[2] * tile : 1));
    for (uint32_t t0 = 0; t0 < (uint32_t)num_topics; t0 += tile)
      ISLECHK(k_tp_tile(c, v, list, normalise ? rs.p : nullptr, G, bases.p, levels, totals.data(), t0, std::min(tile, (uint32_t)num_topics - t0), part_a.p,
                        part_b.p, d_sum.p));
  }
  HIPCHK(c, hipMemcpyAsync(count, d_count.p, cells * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(dominant, d_dom.p, cells * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(sum, d_sum.p, cells * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::copy(docs_host.begin(), docs_host.begin() + G, docs);
  if (unlabelled) *unlabelled = docs_host[G];
  return 0;
}

// ---- held-out scores per document (score_docs.hip; the rule: score_host.h)
#include "score_host.h"  // (included here, above its only users)
extern "C" int isle_hip_score_total(const double* v, uint64_t n, double* out) {
  if (!out || (n && !v)) return ISLE_E_ARG;
  *out = score_total(v, n);
  return 0;
}

// the row of entry e (a position in the arrays the offsets point into) under offsets that lie on the device (rows + 1 of them)
static int sc_row_of(isle_ctx* c, const int64_t* off_dev, uint64_t rows, uint64_t e, uint64_t* row) {
  std::vector<int64_t> off(rows + 1);
  HIPCHK(c, hipMemcpy(off.data(), off_dev, (rows + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
  *row = (uint64_t)(std::upper_bound(off.begin(), off.end(), (int64_t)e) - off.begin()) - 1;
  return 0;
}

// Every refusal that needs no entry comes before the first launch and before any upload; the weight rows are checked on the device before
// the walk reads them.  No collective: with several ranks every rank scores its own rows.  Nothing resident is written, nothing is kept.
extern "C" int isle_hip_score_docs(isle_ctx* c, int which, const float* model_host, uint64_t vocab, int ncols, int weights_source, uint64_t num_rows,
                                   const int64_t* w_offsets, const uint32_t* w_topic, const float* w_weight, int entries_source, uint64_t doc_begin,
                                   const float* counts, const uint32_t* rows_in, const int64_t* offsets, int measure, int normalise, double floor,
                                   double* score, double* tokens, uint32_t* unscored_entries, double* unscored_tokens, uint32_t* floored, double* z_out) {
  if (!c) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  ISLECHK(model_reader_ok(c, which, "score_docs"));
  const std::string why = score_check_args(weights_source, entries_source, measure, normalise, floor, ncols);
  if (!why.empty()) return isle_fail(c, ISLE_E_ARG, "%s", why.c_str());
  const bool infer = weights_source == ISLE_TOPDOCS_INFER, resident = entries_source == ISLE_SCORE_RESIDENT;
  if (infer && !c->res.inf_valid)
    return isle_fail(c, ISLE_E_ARG, "score_docs: no resident result (run isle_hip_infer_resident; a new count matrix voids it)");
  if (resident) ISLECHK(post_prepare_sharded(c, "score_docs"));
  if (vocab == 0 || vocab > 0xfffffff0ull) return isle_fail(c, ISLE_E_ARG, "score_docs: vocab out of range");
  if (infer && num_rows != c->inf_docs) return isle_fail(c, ISLE_E_ARG, "%s", score_rows_text(num_rows, c->inf_docs, "the resident inference result").c_str());
  if (infer && ncols != c->inf_cols)
    return isle_fail(c, ISLE_E_ARG, "score_docs: ncols = %d, the resident inference result has %d topics", ncols, c->inf_cols);
  if (resident) {
    if (doc_begin > c->a_D || num_rows > c->a_D - doc_begin) return isle_fail(c, ISLE_E_ARG, "%s", score_range_text(doc_begin, num_rows, c->a_D).c_str());
    if (vocab != c->a_V) return isle_fail(c, ISLE_E_ARG, "%s", score_vocab_text(vocab, c->a_V).c_str());
    if (infer && doc_begin != c->inf_doc_begin) return isle_fail(c, ISLE_E_ARG, "%s", score_begin_text(doc_begin, c->inf_doc_begin).c_str());
    if (z_out) return isle_fail(c, ISLE_E_ARG, "score_docs: z_out with ISLE_SCORE_RESIDENT (fetch the entries and pass them as ISLE_SCORE_HOST)");
  }
  if (num_rows && (!score || !tokens || !unscored_entries || !unscored_tokens || !floored))
    return isle_fail(c, ISLE_E_ARG, "score_docs: null score / tokens / unscored_entries / unscored_tokens / floored");
  uint64_t w_nnz = infer ? c->inf_n : 0, e_nnz = 0;
  if (!infer && num_rows) {
    if (!w_offsets) return isle_fail(c, ISLE_E_ARG, "score_docs: null w_offsets with %llu rows", (unsigned long long)num_rows);
    const std::string bad_off = score_check_offsets("w_offsets", w_offsets, num_rows);
    if (!bad_off.empty()) return isle_fail(c, ISLE_E_ARG, "%s", bad_off.c_str());
    w_nnz = (uint64_t)w_offsets[num_rows];
    if (w_nnz && (!w_topic || !w_weight)) return isle_fail(c, ISLE_E_ARG, "score_docs: null w_topic / w_weight with %llu entries", (unsigned long long)w_nnz);
  }
  if (!resident && num_rows) {
    if (!offsets) return isle_fail(c, ISLE_E_ARG, "score_docs: null offsets with %llu rows", (unsigned long long)num_rows);
    const std::string bad_off = score_check_offsets("offsets", offsets, num_rows);
    if (!bad_off.empty()) return isle_fail(c, ISLE_E_ARG, "%s", bad_off.c_str());
    e_nnz = (uint64_t)offsets[num_rows];
    if (e_nnz && (!counts || !rows_in)) return isle_fail(c, ISLE_E_ARG, "score_docs: null counts / rows with %llu entries", (unsigned long long)e_nnz);
  }
  const float* dev = nullptr;
  DevBuf<float> up, packed, up_value, e_cnt;
  DevBuf<int64_t> up_off, e_off;
  DevBuf<uint32_t> up_topic, e_rows, d_ue, d_fl;
  DevBuf<uint64_t> err;
  DevBuf<double> rs, d_score, d_tok, d_ut, d_z;
  StreamDrain drain(c);
  ISLECHK(model_source(c, which, model_host, vocab, ncols, "score_docs", &up, &dev));
  if (!num_rows) return 0;
  const int ld = (ncols + 3) & ~3;
  TdView w = {c->inf_off.p, c->inf_topic.p, c->inf_weight.p, num_rows, w_nnz, 0, (uint32_t)ncols, 0, ISLE_T_INFER};
  if (!infer) ISLECHK(td_upload(c, num_rows, w_nnz, w_offsets, w_topic, w_weight, up_off, up_topic, up_value, &w));
  HIPCHK(c, err.reserve(1));
  HIPCHK(c, rs.reserve(num_rows));
  uint64_t bad = ~0ull;
  ISLECHK(k_sc_rows(c, w, rs.p, err.p, &bad));
  if (bad != ~0ull) {
    const uint64_t e = bad >> 2;
    uint64_t row = 0;
    uint32_t tp = 0;
    float wt = 0.f;
    ISLECHK(sc_row_of(c, w.off, num_rows, e, &row));
    HIPCHK(c, hipMemcpy(&tp, w.topic + e, sizeof(tp), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(&wt, w.value + e, sizeof(wt), hipMemcpyDeviceToHost));
    return isle_fail(c, ISLE_E_ARG, "%s", score_weight_text((unsigned)(bad & 3), e, row, tp, wt, (uint32_t)ncols).c_str());
  }
  // the entries: documents [doc_begin, doc_begin + num_rows) of A where they lie, or the caller's, uploaded
  const float* cnt_dev = c->a_cnt.p;
  const uint32_t* word_dev = c->a_rows.p;
  const int64_t* off_dev = resident ? c->a_offs.p + doc_begin : nullptr;
  if (!resident) {
    HIPCHK(c, e_off.reserve(num_rows + 1));
    HIPCHK(c, e_cnt.reserve(e_nnz ? e_nnz : 1));
    HIPCHK(c, e_rows.reserve(e_nnz ? e_nnz : 1));
    HIPCHK(c, hipMemcpy(e_off.p, offsets, (num_rows + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
    if (e_nnz) HIPCHK(c, hipMemcpy(e_cnt.p, counts, e_nnz * sizeof(float), hipMemcpyHostToDevice));
    if (e_nnz) HIPCHK(c, hipMemcpy(e_rows.p, rows_in, e_nnz * sizeof(uint32_t), hipMemcpyHostToDevice));
    cnt_dev = e_cnt.p;
    word_dev = e_rows.p;
    off_dev = e_off.p;
  }
  HIPCHK(c, packed.reserve((size_t)vocab * ld));
  ISLECHK(k_inf_pack(c, dev, vocab, ncols, packed.p));
  HIPCHK(c, d_score.reserve(num_rows));
  HIPCHK(c, d_tok.reserve(num_rows));
  HIPCHK(c, d_ut.reserve(num_rows));
  HIPCHK(c, d_ue.reserve(num_rows));
  HIPCHK(c, d_fl.reserve(num_rows));
  const bool with_z = z_out && e_nnz;
  if (with_z) HIPCHK(c, d_z.reserve(e_nnz));
  ISLECHK(k_sc_walk(c, w, packed.p, ld, vocab, cnt_dev, word_dev, off_dev, normalise ? rs.p : nullptr, measure, floor, d_score.p, d_tok.p, d_ue.p, d_ut.p,
                    d_fl.p, with_z ? d_z.p : nullptr, err.p, &bad));
  if (bad != ~0ull) {
    const uint64_t e = bad >> 1;
    uint64_t row = 0;
    uint32_t wd = 0;
    float ct = 0.f;
    ISLECHK(sc_row_of(c, off_dev, num_rows, e, &row));
    HIPCHK(c, hipMemcpy(&wd, word_dev + e, sizeof(wd), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(&ct, cnt_dev + e, sizeof(ct), hipMemcpyDeviceToHost));
    return isle_fail(c, ISLE_E_ARG, "%s", score_entry_text((unsigned)(bad & 1), e, row, wd, ct, vocab).c_str());
  }
  HIPCHK(c, hipMemcpyAsync(score, d_score.p, num_rows * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(tokens, d_tok.p, num_rows * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(unscored_tokens, d_ut.p, num_rows * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(unscored_entries, d_ue.p, num_rows * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(floored, d_fl.p, num_rows * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  if (with_z) HIPCHK(c, hipMemcpyAsync(z_out, d_z.p, e_nnz * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int isle_hip_avg_doc_sz(isle_ctx* c, float* out) {
  if (!c) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  ISLECHK(post_prepare_sharded(c, "avg_doc_sz"));
  if (!out) return isle_fail(c, ISLE_E_ARG, "avg_doc_sz: null out");
  ISLECHK(ensure_avg_doc_sz(c));
  *out = c->a_avg;
  return 0;
}

// ---- near-duplicate documents by MinHash (near_dups.hip; the rule: neardup_host.h)
#include "neardup_host.h"  // (included here, above its only users)
// what the four calls check before anything is launched: every refusal is a rank's own and comes before any collective (there is none)
static int nd_args_ok(isle_ctx* c, const char* who, uint64_t num, uint64_t den, int bands, int rows_per_band) {
  const std::string why = nd_check_args(who, c->res.a_ready, num, den, bands, rows_per_band, c->world);
  if (!why.empty()) return isle_fail(c, ISLE_E_ARG, "%s", why.c_str());
  return 0;
}

extern "C" int isle_hip_neardup_key_form(isle_ctx* c, int form) {
  if (!c) return ISLE_E_ARG;
  if (form != ISLE_NEARDUP_KEY_AUTO && form != ISLE_NEARDUP_KEY_FULL && form != ISLE_NEARDUP_KEY_NARROW)
    return isle_fail(c, ISLE_E_ARG, "neardup_key_form: unknown form %d", form);
  c->neardup_key_form = form;
  return 0;
}

extern "C" int isle_hip_doc_signatures(isle_ctx* c, int bands, int rows_per_band, uint64_t* sig_out, uint64_t* keys_out) {
  if (!c) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  ISLECHK(nd_args_ok(c, "doc_signatures", 1, 1, bands, rows_per_band));
  const uint64_t D = c->a_D, H = (uint64_t)bands * rows_per_band;
  DevBuf<uint64_t> sig, keys;
  StreamDrain drain(c);
  if (sig_out) HIPCHK(c, sig.reserve(D ? D * H : 1));
  if (keys_out) HIPCHK(c, keys.reserve(D ? D * bands : 1));
  ISLECHK(k_nd_signatures(c, bands, rows_per_band, sig_out ? sig.p : nullptr, keys_out ? keys.p : nullptr));
  if (sig_out && D) HIPCHK(c, hipMemcpyAsync(sig_out, sig.p, D * H * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  if (keys_out && D) HIPCHK(c, hipMemcpyAsync(keys_out, keys.p, D * bands * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int isle_hip_doc_jaccard(isle_ctx* c, uint64_t n_pairs, const uint32_t* a, const uint32_t* b, uint32_t* inter_out, uint32_t* uni_out) {
  if (!c) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  ISLECHK(nd_args_ok(c, "doc_jaccard", 1, 1, 1, 1));
  if (n_pairs && (!a || !b)) return isle_fail(c, ISLE_E_ARG, "doc_jaccard: null pairs");
  const uint64_t bad = nd_first_bad_pair(n_pairs, a, b, c->a_D);
  if (bad < n_pairs) return isle_fail(c, ISLE_E_ARG, "%s", nd_bad_pair(bad, a[bad], b[bad], c->a_D).c_str());
  if (!n_pairs) return 0;
  DevBuf<uint32_t> a_dev, b_dev, inter, uni;
  StreamDrain drain(c);
  HIPCHK(c, a_dev.reserve(n_pairs));
  HIPCHK(c, b_dev.reserve(n_pairs));
  HIPCHK(c, inter.reserve(n_pairs));
  HIPCHK(c, uni.reserve(n_pairs));
  HIPCHK(c, hipMemcpyAsync(a_dev.p, a, n_pairs * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(b_dev.p, b, n_pairs * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  ISLECHK(k_nd_jaccard(c, n_pairs, a_dev.p, b_dev.p, inter.p, uni.p));
  if (inter_out) HIPCHK(c, hipMemcpyAsync(inter_out, inter.p, n_pairs * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  if (uni_out) HIPCHK(c, hipMemcpyAsync(uni_out, uni.p, n_pairs * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

// what isle_hip_doc_near_duplicates and isle_hip_prune_near_docs share: the keys, the resolution, the roots and the kept flags
struct NdFound {
  DevBuf<uint64_t> keys;
  DevBuf<uint32_t> parent, first_of, keep;
  uint64_t kept = 0, pairs_tested = 0, rounds = 0;
};
static int nd_find(isle_ctx* c, uint64_t num, uint64_t den, int bands, int rows_per_band, NdFound& f) {
  const uint64_t D = c->a_D;
  HIPCHK(c, f.keys.reserve(D ? D * bands : 1));
  HIPCHK(c, f.parent.reserve(D ? D : 1));
  HIPCHK(c, f.first_of.reserve(D ? D : 1));
  HIPCHK(c, f.keep.reserve(D ? D : 1));
  ISLECHK(k_nd_signatures(c, bands, rows_per_band, nullptr, f.keys.p));
  return k_nd_resolve(c, route_neardup_key(c->neardup_key_form), num, den, bands, f.keys.p, f.parent.p, f.first_of.p, f.keep.p, &f.kept, &f.pairs_tested, &f.rounds);
}

extern "C" int isle_hip_doc_near_duplicates(isle_ctx* c, uint64_t num, uint64_t den, int bands, int rows_per_band, uint32_t* parent_out, uint32_t* first_of_out,
                                            uint64_t* n_dropped, uint64_t* pairs_tested, uint64_t* rounds) {
  if (!c) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  ISLECHK(nd_args_ok(c, "doc_near_duplicates", num, den, bands, rows_per_band));
  const uint64_t D = c->a_D;
  NdFound f;
  StreamDrain drain(c);
  ISLECHK(nd_find(c, num, den, bands, rows_per_band, f));
  if (parent_out && D) HIPCHK(c, hipMemcpyAsync(parent_out, f.parent.p, D * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  if (first_of_out && D) HIPCHK(c, hipMemcpyAsync(first_of_out, f.first_of.p, D * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (n_dropped) *n_dropped = D - f.kept;
  if (pairs_tested) *pairs_tested = f.pairs_tested;
  if (rounds) *rounds = f.rounds;
  return 0;
}

// For the ledger an ingest of the pruned matrix, as isle_hip_prune_docs: A_rewrite_begins is raised once every refusal is behind and the
// pruned matrix lies complete in the twin buffers, right before they are swapped in; install_A ends it.
extern "C" int isle_hip_prune_near_docs(isle_ctx* c, uint64_t num, uint64_t den, int bands, int rows_per_band, uint64_t* new_docs_out, uint32_t* kept_docs_out,
                                        uint32_t* parent_out, uint32_t* first_of_out, uint64_t* nnz_out, uint64_t* docs_global_out, uint64_t* n_dropped) {
  if (!c) return ISLE_E_ARG;
  ISLECHK(isle_enter(c));
  ISLECHK(nd_args_ok(c, "prune_near_docs", num, den, bands, rows_per_band));
  const uint64_t D = c->a_D;
  NdFound f;
  DevBuf<uint32_t> words, kept_docs, new_rows;
  DevBuf<uint64_t> tokens;
  DevBuf<float> new_cnt;
  DevBuf<int64_t> new_offs;
  StreamDrain drain(c);
  ISLECHK(nd_find(c, num, den, bands, rows_per_band, f));
  // ---- the pruned matrix out of place: the exact duplicates' compaction with these flags
  HIPCHK(c, words.reserve(D ? D : 1));
  HIPCHK(c, tokens.reserve(D ? D : 1));
  HIPCHK(c, kept_docs.reserve(D ? D : 1));
  ISLECHK(k_docs_len_hash(c, words.p, tokens.p, nullptr));
  uint64_t total = 0;
  ISLECHK(k_docs_compact(c, f.keep.p, words.p, f.kept, new_cnt, new_rows, new_offs, kept_docs.p, &total));
  if (kept_docs_out && f.kept) HIPCHK(c, hipMemcpyAsync(kept_docs_out, kept_docs.p, f.kept * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  if (parent_out && D) HIPCHK(c, hipMemcpyAsync(parent_out, f.parent.p, D * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  if (first_of_out && D) HIPCHK(c, hipMemcpyAsync(first_of_out, f.first_of.p, D * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  // ... and swapped in: the old buffers go with this call
  c->res.A_rewrite_begins();
  std::swap(c->a_cnt.p, new_cnt.p), std::swap(c->a_cnt.cap, new_cnt.cap);
  std::swap(c->a_rows.p, new_rows.p), std::swap(c->a_rows.cap, new_rows.cap);
  std::swap(c->a_offs.p, new_offs.p), std::swap(c->a_offs.cap, new_offs.cap);
  c->a_D = f.kept;
  c->a_nnz = total;
  if (new_docs_out) *new_docs_out = f.kept;
  if (docs_global_out) *docs_global_out = f.kept;
  if (n_dropped) *n_dropped = D - f.kept;
  return install_A(c, 0, f.kept, total, nullptr, nnz_out);
}
