"""Python binding of the C ABI (one object = one isle_ctx = one GPU).

Method names follow the reference methods they replace (ISLE::FPSparseMatrix<float>,
/root/reference include/sparseMatrix.h:242-466); see include/isle_hip.h for the contract.
numpy arrays in, numpy arrays out; all device work happens inside libisle_hip.so.
"""
import ctypes as C
import os

import numpy as np

from ._lib import IsleHipError, load_library

TIMING_FAMILIES = ["gram_pass1", "gram_pass2", "ortho", "qr", "evd", "rotate", "project", "kmpp", "lloyd_proj",
                   "sparse_assign", "sparse_update", "op_build", "comm", "threshold", "post", "ingest", "infer", "lift"]

BLOCK_KS_MAX_ITERS = 100      # include/hyperparams.h:38
BLOCK_KS_BLOCK_SIZE = 10      # include/hyperparams.h:39
BLOCK_KS_TOLERANCE = 1e-4     # include/hyperparams.h:40
MAX_KMEANS_LOWD_REPS = 10     # include/hyperparams.h:60
MAX_KMEANS_REPS = 10          # include/hyperparams.h:68


W0_C, EPS2_C, EPS3_C, RHO_C = 1.0, 1.0 / 3.0, 5.0, 1.1   # include/hyperparams.h:8-12


def catchword_rank(num_docs, num_topics, sample_rate=None):
    """The rank r that ISLETrainer::train passes to rth_highest_element (src/trainer.cpp:579-583): eps2_c * w0_c * num_docs
    (* sample_rate) / (2 num_topics), float operands in double arithmetic, floored."""
    x = EPS2_C * W0_C * float(np.float32(num_docs))
    if sample_rate is not None:
        x = x * float(np.float32(sample_rate))
    return int(np.floor(x / float(np.float32(2.0 * num_topics))))


def model_rank_threshold(num_docs, num_topics):
    """rank_threshold of SparseMatrix::construct_topic_model (src/sparseMatrix.cpp:720)."""
    return int(EPS3_C * W0_C * float(np.float32(num_docs)) / (float(np.float32(num_topics)) * 2.0))


EDGE_TOPIC_MIN_DOCS = 1            # include/hyperparams.h:77
EDGE_TOPIC_PRIMARY_RATIO = 0.7     # include/hyperparams.h:79


def select_edge_pairs(top1, top2, max_edge_topics, min_docs=EDGE_TOPIC_MIN_DOCS):
    """Pair selection of ISLETrainer::construct_edge_topics_v2 (src/trainer.cpp:1116-1145), the host half of the edge-topic stage as
    isle_amd/host/fpsparse_hip.h runs it: the documents' (top topic, second topic) pairs are counted, pairs with >= min_docs documents
    are candidates, the max_edge_topics most frequent are kept (ties in the count by (primary, secondary) ascending — the reference's
    sort is unstable there).  top1 / top2: int32 per document of A, -1 where the document has no such topic (construct_topic_model,
    src/sparseMatrix.cpp:687-708).  -> int64 (n, 3): primary, secondary, documents."""
    t1 = np.asarray(top1, np.int64)
    t2 = np.asarray(top2, np.int64)
    ok = (t1 >= 0) & (t2 >= 0)
    if not ok.any():
        return np.zeros((0, 3), np.int64)
    base = int(max(t1.max(), t2.max())) + 1
    key, cnt = np.unique(t1[ok] * base + t2[ok], return_counts=True)  # ascending (primary, secondary)
    keep = cnt >= min_docs
    key, cnt = key[keep], cnt[keep]
    order = np.argsort(-cnt, kind="stable")[:max(int(max_edge_topics), 0)]
    return np.stack([key[order] // base, key[order] % base, cnt[order]], axis=1).astype(np.int64)


DEFAULT_COHERENCE_EPS = 1e-5        # include/hyperparams.h:74
DEFAULT_COHERENCE_NUM_WORDS = 5     # include/hyperparams.h:75


def top_words(model, n, vocab_size=None):
    """The n heaviest words of every topic, heaviest first and the lower word id first among equal weights: the trainer's rule
    (DenseMatrix::find_n_top_words, src/denseMatrix.cpp:92-107, as isle_amd/host/trainer_hip.h applies it).  NaN weights (the topic
    vector of an empty cluster) sort last.  model: a (V, cols) array, e.g. the V x k topic model of construct_topic_model or the
    V x n edge model of edge_topics, or the same as a flat column-major buffer (get_basic_model / get_edge_model) with vocab_size
    given.  -> uint32 (cols, min(n, V)), the rows what HotPath.topic_coherence takes."""
    M = np.asarray(model)
    if M.ndim == 1:
        if vocab_size is None:
            raise ValueError("a flat model needs vocab_size")
        M = M.reshape(int(vocab_size), -1, order="F")
    if M.ndim != 2:
        raise ValueError("model must be (V, cols) or a flat column-major buffer")
    V, k = M.shape
    n = min(int(n), V)
    out = np.empty((k, n), np.uint32)
    if n == 0 or k == 0:
        return out
    W = np.where(np.isnan(M), -np.inf, M.astype(np.result_type(M.dtype, np.float32), copy=False))
    kth = np.partition(W, V - n, axis=0)[V - n]          # the n-th largest weight of every column
    for t in range(k):
        cand = np.flatnonzero(W[:, t] >= kth[t])          # ascending ids: every word that can be among the n
        order = np.lexsort((cand, -W[cand, t]))[:n]       # weight descending, then id ascending
        out[t] = cand[order]
    return out


TEXT_FORMATS = {"sparse": 0, "dense": 1}   # ISLE_TEXT_SPARSE, ISLE_TEXT_DENSE
_TEXT_SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.c_void_p)   # isle_text_sink_fn


def entry_text(w, format="dense"):
    """One model entry as the reference's writers print it (isle_hip_entry_text, the library's host copy of the digit rule its kernels
    compile): "sparse" -> the weight text, or "" for an entry the sparse writer skips (not w > 1e-8f); "dense" -> "0.0", "nan" or the
    weight text.  -1 for a printed entry outside the writer's domain (negative, infinite, >= 2^31).  No GPU needed."""
    buf = C.create_string_buffer(16)
    n = load_library().isle_hip_entry_text(C.c_float(float(np.float32(w))), TEXT_FORMATS[format], buf)
    return -1 if n < 0 else buf.raw[:n].decode("ascii")


DOC_TEXT_KINDS = {"entries": 0, "top": 1}   # ISLE_DOCTEXT_ENTRIES, ISLE_DOCTEXT_TOP


def doc_line_text(doc_number, topic_number, w):
    """One line "<doc>\\t<topic>\\t<weight>\\n" of the per-document topic files for the numbers as printed (isle_hip_doc_line_text, the
    host copy of what the kernels of infer_text.hip compile) -> bytes, or -1 outside the writers' domain (a number >= 0x7fffffff, a
    weight that is negative, NaN, infinite or >= 2^31).  No GPU needed."""
    buf = C.create_string_buffer(40)
    n = load_library().isle_hip_doc_line_text(int(doc_number), int(topic_number), C.c_float(float(np.float32(w))), buf)
    return -1 if n < 0 else buf.raw[:n]


DOC_REPORT_KINDS = {"catchwords": 0, "topic_sums": 1, "topic_sums_by_doc": 2, "top_two": 3}   # ISLE_DOCREPORT_*


def top_two_line_text(doc_number, t1_number, t2_number):
    """One line "<doc>\\t<top1>\\t<top2>\\n" of TopTwoTopicsPerDoc.txt for the numbers as printed (isle_hip_top_two_line_text, the host
    copy of what the kernels of doc_report.hip compile) -> bytes, or -1 for a number >= 0x7fffffff.  No GPU needed."""
    buf = C.create_string_buffer(40)
    n = load_library().isle_hip_top_two_line_text(int(doc_number), int(t1_number), int(t2_number), buf)
    return -1 if n < 0 else buf.raw[:n]


def parse_weight(token, format="sparse"):
    """One weight token of a model file as the library's readers take it (isle_hip_parse_weight, the host copy of the rule the loader's
    kernels compile): <digits>[.<digits>] -> np.float32; "nan" under "dense" -> the quiet NaN.  None for a token outside the grammar.
    No GPU needed."""
    raw = token if isinstance(token, bytes) else str(token).encode("ascii")
    out = C.c_float()
    rc = load_library().isle_hip_parse_weight(raw, len(raw), TEXT_FORMATS[format], C.byref(out))
    return None if rc else np.float32(out.value)


def score_total(v):
    """The corpus total of per-document values: the ascending sequential sum in double (isle_amd/csrc/score_host.h score_total), on the
    host through the library, so that Python and C++ get the same bits and shards side by side give the single-rank total."""
    v = np.ascontiguousarray(v, np.float64).reshape(-1)
    out = C.c_double(0.0)
    if load_library().isle_hip_score_total(_p(v) if v.size else None, int(v.size), C.byref(out)) != 0:
        raise IsleHipError("score_total: bad arguments")
    return float(out.value)


def _docs_mix(x):
    """docs_mix of isle_amd/csrc/docs_host.h (the finaliser of splitmix64) on a uint64 array."""
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def held_out_mask(docs, words, seed, num, den, doc_offset=0):
    """score_held_out of isle_amd/csrc/score_host.h for every (doc_offset + doc, word) -> bool array."""
    if not (int(den) >= 1 and 0 <= int(num) <= int(den)):
        raise ValueError("held-out share num / den: 0 <= num <= den, den >= 1")
    key = ((np.asarray(docs, np.uint64) + np.uint64(doc_offset)) << np.uint64(32)) | np.asarray(words, np.uint64)
    return _docs_mix(np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF) ^ key) % np.uint64(den) < np.uint64(num)


def split_held_out(counts, rows, offs, seed, num, den, doc_offset=0):
    """Splits a count matrix in CSC by entry for document completion: the entry (doc, word) is held out when
    docs_mix(seed ^ (((doc_offset + doc) << 32) | word)) % den < num (score_held_out, isle_amd/csrc/score_host.h).  The split is
    deterministic and does not depend on how the documents are sharded: doc_offset is the shard's first document in the corpus.
    -> ((counts, rows, offs) observed, (counts, rows, offs) held), both in the input's order."""
    counts = np.ascontiguousarray(counts, np.float32)
    rows = _as_u32(rows, "rows")
    offs = np.ascontiguousarray(offs, np.int64)
    D = offs.size - 1
    doc = np.repeat(np.arange(D, dtype=np.uint64), np.diff(offs))
    held = held_out_mask(doc, rows, seed, num, den, doc_offset)

    def part(m):
        o = np.zeros(D + 1, np.int64)
        np.cumsum(np.bincount(doc[m].astype(np.int64), minlength=D), out=o[1:])
        return counts[m], rows[m], o

    return part(~held), part(held)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _as_u32(a, name):
    """A flat contiguous uint32 array holding exactly the values of `a`, or ValueError: nothing is wrapped or truncated."""
    a = np.asarray(a)
    if a.ndim != 1:
        a = a.reshape(-1)
    if a.dtype == np.uint32:
        return np.ascontiguousarray(a)
    if a.size == 0:
        return np.empty(0, np.uint32)
    if a.dtype.kind not in "iubf":
        raise ValueError("%s: not an array of numbers" % name)
    if a.dtype.kind == "f" and not np.all(a == np.floor(a)):   # (NaN and infinities fail here or below)
        raise ValueError("%s holds a value that is not a whole number" % name)
    if a.min() < 0 or a.max() > 0xFFFFFFFF:
        raise ValueError("%s holds a value outside 0 .. 4294967295" % name)
    return np.ascontiguousarray(a.astype(np.uint32))


class HotPath:
    def __init__(self, device=0):
        self._lib = load_library()
        self._h = self._lib.isle_hip_create(device)
        if not self._h:
            raise IsleHipError("isle_hip_create(%d) failed: no usable HIP device (no CPU fallback exists)" % device)
        self.V = self.D = self.nnz = 0
        self.doc_offset = 0

    def close(self):
        if getattr(self, "_h", None):
            self._lib.isle_hip_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, allow=()):
        if rc != 0 and rc not in allow:
            raise IsleHipError("isle_hip error %d: %s" % (rc, self._lib.isle_hip_last_error(self._h).decode()))
        return rc

    # ---- multi-GPU ------------------------------------------------------------------------
    @staticmethod
    def comm_unique_id():
        buf = np.zeros(128, np.uint8)
        rc = load_library().isle_hip_comm_unique_id(_p(buf))
        if rc != 0:
            raise IsleHipError("ncclGetUniqueId failed")
        return buf

    def comm_init(self, world, rank, uid):
        uid = np.ascontiguousarray(uid, np.uint8)
        self._chk(self._lib.isle_hip_comm_init(self._h, world, rank, _p(uid)))
        self._world, self._rank = int(world), int(rank)

    def comm_init_host(self, world, rank, exchange):
        """Rehearsal transport (tests only; include/isle_hip.h): every collective is staged through host memory and
        handed to exchange(kind, array, count) -> None, which must complete it in place.  kind: 0 all-reduce sum,
        1 all-reduce max, 2 all-gather (array has world * count elements, this rank's part filled in)."""
        dts = [np.float32, np.float64, np.int32, np.uint32, np.uint64]

        def tramp(user, kind, buf, count, dtype):
            try:
                n = count * (world if kind == 2 else 1)
                dt = np.dtype(dts[dtype])
                a = np.frombuffer((C.c_char * (n * dt.itemsize)).from_address(buf), dtype=dt)
                exchange(kind, a, count)
                return 0
            except Exception as e:  # never let an exception cross the C boundary
                import traceback
                traceback.print_exc()
                return 1

        self._xchg_cb = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_int)(tramp)
        self._chk(self._lib.isle_hip_comm_init_host(self._h, world, rank, C.cast(self._xchg_cb, C.c_void_p), None))
        self._world, self._rank = int(world), int(rank)

    @staticmethod
    def gloo_exchange(dist, world, rank):
        """exchange function for comm_init_host over an initialised torch.distributed (gloo) process group."""
        import torch

        def exchange(kind, a, count):
            if kind == 2:
                # all-gather: a.view(world, count), own row filled; gloo has no unsigned types -> move the bytes
                t = torch.from_numpy(a.view(np.uint8).reshape(world, -1))
                parts = [torch.empty_like(t[0]) for _ in range(world)]
                dist.all_gather(parts, t[rank].clone())
                for r in range(world):
                    t[r].copy_(parts[r])
                return
            signed = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype)
            t = torch.from_numpy(a.view(signed) if signed else a)
            dist.all_reduce(t, op=dist.ReduceOp.MAX if kind == 1 else dist.ReduceOp.SUM)
        return exchange

    @staticmethod
    def plan_shards(offs, parts):
        offs = np.ascontiguousarray(offs, np.int64)
        bounds = np.zeros(parts + 1, np.uint64)
        rc = load_library().isle_hip_plan_shards(offs.shape[0] - 1, _p(offs), parts, _p(bounds))
        if rc != 0:
            raise IsleHipError("plan_shards failed")
        return bounds

    # ---- input ----------------------------------------------------------------------------
    def upload_csc(self, V, vals, rows, offs, doc_offset=0, docs_global=0):
        vals = np.ascontiguousarray(vals, np.float32)
        offs = np.ascontiguousarray(offs, np.int64)
        D = offs.shape[0] - 1
        nnz = int(offs[-1])
        if rows.dtype == np.uint64:
            rows = np.ascontiguousarray(rows)
            fn = self._lib.isle_hip_upload_csc_u64
        else:
            rows = np.ascontiguousarray(rows, np.uint32)
            fn = self._lib.isle_hip_upload_csc_u32
        self._chk(fn(self._h, V, D, nnz, _p(vals), _p(rows), _p(offs), doc_offset, docs_global))
        self.V, self.D, self.nnz, self.doc_offset = int(V), D, nnz, int(doc_offset)
        self.D_global = int(docs_global) if docs_global else D

    # ---- upstream stage: thresholding on the device ---------------------------------------
    def upload_counts(self, V, counts, rows, offs, doc_offset=0, docs_global=0):
        """A = word-document counts in CSC (SparseMatrix::populate_CSC, src/sparseMatrix.cpp:58-133)."""
        counts = np.ascontiguousarray(counts, np.float32)
        rows = np.ascontiguousarray(rows, np.uint32)
        offs = np.ascontiguousarray(offs, np.int64)
        D = offs.shape[0] - 1
        self._chk(self._lib.isle_hip_upload_counts_u32(self._h, V, D, int(offs[-1]), _p(counts), _p(rows), _p(offs),
                                                       doc_offset, docs_global))
        self._a_shape = (int(V), D, int(offs[-1]))

    @property
    def a_doc_offset(self):
        """The number in the corpus of the first document of the resident count matrix A (upload_counts / feed_finalize / the sharded
        tdf ingest); read from the context.  Separate from doc_offset, which is B's first column."""
        off = C.c_uint64()
        self._chk(self._lib.isle_hip_counts_shape(self._h, None, None, None, C.byref(off), None))
        return int(off.value)

    def ingest_tdf(self, text, vocab_size, num_docs, max_entries=0):
        """tdf text (bytes) -> the context's count matrix A, on the device (include/utils.h:158-228,
        src/trainer.cpp:236-247, src/sparseMatrix.cpp:58-87).  -> dict(entries_read, nnz)."""
        buf = np.frombuffer(text, dtype=np.uint8) if not isinstance(text, np.ndarray) else text
        nr, nz = C.c_uint64(), C.c_uint64()
        self._chk(self._lib.isle_hip_ingest_tdf(self._h, _p(buf) if buf.size else None, int(buf.size), int(vocab_size), int(num_docs),
                                                int(max_entries), C.byref(nr), C.byref(nz)))
        self._a_shape = (int(vocab_size), int(num_docs), int(nz.value))
        return dict(entries_read=int(nr.value), nnz=int(nz.value))

    # ---- (doc, word, count) triples in batches -> A (isle_hip_feed_*) -----------------------
    def feed_begin(self, vocab_size, num_docs, reserve_entries=0):
        """Opens a feed for a vocab_size x num_docs count matrix (an open one is discarded; the current A stays until feed_finalize)."""
        self._chk(self._lib.isle_hip_feed_begin(self._h, int(vocab_size), int(num_docs), int(reserve_entries)))
        self._feed_shape = (int(vocab_size), int(num_docs))

    def feed(self, docs, words, counts, _piece_entries=0):
        """One batch of entries in any order: 0-based local columns, 0-based word ids, counts (anything np.asarray accepts).  Zero counts
        are skipped; a value that is negative, not whole or above 2^32 - 1 raises ValueError (nothing is wrapped).  _piece_entries (tests): the
        size of the pieces the library cuts the batch into, 0 = its own (isle_hip_feed_entries_pieces)."""
        arrs = [_as_u32(a, name) for a, name in ((docs, "docs"), (words, "words"), (counts, "counts"))]
        if not (arrs[0].shape == arrs[1].shape == arrs[2].shape):
            raise ValueError("docs, words and counts differ in length")
        n = int(arrs[0].size)
        self._chk(self._lib.isle_hip_feed_entries_pieces(self._h, n, *(_p(a) if n else None for a in arrs), int(_piece_entries)))

    def feed_finalize(self, doc_offset=0, docs_global=0):
        """Sorts by (doc, word), keeps the first fed of equal pairs, builds the offsets: the result is the context's count matrix as after
        upload_counts with the same doc_offset / docs_global.  -> (entries_fed, nnz)."""
        fed, nz = C.c_uint64(), C.c_uint64()
        self._chk(self._lib.isle_hip_feed_finalize(self._h, int(doc_offset), int(docs_global), C.byref(fed), C.byref(nz)))
        self._a_shape = self._feed_shape + (int(nz.value),)
        return int(fed.value), int(nz.value)

    # ---- tdf text in pieces cut anywhere -> A (isle_hip_tdf_*) -------------------------------
    def tdf_begin(self, vocab_size, num_docs, reserve_entries=0, _piece_bytes=0):
        """Opens a text stream for a vocab_size x num_docs count matrix (an open stream or feed is discarded; the current A stays until
        tdf_finalize succeeds).  _piece_bytes (tests): the size of the pieces the text travels in, 0 = the library's own."""
        self._chk(self._lib.isle_hip_tdf_begin(self._h, int(vocab_size), int(num_docs), int(reserve_entries), int(_piece_bytes)))
        self._feed_shape = (int(vocab_size), int(num_docs))

    def tdf_write(self, data):
        """The next bytes of the text (bytes, bytearray, memoryview or a uint8 array), cut anywhere.  The first bad line of the text so far
        raises here or in tdf_finalize, whichever learns of it first; the stream is gone then."""
        if isinstance(data, np.ndarray):
            if data.dtype != np.uint8:
                raise ValueError("tdf_write takes bytes: a uint8 array, not %s (nothing is cast)" % data.dtype)
            buf = np.ascontiguousarray(data)
        else:
            buf = np.frombuffer(data, dtype=np.uint8)
        self._chk(self._lib.isle_hip_tdf_write(self._h, _p(buf) if buf.size else None, int(buf.size)))

    def tdf_finalize(self, max_entries=0):
        """-> dict(entries_read, nnz); the context's count matrix is what ingest_tdf of all the bytes written would have made it."""
        nr, nz = C.c_uint64(), C.c_uint64()
        self._chk(self._lib.isle_hip_tdf_finalize(self._h, int(max_entries), C.byref(nr), C.byref(nz)))
        self._a_shape = self._feed_shape + (int(nz.value),)
        return dict(entries_read=int(nr.value), nnz=int(nz.value))

    def _pump(self, f, b=0, e=None):
        """The open file f (unbuffered) into the open text stream, read straight into the stream's page-locked buffers (readinto, no copy in
        between).  With e: the lines of the byte range [b, e) only, those whose first byte s has b <= s < e (the rule of tdf_pump::file_range,
        isle_amd/host/tdf_pump.h): with b > 0 the bytes through the first newline at or after b - 1 are another range's, and the last line ends
        with the first newline at a position >= e - 1 or with the file.  -> bytes committed."""
        if e is not None and b >= e:
            return 0
        left, at = b"", b
        if e is not None and b > 0:
            f.seek(b - 1)
            pos = b - 1
            while True:
                chunk = f.read(4096)
                if not chunk:
                    return 0                    # the file ends inside the line that began before b
                i = chunk.find(b"\n")
                if i >= 0:
                    at, left = pos + i + 1, chunk[i + 1:]
                    break
                pos += len(chunk)
            if at >= e:
                return 0
        buf, cap = C.c_void_p(), C.c_uint64()
        total, done = 0, False
        while not done:
            self._chk(self._lib.isle_hip_tdf_acquire(self._h, C.byref(buf), C.byref(cap)))
            got = 0
            try:
                view = memoryview((C.c_char * cap.value).from_address(buf.value)).cast("B")
                while got < cap.value and not done:      # a read may return fewer bytes than asked for; only 0 is the end of the file
                    if left:
                        r = min(len(left), cap.value - got)
                        view[got:got + r] = left[:r]
                        left = left[r:]
                    else:
                        r = f.readinto(view[got:])
                        if not r:
                            done = True
                            break
                    if e is not None:
                        start = got + max(e - 1 - at, 0)  # of these r bytes, the first that may be the closing newline
                        nl = bytes(view[start:got + r]).find(b"\n") if start < got + r else -1
                        if nl >= 0:
                            r, done = start + nl + 1 - got, True
                    got += r
                    at += r
                del view
            except BaseException:           # a read error: the buffer goes back; the stream stays open until the next begin discards it
                self._lib.isle_hip_tdf_commit(self._h, 0)
                raise
            self._chk(self._lib.isle_hip_tdf_commit(self._h, got))
            total += got
        return total

    def ingest_tdf_file(self, path, vocab_size, num_docs, max_entries=0, _piece_bytes=0):
        """ingest_tdf of a file's bytes without holding them: the file is read straight into the stream's page-locked buffers (readinto,
        no copy in between), piece by piece, each piece parsed on the device while the next is read.  -> dict(entries_read, nnz).
        A file that cannot be opened opens no stream; after a read error the stream stays open, holding what was read, until the next
        tdf_begin or feed_begin discards it."""
        with open(path, "rb", buffering=0) as f:      # before tdf_begin: a file that is not there opens no stream and discards no feed
            self.tdf_begin(vocab_size, num_docs, _piece_bytes=_piece_bytes)
            self._pump(f)
        return self.tdf_finalize(max_entries)

    # ---- one tdf file onto document shards: counting stream and plan (pass 1), windowed stream (pass 2) --------------------------------
    def tdf_begin_counts(self, vocab_size, num_docs, _piece_bytes=0):
        """Opens a text stream that counts the valid lines per document and holds no entry (isle_hip_tdf_begin_counts); tdf_write feeds it."""
        self._chk(self._lib.isle_hip_tdf_begin_counts(self._h, int(vocab_size), int(num_docs), int(_piece_bytes)))
        self._feed_shape = (int(vocab_size), int(num_docs))

    def tdf_finalize_counts(self, parts, agree_tag=0, fetch_doc_lines=False):
        """Ends the counting stream; collective under a communicator (agree_tag, the file's size, must be alike on all ranks).
        -> dict(bounds (parts + 1, int64: shard p holds documents bounds[p] .. bounds[p + 1], balanced by lines), lines_local, lines_global,
        doc_lines (uint32 per document over all ranks, or None))."""
        bounds = np.zeros(int(parts) + 1, np.uint64)
        doc_lines = np.zeros(self._feed_shape[1], np.uint32) if fetch_doc_lines else None
        ll, lg = C.c_uint64(), C.c_uint64()
        self._chk(self._lib.isle_hip_tdf_finalize_counts(self._h, int(parts), int(agree_tag), _p(bounds), _p(doc_lines) if fetch_doc_lines else None,
                                                         C.byref(ll), C.byref(lg)))
        return dict(bounds=bounds.astype(np.int64), lines_local=int(ll.value), lines_global=int(lg.value), doc_lines=doc_lines)

    def tdf_begin_window(self, vocab_size, num_docs, doc_begin, doc_end, reserve_entries=0, _piece_bytes=0):
        """Opens a text stream over the whole text that keeps the entries of documents doc_begin <= doc < doc_end (0-based) only
        (isle_hip_tdf_begin_window); tdf_write feeds it, tdf_finalize ends it: A becomes those columns of what ingest_tdf gives."""
        self._chk(self._lib.isle_hip_tdf_begin_window(self._h, int(vocab_size), int(num_docs), int(doc_begin), int(doc_end), int(reserve_entries),
                                                      int(_piece_bytes)))
        self._feed_shape = (int(vocab_size), int(doc_end) - int(doc_begin))

    def ingest_tdf_file_sharded(self, path, vocab_size, num_docs, max_entries=0, parts=None, part=None, _piece_bytes=0):
        """One tdf file onto document shards in two passes, no rank holding the corpus.  Under a communicator parts = world and part =
        rank: pass 1 counts the lines per document over this rank's byte range of the file (collective), pass 2 streams the whole file and
        keeps the documents bounds[part] .. bounds[part + 1].  Without a communicator parts and part are given and pass 1 reads the whole
        file.  A becomes the shard, with its doc_offset and docs_global.  -> dict(bounds, entries_read, nnz, lines_local, lines_global)."""
        world = getattr(self, "_world", 1)
        rank = getattr(self, "_rank", 0)
        if world > 1:
            if parts not in (None, world) or part not in (None, rank):
                raise ValueError("under a communicator parts and part are the world size and the rank")
            parts, part = world, rank
        elif parts is None or part is None:
            raise ValueError("without a communicator parts and part must be given")
        if not 0 <= int(part) < int(parts):
            raise ValueError("part %r of %r" % (part, parts))
        with open(path, "rb", buffering=0) as f:
            size = os.fstat(f.fileno()).st_size
            self.tdf_begin_counts(vocab_size, num_docs, _piece_bytes=_piece_bytes)
            if world > 1:
                self._pump(f, size * rank // world, size * (rank + 1) // world)
            else:
                self._pump(f)
            plan = self.tdf_finalize_counts(parts, agree_tag=size)
            b = plan["bounds"]
            f.seek(0)
            self.tdf_begin_window(vocab_size, num_docs, b[part], b[part + 1], _piece_bytes=_piece_bytes)
            self._pump(f)
        res = self.tdf_finalize(max_entries)
        return dict(res, bounds=b, lines_local=plan["lines_local"], lines_global=plan["lines_global"])

    def upload_coo(self, V, D, docs, words, counts, batch=None):
        """feed_begin + feed + feed_finalize for triples held in arrays, fed in slices of `batch` entries (None: one call).
        -> (entries_fed, nnz)."""
        docs, words, counts = (_as_u32(a, name) for a, name in ((docs, "docs"), (words, "words"), (counts, "counts")))
        if not (docs.shape == words.shape == counts.shape):
            raise ValueError("docs, words and counts differ in length")
        n = int(docs.size)
        step = n if batch is None else int(batch)
        if batch is not None and step < 1:
            raise ValueError("batch must be positive")
        self.feed_begin(V, D, reserve_entries=n)
        for at in range(0, n, max(step, 1)):
            self.feed(docs[at:at + step], words[at:at + step], counts[at:at + step])
        return self.feed_finalize()

    def get_A(self):
        V, D, nnz = self._a_shape
        cnt, rows, offs = np.empty(nnz, np.float32), np.empty(nnz, np.uint32), np.empty(D + 1, np.int64)
        self._chk(self._lib.isle_hip_get_A(self._h, _p(cnt), _p(rows), _p(offs)))
        return cnt, rows, offs

    # ---- the vocabulary pruned by document frequency, on the resident A (include/isle_hip.h, isle_hip_prune_vocab) -----------------
    def _counts_shape(self):
        v = [C.c_uint64() for _ in range(5)]
        self._chk(self._lib.isle_hip_counts_shape(self._h, *(C.byref(x) for x in v)))
        return tuple(int(x.value) for x in v)

    def vocab_hist_form(self, form="auto"):
        """Which form of the document-frequency kernel this context asks for: "auto" (the library's rule), "lds" (workgroup-private
        counters in LDS, one atomic per (workgroup, word)) or "global" (one global atomic per entry).  Same integers either way."""
        self._chk(self._lib.isle_hip_vocab_hist_form(self._h, {"auto": 0, "lds": 1, "global": 2}[form]))

    def word_doc_freq(self):
        """df uint32 (vocab,): the documents of the whole corpus that hold each word of the resident count matrix.  Nothing resident
        changes.  Under comm_init / comm_init_host COLLECTIVE: every rank calls, a rank without documents included, and gets the
        corpus's table."""
        df = np.empty(self._counts_shape()[0], np.uint32)
        self._chk(self._lib.isle_hip_word_doc_freq(self._h, _p(df)))
        return df

    def prune_vocab(self, min_df=1, max_df=None, keep_n=None):
        """Drops the words of the resident count matrix A that occur in fewer than min_df or more than max_df documents of the corpus,
        and all but the keep_n most frequent of the rest (the larger df first, the smaller word id among equal df); the kept words are
        renumbered in ascending old id and A is compacted on the device (isle_hip_prune_vocab states the rule).  max_df: None = no upper
        bound; an int = that many documents; a float in (0, 1] = floor(max_df * docs_global) documents, docs_global the corpus's
        document count (a float of 1.0 is the whole corpus, the int 1 one document).  keep_n: None = no cap.
        For everything resident this is an ingest of the pruned matrix: run threshold() next.  A refusal (IsleHipError: min_df above
        max_df, no word kept, ...) leaves A as it was.  Under comm_init / comm_init_host COLLECTIVE, with the same arguments on every rank.
        -> dict(vocab, kept_words uint32 (vocab,): new id -> old id, df uint32 (old vocab,), nnz (this rank's), docs_emptied (the corpus's))."""
        V, _, _, _, docs_global = self._counts_shape()
        if max_df is None:
            top = 0
        elif isinstance(max_df, (float, np.floating)):
            if not 0.0 < max_df <= 1.0:
                raise ValueError("max_df: a float is a share of the corpus in (0, 1]")
            top = int(np.floor(float(max_df) * docs_global))
            if top == 0:
                raise ValueError("max_df = %r of %d documents is no document" % (max_df, docs_global))
        else:
            top = int(max_df)
            if top < 1:
                raise ValueError("max_df: at least 1 document (None: no upper bound)")
        keep = 0 if keep_n is None else int(keep_n)
        if int(min_df) < 0 or (keep_n is not None and keep < 1):
            raise ValueError("min_df >= 0 and keep_n >= 1 (None: no cap)")
        nv, nz, gone = C.c_uint64(), C.c_uint64(), C.c_uint64()
        kept, df = np.empty(V, np.uint32), np.empty(V, np.uint32)
        self._chk(self._lib.isle_hip_prune_vocab(self._h, int(min_df), top, keep, C.byref(nv), _p(kept), _p(df), C.byref(nz), C.byref(gone)))
        self._a_shape = self._counts_shape()[:3]
        return dict(vocab=int(nv.value), kept_words=kept[:int(nv.value)].copy(), df=df, nnz=int(nz.value), docs_emptied=int(gone.value))

    # ---- documents pruned by length and as exact duplicates, on the resident A (include/isle_hip.h, isle_hip_prune_docs) -----------
    def doc_hash_form(self, form="auto"):
        """Which key this context sorts documents by before it compares their contents: "auto" (the library's rule), "full" (the 64-bit
        document hash) or "narrow" (the same hash cut to 2 bits: every run holds many unequal documents).  Same result either way."""
        self._chk(self._lib.isle_hip_doc_hash_form(self._h, {"auto": 0, "full": 1, "narrow": 2}[form]))

    def doc_lengths(self):
        """(words uint32 (D,), tokens uint64 (D,)) of this rank's documents of the resident count matrix: the entries of each column and
        the sum of their counts, each truncated to an integer.  Nothing resident changes; never collective."""
        D = self._counts_shape()[1]
        words, tokens = np.empty(D, np.uint32), np.empty(D, np.uint64)
        self._chk(self._lib.isle_hip_doc_lengths(self._h, _p(words), _p(tokens)))
        return words, tokens

    def doc_duplicates(self):
        """dict(first_of uint32 (D,): the smallest document with the same column (rows and count bits) as each document, itself where it
        is the first of its kind; n_duplicates: the documents that are not).  Nothing resident changes.  One rank only: refused under a
        communicator of several ranks."""
        D = self._counts_shape()[1]
        first, n = np.empty(D, np.uint32), C.c_uint64()
        self._chk(self._lib.isle_hip_doc_duplicates(self._h, _p(first), C.byref(n)))
        return dict(first_of=first, n_duplicates=int(n.value))

    def prune_docs(self, min_words=1, max_words=None, min_tokens=0, max_tokens=None, drop_duplicates=False):
        """Drops the documents of the resident count matrix A with fewer than min_words or more than max_words entries, or with fewer
        than min_tokens or more than max_tokens tokens (None: no upper bound), and with drop_duplicates every document whose column
        equals an earlier one's bit for bit; the kept documents are renumbered in ascending old id and A is compacted on the device
        (isle_hip_prune_docs states the rule).  For everything resident this is an ingest of the pruned matrix: run threshold() next.
        A refusal (IsleHipError: a minimum above its maximum, no document kept, duplicates under several ranks, ...) leaves A as it
        was.  Under comm_init / comm_init_host COLLECTIVE without drop_duplicates, with the same arguments on every rank.
        -> dict(docs (this rank's), kept_docs uint32 (docs,): new id -> old number in the corpus, first_of uint32 (old docs,):
        0xffffffff where dropped by length, the representative where dropped as a duplicate, nnz (this rank's), docs_global,
        dropped_short, dropped_long, dropped_duplicate (the corpus's))."""
        top_w = 0 if max_words is None else int(max_words)
        top_t = 0 if max_tokens is None else int(max_tokens)
        if int(min_words) < 0 or int(min_tokens) < 0 or (max_words is not None and top_w < 1) or (max_tokens is not None and top_t < 1):
            raise ValueError("min_words >= 0, min_tokens >= 0, max_words >= 1 and max_tokens >= 1 (None: no upper bound)")
        D = self._counts_shape()[1]
        nd, nz, dg = C.c_uint64(), C.c_uint64(), C.c_uint64()
        kept, first, dropped = np.empty(max(D, 1), np.uint32), np.empty(max(D, 1), np.uint32), np.zeros(3, np.uint64)
        self._chk(self._lib.isle_hip_prune_docs(self._h, int(min_words), top_w, int(min_tokens), top_t, int(bool(drop_duplicates)), C.byref(nd), _p(kept),
                                                _p(first), C.byref(nz), C.byref(dg), _p(dropped)))
        self._a_shape = self._counts_shape()[:3]
        return dict(docs=int(nd.value), kept_docs=kept[:int(nd.value)].copy(), first_of=first[:D].copy(), nnz=int(nz.value), docs_global=int(dg.value),
                    dropped_short=int(dropped[0]), dropped_long=int(dropped[1]), dropped_duplicate=int(dropped[2]))

    # ---- near-duplicate documents by MinHash, on the resident A (include/isle_hip.h, isle_hip_prune_near_docs) -----------------------
    def neardup_key_form(self, form="auto"):
        """Which key this context sorts a band's live documents by before the exact Jaccard test: "auto" (the library's rule), "full"
        (the band's 64-bit key) or "narrow" (the same key cut to 2 bits: every group holds many dissimilar documents; for the tests).
        The form decides which pairs become candidates: with a threshold below 1 the two may answer differently."""
        self._chk(self._lib.isle_hip_neardup_key_form(self._h, {"auto": 0, "full": 1, "narrow": 2}[form]))

    @staticmethod
    def _neardup_threshold(threshold):
        """a float becomes Fraction(threshold).limit_denominator(1000), a (num, den) tuple is taken as it is -> (num, den)"""
        if isinstance(threshold, tuple):
            num, den = threshold
            return int(num), int(den)
        from fractions import Fraction
        f = Fraction(float(threshold)).limit_denominator(1000)
        return f.numerator, f.denominator

    def doc_signatures(self, bands=16, rows_per_band=4, sig=True, keys=True):
        """MinHash signatures and band keys of this rank's documents of the resident count matrix: dict(sig uint64 (D, bands *
        rows_per_band), keys uint64 (bands, D), not cut), each only where asked for.  Nothing resident changes."""
        D = self._counts_shape()[1]
        H = int(bands) * int(rows_per_band)
        ok = 1 <= int(bands) <= 64 and 1 <= int(rows_per_band) <= 8 and H <= 128     # (the library refuses by name; no buffer is sized from a refused shape)
        s = np.empty((D, H), np.uint64) if sig and ok else None
        k = np.empty((int(bands), D), np.uint64) if keys and ok else None
        self._chk(self._lib.isle_hip_doc_signatures(self._h, int(bands), int(rows_per_band), None if s is None else _p(s), None if k is None else _p(k)))
        out = {}
        if s is not None:
            out["sig"] = s
        if k is not None:
            out["keys"] = k
        return out

    def doc_jaccard(self, a, b):
        """(inter uint32 (n,), uni uint32 (n,)): the exact sizes of the intersection and the union of the word sets of the documents
        a[i] and b[i] of this rank (a[i] == b[i] allowed).  Nothing resident changes."""
        a, b = np.ascontiguousarray(a, np.uint32).reshape(-1), np.ascontiguousarray(b, np.uint32).reshape(-1)
        if a.size != b.size:
            raise ValueError("doc_jaccard: %d and %d documents" % (a.size, b.size))
        inter, uni = np.empty(a.size, np.uint32), np.empty(a.size, np.uint32)
        self._chk(self._lib.isle_hip_doc_jaccard(self._h, a.size, _p(a), _p(b), _p(inter), _p(uni)))
        return inter, uni

    def near_duplicates(self, threshold=0.8, bands=16, rows_per_band=4):
        """The documents of the resident count matrix whose word set has Jaccard similarity >= threshold with an earlier document's,
        found by MinHash banding and verified exactly (isle_hip_doc_near_duplicates states the rule).  threshold: a float (it becomes
        Fraction(threshold).limit_denominator(1000)) or a (num, den) tuple.  Nothing resident changes.  One rank only.
        -> dict(parent uint32 (D,): the verified neighbour, the document itself where it has none; first_of uint32 (D,): the root of
        the parent chain; n_dropped, pairs_tested, rounds, num, den)."""
        num, den = self._neardup_threshold(threshold)
        D = self._counts_shape()[1]
        parent, first = np.empty(D, np.uint32), np.empty(D, np.uint32)
        nd, pt, rd = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._chk(self._lib.isle_hip_doc_near_duplicates(self._h, num, den, int(bands), int(rows_per_band), _p(parent), _p(first), C.byref(nd), C.byref(pt),
                                                         C.byref(rd)))
        return dict(parent=parent, first_of=first, n_dropped=int(nd.value), pairs_tested=int(pt.value), rounds=int(rd.value), num=num, den=den)

    def prune_near_docs(self, threshold=0.8, bands=16, rows_per_band=4):
        """Drops every document of the resident count matrix A that near_duplicates attaches to an earlier one; the kept documents are
        renumbered in ascending old id and A is compacted on the device.  For everything resident this is an ingest of the pruned
        matrix: run threshold() next.  A refusal leaves A as it was.  One rank only.
        -> dict(docs, kept_docs uint32 (docs,): new id -> old number in the corpus, parent and first_of uint32 (old docs,), nnz,
        docs_global, n_dropped, num, den)."""
        num, den = self._neardup_threshold(threshold)
        D = self._counts_shape()[1]
        kept, parent, first = np.empty(max(D, 1), np.uint32), np.empty(max(D, 1), np.uint32), np.empty(max(D, 1), np.uint32)
        nd, nz, dg, gone = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._chk(self._lib.isle_hip_prune_near_docs(self._h, num, den, int(bands), int(rows_per_band), C.byref(nd), _p(kept), _p(parent), _p(first), C.byref(nz),
                                                     C.byref(dg), C.byref(gone)))
        self._a_shape = self._counts_shape()[:3]
        return dict(docs=int(nd.value), kept_docs=kept[:int(nd.value)].copy(), parent=parent[:D].copy(), first_of=first[:D].copy(), nnz=int(nz.value),
                    docs_global=int(dg.value), n_dropped=int(gone.value), num=num, den=den)

    def threshold(self, num_topics, sample_rate=0.0, sample_seed=0):
        """normalize_docs + compute_thresholds + (sampled_)threshold_and_copy on the device
        (src/trainer.cpp:430-485); B becomes this context's matrix.  Returns a dict of scalars."""
        dk, nk, ab = C.c_uint64(), C.c_uint64(), C.c_uint64()
        avg = C.c_float()
        self._chk(self._lib.isle_hip_threshold(self._h, int(num_topics), float(sample_rate), int(sample_seed),
                                               C.byref(dk), C.byref(nk), C.byref(ab), C.byref(avg)))
        V, D, nnz, off, glob = (C.c_uint64() for _ in range(5))
        self._chk(self._lib.isle_hip_shape(self._h, C.byref(V), C.byref(D), C.byref(nnz), C.byref(off), C.byref(glob)))
        self.V, self.D, self.nnz = int(V.value), int(D.value), int(nnz.value)
        self.doc_offset, self.D_global = int(off.value), int(glob.value)
        return dict(docs_kept=int(dk.value), nnz_kept=int(nk.value), entries_above_threshold=int(ab.value),
                    avg_doc_sz=float(avg.value))

    def shape(self):
        """(V, D, nnz, doc_offset, docs_global) of the context's B (isle_hip_shape)."""
        v = [C.c_uint64() for _ in range(5)]
        self._chk(self._lib.isle_hip_shape(self._h, *(C.byref(x) for x in v)))
        return tuple(int(x.value) for x in v)

    def get_B(self, with_threshold_outputs=True):
        """Host copy of the context's B: dict(V, D, nnz, vals, rows, offs[, original_cols, zetas])."""
        out = dict(V=self.V, D=self.D, nnz=self.nnz, vals=np.empty(self.nnz, np.float32), rows=np.empty(self.nnz, np.uint32),
                   offs=np.empty(self.D + 1, np.int64))
        oc = ze = None
        if with_threshold_outputs:
            oc = out["original_cols"] = np.empty(self.D, np.uint64)
            ze = out["zetas"] = np.empty(self.V, np.float32)
        self._chk(self._lib.isle_hip_get_B(self._h, _p(out["vals"]), _p(out["rows"]), _p(out["offs"]),
                                           _p(oc) if oc is not None else None, _p(ze) if ze is not None else None))
        return out

    # ---- downstream stage: catchwords, topic model, edge topics ---------------------------
    def find_catchwords(self, num_topics, r, assign=None, rho=1.1, fetch_thresholds=True):
        """rth_highest_element per topic + find_catchwords (src/trainer.cpp:586-627).
        -> dict(thresholds (V,k) F-order or None, catch_topic int32[V], num_catchwords).
        Under comm_init / comm_init_host the call is collective: every rank holds its documents of A (upload_counts with doc_offset /
        docs_global) and passes the same num_topics, r and rho; assign is the partition of the columns of B this rank kept (or the
        resident one).  All three results are replicated: those of the whole corpus, bit-identical on every rank."""
        V = self.V
        thr = np.empty((V, num_topics), np.float32, order="F") if fetch_thresholds else None
        ct = np.empty(V, np.int32)
        n = C.c_uint64()
        a = None if assign is None else np.ascontiguousarray(assign, np.uint32)
        self._chk(self._lib.isle_hip_catchwords(self._h, int(num_topics), _p(a), int(r), float(rho), _p(thr), _p(ct), C.byref(n)))
        self._post_k = int(num_topics)
        return dict(thresholds=thr, catch_topic=ct, num_catchwords=int(n.value))

    def construct_topic_model(self, num_topics, rank_threshold, num_docs_A, fetch_sums=True):
        """SparseMatrix::construct_topic_model (src/sparseMatrix.cpp:597-838) on the device.
        Under comm_init / comm_init_host the call is collective (the same num_topics and rank_threshold on every rank) and num_docs_A is
        the rank's own document count.  model and model_threshold are replicated: the whole corpus's, bit-identical on every rank.
        top1 / top2, dts_off / dts_topic / dts_val and num_sums are the shard's: the rank's own documents, numbered from 0."""
        V = self.V
        M = np.empty((V, num_topics), np.float32, order="F")
        mt = np.empty(num_topics, np.float32)
        t1 = np.empty(num_docs_A, np.int32)
        t2 = np.empty(num_docs_A, np.int32)
        n = C.c_uint64()
        self._chk(self._lib.isle_hip_topic_model(self._h, int(num_topics), int(rank_threshold), _p(M), _p(mt), _p(t1), _p(t2), C.byref(n)))
        out = dict(model=M, model_threshold=mt, top1=t1, top2=t2, num_sums=int(n.value))
        if fetch_sums:
            off = np.empty(num_docs_A + 1, np.int64)
            tp = np.empty(out["num_sums"], np.uint32)
            va = np.empty(out["num_sums"], np.float32)
            self._chk(self._lib.isle_hip_get_doc_topic_sums(self._h, _p(off), _p(tp), _p(va)))
            out.update(dts_off=off, dts_topic=tp, dts_val=va)
        return out

    def edge_topics(self, pairs, primary_ratio=0.7):
        """FPaxpy pair of construct_edge_topics_v2 (src/trainer.cpp:1152-1159): pairs (n,2) -> (V,n) F-order."""
        pairs = np.ascontiguousarray(pairs, np.int64).reshape(-1, 2)
        n = pairs.shape[0]
        E = np.empty((self.V, n), np.float32, order="F")
        self._chk(self._lib.isle_hip_edge_topics(self._h, _p(pairs), n, float(primary_ratio), _p(E)))
        return E

    def select_edge_pairs(self, max_edge_topics, min_docs=EDGE_TOPIC_MIN_DOCS, top1=None, top2=None, num_topics=None):
        """select_edge_pairs() on the device (isle_hip_select_edge_pairs), bit-equal to it: over the resident top-two topics of the last
        construct_topic_model (top1 and top2 None; nothing is fetched), or over the given int32 arrays with num_topics given (every id in
        -1 .. num_topics - 1).  -> (int64 (n, 3): primary, secondary, documents; dict(candidates, threshold)), threshold the count of
        the first candidate cut off, None when nothing was cut.
        Under comm_init / comm_init_host the call is collective: the resident form counts the documents of the rank's shard, the other
        form takes the top topics of the rank's own documents; the pair counts are summed over the ranks and every rank returns the
        same selection, that of the whole corpus (replicated)."""
        if top1 is None and top2 is None:
            docs = getattr(self, "_a_shape", (0, 0))[1]
            k = getattr(self, "_post_k", 0) if num_topics is None else int(num_topics)
            t1 = t2 = None
        else:
            if num_topics is None:
                raise ValueError("num_topics is needed with top1 / top2")
            t1 = None if top1 is None else np.ascontiguousarray(top1, np.int32).reshape(-1)
            t2 = None if top2 is None else np.ascontiguousarray(top2, np.int32).reshape(-1)
            if t1 is not None and t2 is not None and t1.size != t2.size:
                raise ValueError("top1 and top2 differ in length")
            docs = int((t1 if t1 is not None else t2).size)
            k = int(num_topics)
        # (several ranks: the candidates are those of all ranks' documents, so this rank's count is no bound on them)
        cap = max(min(int(max_edge_topics), k * k), 0)
        if getattr(self, "_world", 1) <= 1:
            cap = min(cap, docs)
        pairs = np.empty((cap, 3), np.int64)
        nsel, ncand, thr = C.c_uint64(), C.c_uint64(), C.c_uint64()
        # (an empty array still hands the library a non-null pointer: which of top1 / top2 was given is what it sees)
        one = np.zeros(1, np.int32)
        self._chk(self._lib.isle_hip_select_edge_pairs(self._h, None if t1 is None else _p(t1 if t1.size else one),
                                                       None if t2 is None else _p(t2 if t2.size else one), docs, k, int(max_edge_topics),
                                                       int(min_docs), _p(pairs) if cap else None, cap, C.byref(nsel), C.byref(ncand), C.byref(thr)))
        n = int(nsel.value)
        cut = int(ncand.value) > n
        return pairs[:n], dict(candidates=int(ncand.value), threshold=int(thr.value) if cut else None)

    def edge_top_words(self, pairs, n, primary_ratio=EDGE_TOPIC_PRIMARY_RATIO, model="catch"):
        """The n heaviest words of the edge topics primary_ratio * M[:, p] + (1 - primary_ratio) * M[:, s], by the rule of top_words()
        and with the entries of edge_topics() (bit-equal to both), formed on the device from the model's two columns: no (V, n_edge)
        matrix exists anywhere.  pairs: (n_edge, 2) or the (n_edge, 3) of select_edge_pairs; model as in model_top_words.
        -> (ids uint32 (n_edge, n), weights float32 (n_edge, n))."""
        pairs = np.asarray(pairs, np.int64)
        if pairs.ndim != 2 or pairs.shape[1] not in (2, 3):
            pairs = pairs.reshape(-1, 2)
        pq = np.ascontiguousarray(pairs[:, :2])
        ne = pq.shape[0]
        if isinstance(model, str):
            which, host = self._MODELS[model], None
            V, cols = self._resident_shape(model)
        else:
            host = np.asfortranarray(model, np.float32)
            if host.ndim != 2:
                raise ValueError("model must be (V, cols)")
            which, (V, cols) = 2, host.shape
        ids = np.empty((ne, int(n)), np.uint32)
        w = np.empty((ne, int(n)), np.float32)
        self._chk(self._lib.isle_hip_edge_top_words(self._h, which, _p(host), int(V), int(cols), _p(pq) if ne else None, ne, float(primary_ratio),
                                                    int(n), _p(ids), _p(w)))
        return ids, w

    def topic_coherence(self, top_words, eps=DEFAULT_COHERENCE_EPS, fetch_counts=True):
        """UMass coherence of each topic's top words over the count matrix A (SparseMatrix::topic_coherence,
        src/sparseMatrix.cpp:841-1016; the formula, the NaN rule and the deviations: include/isle_hip.h).  top_words: (num_topics, M)
        word ids, heaviest first (see top_words()).  -> dict(coherence float64 (num_topics,), doc_freq uint64 (num_topics, M),
        co_doc_freq uint64 (num_topics, M(M-1)/2) with (i, j) at i(i-1)/2 + j); the two count arrays are None without fetch_counts."""
        tw = np.ascontiguousarray(top_words, np.uint32)
        if tw.ndim != 2:
            raise ValueError("top_words must be (num_topics, M)")
        n, M = tw.shape
        coh = np.empty(n, np.float64)
        df = np.empty((n, M), np.uint64) if fetch_counts else None
        co = np.empty((n, max(M * (M - 1) // 2, 0)), np.uint64) if fetch_counts else None
        self._chk(self._lib.isle_hip_topic_coherence(self._h, n, M, _p(tw), float(eps), _p(coh), _p(df), _p(co)))
        return dict(coherence=coh, doc_freq=df, co_doc_freq=co)

    # ---- the cluster-average model and what reads a model (include/isle_hip.h for the rules and the deviations) -----------------
    _MODELS = {"catch": 0, "avg": 1, "loaded": 3}   # ISLE_MODEL_CATCH, ISLE_MODEL_AVG, ISLE_MODEL_LOADED; ISLE_MODEL_HOST = 2

    def _a_vocab(self):
        return getattr(self, "_a_shape", (self.V,))[0]

    def _resident_shape(self, model):
        """(V, cols) of the resident model a name stands for: the loaded model's own, else V of A and the topics of the last pass."""
        if model == "loaded":
            V, cols = C.c_uint64(), C.c_int()
            self._chk(self._lib.isle_hip_get_loaded_model(self._h, None, C.byref(V), C.byref(cols)))   # refused when nothing is loaded
            return int(V.value), int(cols.value)
        return self._a_vocab(), getattr(self, "_post_k", 0)

    # ---- model files read back on the device (include/isle_hip.h for the rule, the deviations and the errors) ----------------------
    def load_model_text(self, text, vocab, cols, format="sparse", base=1):
        """The text of a model file (bytes; "sparse": "<topic> <word> <weight>" lines with ids minus base, "dense": one line per
        column) parsed on the device into the resident model "loaded", which model_top_words, topic_diversity, model_text /
        write_model / model_text_size and infer_resident take as model="loaded".  It is independent of A and of the other resident
        models and lives until the next successful load.  A refused text (IsleHipError naming the first offending line and the kind
        of error) leaves the previous model in place.  Under comm_init / comm_init_host: no collective, each rank loads for itself.
        -> entries read (sparse: lines, dense: vocab x cols)."""
        buf = np.frombuffer(text, dtype=np.uint8) if not isinstance(text, np.ndarray) else text
        fmt = TEXT_FORMATS[format] if isinstance(format, str) else int(format)
        n = C.c_uint64()
        self._chk(self._lib.isle_hip_load_model_text(self._h, _p(buf) if buf.size else None, int(buf.size), int(vocab), int(cols), fmt, int(base),
                                                     C.byref(n)))
        return int(n.value)

    def load_model(self, path, vocab, cols, format="sparse", base=1):
        """load_model_text of a file."""
        return self.load_model_text(np.fromfile(path, dtype=np.uint8), vocab, cols, format, base)

    def loaded_model(self):
        """The resident loaded model -> (V, cols) F-order float32."""
        M = np.empty(self._resident_shape("loaded"), np.float32, order="F")
        self._chk(self._lib.isle_hip_get_loaded_model(self._h, _p(M), None, None))
        return M

    def avg_topic_model(self, num_topics, fetch=True):
        """The cluster-average topic model (ISLETrainer::output_avg_topic_coherence, src/trainer.cpp:705-745): every topic the
        L1-normalised sum of its cluster's normalised documents, no catchwords; after find_catchwords(num_topics).  Exact sums,
        bitwise reproducible, NaN columns for empty clusters.  The model stays resident.  -> (V, num_topics) F-order float32, or None."""
        M = np.empty((self._a_vocab(), int(num_topics)), np.float32, order="F") if fetch else None
        self._chk(self._lib.isle_hip_avg_topic_model(self._h, int(num_topics), _p(M)))
        return M

    def model_top_words(self, n=10, model="catch", with_weights=False):
        """The n heaviest words of every topic, on the device, by the rule of top_words() (bit-equal to it).  model: "catch" (the
        resident topic model), "avg" (the resident average model), "loaded" (the model of load_model_text) or a (V, cols) array.  -> uint32 (cols, n), and float32 (cols, n)
        weights with with_weights."""
        if isinstance(model, str):
            which, host = self._MODELS[model], None
            V, cols = self._resident_shape(model)
        else:
            host = np.asfortranarray(model, np.float32)
            if host.ndim != 2:
                raise ValueError("model must be (V, cols)")
            which, (V, cols) = 2, host.shape
        ids = np.empty((cols, int(n)), np.uint32)
        w = np.empty((cols, int(n)), np.float32) if with_weights else None
        self._chk(self._lib.isle_hip_model_top_words(self._h, which, _p(host), int(V), int(cols), int(n), _p(ids), _p(w)))
        return (ids, w) if with_weights else ids

    # ---- two models compared: L1 distances and topic matching (include/isle_hip.h, isle_hip_compare_models) ------------------------
    def _model_side(self, model):
        """-> (which, host array or None, V, cols) of a model named as in model_top_words"""
        if isinstance(model, str):
            V, cols = self._resident_shape(model)
            return self._MODELS[model], None, V, cols
        host = np.asfortranarray(model, np.float32)
        if host.ndim != 2:
            raise ValueError("model must be (V, cols)")
        return 2, host, host.shape[0], host.shape[1]

    @staticmethod
    def _match_outputs(na, nb):
        ok = 1 <= na <= 8192 and 1 <= nb <= 8192       # beyond: the library refuses before it writes
        return (np.empty(na if ok else 1, np.int32), np.empty(nb if ok else 1, np.int32), np.empty(na if ok else 1, np.float64), C.c_uint64(), C.c_double(),
                C.c_uint32())

    def model_dist_slices(self, n=0):
        """How many word slices this context's distance kernel cuts the vocabulary into: 0 (the library's rule) or n >= 1 (capped at
        ceil(V / 64)).  With exactly representable sums the same bits either way; otherwise the order of summation follows it."""
        self._chk(self._lib.isle_hip_model_dist_slices(self._h, int(n)))

    def compare_models(self, a="catch", b="loaded", fetch_dist=True, match=True):
        """The L1 distance of every topic of model a to every topic of model b, in double on the device, and the greedy matching of the
        topics by it (isle_hip_compare_models states the rule).  Each side: "catch", "avg", "loaded" or a (V, cols) array; both may be
        arrays, both may name the same model.  A column with a non-finite entry (an empty cluster's in "avg") gives NaN distances and
        stays unmatched.  Nothing resident changes; under comm_init / comm_init_host each rank answers for itself ("avg" is refused).
        -> dict(dist float64 (cols_a, cols_b) or None, match_a int32 (cols_a,): the matched topic of b or -1, match_b int32 (cols_b,),
        match_dist float64 (cols_a,): NaN where unmatched, n_matched, mean_dist, rounds); the match entries are None without match."""
        wa, ha, Va, ka = self._model_side(a)
        wb, hb, Vb, kb = self._model_side(b)
        if ha is not None and hb is not None and Va != Vb:
            raise ValueError("the two models have %d and %d words" % (Va, Vb))
        V = Vb if ha is None and hb is not None else Va
        ok = 1 <= ka <= 8192 and 1 <= kb <= 8192
        dist = np.empty((ka, kb) if ok else (1, 1), np.float64) if fetch_dist else None
        ma, mb, md, n, mean, rounds = self._match_outputs(ka, kb)
        if not match:
            ma = mb = md = None
        self._chk(self._lib.isle_hip_compare_models(self._h, wa, _p(ha), int(ka), wb, _p(hb), int(kb), int(V), _p(dist), _p(ma), _p(mb), _p(md),
                                                    C.byref(n) if match else None, C.byref(mean) if match else None, C.byref(rounds)))
        return dict(dist=dist, match_a=ma, match_b=mb, match_dist=md, n_matched=int(n.value) if match else None,
                    mean_dist=float(mean.value) if match else None, rounds=int(rounds.value))

    def match_topics(self, dist):
        """The greedy matching of the rows and columns of a (na, nb) float64 matrix on the device, by the rule of compare_models: an
        edge where the entry is finite, edges in the order (value, row, column).  -> dict(match_a, match_b, match_dist, n_matched,
        mean_dist, rounds)."""
        d = np.ascontiguousarray(dist, np.float64)
        if d.ndim != 2:
            raise ValueError("dist must be (na, nb)")
        na, nb = d.shape
        ma, mb, md, n, mean, rounds = self._match_outputs(na, nb)
        self._chk(self._lib.isle_hip_match_topics(self._h, _p(d) if d.size else None, int(na), int(nb), _p(ma), _p(mb), _p(md), C.byref(n), C.byref(mean),
                                                  C.byref(rounds)))
        return dict(match_a=ma, match_b=mb, match_dist=md, n_matched=int(n.value), mean_dist=float(mean.value), rounds=int(rounds.value))

    def topic_diversity(self, num_topics, model="catch"):
        """Topic diversity (ISLETrainer::output_topic_diversity, src/trainer.cpp:750-774) of a resident model, in double:
        dist[t] = |m_t - mean topic|^2 over the finite topics (NaN for the others) and their mean.  -> dict(dist float64 (k,), avg)."""
        dist = np.empty(int(num_topics), np.float64)
        avg = C.c_double()
        self._chk(self._lib.isle_hip_topic_diversity(self._h, self._MODELS[model], int(num_topics), _p(dist), C.byref(avg)))
        return dict(dist=dist, avg=float(avg.value))

    # ---- model files: the reference's text formatted on the device (include/isle_hip.h for the layouts and the domain) ------------
    def _text_call(self, call, consume):
        """Runs call(sink) with a sink that hands every piece to consume(memoryview); consume is None: the size query.  An exception
        in consume stops the delivery and is raised here.  -> (nbytes, nentries)."""
        err = []

        def tramp(ptr, n, user):
            try:
                consume(memoryview((C.c_char * n).from_address(ptr)))
                return 0
            except BaseException as e:  # never let an exception cross the C boundary
                err.append(e)
                return 1

        sink = _TEXT_SINK(tramp) if consume is not None else None
        nb, ne = C.c_uint64(), C.c_uint64()
        rc = call(C.cast(sink, C.c_void_p) if sink is not None else None, C.byref(nb), C.byref(ne))
        if err:
            raise err[0]
        self._chk(rc)
        return int(nb.value), int(ne.value)

    def _model_text_call(self, which, format, consume):
        if isinstance(which, str):
            code, host = self._MODELS[which], None
            V, cols = self._resident_shape(which)
        else:
            host = np.asfortranarray(which, np.float32)
            if host.ndim != 2:
                raise ValueError("model must be (V, cols)")
            code, (V, cols) = 2, host.shape
        fmt = TEXT_FORMATS[format] if isinstance(format, str) else int(format)
        return self._text_call(lambda sink, nb, ne: self._lib.isle_hip_model_text(self._h, code, _p(host), int(V), int(cols), fmt, sink, None,
                                                                                  nb, ne), consume)

    def model_text(self, which="catch", format="sparse"):
        """The text of a model file: "catch" (the resident topic model; sparse = M_hat_catch_sparse), "avg" (the resident average
        model; dense = M_hat_avg) or a (V, cols) array.  -> bytes."""
        parts = []
        self._model_text_call(which, format, lambda mv: parts.append(bytes(mv)))
        return b"".join(parts)

    def write_model(self, path, which="catch", format="sparse"):
        """model_text streamed into a file piece by piece; the whole text is never held.  -> (nbytes, nentries)."""
        with open(path, "wb") as f:
            return self._model_text_call(which, format, f.write)

    def model_text_size(self, which="catch", format="sparse"):
        """The counting pass alone.  -> (nbytes, nentries)."""
        return self._model_text_call(which, format, None)

    def edge_topics_text(self, pairs, primary_ratio=0.7, format="sparse", path=None):
        """The text of the edge model edge_topics(pairs, primary_ratio) returns (EdgeModel_sparse), formed and formatted on the device
        without the V x n floats.  -> bytes, or (nbytes, nentries) after streaming into `path`."""
        pairs = np.ascontiguousarray(pairs, np.int64).reshape(-1, 2)
        fmt = TEXT_FORMATS[format] if isinstance(format, str) else int(format)

        def call(sink, nb, ne):
            return self._lib.isle_hip_edge_topics_text(self._h, _p(pairs), pairs.shape[0], float(primary_ratio), fmt, sink, None, nb, ne)

        if path is not None:
            with open(path, "wb") as f:
                return self._text_call(call, f.write)
        parts = []
        self._text_call(call, lambda mv: parts.append(bytes(mv)))
        return b"".join(parts)

    # ---- corpus diagnostics of the trainer on A (include/isle_hip.h for the rules and the deviations) ----------------------
    def log_combinatorial(self):
        """SparseMatrix::compute_log_combinatorial (src/sparseMatrix.cpp:1018-1043) on the count matrix A: every document's
        log(N_d! / prod c!) from the reference's fp32 table, bit for bit.  -> float32 (docs,)."""
        D = getattr(self, "_a_shape", (0, 0, 0))[1]
        out = np.empty(max(D, 1), np.float32)
        self._chk(self._lib.isle_hip_log_combinatorial(self._h, _p(out), None))
        return out[:D]

    def distinct_top_five_sets(self, m=(2, 5, 10, 20, 50, 100, 200, 500), fetch_quintuples=False):
        """SparseMatrix::count_distint_top_five_words (src/sparseMatrix.cpp:170-215) on the count matrix A for every min_distinct in m
        (the trainer's eight by default).  -> dict(counts {m: count}, num_quintuples, run_lengths uint64 (runs,), quintuples float32
        (num_quintuples, 5) sorted lexicographically, or None without fetch_quintuples)."""
        ms = np.ascontiguousarray(m, np.int32).reshape(-1)
        D = getattr(self, "_a_shape", (0, 0, 0))[1]
        cnt = np.empty(max(ms.size, 1), np.uint64)
        nq, nr = C.c_uint64(), C.c_uint64()
        runs = np.empty(max(D, 1), np.uint64)
        q = np.empty((max(D, 1), 5), np.float32) if fetch_quintuples else None
        self._chk(self._lib.isle_hip_distinct_top_five(self._h, int(ms.size), _p(ms), _p(cnt), C.byref(nq), _p(q), _p(runs), C.byref(nr)))
        return dict(counts={int(v): int(c) for v, c in zip(ms, cnt)}, num_quintuples=int(nq.value), run_lengths=runs[:nr.value].copy(),
                    quintuples=None if q is None else q[:nq.value].copy())

    def frobenius(self):
        out = C.c_float()
        self._chk(self._lib.isle_hip_frobenius(self._h, C.byref(out)))
        return out.value

    # ---- eigensolver ----------------------------------------------------------------------
    def gram_apply(self, X):
        X = np.asfortranarray(X, dtype=np.float32)
        assert X.shape[0] == self.V
        Z = np.empty_like(X, order="F")
        self._chk(self._lib.isle_hip_gram_apply(self._h, _p(X), X.shape[1], _p(Z)))
        return Z

    def operator_form(self):
        """1 = LDS-banded Gram apply (row-constant B), 0 = gather form, -1 = operator not built yet."""
        f = C.c_int()
        self._chk(self._lib.isle_hip_operator_form(self._h, C.byref(f)))
        return f.value

    def compute_block_ks(self, num_topics, blk=BLOCK_KS_BLOCK_SIZE, ncv=None, maxit=BLOCK_KS_MAX_ITERS,
                         tol=BLOCK_KS_TOLERANCE, seed=1, allow_noconv=False):
        """FPSparseMatrix::compute_block_ks(num_topics, evalues) — src/sparseMatrix.cpp:1195-1220."""
        ncv = 2 * num_topics + BLOCK_KS_BLOCK_SIZE if ncv is None else ncv
        ev = np.empty(num_topics, np.float32)
        nconv, rst, nap = C.c_int(), C.c_int(), C.c_int()
        rc = self._lib.isle_hip_block_ks(self._h, num_topics, ncv, maxit, blk, tol, seed, _p(ev), C.byref(nconv), C.byref(rst),
                                         C.byref(nap))
        self._chk(rc, allow=(-3,) if allow_noconv else ())
        return dict(rc=rc, evals=ev, nconv=nconv.value, restarts=rst.value, napplies=nap.value)

    def block_ks_dense(self, A, nev, blk=BLOCK_KS_BLOCK_SIZE, ncv=None, maxit=BLOCK_KS_MAX_ITERS, tol=BLOCK_KS_TOLERANCE, seed=1,
                       start_block=None, allow_noconv=False):
        """BlockKs<utils::ArmaMatProdOp> (block-ks/ks_utils.h:167-182): the solver of compute_block_ks on a dense symmetric A."""
        A = np.asfortranarray(A, dtype=np.float32)
        n = A.shape[0]
        assert A.shape == (n, n)
        ncv = 2 * nev + BLOCK_KS_BLOCK_SIZE if ncv is None else ncv
        ev = np.empty(nev, np.float32)
        U = np.empty((n, nev), np.float32, order="F")
        sb = None if start_block is None else np.asfortranarray(start_block, dtype=np.float32)
        nconv, nref, rst, nap = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        rc = self._lib.isle_hip_block_ks_dense(self._h, _p(A), n, nev, ncv, maxit, blk, tol, seed, _p(sb), _p(ev), _p(U), C.byref(nconv),
                                               C.byref(nref), C.byref(rst), C.byref(nap))
        self._chk(rc, allow=(-3,) if allow_noconv else ())
        return dict(rc=rc, evals=ev, U=U, nconv=nconv.value, nconv_ref_rule=nref.value, restarts=rst.value, napplies=nap.value)

    def get_U(self, k):
        U = np.empty((self.V, k), np.float32, order="F")
        self._chk(self._lib.isle_hip_get_U(self._h, _p(U)))
        return U

    def set_U(self, U):
        U = np.asfortranarray(U, dtype=np.float32)
        self._chk(self._lib.isle_hip_set_U(self._h, _p(U), U.shape[1]))

    def eig_sym(self, S, nvec=None):
        """Small symmetric EVD of the matrix the UPPER triangle of S defines: (evals descending, vecs).  nvec=None: all n eigenvectors
        (isle_hip_eig_sym).  nvec < n: only the leading ones, as truncate() asks for them (isle_hip_eig_sym_leading): vecs is n x nvec, and
        evals[nvec:] is zero where the tridiagonal solver answered, all eigenvalues where the Jacobi solver did (eig_info says which)."""
        S = np.asfortranarray(S, dtype=np.float32)
        n = S.shape[0]
        assert S.shape == (n, n)
        e = np.empty(n, np.float32)
        if nvec is None:
            v = np.empty((n, n), np.float32, order="F")
            self._chk(self._lib.isle_hip_eig_sym(self._h, _p(S), n, _p(e), _p(v)))
        else:
            v = np.empty((n, int(nvec)), np.float32, order="F")
            self._chk(self._lib.isle_hip_eig_sym_leading(self._h, _p(S), n, int(nvec), _p(e), _p(v)))
        return e, v

    EIG_INFO = ("solver", "td_tried", "td_form", "td_bailed", "td_back", "td_rejected", "jacobi_sweeps", "n", "nvec")
    EIG_SOLVER = {0: None, 1: "tridiagonal", 2: "jacobi"}
    EIG_FORM = {0: None, 1: "persistent", 2: "chain"}
    EIG_BACK = {0: None, 1: "wy", 2: "seq8", 3: "seq4"}

    def eig_info(self):
        """What the most recent small EVD of this context did (isle_hip_eig_info): dict(solver "tridiagonal" | "jacobi" | None, td_tried,
        td_form "persistent" | "chain" | None, td_bailed, td_back "wy" | "seq8" | "seq4" | None, td_rejected, td_defect, jacobi_sweeps, n, nvec)."""
        w = (C.c_int * len(self.EIG_INFO))()
        d = C.c_float()
        self._chk(self._lib.isle_hip_eig_info(self._h, w, C.byref(d)))
        r = dict(zip(self.EIG_INFO, (int(x) for x in w)))
        r.update(solver=self.EIG_SOLVER[r["solver"]], td_form=self.EIG_FORM[r["td_form"]], td_back=self.EIG_BACK[r["td_back"]],
                 td_tried=bool(r["td_tried"]), td_bailed=bool(r["td_bailed"]), td_rejected=bool(r["td_rejected"]), td_defect=float(d.value))
        return r

    # ---- k-means --------------------------------------------------------------------------
    def kmeans_init_on_projected_space(self, k, inject_seeds=None, rng_seed=1):
        seeds = np.empty(k, np.uint64)
        Cl = np.empty((k, k), np.float32)
        res, rounds = C.c_float(), C.c_int()
        inj = None if inject_seeds is None else np.ascontiguousarray(inject_seeds, np.uint64)
        self._chk(self._lib.isle_hip_kmeanspp_projected(self._h, k, _p(inj), rng_seed, _p(seeds), _p(Cl), C.byref(res),
                                                       C.byref(rounds)))
        return dict(seeds=seeds, C_lowd=Cl, residual=res.value, rounds=rounds.value)

    def get_min_dist(self):
        md = np.empty(self.D, np.float32)
        self._chk(self._lib.isle_hip_get_min_dist(self._h, _p(md)))
        return md

    def run_lloyds_on_projected_space(self, k, C_lowd, max_reps=MAX_KMEANS_LOWD_REPS):
        Cl = np.array(C_lowd, dtype=np.float32, order="C", copy=True)
        it = C.c_int()
        assign = np.empty(self.D, np.uint32)
        self._chk(self._lib.isle_hip_lloyds_projected(self._h, k, _p(Cl), max_reps, C.byref(it), _p(assign)))
        return self._with_trace(dict(C_lowd=Cl, iters=it.value, assign=assign), "projected")

    def left_multiply_by_U(self, C_lowd, fetch=True):
        """centers (V x n, F-order) = U * C_lowd^T, centre c = row c of C_lowd (ld_in = k)."""
        Cl = np.ascontiguousarray(C_lowd, dtype=np.float32)
        n, k = Cl.shape
        out = np.empty((self.V, n), np.float32, order="F") if fetch else None
        self._chk(self._lib.isle_hip_lift_centers(self._h, _p(Cl), k, n, _p(out)))
        return out

    def run_lloyds(self, k, centers=None, max_reps=MAX_KMEANS_REPS, fetch_centers=True):
        cin = None if centers is None else np.asfortranarray(centers, dtype=np.float32)
        cout = np.empty((self.V, k), np.float32, order="F") if fetch_centers else None
        assign = np.empty(self.D, np.uint32)
        it = C.c_int()
        self._chk(self._lib.isle_hip_lloyds_sparse(self._h, k, _p(cin), _p(cout), _p(assign), max_reps, C.byref(it)))
        return self._with_trace(dict(centers=cout, assign=assign, iters=it.value), "word")

    # ---- the k-means objective ------------------------------------------------------------------
    SPACES = {"word": 0, "projected": 1}

    def _space(self, space):
        if space not in self.SPACES:
            raise ValueError("space must be 'word' or 'projected', not %r" % (space,))
        return self.SPACES[space]

    def kmeans_objective(self, k, space="word", assign=None, centers=None, fetch_docs=False):
        """Per-cluster and total k-means objective of a partition (include/isle_hip.h, isle_hip_kmeans_objective).
        assign / centers None: the resident ones of the last loop in `space`.  centers: vocab x k (word), k x k rows = centres
        (projected).  Returns dict(sums, sizes, total[, doc_dist]); collective over document shards."""
        sp = self._space(space)
        a = c = None
        if assign is not None:
            a = _as_u32(assign, "assign")
            if a.shape[0] != self.D:
                raise ValueError("assign has %d entries, the shard %d documents" % (a.shape[0], self.D))
            if self.D == 0:
                a = np.zeros(1, np.uint32)  # a rank without documents still passes an explicit (empty) partition
        if centers is not None:
            c = np.asfortranarray(centers, dtype=np.float32) if sp == 0 else np.ascontiguousarray(centers, dtype=np.float32)
            if c.shape != ((self.V, k) if sp == 0 else (k, k)):
                raise ValueError("centers have shape %r" % (c.shape,))
        sums = np.empty(k, np.float64)
        sizes = np.empty(k, np.uint64)
        total = C.c_double()
        dd = np.empty(self.D, np.float64) if fetch_docs else None
        self._chk(self._lib.isle_hip_kmeans_objective(self._h, sp, k, _p(a), _p(c), _p(sums), _p(sizes), C.byref(total), _p(dd)))
        out = dict(sums=sums, sizes=sizes, total=total.value)
        if fetch_docs:
            out["doc_dist"] = dd
        return out

    def get_projection(self, k):
        """The shard's rows of P = B^T U as the device holds them (D x k): the documents of space="projected"."""
        P = np.empty((self.D, k), np.float32)
        self._chk(self._lib.isle_hip_get_projection(self._h, k, _p(P)))
        return P

    def lloyds_trace(self, on=True):
        """While on, run_lloyds / run_lloyds_on_projected_space also return "objective": the total objective after every centre update."""
        self._chk(self._lib.isle_hip_lloyds_trace(self._h, 1 if on else 0))
        self._trace = bool(on)

    def _with_trace(self, out, space):
        if getattr(self, "_trace", False):
            n = C.c_int()
            self._chk(self._lib.isle_hip_lloyds_trace_get(self._h, self.SPACES[space], None, 0, C.byref(n)))
            tr = np.empty(n.value, np.float64)
            self._chk(self._lib.isle_hip_lloyds_trace_get(self._h, self.SPACES[space], _p(tr), n.value, None))
            out["objective"] = tr
        return out

    # ---- measurement ------------------------------------------------------------------------
    # ---- inference -------------------------------------------------------
    def infer(self, model_by_word, offs, rows, counts, iters=15, Lf=10.0, avg_doc_sz=None, want_weights=True):
        """ISLEInfer over a count matrix in CSC (drivers/ISLEInfer.cpp:60-112, src/infer.cpp:361-492).
        model_by_word: V x k row-major.  Returns weights (D x k), top_topic / top_weight (D x 5), llh (D x 2), nconverged."""
        M = np.ascontiguousarray(model_by_word, np.float32)
        V, k = M.shape
        offs = np.ascontiguousarray(offs, np.int64)
        rows = np.ascontiguousarray(rows, np.uint32)
        counts = np.ascontiguousarray(counts, np.float32)
        D = offs.shape[0] - 1
        if avg_doc_sz is None:  # populate_CSC, src/sparseMatrix.cpp:87-98
            nz = int((np.diff(offs) > 0).sum())
            avg_doc_sz = float(int(counts.astype(np.float64).sum()) // max(nz, 1))
        W = np.empty((D, k), np.float32) if want_weights else None
        tt = np.empty((D, 5), np.int32)
        tw = np.empty((D, 5), np.float32)
        llh = np.empty((D, 2), np.float32)
        nc = C.c_uint64()
        self._chk(self._lib.isle_hip_infer(self._h, V, k, _p(M), D, rows.shape[0], _p(counts), _p(rows), _p(offs), int(iters), float(Lf),
                                           float(avg_doc_sz), _p(W) if want_weights else None, _p(tt), _p(tw), _p(llh), C.byref(nc)))
        return dict(weights=W, top_topic=tt, top_weight=tw, llh=llh, nconverged=int(nc.value), avg_doc_sz=avg_doc_sz)

    def infer_resident(self, model="catch", docs=None, iters=15, Lf=10.0, min_weight=None, chunk_docs=0, fetch_entries=True):
        """Topic weights of documents of the resident count matrix A under a resident model ("catch", "avg") or a (V, cols) array, the
        iterations of infer() on the device-resident data: the same bits for the same fp32 model and documents.  docs: None (all of
        A) or (begin, end); row 0 of the outputs is document `begin`.  avg_doc_sz is the corpus value of the context, over all of A.
        The weights come back sparse: for every converged document the topics with weight > min_weight (None: 1 / cols), ascending,
        as CSR (offs int64 (n + 1,), topic uint32, weight float32); the dense (n, cols) matrix never exists.  chunk_docs: documents
        per pass on the device (0: a 1 GiB budget of dense weights); no result depends on it.
        Under comm_init / comm_init_host: docs and every output are this rank's own documents', rows numbered from docs[0]; avg_doc_sz
        is the corpus value over all ranks.  Where threshold() has not left it behind (B uploaded from the host) the call is COLLECTIVE
        (one all-reduce of two totals): every rank calls, in the same order, a rank without documents included.  The shards' entries
        side by side are the single-rank run's, bit for bit.  model="avg" is refused there.
        -> dict(top_topic, top_weight, llh, nconverged, nentries, avg_doc_sz[, offs, topic, weight])."""
        if isinstance(model, str):
            which, host = self._MODELS[model], None
            V, cols = self._resident_shape(model)
        else:
            host = np.asfortranarray(model, np.float32)
            if host.ndim != 2:
                raise ValueError("model must be (V, cols)")
            which, (V, cols) = 2, host.shape
        b, e = (0, getattr(self, "_a_shape", (0, 0, 0))[1]) if docs is None else (int(docs[0]), int(docs[1]))
        n = max(e - b, 0)
        tt = np.empty((n, 5), np.int32)
        tw = np.empty((n, 5), np.float32)
        llh = np.empty((n, 2), np.float32)
        nc, ne = C.c_uint64(), C.c_uint64()
        self._chk(self._lib.isle_hip_infer_resident(self._h, which, _p(host), int(V), int(cols), b, e, int(iters), float(Lf),
                                                    -1.0 if min_weight is None else float(min_weight), int(chunk_docs), _p(tt), _p(tw),
                                                    _p(llh), C.byref(nc), C.byref(ne)))
        self._inf_rows = n
        self._inf_begin = b
        self._inf_cols = int(cols)
        out = dict(top_topic=tt, top_weight=tw, llh=llh, nconverged=int(nc.value), nentries=int(ne.value), avg_doc_sz=self.avg_doc_sz())
        if fetch_entries:
            out.update(zip(("offs", "topic", "weight"), self.infer_entries(n, out["nentries"])))
        return out

    # ---- the per-document topic files formatted on the device (include/isle_hip.h, isle_hip_infer_text) --------------------------
    def _infer_text_call(self, what, rows, base, consume):
        kind = DOC_TEXT_KINDS[what] if isinstance(what, str) else int(what)
        b, e = (0, getattr(self, "_inf_rows", 0)) if rows is None else (int(rows[0]), int(rows[1]))
        return self._text_call(lambda sink, nb, nl: self._lib.isle_hip_infer_text(self._h, kind, b, e, int(base), sink, None, nb, nl), consume)

    def infer_text(self, what="entries", rows=None, base=1):
        """The lines "<row + base>\\t<topic + 1>\\t<weight>\\n" of rows (None: all; or (begin, end), row 0 = the first document) of the
        last infer_resident, formatted on the device from the resident result: "entries" (every entry, DocTopicWeights.tsv) or "top"
        (the at most five heaviest topics of a document, ISLEInfer's top_topics_* files).  Under comm_init / comm_init_host: no
        collective; base stays the caller's: after infer_resident(docs=(b, e)) pass base + a_doc_offset + b, and the ranks' texts in
        rank order are the corpus's file.  -> bytes."""
        parts = []
        self._infer_text_call(what, rows, base, lambda mv: parts.append(bytes(mv)))
        return b"".join(parts)

    def write_infer_text(self, path, what="entries", rows=None, base=1):
        """infer_text streamed into a file piece by piece; the whole text is never held.  -> (nbytes, nlines)."""
        with open(path, "wb") as f:
            return self._infer_text_call(what, rows, base, f.write)

    def infer_text_size(self, what="entries", rows=None, base=1):
        """The counting pass alone.  -> (nbytes, nlines)."""
        return self._infer_text_call(what, rows, base, None)

    # ---- the trainer's per-document report files formatted on the device (include/isle_hip.h, isle_hip_doc_report_text) -----------
    def _doc_report_call(self, what, docs, consume):
        kind = DOC_REPORT_KINDS[what] if isinstance(what, str) else int(what)
        b, e = (0, getattr(self, "_a_shape", (0, 0, 0))[1]) if docs is None else (int(docs[0]), int(docs[1]))
        return self._text_call(lambda sink, nb, nl: self._lib.isle_hip_doc_report_text(self._h, kind, b, e, sink, None, nb, nl), consume)

    def doc_report_text(self, what, docs=None):
        """A per-document report file of the trainer for documents docs (None: all of A; or (begin, end)), formatted on the device from
        what find_catchwords / construct_topic_model left resident; every number is printed 1-based:
          "catchwords"         DocCatchword.tsv: "<doc>\\t<word>\\t<normalised value>\\n" for every entry of A whose word is a catchword
          "topic_sums"         DocTopicCatchwordSums.tsv: "<doc>\\t<topic>\\t<sum>\\n", topic ascending, then value descending, ties by
                               document ascending (the reference's order up to its unstable ties)
          "topic_sums_by_doc"  the same lines, (document, topic) ascending
          "top_two"            TopTwoTopicsPerDoc.txt: "<doc>\\t<top1>\\t<top2>\\n" for every document that has both
        Under comm_init / comm_init_host: docs are this rank's own documents and <doc> is a_doc_offset + doc + 1, the number in the
        corpus.  "catchwords", "topic_sums_by_doc" and "top_two" involve no collective: the ranks' texts in rank order are the corpus's
        file.  "topic_sums" is COLLECTIVE (write_doc_report and doc_report_size too): all ranks ask for it together, a rank without
        documents included; the sums of all ranks are ordered as one and rank q receives lines [slice(q), slice(q + 1)) of the L lines
        of the corpus's file, slice(q) = q * (L // W) + min(q, L % W): the ranks' texts in rank order are the single-rank file.
        -> bytes."""
        parts = []
        self._doc_report_call(what, docs, lambda mv: parts.append(bytes(mv)))
        return b"".join(parts)

    def write_doc_report(self, path, what, docs=None):
        """doc_report_text streamed into a file piece by piece; the whole text is never held.  -> (nbytes, nlines)."""
        with open(path, "wb") as f:
            return self._doc_report_call(what, docs, f.write)

    def doc_report_size(self, what, docs=None):
        """The counting pass alone.  -> (nbytes, nlines)."""
        return self._doc_report_call(what, docs, None)

    def avg_doc_sz(self):
        """avg_doc_sz of the resident count matrix (populate_CSC, src/sparseMatrix.cpp:87-98: floor(tokens / non-empty documents)).
        Under comm_init / comm_init_host: the corpus value over all ranks' documents; COLLECTIVE where threshold() has not left it
        behind (every rank calls, a rank without documents included)."""
        v = C.c_float()
        self._chk(self._lib.isle_hip_avg_doc_sz(self._h, C.byref(v)))
        return float(v.value)

    def infer_entries(self, num_docs, nentries):
        """The entries of the last infer_resident (num_docs, nentries as it returned them) -> (offs, topic, weight)."""
        off = np.empty(num_docs + 1, np.int64)
        tp = np.empty(nentries, np.uint32)
        wt = np.empty(nentries, np.float32)
        self._chk(self._lib.isle_hip_get_infer_entries(self._h, _p(off), _p(tp), _p(wt)))
        return off, tp, wt

    # ---- the heaviest documents of every topic, selected on the device (include/isle_hip.h, isle_hip_topic_top_docs) ---------------
    _TOPDOCS = {"infer": 0, "sums": 1}

    def topic_top_docs(self, n, source="infer", num_topics=None, doc_base=0):
        """The n (1 .. 256) heaviest documents of every topic, by an exact selection on the device over entries stored by document:
        source "infer" (the entries of the last infer_resident; row 0 is its first document), "sums" (the document-topic catchword sums
        of the last construct_topic_model) or a CSR (doc_offsets (rows + 1,), topic, value) uploaded for the call, topics ascending
        strictly within a row.  The document of a row is doc_base + row.  The heavier value comes first, in the order of the fp32 bits
        (ord(b) = b ^ (0xffffffff if b >> 31 else 0x80000000): for positive finite values the numeric order), the smaller document among
        bit-equal values.  num_topics: None = that of the source ("sums": the topic model's; "infer": the model's columns; a CSR: its
        largest topic + 1).  Nothing resident changes and nothing is kept.
        Under comm_init / comm_init_host the call is COLLECTIVE: every rank calls with the same source kind, num_topics and n, a rank
        without rows or entries included, and passes its own doc_base (a_doc_offset, plus docs[0] of infer_resident for "infer"); every
        rank gets the corpus's lists, bit-identical, the lists one rank holding all entries gets.
        -> dict(docs uint32 (num_topics, n), values float32 (num_topics, n), counts uint32 (num_topics,) = min(n, entries of the topic),
        topic_entries uint64 (num_topics,)); the unused slots hold 0xffffffff / 0.0."""
        off = tp = va = None
        rows = 0
        if isinstance(source, str):
            kind = self._TOPDOCS[source]
            if num_topics is None:
                num_topics = getattr(self, "_post_k", 0) if source == "sums" else getattr(self, "_inf_cols", 0)
        else:
            kind = 2
            off = np.ascontiguousarray(source[0], np.int64)
            tp = _as_u32(source[1], "topic")
            va = np.ascontiguousarray(source[2], np.float32)
            if off.ndim != 1 or off.size < 1 or va.ndim != 1 or tp.size != va.size or (off.size > 1 and int(off[-1]) != tp.size):
                raise ValueError("source: (doc_offsets (rows + 1,), topic, value) with doc_offsets[-1] entries")
            rows = off.size - 1
            if num_topics is None:
                num_topics = int(tp.max()) + 1 if tp.size else 1
        k, n = int(num_topics), int(n)
        shape = (max(k, 0), max(n, 0))
        docs = np.empty(shape, np.uint32)
        values = np.empty(shape, np.float32)
        counts = np.empty(shape[0], np.uint32)
        entries = np.empty(shape[0], np.uint64)
        self._chk(self._lib.isle_hip_topic_top_docs(self._h, kind, k, n, int(doc_base), rows, _p(off), _p(tp), _p(va), _p(docs), _p(values), _p(counts),
                                                    _p(entries)))
        return dict(docs=docs, values=values, counts=counts, topic_entries=entries)

    # ---- the documents most similar to a query document, scored and selected on the device (include/isle_hip.h, isle_hip_similar_docs) ----
    _SIM = {"dot": 0, "cosine": 1, "bhattacharyya": 2}

    def simdocs_table_form(self, form="auto"):
        """The home of similar_docs' query table: "auto" (LDS while the table fits in 64 KiB, else global memory), "lds", "global".  A
        setting of the context; both homes give the same bits ("lds" where the table does not fit is global all the same)."""
        self._chk(self._lib.isle_hip_simdocs_table_form(self._h, {"auto": 0, "lds": 1, "global": 2}.get(form, form)))

    def similar_docs(self, queries, n, source="infer", measure="cosine", num_topics=None, doc_base=0, exclude=None):
        """The n (1 .. 256) documents most similar to each of 1 .. 64 queries, over sparse topic weights stored by document: source as
        topic_top_docs ("infer", "sums" or a CSR (doc_offsets, topic, weight)); the document of a row is doc_base + row.  queries: an
        integer array of rows of the source (gathered on the device; a query's own document is excluded unless exclude is given), or a
        CSR (q_offsets (Q + 1,), q_topic, q_weight), topics ascending strictly within a query.  measure "dot", "cosine" or
        "bhattacharyya" (include/isle_hip.h states the arithmetic; device and host agree bit for bit).  A row is a candidate of a query
        when they STORE a common topic, whatever the weights; exclude: per query a document that is no candidate (0xffffffff: none).
        The higher score comes first, the smaller document among bit-equal scores.  Weights are finite, >= 0 and < 2^31.
        Under comm_init / comm_init_host the call is COLLECTIVE as topic_top_docs: the same queries (a CSR: rows are refused) on every
        rank, each rank its own doc_base; every rank gets the corpus's lists.
        -> dict(docs uint32 (Q, n), scores float32 (Q, n), counts uint32 (Q,) = min(n, candidates), candidates uint64 (Q,)); the unused
        slots hold 0xffffffff / 0.0."""
        off = tp = va = None
        rows = 0
        if isinstance(source, str):
            kind = self._TOPDOCS[source]
            if num_topics is None:
                num_topics = getattr(self, "_post_k", 0) if source == "sums" else getattr(self, "_inf_cols", 0)
        else:
            kind = 2
            off = np.ascontiguousarray(source[0], np.int64)
            tp = _as_u32(source[1], "topic")
            va = np.ascontiguousarray(source[2], np.float32)
            if off.ndim != 1 or off.size < 1 or va.ndim != 1 or tp.size != va.size or (off.size > 1 and int(off[-1]) != tp.size):
                raise ValueError("source: (doc_offsets (rows + 1,), topic, weight) with doc_offsets[-1] entries")
            rows = off.size - 1
        qrows = qo = qt = qw = None
        if isinstance(queries, (tuple, list)) and len(queries) == 3 and np.ndim(queries[0]) >= 1:
            qo = np.ascontiguousarray(queries[0], np.int64)
            qt = _as_u32(queries[1], "q_topic")
            qw = np.ascontiguousarray(queries[2], np.float32)
            if qo.ndim != 1 or qo.size < 1 or qw.ndim != 1 or qt.size != qw.size:
                raise ValueError("queries: rows, or (q_offsets (Q + 1,), q_topic, q_weight)")
            Q = qo.size - 1
            if num_topics is None:
                num_topics = max(int(tp.max()) + 1 if tp is not None and tp.size else 1, int(qt.max()) + 1 if qt.size else 1)
        else:
            qrows = np.ascontiguousarray(queries, np.uint64).reshape(-1)
            Q = qrows.size
            if num_topics is None:
                num_topics = int(tp.max()) + 1 if tp is not None and tp.size else 1
        ex = None
        if exclude is not None:
            ex = np.ascontiguousarray(exclude, np.uint32).reshape(-1)
            if ex.size != Q:
                raise ValueError("exclude: one document per query")
        n = int(n)
        shape = (max(Q, 0), max(n, 0))
        docs = np.empty(shape, np.uint32)
        scores = np.empty(shape, np.float32)
        counts = np.empty(shape[0], np.uint32)
        cand = np.empty(shape[0], np.uint64)
        self._chk(self._lib.isle_hip_similar_docs(self._h, kind, self._SIM.get(measure, measure), int(num_topics), n, int(doc_base), rows, _p(off), _p(tp),
                                                  _p(va), Q, _p(qrows), _p(qo), _p(qt), _p(qw), _p(ex), _p(docs), _p(scores), _p(counts), _p(cand)))
        return dict(docs=docs, scores=scores, counts=counts, candidates=cand)

    # ---- topic prevalence by group of documents, summed on the device (include/isle_hip.h, isle_hip_topic_prevalence) ----------------
    GROUP_NONE = 0xFFFFFFFF

    def prevalence_tile_form(self, form="auto"):
        """The topics of one private table of topic_prevalence: "auto" / "wide" (1024) or "narrow" (64, so that small tests cross tile
        edges).  A setting of the context; both forms give the same bits."""
        self._chk(self._lib.isle_hip_prevalence_tile_form(self._h, {"auto": 0, "wide": 1, "narrow": 2}.get(form, form)))

    def topic_prevalence(self, source="infer", groups=None, num_groups=None, normalise=False, num_topics=None):
        """How much of the corpus each topic is, by group of documents, over sparse topic weights stored by document: source as
        topic_top_docs ("infer", "sums" or a CSR (doc_offsets, topic, weight)).  groups: one uint32 label per row (GROUP_NONE = 0xffffffff:
        the row belongs to no group and is counted in `unlabelled` alone), or None: every row has label 0.  num_groups: None = the largest
        label that is not GROUP_NONE + 1, or 1 without labels.  normalise: every row's weights divided by the row's sum first.  Weights
        are finite, >= 0 and < 2^31.  The sums are added in a stated order (include/isle_hip.h: rows ascending, 64 at a time, level by
        level), so they are the same bits on every call and equal isle_amd/csrc/prevalence_host.h's host loop bit for bit.
        One rank only: under comm_init / comm_init_host with several ranks the call is refused.  Nothing resident changes.
        -> dict(docs uint64 (G,), unlabelled int, count uint64 (G, k) = rows of the group that store the topic, dominant uint64 (G, k) =
        rows whose heaviest topic it is, sum float64 (G, k), mean float64 (G, k) = sum / docs, NaN for a group without rows)."""
        off = tp = va = None
        rows = 0
        if isinstance(source, str):
            kind = self._TOPDOCS[source]
            if num_topics is None:
                num_topics = getattr(self, "_post_k", 0) if source == "sums" else getattr(self, "_inf_cols", 0)
        else:
            kind = 2
            off = np.ascontiguousarray(source[0], np.int64)
            tp = _as_u32(source[1], "topic")
            va = np.ascontiguousarray(source[2], np.float32)
            if off.ndim != 1 or off.size < 1 or va.ndim != 1 or tp.size != va.size or (off.size > 1 and int(off[-1]) != tp.size):
                raise ValueError("source: (doc_offsets (rows + 1,), topic, weight) with doc_offsets[-1] entries")
            rows = off.size - 1
            if num_topics is None:
                num_topics = int(tp.max()) + 1 if tp.size else 1
        lab = None
        if groups is not None:
            lab = _as_u32(groups, "groups").reshape(-1)
            have = rows if kind == 2 else (getattr(self, "_a_shape", (0, 0, 0))[1] if kind == 1 else getattr(self, "_inf_rows", 0))
            if lab.size != have:  # (the library reads one label per row of the source)
                raise ValueError("groups: %d labels for the %d rows of the source" % (lab.size, have))
            if num_groups is None:
                real = lab[lab != self.GROUP_NONE]
                num_groups = int(real.max()) + 1 if real.size else 1
        elif num_groups is None:
            num_groups = 1
        k, G = int(num_topics), int(num_groups)
        if not 0 <= G <= 0xFFFFFFFF:
            raise ValueError("num_groups: a 32-bit number")
        shape = (G, max(k, 0))
        docs = np.zeros(G, np.uint64)
        count = np.zeros(shape, np.uint64)
        dominant = np.zeros(shape, np.uint64)
        total = np.zeros(shape, np.float64)
        none = C.c_uint64(0)
        self._chk(self._lib.isle_hip_topic_prevalence(self._h, kind, k, rows, _p(off), _p(tp), _p(va), _p(lab), G, int(normalise), _p(docs), C.byref(none),
                                                      _p(count), _p(dominant), _p(total)))
        with np.errstate(divide="ignore", invalid="ignore"):
            mean = total / docs.astype(np.float64)[:, None]
        return dict(docs=docs, unlabelled=int(none.value), count=count, dominant=dominant, sum=total, mean=mean)

    # ---- held-out scores per document (include/isle_hip.h, isle_hip_score_docs) ------------------------------------------------------
    _SCORE_MEASURES = {"log": 0, "prob": 1}

    def score_docs(self, model="catch", weights="infer", entries="resident", docs=None, measure="log", normalise=False, floor=0.0, with_z=False):
        """How well topic weights predict the entries of a count matrix, per document: z = M[w, :] . theta[:, d] at every entry (w, c), the
        term c log z ("log") or c z ("prob"), summed per document in a stated order (include/isle_hip.h; the rule:
        isle_amd/csrc/score_host.h).  model: as infer_resident.  weights: "infer" (the rows of the last infer_resident) or a CSR
        (offs, topic, weight), topics ascending strictly within a row.  entries: "resident" (documents docs = (begin, end) of A; None: the
        documents of the last infer_resident with weights="infer", else the first rows of A) or a CSC (counts, rows, offs) uploaded for
        the call.  normalise: every row's weights divided by the row's sum first.  floor > 0: an entry with z < floor is scored at floor
        and counted in `floored`; otherwise an entry with z == 0, and always one with z NaN, infinite or negative, is unscored: it adds
        nothing and is counted.  with_z (a caller's CSC only): z of every entry.  Nothing resident changes.
        Under comm_init / comm_init_host: no collective; every rank scores its own rows, and the ranks' arrays side by side are the
        single-rank arrays bit for bit.  model="avg" is refused there.
        -> dict(score, tokens, unscored_tokens float64 (n,), unscored_entries, floored uint32 (n,), total_score, total_tokens (through
        score_total), perplexity = exp(-total_score / total_tokens) for "log" (NaN without tokens; None for "prob")[, z float64])."""
        if isinstance(model, str):
            which, host = self._MODELS[model], None
            V, cols = self._resident_shape(model)
        else:
            host = np.asfortranarray(model, np.float32)
            if host.ndim != 2:
                raise ValueError("model must be (V, cols)")
            which, (V, cols) = 2, host.shape
        woff = wtp = wva = None
        if isinstance(weights, str):
            if weights != "infer":
                raise ValueError("weights: \"infer\" or (offs, topic, weight)")
            wkind, n = 0, None  # (the rows are the entries' documents; the library holds them to the resident result's)
        else:
            wkind = 2
            woff = np.ascontiguousarray(weights[0], np.int64)
            wtp = _as_u32(weights[1], "topic")
            wva = np.ascontiguousarray(weights[2], np.float32)
            if woff.ndim != 1 or woff.size < 1 or wva.ndim != 1 or wtp.size != wva.size or (woff.size > 1 and int(woff[-1]) != wtp.size):
                raise ValueError("weights: (offs (rows + 1,), topic, weight) with offs[-1] entries")
            n = woff.size - 1
        cnt = rws = off = None
        begin = 0
        if isinstance(entries, str):
            if entries != "resident":
                raise ValueError("entries: \"resident\" or (counts, rows, offs)")
            ekind = 0
            if docs is not None:
                begin, have = int(docs[0]), max(int(docs[1]) - int(docs[0]), 0)
            else:
                begin, have = (getattr(self, "_inf_begin", 0), getattr(self, "_inf_rows", 0)) if wkind == 0 else (0, n)
            if n is not None and have != n:
                raise ValueError("docs: %d documents for %d weight rows" % (have, n))
            n = have
        else:
            ekind = 1
            cnt = np.ascontiguousarray(entries[0], np.float32)
            rws = _as_u32(entries[1], "rows")
            off = np.ascontiguousarray(entries[2], np.int64)
            if off.ndim != 1 or off.size < 1 or cnt.ndim != 1 or rws.size != cnt.size or (off.size > 1 and int(off[-1]) != cnt.size):
                raise ValueError("entries: (counts, rows, offs (docs + 1,)) with offs[-1] entries")
            if n is not None and off.size - 1 != n:
                raise ValueError("entries: %d documents for %d weight rows" % (off.size - 1, n))
            n = off.size - 1
        if with_z and ekind != 1:
            raise ValueError("with_z needs a caller's CSC (fetch A with get_A and pass it)")
        score = np.zeros(n, np.float64)
        tokens = np.zeros(n, np.float64)
        ut = np.zeros(n, np.float64)
        ue = np.zeros(n, np.uint32)
        fl = np.zeros(n, np.uint32)
        z = np.zeros(cnt.size, np.float64) if with_z else None
        m = self._SCORE_MEASURES[measure] if isinstance(measure, str) else int(measure)
        self._chk(self._lib.isle_hip_score_docs(self._h, which, _p(host), int(V), int(cols), wkind, n, _p(woff), _p(wtp), _p(wva), ekind, begin, _p(cnt),
                                                _p(rws), _p(off), m, int(normalise), float(floor), _p(score), _p(tokens), _p(ue), _p(ut), _p(fl),
                                                _p(z)))
        out = dict(score=score, tokens=tokens, unscored_entries=ue, unscored_tokens=ut, floored=fl, total_score=score_total(score),
                   total_tokens=score_total(tokens), perplexity=None)
        if m == 0:
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                out["perplexity"] = float(np.exp(-np.float64(out["total_score"]) / np.float64(out["total_tokens"])))
        if with_z:
            out["z"] = z
        return out

    def completion_score(self, V, counts, rows, offs, model, seed=0, num=1, den=2, iters=15, Lf=10.0, floor=0.0, doc_offset=0):
        """Document completion, the held-out measure of a topic model: split_held_out(counts, rows, offs, seed, num, den, doc_offset);
        upload_counts of the observed part, which REPLACES THE RESIDENT COUNT MATRIX A (and voids what was derived from it);
        infer_resident(model, min_weight=0.0) on it; score_docs of the held part as a caller's CSC with weights="infer", measure "log",
        normalise=True.  model: a (V, cols) array, or "loaded" (a resident catch or average model goes with the A it came from).
        -> score_docs' dict, and observed / held (the two CSC parts), nconverged."""
        obs, held = split_held_out(counts, rows, offs, seed, num, den, doc_offset)
        self.upload_counts(V, *obs)
        inf = self.infer_resident(model, iters=iters, Lf=Lf, min_weight=0.0, fetch_entries=False)
        out = self.score_docs(model, weights="infer", entries=held, measure="log", normalise=True, floor=floor)
        out.update(observed=obs, held=held, nconverged=inf["nconverged"])
        return out

    def timing_enable(self, on=True):
        """0 / False: off; 1 / True: events around every launch; 2: around the Gram-apply launches only."""
        self._chk(self._lib.isle_hip_timing_enable(self._h, int(on)))

    def timing_reset(self):
        self._chk(self._lib.isle_hip_timing_reset(self._h))

    def timing_get(self):
        n = len(TIMING_FAMILIES)
        ms = np.zeros(n, np.float64)
        cnt = np.zeros(n, np.uint64)
        self._chk(self._lib.isle_hip_timing_get(self._h, _p(ms), _p(cnt)))
        return {f: (float(ms[i]), int(cnt[i])) for i, f in enumerate(TIMING_FAMILIES)}

    def synchronize(self):
        self._chk(self._lib.isle_hip_synchronize(self._h))
