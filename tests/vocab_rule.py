"""The rule of isle_hip_prune_vocab (include/isle_hip.h, isle_amd/csrc/vocab_host.h) in numpy, and the case table the vocabulary tests share
(a plain module: no torch, no GPU, no library).  A count crosses as its 32 bits.

  df[w]    the documents whose column holds word w          passes   min_df <= df[w] <= max_df' (max_df, or the document count at 0)
  keep_n   > 0 and more passers: the keep_n with the largest (df, -w)      new ids  the kept words in ascending old id
  new A    every document's entries of kept words, in order, counts bit for bit      emptied  documents that had entries and have none"""
from collections import namedtuple

import numpy as np

PART = 16384            # vocab_host.h VOCAB_DF_PART (test_vocab_rule_cpu.py holds this copy to the header through vocab_host_main)
SCAN_TILE = 4096        # scan.h
DROPPED = 0xFFFFFFFF

Case = namedtuple("Case", "name V offs rows counts min_df max_df keep_n aim device")


def csc(V, docs, counts=None):
    """docs: one collection of word ids per document -> (offs int64, rows uint32 ascending per document, counts float32 (default 1 .. 9))"""
    offs = np.zeros(len(docs) + 1, np.int64)
    rows = []
    for d, w in enumerate(docs):
        w = np.unique(np.asarray(w, np.int64))
        assert w.size == 0 or (0 <= w[0] and w[-1] < V)
        rows.append(w)
        offs[d + 1] = offs[d] + w.size
    rows = np.concatenate(rows).astype(np.uint32) if rows else np.zeros(0, np.uint32)
    if counts is None:
        counts = (1 + (np.arange(rows.size) * 7 + 3) % 9).astype(np.float32)
    counts = np.asarray(counts, np.float32)
    assert counts.size == rows.size and (counts > 0).all()
    return offs, rows, counts


def df_of(V, rows):
    return np.bincount(rows, minlength=V).astype(np.uint32)


def max_df_of(max_df, docs_global):
    return max_df if max_df else docs_global


def check_args(min_df, max_df, keep_n, docs_global):
    """the refusals that need no table: '' = accepted"""
    top = max_df_of(max_df, docs_global)
    if min_df > top:
        return "prune_vocab: min_df = %d > max_df = %d%s" % (min_df, top, "" if max_df else " (the corpus's document count)")
    if keep_n >= 2 ** 32:
        return "prune_vocab: keep_n = %d, 2^32 or more" % keep_n
    return ""


def rule_on_df(df, min_df, max_df, keep_n, docs_global):
    """-> (text, remap uint32 (V,), kept_words uint32)"""
    text = check_args(min_df, max_df, keep_n, docs_global)
    if text:
        return text, None, None
    top = max_df_of(max_df, docs_global)
    d = df.astype(np.int64)
    passers = np.flatnonzero((d >= min_df) & (d <= top))
    if keep_n and passers.size > keep_n:
        order = np.lexsort((passers, -d[passers]))   # by df descending, then by word ascending
        passers = np.sort(passers[order[:keep_n]])
    if passers.size == 0:
        return "prune_vocab: no word kept (min_df = %d, max_df = %d, keep_n = %d)" % (min_df, top, keep_n), None, None
    remap = np.full(df.size, DROPPED, np.uint32)
    remap[passers] = np.arange(passers.size, dtype=np.uint32)
    return "", remap, passers.astype(np.uint32)


def prune_csc(offs, rows, counts, remap):
    """-> (offs, rows, counts, documents emptied)"""
    keep = remap[rows] != DROPPED
    pos = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)
    new_offs = pos[offs]
    emptied = int(((np.diff(offs) > 0) & (np.diff(new_offs) == 0)).sum())
    return new_offs, remap[rows[keep]].astype(np.uint32), counts[keep].copy(), emptied


def rule(case, docs_global=None, df=None):
    """What isle_hip_prune_vocab answers for the case as one rank holds it (df: the corpus's, where the case is a shard of one)."""
    D = case.offs.size - 1
    docs_global = D if docs_global is None else docs_global
    df = df_of(case.V, case.rows) if df is None else df
    text, remap, kept = rule_on_df(df, case.min_df, case.max_df, case.keep_n, docs_global)
    if text:
        return dict(text=text, df=df)
    offs, rows, counts, emptied = prune_csc(case.offs, case.rows, case.counts, remap)
    return dict(text="", df=df, kept_words=kept, vocab=int(kept.size), offs=offs, rows=rows, counts=counts.view(np.uint32), nnz=int(rows.size),
                docs_emptied=emptied, remap=remap)


def share(case, cut, rank):
    """rank's documents [cut[rank], cut[rank + 1]) of the case -> (offs, rows, counts, doc_offset)"""
    b, e = int(cut[rank]), int(cut[rank + 1])
    lo, hi = int(case.offs[b]), int(case.offs[e])
    return case.offs[b:e + 1] - lo, case.rows[lo:hi], case.counts[lo:hi], b


def rule_share(case, cut, rank):
    """rank's slice of the single-rank result: (offs, rows, count bits)"""
    want = rule(case)
    b, e = int(cut[rank]), int(cut[rank + 1])
    lo, hi = int(want["offs"][b]), int(want["offs"][e])
    return want["offs"][b:e + 1] - lo, want["rows"][lo:hi], want["counts"][lo:hi]


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------
def _zipf_docs(V, D, seed, mean_len=20, must=()):
    """D documents of words drawn with a heavy head (word = V u^3); the words of `must` are spread over the first documents so that every
    one of them occurs, each in a different number of documents"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 2 * mean_len, size=D)
    docs = [np.minimum(V - 1, (V * rng.random(n) ** 3).astype(np.int64)) for n in lens]
    for i, w in enumerate(must):
        for d in range(1 + i % 5):
            docs[(3 * i + d) % D] = np.append(docs[(3 * i + d) % D], w)
    return docs


def _exact_nnz(V, nnz, seed):
    """a corpus of exactly nnz entries (documents of up to 40 words, the last one cut; a few empty documents between)"""
    rng = np.random.default_rng(seed)
    docs, left = [], nnz
    while left > 0:
        n = min(left, int(rng.integers(1, 41)))
        docs.append(rng.choice(V, size=n, replace=False))
        left -= n
        if len(docs) % 9 == 0:
            docs.append([])
    return docs or [[], [], []]


def _table():
    T = []

    def add(name, V, docs, min_df=1, max_df=0, keep_n=0, aim="", device=True, counts=None):
        offs, rows, cnt = csc(V, docs, counts)
        T.append(Case(name, V, offs, rows, cnt, min_df, max_df, keep_n, aim, device))

    # ---- the rule's edges: small, also on the device
    # df: w0 5, w1 3, w2 3, w3 3, w4 1, w5 0, w6 2, w7 0
    small = [[0, 1, 2, 3], [0, 1, 2, 3, 6], [0, 1, 2, 3, 6], [0, 4], [0], []]
    add("ties_cut_inside", 8, small, keep_n=2, aim="tie")          # w0, then the smallest id of three words with df 3
    add("ties_cut_inside_3", 8, small, keep_n=3, aim="tie")
    add("keep_n_equals_passers", 8, small, keep_n=6, aim="keep_n")
    add("keep_n_one_below", 8, small, keep_n=5, aim="keep_n")      # the df = 1 word goes
    add("keep_n_above", 8, small, keep_n=7, aim="keep_n")
    add("keep_n_one", 8, small, keep_n=1, aim="keep_n")
    add("min_equals_max", 8, small, min_df=3, max_df=3, aim="band")
    add("min_zero_keeps_absent", 8, small, min_df=0, aim="absent")  # w5 and w7 stay: ids unchanged, A bit-equal
    add("min_zero_max_small", 8, small, min_df=0, max_df=1, aim="absent")
    add("max_df_none_is_doc_count", 8, small + [[0]], min_df=6, aim="band")  # df[w0] = 6 = 7 documents - 1
    add("refuse_min_above_max", 8, small, min_df=4, max_df=3, aim="refusal")
    add("refuse_min_above_docs", 8, small, min_df=7, aim="refusal")
    add("refuse_keep_n_2_32", 8, small, keep_n=2 ** 32, aim="refusal")
    add("refuse_nothing_kept", 8, small, min_df=4, max_df=4, aim="refusal")
    # ---- the scan's tile edges, nnz = 0 with D > 0 among them
    add("nnz_0", 50, [[], [], [], []], min_df=0, aim="nnz")
    for nnz in (SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 2 * SCAN_TILE + 1):
        add("nnz_%d" % nnz, 700, _exact_nnz(700, nnz, nnz), min_df=3, max_df=40, aim="nnz")
    # ---- the vocabulary at the edges of the LDS parts: words either side of every part boundary occur
    for V in (PART - 1, PART, PART + 1, 2 * PART + 3):
        edge = [w for w in (0, 1, PART - 2, PART - 1, PART, PART + 1, 2 * PART - 1, 2 * PART, 2 * PART + 1, 2 * PART + 2, V - 2, V - 1) if w < V]
        add("V_%d" % V, V, _zipf_docs(V, 3000, V, must=edge), min_df=2, aim="part")
    # ---- a head word in every one of 70 000 documents, a second in all but one: df > 65 535, the head maximally contended
    D = 70000
    head = [[0, 1, 2 + d % 50] for d in range(D)]
    head[12345] = [0, 2]
    add("head_70000", 60, head, min_df=2, max_df=D - 1, aim="head")             # word 0 (df = D) goes, word 1 (df = D - 1) stays
    # ---- documents: empty ones at both ends, a run of 2000 empty ones, documents that lose all / the first / the last entry
    docs = [[]] + [[5, 6, 7]] * 3 + [[]] * 2000 + [[1, 5, 6], [5, 6, 9], [1, 9], [5, 6, 7], [2, 5, 6, 7]] + [[5, 7]] * 2 + [[]]
    add("documents", 10, docs, min_df=2, aim="documents")                      # w1 and w9 (df 2) stay, w2 (df 1) goes ...
    add("documents_lose", 10, docs, min_df=3, aim="documents")                 # ... here w1, w2 and w9 go: [1, 9] loses all, [1, 5, 6] its first, [5, 6, 9] its last
    add("one_document_all_words", 5000, [np.arange(5000)] + [np.arange(0, 5000, 2)], min_df=2, aim="documents")
    # ---- counts: fractional, above 2^24, and bit patterns that no integer has
    rng = np.random.default_rng(11)
    cd = _zipf_docs(900, 400, 11)
    n = int(sum(np.unique(d).size for d in cd))
    cnt = np.where(rng.random(n) < 0.3, rng.random(n).astype(np.float32) * 3 + np.float32(0.125), np.float32(1)).astype(np.float32)
    cnt[::5] = np.float32(2 ** 24) + np.float32(2) * rng.integers(1, 1000, size=cnt[::5].size).astype(np.float32)
    cnt[1::11] = np.float32(4294967040.0)
    add("counts", 900, cd, min_df=2, max_df=150, counts=cnt, aim="counts")
    add("keeps_everything", 900, cd, min_df=0, counts=cnt, aim="identity")
    return T


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
DEVICE = [c for c in CASES if c.device]

# ---- document shards: cuts by world; the table's cases cut so that a word reaches min_df = 2 only summed over two ranks, one rank has no
# documents and one has documents and no entries
_sh = [[], [], [1, 3], [3, 4], [2, 3, 4], [2, 4, 5], [0, 4], [0, 5, 6], [0, 6]]   # df: w0 3, w1 1, w2 2, w3 3, w4 4, w5 2, w6 2
SHARDED = [Case("sh_min_df_across_ranks", 8, *csc(8, _sh), 2, 0, 0, "shard", True),
           Case("sh_keep_n_ties", 8, *csc(8, _sh), 1, 0, 3, "shard", True),      # w4, then w0 before w3 (df 3 both)
           Case("sh_zipf", 3000, *csc(3000, _zipf_docs(3000, 1500, 5)), 3, 400, 700, "shard", True)]
SHARD_REFUSAL = Case("sh_nothing_kept", 8, *csc(8, _sh), 5, 0, 0, "refusal", True)


def cuts(case, world):
    D = case.offs.size - 1
    if world == 1:
        return [0, D]
    if D == 9:   # _sh: w2 lies in documents 4 and 5, one either side of the cut at 5: df 1 on each of two ranks, 2 summed
        return [0, 5, 9] if world == 2 else [0, 2, 2, 9]   # three ranks: rank 0 has documents and no entries, rank 1 no documents
    return [0, D // 2, D] if world == 2 else [0, D // 3, D // 3, D]
