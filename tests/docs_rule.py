"""The rule of isle_hip_doc_lengths / isle_hip_doc_duplicates / isle_hip_prune_docs (include/isle_hip.h, isle_amd/csrc/docs_host.h) in numpy,
and the case table the document-prune tests share (a plain module: no torch, no GPU, no library).  A count crosses as its 32 bits.

  words[d]   the entries of document d               tokens[d]  the sum of (uint64)count over them
  passes     min_words <= words <= max_words' and min_tokens <= tokens <= max_tokens' (a maximum of 0: no bound)
  equal      the same rows and the same count BITS, entry by entry; all empty documents are equal
  first_of   with drop_duplicates the smallest document equal to d, else d          kept   passes and first_of[d] == d
  new A      the kept documents' columns in ascending old id, bit for bit; kept_docs[new] = doc_offset + old
  reported   first_of = 0xffffffff where dropped by length; dropped = [below, above, duplicate], the first failing test of
             words-min, tokens-min, words-max, tokens-max deciding"""
from collections import namedtuple

import numpy as np

SCAN_TILE = 4096        # scan.h
SORT_TILE = 2048        # ingest.hip: the radix sort's keys per workgroup
DROPPED = 0xFFFFFFFF    # docs_host.h DOCS_DROPPED (test_docs_rule_cpu.py holds these copies to the header through docs_host_main)
NARROW_BITS = 2         # docs_host.h DOCS_NARROW_BITS
BIG = np.float32(4294967040.0)   # the largest float below 2^32

Case = namedtuple("Case", "name V offs rows counts min_words max_words min_tokens max_tokens dups aim")


def default_count(w):
    """a count that depends on the word alone: documents with the same rows are equal"""
    return (1 + (np.asarray(w, np.int64) * 7 + 3) % 9).astype(np.float32)


def csc(V, docs):
    """docs: per document a collection of word ids, or (word ids ascending, counts) -> (offs int64, rows uint32, counts float32)"""
    offs = np.zeros(len(docs) + 1, np.int64)
    rows, counts = [], []
    for d, doc in enumerate(docs):
        if isinstance(doc, tuple):
            w, c = np.asarray(doc[0], np.int64), np.asarray(doc[1], np.float32)
            assert w.size == c.size and (np.diff(w) > 0).all()
        else:
            w = np.unique(np.asarray(doc, np.int64))
            c = default_count(w)
        assert w.size == 0 or (0 <= w[0] and w[-1] < V)
        rows.append(w)
        counts.append(c)
        offs[d + 1] = offs[d] + w.size
    rows = np.concatenate(rows).astype(np.uint32) if rows else np.zeros(0, np.uint32)
    counts = np.concatenate(counts).astype(np.float32) if counts else np.zeros(0, np.float32)
    assert (counts > 0).all()
    return offs, rows, counts


# ---- the hash the device sorts by (docs_host.h docs_mix / docs_entry_hash / docs_hash_host): only to BUILD cases that collide for certain
_M = (1 << 64) - 1


def mix(x):
    x = (x + 0x9E3779B97F4A7C15) & _M
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M
    return x ^ (x >> 31)


def doc_hash(rows, count_bits):
    return sum(mix((int(r) << 32) | int(b)) for r, b in zip(rows, count_bits)) & _M


def narrow_key(words):
    w = np.unique(np.asarray(words, np.int64))
    return doc_hash(w, default_count(w).view(np.uint32)) & ((1 << NARROW_BITS) - 1)


# ---- the rule
def lengths(offs, counts):
    """-> (words uint32, tokens uint64)"""
    c = np.concatenate([np.zeros(1, np.uint64), np.cumsum(counts.astype(np.uint64), dtype=np.uint64)])
    return np.diff(offs).astype(np.uint32), c[offs[1:]] - c[offs[:-1]]


def first_of(offs, rows, counts):
    """the smallest document with the same content, by content alone (a dictionary of the bytes) -> uint32 (D,)"""
    bits = counts.view(np.uint32)
    seen, out = {}, np.empty(offs.size - 1, np.uint32)
    for d in range(offs.size - 1):
        s, e = int(offs[d]), int(offs[d + 1])
        out[d] = seen.setdefault(rows[s:e].tobytes() + bits[s:e].tobytes(), d)
    return out


def check_args(min_words, max_words, min_tokens, max_tokens, dups, world=1, who="prune_docs", has_A=True):
    """the refusals that need no table: '' = accepted"""
    if not has_A:
        return "%s: no count matrix" % who
    if dups not in (0, 1):
        return "%s: drop_duplicates = %d, neither 0 nor 1" % (who, dups)
    if dups and world > 1:
        return "%s: duplicates with %d ranks: equality across ranks needs the contents exchanged" % (who, world)
    if max_words and min_words > max_words:
        return "%s: min_words = %d > max_words = %d" % (who, min_words, max_words)
    if max_tokens and min_tokens > max_tokens:
        return "%s: min_tokens = %d > max_tokens = %d" % (who, min_tokens, max_tokens)
    return ""


def none_kept(c):
    return "prune_docs: no document kept (min_words = %d, max_words = %d, min_tokens = %d, max_tokens = %d, drop_duplicates = %d)" % (
        c.min_words, c.max_words, c.min_tokens, c.max_tokens, c.dups)


def fails(words, tokens, c):
    """0 passes, 1 below, 2 above: the first failing test"""
    w, t = words.astype(np.uint64), tokens
    below = (w < c.min_words) | (t < c.min_tokens)
    above = ((w > c.max_words) if c.max_words else np.zeros(w.size, bool)) | ((t > c.max_tokens) if c.max_tokens else np.zeros(w.size, bool))
    return np.where(below, 1, np.where(above, 2, 0))


def rule(case, doc_offset=0):
    """What the three calls answer for the case as one rank holds it."""
    D = case.offs.size - 1
    words, tokens = lengths(case.offs, case.counts)
    all_first = first_of(case.offs, case.rows, case.counts)
    out = dict(words=words, tokens=tokens, all_first_of=all_first, n_duplicates=int((all_first != np.arange(D)).sum()))
    out["text"] = check_args(case.min_words, case.max_words, case.min_tokens, case.max_tokens, case.dups)
    if out["text"]:
        return out
    f = fails(words, tokens, case)
    first = all_first.copy() if case.dups else np.arange(D, dtype=np.uint32)
    dup = (f == 0) & (first != np.arange(D))
    keep = (f == 0) & ~dup
    first[f != 0] = DROPPED
    out.update(keep=keep, first_of=first, dropped=[int((f == 1).sum()), int((f == 2).sum()), int(dup.sum())], docs=int(keep.sum()))
    if not keep.any():
        out["text"] = none_kept(case)
        return out
    lens = np.diff(case.offs)
    entry = np.repeat(keep, lens)
    new_offs = np.concatenate([[0], np.cumsum(lens[keep])]).astype(np.int64)
    out.update(kept_docs=(doc_offset + np.flatnonzero(keep)).astype(np.uint32), offs=new_offs, rows=case.rows[entry], counts=case.counts[entry].view(np.uint32),
               nnz=int(entry.sum()), docs_global=int(keep.sum()))
    return out


def share(case, cut, rank):
    """rank's documents [cut[rank], cut[rank + 1]) of the case -> (offs, rows, counts, doc_offset)"""
    b, e = int(cut[rank]), int(cut[rank + 1])
    lo, hi = int(case.offs[b]), int(case.offs[e])
    return case.offs[b:e + 1] - lo, case.rows[lo:hi], case.counts[lo:hi], b


def rule_share(case, cut, rank):
    """rank's slice of the single-rank result: (offs, rows, count bits, kept_docs, new doc_offset)"""
    want = rule(case)
    b, e = int(cut[rank]), int(cut[rank + 1])
    nb, ne = int(want["keep"][:b].sum()), int(want["keep"][:e].sum())
    lo, hi = int(want["offs"][nb]), int(want["offs"][ne])
    return want["offs"][nb:ne + 1] - lo, want["rows"][lo:hi], want["counts"][lo:hi], want["kept_docs"][nb:ne], nb


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------
def _pool_docs(V, D, seed, contents=48):
    """D documents drawn from a pool of few distinct contents (0 .. 6 words each): many duplicates, and in the narrow form a run holds at
    most the pool's contents, so the rounds stay few"""
    rng = np.random.default_rng(seed)
    pool = [rng.choice(V, size=int(rng.integers(0, 7)), replace=False) for _ in range(contents)]
    return [pool[i] for i in rng.integers(0, contents, size=D)]


def _colliding(V, per_key=3):
    """per narrow key, per_key distinct two-word contents with that key"""
    found = {k: [] for k in range(1 << NARROW_BITS)}
    for a in range(V - 1):
        doc = [a, a + 1]
        k = narrow_key(doc)
        if len(found[k]) < per_key:
            found[k].append(doc)
    assert all(len(v) == per_key for v in found.values())
    return found


def _table():
    T = []

    def add(name, V, docs, min_words=0, max_words=0, min_tokens=0, max_tokens=0, dups=0, aim=""):
        T.append(Case(name, V, *csc(V, docs), min_words, max_words, min_tokens, max_tokens, dups, aim))

    # ---- the rule's edges.  (words, tokens): e0 (0, 0)  e1 (1, 3)  e2 (2, 2)  e3 (5, 5)  e4 (1, 1000)  e5 (3, 4: 2 + 2.5 + 0.5 truncated)  e6 (4, 4)
    edge = [([], []), ([1], [3]), ([1, 2], [1, 1]), ([0, 1, 2, 3, 4], [1] * 5), ([7], [1000]), ([0, 1, 2], [2, 2.5, 0.5]), ([3, 4, 5, 6], [1] * 4)]
    add("bounds_equal_a_length", 12, edge, min_words=2, max_words=4, aim="edge")
    add("min_equals_max", 12, edge, min_words=3, max_words=3, aim="edge")
    add("max_zero_is_none", 12, edge, min_words=1, aim="edge")
    add("fails_a_minimum_and_a_maximum", 12, edge, min_words=2, max_tokens=500, aim="edge")      # e4: one word, 1000 tokens: below
    add("tokens_min_before_words_max", 12, edge, min_tokens=5, max_words=2, aim="edge")           # e6: 4 tokens, 4 words: below; e3: above
    add("words_only", 12, edge, max_words=1, aim="edge")
    add("tokens_only", 12, edge, min_tokens=3, max_tokens=5, aim="edge")
    add("tokens_min_equals_max", 12, edge, min_tokens=4, max_tokens=4, aim="edge")
    add("refuse_min_words_above_max", 12, edge, min_words=5, max_words=4, aim="refusal")
    add("refuse_min_tokens_above_max", 12, edge, min_tokens=9, max_tokens=8, aim="refusal")
    add("refuse_nothing_kept", 12, edge, min_words=6, aim="refusal")
    add("refuse_nothing_kept_band", 12, edge, min_tokens=6, max_tokens=999, aim="refusal")
    # ---- equality's edges
    up = np.nextafter(np.float32(1), np.float32(2))
    eq = [[1, 2, 3], [1, 2, 3],                                       # 0, 1: a pair, adjacent
          [4, 5], [7, 8, 9], [10, 11], [], [],                        # 2: first of a far pair; 4: first of a triple; 5, 6: empty
          ([20, 21], [1, 1]), ([20, 21], [1, up]),                    # 7, 8: the same rows, one count differs in its last bit
          [10, 11],                                                   # 9: the triple's second
          ([30, 31, 32], [2, 2, 2]), ([30, 31, 33], [2, 2, 2]), ([29, 31, 32], [2, 2, 2]),   # 10, 11, 12: the last row differs, the first row differs
          [10, 11], [],                                               # 13: the triple's third; 14: empty
          ([40, 41], [3, 4]), ([40, 41, 42], [3, 4, 5]),              # 15, 16: a strict prefix of the other
          [4, 5],                                                     # 17: the far pair's second
          ([44, 45], [0.625, BIG]), ([46, 47], [BIG, BIG]), ([44, 45], [0.625, BIG]), ([46, 47], [BIG, BIG])]   # 18 .. 21: fractional bits, tokens > 2^32
    add("equality", 50, eq, dups=1, aim="equality")
    add("equality_min_words_1", 50, eq, min_words=1, dups=1, aim="equality")    # no empty document stays
    add("equality_not_asked", 50, eq, aim="equality")
    add("equality_and_bounds", 50, eq, min_words=2, max_words=2, max_tokens=2 ** 32, dups=1, aim="equality")
    # ---- collisions made certain: in the narrow form every run alternates three contents of its key, X, Y, Z, X, Y, Z, ...
    col = _colliding(200)
    add("alternating_runs", 200, [col[d % 4][(d // 4) % 3] for d in range(300)], dups=1, aim="collide")
    # ---- the sort's and the scan's tiles
    for D in (SORT_TILE - 1, SORT_TILE, SORT_TILE + 1, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 2 * SCAN_TILE + 1):
        add("D_%d" % D, 300, _pool_docs(300, D, D), min_words=1, max_words=5, dups=1, aim="tile")
    add("D_4097_not_asked", 300, _pool_docs(300, SCAN_TILE + 1, 7), min_words=2, max_tokens=25, aim="tile")
    add("nnz_0", 9, [[]] * 5, dups=1, aim="nnz")
    add("nnz_0_not_asked", 9, [[]] * 5, aim="nnz")
    # ---- a document and the wave: 63, 64, 65 and 5000 entries, each twice; two of 5000 entries that differ in the last entry only
    long_rows = np.arange(0, 5000)
    long_cnt = default_count(long_rows)
    other_cnt = long_cnt.copy()
    other_cnt[-1] += 1
    wave = [np.arange(63), np.arange(64), np.arange(65), long_rows, (long_rows, other_cnt), np.arange(65), np.arange(64), np.arange(63), long_rows,
            (np.append(long_rows[:-1], 5001), long_cnt)]
    add("wave", 6000, wave, dups=1, aim="wave")
    add("wave_bounds", 6000, wave, min_words=64, max_words=5000, max_tokens=int(long_cnt.sum()), dups=1, aim="wave")
    # ---- empty documents at both ends and in a run of 2000
    add("empties", 10, [[]] + [[5, 6, 7]] * 3 + [[]] * 2000 + [[1, 5, 6], [5, 6, 9], [1, 9], [5, 6, 7]] + [[5, 7]] * 2 + [[]], dups=1, aim="empty")
    add("empties_min_words_1", 10, [[]] + [[5, 6, 7]] * 3 + [[]] * 2000 + [[1, 5, 6], [5, 6, 9], [1, 9], [5, 6, 7]] + [[5, 7]] * 2 + [[]], min_words=1, aim="empty")
    # ---- 70 000 copies of a one-word document: a 16-bit counter anywhere would wrap, one run holds everything
    add("copies_70000", 5, [[3]] * 70000, dups=1, aim="copies")
    # ---- identity: every document stays, A bit-equal
    uniq = [[d, 600 + d % 7, 700 + (d * d) % 500] for d in range(500)]
    add("identity", 1300, uniq, dups=1, aim="identity")
    add("identity_not_asked", 1300, uniq + [[1, 601, 701]], aim="identity")
    return T


CASES = _table()
BY_NAME = {c.name: c for c in CASES}

# ---- document shards (drop_duplicates off: the only sharded form)
_sh_a = [[1], [2], [1, 3, 5], [3, 4], [2, 3, 4], [2, 4, 5, 6], [0], [0, 5, 6], [0, 6, 7]]                                    # the first two: one word
_sh_b = [[0, 1, 2, 3, 4, 5]] * 2 + [[1, 2, 3, 4, 5, 6, 7]] * 3 + [[1, 2], [3], [], [4, 5, 6]]                                # the first five: too long
_rng = np.random.default_rng(5)
_sh_c = [_rng.choice(400, size=int(_rng.integers(0, 40)), replace=False) for _ in range(1500)]
SHARDED = [Case("sh_low_ranks_all_dropped", 8, *csc(8, _sh_a), 2, 0, 0, 0, 0, "shard"),
           Case("sh_rank_left_with_nothing", 8, *csc(8, _sh_b), 1, 5, 0, 0, 0, "shard"),
           Case("sh_random", 400, *csc(400, _sh_c), 3, 30, 20, 150, 0, "shard")]
SHARD_REFUSAL = Case("sh_nothing_kept", 8, *csc(8, _sh_a), 5, 0, 0, 0, 0, "refusal")


def cuts(case, world):
    D = case.offs.size - 1
    if world == 1:
        return [0, D]
    if D == 9:   # world 2: rank 0 holds the first five documents; world 3: rank 0 the first two, rank 1 none
        return [0, 5, 9] if world == 2 else [0, 2, 2, 9]
    return [0, D // 2, D] if world == 2 else [0, D // 3, D // 3, D]
