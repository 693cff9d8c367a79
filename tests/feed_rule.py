"""The plain rule of the triple feed (isle_hip_feed_begin / _entries / _finalize): entries in the order they were offered -> count matrix
A (CSC).  No GPU, no torch.

  skipped   an entry with count 0 is dropped before anything else: it takes no part in duplicate resolution.
  order     the others sorted by (doc, word), stably: entries with the same (doc, word) stay in the order they were offered.
  first     of several entries with the same (doc, word) the one offered first survives.
  offsets   over all D columns, empty documents included.
  counts    become float32 by round-to-nearest-even (what np.float32 does): 4294967295 -> 4294967296.0.

base_corpus() is the corpus the feed tests share: repeated pairs with different counts, zero counts, some of them ahead of a non-zero
entry of the same pair."""
import numpy as np


def feed_rule(docs, words, counts, D):
    """0-based docs / words and counts in offered order -> (counts_f32, rows_u32, offs_i64)."""
    docs = np.asarray(docs, np.int64).reshape(-1)
    words = np.asarray(words, np.int64).reshape(-1)
    counts = np.asarray(counts, np.uint64).reshape(-1)
    keep = counts != 0
    docs, words, counts = docs[keep], words[keep], counts[keep]
    order = np.lexsort((np.arange(len(docs)), words, docs))   # position last: the first offered leads its group
    docs, words, counts = docs[order], words[order], counts[order]
    first = np.ones(len(docs), bool)
    first[1:] = (docs[1:] != docs[:-1]) | (words[1:] != words[:-1])
    docs, words, counts = docs[first], words[first], counts[first]
    offs = np.zeros(D + 1, np.int64)
    offs[1:] = np.cumsum(np.bincount(docs, minlength=D))
    return counts.astype(np.float32), words.astype(np.uint32), offs


BASE_V, BASE_D = 300, 500


def base_corpus():
    """-> (docs, words, counts) uint32, about 6000 entries in shuffled order over 300 words x 500 documents: 5600 distinct pairs, 300 of
    them offered a second time with another count (about 5 %), 100 zero counts among the shuffled entries (60 on pairs of their own, 40 on
    pairs that also have a non-zero entry) and 20 more zero counts at the very front on pairs whose non-zero entry comes later (about 2 %
    in all)."""
    rng = np.random.default_rng(20240607)
    pair = rng.choice(BASE_V * BASE_D, 5660, replace=False)
    doc, word = pair // BASE_V, pair % BASE_V
    cnt = rng.integers(1, 50, 5660)
    cnt[5600:] = 0                                            # 60 pairs that only ever carry a zero
    again = rng.choice(5600, 300, replace=False)
    zero_on = rng.choice(5600, 40, replace=False)
    docs = np.concatenate([doc, doc[again], doc[zero_on]])
    words = np.concatenate([word, word[again], word[zero_on]])
    counts = np.concatenate([cnt, cnt[again] + 100, np.zeros(40, np.int64)])
    perm = rng.permutation(len(docs))
    docs, words, counts = docs[perm], words[perm], counts[perm]
    lead = rng.choice(5600, 20, replace=False)                # zero counts ahead of the pair's non-zero entry: it must survive
    docs = np.concatenate([doc[lead], docs])
    words = np.concatenate([word[lead], words])
    counts = np.concatenate([np.zeros(20, np.int64), counts])
    return docs.astype(np.uint32), words.astype(np.uint32), counts.astype(np.uint32)
