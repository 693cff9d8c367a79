"""The rule of isle_hip_doc_signatures / isle_hip_doc_jaccard / isle_hip_doc_near_duplicates / isle_hip_prune_near_docs (include/isle_hip.h,
isle_amd/csrc/neardup_host.h) in numpy and Python integers, and the case table the near-duplicate tests share (a plain module: no torch, no
GPU, no library).  Every quantity is an integer and every comparison made with it is ==.

  S_d        the rows of document d (counts are ignored), n_d their number
  similar    inter den >= num uni, inter = |S_a & S_b|, uni = n_a + n_b - inter (two empty documents are similar: 0 >= 0)
  nd_hash    mix(((i + 1) << 32) | w); sig[d][i] = min over S_d (all ones for an empty document)
  key[b][d]  k = 0; k = mix(k ^ sig[d][b rows_per_band + j]) for j = 0 .. rows_per_band - 1; the narrow form keeps its 2 low bits
  resolution band by band over the live documents (parent[d] == d), grouped by key: leader clustering in ascending document order, a
             document takes the first similar leader as its parent, else becomes a leader
  first_of   the root of the parent chain; kept <=> first_of[d] == d; pairs_tested the (document, leader) tests; rounds the largest number
             of leaders in a group, summed over the bands
  new A      the kept documents' columns in ascending old id, bit for bit; kept_docs[new] = doc_offset + old"""
from collections import namedtuple

import numpy as np

import docs_rule as dr   # csc, default_count, the tile sizes and the narrow width: one statement of each

KEY_AUTO, KEY_FULL, KEY_NARROW = 0, 1, 2     # neardup_host.h ND_KEY_* (test_neardup_rule_cpu.py holds these copies to the header)
MAX_BANDS, MAX_ROWS, MAX_H, MAX_DEN = 64, 8, 128, 65535
EMPTY_SIG = (1 << 64) - 1
FORMS = ("full", "narrow")
_M = (1 << 64) - 1

Case = namedtuple("Case", "name V offs rows counts num den bands rows_per_band pairs aim")


# ---- the hashes, on numpy uint64 (products wrap mod 2^64)
def mix(x):
    with np.errstate(over="ignore"):
        x = np.asarray(x, np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def nd_hash(i, w):
    return mix((np.uint64(i + 1) << np.uint64(32)) | np.asarray(w, np.uint64))


def signatures(offs, rows, H):
    """-> uint64 (D, H)"""
    D = offs.size - 1
    sig = np.full((D, H), EMPTY_SIG, np.uint64)
    full = np.flatnonzero(np.diff(offs) > 0)
    if full.size:
        r = rows.astype(np.uint64)
        for i in range(H):
            sig[full, i] = np.minimum.reduceat(nd_hash(i, r), offs[full])   # the starts of the non-empty documents cut the entries exactly
    return sig


def band_keys(sig, bands, rows_per_band):
    """-> uint64 (bands, D), not cut"""
    keys = np.zeros((bands, sig.shape[0]), np.uint64)
    for b in range(bands):
        for j in range(rows_per_band):
            keys[b] = mix(keys[b] ^ sig[:, b * rows_per_band + j])
    return keys


def cut(keys, form):
    return keys & np.uint64((1 << dr.NARROW_BITS) - 1) if form == "narrow" else keys


def check_args(who, has_A=True, num=1, den=1, bands=1, rows_per_band=1, world=1):
    """the refusals: '' = accepted"""
    if not has_A:
        return "%s: no count matrix" % who
    if world > 1:
        return "%s: near duplicates with %d ranks: similarity across ranks needs the contents exchanged: out of scope" % (who, world)
    if num < 1 or num > den or den > MAX_DEN:
        return "%s: threshold %d/%d, not 1 <= num <= den <= %d" % (who, num, den, MAX_DEN)
    if bands < 1 or bands > MAX_BANDS or rows_per_band < 1 or rows_per_band > MAX_ROWS or bands * rows_per_band > MAX_H:
        return "%s: bands = %d, rows_per_band = %d, not 1 <= bands <= %d, 1 <= rows_per_band <= %d, bands rows_per_band <= %d" % (
            who, bands, rows_per_band, MAX_BANDS, MAX_ROWS, MAX_H)
    return ""


def bad_pair(at, a, b, D):
    return "doc_jaccard: pair %d names documents %d and %d of %d" % (at, a, b, D)


def jaccard(offs, rows, pairs):
    """-> (inter uint32 (n,), uni uint32 (n,))"""
    inter = np.array([np.intersect1d(rows[offs[a]:offs[a + 1]], rows[offs[b]:offs[b + 1]], assume_unique=True).size for a, b in pairs], np.uint32)
    n = np.diff(offs)
    p = np.asarray(pairs, np.int64).reshape(-1, 2)
    return inter, (n[p[:, 0]] + n[p[:, 1]] - inter).astype(np.uint32)


def lengths_allow(na, nb, num, den):
    return min(na, nb) * den >= num * max(na, nb)


def similar(inter, na, nb, num, den):
    return inter * den >= num * (na + nb - inter)


def resolve(offs, rows, keys, form, num, den, trace=None):
    """keys (bands, D) uncut -> (parent uint32, first_of uint32, pairs_tested, rounds).  trace: a list that receives
    (band, document, leader, allowed by the lengths, similar) per test."""
    D = offs.size - 1
    n = np.diff(offs).tolist()
    content, cid = {}, np.empty(D, np.int64)     # equal word sets answer alike: one intersection per pair of contents
    for d in range(D):
        cid[d] = content.setdefault(rows[offs[d]:offs[d + 1]].tobytes(), d)
    cid = cid.tolist()
    known = {}

    def test(d, l):
        if not lengths_allow(n[d], n[l], num, den):
            return False, False
        at = (cid[d], cid[l])
        if at not in known:
            known[at] = int(np.intersect1d(rows[offs[d]:offs[d + 1]], rows[offs[l]:offs[l + 1]], assume_unique=True).size)
        return True, similar(known[at], n[d], n[l], num, den)

    parent = list(range(D))
    pairs_tested = rounds = 0
    for b in range(keys.shape[0]):
        k = cut(keys[b], form).tolist()
        leaders, most = {}, 0
        for d in range(D):
            if parent[d] != d:
                continue
            ls = leaders.setdefault(k[d], [])
            for l in ls:
                pairs_tested += 1
                allowed, sim = test(d, l)
                if trace is not None:
                    trace.append((b, d, l, allowed, sim))
                if sim:
                    parent[d] = l
                    break
            else:
                ls.append(d)
                most = max(most, len(ls))
        rounds += most
    first = list(range(D))
    for d in range(D):
        if parent[d] != d:
            first[d] = first[parent[d]]
    return np.array(parent, np.uint32), np.array(first, np.uint32), pairs_tested, rounds


_RULES = {}


def rule(case, form, doc_offset=0):
    """What the calls answer for the case in one form of the key (computed once per (case, form, doc_offset); treat it as read-only)."""
    at = (case.name, form, doc_offset)
    if at in _RULES:
        return _RULES[at]
    D = case.offs.size - 1
    out = dict(text=check_args("doc_near_duplicates", True, case.num, case.den, case.bands, case.rows_per_band))
    if out["text"]:
        _RULES[at] = out
        return out
    sig = signatures(case.offs, case.rows, case.bands * case.rows_per_band)
    keys = band_keys(sig, case.bands, case.rows_per_band)
    trace = []
    parent, first, tested, rounds = resolve(case.offs, case.rows, keys, form, case.num, case.den, trace)
    keep = first == np.arange(D)
    inter, uni = jaccard(case.offs, case.rows, case.pairs)
    lens = np.diff(case.offs)
    entry = np.repeat(keep, lens)
    out.update(sig=sig, keys=keys, parent=parent, first_of=first, keep=keep, n_dropped=int((~keep).sum()), pairs_tested=tested, rounds=rounds, trace=trace,
               inter=inter, uni=uni, docs=int(keep.sum()), kept_docs=(doc_offset + np.flatnonzero(keep)).astype(np.uint32),
               offs=np.concatenate([[0], np.cumsum(lens[keep])]).astype(np.int64), rows=case.rows[entry], counts=case.counts[entry].view(np.uint32),
               nnz=int(entry.sum()))
    _RULES[at] = out
    return out


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------
def _key0(words, bands, rows_per_band):
    """the narrow key of band 0 of one word set"""
    w = np.unique(np.asarray(words, np.int64))
    offs = np.array([0, w.size], np.int64)
    return int(cut(band_keys(signatures(offs, w.astype(np.uint32), bands * rows_per_band), bands, rows_per_band)[0], "narrow")[0])


def _together(make, bands, rows_per_band, start=0, step=1, tries=4000):
    """make(shift) -> word sets; the first shift from start at which all of them share band 0's narrow key, so that the narrow form tests
    them against each other for certain -> (shift, word sets)"""
    for s in range(start, start + tries * step, step):
        docs = make(s)
        if len({_key0(d, bands, rows_per_band) for d in docs}) == 1:
            return s, docs
    raise AssertionError("no shift puts the documents into one group")


def _length_docs():
    """documents of 0, 1, 63, 64, 65 and 5000 entries, each with a copy and near copies; empty documents at both ends"""
    big = np.arange(100, 5100)
    docs = [[], [7]]
    for n in (63, 64, 65):
        base = np.arange(1000, 1000 + n)
        docs += [base, base[:-1], np.append(base[1:], 3000 + n)]     # n, a subset of n - 1, one word replaced
    docs += [big, big[:-1], np.append(big[:4000], np.arange(6000, 7000)),   # 5000; 4999 of them; inter 4000, uni 6000
             np.append(big[500:], np.arange(7000, 7500)),                   # inter 4500, uni 5500: 4500 5 = 22500 >= 4 5500 = 22000
             [7], np.arange(1000, 1064), [], big, []]
    return docs


def _threshold_docs(bands, rows_per_band):
    """pairs on and off the threshold 4/5 and on and off the length filter's boundary, each pair (or triple) in word ids of its own and
    shifted until the narrow form puts it into one group.  -> (docs, named: name -> document numbers)"""
    docs, named = [], {}

    def put(name, make, base):
        _, got = _together(lambda s: make(base + 40 * s), bands, rows_per_band)
        named[name] = list(range(len(docs), len(docs) + len(got)))
        docs.extend(got)

    put("on_threshold", lambda o: [np.arange(o, o + 5), np.arange(o, o + 4)], 0)                       # inter 4, uni 5: 20 >= 20, lengths 16 < 20? no: 4 5 >= 4 5
    put("below_threshold", lambda o: [np.arange(o, o + 4500), np.arange(o + 501, o + 5000)], 200000)   # inter 3999, uni 5000: 19995 < 20000
    put("above_threshold", lambda o: [np.arange(o, o + 4500), np.arange(o + 500, o + 5000)], 600000)   # inter 4000, uni 5000: 20000 >= 20000
    put("filter_on", lambda o: [np.arange(o, o + 5), np.append(np.arange(o, o + 3), o + 9)], 1000000)  # lengths 4, 5 (on the boundary: read), inter 3, uni 6
    put("filter_off", lambda o: [np.arange(o, o + 6), np.arange(o, o + 4)], 1200000)                   # lengths 4, 6: 20 < 24, decided without reading; inter 4, uni 6
    put("filter_off_by_one", lambda o: [np.arange(o, o + 10), np.arange(o, o + 8), np.arange(o, o + 7)], 1400000)   # 8 of 10: on; 7 of 10: 35 < 40 filtered, 7 of 8: similar
    put("subset", lambda o: [np.arange(o, o + 20), np.arange(o, o + 20, 2), np.arange(o, o + 17)], 1600000)        # half (filtered), 17 of 20 (similar)
    put("disjoint", lambda o: [np.arange(o, o + 12), np.arange(o + 12, o + 24), np.arange(o + 6, o + 18)], 1800000)  # equal lengths: read, inter 0 and 6
    return docs, named


def _pool_docs(V, D, seed, bases=12):
    """D documents drawn from a pool of few contents: bases of 10 .. 14 words, each with a subset missing one word (similar at 4/5) and a
    variant with one word replaced (11 of 13 at 12 words: similar), two with three replaced (dissimilar), and the empty document"""
    rng = np.random.default_rng(seed)
    pool = [np.zeros(0, np.int64)]
    for _ in range(bases):
        base = np.sort(rng.choice(V - 50, size=int(rng.integers(10, 15)), replace=False))
        pool += [base, base[1:], np.append(base[:-1], V - 1 - int(rng.integers(0, 50)))]
        pool += [np.append(base[:-3], V - 50 + np.array([1, 2, 3]) + 4 * i) for i in range(2)]
    return [pool[i] for i in rng.integers(0, len(pool), size=D)]


def _alternating(bands, rows_per_band, per_key=3):
    """per narrow key of band 0, per_key mutually disjoint two-word sets with that key"""
    found = {k: [] for k in range(1 << dr.NARROW_BITS)}
    a = 0
    while any(len(v) < per_key for v in found.values()):
        k = _key0([a, a + 1], bands, rows_per_band)
        if len(found[k]) < per_key:
            found[k].append([a, a + 1])
        a += 2
    return found, a + 2


# The cross-band chain, FULL form: a document attaches in a band > 0 to a leader that attaches to another in a later band, so first_of differs
# from parent.  chain_docs(seed) draws a family of overlapping word sets; find_chain_seed() is the search that gave CHAIN_SEED.
CHAIN_BANDS, CHAIN_ROWS, CHAIN_NUM, CHAIN_DEN, CHAIN_SEED = 8, 1, 1, 2, 0


def chain_docs(seed, D=60, V=400):
    rng = np.random.default_rng(seed)
    base = rng.choice(V, size=30, replace=False)
    return [np.unique(np.append(rng.choice(base, size=int(rng.integers(14, 24)), replace=False), rng.choice(V, size=int(rng.integers(0, 6)), replace=False)))
            for _ in range(D)]


def chain_depth(case, form="full"):
    """(the longest parent chain, whether a document attached in a band > 0 to a parent that attached in a later band)"""
    r = rule(case, form)
    band_of = {d: b for b, d, l, _, sim in r["trace"] if sim}
    deep = any(r["parent"][d] != d and r["parent"][r["parent"][d]] != r["parent"][d] and band_of[d] > 0 and band_of[int(r["parent"][d])] > band_of[d]
               for d in range(case.offs.size - 1))
    depth = 0
    for d in range(case.offs.size - 1):
        n, x = 0, d
        while r["parent"][x] != x:
            x, n = int(r["parent"][x]), n + 1
        depth = max(depth, n)
    return depth, deep


def _chain_case(seed, name="cross_band_chain"):
    return Case(name, 400, *dr.csc(400, chain_docs(seed)), CHAIN_NUM, CHAIN_DEN, CHAIN_BANDS, CHAIN_ROWS, _default_pairs(60), "chain")


def find_chain_seed(limit=2000):
    for seed in range(limit):
        c = _chain_case(seed, "chain_search_%d" % seed)
        depth, deep = chain_depth(c)
        if depth >= 2 and deep:
            return seed
    raise AssertionError("no seed below %d gives a chain" % limit)


def _default_pairs(D, extra=()):
    """the pairs isle_hip_doc_jaccard is asked: neighbours, a document with itself, the two ends, and the case's own"""
    if D == 0:
        return np.zeros((0, 2), np.uint32)
    p = [(d, d + 1) for d in range(min(D - 1, 300))] + [(0, 0), (D - 1, D - 1), (D - 1, 0), (0, D - 1)] + [tuple(x) for x in extra]
    return np.array(p, np.uint32).reshape(-1, 2)


def _table():
    T = []

    def add(name, V, docs, num, den, bands, rows_per_band, aim, pairs=()):
        T.append(Case(name, V, *dr.csc(V, docs), num, den, bands, rows_per_band, _default_pairs(len(docs), pairs), aim))

    # ---- a document and the wave, under every lane-ownership edge of the signature kernel: H = 1, 63, 64, 65, 64 and 128
    ld = _length_docs()
    far = [(d, e) for d in (2, 5, 8, 11) for e in (11, 12, 13, 14, 18)]
    for bands, rpb in ((1, 1), (63, 1), (64, 1), (13, 5), (16, 4), (16, 8)):
        add("lengths_%dx%d" % (bands, rpb), 8000, ld, 4, 5, bands, rpb, "lengths", far)
    # ---- the threshold and the length filter, on and off
    td, named = _threshold_docs(16, 4)
    add("threshold_edges", 2200000, td, 4, 5, 16, 4, "threshold", [(v[0], x) for v in named.values() for x in v[1:]])
    global THRESHOLD_DOCS
    THRESHOLD_DOCS = named
    # ---- num == den: equal word sets and nothing else, whatever the counts
    eq = [[1, 2, 3], ([1, 2, 3], [5, 6, 7]), [1, 2], [1, 2, 3, 4], [], [9], [1, 2, 3], [], ([9], [2]), [1, 2, 4], [2, 3], [1, 2]]
    add("equal_sets_1x1", 12, eq, 1, 1, 1, 1, "equal")
    add("equal_sets_13x5", 12, eq, 7, 7, 13, 5, "equal")
    add("equal_sets_pool", 700, _pool_docs(700, 1500, 3), 65535, 65535, 16, 4, "equal")
    # ---- in the narrow form every group of band 0 alternates three mutually disjoint word sets X, Y, Z, X, Y, Z, ...
    alt, top = _alternating(2, 2)
    add("alternating_groups", top, [alt[d % 4][(d // 4) % 3] for d in range(300)], 4, 5, 2, 2, "alternate")
    # ---- a chain across bands (full form)
    T.append(_chain_case(CHAIN_SEED))
    # ---- one group of 70 000 copies: one leader, one round; a 16-bit counter anywhere would wrap
    add("copies_70000", 5, [[3]] * 70000, 4, 5, 1, 1, "copies")
    # ---- the sort's and the scan's tiles
    for D in (dr.SORT_TILE - 1, dr.SORT_TILE, dr.SORT_TILE + 1, dr.SCAN_TILE - 1, dr.SCAN_TILE, dr.SCAN_TILE + 1, 2 * dr.SCAN_TILE + 1):
        add("D_%d" % D, 700, _pool_docs(700, D, D), 4, 5, 16, 4, "tile")
    # ---- empty documents at both ends and in a run of 2000
    add("empties", 40, [[]] + [[5, 6, 7, 8, 9]] * 3 + [[]] * 2000 + [[5, 6, 7, 8], [5, 6, 9], [1, 9], [5, 6, 7, 8, 9, 10]] + [[5, 7]] * 2 + [[]], 4, 5, 16, 4, "empty")
    return T


THRESHOLD_DOCS = {}
CASES = _table()
BY_NAME = {c.name: c for c in CASES}


def recall_case(seed=1, pairs=200, V=60000):
    """200 planted pairs of Jaccard >= 0.9 among unrelated documents, at 16 x 4 and 4/5: every pair must end with a common first_of.  A pair
    of Jaccard s shares a band's key with probability s^4, so it is missed with (1 - 0.9^4)^16 = 4e-8."""
    rng = np.random.default_rng(seed)
    docs = []
    for _ in range(pairs):
        base = np.sort(rng.choice(V, size=int(rng.integers(40, 80)), replace=False))
        other = base.copy()
        other[:2] = V + rng.choice(V, size=2, replace=False)        # n words, 2 replaced: inter n - 2, uni n + 2, >= 38/42 > 0.9
        docs += [base, other]
    order = rng.permutation(len(docs))
    where = np.empty(len(docs), np.int64)
    where[order] = np.arange(len(docs))
    planted = [(int(where[2 * i]), int(where[2 * i + 1])) for i in range(pairs)]
    return Case("recall", 2 * V, *dr.csc(2 * V, [docs[i] for i in order]), 4, 5, 16, 4, np.array(planted, np.uint32), "recall")
