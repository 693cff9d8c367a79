"""The rule of isle_hip_topic_top_docs in numpy, a cutter of triples into rank shares, and the case table (a plain module, importable
without torch and without a GPU).  An entry is (row, topic, value bits); the document of a row is doc_base + row; per topic the entries go
by (ord(bits) descending, document ascending) and the first n are the result.  Nothing here reads isle_amd/csrc/topdocs_host.h: the table
is what tests/test_topdocs_rule_cpu.py holds the header's host statement to, and what the GPU tests hold the kernels to, bit for bit."""
import numpy as np

MAX_N = 256
IT_WIN = 1024
U32 = np.uint32


def f2b(values):
    return np.asarray(values, np.float32).view(U32).copy()


def ord_bits(bits):
    bits = np.asarray(bits, U32)
    return bits ^ np.where(bits >> U32(31), U32(0xFFFFFFFF), U32(0x80000000)).astype(U32)


class Case:
    """name, num_topics, n, doc_base, off int64 (rows + 1), topic uint32, bits uint32 (the values' bits), aim: what the case aims at (a key
    of test_topdocs_rule_cpu.AIMS), device: False where the C ABI refuses the call by its own limits (n > 256) and only the host statement runs"""

    def __init__(self, name, num_topics, n, doc_base, off, topic, bits, aim, device=True, **facts):
        self.name, self.num_topics, self.n, self.doc_base, self.aim, self.device, self.facts = name, int(num_topics), int(n), int(doc_base), aim, device, facts
        self.off = np.ascontiguousarray(off, np.int64)
        self.topic = np.ascontiguousarray(topic, U32)
        self.bits = np.ascontiguousarray(bits, U32)
        assert self.off[0] == 0 and self.off[-1] == self.topic.size == self.bits.size and (np.diff(self.off) >= 0).all()

    @property
    def rows(self):
        return self.off.size - 1

    @property
    def values(self):
        return self.bits.view(np.float32)

    def row_of_entry(self):
        return np.repeat(np.arange(self.rows, dtype=np.int64), np.diff(self.off))

    def at(self, n, device=True):
        return Case("%s_n%d" % (self.name, n), self.num_topics, n, self.doc_base, self.off, self.topic, self.bits, self.aim, device, **self.facts)


def rule(case):
    """-> dict(docs uint32 (T, n), values (bits) uint32 (T, n), counts uint32 (T,), topic_entries uint64 (T,))"""
    T, n = case.num_topics, case.n
    docs = np.full((T, n), 0xFFFFFFFF, U32)
    vals = np.zeros((T, n), U32)
    counts = np.zeros(T, U32)
    entries = np.zeros(T, np.uint64)
    doc = (case.doc_base + case.row_of_entry()).astype(np.int64)
    o = ord_bits(case.bits).astype(np.int64)
    order = np.lexsort((doc, -o, case.topic.astype(np.int64)))  # topic ascending, ord descending, document ascending
    tp = case.topic[order]
    first = np.searchsorted(tp, np.arange(T + 1))
    for t in range(T):
        sel = order[first[t]:first[t + 1]]
        m = min(n, sel.size)
        docs[t, :m] = doc[sel[:m]]
        vals[t, :m] = case.bits[sel[:m]]
        counts[t] = m
        entries[t] = sel.size
    return dict(docs=docs, values=vals, counts=counts, topic_entries=entries)


def cuts(case, world):
    """row bounds of `world` shares: two halves; three shares with an empty one in the middle — and, where the case begins with empty rows,
    the first share holds exactly those (rows and no entries)"""
    R = case.rows
    if world == 1:
        return [0, R]
    if world == 2:
        return [0, R // 2, R]
    lead = int(np.argmax(np.diff(case.off) > 0)) if case.topic.size else 0
    a = lead if lead > 0 else R // 3
    return [0, a, a, R]


def share(case, bounds, q):
    """-> (doc_base, off, topic, bits) of rows [bounds[q], bounds[q + 1]), offsets from 0"""
    b, e = bounds[q], bounds[q + 1]
    lo, hi = int(case.off[b]), int(case.off[e])
    return case.doc_base + b, case.off[b:e + 1] - lo, case.topic[lo:hi], case.bits[lo:hi]


# ---- builders -----------------------------------------------------------------------------------------------------------------------------------
def from_rows(rows):
    """rows: per row a list of (topic, bits), topics ascending -> off, topic, bits"""
    off = np.zeros(len(rows) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in rows])
    flat = [x for r in rows for x in r]
    return off, np.array([x[0] for x in flat], U32), np.array([x[1] for x in flat], U32)


def random_rows(seed, T, R=3000, lead=3):
    """R rows behind `lead` empty ones, each with a random subset of at most six topics; half of the positive values from a grid of 39
    numbers that reaches above the others, so that bit-equal values meet at the top of every topic"""
    rng = np.random.default_rng(seed)
    rows = [[] for _ in range(lead)]
    for _ in range(R):
        m = int(rng.integers(0, min(T, 6) + 1))
        tp = np.sort(rng.choice(T, m, replace=False))
        v = np.where(rng.random(m) < 0.5, rng.integers(1, 40, m) / 8.0, rng.random(m) * 4 + 1e-3).astype(np.float32)
        rows.append(list(zip(tp.tolist(), f2b(v).tolist())))
    return from_rows(rows)


def byte_rows(k, lead=3):
    """one topic, one entry per row, values that differ in byte k only (positive finite), in a shuffled order"""
    js = np.arange(1, 0x7F) if k == 3 else np.arange(256)
    bits = (U32(0x3F345678) & ~(U32(0xFF) << U32(8 * k))) | (js.astype(U32) << U32(8 * k))
    np.random.default_rng(10 + k).shuffle(bits)
    rows = [[] for _ in range(lead)] + [[(0, int(b))] for b in bits]
    return from_rows(rows)


def tie_rows(lead=3, R=700):
    """topic 1 in every row with one value; topic 0 in every third row, random"""
    rng = np.random.default_rng(7)
    one = int(f2b([0.375])[0])
    rows = [[] for _ in range(lead)]
    for r in range(R):
        rows.append(([(0, int(f2b([rng.random() + 0.5])[0]))] if r % 3 == 0 else []) + [(1, one)])
    return from_rows(rows)


SPECIALS = [0xBF800000, 0x80000000, 0x00000000, 0x00000001, 0x007FFFFF, 0x80000001, 0x7F800000, 0xFF800000, 0x7FC00000, 0x3F800000, 0x7F7FFFFF,
            0xFF7FFFFF, 0xC0000000, 0x00800000]  # -1, -0, +0, two denormals, a negative denormal, +inf, -inf, a NaN, 1, +-max, -2, the least normal


def special_rows():
    rows = []
    for i, b in enumerate(SPECIALS + SPECIALS[::-1]):  # topic 1 meets every pattern twice: the documents decide
        rows.append(([(0, SPECIALS[(3 * i) % len(SPECIALS)])] if i % 2 else []) + [(1, b)])
    return from_rows(rows)


def tile_rows(nnz, T=5):
    rng = np.random.default_rng(nnz)
    return from_rows([[(int(rng.integers(0, T)), int(f2b([rng.integers(1, 40) / 8.0])[0]))] for _ in range(nnz)])


def empty_run_rows():
    a, b = int(f2b([2.0])[0]), int(f2b([3.0])[0])
    return from_rows([[(0, a), (1, b), (2, a)]] + [[] for _ in range(IT_WIN + 76)] + [[(0, b), (2, b)]] + [[] for _ in range(5)] + [[(1, a)]])


def wide_row():
    rng = np.random.default_rng(1500)
    v = f2b(rng.integers(1, 30, 1500) / 4.0)
    return from_rows([[(t, int(v[t])) for t in range(1500)], [(t, int(v[(t * 7) % 1500])) for t in range(0, 1500, 3)], [], [(1499, int(v[0]))]])


def _cases():
    out = []
    one = from_rows([[(0, int(f2b([1.5])[0]))]])
    out.append(Case("one_entry_n1", 1, 1, 0, *one, aim="one"))
    out.append(Case("one_entry_n256", 1, 256, 0, *one, aim="one"))
    out.append(Case("no_rows", 3, 5, 11, *from_rows([]), aim="no_rows"))
    out.append(Case("rows_without_entries", 3, 5, 11, *from_rows([[], [], [], [], []]), aim="no_entries"))
    few = from_rows([[(0, 5), (1, 9)], [(1, 9), (3, 1)], [], [(0, 7), (1, 2)], [(0, 6)]] + [[(1, 100 + r)] for r in range(12)])
    out.append(Case("absent_topic_and_fewer_than_n", 4, 5, 0, *few, aim="fewer"))
    for T in (3, 64, 65, 257):
        base = Case("bins_T%d" % T, T, 1, 1000, *random_rows(T, T), aim="bins", lds=T <= 64)
        out += [base.at(n) for n in (1, 5, 32, 256)]
    for k in range(4):
        base = Case("value_byte%d" % k, 1, 5, 40, *byte_rows(k), aim="byte", byte=k)
        out += [base.at(5), base.at(100)]
    low = Case("tie_low_bytes", 2, 5, 0x10000 - 300, *tie_rows(), aim="tie", straddle=(1 << 8, 1 << 16))
    out += [low.at(5), low.at(256), low.at(300, device=False)]
    top = Case("tie_top_byte", 2, 5, 0xFFF00000, *tie_rows(), aim="tie", straddle=())
    out += [top.at(5), top.at(256), top.at(300, device=False)]
    sp = Case("specials", 2, 5, 3, *special_rows(), aim="specials")
    out += [sp.at(5), sp.at(32)]
    out += [Case("tile_%d_entries" % z, 5, 32, 0, *tile_rows(z), aim="tile", nnz=z) for z in (1023, 1024, 1025)]
    out.append(Case("empty_run", 3, 5, 9, *empty_run_rows(), aim="empty_run"))
    out.append(Case("row_of_1500", 1500, 5, 0, *wide_row(), aim="wide_row"))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
# the cases the sharded test cuts: ties, value bytes, the empty shapes and the bins' homes
SHARDED = [c.name for c in CASES if c.device and (c.aim in ("tie", "byte", "one", "no_rows", "no_entries", "fewer") or c.name in (
    "bins_T3_n5", "bins_T64_n256", "bins_T65_n32", "bins_T257_n1"))]


class Refusal:
    """a call through the caller's CSR that ISLE_E_ARG answers, and a piece of the text it gives"""

    def __init__(self, name, num_topics, n, doc_base, rows, text):
        self.name, self.num_topics, self.n, self.doc_base, self.text = name, num_topics, n, doc_base, text
        self.off, self.topic, self.bits = from_rows(rows)

    @property
    def values(self):
        return self.bits.view(np.float32)


def _refusals():
    ok = [[(0, 1), (2, 1)] for _ in range(1200)]  # entries 0 .. 2399: the bad ones lie in the second and third tile
    big = [list(r) for r in ok]
    big[700] = [(0, 1), (3, 1)]   # entry 1401
    big[1100] = [(1, 1), (3, 1)]  # entry 2201: the first one is named
    rep = [list(r) for r in ok]
    rep[600] = [(2, 1), (2, 1)]   # entry 1201 repeats its row's topic
    desc = [list(r) for r in ok]
    desc[1] = [(2, 1), (0, 1)]    # entry 3 descends
    desc[900] = [(2, 1), (1, 1)]
    return [
        Refusal("topic_is_num_topics", 3, 5, 0, big, "entry 1401 (row 700) has topic 3 >= num_topics 3"),
        Refusal("repeated_topic", 3, 5, 0, rep, "entry 1201 (row 600), topic 2: the topics of a row must ascend strictly"),
        Refusal("descending_pair", 3, 5, 0, desc, "entry 3 (row 1), topic 0: the topics of a row must ascend strictly"),
        Refusal("n_0", 3, 0, 0, ok, "n = 0 not in [1, 256]"),
        Refusal("n_257", 3, 257, 0, ok, "n = 257 not in [1, 256]"),
        Refusal("doc_base_too_large", 3, 5, 0xFFFFFFF1 - 1199, ok, "doc_base %d + 1200 rows exceed 4294967281" % (0xFFFFFFF1 - 1199)),
    ]


REFUSALS = _refusals()
