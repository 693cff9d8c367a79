"""The rule of isle_hip_topic_prevalence (include/isle_hip.h; isle_amd/csrc/prevalence_host.h) stated in numpy, elementwise over rows, and once
more in scalar Python, with the table of cases the CPU and the GPU tests share.

A row is a document's entries (topic, weight), topics ascending strictly; weights are fp32, finite, >= 0 and < 2^31, -0.0 counts as 0.
  rs_r          0.0, then rs_r + (double)w over the row's entries in stored order
  x_r(t)        (double)w, with normalise (double)w / rs_r (+0.0 where rs_r == 0); +0.0 where w == 0 and for a topic the row does not store
  dominant      the entry with the largest weight, the smaller topic among equal weights
  docs[g]       rows labelled g; count[g,t] rows of g that store t; dominant[g,t] rows of g whose dominant topic is t
  sum[g,t]      the rows of g ascending, folded 64 at a time, each fold (((0.0 + v_0) + v_1) + ..), until one value is left (at least once)
A label 0xffffffff puts the row into no group: it is counted in `unlabelled` alone.  Every array of a result is an integer array: sum holds
the bits of the doubles."""
import numpy as np

FAN = 64
NONE = 0xFFFFFFFF
TILE_WIDE, TILE_NARROW = 1024, 64
FORMS = ("wide", "narrow")
FIELDS = ("docs", "unlabelled", "count", "dominant", "sum")


class Case:
    def __init__(self, name, num_topics, rows, groups=None, num_groups=1, order=False):
        """rows: (doc_offsets, topic, weight); groups: one label per row or None; order: the tree's sums differ from a sequential sum"""
        self.name, self.num_topics, self.num_groups, self.order = name, int(num_topics), int(num_groups), order
        self.off = np.ascontiguousarray(rows[0], np.int64)
        self.topic = np.ascontiguousarray(rows[1], np.uint32)
        self.weight = np.ascontiguousarray(rows[2], np.float32)
        self.rows = self.off.size - 1
        self.groups = None if groups is None else np.ascontiguousarray(groups, np.uint32)
        assert self.groups is None or self.groups.size == self.rows

    def source_arg(self):
        return (self.off, self.topic, self.weight)

    def labels(self):
        return np.zeros(self.rows, np.uint32) if self.groups is None else self.groups


def d2b(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def row_of_entry(c):
    return np.repeat(np.arange(c.rows, dtype=np.int64), np.diff(c.off))


def row_sums(c):
    """the rows' sums in stored order, all rows at once: column j of the padded rows is added in step j (+0.0 changes no bits)"""
    length = np.diff(c.off)
    rs = np.zeros(c.rows, np.float64)
    for j in range(int(length.max()) if c.rows else 0):
        have = length > j
        col = np.zeros(c.rows, np.float64)
        col[have] = c.weight[c.off[:-1][have] + j].astype(np.float64)
        rs = rs + col
    return rs


def terms(c, normalise):
    """x as a dense rows x k matrix of doubles"""
    k = c.num_topics
    x = np.zeros((c.rows, k), np.float64)
    if c.topic.size:
        r = row_of_entry(c)
        w = c.weight.astype(np.float64)
        if normalise:
            rs = row_sums(c)[r]
            with np.errstate(divide="ignore", invalid="ignore"):
                w = np.where(rs == 0.0, 0.0, w / rs)
        x[r, c.topic] = np.where(c.weight == 0, 0.0, w)
    return x


def fold(v):
    """(n, k) -> (ceil(n / 64), k): 64 consecutive values added in order to 0.0"""
    n, k = v.shape
    m = (n + FAN - 1) // FAN
    pad = np.zeros((m * FAN, k), np.float64)
    pad[:n] = v
    pad = pad.reshape(m, FAN, k)
    acc = np.zeros((m, k), np.float64)
    for j in range(FAN):
        acc = acc + pad[:, j, :]
    return acc


def rule(c, normalise):
    k, G = c.num_topics, c.num_groups
    lab = c.labels().astype(np.int64)
    inside = lab != NONE
    docs = np.bincount(lab[inside], minlength=G).astype(np.uint64)
    count = np.zeros((G, k), np.uint64)
    dominant = np.zeros((G, k), np.uint64)
    r = row_of_entry(c)
    if c.topic.size:
        keep = inside[r]
        np.add.at(count, (lab[r][keep], c.topic[keep].astype(np.int64)), 1)
        dense = np.full((c.rows, k), -1.0, np.float64)   # absent below every weight; argmax keeps the first, i.e. the smaller topic
        dense[r, c.topic] = c.weight.astype(np.float64)  # (-0.0 == +0.0 under the comparison)
        has = (np.diff(c.off) > 0) & inside
        np.add.at(dominant, (lab[has], np.argmax(dense[has], axis=1)), 1)
    x = terms(c, normalise)
    total = np.zeros((G, k), np.float64)
    for g in np.unique(lab[inside]).tolist():
        v = x[lab == g]
        while True:
            v = fold(v)
            if v.shape[0] == 1:
                break
        total[g] = v[0]
    return dict(docs=docs, unlabelled=np.array([int((~inside).sum())], np.uint64), count=count, dominant=dominant, sum=d2b(total).reshape(G, k))


def scalar_terms(c, normalise):
    """per row a dict topic -> x, Python floats; and per row the dominant topic or None"""
    xs, dom = [], []
    for r in range(c.rows):
        b, e = int(c.off[r]), int(c.off[r + 1])
        rs = 0.0
        for w in c.weight[b:e].tolist():
            rs = rs + w
        row = {}
        best = None
        for t, w in zip(c.topic[b:e].tolist(), c.weight[b:e].tolist()):
            if w == 0:
                x = 0.0
            elif not normalise:
                x = w
            else:
                x = 0.0 if rs == 0.0 else w / rs
            row[t] = x
            if best is None or w > best[0]:
                best = (w, t)
        xs.append(row)
        dom.append(None if best is None else best[1])
    return xs, dom


def rule_scalar(c, normalise, sequential=False):
    """the rule cell by cell; sequential: sum[g,t] as a plain ascending sequential sum instead of the tree"""
    k, G = c.num_topics, c.num_groups
    lab = c.labels().tolist()
    xs, dom = scalar_terms(c, normalise)
    docs = np.zeros(G, np.uint64)
    count = np.zeros((G, k), np.uint64)
    dominant = np.zeros((G, k), np.uint64)
    total = np.zeros((G, k), np.float64)
    members = {}
    none = 0
    for r, g in enumerate(lab):
        if g == NONE:
            none += 1
            continue
        members.setdefault(g, []).append(r)
        docs[g] += 1
        for t in xs[r]:
            count[g, t] += 1
        if dom[r] is not None:
            dominant[g, dom[r]] += 1
    for g, rows in members.items():
        for t in range(k):
            v = [xs[r].get(t, 0.0) for r in rows]
            if sequential:
                s = 0.0
                for a in v:
                    s = s + a
                total[g, t] = s
                continue
            while True:
                nxt = []
                for i in range(0, len(v), FAN):
                    s = 0.0
                    for a in v[i:i + FAN]:
                        s = s + a
                    nxt.append(s)
                v = nxt
                if len(v) == 1:
                    break
            total[g, t] = v[0]
    return dict(docs=docs, unlabelled=np.array([none], np.uint64), count=count, dominant=dominant, sum=d2b(total).reshape(G, k))


def first_fault_text(c):
    """the refusal of the call for rows that break the rule, as the header words it: a bad label before a bad entry, each the first"""
    k, G = c.num_topics, c.num_groups
    lab = c.labels()
    bad = np.nonzero((lab != NONE) & (lab >= G))[0]
    if bad.size:
        return "topic_prevalence: row %d has label %d >= num_groups %d (0xffffffff: no group)" % (bad[0], lab[bad[0]], G)
    for r in range(c.rows):
        for e in range(int(c.off[r]), int(c.off[r + 1])):
            t, w = int(c.topic[e]), c.weight[e]
            if t >= k:
                return "topic_prevalence: entry %d (row %d) has topic %d >= num_topics %d" % (e, r, t, k)
            if e > c.off[r] and int(c.topic[e - 1]) >= t:
                return "topic_prevalence: entry %d (row %d), topic %d: the topics of a row must ascend strictly" % (e, r, t)
            if not (w >= 0 and w < 2.0 ** 31):
                return "topic_prevalence: entry %d (row %d) has weight %s: a weight is finite, >= 0 and < 2^31" % (e, r, "%g" % float(w))
    return ""


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------------
def make_rows(seed, rows, k, max_len, wide=True, empty_every=0):
    """rows of 0 .. max_len distinct ascending topics; wide: weights 2^-40 .. 2^20 with random mantissas, else small integers"""
    rng = np.random.RandomState(seed)
    off, topic, weight = [0], [], []
    for r in range(rows):
        n = 0 if (empty_every and r % empty_every == empty_every - 1) else int(rng.randint(1, min(k, max_len) + 1))
        t = np.sort(rng.choice(k, n, replace=False))
        w = (rng.uniform(1.0, 2.0, n) * 2.0 ** rng.randint(-40, 20, n)) if wide else rng.randint(1, 9, n)
        topic += t.tolist()
        weight += np.asarray(w, np.float32).tolist()
        off.append(len(topic))
    return np.array(off, np.int64), np.array(topic, np.uint32), np.array(weight, np.float32)


def _three_groups():
    # sizes 0, 64 and 65 interleaved, every fifth row in no group: list order is not row order
    lab, left = [], {1: 64, 2: 65}
    i = 0
    while left[1] or left[2]:
        if i % 5 == 4:
            lab.append(NONE)
        else:
            g = 1 if (i % 2 == 0 and left[1]) or not left[2] else 2
            lab.append(g)
            left[g] -= 1
        i += 1
    return np.array(lab, np.uint32)


def _special():
    nz = np.float32(-0.0)
    rows = [[], [(0, 0.0), (2, 0.0)], [(1, nz), (3, 2.5)], [(0, 1.5), (1, 3.0), (3, 3.0)], [(2, nz)], [], [(0, 2.0 ** -40), (3, 2.0 ** 20)], [(1, nz), (2, 0.0)]]
    off, topic, weight = [0], [], []
    for row in rows:
        topic += [t for t, _ in row]
        weight += [w for _, w in row]
        off.append(len(topic))
    return (np.array(off, np.int64), np.array(topic, np.uint32), np.array(weight, np.float32)), np.array([0, 1, 0, 1, 1, NONE, 0, 0], np.uint32)


def _cases():
    out = [Case("rows0", 3, (np.zeros(1, np.int64), np.zeros(0, np.uint32), np.zeros(0, np.float32))),
           Case("rows1", 3, make_rows(1, 1, 3, 3))]
    for n in (63, 64, 65):
        out.append(Case("one_group_%d" % n, 5, make_rows(10 + n, n, 5, 5)))
    out.append(Case("one_group_130", 5, make_rows(7, 130, 5, 5), order=True))
    for n in (4096, 4097):
        out.append(Case("one_group_%d" % n, 3, make_rows(n, n, 3, 3, empty_every=17), order=True))
    lab = _three_groups()
    out.append(Case("three_groups_0_64_65", 7, make_rows(3, lab.size, 7, 7, empty_every=11), lab, 3))
    rng = np.random.RandomState(5)
    out.append(Case("g1000_on_700_rows", 4, make_rows(4, 700, 4, 4), rng.randint(0, 1000, 700), 1000))
    for k in (1, 64, 65, 200, 1024, 1025):
        rows = make_rows(100 + k, 150, k, 100)
        rows[1][-1] = k - 1  # the last topic is stored (the last entry is its row's largest topic)
        out.append(Case("k%d" % k, k, rows, np.arange(150) % 2, 2, order=k > 1))
    rows = make_rows(77, 200, 4100, 100)
    rows[1][-1] = 4099
    out.append(Case("k4100_one_group", 4100, rows, order=True))  # five wide tiles; the counters too many for LDS, and no labels
    rows, lab = _special()
    out.append(Case("special_rows", 4, rows, lab, 2))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


# ---- rows that are refused on the device: the text names the first offender ------------------------------------------------------------------------
def _broken(name, **change):
    off, topic, weight = (a.copy() for a in make_rows(9, 300, 6, 6, wide=False))
    lab = (np.arange(300) % 3).astype(np.uint32)
    for e, w in change.get("weights", []):
        weight[e] = w
    for e, t in change.get("topics", []):
        topic[e] = t
    for r, g in change.get("labels", []):
        lab[r] = g
    return Case(name, 6, (off, topic, weight), lab, 3)


def _refusals():
    base = _broken("base")
    two = int(np.nonzero(np.diff(base.off) >= 2)[0][40])  # a row with two entries at least, somewhere in the middle
    e2 = int(base.off[two]) + 1
    return [_broken("bad_label", labels=[(17, 3), (250, 9)]),
            _broken("label_none_is_no_fault_but_7_is", labels=[(5, NONE), (299, 7)]),
            _broken("negative_weight_first_of_two", weights=[(e2, -1.0), (e2 + 300, np.inf)]),
            _broken("nan_weight", weights=[(e2 + 5, np.nan)]),
            _broken("weight_2_pow_31", weights=[(e2 + 9, 2.0 ** 31)]),
            _broken("topic_out_of_range", topics=[(int(base.off[two + 1]) - 1, 6)]),
            _broken("topics_do_not_ascend", topics=[(e2, int(base.topic[e2 - 1]))]),
            _broken("label_before_entry", labels=[(280, 4)], weights=[(3, -2.0)])]


REFUSALS = _refusals()
