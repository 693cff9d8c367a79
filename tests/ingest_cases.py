"""The case table of the ingest certificate: texts at the tile, digit and range edges of ingest.hip, its radix sort and its scans.
test_gpu_ingest_certified.py runs every case on the device, test_ingest_rule_cpu.py runs all but the two large ones through the host
parser; both compare with tests/ingest_rule.py.  No GPU, no torch.

The numbers the cases aim at: count_nl16 reads 16 bytes per thread and 4096 per workgroup; the parse grid, the flag pass and the
compaction work in blocks of 256 lines or entries; a wave is 64 lanes; the sort takes 2048 keys per workgroup and 8 key bits per pass,
over ceil(log2 V) + ceil(log2 D) bits; the scan takes 4096 inputs per block and carries over blocks of 256 block sums, so its carry loop
runs twice from 1,048,577 inputs on.

Every text stays under 64 KB except the two large cases (a million lines; 2^24 + 1 documents with the 8-pass sort) and the three texts
of 70,000 lines of the error-order cases, which no 64 KB can hold."""
import numpy as np

from ingest_rule import csc_from_entries, ingest_rule, text_from_entries

VMAX = 0xfffffff0          # the library's largest vocabulary / document count
SMALL_TEXT = 64 * 1024


class Case:
    def __init__(self, id, V, D, make, large=False, long_text=False):
        self.id, self.V, self.D, self._make, self.large, self.long_text = id, int(V), int(D), make, large, long_text
        self._built = None

    def build(self):
        """-> (text, arrays): arrays = (doc, word, cnt) as written, in file order, where the text holds valid entries only; else None."""
        if self._built is not None:
            return self._built
        made = self._make()
        built = (made, None) if isinstance(made, (bytes, bytearray)) else (made[0], made[1])
        if not self.large:
            self._built = built
        return built

    def expected(self, text, arrays):
        """The rule's verdict; for the large cases the same from the arrays (test_ingest_rule_cpu.py ties the two on every other case)."""
        if self.large:
            return ("ok",) + csc_from_entries(*arrays, self.D) + (len(arrays[0]),)
        return ingest_rule(text, self.V, self.D)

    def __repr__(self):
        return self.id


CASES = []


def case(id, V, D, **kw):
    def deco(fn):
        CASES.append(Case(id, V, D, fn, **kw))
        return fn
    return deco


def fixed(id, V, D, text, **kw):
    CASES.append(Case(id, V, D, lambda: text, **kw))


def lines_of(doc, word, cnt, blank_every=0, final_newline=True):
    """Small texts, line by line: "<doc> <word> <cnt>\\n", an empty line as every blank_every-th line."""
    out, nline = [], 0
    for d, w, c in zip(doc, word, cnt):
        if blank_every and nline % blank_every == blank_every - 1:
            out.append(b"\n")
            nline += 1
        out.append(b"%d %d %d\n" % (d, w, c))
        nline += 1
    text = b"".join(out)
    return text if final_newline else text[:-1]


def unique_pairs(n, V, D, seed):
    """n distinct (doc, word) pairs, 1-based, shuffled; counts = 1-based position in the file."""
    assert n <= V * D
    rng = np.random.default_rng(seed)
    flat = rng.permutation(rng.choice(V * D, size=n, replace=False))
    return flat // V + 1, flat % V + 1, np.arange(1, n + 1)


# ---------------------------------------------------------------- newline geometry (ing_nl_count_k, ing_nl_fill_k, count_nl16)
def exact_length(n, final_newline=True):
    """Short lines, the last one padded with leading blanks so that the text has exactly n bytes."""
    out, used, i = [], 0, 0
    core = b"2 3 4\n" if final_newline else b"2 3 4"
    while n - used > 40 + len(core):
        ln = b"%d %d %d\n" % (i % 5 + 1, i % 4 + 1, i + 1)
        out.append(ln)
        used += len(ln)
        i += 1
    assert n - used >= len(core)
    out.append(b" " * (n - used - len(core)) + core)
    text = b"".join(out)
    assert len(text) == n
    return text


fixed("nl-n0", 5, 5, b"")
fixed("nl-n1", 5, 5, b"\n")
fixed("nl-n5", 5, 5, b"1 1 1")
for _n in (15, 16, 17, 4095, 4096, 4097, 8192):
    fixed("nl-n%d" % _n, 5, 5, exact_length(_n, final_newline=_n % 2 == 1))
for _at in (15, 16):            # one line padded with leading zeros: its '\n' is byte _at
    fixed("nl-newline-at-%d" % _at, 5, 5, b"0" * (_at - 5) + b"1 2 3\n" + b"2 1 7\n3 3 9")
for _at in (4095, 4096):        # the same with leading blanks, across a whole 4096-byte tile
    fixed("nl-newline-at-%d" % _at, 5, 5, b" " * (_at - 5) + b"1 2 3\n" + b"2 1 7\n3 3 9\n")
fixed("nl-newline-in-last-partial-chunk", 5, 5, exact_length(51) + b"2 1 5")          # 56 bytes: '\n' at 50, in the chunk 48..55
fixed("nl-only-blank-lines", 5, 5, b"\n\n  \n\t\r\n \t \n\r\n" + b"\n" * 40 + b"   ")
fixed("nl-last-line-ends-in-cr", 5, 5, b"1 1 1\n2 2 2\r")
fixed("nl-last-line-trailing-blanks", 5, 5, b"1 1 1\n2 2 2  \t ")
fixed("nl-line-longer-than-a-tile", 5, 5, b" " * 5000 + b"1 2 3\n" + b"2 1 1\n")


# ---------------------------------------------------------------- line counts (ing_parse_k's grid, the scan of `valid`, ing_pack_k)
def _lines_case(nlines):
    def make():
        n = nlines - nlines // 3                       # every third line is blank
        doc, word, cnt = unique_pairs(n, 50, 97, seed=nlines)
        text = lines_of(doc, word, cnt, blank_every=3)
        if nlines % 3 == 0:
            text += b"\n"                              # the blank line that would follow the last entry
        assert text.count(b"\n") == nlines
        return text, (doc, word, cnt)
    return make


for _nl in (1, 255, 256, 257, 4095, 4096, 4097):
    CASES.append(Case("lines-%d" % _nl, 50, 97, _lines_case(_nl)))

MILLION_LINES = 1100000        # more than 256 * 4096 = 1,048,576 inputs: the scan's carry loop runs twice


@case("lines-million", 3000, 5000, large=True)
def _million():
    n = MILLION_LINES * 6 // 7                         # six entries, then a blank line
    j = np.arange(n, dtype=np.int64)
    pair = (j * 7919) % (3000 * 5000)                  # 7919 is prime to V * D: the pairs are distinct
    doc, word, cnt = pair // 3000 + 1, pair % 3000 + 1, j % 1000 + 1
    text = text_from_entries(doc, word, cnt, eol=[b"\n"] * 5 + [b"\n\n"], sep=[b" ", b"\t"])
    return text + b"\n" * (MILLION_LINES - (n + n // 6)), (doc, word, cnt)


# ---------------------------------------------------------------- sort passes: 1 to 8, both parities of the ping-pong
def wide_words(n, V, rng):
    """Word ids from both ends of 1..V and from rows (word - 1) that are multiples of 256 and of 65536."""
    kind = rng.integers(0, 4, size=n)
    low = rng.integers(1, 300, size=n)
    high = V - rng.integers(0, 300, size=n)
    m256 = rng.integers(0, V // 256, size=n) * 256 + 1
    m64k = rng.integers(0, V // 65536, size=n) * 65536 + 1
    return np.choose(kind, [low, high, m256, m64k])


def _passes_case(V, D, n, words):
    def make():
        rng = np.random.default_rng(V % 1000 + D % 1000 + n)
        if words == "any" and n > V * D:               # more lines than pairs: mostly repeats
            doc, word = rng.integers(1, D + 1, size=n), rng.integers(1, V + 1, size=n)
        elif words == "any":
            doc, word, _ = unique_pairs(n, V, D, seed=n)
        else:
            if words == "wide":
                word = wide_words(n, V, rng)
            else:                                      # every row a multiple of `words`: whole passes in which every key has digit 0
                word = rng.integers(0, V // words, size=n) * words + 1
            doc = (np.arange(n, dtype=np.int64) * D) // n + 1 if D > n else rng.integers(1, D + 1, size=n)   # spread evenly over many documents
            doc[0], doc[-1] = 1, D
            doc = rng.permutation(doc)
        cnt = np.arange(1, n + 1)                      # file order: a repeated pair shows which one survived
        return text_from_entries(doc, word, cnt), (doc, word, cnt)
    return make


PASSES = [  # passes, key bits, V, D, entries, word ids
    (1, 7, 8, 9, 5000, "any"),            # 72 pairs only: mostly repeats
    (2, 16, 200, 200, 5000, "any"),
    (3, 24, 65537, 100, 4400, "any"),     # fewer entries from here on, ids are longer: the text stays under 64 KB
    (4, 25, 3000, 5000, 4400, "any"),
    (5, 33, VMAX, 2, 3500, "wide"),
    (6, 44, VMAX, 4096, 2800, "wide"),
    (7, 52, VMAX, 1 << 20, 2600, "wide"),
    (8, 57, VMAX, (1 << 24) + 1, 5000, "wide"),
]
for _p, _bits, _V, _D, _n, _w in PASSES:
    CASES.append(Case("passes-%d" % _p, _V, _D, _passes_case(_V, _D, _n, _w), large=_p == 8))
CASES.append(Case("passes-5-rows-multiples-of-256", VMAX, 2, _passes_case(VMAX, 2, 3000, 256)))
CASES.append(Case("passes-6-rows-multiples-of-65536", VMAX, 4096, _passes_case(VMAX, 4096, 2700, 65536)))


def key_bits(V, D):
    wbits = dbits = 1
    while (1 << wbits) < V:
        wbits += 1
    while (1 << dbits) < D:
        dbits += 1
    return wbits + dbits


# ---------------------------------------------------------------- sort sizes and shapes
def _size_case(ne):
    def make():
        doc, word, cnt = unique_pairs(ne, 1000, 1000, seed=ne)
        return lines_of(doc, word, cnt, final_newline=ne % 2 == 0), (doc, word, cnt)
    return make


for _ne in (1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097):
    CASES.append(Case("sort-ne%d" % _ne, 1000, 1000, _size_case(_ne)))


def _ordered(reverse):
    def make():
        doc, word, cnt = unique_pairs(4097, 1000, 1000, seed=5)
        order = np.lexsort((word, doc))
        order = order[::-1] if reverse else order
        doc, word = doc[order], word[order]
        return lines_of(doc, word, cnt), (doc, word, cnt)
    return make


CASES.append(Case("sort-already-sorted", 1000, 1000, _ordered(False)))
CASES.append(Case("sort-reverse-sorted", 1000, 1000, _ordered(True)))


@case("sort-one-low-byte", 70000, 300)
def _one_low_byte():                                   # every row is 0x5a modulo 256: the first pass moves nothing apart
    rng = np.random.default_rng(6)
    flat = rng.permutation(rng.choice(273 * 300, size=4097, replace=False))
    doc, word, cnt = flat // 273 + 1, (flat % 273) * 256 + 0x5a + 1, np.arange(1, 4098)
    return lines_of(doc, word, cnt), (doc, word, cnt)


@case("sort-one-digit-takes-a-whole-tile", 200, 3000)
def _one_digit():                                      # 2048 keys, one workgroup, one word: in the first pass one digit receives them all
    doc = np.random.default_rng(7).permutation(3000)[:2048] + 1
    word, cnt = np.full(2048, 77), np.arange(1, 2049)
    return lines_of(doc, word, cnt), (doc, word, cnt)


# ---------------------------------------------------------------- stability and de-duplication: the counts are the file order
fixed("dup-5000-lines-one-pair", 9, 9, b"".join(b"5 5 %d\n" % (i + 1) for i in range(5000)))


def _group_at(before, group, after, seed):
    """Sorted sequence: `before` distinct keys, one key `group` times, `after` distinct keys; shuffled into file order."""
    def make():
        V, D = 100, 100
        mid = (D // 2) * V + V // 2
        rng = np.random.default_rng(seed)
        lo = rng.choice(mid, size=before, replace=False)
        hi = mid + 1 + rng.choice(V * D - mid - 1, size=after, replace=False)
        flat = rng.permutation(np.concatenate([lo, np.full(group, mid), hi]))
        doc, word, cnt = flat // V + 1, flat % V + 1, np.arange(1, len(flat) + 1)
        return lines_of(doc, word, cnt), (doc, word, cnt)
    return make


CASES.append(Case("dup-group-of-300-across-sorted-index-2048", 100, 100, _group_at(1900, 300, 500, 8)))
CASES.append(Case("dup-group-of-3-across-sorted-index-256", 100, 100, _group_at(255, 3, 100, 9)))


@case("dup-members-in-other-waves-and-tiles", 1000, 1000)
def _far_members():                                    # members of a group 70, 2100 and 4200 lines apart: other waves, other sort tiles
    doc, word, cnt = unique_pairs(5000, 1000, 1000, seed=10)
    for g in range(40):
        first = 10 + 7 * g
        for gap in (70, 2100, 4200):
            doc[first + gap], word[first + gap] = doc[first], word[first]
    return lines_of(doc, word, cnt), (doc, word, cnt)


# ---------------------------------------------------------------- offsets
fixed("offs-only-document-1", 20, 50, b"1 3 1\n1 20 2\n1 1 3\n")
fixed("offs-only-document-D", 20, 50, b"50 3 1\n50 20 2\n50 1 3\n")
fixed("offs-empty-runs-start-middle-end", 20, 50, b"30 2 1\n11 1 2\n10 5 3\n31 7 4\n12 9 5\n10 4 6\n")
fixed("offs-D-is-1", 20, 1, b"1 20 1\n1 1 2\n1 7 3\n")
CASES.append(Case("offs-one-entry-per-document", 20, 300, lambda: lines_of(np.random.default_rng(11).permutation(300) + 1,
                                                                             np.arange(300) % 20 + 1, np.arange(1, 301))))

# ---------------------------------------------------------------- ranges
ZEROS40 = b"0" * 40
fixed("range-doc-D-and-word-V", 7, 9, b"9 7 3\n1 1 1\n")
fixed("range-doc-D-plus-1", 7, 9, b"1 1 1\n10 7 3\n")
fixed("range-word-V-plus-1", 7, 9, b"1 1 1\n\n9 8 3\n")
fixed("range-doc-0", 7, 9, b"0 1 1\n")
fixed("range-word-0", 7, 9, b"1 0 1\n")
fixed("range-last-word-of-the-widest-vocabulary", VMAX, 3, b"2 4294967280 5\n2 1 6\n")
fixed("range-word-past-the-widest-vocabulary", VMAX, 3, b"2 4294967281 5\n")
fixed("range-counts-at-float32-edges", 9, 9, b"1 1 1\n1 2 16777216\n1 3 16777217\n1 4 4294967295\n1 5 16777219\n1 6 4294967167\n")
fixed("range-count-2^32", 9, 9, b"1 1 1\n1 1 4294967296\n")
fixed("range-count-20-nines", 9, 9, b"1 1 99999999999999999999\n")
fixed("range-count-2^64", 9, 9, b"1 1 18446744073709551616\n")           # 0 modulo 2^64: still kind 6, never "count is 0"
fixed("range-count-2^64-plus-3", 9, 9, b"1 1 18446744073709551619\n")
fixed("range-doc-2^64-plus-1", 9, 9, b"18446744073709551617 1 3\n")
fixed("range-word-2^64-plus-1", 9, 9, b"1 18446744073709551617 3\n")
fixed("range-doc-30-digits", 9, 9, b"100000000000000000000000000001 1 3\n")
fixed("range-word-30-digits", 9, 9, b"1 100000000000000000000000000001 3\n")
fixed("range-40-leading-zeros-in-each-field", 9, 9, ZEROS40 + b"1 " + ZEROS40 + b"2 " + ZEROS40 + b"3\n" + b"2 2 " + ZEROS40 + b"7\n")

# ---------------------------------------------------------------- errors
fixed("err-kind1-bad-character", 5, 5, b"1 2 3\n\n1 x 3\n2 2 2\n")
fixed("err-kind2-four-fields", 5, 5, b"1 2 3\n\n2 2 2\n1 2 3 4\n")
fixed("err-kind3-two-fields", 5, 5, b"1 2 3\n1 2\n")
fixed("err-kind3-one-field", 5, 5, b"1 2 3\n\n\n  7  \n")
fixed("err-kind3-two-fields-no-last-newline", 5, 5, b"1 1 1\n2 2")
fixed("err-kind4-doc-too-large", 5, 5, b"1 2 3\n6 1 1\n")
fixed("err-kind5-count-0", 5, 5, b"1 1 1\n2 2 0\n")
fixed("err-kind6-count-too-large", 5, 5, b"1 1 1\n\r\n2 2 4294967296")
fixed("err-bad-character-before-the-fourth-field", 5, 5, b"1 2 x 3 4\n")
fixed("err-fourth-field-before-the-bad-character", 5, 5, b"1 2 3 4 x\n")
fixed("err-bad-character-beats-the-id-range", 5, 5, b"9 9 0 .\n")
fixed("err-id-range-beats-count-0", 5, 5, b"9 1 0\n")
for _name, _byte in (("vt", b"\v"), ("ff", b"\f"), ("minus", b"-"), ("plus", b"+"), ("dot", b"."), ("nul", b"\0"), ("0x80", b"\x80"),
                     ("0xff", b"\xff"), ("letter", b"e"), ("comma", b","), ("slash", b"/"), ("colon", b":")):
    fixed("err-byte-%s" % _name, 5, 5, b"1 2 3\n2 " + _byte + b"2 3\n")
    if _name in ("vt", "ff", "nul"):                   # as a would-be separator, where split() would have taken it
        fixed("err-byte-%s-between-fields" % _name, 5, 5, b"1 2 3\n2" + _byte + b"2 3\n")

BAD_LINE = {1: b"1 x 1\n", 2: b"1 2 3 4\n", 3: b"1 2\n"}


def _bad_lines(nlines, where):
    """nlines lines "<d> <w> 1"; `where` maps a 1-based line to the kind of bad line that stands there."""
    def make():
        j = np.arange(nlines)
        text = text_from_entries(j % 9 + 1, j % 7 + 1, np.ones(nlines, np.int64))
        starts = np.concatenate([[0], np.flatnonzero(np.frombuffer(text, np.uint8) == 10) + 1])
        out, at = [], 0
        for line in sorted(where):
            out += [text[at:starts[line - 1]], BAD_LINE[where[line]]]
            at = starts[line]
        return b"".join(out + [text[at:]])
    return make


for _id, _where in (("err-first-of-three-kinds-3-1-2", {3: 3, 300: 1, 70000: 2}), ("err-first-of-three-kinds-1-2-3", {3: 1, 300: 2, 70000: 3}),
                    ("err-first-of-three-kinds-2-3-1", {3: 2, 300: 3, 70000: 1}),
                    ("err-first-of-three-in-late-blocks", {69300: 3, 69600: 1, 69900: 2})):
    CASES.append(Case(_id, 9, 9, _bad_lines(70000, _where), long_text=True))

assert len({c.id for c in CASES}) == len(CASES)
