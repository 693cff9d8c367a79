"""The plain rule of tdf ingest: text -> count matrix A (CSC), or the first bad line and its kind.  No GPU, no torch.

One byte-level state machine, one loop, exact Python integers: no split(), no int() on a token, nothing that accepts more than the
parsers do.  The rules are those of the headers of isle_amd/csrc/ingest.hip and isle_amd/host/prestage.h:

  lines     end at '\\n' (the last newline is optional); '\\r' is ignored wherever it stands; a line without a digit is skipped, it is no
            entry, and it still counts as a line for the line number of an error.
  fields    separated by blanks and tabs only.  Any byte other than a digit, blank, tab, '\\r' or '\\n' is kind 1 ("bad character"):
            '\\v', '\\f', '-', '+', '.', NUL and bytes of 0x80 and above among them.  A fourth field is kind 2, fewer than three kind 3.
  values    exact non-negative integers of any length: leading zeros are free, no width is ever counted.
  ids       a doc id outside 1..D or a word id outside 1..V is kind 4.
  counts    0 is kind 5, above 4294967295 kind 6; the others become float32 by round-to-nearest-even (what np.float32 does).
  errors    the lowest bad line and that line's kind.  Within a line: the character scan from the left (kinds 1 and 2, whichever comes
            first), then the number of fields, the id range, count zero, count range.
  result    entries sorted by (doc, word); of repeated pairs the first in file order survives; offsets include empty documents.

text_from_entries writes large texts with vectorised numpy and csc_from_entries states the sort / de-duplication / CSC step on arrays, so
that a million-line case spends no seconds in a Python loop and its expected matrix is not parsed back from its own text.
test_ingest_rule_cpu.py ties the two to the rule at sizes where the rule is quick."""
import numpy as np

KINDS = {1: "bad character", 2: "more than three fields", 3: "fewer than three fields",
         4: "doc/word id is 0 or exceeds <num_docs>/<vocab_size>", 5: "count is 0", 6: "count exceeds 4294967295"}
COUNT_MAX = 4294967295

_NL, _CR, _BLANK, _TAB, _ZERO, _NINE = 10, 13, 32, 9, 48, 57


def ingest_rule(text, V, D):
    """-> ("ok", counts_f32, rows_u32, offs_i64, entries_read) or ("error", kind, 1-based line)."""
    text = bytes(text)
    if text and text[-1] != _NL:
        text += b"\n"                                  # the last newline is optional
    entries = []                                       # (doc, word, position in the file, count), ids 0-based
    line, field, state, was_ws, any_digit = 1, [0, 0, 0], 0, False, False
    for ch in text:
        if _ZERO <= ch <= _NINE:                       # the common case first; the order of these tests decides nothing
            if was_ws and any_digit:
                state += 1
                if state > 2:
                    return ("error", 2, line)
            was_ws, any_digit = False, True
            field[state] = field[state] * 10 + (ch - _ZERO)
        elif ch == _BLANK or ch == _TAB:
            was_ws = True
        elif ch == _NL:
            if any_digit:
                if state != 2:
                    return ("error", 3, line)
                if not (1 <= field[0] <= D and 1 <= field[1] <= V):
                    return ("error", 4, line)
                if field[2] == 0:
                    return ("error", 5, line)
                if field[2] > COUNT_MAX:
                    return ("error", 6, line)
                entries.append((field[0] - 1, field[1] - 1, len(entries), field[2]))
            line, field, state, was_ws, any_digit = line + 1, [0, 0, 0], 0, False, False
        elif ch != _CR:
            return ("error", 1, line)
    entries_read = len(entries)
    entries.sort()                                     # (doc, word, position): the first in the file leads its group
    counts, rows, offs = [], [], [0] * (D + 1)
    last = None
    for doc, word, _, cnt in entries:
        if (doc, word) == last:
            continue
        last = (doc, word)
        counts.append(cnt)
        rows.append(word)
        offs[doc + 1] += 1
    offs = np.cumsum(np.array(offs, np.int64))
    return ("ok", np.array(counts, np.uint64).astype(np.float32), np.array(rows, np.uint32), offs, entries_read)


def csc_from_entries(doc, word, cnt, D):
    """The rule's last step on arrays: 1-based doc / word ids and counts in file order (all valid) -> (counts_f32, rows_u32, offs_i64)."""
    doc = np.asarray(doc, np.int64) - 1
    word = np.asarray(word, np.int64) - 1
    cnt = np.asarray(cnt, np.uint64)
    order = np.lexsort((np.arange(len(doc)), word, doc))   # position in the file last: the first occurrence leads its group
    doc, word, cnt = doc[order], word[order], cnt[order]
    first = np.ones(len(doc), bool)
    first[1:] = (doc[1:] != doc[:-1]) | (word[1:] != word[:-1])
    doc, word, cnt = doc[first], word[first], cnt[first]
    offs = np.zeros(D + 1, np.int64)
    offs[1:] = np.cumsum(np.bincount(doc, minlength=D))
    return cnt.astype(np.float32), word.astype(np.uint32), offs


def _decimal(a):
    """uint64 array (values below 10^10) -> (n x 10 matrix of ASCII digits, n x 10 mask of the digits to keep: no leading zeros)."""
    a = np.asarray(a, np.uint64)
    assert a.size == 0 or int(a.max()) < 10 ** 10
    pw = 10 ** np.arange(9, -1, -1, dtype=np.uint64)
    dig = ((a[:, None] // pw[None, :]) % np.uint64(10)).astype(np.uint8) + np.uint8(_ZERO)
    keep = a[:, None] >= pw[None, :]
    keep[:, -1] = True                                  # the value 0 is written "0"
    return dig, keep


def _cycled(pieces, n):
    """bytes, or a sequence of bytes used in turn line after line -> (n x w matrix, n x w mask)."""
    pieces = [pieces] if isinstance(pieces, (bytes, bytearray)) else list(pieces)
    w = max(len(p) for p in pieces)
    mat = np.zeros((len(pieces), max(w, 1)), np.uint8)
    keep = np.zeros((len(pieces), max(w, 1)), bool)
    for i, p in enumerate(pieces):
        mat[i, :len(p)] = np.frombuffer(bytes(p), np.uint8)
        keep[i, :len(p)] = True
    idx = np.arange(n) % len(pieces)
    return mat[idx], keep[idx]


def text_from_entries(doc, word, cnt, *, eol=b"\n", sep=b" "):
    """"<doc><sep><word><sep><cnt><eol>" per entry, the values as they are to stand in the file (ids 1-based).  eol and sep are bytes, or
    sequences of bytes taken in turn: eol=[b"\\n", b"\\n\\n"] leaves a blank line after every second entry."""
    n = len(doc)
    parts = [_decimal(doc), _cycled(sep, n), _decimal(word), _cycled(sep, n), _decimal(cnt), _cycled(eol, n)]
    mat = np.concatenate([p[0] for p in parts], axis=1)
    keep = np.concatenate([p[1] for p in parts], axis=1)
    return mat[keep].tobytes()                          # row-major selection: line after line, byte after byte
