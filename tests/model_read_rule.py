"""The reading rule of model files (include/isle_hip.h, isle_hip_load_model_text), restated in Python for its tests: numpy fp32 steps
for the digits, math.pow for the place, Python doubles for the combination.  Independent of the library: no call into it."""
import math
import re

import numpy as np

MAX_TOKEN = 64
MAX_ID_DIGITS = 18
MAX_SPARSE_LINE = 4096   # bytes of a sparse line without its newline; a longer one is refused as a bad character
MAX_CR_RUN = 64          # consecutive '\r' of a dense text; a longer run is refused as a bad character
QNAN = np.array([0x7fc00000], np.uint32).view(np.float32)[0]
KINDS = ("bad character", "too many fields", "too few fields", "id zero or out of range", "token too long", "wrong token count",
         "wrong line count")


class ModelReadError(ValueError):
    def __init__(self, line, kind):
        assert kind in KINDS
        ValueError.__init__(self, "line %d: %s" % (line, kind))
        self.line, self.kind = line, kind


def _digits(s):
    """fp32, digit by digit: v = v * 10 rounded, then v = v + d rounded."""
    v = np.float32(0)
    with np.errstate(over="ignore"):
        for ch in s:
            v = np.float32(v * np.float32(10))
            v = np.float32(v + np.float32(ch - 48))
    return v


def weight_error(tok, format="sparse"):
    """None for a token inside the grammar, else the kind of its first violation in byte order."""
    if format == "dense" and tok == b"nan":
        return None
    point = False
    for i, ch in enumerate(tok):
        if i >= MAX_TOKEN:
            return "token too long"
        if 48 <= ch <= 57:
            continue
        if ch == 46 and not point:
            point = True
            continue
        return "bad character"
    return None if re.search(rb"\d", tok) else "bad character"   # at least one digit


def parse_weight(tok, format="sparse"):
    """-> np.float32, or None for a token outside the grammar."""
    if weight_error(tok, format):
        return None
    if tok == b"nan":
        return QNAN
    before, _, after = tok.partition(b".")
    vb, va = _digits(before), _digits(after)
    with np.errstate(over="ignore"):
        return np.float32(float(vb) + float(va) * math.pow(0.1, len(after)))   # two double operations, one rounding to float


def _lines(text):
    """(1-based physical line number, its fields); '\\r' is ignored everywhere, blanks and tabs separate."""
    for no, ln in enumerate(bytes(text).replace(b"\r", b"").split(b"\n"), 1):
        yield no, [f for f in re.split(rb"[ \t]+", ln) if f]


def _last_line(text):
    n = bytes(text).count(b"\n") + 1
    return n - 1 if bytes(text).endswith(b"\n") else n


def parse_sparse(text, vocab, ncols, base=1):
    """-> (model (vocab, ncols) float32 F-order, lines parsed).  The last line naming a cell wins; other cells are +0."""
    M = np.zeros((vocab, ncols), np.float32, order="F")
    n = 0
    raw = bytes(text).split(b"\n")
    for no, f in _lines(text):
        if len(raw[no - 1]) > MAX_SPARSE_LINE:
            raise ModelReadError(no, "bad character")   # (the line is the rule; a violation before byte 4097 may be named instead)
        if not f:
            continue
        for x in f[:2]:
            for i, ch in enumerate(x):
                if not 48 <= ch <= 57:
                    raise ModelReadError(no, "bad character")
                if i >= MAX_ID_DIGITS:
                    raise ModelReadError(no, "id zero or out of range")
        if len(f) > 2:
            bad = weight_error(f[2], "sparse")
            if bad and not (bad == "bad character" and re.fullmatch(rb"\.?", f[2])):   # "." is found wanting at the line's end
                raise ModelReadError(no, bad)
        if len(f) > 3:
            raise ModelReadError(no, "too many fields")
        if len(f) < 3:
            raise ModelReadError(no, "too few fields")
        w = parse_weight(f[2], "sparse")
        if w is None:
            raise ModelReadError(no, "bad character")
        t, r = int(f[0]) - base, int(f[1]) - base
        if not (0 <= t < ncols and 0 <= r < vocab):
            raise ModelReadError(no, "id zero or out of range")
        M[r, t] = w
        n += 1
    return M, n


def parse_dense(text, vocab, ncols):
    """-> (model (vocab, ncols) float32 F-order, vocab * ncols).  Token j of the t-th non-blank line is model[j, t]."""
    M = np.zeros((vocab, ncols), np.float32, order="F")
    t = 0
    raw = bytes(text).split(b"\n")
    for no, f in _lines(text):
        if b"\r" * (MAX_CR_RUN + 1) in raw[no - 1]:
            raise ModelReadError(no, "bad character")   # (the line is the rule; an earlier violation of the line may be named instead)
        if not f:
            continue
        vals = []
        for x in f:
            bad = weight_error(x, "dense")
            if bad:
                raise ModelReadError(no, bad)
            vals.append(parse_weight(x, "dense"))
        if len(f) != vocab:
            raise ModelReadError(no, "wrong token count")
        if t < ncols:
            M[:, t] = vals
        t += 1
    if t != ncols:
        raise ModelReadError(_last_line(text), "wrong line count")
    return M, vocab * ncols
