"""The lag table of one book in plain Python: what bk_lags_enable's device fold must leave in a book's K rows and carry.

``fold(hist, K)`` walks an ``[n_steps, W]`` level-2 history (``env.history()[:, b]``) step by step, in the order of the
contract in include/bourse_amd.h, with Python's unbounded integers; only at the end are the words reduced modulo 2**64
(``sum_h4`` modulo 2**128, signed words to two's complement).  ``cuts`` lists the steps IN FRONT OF which the book's past is
forgotten, as a reset of the book at that step count does.  It shares no code with bourse_amd/csrc/lag_fold.hpp or
lags.hpp, and every GPU test compares against it."""
import numpy as np

FIELDS = ("n_pairs", "sum_dd", "sum_abs_dd", "n_h", "sum_h", "sum_abs_h", "sum_h2", "sum_h4_lo", "sum_h4_hi", "max_abs_h")
SIGNED = ("sum_dd", "sum_h")
LAG_DTYPE = np.dtype({"names": list(FIELDS), "formats": ["<i8" if n in SIGNED else "<u8" for n in FIELDS],
                      "offsets": [8 * i for i in range(10)], "itemsize": 80})
SUMS = ("n_pairs", "sum_dd", "sum_abs_dd", "n_h", "sum_h", "sum_abs_h", "sum_h2", "sum_h4", "max_abs_h")
M64 = (1 << 64) - 1
M128 = (1 << 128) - 1
NO_ASK = 0xFFFFFFFF


def cleared(K):
    """the unreduced sums of K rows without a step, and an empty past"""
    assert 1 <= K <= 64
    return {"K": K, "rows": [{n: 0 for n in SUMS} for _ in range(K)], "past": []}


def fold(hist, K=None, cuts=(), first_step=0, into=None):
    """fold the records hist[i] = step first_step + i into the sums ``into`` (default: K cleared rows) and return them.
    ``past`` holds m of every step since the start (None: one-sided), the latest last; only the last K + 1 are kept."""
    s = cleared(K) if into is None else into
    K = s["K"]
    past = s["past"]
    cuts = set(int(c) for c in cuts)
    for i, rec in enumerate(hist):
        if first_step + i in cuts:
            past = []
        bid, ask = int(rec[1]), int(rec[2])
        m = bid + ask if bid != 0 and ask != NO_ASK else None
        past.append(m)  # past[-1] is step s, past[-1 - k] step s - k; a step in front of the start is not two-sided
        at = lambda k: past[-1 - k] if k < len(past) else None
        for k in range(1, K + 1):
            row = s["rows"][k - 1]
            if m is not None and at(k) is not None:
                h = m - at(k)
                a = abs(h)
                row["n_h"] += 1
                row["sum_h"] += h
                row["sum_abs_h"] += a
                row["sum_h2"] += a * a
                row["sum_h4"] += a ** 4
                row["max_abs_h"] = max(row["max_abs_h"], a)
            if m is not None and at(1) is not None and at(k) is not None and at(k + 1) is not None:
                d, dk = m - at(1), at(k) - at(k + 1)
                row["n_pairs"] += 1
                row["sum_dd"] += d * dk
                row["sum_abs_dd"] += abs(d) * abs(dk)
        past = past[-(K + 1):]
    s["past"] = past
    return s


def cut(s):
    """what a reset of the book does: the past is forgotten, the sums go on"""
    s["past"] = []
    return s


def words(s):
    """the K rows' ten words each, as unsigned Python integers: [K][10]"""
    out = []
    for row in s["rows"]:
        w = {n: row[n] & M64 for n in SUMS if n != "sum_h4"}
        w["sum_h4_lo"] = row["sum_h4"] & M64
        w["sum_h4_hi"] = (row["sum_h4"] & M128) >> 64
        out.append([w[n] for n in FIELDS])
    return out


def carry(s):
    """the K + 1 carry words: entry j is the step j + 1 back from the next one - bit 63 two-sided, the low bits m; else 0"""
    past = s["past"]
    out = []
    for j in range(s["K"] + 1):
        m = past[-1 - j] if j < len(past) else None
        out.append(0 if m is None else (1 << 63) | m)
    return out


def table(s):
    """... as LAG_DTYPE records [K]"""
    r = np.zeros(s["K"], dtype=LAG_DTYPE)
    for k, w in enumerate(words(s)):
        for n, x in zip(FIELDS, w):
            r[k][n] = x - (1 << 64) if n in SIGNED and x >> 63 else x
    return r


def rows(hist, K, cuts=None, first_step=0):
    """hist [n_steps, n_books, W] -> LAG_DTYPE [n_books, K]; cuts: {book: steps}"""
    cuts = cuts or {}
    return np.array([table(fold(hist[:, b], K, cuts.get(b, ()), first_step)) for b in range(hist.shape[1])], dtype=LAG_DTYPE)
