"""The cross table of one market in plain Python: what bk_cross_enable's device fold must leave in a market's S * A * A rows
and carry.

``fold(hist, spans, A)`` walks an ``[n_steps, A, W]`` level-2 history (``env.history()[:, m * A:(m + 1) * A]``) step by step,
in the order of the contract in include/bourse_amd.h, with Python's unbounded integers; only at the end are the words
reduced modulo 2**64 (signed words to two's complement).  ``cuts`` lists the steps IN FRONT OF which the market's past is
forgotten, as a reset of the market at that step count does.  It shares no code with bourse_amd/csrc/cross_fold.hpp or
cross.hpp, and every GPU test compares against it."""
import numpy as np

FIELDS = ("n", "sum_x", "sum_y", "sum_xx", "sum_yy", "sum_xy", "n_lead", "sum_lead")
SIGNED = ("sum_x", "sum_y", "sum_xy", "sum_lead")
CROSS_DTYPE = np.dtype({"names": list(FIELDS), "formats": ["<i8" if n in SIGNED else "<u8" for n in FIELDS],
                        "offsets": [8 * i for i in range(8)], "itemsize": 64})
M64 = (1 << 64) - 1
NO_ASK = 0xFFFFFFFF


def cleared(spans, A):
    """the unreduced sums of S * A * A rows without a step, and an empty past of every asset"""
    spans = tuple(int(h) for h in spans)
    assert 1 <= len(spans) <= 4 and all(1 <= h <= 64 for h in spans) and 2 <= A <= 8
    return {"spans": spans, "A": A, "rows": [[[{n: 0 for n in FIELDS} for _ in range(A)] for _ in range(A)] for _ in spans],
            "past": [[] for _ in range(A)]}


def fold(hist, spans=None, A=None, cuts=(), first_step=0, into=None):
    """fold the records hist[i, a] = step first_step + i of asset a into the sums ``into`` (default: cleared rows) and return
    them.  ``past[a]`` holds m of every step of asset a since the start (None: one-sided), the latest last; only the last
    2 * Hmax + 1 are kept."""
    s = cleared(spans, hist.shape[1] if A is None else A) if into is None else into
    spans, A = s["spans"], s["A"]
    assert hist.shape[1] == A
    keep = 2 * max(spans) + 1
    past = s["past"]
    cuts = set(int(c) for c in cuts)
    for i, recs in enumerate(hist):
        if first_step + i in cuts:
            past = [[] for _ in range(A)]
        for a in range(A):
            bid, ask = int(recs[a][1]), int(recs[a][2])
            past[a].append(bid + ask if bid != 0 and ask != NO_ASK else None)
        at = lambda x, k: past[x][-1 - k] if k < len(past[x]) else None  # a step in front of the start is not two-sided
        for j, h in enumerate(spans):
            for a in range(A):
                if at(a, 0) is None or at(a, h) is None:
                    continue
                x = at(a, 0) - at(a, h)
                for b in range(A):
                    row = s["rows"][j][a][b]
                    if at(b, 0) is not None and at(b, h) is not None:
                        y = at(b, 0) - at(b, h)
                        row["n"] += 1
                        row["sum_x"] += x
                        row["sum_y"] += y
                        row["sum_xx"] += x * x
                        row["sum_yy"] += y * y
                        row["sum_xy"] += x * y
                    if at(b, h) is not None and at(b, 2 * h) is not None:
                        row["n_lead"] += 1
                        row["sum_lead"] += x * (at(b, h) - at(b, 2 * h))
        past = [p[-keep:] for p in past]
    s["past"] = past
    return s


def cut(s):
    """what a reset of the market does: the past of every asset is forgotten, the sums go on"""
    s["past"] = [[] for _ in range(s["A"])]
    return s


def words(s):
    """the rows' eight words each, as unsigned Python integers: [S][A][A][8]"""
    return [[[[row[n] & M64 for n in FIELDS] for row in of_a] for of_a in of_j] for of_j in s["rows"]]


def carry(s):
    """the 2 * Hmax carry words of every asset, forward in time: entry i is the step 2 * Hmax - i back from the next one -
    bit 63 two-sided, the low bits m; else 0"""
    C = 2 * max(s["spans"])
    out = []
    for p in s["past"]:
        ms = [p[i - C] if -len(p) <= i - C else None for i in range(C)]
        out.append([0 if m is None else (1 << 63) | m for m in ms])
    return out


def table(s):
    """... as CROSS_DTYPE records [S, A, A]"""
    A = s["A"]
    r = np.zeros((len(s["spans"]), A, A), dtype=CROSS_DTYPE)
    for j, of_j in enumerate(words(s)):
        for a in range(A):
            for b in range(A):
                for n, x in zip(FIELDS, of_j[a][b]):
                    r[j, a, b][n] = x - (1 << 64) if n in SIGNED and x >> 63 else x
    return r


def rows(hist, spans, A, cuts=None, first_step=0):
    """hist [n_steps, n_markets * A, W] -> CROSS_DTYPE [n_markets, S, A, A]; cuts: {market: steps}"""
    cuts = cuts or {}
    NM = hist.shape[1] // A
    assert NM * A == hist.shape[1]
    return np.array([table(fold(hist[:, m * A:(m + 1) * A], spans, A, cuts.get(m, ()), first_step)) for m in range(NM)], dtype=CROSS_DTYPE)
