"""The series moments of one book in plain Python: what bk_series_enable's device fold must leave in a book's row.

``fold(hist)`` walks an ``[n_steps, W]`` level-2 history (``env.history()[:, b]``) record by record, in the order of the
contract in include/bourse_amd.h, with Python's unbounded integers; only at the end are the words reduced modulo 2**64
(``sum_d4`` modulo 2**128, signed words to two's complement).  ``cuts`` lists the steps IN FRONT OF which the carry is
zeroed, as a reset of the book at that step count does.  It shares no code with bourse_amd/csrc/series_fold.hpp or
series.hpp, and every GPU test compares against it."""
import numpy as np

FIELDS = ("n_steps", "n_two_sided", "sum_m", "sum_spread", "sum_spread_sq", "sum_bid_vol", "sum_ask_vol", "sum_trade_vol",
          "sum_trade_vol_sq", "n_trade_steps", "n_ret", "sum_d", "sum_abs_d", "sum_d2", "sum_d4_lo", "sum_d4_hi", "max_abs_d",
          "n_pairs", "sum_dd", "sum_abs_dd", "min_m", "max_m", "carry_m", "carry_d")
SIGNED = ("sum_d", "sum_dd", "carry_d")
SERIES_DTYPE = np.dtype({"names": list(FIELDS), "formats": ["<i8" if n in SIGNED else "<u8" for n in FIELDS],
                         "offsets": [8 * i for i in range(24)], "itemsize": 192})
M64 = (1 << 64) - 1
M128 = (1 << 128) - 1
NO_ASK = 0xFFFFFFFF


def cleared():
    """the unreduced sums of a row without a record"""
    s = {n: 0 for n in FIELDS if n not in ("sum_d4_lo", "sum_d4_hi", "carry_m", "carry_d")}
    s["sum_d4"] = 0
    s["min_m"] = M64
    s["carry"] = (0, 0, 0, 0)  # have_m, m_prev, have_d, d_prev
    return s


def fold(hist, cuts=(), first_step=0, into=None):
    """fold the records hist[i] = step first_step + i into the sums ``into`` (default: a cleared row) and return them"""
    s = cleared() if into is None else into
    have_m, m_prev, have_d, d_prev = s["carry"]
    cuts = set(int(c) for c in cuts)
    for i, rec in enumerate(hist):
        if first_step + i in cuts:
            have_m = m_prev = have_d = d_prev = 0
        tv, bid, ask, ask_vol, bid_vol = (int(x) for x in rec[:5])
        s["n_steps"] += 1
        s["sum_trade_vol"] += tv
        s["sum_trade_vol_sq"] += tv * tv
        s["n_trade_steps"] += 1 if tv > 0 else 0
        s["sum_bid_vol"] += bid_vol
        s["sum_ask_vol"] += ask_vol
        two = bid != 0 and ask != NO_ASK
        if not two:
            have_m = m_prev = have_d = d_prev = 0
            continue
        m = bid + ask
        sp = (ask - bid) & 0xFFFFFFFF
        s["n_two_sided"] += 1
        s["sum_m"] += m
        s["sum_spread"] += sp
        s["sum_spread_sq"] += sp * sp
        s["min_m"] = min(s["min_m"], m)
        s["max_m"] = max(s["max_m"], m)
        if have_m:
            d = m - m_prev
            a = abs(d)
            s["n_ret"] += 1
            s["sum_d"] += d
            s["sum_abs_d"] += a
            s["sum_d2"] += a * a
            s["sum_d4"] += a ** 4
            s["max_abs_d"] = max(s["max_abs_d"], a)
            if have_d:
                s["n_pairs"] += 1
                s["sum_dd"] += d * d_prev
                s["sum_abs_dd"] += a * abs(d_prev)
            have_d, d_prev = 1, d
        else:
            have_d, d_prev = 0, 0
        have_m, m_prev = 1, m
    s["carry"] = (have_m, m_prev, have_d, d_prev)
    return s


def cut(s):
    """what a reset of the book does to its sums: the carry is zeroed, nothing else"""
    s["carry"] = (0, 0, 0, 0)
    return s


def words(s):
    """the row's 24 words as unsigned Python integers"""
    have_m, m_prev, have_d, d_prev = s["carry"]
    w = {n: s[n] & M64 for n in FIELDS if n in s}
    w["sum_d4_lo"] = s["sum_d4"] & M64
    w["sum_d4_hi"] = (s["sum_d4"] & M128) >> 64
    w["carry_m"] = (m_prev if have_m else 0) | (have_m << 63) | (have_d << 62)
    w["carry_d"] = (d_prev if have_d else 0) & M64
    return [w[n] for n in FIELDS]


def row(s):
    """... as one SERIES_DTYPE record"""
    r = np.zeros((), dtype=SERIES_DTYPE)
    for n, x in zip(FIELDS, words(s)):
        r[n] = x - (1 << 64) if n in SIGNED and x >> 63 else x
    return r


def rows(hist, cuts=None, first_step=0):
    """hist [n_steps, n_books, W] -> SERIES_DTYPE [n_books]; cuts: {book: steps}"""
    cuts = cuts or {}
    return np.array([row(fold(hist[:, b], cuts.get(b, ()), first_step)) for b in range(hist.shape[1])], dtype=SERIES_DTYPE)
