"""The depth table of one book in plain Python: what bk_depth_enable's device fold must leave in a book's rows and carry.

``fold(hist)`` walks an ``[n_steps, 5 + 4 L]`` level-2 history (``env.history()[:, b]``) step by step, in the order of the
contract in include/bourse_amd.h, with Python's unbounded integers; only at the end are the words reduced modulo 2**64.
The book's past is the step before - whether it was two-sided, twice its mid, and its cumulative imbalance per level - and is
forgotten at a cut; ``cuts`` lists the steps IN FRONT OF which that happens, as a reset of the book at that step count does.
It shares no code with bourse_amd/csrc/depth_fold.hpp or depth.hpp, and every GPU test compares against it."""
import numpy as np

FIELDS = ("sum_bid_vol", "sum_ask_vol", "sum_bid_vol_sq", "sum_ask_vol_sq", "sum_bid_orders", "sum_ask_orders", "n_bid_steps",
          "n_ask_steps", "sum_imb", "sum_imb_sq", "n_signed", "sum_sign_d", "n_agree", "sum_imb_d", "n_move", "sum_abs_imb")
HEADER_FIELDS = ("n_steps", "n_two_sided", "n_pairs", "sum_d", "sum_abs_d", "n_up", "n_down", "n_bid_side", "n_ask_side")
M64 = (1 << 64) - 1
NO_ASK = 0xFFFFFFFF


def levels_of(hist):
    W = np.asarray(hist).shape[-1]
    assert W >= 9 and (W - 5) % 4 == 0
    return (W - 5) // 4


def cleared(L):
    """the unreduced sums [L] of the levels and of the header without a step, and no past"""
    return {"L": L, "rows": [{n: 0 for n in FIELDS} for _ in range(L)], "header": {n: 0 for n in HEADER_FIELDS}, "past": None}


def fold(hist, cuts=(), first_step=0, into=None):
    """fold the records hist[i] = step first_step + i into ``into`` (default: a cleared table) and return it"""
    hist = np.asarray(hist)
    s = cleared(levels_of(hist)) if into is None else into
    L, h = s["L"], s["header"]
    assert levels_of(hist) == L
    past = s["past"]  # None, or (m or None, [I_q]) of the step before
    cuts = set(int(c) for c in cuts)
    for i, rec in enumerate(hist):
        if first_step + i in cuts:
            past = None
        rec = [int(x) for x in rec]
        bid, ask = rec[1], rec[2]
        two = bid != 0 and ask != NO_ASK
        m = bid + ask if two else None
        h["n_steps"] += 1
        h["n_two_sided"] += 1 if two else 0
        h["n_bid_side"] += 1 if bid != 0 else 0
        h["n_ask_side"] += 1 if ask != NO_ASK else 0
        pair = two and past is not None and past[0] is not None
        d = m - past[0] if pair else None
        if pair:
            h["n_pairs"] += 1
            h["sum_d"] += d
            h["sum_abs_d"] += abs(d)
            h["n_up"] += 1 if d > 0 else 0
            h["n_down"] += 1 if d < 0 else 0
        imb, run = [], 0
        for q in range(L):
            bv, bn, av, an = rec[5 + 4 * q:9 + 4 * q]
            run += bv - av
            imb.append(run)
            r = s["rows"][q]
            r["sum_bid_vol"] += bv
            r["sum_ask_vol"] += av
            r["sum_bid_vol_sq"] += bv * bv
            r["sum_ask_vol_sq"] += av * av
            r["sum_bid_orders"] += bn
            r["sum_ask_orders"] += an
            r["n_bid_steps"] += 1 if bn > 0 else 0
            r["n_ask_steps"] += 1 if an > 0 else 0
            if two:
                r["sum_imb"] += run
                r["sum_imb_sq"] += run * run
                r["sum_abs_imb"] += abs(run)
            if pair:
                J = past[1][q]
                sign = (J > 0) - (J < 0)
                r["n_signed"] += 1 if J != 0 else 0
                r["sum_sign_d"] += sign * d
                r["n_agree"] += 1 if sign * d > 0 else 0
                r["sum_imb_d"] += J * d
                r["n_move"] += 1 if J != 0 and d != 0 else 0
        past = (m, imb)
    s["past"] = past
    return s


def cut(s):
    """what a reset of the book does: the past is forgotten, the sums go on"""
    s["past"] = None
    return s


def words(s):
    """the L + 1 rows of 16 words modulo 2**64 as Python integers"""
    out = [[r[n] & M64 for n in FIELDS] for r in s["rows"]]
    out.append([s["header"][n] & M64 for n in HEADER_FIELDS] + [0] * (16 - len(HEADER_FIELDS)))
    return out


def carry(s):
    """the L + 1 carry words: I_q of the last step per level, then its word - bit 63 two-sided, the low bits m; all 0
    behind a cut or a clear"""
    if s["past"] is None:
        return [0] * (s["L"] + 1)
    m, imb = s["past"]
    return [x & M64 for x in imb] + [0 if m is None else (1 << 63) | m]


def table(s):
    """... as uint64 [L + 1, 16]"""
    return np.array(words(s), dtype=np.uint64)


def rows(hist, cuts=None, first_step=0):
    """hist [n_steps, n_books, W] -> uint64 [n_books, L + 1, 16]; cuts: {book: steps}"""
    cuts = cuts or {}
    return np.array([table(fold(hist[:, b], cuts.get(b, ()), first_step)) for b in range(hist.shape[1])], dtype=np.uint64)
