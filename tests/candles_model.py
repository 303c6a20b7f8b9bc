"""The candle table of one book in plain Python: what bk_candles_enable's device fold must leave in a book's bars and carry.

``fold(hist, cfg)`` walks an ``[n_steps, W]`` level-2 history (``env.history()[:, b]``) step by step, in the order of the
contract in include/bourse_amd.h, with Python's unbounded integers; only at the end are the words reduced modulo 2**64.
``cfg`` is ``config(width, n)``: bars of ``width`` steps, ``n`` slots.  Step ``first_step + i`` belongs to bar
``(first_step + i) // width``, kept as a dict per bar; ``table`` then lays the bars that still own their slot into the ``n``
slots - a bar is pushed out by any later bar of the same slot, which is all the device's skipping of bars amounts to.  The
book's past is the step before - twice its mid, None where one-sided - and is forgotten at a cut; ``cuts`` lists the steps IN
FRONT OF which that happens, as a reset of the book at that step count does.  It shares no code with
bourse_amd/csrc/candle_fold.hpp or candles.hpp, and every GPU test compares against it."""
import numpy as np

FIELDS = ("first_step", "n_steps", "n_two_sided", "open_m", "high_m", "low_m", "close_m", "sum_m", "sum_spread", "sum_trade_vol",
          "n_trade_steps", "n_ret", "sum_d", "sum_abs_d", "sum_d2", "max_abs_d")
SIGNED = ("sum_d",)
CANDLE_DTYPE = np.dtype({"names": list(FIELDS), "formats": ["<i8" if n in SIGNED else "<u8" for n in FIELDS],
                         "offsets": [8 * i for i in range(16)], "itemsize": 128})
M64 = (1 << 64) - 1
NO_ASK = 0xFFFFFFFF


def config(width, n):
    assert 1 <= int(width) <= 1 << 20 and 1 <= int(n) <= 1 << 16
    return {"width": int(width), "n": int(n)}


def cleared(cfg):
    """no bar and no past"""
    return {"cfg": cfg, "bars": {}, "past": None, "have_past": False}


def fold(hist, cfg=None, cuts=(), first_step=0, into=None):
    """fold the records hist[i] = step first_step + i into ``into`` (default: a cleared table of ``cfg``) and return it"""
    s = cleared(cfg) if into is None else into
    W, N = s["cfg"]["width"], s["cfg"]["n"]
    past = s["past"] if s["have_past"] else None  # twice the mid of the step before, None: one-sided, cut, or no step
    cuts = set(int(c) for c in cuts)
    for i, rec in enumerate(hist):
        step = first_step + i
        if step in cuts:
            past = None
        tv, bid, ask = int(rec[0]), int(rec[1]), int(rec[2])
        j = step // W
        bar = s["bars"].get(j)
        if bar is None:
            bar = s["bars"][j] = {n: 0 for n in FIELDS}
            bar["first_step"] = step
            bar["has_m"] = False
            for old in [k for k in s["bars"] if k < j and (j - k) % N == 0]:
                del s["bars"][old]  # the slot is this bar's now
        bar["n_steps"] += 1
        bar["sum_trade_vol"] += tv
        bar["n_trade_steps"] += 1 if tv > 0 else 0
        m = bid + ask if bid != 0 and ask != NO_ASK else None
        if m is not None:
            bar["n_two_sided"] += 1
            if not bar["has_m"]:
                bar["open_m"] = bar["high_m"] = bar["low_m"] = m
                bar["has_m"] = True
            bar["high_m"] = max(bar["high_m"], m)
            bar["low_m"] = min(bar["low_m"], m)
            bar["close_m"] = m
            bar["sum_m"] += m
            bar["sum_spread"] += (ask - bid) & 0xFFFFFFFF
            if past is not None:
                d = m - past
                bar["n_ret"] += 1
                bar["sum_d"] += d
                bar["sum_abs_d"] += abs(d)
                bar["sum_d2"] += d * d
                bar["max_abs_d"] = max(bar["max_abs_d"], abs(d))
        past = m
        s["have_past"] = True
    s["past"] = past
    return s


def cut(s):
    """what a reset of the book does: the past is forgotten, the bars go on"""
    s["past"], s["have_past"] = None, False
    return s


def words(s):
    """the n slots of 16 words modulo 2**64 as Python integers: bar j in slot j % n, an empty slot all zeros"""
    N = s["cfg"]["n"]
    out = [[0] * 16 for _ in range(N)]
    for j in sorted(s["bars"]):  # (a later bar of the same slot has already pushed the earlier one out; sorted all the same)
        out[j % N] = [s["bars"][j][n] & M64 for n in FIELDS]
    return out


def carry(s):
    """the carry word: the last step's - bit 63 two-sided, the low bits m; 0 behind a cut or a clear"""
    return 0 if not s["have_past"] or s["past"] is None else (1 << 63) | s["past"]


def table(s):
    """... as CANDLE_DTYPE [n]"""
    return np.array(words(s), dtype=np.uint64).view(CANDLE_DTYPE).reshape(-1)


def rows(hist, cfg, cuts=None, first_step=0):
    """hist [n_steps, n_books, W] -> CANDLE_DTYPE [n_books, n]; cuts: {book: steps}"""
    cuts = cuts or {}
    return np.array([table(fold(hist[:, b], cfg, cuts.get(b, ()), first_step)) for b in range(hist.shape[1])], dtype=CANDLE_DTYPE)
