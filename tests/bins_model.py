"""The bin table of one book in plain Python: what bk_bins_enable's device fold must leave in a book's counts and carry.

``fold(hist, cfg)`` walks an ``[n_steps, W]`` level-2 history (``env.history()[:, b]``) step by step, in the order of the
contract in include/bourse_amd.h, with Python's unbounded integers; only at the end are the counts reduced modulo 2**64.
``cfg`` is ``config(spans, n_bins, ret_width, spread_width, vol_width)``.  The book's past - twice the mid of every step since
the start, None where one-sided - is kept as a list and forgotten at a cut; ``cuts`` lists the steps IN FRONT OF which that
happens, as a reset of the book at that step count does.  It shares no code with bourse_amd/csrc/bin_fold.hpp or bins.hpp,
and every GPU test compares against it."""
import numpy as np

M64 = (1 << 64) - 1
NO_ASK = 0xFFFFFFFF


def config(spans=(1,), n_bins=64, ret_width=1, spread_width=1, vol_width=1):
    spans = tuple(int(k) for k in spans)
    assert 1 <= len(spans) <= 4 and all(1 <= k <= 64 for k in spans)
    assert 2 <= n_bins <= 256 and n_bins % 2 == 0 and min(ret_width, spread_width, vol_width) >= 1
    return {"spans": spans, "n_bins": int(n_bins), "ret_width": int(ret_width), "spread_width": int(spread_width),
            "vol_width": int(vol_width)}


def cleared(cfg):
    """the unreduced counts [S + 2][B] without a step, and an empty past"""
    return {"cfg": cfg, "counts": [[0] * cfg["n_bins"] for _ in range(len(cfg["spans"]) + 2)], "past": []}


def fold(hist, cfg=None, cuts=(), first_step=0, into=None):
    """fold the records hist[i] = step first_step + i into ``into`` (default: a cleared table of ``cfg``) and return it"""
    s = cleared(cfg) if into is None else into
    cfg = s["cfg"]
    B, spans = cfg["n_bins"], cfg["spans"]
    S = len(spans)
    past = s["past"]
    cuts = set(int(c) for c in cuts)
    for i, rec in enumerate(hist):
        if first_step + i in cuts:
            past = []
        tv, bid, ask = int(rec[0]), int(rec[1]), int(rec[2])
        m = bid + ask if bid != 0 and ask != NO_ASK else None
        past.append(m)  # past[-1] is step s, past[-1 - k] step s - k; a step in front of the start is not two-sided
        for j, k in enumerate(spans):
            back = past[-1 - k] if k < len(past) else None
            if m is not None and back is not None:
                q = (m - back) // cfg["ret_width"]  # (Python's // is the floor)
                s["counts"][j][max(0, min(B - 1, q + B // 2))] += 1
        if m is not None:
            s["counts"][S][min(((ask - bid) & 0xFFFFFFFF) // cfg["spread_width"], B - 1)] += 1
        s["counts"][S + 1][min(tv // cfg["vol_width"], B - 1)] += 1
        past = past[-max(spans):]
    s["past"] = past
    return s


def cut(s):
    """what a reset of the book does: the past is forgotten, the counts go on"""
    s["past"] = []
    return s


def counts(s):
    """the counts modulo 2**64 as Python integers: [S + 2][B]"""
    return [[c & M64 for c in row] for row in s["counts"]]


def carry(s):
    """the Kmax carry words: entry i is the step i + 1 back from the next one - bit 63 two-sided, the low bits m; else 0"""
    past = s["past"]
    out = []
    for i in range(max(s["cfg"]["spans"])):
        m = past[-1 - i] if i < len(past) else None
        out.append(0 if m is None else (1 << 63) | m)
    return out


def table(s):
    """... as uint64 [S + 2, B]"""
    return np.array(counts(s), dtype=np.uint64)


def rows(hist, cfg, cuts=None, first_step=0):
    """hist [n_steps, n_books, W] -> uint64 [n_books, S + 2, B]; cuts: {book: steps}"""
    cuts = cuts or {}
    return np.array([table(fold(hist[:, b], cfg, cuts.get(b, ()), first_step)) for b in range(hist.shape[1])], dtype=np.uint64)
