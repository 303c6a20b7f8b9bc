"""A model of the flow table (bk_flow_enable; include/bourse_amd.h) in plain Python integers.  It shares no code with the
kernel or with bourse_amd/csrc/flow_fold.hpp: it keeps the book's last K records as a list, visits every index of a fold
one by one, and asks for each whether it can be read.

A tape is a sequence of records ``(price, vol, side_is_bid)`` indexed as the book counts them.  ``FlowModel.fold(tape,
total, base, capacity)`` folds the indices ``[seen, total)`` the way one device fold does that read ``total`` and ``base``
from the header; ``cut(total)`` is what a reset does, ``clear(total)`` a full clear.  ``words()`` is the book's
``8 + 6 K`` words modulo 2^64, ``carry()`` the K window words as the device keeps them."""
M64 = (1 << 64) - 1
BASE = ("n_trades", "n_buy", "sum_vol", "buy_vol", "sum_vol_sq", "notional", "max_vol", "n_lost")
LAG = ("n_pairs", "sum_ss", "sum_resp", "sum_back", "sum_abs_dp", "sum_dp2")


class FlowModel:
    def __init__(self, n_lags, seen=0):
        assert 1 <= n_lags <= 64
        self.K = n_lags
        self.clear(seen)

    def clear(self, seen):
        self.base = dict.fromkeys(BASE, 0)
        self.lags = [dict.fromkeys(LAG, 0) for _ in range(self.K)]
        self.cut(seen)

    def cut(self, seen):
        """no pair reaches over this point; the sums go on"""
        self.last = [None] * self.K  # last[j]: the record of index seen - 1 - j as (price, sign), None if it was not read
        self.seen = seen

    def fold(self, tape, total, base=0, capacity=1 << 62):
        i = self.seen
        while i < total:
            if not (base <= i and i - base < capacity):
                # unreadable; a run of them that outlasts the window is skipped in one stride (the device must not walk it)
                nxt = base if i < base else total
                run = min(nxt, total) - i
                if run > self.K:
                    self.base["n_lost"] += run - self.K
                    self.last = [None] * self.K
                    i += run - self.K
                self.base["n_lost"] += 1
                self.last = [None] + self.last[:-1]
                i += 1
                continue
            price, vol, side_is_bid = (int(x) for x in tape[i])
            s = 1 if side_is_bid == 0 else -1
            b = self.base
            b["n_trades"] += 1
            b["n_buy"] += s > 0
            b["sum_vol"] += vol
            b["buy_vol"] += vol if s > 0 else 0
            b["sum_vol_sq"] += vol * vol
            b["notional"] += vol * price
            b["max_vol"] = max(b["max_vol"], vol)
            for k in range(1, self.K + 1):
                old = self.last[k - 1]
                if old is None:
                    continue
                dp = price - old[0]
                row = self.lags[k - 1]
                row["n_pairs"] += 1
                row["sum_ss"] += s * old[1]
                row["sum_resp"] += old[1] * dp
                row["sum_back"] += s * dp
                row["sum_abs_dp"] += abs(dp)
                row["sum_dp2"] += dp * dp
            self.last = [(price, s)] + self.last[:-1]
            i += 1
        self.seen = max(self.seen, total)

    def words(self):
        out = [self.base[n] & M64 for n in BASE]
        for row in self.lags:
            out += [row[n] & M64 for n in LAG]
        return out

    def carry(self):
        return [0 if r is None else (1 << 63) | ((1 << 62) if r[1] > 0 else 0) | r[0] for r in self.last]


def fold_tape(tape, n_lags, folds, cuts=(), start=0):
    """``folds``: one ``(total, base, capacity)`` per fold, in order; ``cuts``: ``{index of a fold: the count the reset behind it
    restores}``.  Returns ``(words, carry, cursor)``."""
    m = FlowModel(n_lags, start)
    cuts = dict(cuts)
    for n, (total, base, capacity) in enumerate(folds):
        m.fold(tape, total, base, capacity)
        if n in cuts:
            m.cut(cuts[n])
    return m.words(), m.carry(), m.seen


def brute_words(tape, n_lags, readable):
    """The same words by a double loop over all pairs of a tape of which ``readable[i]`` says whether index i was read."""
    m = FlowModel(n_lags)
    for i, rec in enumerate(tape):
        if not readable[i]:
            m.base["n_lost"] += 1
            continue
        p, v, side = (int(x) for x in rec)
        s = 1 if side == 0 else -1
        m.base["n_trades"] += 1
        m.base["n_buy"] += s > 0
        m.base["sum_vol"] += v
        m.base["buy_vol"] += v if s > 0 else 0
        m.base["sum_vol_sq"] += v * v
        m.base["notional"] += v * p
        m.base["max_vol"] = max(m.base["max_vol"], v)
        for k in range(1, n_lags + 1):
            if i - k < 0 or not readable[i - k]:
                continue
            q, _, side_k = (int(x) for x in tape[i - k])
            sk = 1 if side_k == 0 else -1
            row, dp = m.lags[k - 1], p - q
            row["n_pairs"] += 1
            row["sum_ss"] += s * sk
            row["sum_resp"] += sk * dp
            row["sum_back"] += s * dp
            row["sum_abs_dp"] += abs(dp)
            row["sum_dp2"] += dp * dp
    return m.words()


def rows_of(words_per_book, n_lags):
    """a list of per-book word lists -> a ``flow_dtype(n_lags)`` array, for a bit-for-bit comparison with ``env.flow()``"""
    import numpy as np

    from bourse_amd import _lib

    a = np.array(words_per_book, dtype=np.uint64).reshape(len(words_per_book), 8 + 6 * n_lags)
    return np.ascontiguousarray(a).view(_lib.flow_dtype(n_lags)).reshape(len(words_per_book))
