"""The per-step trade bars of one book in plain Python: what bk_trade_bars_enable's device fold must leave in a book's ring.

``fold(trades, counts, window)`` takes a book's ``trades_array()`` (the oracle's, or the device's own reader's: the fields
``side``, ``price``, ``vol`` of a trade, in record order) and ``counts``, the number of records each step made, and returns
the ring ``[window]`` of ``(open, high, low, close, buy_vol, sell_vol, notional, n_buy, n_sell)`` as it stands after the
last of those steps.  Python ints reduced modulo 2**64 (the counts: 2**32) once at the end; shares no code with
bourse_amd/csrc/trade_bar_fold.hpp or trade_bars.hpp, and every GPU test compares against it.

The rule (include/bourse_amd.h): step ``k`` (``first_step`` is the step counter of ``counts[0]``) goes to slot
``k % window``.  ``side`` is side_is_bid, the PASSIVE order's side: 0 means the aggressor bought, 1 that it sold.  open /
close are the prices of the step's first / last record, high / low the largest / smallest.  A step without a record still
writes its slot: all four prices are the close of slot ``(k - 1) % window`` as it was before the write, every other word 0.
The ring starts as zeros, so the carried price is 0 until the first trade.

Plain module: importing it needs numpy alone.
"""
import numpy as np

M64 = (1 << 64) - 1
M32 = (1 << 32) - 1
TRADE_BAR_DTYPE = np.dtype([("open", "<u4"), ("high", "<u4"), ("low", "<u4"), ("close", "<u4"), ("buy_vol", "<u8"),
                            ("sell_vol", "<u8"), ("notional", "<u8"), ("n_buy", "<u4"), ("n_sell", "<u4")])
CLOSE = 3


def bar_ints(side, price, vol):
    """The bar of one step's records (at least one) in unbounded ints: lists of side_is_bid, price and vol."""
    buy = [v for s, v in zip(side, vol) if s == 0]
    sell = [v for s, v in zip(side, vol) if s != 0]
    return [price[0], max(price), min(price), price[-1], sum(buy), sum(sell), sum(p * v for p, v in zip(price, vol)),
            len(buy), len(sell)]


def fold_ints(trades, counts, window, first_step=0, first=0):
    """The ring as lists of unbounded Python ints, folding ``counts[j]`` records per step from record ``first`` on."""
    ring = [[0] * 9 for _ in range(window)]
    side, price, vol = ([int(x) for x in trades[f]] for f in ("side", "price", "vol"))
    pos = first
    for j, n in enumerate(counts):
        k = first_step + j
        carried = ring[(k - 1) % window][CLOSE]  # read before the write: with window 1 it is the slot itself
        if n == 0:
            ring[k % window] = [carried] * 4 + [0] * 5
        else:
            ring[k % window] = bar_ints(side[pos:pos + n], price[pos:pos + n], vol[pos:pos + n])
        pos += n
    assert pos <= len(side), (pos, len(side))
    return ring


def to_rows(ring):
    """Unbounded rows -> TRADE_BAR_DTYPE: the 64-bit words modulo 2**64, the counts modulo 2**32."""
    out = np.zeros(len(ring), dtype=TRADE_BAR_DTYPE)
    for i, (o, h, l, c, bv, sv, nt, nb, ns) in enumerate(ring):
        out[i] = (o, h, l, c, bv & M64, sv & M64, nt & M64, nb & M32, ns & M32)
    return out


def fold(trades, counts, window, first_step=0, first=0):
    return to_rows(fold_ints(trades, counts, window, first_step, first))
