"""The trader accounts of one book in plain Python: what bk_accounts_enable's device fold must leave in a book's rows.

``fold(trades, orders, n_traders)`` takes a book's ``trades_array()`` and ``orders_array()`` (the oracle's, or the device's
own readers': the fields ``side``, ``price``, ``vol``, ``active_id``, ``passive_id`` of a trade, ``trader_id`` of an order)
and returns ``[n_traders]`` rows of ``(position, cash, volume, fills)``.  Python ints reduced modulo 2**64 once at the end;
shares no code with bourse_amd/csrc/account_fold.hpp or accounts.hpp, and every GPU test compares against it.

The rule (include/bourse_amd.h): the buyer of a trade record is the passive order's trader when ``side`` (side_is_bid: the
passive order's side) is 1, else the active order's trader; the other one sells.  The buyer's position grows by vol and the
cash falls by vol * price, the seller's the other way round; both count vol in ``volume`` and 1 in ``fills`` (a self-trade:
twice in one row).  A trader id >= n_traders has no row.

Plain module: importing it needs numpy alone.
"""
import numpy as np

M64 = (1 << 64) - 1
ACCOUNT_DTYPE = np.dtype([("position", "<i8"), ("cash", "<i8"), ("volume", "<u8"), ("fills", "<u8")])


def _signed(x):
    x &= M64
    return x - (1 << 64) if x >> 63 else x


def record(side_is_bid, price, vol, active_trader, passive_trader):
    """One trade record as ((buyer, (d_position, d_cash, d_volume, d_fills)), (seller, (...))) in unbounded ints."""
    buyer, seller = (passive_trader, active_trader) if side_is_bid else (active_trader, passive_trader)
    return (buyer, (vol, -vol * price, vol, 1)), (seller, (-vol, vol * price, vol, 1))


def fold_ints(trades, orders, n_traders, first=0):
    """Rows as lists of unbounded Python ints, from trade record ``first`` on."""
    rows = [[0, 0, 0, 0] for _ in range(n_traders)]
    trader = [int(t) for t in orders["trader_id"]]
    for k in range(first, len(trades)):
        t = trades[k]
        for who, delta in record(int(t["side"]), int(t["price"]), int(t["vol"]), trader[int(t["active_id"])],
                                 trader[int(t["passive_id"])]):
            if who < n_traders:
                for i in range(4):
                    rows[who][i] += delta[i]
    return rows


def to_rows(rows):
    """Unbounded rows -> ACCOUNT_DTYPE, every word modulo 2**64 (two's complement for the signed ones)."""
    out = np.zeros(len(rows), dtype=ACCOUNT_DTYPE)
    for i, (p, c, v, f) in enumerate(rows):
        out[i] = (_signed(p), _signed(c), v & M64, f & M64)
    return out


def fold(trades, orders, n_traders, first=0):
    return to_rows(fold_ints(trades, orders, n_traders, first))


def parties_per_chunk(trades, orders, first, n_traders, chunk=64):
    """The largest number of parties (of ids < n_traders) that one chunk of `chunk` records, counted from record `first`,
    has on a single trader - what the device's in-wave conflict resolution meets."""
    trader = orders["trader_id"]
    worst = 0
    for lo in range(first, len(trades), chunk):
        t = trades[lo:lo + chunk]
        ids = np.concatenate([trader[t["active_id"].astype(np.int64)], trader[t["passive_id"].astype(np.int64)]])
        ids = ids[ids < n_traders]
        if len(ids):
            worst = max(worst, int(np.bincount(ids.astype(np.int64)).max()))
    return worst
