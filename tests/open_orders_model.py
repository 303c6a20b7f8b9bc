"""The open-order rows of one book in plain Python: what bk_open_orders_enable's device refresh must leave in a book's rows.

``rows(orders, n_traders, depth)`` takes a book's ``orders_array()`` (the oracle's, or the device's own readers': the fields
``status``, ``trader_id``, ``order_id``, ``side``, ``price``, ``vol``) and returns ``(summary[n_traders],
entries[n_traders, depth])``.  Python ints only; shares no code with bourse_amd/csrc/open_order_rows.hpp or
open_orders.hpp, and every GPU test compares against it.

The rule (include/bourse_amd.h): the orders with status Active (1) rest.  Those of a trader id >= n_traders have no row; with
``max_orders`` given, those of an order id >= max_orders are left out too (the device has no record to look their trader up
in).  Per trader: the sum of the remaining volume and the count per side, the highest own bid price (0 without a bid) and
the lowest own ask price (0xFFFFFFFF without an ask); the entries are the trader's resting orders of either side in
ascending order id, the first ``depth`` of them, padded with the empty entry (0xFFFFFFFF, 0, 0, 0).

Plain module: importing it needs numpy alone.
"""
import numpy as np

ACTIVE = 1
OPEN_SUMMARY_DTYPE = np.dtype([("bid_vol", "<u8"), ("ask_vol", "<u8"), ("n_bid", "<u4"), ("n_ask", "<u4"), ("best_bid", "<u4"),
                               ("best_ask", "<u4")])
OPEN_ORDER_DTYPE = np.dtype([("order_id", "<u4"), ("price", "<u4"), ("vol", "<u4"), ("side_is_bid", "<u4")])
EMPTY_SUMMARY = (0, 0, 0, 0, 0, 0xFFFFFFFF)
EMPTY_ENTRY = (0xFFFFFFFF, 0, 0, 0)


def resting(orders, n_traders, max_orders=None):
    """{trader: [(order id, price, remaining volume, side_is_bid), ...] in ascending order id} of the traders with a row"""
    by_trader = {}
    for o in orders:
        if int(o["status"]) != ACTIVE or int(o["trader_id"]) >= n_traders:
            continue
        if max_orders is not None and int(o["order_id"]) >= max_orders:
            continue
        by_trader.setdefault(int(o["trader_id"]), []).append((int(o["order_id"]), int(o["price"]), int(o["vol"]), int(o["side"]) & 1))
    return {t: sorted(v) for t, v in by_trader.items()}


def rows_ints(orders, n_traders, depth, max_orders=None):
    """(summary rows, entry lists) as tuples of Python ints"""
    mine = resting(orders, n_traders, max_orders)
    summary, entries = [], []
    for t in range(n_traders):
        own = mine.get(t, [])
        bids, asks = [o for o in own if o[3]], [o for o in own if not o[3]]
        summary.append((sum(o[2] for o in bids), sum(o[2] for o in asks), len(bids), len(asks),
                        max((o[1] for o in bids), default=0), min((o[1] for o in asks), default=0xFFFFFFFF)))
        listed = own[:depth]
        entries.append(listed + [EMPTY_ENTRY] * (depth - len(listed)))
    return summary, entries


def rows(orders, n_traders, depth, max_orders=None):
    s, e = rows_ints(orders, n_traders, depth, max_orders)
    summary = np.array(s, dtype=OPEN_SUMMARY_DTYPE)
    entries = np.zeros((n_traders, depth), dtype=OPEN_ORDER_DTYPE)
    for t in range(n_traders):
        for k in range(depth):
            entries[t, k] = e[t][k]
    return summary, entries
