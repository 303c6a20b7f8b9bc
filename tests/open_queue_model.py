"""The queue rows of one book in plain Python: what bk_open_queue_enable's device refresh must leave beside a book's entries.

``rows(orders, key_time, entries)`` takes a book's ``orders_array()`` (the fields ``status``, ``order_id``, ``side``,
``price``, ``vol``), the time of every order's priority key by order id (a book view's ``keys()[2]``: the arrival, or the
modification that re-keyed the order) and the open-order model's entry lists (``open_orders_model.rows_ints(..)[1]``: per
trader ``depth`` tuples ``(order id, price, remaining volume, side_is_bid)``), and returns ``queue[n_traders, depth]``.  Python
ints only; shares no code with bourse_amd/csrc/open_queue_rows.hpp or open_queue.hpp, and every GPU test compares against it.

The rule (include/bourse_amd.h): the orders with status Active (1) rest, whoever owns them.  On its side they stand in
priority order - a bid's higher price first, an ask's lower, then the key time, then the id.  (The device orders a level by
its pool stamp; the two agree while a step has fewer events than step_size, as all of the project's parity does.)  The row of
a listed order: the volume and the count of the orders before it, the part of both at its own price, and the volume of
everything at its price, itself included.  An unused entry, and an entry whose id does not rest, has the all-zero row.

Plain module: importing it needs numpy alone.
"""
import numpy as np

ACTIVE = 1
NO_ORDER = 0xFFFFFFFF
OPEN_QUEUE_DTYPE = np.dtype([("ahead_vol", "<u8"), ("level_ahead_vol", "<u8"), ("level_vol", "<u8"), ("ahead_orders", "<u4"),
                             ("level_ahead_orders", "<u4")])
EMPTY_ROW = (0, 0, 0, 0, 0)


def sides(orders, key_time):
    """{side_is_bid: [(order id, price, remaining volume), ...] in priority order} of the resting orders"""
    out = {0: [], 1: []}
    for o in orders:
        if int(o["status"]) == ACTIVE:
            i = int(o["order_id"])
            out[int(o["side"]) & 1].append((int(o["price"]), int(key_time[i]), i, int(o["vol"])))
    out[0].sort(key=lambda x: (x[0], x[1], x[2]))
    out[1].sort(key=lambda x: (-x[0], x[1], x[2]))
    return {s: [(i, p, v) for p, _, i, v in q] for s, q in out.items()}


def rows_ints(orders, key_time, entries):
    """per trader a list of depth rows as tuples of Python ints"""
    queues = sides(orders, key_time)
    place = {i: (s, k) for s, q in queues.items() for k, (i, _, _) in enumerate(q)}
    out = []
    for listed in entries:
        rows = []
        for entry in listed:
            i = int(entry[0])
            if i == NO_ORDER or i not in place:
                rows.append(EMPTY_ROW)
                continue
            s, k = place[i]
            q, price = queues[s], queues[s][k][1]
            before = q[:k]
            level_before = [x for x in before if x[1] == price]
            rows.append((sum(x[2] for x in before), sum(x[2] for x in level_before), sum(x[2] for x in q if x[1] == price),
                         len(before), len(level_before)))
        out.append(rows)
    return out


def rows(orders, key_time, entries):
    r = rows_ints(orders, key_time, entries)
    depth = len(r[0]) if r else 0
    out = np.zeros((len(r), depth), dtype=OPEN_QUEUE_DTYPE)
    for t, listed in enumerate(r):
        for k, row in enumerate(listed):
            out[t, k] = row
    return out
