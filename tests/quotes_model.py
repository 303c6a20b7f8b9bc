"""bk_submit_quotes in plain Python: the dense instruction grid a book's quote rows stand for.

``expand(entries_of_book, quotes_of_book, depth)`` takes the book's entry lists as ``open_orders_model.rows_ints`` returns
them (per trader ``depth`` tuples ``(order id, price, remaining volume, side_is_bid)``, unused ones ``(0xFFFFFFFF, 0, 0,
0)``) and one quote row ``(bid_price, bid_vol, ask_price, ask_vol)`` per trader, and returns the grid ``(action, side, vol,
trader, price, order_id)`` as six numpy arrays of ``n_traders * (depth + 2)`` elements in ``ingress_support.apply_oracle``'s
/ ``submit``'s format.  Python ints only; shares no code with bourse_amd/csrc/quote_rows.hpp or quotes_ingress.hpp.

The rule (include/bourse_amd.h): a trader's positions ``0 .. depth-1`` are its entry slots, ``depth`` is the new bid and
``depth + 1`` the new ask.  Per side with target ``(P, V)``: ``V == KEEP`` does nothing; ``V == 0`` cancels every listed order of
the side; otherwise the keeper is the first listed order of the side at price ``P``, every other listed order of the side is
cancelled, a keeper holding more than ``V`` gets a volume-only modification to ``V``, one holding less stays and a new order
``(P, V - held)`` follows, and without a keeper the new order is ``(P, V)``.

``counts`` (a dict, optional) receives what happened: cancel, reduce, topup, fresh, untouched, keep_side, pulled_side, and
under ``keepers`` the ids of the orders that kept.

Plain module: importing it needs numpy alone.
"""
import numpy as np

KEEP = 0xFFFFFFFF
NO_ORDER = 0xFFFFFFFF
MOD = 0x80000003
NOTHING = (0, 0, 0, 0, 0, 0)


def side_plan(listed, price, vol):
    """One side of one trader: `listed` = [(slot, order id, price, remaining volume)] in list order.  Returns ({slot: element},
    new-order element or None, what happened as a list of words, the keeper's id or None); elements without the trader."""
    if vol == KEEP:
        return {}, None, ["keep_side"], None
    if vol == 0:
        return {slot: ("cancel", oid) for slot, oid, _, _ in listed}, None, ["pulled_side"] + ["cancel"] * len(listed), None
    at_price = [x for x in listed if x[2] == price]
    keeper = at_price[0] if at_price else None
    slots, words = {}, []
    for x in listed:
        if x is not keeper:
            slots[x[0]] = ("cancel", x[1])
            words.append("cancel")
    if keeper is None:
        return slots, (price, vol), words + ["fresh"], None
    held = keeper[3]
    if held > vol:
        slots[keeper[0]] = ("reduce", keeper[1], vol)
        return slots, None, words + ["reduce"], keeper[1]
    if held < vol:
        return slots, (price, vol - held), words + ["topup"], keeper[1]
    return slots, None, words + ["untouched"], keeper[1]


def expand(entries_of_book, quotes_of_book, depth, counts=None):
    G = depth + 2
    grid = []
    assert len(entries_of_book) == len(quotes_of_book)
    for t, (entries, quote) in enumerate(zip(entries_of_book, quotes_of_book)):
        assert len(entries) == depth
        bid_price, bid_vol, ask_price, ask_vol = (int(x) for x in quote)
        row = [NOTHING] * G
        for is_bid, price, vol, new_at in ((1, bid_price, bid_vol, depth), (0, ask_price, ask_vol, depth + 1)):
            listed = [(k, int(e[0]), int(e[1]), int(e[2])) for k, e in enumerate(entries)
                      if int(e[0]) != NO_ORDER and (int(e[3]) & 1) == is_bid]
            slots, new, words, keeper = side_plan(listed, price, vol)
            for k, what in slots.items():
                row[k] = (2, 0, 0, t, 0, what[1]) if what[0] == "cancel" else (MOD, 4, what[2], t, 0, what[1])
            if new is not None:
                row[new_at] = (1, is_bid, new[1], t, new[0], 0)
            if counts is not None:
                for w in words:
                    counts[w] = counts.get(w, 0) + 1
                if keeper is not None:
                    counts.setdefault("keepers", []).append(keeper)
        grid += row
    col = lambda k, dt: np.array([r[k] for r in grid], dtype=dt)
    return (col(0, np.uint32), col(1, np.uint8), col(2, np.uint32), col(3, np.uint32), col(4, np.uint32), col(5, np.uint64))

