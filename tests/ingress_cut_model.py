"""Where a market's instruction batches stop, one element at a time: the rule every submit entry of a device-ingress env
and bk_submit_quotes must follow (include/bourse_amd.h: BK_PRICE_NOT_TICK_MULTIPLE, BK_CAPACITY, ``status``, ``out_ids``).

``run_market(books, queue_len, queue_cap)`` takes one market: its books in asset order as ``(tick, next_id, batch)`` -
the book's tick size, its id counter at the call and its batch ``(action, side, vol, trader, price, order_id)`` as six
equally long sequences -, the length of the market's event queue at the call and the queue's capacity.  A book on its own
is a market of one asset.

The rule for element i of a book's batch:
  * it is NEW when ``action == 1``;
  * it is an EVENT when ``action`` is 1, 2 or BK_ACTION_MODIFY; every other action (0, 3, 7, ...) is applied and
    produces nothing;
  * a new element whose price the tick does not divide stops the book with code 1;
  * otherwise an event stops the book with code 3 when the queue is full;
  * otherwise the element is applied: an event takes the next queue position, a new order the book's next id.

What follows from it:
  * ``applied`` is i at a stop, else the length of the batch;
  * an element that is no event and stands after the queue filled, but before the first event that does not fit, counts
    as applied;
  * a bad price is looked at before the queue is: a new order with a bad price on a full queue stops with code 1;
  * the next asset starts with the queue length the previous one left - after a sibling's stop too.

Per book the result holds ``code``, ``applied``, ``ids`` (per element: the id a new order took, NO_ID = 2**64 - 1 for
an applied element that created nothing, UNTOUCHED from the stop on - no u64 value, see ``ids_array``), ``prefix`` (the
applied elements as six numpy arrays: what an oracle is fed) and ``next_id`` (the id counter the call leaves); for the
market ``events`` - ``(asset, element)`` in queue order, the call's own - and ``queue_len`` after the call.

Plain Python over the elements: no passes, no lanes, no ballots.  It imports nothing of bourse_amd and shares no text with
book_device.hpp's k_ingest or quotes_ingress.hpp's k_submit.
"""
from collections import namedtuple

import numpy as np

MODIFY = 0x80000003  # BK_ACTION_MODIFY
OK, PRICE, CAPACITY = 0, 1, 3  # BK_OK, BK_PRICE_NOT_TICK_MULTIPLE, BK_CAPACITY
NO_ID = 2**64 - 1
UNTOUCHED = -1
DTYPES = (np.uint32, np.uint8, np.uint32, np.uint32, np.uint32, np.uint64)

Book = namedtuple("Book", "code applied ids prefix next_id")
Market = namedtuple("Market", "books events queue_len")


def is_new(action):
    return int(action) == 1


def is_event(action):
    return int(action) in (1, 2, MODIFY)


def run_book(tick, next_id, batch, queue_len, queue_cap):
    """one book: (Book, the elements that were queued in order, the queue length it leaves)"""
    action, price = batch[0], batch[4]
    n = len(action)
    code, applied, ids, queued = OK, n, [], []
    for i in range(n):
        if is_new(action[i]) and int(price[i]) % tick != 0:
            code, applied = PRICE, i
            break
        if is_event(action[i]):
            if queue_len >= queue_cap:
                code, applied = CAPACITY, i
                break
            queue_len += 1
            queued.append(i)
        if is_new(action[i]):
            ids.append(next_id)
            next_id += 1
        else:
            ids.append(NO_ID)
    ids += [UNTOUCHED] * (n - applied)
    prefix = tuple(np.asarray(x, dtype=dt)[:applied].copy() for x, dt in zip(batch, DTYPES))
    return Book(code, applied, ids, prefix, next_id), queued, queue_len


def run_market(books, queue_len, queue_cap):
    out, events = [], []
    for asset, (tick, next_id, batch) in enumerate(books):
        book, queued, queue_len = run_book(int(tick), int(next_id), batch, queue_len, queue_cap)
        out.append(book)
        events += [(asset, i) for i in queued]
    return Market(out, events, queue_len)


def ids_array(ids, untouched):
    """a book's (or several books', concatenated) ids as u64, with `untouched` where the call writes nothing"""
    return np.array([untouched if i == UNTOUCHED else i for i in ids], dtype=np.uint64)
