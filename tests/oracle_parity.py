"""The comparison of a device env with the CPU oracle, bit for bit: the one copy every GPU test and fuzzer calls.

``env`` is a bourse_amd ManyBookEnv / ManyMarketEnv (or anything that answers the same readers), ``view`` an oracle book
(pyoracle._BookView: ``ManyBooks.book(b)``, ``StepEnv.book``, an ``OrderBook``).  The device's and the oracle's records carry
the same field names, so "every field" means every field of either.  pytest rewrites asserts only in test modules: every
assert here carries its own message - the tag (the book, unless the caller names it otherwise), what was compared and the
first differing index.

Plain module next to kernel_cases.py: tests and scripts/ import it the same way.  Importing it needs numpy alone and
initialises nothing: the oracle's Python module is imported only where a check builds the oracle's JSON state.
"""
import numpy as np

MAX_PRICE = 2**32 - 1  # u32::MAX, the price a bid's key is flipped through (pyoracle.MAX_PRICE)


def _first(got, want):
    """(index, got, want) at the first element where two equally shaped arrays differ."""
    i = tuple(int(x) for x in np.argwhere(np.asarray(got) != np.asarray(want))[0])
    i = i[0] if len(i) == 1 else i
    return i, np.asarray(got)[i], np.asarray(want)[i]


def same_array(got, want, tag, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{tag}: {what}: shape {got.shape} vs {want.shape}"
    if not np.array_equal(got, want):
        i, g, w = _first(got, want)
        raise AssertionError(f"{tag}: {what} differs first at {i}: {g} vs {w}")


def same_records(got, want, tag, what):
    """Two record arrays (trades or orders): equal length, then every field."""
    assert len(got) == len(want), f"{tag}: {len(got)} {what} records vs {len(want)}"
    assert got.dtype.names == want.dtype.names, f"{tag}: {what} fields {got.dtype.names} vs {want.dtype.names}"
    for f in want.dtype.names:
        same_array(got[f], want[f], tag, f"{what} field {f}")


def no_flags(env, allow=0):
    f = env.flags()
    assert not (f & ~np.uint32(allow)).any(), f"device flags {np.unique(f)} in books {np.flatnonzero(f & ~np.uint32(allow))[:8]}"


def same_history(hist, want, tag="L2 history"):
    """Level-2 records of a run: [step, book, word], or one book's [step, word]."""
    assert hist.shape == want.shape, f"{tag}: shape {hist.shape} vs {want.shape}"
    if not np.array_equal(hist, want):
        bad = tuple(int(x) for x in np.argwhere(hist != want)[0])
        axes = "(step, book, word)" if hist.ndim == 3 else "(step, word)"
        raise AssertionError(f"{tag} differs first at {axes} = {bad}: {hist[bad]} vs {want[bad]}")


def same_trades(env, b, view, tag=None):
    same_records(env.trades(b, first=0), view.trades_array(), (b,) if tag is None else tag, "trade")


def _live_set(a):
    return set(zip(a["order_id"].tolist(), a["price"].tolist(), a["vol"].tolist(), a["side"].tolist()))


def same_live(env, b, view, tag=None, priority=True):
    """The resting orders of device book b are the oracle's Active ones: count, the set of (id, price, vol, side) and, with
    ``priority``, each side's ids in price-time priority - bids by price descending, asks ascending, then the time of the
    oracle's key (the arrival, or the modification that re-keyed the order), then the id."""
    tag = (b,) if tag is None else tag
    o = view.orders_array()
    act = o[o["status"] == 1]
    live = env.live_orders(b)
    assert len(live) == len(act), f"{tag}: {len(live)} live orders vs {len(act)}"
    got, want = _live_set(live), _live_set(act)
    assert got == want, f"{tag}: live orders (id, price, vol, side): only on the device {sorted(got - want)[:4]}, " \
                        f"only in the oracle {sorted(want - got)[:4]}"
    if priority:
        key_t = view.keys()[2]
        for side in (1, 0):
            ids = live["order_id"][live["side"] == side].tolist()
            rule = sorted(ids, key=lambda i: (-int(o["price"][i]) if side else int(o["price"][i]), int(key_t[i]), i))
            if ids != rule:
                k = next(k for k, (x, y) in enumerate(zip(ids, rule)) if x != y)
                raise AssertionError(f"{tag}: {'bids' if side else 'asks'} out of priority order first at position {k}: "
                                     f"id {ids[k]} vs {rule[k]}")


def same_orders(env, b, view, tag=None):
    """The whole order log, field by field; order_status answers for the middle order."""
    tag = (b,) if tag is None else tag
    want = view.orders_array()
    same_records(env.orders(b), want, tag, "order")
    assert env.order_count(b) == len(want), f"{tag}: order_count {env.order_count(b)} vs {len(want)}"
    if len(want):
        i = len(want) // 2
        got = env.order_status(b, int(want["order_id"][i]))
        assert got == int(want["status"][i]), f"{tag}: order_status of id {int(want['order_id'][i])}: {got} vs {int(want['status'][i])}"


def same_keys(env, b, view, tag=None):
    """env.order_keys(b) against the oracle's keys: a bid's key price is MAX_PRICE - price on the oracle's side."""
    tag = (b,) if tag is None else tag
    kp, kt = env.order_keys(b)
    wb, wp, wt = view.keys()
    assert len(kp) == len(wp), f"{tag}: {len(kp)} order keys vs {len(wp)}"
    same_array(np.where(wb == 1, MAX_PRICE - kp.astype(np.uint64), kp), wp, tag, "key price")
    same_array(kt, wt, tag, "key time")


def oracle_state(view):
    """The oracle book as the reference's JSON snapshot holds it (OrderBook.state reads through a view's own queries)."""
    import pyoracle

    view._trading = True
    return pyoracle.OrderBook.state(view)


def same_book(env, b, view, *, orders=False, keys=False, state=False, priority=True, tag=None):
    """Device book b against an oracle view: trades and live orders; optionally the order log, the keys, the JSON state."""
    tag = (b,) if tag is None else tag
    same_trades(env, b, view, tag)
    same_live(env, b, view, tag, priority)
    if orders:
        same_orders(env, b, view, tag)
    if keys:
        same_keys(env, b, view, tag)
    if state:
        assert env.book_state(b) == oracle_state(view), f"{tag}: book_state differs from the oracle's state()"


# ------------------------------------------------------------------------------------------- one env against another
def snapshot(env, books=None):
    """Everything a run leaves that a second env can be held against (per-book items for ``books``, default all)."""
    books = range(env.n_books) if books is None else books
    return {"history": env.history(), "trade_counts": env.trade_counts(), "order_counts": env.order_counts(),
            "flags": env.flags(), "trades": [env.trades(b, first=0) for b in books],
            "live": [env.live_orders(b) for b in books], "rng": [env.rng_state(b) for b in books],
            "time": [env.time(b) for b in books]}


def assert_same(x, y):
    """Two snapshots (or dicts shaped like them: arrays, or per-book lists of arrays / tuples / numbers)."""
    assert x.keys() == y.keys(), f"snapshot items {sorted(x)} vs {sorted(y)}"
    for k in x:
        if isinstance(x[k], list):
            assert len(x[k]) == len(y[k]), f"{k}: {len(x[k])} books vs {len(y[k])}"
            for i, (u, v) in enumerate(zip(x[k], y[k])):
                if isinstance(u, np.ndarray) and u.dtype.names:
                    same_records(u, v, (k, i), k)
                elif isinstance(u, np.ndarray):
                    same_array(u, v, (k, i), k)
                else:
                    assert u == v, f"{(k, i)}: {u} vs {v}"
        else:
            same_array(x[k], y[k], k, "snapshot")
