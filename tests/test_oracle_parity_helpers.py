"""The shared device-against-oracle checks (tests/oracle_parity.py) bite: run without a GPU on a stand-in env that answers
the readers of ManyBookEnv from copies of an oracle run's own data.  The unmodified stand-in passes every check; each single
change of one value makes the matching check raise."""
import copy

import numpy as np
import pytest

import oracle_parity as P

C3_GROUPS = [(64, (32, 64), (10, 20), 2, 0.8), (64, (32, 64), (50, 70), 2, 0.2)]
N_BOOKS, STEPS, BOOK = 4, 30, 1


class StandIn:
    """The readers the checks call, answered from copies of the oracle's data in the device's forms (key prices of bids
    flipped through MAX_PRICE, live orders in price-time priority)."""

    def __init__(self, ref, n_books):
        self.n_books = n_books
        views = [ref.book(b) for b in range(n_books)]
        self.hist = ref.history().copy()
        self.trade_recs = [v.trades_array().copy() for v in views]
        self.order_recs = [v.orders_array().copy() for v in views]
        self.keys = []
        self.live = []
        for v, o in zip(views, self.order_recs):
            kb, kp, kt = v.keys()
            self.keys.append([np.where(kb == 1, P.MAX_PRICE - kp.astype(np.uint64), kp).astype(np.uint32), kt.copy()])
            act = [i for i in range(len(o)) if o["status"][i] == 1]
            bids = sorted((i for i in act if o["side"][i] == 1), key=lambda i: (-int(o["price"][i]), int(kt[i]), i))
            asks = sorted((i for i in act if o["side"][i] == 0), key=lambda i: (int(o["price"][i]), int(kt[i]), i))
            self.live.append(o[bids + asks].copy())
        self.rng = [[int(x) for x in r] for r in ref.rng_states()]
        self.times = [v.get_time() for v in views]
        self.flag_words = np.zeros(n_books, dtype=np.uint32)
        self.states = [copy.deepcopy(P.oracle_state(v)) for v in views]

    def history(self):
        return self.hist

    def trades(self, b, first=0):
        return self.trade_recs[b][first:]

    def orders(self, b):
        return self.order_recs[b]

    def order_count(self, b):
        return len(self.order_recs[b])

    def order_status(self, b, order_id):
        return int(self.order_recs[b]["status"][order_id])

    def order_keys(self, b):
        return tuple(self.keys[b])

    def live_orders(self, b):
        return self.live[b]

    def rng_state(self, b):
        return tuple(self.rng[b])

    def time(self, b):
        return self.times[b]

    def flags(self):
        return self.flag_words

    def trade_counts(self):
        return np.array([len(t) for t in self.trade_recs], dtype=np.uint64)

    def order_counts(self):
        return np.array([len(o) for o in self.order_recs], dtype=np.uint64)

    def book_state(self, b):
        return self.states[b]


@pytest.fixture(scope="module")
def ref(oracle):
    r = oracle.ManyBooks(N_BOOKS, 101, 0, 2, 100_000, True, 10, C3_GROUPS)
    r.run(STEPS)
    return r


@pytest.fixture
def env(ref):
    return StandIn(ref, N_BOOKS)


def test_the_input_is_busy(ref):
    v = ref.book(BOOK)
    assert v.n_orders() > 1000 and v.n_trades() > 500 and int((v.orders_array()["status"] == 1).sum()) > 10


def test_the_unmodified_stand_in_passes_every_check(env, ref):
    P.no_flags(env)
    P.same_history(env.history(), ref.history())
    for b in range(N_BOOKS):
        P.same_history(env.history()[:, b], ref.history()[:, b], f"L2 history of book {b}")
        P.same_book(env, b, ref.book(b), orders=True, keys=True, state=True, priority=True)
    P.assert_same(P.snapshot(env), P.snapshot(StandIn(ref, N_BOOKS)))
    P.assert_same(P.snapshot(env, books=[0, 3]), P.snapshot(StandIn(ref, N_BOOKS), books=[0, 3]))


def _bump(arr, i, field=None):
    """Change one value in place and assert that it changed."""
    a = arr if field is None else arr[field]
    before = a[i].copy()
    a[i] = before ^ a.dtype.type(1)
    assert a[i] != before


def _swap_a_tie(env):
    """Swap two adjacent live orders of one side at one price; the input must hold such a pair."""
    live = env.live[BOOK]
    for k in range(len(live) - 1):
        if live["side"][k] == live["side"][k + 1] and live["price"][k] == live["price"][k + 1]:
            ids = live["order_id"].tolist()
            live[[k, k + 1]] = live[[k + 1, k]]
            assert live["order_id"].tolist() != ids and sorted(live["order_id"].tolist()) == sorted(ids)
            return
    pytest.fail("no two resting orders of one side share a price: the priority check has nothing to order")


def _drop_last_trade(env):
    n = len(env.trade_recs[BOOK])
    env.trade_recs[BOOK] = env.trade_recs[BOOK][:-1]
    assert len(env.trade_recs[BOOK]) == n - 1


def _same_book_all(env, ref):
    P.same_book(env, BOOK, ref.book(BOOK), orders=True, keys=True, state=True)


MUTATIONS = {
    "one trade's vol": (lambda e: _bump(e.trade_recs[BOOK], len(e.trade_recs[BOOK]) // 2, "vol"),
                        lambda e, r: P.same_trades(e, BOOK, r.book(BOOK))),
    "a dropped last trade": (_drop_last_trade, lambda e, r: P.same_trades(e, BOOK, r.book(BOOK))),
    "one live order's vol": (lambda e: _bump(e.live[BOOK], len(e.live[BOOK]) // 2, "vol"),
                             lambda e, r: P.same_live(e, BOOK, r.book(BOOK), priority=False)),
    "two tied live orders swapped": (_swap_a_tie, lambda e, r: P.same_live(e, BOOK, r.book(BOOK))),
    "one order's end_time": (lambda e: _bump(e.order_recs[BOOK], len(e.order_recs[BOOK]) // 3, "end_time"),
                             lambda e, r: P.same_orders(e, BOOK, r.book(BOOK))),
    "one key time": (lambda e: _bump(e.keys[BOOK][1], len(e.keys[BOOK][1]) // 2), lambda e, r: P.same_keys(e, BOOK, r.book(BOOK))),
    "one key price": (lambda e: _bump(e.keys[BOOK][0], len(e.keys[BOOK][0]) // 2), lambda e, r: P.same_keys(e, BOOK, r.book(BOOK))),
    "one L2 word": (lambda e: _bump(e.hist, (STEPS // 2, BOOK, 3)), lambda e, r: P.same_history(e.history(), r.history())),
    "one RNG word": (lambda e: e.rng[BOOK].__setitem__(1, e.rng[BOOK][1] ^ 1),
                     lambda e, r: P.assert_same(P.snapshot(e), P.snapshot(StandIn(r, N_BOOKS)))),
    "one flag bit": (lambda e: _bump(e.flag_words, BOOK), lambda e, r: P.no_flags(e)),
}


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_one_change_makes_the_matching_check_raise(env, ref, name):
    mutate, check = MUTATIONS[name]
    check(env, ref)  # passes before the change
    mutate(env)
    if name == "one RNG word":
        assert env.rng_state(BOOK) != StandIn(ref, N_BOOKS).rng_state(BOOK)
    with pytest.raises(AssertionError):
        check(env, ref)


@pytest.mark.parametrize("name", [n for n in MUTATIONS if n not in ("one L2 word", "one RNG word", "one flag bit")])
def test_same_book_with_every_option_raises_on_each_book_change(env, ref, name):
    MUTATIONS[name][0](env)
    with pytest.raises(AssertionError):
        _same_book_all(env, ref)


def test_a_swapped_tie_passes_only_without_the_priority_check(env, ref):
    _swap_a_tie(env)
    P.same_live(env, BOOK, ref.book(BOOK), priority=False)
    with pytest.raises(AssertionError, match="priority order"):
        P.same_live(env, BOOK, ref.book(BOOK))


def test_an_allowed_flag_passes_and_the_snapshot_still_sees_it(env, ref):
    env.flag_words[BOOK] = 64
    P.no_flags(env, allow=64)
    with pytest.raises(AssertionError, match="device flags"):
        P.no_flags(env, allow=2)
    with pytest.raises(AssertionError):
        P.assert_same(P.snapshot(env), P.snapshot(StandIn(ref, N_BOOKS)))


def test_the_messages_name_the_tag_and_the_first_differing_index(env, ref):
    i = len(env.trade_recs[BOOK]) // 2
    _bump(env.trade_recs[BOOK], i, "vol")
    with pytest.raises(AssertionError, match=rf"\('m', 7\): trade field vol differs first at {i}:"):
        P.same_trades(env, BOOK, ref.book(BOOK), tag=("m", 7))
    _bump(env.hist, (5, 2, 9))
    with pytest.raises(AssertionError, match=r"differs first at \(step, book, word\) = \(5, 2, 9\)"):
        P.same_history(env.history(), ref.history())
