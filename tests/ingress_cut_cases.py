"""The runs of tests/test_gpu_ingress_cuts.py, made without a GPU: what each env is fed, submit by submit, and what
tests/ingress_cut_model.py says every book must report.  tests/test_ingress_cut_model.py asserts every case's conditions
on the CPU, the GPU module asserts them again before it touches the device.

A case is a list of steps, a step a list of submits, a submit the batch of every book with the model's result per book.
Every case runs: the warm-up steps (W resting orders per book, which the later cancellations and modifications name, in
pieces the queue takes), the main step - at most one submit that fills the failing book's queue, then the submit under
test -, and one further well-formed step.

Shapes: 6 books with tick 2, or 4 markets of 2 assets.  The failing book is book 2 (its market's books are 2 and 3); its
neighbours carry batches of 150, 1, 0, 64 and 150 elements (one more of 1 on a market env), so its batch starts at element
151 of the arrays.  A neighbour's batch is a well-formed mix whose events beyond the queue's room are turned into no-ops.
"""
from collections import namedtuple

import numpy as np

import ingress_cut_model as M

MOD = M.MODIFY
W = 8  # resting orders per book from the warm-up: ids 0 .. 7
POOL = 256
FAIL = 2
LENGTHS = {0: 150, 1: 1, 3: 0, 4: 64, 5: 150}
MARKET_LENGTHS = {0: 150, 1: 1, 4: 0, 5: 64, 6: 150, 7: 1}
AMPLE = 160

Submit = namedtuple("Submit", "off ins books under_test")


# --------------------------------------------------------------------------------------------------------- batches
def mix(rng, n, tick, n_ids=W):
    """n elements of all six action kinds of test_gpu_device_ingress.py::_stream_step; cancellations and modifications name
    ids 0 .. n_ids - 1, every price is a multiple of the tick"""
    action = rng.choice([0, 1, 2, MOD, 3, 7], size=n, p=[0.08, 0.5, 0.17, 0.15, 0.05, 0.05]).astype(np.uint32)
    bid = rng.integers(0, 2, size=n).astype(np.uint8)
    has_p, has_v = rng.integers(0, 2, size=n).astype(np.uint8), rng.integers(0, 2, size=n).astype(np.uint8)
    side = np.where(action == MOD, (has_p << 1) | (has_v << 2), bid).astype(np.uint8)
    vol = rng.integers(1, 30, size=n).astype(np.uint32)
    trader = rng.integers(0, 1000, size=n).astype(np.uint32)
    price = (rng.integers(45, 56, size=n) * tick).astype(np.uint32)
    order_id = np.where((action == 2) | (action == MOD), rng.integers(0, n_ids, size=n), 0).astype(np.uint64)
    return [action, side, vol, trader, price, order_id]


def empty():
    return [np.zeros(0, dtype=dt) for dt in M.DTYPES]


def concat(*batches):
    return [np.concatenate([b[k] for b in batches]) for k in range(6)]


def noops(rng, n):
    b = mix(rng, n, 1)
    b[0] = rng.choice([0, 3, 7], size=n).astype(np.uint32)
    return b


def news(n, tick, first=0):
    """n new orders that rest: bids below and asks above every price of a mix"""
    k = first + np.arange(n)
    bid = (k % 2).astype(np.uint8)
    price = np.where(bid == 1, 40 - k // 2 % 8, 60 + k // 2 % 8) * tick
    return [np.ones(n, np.uint32), bid, np.full(n, 50, np.uint32), (2000 + k).astype(np.uint32), price.astype(np.uint32),
            np.zeros(n, np.uint64)]


def events(batch, lo=0, hi=None):
    return sum(M.is_event(a) for a in batch[0][lo:hi])


def set_new(batch, i, price, bid=1):
    batch[0][i], batch[1][i], batch[4][i], batch[5][i] = 1, bid, price, 0


def set_event(batch, i, tick):
    """element i as an event: a new order, a cancellation or a modification, by turns"""
    kind = (1, 2, MOD)[i % 3]
    batch[0][i] = kind
    if kind == 1:
        batch[1][i], batch[4][i], batch[5][i] = i & 1, 50 * tick, 0
    else:
        batch[1][i], batch[5][i] = (6 if kind == MOD else 0), i % W


def set_noop(batch, i):
    batch[0][i] = (0, 3, 7)[i % 3]


def trim(batch, room):
    """the events beyond the first `room` become no-ops"""
    seen = 0
    for i in range(len(batch[0])):
        if M.is_event(batch[0][i]):
            seen += 1
            if seen > room:
                batch[0][i] = 0
    return batch


def join(batches):
    off = np.zeros(len(batches) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(b[0]) for b in batches])
    return off, tuple(np.concatenate([b[k] for b in batches]).astype(dt) for k, dt in enumerate(M.DTYPES))


# --------------------------------------------------------------------------------------------------------- a case
class Case:
    def __init__(self, name, ticks, NM, qcap, stop, want):
        """stop: (book, element) the submit under test must stop at, or None; want: {book: (code, applied)} the case is
        about (the model decides; a case whose model says otherwise is a mistake of the case)"""
        assert 1 <= qcap <= 8192
        self.name, self.ticks, self.NM, self.A, self.B, self.qcap = name, list(ticks), NM, len(ticks), NM * len(ticks), qcap
        self.stop, self.want = stop, want
        self.next_id = [0] * self.B
        self.qlen = [0] * NM
        self.steps, self.step = [], []
        self.n_new = 0

    def submit(self, batches, keep=(), under_test=False):
        """every book's batch in one call; the books not in `keep` are trimmed to the room their market has left"""
        books = []
        for m in range(self.NM):
            mine = range(m * self.A, (m + 1) * self.A)
            assert all(b in keep for b in mine) or not any(b in keep for b in mine)
            room = self.qcap - self.qlen[m]
            for b in mine:
                if b not in keep:
                    trim(batches[b], room)
                    room -= events(batches[b])
            res = M.run_market([(self.ticks[b % self.A], self.next_id[b], batches[b]) for b in mine], self.qlen[m], self.qcap)
            for b, r in zip(mine, res.books):
                assert b in keep or (r.code, r.applied) == (0, len(batches[b][0])), (self.name, b)
                self.next_id[b] = r.next_id
                self.n_new += sum(1 for i in r.ids if i not in (M.NO_ID, M.UNTOUCHED))
            self.qlen[m] = res.queue_len
            books += res.books
        off, ins = join(batches)
        self.step.append(Submit(off, ins, books, under_test))
        return books

    def end_step(self):
        self.steps.append(self.step)
        self.step, self.qlen = [], [0] * self.NM

    def warm_up(self):
        piece = min(W, self.qcap // self.A)
        assert piece >= 1
        for first in range(0, W, piece):
            self.submit([news(min(piece, W - first), self.ticks[b % self.A], first) for b in range(self.B)])
            self.end_step()
        assert self.next_id == [W] * self.B

    @property
    def tested(self):
        return next(s for step in self.steps for s in step if s.under_test)


def assemble(name, ticks, NM, qcap, fail, seed, stop, want, prefill=0):
    """fail: {book: batch} of the failing market; prefill: events an earlier submit of the main step puts on the failing
    market's queue (new orders of its first book)"""
    c = Case(name, ticks, NM, qcap, stop, want)
    rng = np.random.default_rng(seed)
    A, B = c.A, c.B
    lengths = LENGTHS if A == 1 else MARKET_LENGTHS
    c.warm_up()
    if prefill:
        c.submit([news(prefill, ticks[b % A], 100) if b == min(fail) else mix(rng, 3, ticks[b % A]) if b % 2 else empty()
                  for b in range(B)])
    c.submit([fail[b] if b in fail else mix(rng, lengths[b], ticks[b % A]) for b in range(B)], keep=set(fail), under_test=True)
    c.end_step()
    c.submit([mix(rng, 10, ticks[b % A]) for b in range(B)])
    c.end_step()
    c.n_orders = c.n_new + 64
    return c


def assert_conditions(c):
    """what keeps a case from passing vacuously, on the expected side alone"""
    sub = c.tested
    for b, want in c.want.items():
        got = (sub.books[b].code, sub.books[b].applied)
        assert got == want, f"{c.name}: the model gives book {b} {got}, the case is about {want}"
    failing = [b for b, r in enumerate(sub.books) if r.code != 0]
    assert all(b in c.want for b in failing), (c.name, failing)
    assert 0 not in failing and c.B - 1 not in failing
    assert int(sub.off[FAIL]) % 64 != 0
    for step in c.steps:
        for s in step:
            if s is not sub:
                assert all(r.code == 0 for r in s.books), c.name
    if c.A > 1:
        assert events([x[int(sub.off[FAIL + 1]):int(sub.off[FAIL + 2])] for x in sub.ins]) > 0, f"{c.name}: the second asset has no event"
    if c.stop is None:
        return
    b, e = c.stop
    assert sub.books[b].code != 0 and sub.books[b].applied == e
    assert f"pass {e // 64} lane {e % 64}" in c.name, (c.name, e)
    lo, hi = int(sub.off[b]), int(sub.off[b + 1])
    action = sub.ins[0][lo:hi]
    if e >= 64:
        for what, kinds in (("new order", (1,)), ("cancellation", (2,)), ("modification", (MOD,)), ("no-op", (0, 3, 7))):
            assert any(int(a) in kinds for a in action[:e]), f"{c.name}: no {what} before the stop"
    if e != hi - lo - 1:
        assert any(M.is_event(a) for a in action[e + 1:]), f"{c.name}: no event after the stop"


# --------------------------------------------------------------------------------------------------------- single books
NS = (64, 128, 150)
STOPS = (0, 1, 63, 64, 65, 127, 128)


def positions():
    """(n, e): every stop position that exists for the batch length, and the last element"""
    return [(n, e) for n in NS for e in sorted(set(x for x in STOPS if x < n) | {n - 1})]


def _seed(*key):
    return sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) + 11


ALSO = 4  # with `also`, book 4 fails too, behind book 2: a bad price at the last of its 64 elements (pass 0 lane 63)


def _also(rng, qcap, fail, want, also):
    if also:
        fail[ALSO] = trim(mix(rng, LENGTHS[ALSO], 2), qcap)
        set_new(fail[ALSO], 63, 103)
        want[ALSO] = (M.PRICE, 63)
    return fail, want


def price_stop(n, e, also=False):
    """element e is a new order at an odd price on a book with tick 2; the queue has room for everything"""
    rng = np.random.default_rng(_seed(1, n, e))
    batch = mix(rng, n, 2)
    set_new(batch, e, 101, bid=e & 1)
    fail, want = _also(rng, AMPLE, {FAIL: batch}, {FAIL: (M.PRICE, e)}, also)
    return assemble(f"price, n {n}, pass {e // 64} lane {e % 64}", [2], 6, AMPLE, fail, _seed(2, n, e), (FAIL, e), want)


def capacity_stop(n, e, also=False):
    """element e is an event and exactly as many events stand before it as the queue has room for: the queue's capacity is
    their number, or - where there is none - an earlier submit of the step fills the queue"""
    rng = np.random.default_rng(_seed(3, n, e))
    batch = mix(rng, n, 2)
    set_event(batch, e, 2)
    if e == 1:
        set_event(batch, 0, 2)
    before = events(batch, 0, e)
    qcap, prefill = (before, 0) if before else (5, 5)
    fail, want = _also(rng, qcap, {FAIL: batch}, {FAIL: (M.CAPACITY, e)}, also)
    return assemble(f"capacity, n {n}, pass {e // 64} lane {e % 64}", [2], 6, qcap, fail, _seed(4, n, e), (FAIL, e), want,
                    prefill=prefill)


def _single(name, batch, qcap, stop, want, seed):
    return assemble(name, [2], 6, qcap, {FAIL: batch}, seed, stop, {FAIL: want})


def special(which):
    rng = np.random.default_rng(_seed(5, len(which), sum(which.encode())))
    seed = _seed(6, len(which))
    if which == "bad price at 70, queue full at 100":
        batch = mix(rng, 150, 2)
        set_new(batch, 70, 99)
        set_event(batch, 100, 2)
        room = events(batch, 0, 100)  # (were element 70 well-formed, element 100 would be the first that does not fit)
        return _single(f"{which}: pass 1 lane 6", batch, room, (FAIL, 70), (M.PRICE, 70), seed)
    if which == "queue full at 70, bad price at 100":
        batch = mix(rng, 150, 2)
        set_event(batch, 70, 2)
        set_new(batch, 100, 99)
        return _single(f"{which}: pass 1 lane 6", batch, events(batch, 0, 70), (FAIL, 70), (M.CAPACITY, 70), seed)
    if which == "bad price at 20, queue full at 100":
        batch = mix(rng, 150, 2)
        set_new(batch, 20, 99)
        set_event(batch, 100, 2)
        return _single(f"{which}: pass 0 lane 20", batch, events(batch, 0, 100), (FAIL, 20), (M.PRICE, 20), seed)
    if which in ("exact fill", "exact fill, then no-ops", "exact fill, then a cancellation"):
        batch = mix(np.random.default_rng(_seed(5, 128)), 128, 2)  # (the same 128 elements in all three)
        set_event(batch, 127, 2)
        room = events(batch)
        if which == "exact fill":
            return _single(which, batch, room, None, (M.OK, 128), seed)
        if which == "exact fill, then no-ops":
            return _single(which, concat(batch, noops(rng, 22)), room, None, (M.OK, 150), seed)
        tail = mix(rng, 1, 2)
        tail[0][0], tail[5][0] = 2, 3
        return _single(f"{which}: pass 2 lane 0", concat(batch, tail), room, (FAIL, 128), (M.CAPACITY, 128), seed)
    assert which == "no-ops after the queue filled", which
    batch = mix(rng, 150, 2)
    set_event(batch, 60, 2)
    for i in range(61, 70):
        set_noop(batch, i)
    set_event(batch, 70, 2)
    return _single(f"{which}: pass 1 lane 6", batch, events(batch, 0, 61), (FAIL, 70), (M.CAPACITY, 70), seed)


SPECIALS = ("bad price at 70, queue full at 100", "queue full at 70, bad price at 100", "bad price at 20, queue full at 100",
            "exact fill", "exact fill, then no-ops", "exact fill, then a cancellation", "no-ops after the queue filled")


# --------------------------------------------------------------------------------------------------------- markets
def market(which):
    """4 markets of 2 assets; market 1 = books 2 and 3 fails"""
    rng = np.random.default_rng(_seed(7, len(which)))
    seed = _seed(8, len(which))
    if which == "asset 0 fills the queue at 64":
        ticks = [1, 2]
        a0 = mix(rng, 150, 1)
        set_event(a0, 64, 1)
        a1 = concat(noops(rng, 3), mix(rng, 40, 2))
        set_event(a1, 3, 2)
        return assemble(f"{which}: pass 1 lane 0", ticks, 4, events(a0, 0, 64), {2: a0, 3: a1}, seed, (2, 64),
                        {2: (M.CAPACITY, 64), 3: (M.CAPACITY, 3)})
    if which == "asset 0 stops at a bad price at 65, asset 1 at 64":
        # Asset 0's tick must be able to refuse a price: ticks [2, 4].  100 + 2 is a price asset 0 accepts and asset 1 does not.
        ticks = [2, 4]
        a0 = mix(rng, 150, 2)
        a0[4][:65] += (2 * (np.arange(65) % 2)).astype(np.uint32)  # (prices tick 2 accepts and tick 4 would not)
        set_new(a0, 65, 101)
        a1 = mix(rng, 150, 4)
        set_new(a1, 64, 102)
        return assemble(f"{which}: pass 1 lane 1", ticks, 4, AMPLE, {2: a0, 3: a1}, seed, (2, 65), {2: (M.PRICE, 65), 3: (M.PRICE, 64)})
    assert which == "asset 0 whole at odd prices, asset 1 stops at one at 64", which
    ticks = [1, 2]
    a0 = mix(rng, 70, 1)
    a0[4][:] |= 1  # every price odd: tick 1 accepts them
    a1 = mix(rng, 150, 2)
    set_new(a1, 64, 101)
    return assemble(f"{which}: pass 1 lane 0", ticks, 4, AMPLE, {2: a0, 3: a1}, seed, (3, 64), {2: (M.OK, 70), 3: (M.PRICE, 64)})


MARKETS = ("asset 0 fills the queue at 64", "asset 0 stops at a bad price at 65, asset 1 at 64",
           "asset 0 whole at odd prices, asset 1 stops at one at 64")

# the entry sweep: each stop kind at a lane-0 and at a lane-63 edge of a later pass, through every other entry
ENTRY_CASES = [(kind, 150, e) for kind in ("price", "capacity") for e in (64, 127)]
ENTRIES = ("async", "all", "check_status")


def stop_case(kind, n, e, also=False):
    return price_stop(n, e, also) if kind == "price" else capacity_stop(n, e, also)


def every_case():
    for n, e in positions():
        yield price_stop(n, e)
        yield capacity_stop(n, e)
    for w in SPECIALS:
        yield special(w)
    for w in MARKETS:
        yield market(w)


# --------------------------------------------------------------------------------------------------------- quotes
# 40 traders at depth 2: G = 4, a grid of 160 positions, three passes.  After the warm-up every trader of every book rests a
# bid of 10 at 96 (id 2 t) and an ask of 10 at 104 (id 2 t + 1).  Book 1 of 3 stops at grid position `pos`.
NT, DEPTH, G, QB, QTICK = 40, 2, 4, 3, 2
KEEP = 0xFFFFFFFF
QUOTE_STOPS = [("price", 63, 0, 63), ("price", 66, 1, 2), ("price", 127, 1, 63), ("price", 130, 2, 2),
               ("capacity", 64, 1, 0), ("capacity", 127, 1, 63)]  # (kind, position, pass, lane)
QuoteCase = namedtuple("QuoteCase", "entries warm quotes grid qcap want code after")


def quote_rows(rng, upto):
    """quotes of traders 0 .. upto - 1: per side the price moves (a cancellation and a new order), the volume shrinks (a
    modification), grows (a new order) or the side is kept"""
    q = np.full((NT, 4), [0, KEEP, 0, KEEP], dtype=np.uint32)
    for t in range(upto):
        for k, (rest, moved) in enumerate(((96, 94), (104, 106))):
            what = rng.choice(4, p=[0.55, 0.15, 0.15, 0.15])
            q[t, 2 * k:2 * k + 2] = [(moved, 5), (rest, 4), (rest, 15), (0, KEEP)][what]
    return q


def quote_case(expand, kind, pos):
    """`expand`: quotes_model.expand.  The failing call: book 1's traders in front of the stop quote a seeded mix, the stopping
    trader moves both sides - to an odd price on the stopping side, or onto a queue whose capacity is the number of events in
    front of the stop -, three more traders quote behind it; the neighbours' traders quote as book 1's in front of the stop."""
    trader, at = divmod(pos, G)
    rng = np.random.default_rng(17 + pos)
    row = quote_rows(rng, trader)
    row[trader:trader + 4] = (94, 5, 106, 5)
    if kind == "price":
        row[trader, 0 if at == DEPTH else 2] += 1
    quotes = np.stack([row] * QB)
    quotes[[0, 2], trader:] = (0, KEEP, 0, KEEP)
    entries = [[(2 * t, 96, 10, 1), (2 * t + 1, 104, 10, 0)] for t in range(NT)]
    grid = expand(entries, row.tolist(), DEPTH)
    qcap = events(grid, 0, pos) if kind == "capacity" else NT * G
    want = M.run_market([(QTICK, 2 * NT, grid)], 0, qcap).books[0]
    none = np.full((QB, NT, 4), [0, KEEP, 0, KEEP], dtype=np.uint32)
    warm, piece = [], min(NT, qcap // 2)
    for first in range(0, NT, piece):
        q = none.copy()
        q[:, first:first + piece] = (96, 10, 104, 10)
        warm.append(q)
    after = none.copy()
    after[:, :4] = (92, 7, 108, 7)
    return QuoteCase(entries, warm, quotes, grid, qcap, want, M.PRICE if kind == "price" else M.CAPACITY, after)


def assert_quote_conditions(expand, c, kind, pos, pass_, lane):
    assert (c.want.code, c.want.applied) == (c.code, pos) and divmod(c.want.applied, 64) == (pass_, lane)
    at, act = pos % G, int(c.grid[0][pos])
    # the failing position's slot: an entry slot's cancellation for the full queue at 64, else a new order's slot
    assert (act, at < DEPTH) == ((2, True) if (kind, pos) == ("capacity", 64) else (1, False)), (act, at)
    for what, a in (("new order", 1), ("cancellation", 2), ("modification", MOD), ("empty position", 0)):
        assert (c.grid[0][:pos] == a).any(), f"no {what} before the stop"
    assert events(c.grid, pos + 1) > 0, "no event after the stop"
    for b in (0, 2):
        assert M.run_market([(QTICK, 2 * NT, expand(c.entries, c.quotes[b].tolist(), DEPTH))], 0, c.qcap).books[0].code == 0
    assert 16 <= c.qcap <= 8192, c.qcap  # (the further call's sixteen events fit)
