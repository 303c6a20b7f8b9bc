"""tests/ingress_cut_model.py pinned: it gives the values the suite already asserts by hand, its bad-price rule is the oracle's
StepEnvNumpy.submit_instructions, its capacity rule - which the reference has no counterpart of - is written out case by
case here, and every run of tests/test_gpu_ingress_cuts.py meets the conditions that keep it from passing vacuously."""
import numpy as np
import pytest

import ingress_cut_cases as CC
import ingress_cut_model as M
import oracle_parity as P
import quotes_cases as QC
import quotes_model as QM
from ingress_support import SEED, STEP

U = M.UNTOUCHED
NO = M.NO_ID


def batch_of(rows):
    """rows of (action, side, vol, trader, price, order_id)"""
    return [np.array([r[k] for r in rows], dtype=dt) for k, dt in enumerate(M.DTYPES)]


def new(price, bid=1):
    return (1, bid, 5, 0, price, 0)


CANCEL, MODIFY, NOTHING, THREE, SEVEN = (2, 0, 0, 0, 0, 0), (M.MODIFY, 4, 3, 0, 0, 0), (0, 0, 0, 0, 0, 0), (3, 1, 1, 1, 1, 1), (7, 1, 1, 1, 7, 1)


def one(rows, tick=1, next_id=0, queue_len=0, queue_cap=1000):
    res = M.run_market([(tick, next_id, batch_of(rows))], queue_len, queue_cap)
    return res.books[0], res


# ------------------------------------------------------------------------------- what the suite asserts by hand already
def test_the_fifteen_element_call_of_the_device_ingress_test():
    """test_gpu_device_ingress.py::test_device_ingress_capacity_unknown_ids_and_argument_checks: four books, queue capacity 6"""
    n = 15
    off = [0, 4, 12, 12, 15]
    action = np.ones(n, dtype=np.uint32)
    action[13] = 2
    side = (np.arange(n) % 2).astype(np.uint8)
    ins = (action, side, np.full(n, 2), np.arange(n), np.where(side == 1, 99, 101), np.where(np.arange(n) == 13, 40, 0))
    books = [M.run_market([(1, 0, [x[off[b]:off[b + 1]] for x in ins])], 0, 6).books[0] for b in range(4)]
    assert [[b.code, b.applied] for b in books] == [[0, 4], [3, 6], [0, 0], [0, 3]]
    ids = sum((b.ids for b in books), [])
    assert ids == [0, 1, 2, 3] + [0, 1, 2, 3, 4, 5, U, U] + [0, NO, 1]
    assert [b.next_id for b in books] == [4, 6, 0, 2]
    assert M.ids_array(ids, NO)[10:12].tolist() == [NO, NO]  # (that test's out_ids start as u64::MAX)


def test_the_two_quote_failures_of_the_quotes_test(oracle):
    """test_gpu_quotes.py: the off-tick bid of trader 2 of book 1, and the queue of five events under eight"""
    B, NT, depth, tick = 3, 4, 2, 2
    G = depth + 2
    plan = QC.QuotePlan(oracle, B, tick, NT, depth)
    q0 = np.zeros((B, NT, 4), dtype=np.uint32)
    q0[:] = (96, 10, 104, 10)
    plan.step(q0)
    q1 = np.zeros((B, NT, 4), dtype=np.uint32)
    q1[:] = (94, 5, 106, 5)
    q1[1, 2, 0] = 95
    for b, entries in enumerate(plan.entries()):
        grid = QM.expand(entries, q1[b].tolist(), depth)
        r = M.run_market([(tick, plan.refs[b].book.n_orders(), grid)], 0, NT * G).books[0]
        assert (r.code, r.applied) == ((1, 2 * (depth + 2) + depth) if b == 1 else (0, NT * G)), b
        new_ids = np.array(r.ids, dtype=object).reshape(NT, G)[:, depth:].tolist()
        assert new_ids == ([[8, 9], [10, 11], [U, U], [U, U]] if b == 1 else [[8 + 2 * t, 9 + 2 * t] for t in range(NT)])
    B = 2
    none = [[QM.NO_ORDER, 0, 0, 0]] * depth
    q = np.full((B, NT, 4), [0, QM.KEEP, 0, QM.KEEP], dtype=np.uint32)
    q[0, :2] = (96, 10, 104, 10)
    q[1, :] = (96, 10, 104, 10)
    got = [M.run_market([(tick, 0, QM.expand([none] * NT, q[b].tolist(), depth))], 0, 5).books[0] for b in range(B)]
    assert [(r.code, r.applied) for r in got] == [(0, 16), (3, 11)]
    assert np.array(got[1].ids, dtype=object).reshape(NT, G)[:, depth:].tolist() == [[0, 1], [2, 3], [4, U], [U, U]]
    assert np.array(got[0].ids, dtype=object).reshape(NT, G)[:, depth:].tolist() == [[0, 1], [2, 3], [NO, NO], [NO, NO]]


# ------------------------------------------------------------------------------- the bad-price rule is the reference's
def test_the_bad_price_rule_is_the_oracles_submit_instructions(oracle):
    """Batches of 1 to 200 elements with one bad price planted at a random new order: StepEnvNumpy.submit_instructions raises,
    and its book then holds what a second env holds that was given the model's applied prefix - before and after the step."""
    rng = np.random.default_rng(61)
    tick, stops = 2, set()
    for n in range(1, 201):
        batch = CC.mix(rng, n, tick)
        batch[0][batch[0] == M.MODIFY] = 3  # (the reference's numpy entry has no modification: model and oracle both skip a 3)
        at = {150: 0, 151: 1, 152: 63, 153: 64, 154: 65, 155: 127, 156: 128}.get(n, int(rng.integers(0, n)))
        CC.set_new(batch, at, 2 * int(rng.integers(45, 56)) + 1, bid=at & 1)
        r = M.run_market([(tick, CC.W, batch)], 0, 10**9).books[0]
        assert (r.code, r.applied) == (M.PRICE, at) and r.ids[at:] == [U] * (n - at)
        stops.add(at)
        envs = [oracle.StepEnvNumpy(SEED + n, 0, tick, STEP) for _ in range(2)]
        for e in envs:
            e.submit_instructions(CC.news(CC.W, tick))
            e.step()
        with pytest.raises(ValueError):
            envs[0].submit_instructions(batch)
        ids = envs[1].submit_instructions(r.prefix)
        assert ids.tolist() == r.ids[:at], n
        assert envs[1].book.n_orders() == r.next_id
        for stage in ("queued", "stepped"):
            P.same_records(envs[0].book.orders_array(), envs[1].book.orders_array(), (n, stage), "order")
            P.same_records(envs[0].book.trades_array(), envs[1].book.trades_array(), (n, stage), "trade")
            for e in envs:
                e.step()
        P.same_array(envs[0].history(), envs[1].history(), n, "L2 history")
    assert {0, 1, 63, 64, 65, 127, 128} <= stops, sorted(stops)


# ------------------------------------------------------------------------------- the capacity rule, by hand
def test_the_capacity_rule_by_hand():
    # room for two events: the third does not fit, whatever it is
    for third in (new(100), CANCEL, MODIFY):
        r, m = one([new(100), CANCEL, third, new(100)], queue_cap=2)
        assert (r.code, r.applied, r.ids, m.events, m.queue_len) == (3, 2, [0, NO, U, U], [(0, 0), (0, 1)], 2)
    # what is no event never stops a book and takes no room
    r, m = one([NOTHING, THREE, SEVEN, new(100)], queue_cap=1)
    assert (r.code, r.applied, r.ids, m.events) == (0, 4, [NO, NO, NO, 0], [(0, 3)])
    # an exact fill is no failure ...
    r, m = one([new(100), MODIFY, CANCEL], queue_cap=3)
    assert (r.code, r.applied, m.queue_len) == (0, 3, 3)
    # ... nor are no-ops behind it: they count as applied, up to the first event that does not fit
    r, m = one([new(100), MODIFY, CANCEL, NOTHING, SEVEN], queue_cap=3)
    assert (r.code, r.applied, r.ids) == (0, 5, [0, NO, NO, NO, NO])
    r, m = one([new(100), MODIFY, CANCEL, NOTHING, SEVEN, CANCEL, NOTHING], queue_cap=3)
    assert (r.code, r.applied, r.ids, m.queue_len) == (3, 5, [0, NO, NO, NO, NO, U, U], 3)
    # the queue's length at the call counts: a full queue refuses the first event, after the no-ops in front of it
    r, m = one([THREE, NOTHING, new(100)], queue_len=4, queue_cap=4)
    assert (r.code, r.applied, r.ids, r.next_id, m.events) == (3, 2, [NO, NO, U], 0, [])
    r, m = one([new(100)], queue_len=4, queue_cap=4)
    assert (r.code, r.applied, r.ids) == (3, 0, [U])
    # a bad price is looked at first: on a full queue it is still the bad price that is reported
    r, m = one([new(101)], tick=2, queue_len=4, queue_cap=4)
    assert (r.code, r.applied) == (1, 0)
    # the earlier failure is the one reported
    r, m = one([new(100), new(101), new(100)], tick=2, queue_cap=2)
    assert (r.code, r.applied) == (1, 1)
    r, m = one([new(100), new(100), new(101)], tick=2, queue_cap=1)
    assert (r.code, r.applied) == (3, 1)
    # ids go on from the book's counter
    r, m = one([CANCEL, new(100), new(100)], next_id=41)
    assert (r.ids, r.next_id) == ([NO, 41, 42], 43)
    # an empty batch
    r, m = one([], queue_cap=1)
    assert (r.code, r.applied, r.ids) == (0, 0, [])


def test_a_markets_assets_share_one_queue_in_asset_order():
    # asset 0 leaves the queue full: asset 1's no-ops are applied, its first event is not, nothing of it is queued
    m = M.run_market([(1, 0, batch_of([new(7), new(9), new(11)])), (2, 5, batch_of([NOTHING, SEVEN, new(8), CANCEL]))], 1, 3)
    assert [(b.code, b.applied) for b in m.books] == [(3, 2), (3, 2)]
    assert m.events == [(0, 0), (0, 1)] and m.queue_len == 3 and m.books[1].ids == [NO, NO, U, U] and m.books[1].next_id == 5
    # asset 0 stops at a bad price with room left: asset 1's batch follows its prefix; ticks are per asset, ids per book
    m = M.run_market([(2, 3, batch_of([new(8), new(7), new(8)])), (1, 0, batch_of([new(7), CANCEL]))], 0, 8)
    assert [(b.code, b.applied, b.ids) for b in m.books] == [(1, 1, [3, U, U]), (0, 2, [0, NO])]
    assert m.events == [(0, 0), (1, 0), (1, 1)] and m.queue_len == 3
    # ... and part-full: asset 1 gets what is left
    m = M.run_market([(2, 0, batch_of([new(8), new(7)])), (1, 0, batch_of([new(7), CANCEL, MODIFY]))], 0, 3)
    assert [(b.code, b.applied) for b in m.books] == [(1, 1), (3, 2)]
    assert [len(x) for x in m.books[1].prefix] == [2] * 6 and m.books[1].prefix[4].tolist() == [7, 0]


# ------------------------------------------------------------------------------- the GPU module's runs
def test_every_run_of_the_gpu_module_meets_its_conditions():
    names = set()
    for case in CC.every_case():
        CC.assert_conditions(case)
        assert case.name not in names
        names.add(case.name)
        sub = case.tested
        assert len(sub.books) == case.B and case.n_orders <= 4096
    assert len(names) == 2 * len(CC.positions()) + len(CC.SPECIALS) + len(CC.MARKETS)
    # both kinds at each of the eight stop positions of a three-pass batch, and at a pass's last lane in every batch length
    assert [e for n, e in CC.positions() if n == 150] == [0, 1, 63, 64, 65, 127, 128, 149]
    assert {(64, 63), (128, 127), (128, 64)} <= set(CC.positions())
    for kind, n, e in CC.ENTRY_CASES:
        case = CC.stop_case(kind, n, e, also=True)
        CC.assert_conditions(case)
        assert [(b, r.code, r.applied) for b, r in enumerate(case.tested.books) if r.code] == \
            [(CC.FAIL, M.PRICE if kind == "price" else M.CAPACITY, e), (CC.ALSO, M.PRICE, 63)]
    assert {e % 64 for _, _, e in CC.ENTRY_CASES} == {0, 63}


@pytest.mark.parametrize("kind,pos,pass_,lane", CC.QUOTE_STOPS, ids=lambda v: str(v))
def test_every_quote_run_of_the_gpu_module_meets_its_conditions(oracle, kind, pos, pass_, lane):
    c = CC.quote_case(QM.expand, kind, pos)
    CC.assert_quote_conditions(QM.expand, c, kind, pos, pass_, lane)
    plan = QC.QuotePlan(oracle, CC.QB, CC.QTICK, CC.NT, CC.DEPTH)
    for q in c.warm:  # the warm-up leaves the oracle's books with the entries the case was made for
        assert max(int((g != 0).sum()) for g in np.split(plan.step(q)[2][1][0], CC.QB)) <= c.qcap
    assert plan.entries() == [c.entries] * CC.QB and [r.book.n_orders() for r in plan.refs] == [2 * CC.NT] * CC.QB
    for a, b in zip(QM.expand(plan.entries()[1], c.quotes[1].tolist(), CC.DEPTH), c.grid):
        assert np.array_equal(a, b)
