"""Where k_ingest (book_device.hpp) and its copy in quotes::k_submit (quotes_ingress.hpp) stop a book's batch, beyond the
first 64 elements: a bad price or a full queue at lane 0, 1 or 63 of the second and third pass, both in one pass, a queue
that fills exactly at a pass boundary, no-ops behind a full queue, a second asset on the queue its sibling's stop left.

The expected side is tests/ingress_cut_model.py - one element at a time, pinned by tests/test_ingress_cut_model.py -, and it
alone decides every value: each book's status pair, its ids with `out_ids` untouched from the stop on, its id counter, and
the applied prefix that the book's oracle is fed.  tests/ingress_cut_cases.py makes the runs and their conditions, asserted
here before the device is touched.  After the step every book equals its oracle (ingress_support.check: level-2 history,
trades, live orders in priority order, order log, keys), and so it does after one further well-formed step."""
import numpy as np
import pytest

import ingress_cut_cases as CC
import ingress_cut_model as M
import oracle_parity as P
import quotes_cases as QC
import quotes_model as QM
from ingress_support import SEED, STEP, apply_oracle, check, dev, ingress_env, submit
from market_ingress_support import apply_market, check_markets, many_markets, market_env

pytestmark = pytest.mark.gpu
FRESH_ID, FRESH_STATUS = 0x7777777777, 77  # what out_ids / status hold before the call: no id, not u64::MAX, no code


@pytest.fixture(scope="module")
def bk():
    import bourse_amd

    return bourse_amd


# --------------------------------------------------------------------------------------------- instructions: the entries
def _message(code, book, applied):
    if code == M.PRICE:
        return ValueError, rf"book {book}: a price of its batch .*\(element {applied} of"
    return None, rf"book {book}: .* after {applied} elements"


def call_entry(bk, torch, env, sub, entry):
    """the submit under test through `entry`: what the entry reports against the model's books"""
    want_status = [[r.code, r.applied] for r in sub.books]
    flat = sum((r.ids for r in sub.books), [])
    failing = [b for b, r in enumerate(sub.books) if r.code != 0]
    exc, msg = (None, None)
    if failing:
        exc, msg = _message(sub.books[failing[0]].code, failing[0], sub.books[failing[0]].applied)
        exc = exc or bk.CapacityError
    if entry in ("device", "check_status"):
        ids = torch.full((len(flat),), FRESH_ID, dtype=torch.int64, device="cuda")
        status = torch.full((len(sub.books), 2), FRESH_STATUS, dtype=torch.int32, device="cuda")
        args = [dev(torch, sub.off)] + [dev(torch, x) for x in sub.ins]
        if entry == "check_status" and failing:
            with pytest.raises(exc, match=msg):
                env.submit_instructions_device(*args, out_ids=ids, status=status, check_status=True)
        else:
            env.submit_instructions_device(*args, out_ids=ids, status=status, check_status=entry == "check_status")
        got_status, got_ids, untouched = status.cpu().numpy().tolist(), ids.cpu().numpy().view(np.uint64), FRESH_ID
    elif entry == "async":
        ticket = env.submit_instructions_all_async(sub.off.astype(np.uint64), sub.ins)
        got_ids, got_status, bad = env.submit_result(ticket)
        assert bad == (failing[0] if failing else None), f"the lowest failing book: {bad} vs {failing}"
        got_status, untouched = got_status.tolist(), M.NO_ID  # (this entry's ids start as u64::MAX)
    else:
        assert entry == "all", entry
        if failing:  # it raises for the lowest failing book; what the books hold is compared after the step
            with pytest.raises(exc, match=msg):
                env.submit_instructions_all(sub.off.astype(np.uint64), sub.ins)
            return
        got_ids, got_status, untouched = env.submit_instructions_all(sub.off.astype(np.uint64), sub.ins), want_status, M.NO_ID
    assert got_status == want_status, f"status {got_status} vs {want_status}"
    P.same_array(got_ids, M.ids_array(flat, untouched), entry, "out_ids")


def run_case(bk, torch, oracle, case, entry="device"):
    CC.assert_conditions(case)
    A, T = case.A, len(case.steps)
    if A == 1:
        env = ingress_env(bk, torch, case.B, T, CC.POOL, 0, case.qcap, tick=case.ticks[0], n_orders=case.n_orders)
        refs = [oracle.StepEnv(SEED + b, 0, case.ticks[0], STEP) for b in range(case.B)]
    else:
        env = market_env(bk, torch, case.NM, case.ticks, T, CC.POOL, case.qcap, case.n_orders)
        ref = many_markets(oracle, case.NM, case.ticks)
    for s, step in enumerate(case.steps):
        for sub in step:
            if sub.under_test:
                call_entry(bk, torch, env, sub, entry)
            else:
                submit(torch, env, sub.off, sub.ins)
            for b, r in enumerate(sub.books):  # the oracle takes each book's applied prefix, a market's assets in turn
                if A == 1:
                    apply_oracle(refs[b], 0, r.applied, r.prefix)
                else:
                    apply_market(ref, b // A, b % A, 0, r.applied, r.prefix)
        counters = [r.next_id for r in step[-1].books]
        env.step(sync=False)
        if A == 1:
            for r in refs:
                r.step()
            assert [r.book.n_orders() for r in refs] == counters
        else:
            ref.step()
        if s >= T - 2:  # after the step under test, and after the further well-formed one
            env.sync()
            assert [env.order_count(b) for b in range(case.B)] == counters, f"{case.name}: id counters after step {s}"
            if A == 1:
                check(env, refs)
            else:
                check_markets(env, lambda m: (ref, m))
    P.no_flags(env)
    env.close()


@pytest.mark.parametrize("n,e", CC.positions(), ids=lambda v: str(v))
@pytest.mark.parametrize("kind", ["price", "capacity"])
def test_a_stop_at_every_edge_of_every_pass(bk, oracle, kind, n, e):
    """Book 2 of 6 stops at element e of its n: a bad price with room to spare, or the first event the queue has no room
    for - the queue's capacity is the number of events before it (at element 0 an earlier submit of the step filled it)."""
    import torch

    run_case(bk, torch, oracle, CC.stop_case(kind, n, e))


@pytest.mark.parametrize("which", CC.SPECIALS)
def test_both_stops_in_one_pass_exact_fills_and_noops_behind_a_full_queue(bk, oracle, which):
    import torch

    run_case(bk, torch, oracle, CC.special(which))


@pytest.mark.parametrize("which", CC.MARKETS)
def test_a_markets_second_asset_starts_on_the_queue_its_sibling_left(bk, oracle, which):
    """The issue's second market case names ticks [1, 2] and a bad price on asset 0, which tick 1 cannot refuse: that case
    runs on ticks [2, 4] - asset 0's prices are ones its tick accepts and asset 1's would not -, and a third case keeps
    ticks [1, 2] with asset 0 whole at odd prices and asset 1 stopped by one."""
    import torch

    run_case(bk, torch, oracle, CC.market(which))


@pytest.mark.parametrize("entry", CC.ENTRIES)
@pytest.mark.parametrize("kind,n,e", CC.ENTRY_CASES, ids=lambda v: str(v))
def test_every_entry_reports_the_stop(bk, oracle, kind, n, e, entry):
    """lane 0 of pass 1 and lane 63 of pass 1, both kinds, through submit_instructions_all_async + submit_result,
    submit_instructions_all and check_status=True (submit_instructions_device itself: the sweep above).  Book 4 fails too,
    at a bad price in its last element: the entries name book 2, the lowest."""
    import torch

    case = CC.stop_case(kind, n, e, also=True)
    assert [b for b, r in enumerate(case.tested.books) if r.code] == [CC.FAIL, CC.ALSO]
    run_case(bk, torch, oracle, case, entry)


# --------------------------------------------------------------------------------------------- quotes: k_submit's copy
@pytest.mark.parametrize("kind,pos,pass_,lane", CC.QUOTE_STOPS, ids=lambda v: str(v))
def test_quotes_stop_where_the_instruction_entry_stops(bk, oracle, kind, pos, pass_, lane):
    """40 traders at depth 2: a grid of 160 positions, three passes (ingress_cut_cases.quote_case).  After the warm-up
    every trader rests both sides; then book 1 of 3 stops at grid position `pos` - an off-tick new bid or ask, or the first
    event the queue has no room for (an entry slot's cancellation at 64, a new ask at 127) - through failing_step against
    the twin env, which takes the model's grid through k_ingest; then one further well-formed call."""
    import torch

    c = CC.quote_case(QM.expand, kind, pos)
    CC.assert_quote_conditions(QM.expand, c, kind, pos, pass_, lane)
    NT, depth, G, B = CC.NT, CC.DEPTH, CC.G, CC.QB
    plan = QC.QuotePlan(oracle, B, CC.QTICK, NT, depth)
    envs = []
    for _ in range(2):
        e = ingress_env(bk, torch, B, len(c.warm) + 2, CC.POOL, 0, c.qcap, tick=CC.QTICK, n_orders=4 * NT * G)
        e.enable_open_orders(NT, depth)
        envs.append(e)
    env, twin = envs

    def whole_step(q):
        plan.step(q)
        s = len(plan.steps) - 1
        ids, status = QC.outputs(torch, plan)
        env.submit_quotes(QC.quotes_dev(torch, q), ids, status, check_status=True)
        env.step(sync=False)
        P.same_array(ids.cpu().numpy().view(np.uint64), plan.steps[s][3], f"step {s}", "out_ids")
        twin_ids, twin_status = QC.twin_step(torch, twin, plan, s)
        P.same_array(twin_ids, plan.steps[s][3], f"step {s}", "the twin's out_ids")
        assert twin_status.tolist() == [[0, NT * G]] * B

    for q in c.warm:
        whole_step(q)
    assert plan.entries() == [c.entries] * B, "the warm-up left other entries than the case was made for"
    assert [r.book.n_orders() for r in plan.refs] == [2 * NT] * B
    raises = (ValueError, "book 1: a quoted price") if kind == "price" else (bk.CapacityError, "book 1")
    QC.failing_step(torch, env, twin, plan, c.quotes, (1, pos), c.code, raises)
    new_ids = np.array(c.want.ids, dtype=object).reshape(NT, G)[:, depth:].reshape(-1).tolist()
    P.same_array(plan.steps[-1][3][1].reshape(-1), M.ids_array(new_ids, QC.UNTOUCHED), "book 1", "failing_step's ids against the model's")
    for e in (env, twin):
        check(e, plan.refs)
        assert [e.order_count(b) for b in range(B)] == [r.book.n_orders() for r in plan.refs]
        assert e.order_count(1) == c.want.next_id
    whole_step(c.after)
    for e in (env, twin):
        check(e, plan.refs)
        P.no_flags(e)
        e.close()

