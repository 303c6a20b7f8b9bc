"""The on-device Noise / Momentum agents against tests/agents_model.py - a plain-Python model of the reference's agents and of
rand / rand_xoshiro / rand_distr over libm that shares no code with the kernels.  pyoracle is not imported here: every
other GPU test of this agent family compares a kernel with the CPU oracle, whose sampling chain is the kernels' own text.

a. ingress::k_update_members, fed mode: before every update the model is given the device book's order statuses and its
   touch (the best Active bid and ask of env.orders(b)); after it the book's generator, the orders it appended and every
   member's list must be the model's, and after the step the generator again (the model shuffles the queue it counted).
b. bk_run's pipelines (k_run_mixed, k_agents_mixed_lanes, k_agents_mixed, k_agents_mixed_wave), resting mode: trading is
   off, so the model's own record of placed-minus-cancelled orders is the book - live orders in priority order, the
   generator and the level-2 touch and side volumes of every step.
c. members wider than a wave on the ingress path (tests/ingress_support.py::wide_set), fed mode as in a.

Equality is exact throughout (see tests/test_agents_model.py, EXACTNESS: a failure message carries the offset at 50 digits)."""
import numpy as np
import pytest

import agents_model as M
from ingress_support import (SEED, STEP, WIDE_STEPS, BusyCounts, ingress_env, members_env, submit, thin_flow, wide_flow,
                             wide_set, wide_trading)
from members_ingress_cases import MOM, NOISE, member_set

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bk():
    import bourse_amd

    return bourse_amd


# ------------------------------------------------------------------------------------------- a, c. the ingress path, fed
class FedRun:
    """a device env with device ingress beside one model AgentSet and generator per book"""

    def __init__(self, env, torch, members_of, tick):
        self.env, self.torch, self.B, self.tick = env, torch, env.n_books, tick
        self.members = [members_of(b) for b in range(self.B)]
        self.rngs = [M.Rng(seed=SEED + b) for b in range(self.B)]
        self.models = [M.AgentSet(m) for m in self.members]
        self.busy = BusyCounts(self.members[0])
        self.queued = [0] * self.B
        self.steps = self.orders = self.off_grid = self.max_live = 0

    def _same_rng(self, b, when):
        got, want = self.env.rng_state(b), self.rngs[b].state()
        assert got == want, f"book {b}, step {self.steps}, {when}: device rng {got} vs model {want}"

    def update(self):
        env = self.env
        env.sync()
        before = [env.orders(b) for b in range(self.B)]
        env.update_members()
        for b in range(self.B):
            model, o = self.models[b], before[b]
            status, n0 = o["status"], len(o)
            act = o[status == 1]
            bids, asks = act["price"][act["side"] == 1], act["price"][act["side"] == 0]
            self.max_live = max(self.max_live, len(act))
            view = M.BookView(lambda i: int(status[i]), int(bids.max()) if len(bids) else 0,
                              int(asks.min()) if len(asks) else M.MAX_PRICE, n0, self.tick)
            lists0 = {j: model.order_list(j) for j in self.busy.kinds}
            model.update(view, self.rngs[b])
            self._same_rng(b, "after the update")
            created = env.orders(b)[n0:]
            new = [e for e in view.events if e[0] == "new"]
            assert len(created) == len(new), f"book {b}, step {self.steps}: {len(created)} orders appended vs {len(new)}"
            for o1, e in zip(created, new):
                got = tuple(int(o1[k]) for k in ("order_id", "side", "price", "vol", "trader_id", "arr_time", "status"))
                want = (e[1], e[2], e[5], e[3], e[4], self.steps * STEP, M.NEW)
                assert got == want, (f"book {b}, step {self.steps}: order (id, side, price, vol, trader, arrival, status) "
                                     f"{got} vs {want}", M.explain_price(view.draws[e[1]], e[2]) if e[1] in view.draws else "")
            for j in range(len(model.members)):
                got = [int(i) for i in env.member_orders(b, j)]
                assert got == model.order_list(j), f"book {b}, step {self.steps}, member {j}: {got} vs {model.order_list(j)}"
            self.busy.note(b, self.members[b], status, n0, lists0, {j: model.order_list(j) for j in self.busy.kinds},
                           {k: created[k] for k in ("trader_id", "side", "price")}, view.mid_price())
            self.queued[b] += len(view.events)
            self.orders, self.off_grid = self.orders + len(new), self.off_grid + view.off_grid

    def submit(self, off, ins):
        submit(self.torch, self.env, off, ins)
        for b in range(self.B):
            self.queued[b] += int(off[b + 1] - off[b])

    def step(self):
        self.env.step()
        for b in range(self.B):
            self.rngs[b].shuffle(list(range(self.queued[b])))  # Env::step's shuffle of the queue (env.rs:121)
            self.queued[b] = 0
            self._same_rng(b, "after the step's shuffle")
        self.steps += 1


def _table_row(b):
    r = np.random.default_rng(500 + b)
    return [("noise", 100 * (b % 5), 12, dict(NOISE, p_limit=float(np.float32(r.uniform(0.2, 0.6))), p_cancel=0.2,
                                              price_dist_mu=float(r.uniform(-0.5, 1.0)), price_dist_sigma=float(r.uniform(0.5, 2.0)))),
            ("momentum", 2000 + b, 8, dict(MOM, demand=float(r.uniform(4.0, 30.0)), decay=float(r.uniform(0.3, 1.0)),
                                           price_dist_mu=float(r.uniform(0.0, 1.0)), price_dist_sigma=float(r.uniform(1.0, 8.0))))]


@pytest.mark.parametrize("which,pool,tick", [(w, p, t) for w in ("noise", "momentum", "mixed") for p in (64, 256) for t in (1, 2)]
                         + [("table", 256, 1)])
def test_update_members_equals_the_model(bk, which, pool, tick):
    import torch

    B, T = 33, 10
    members_of = _table_row if which == "table" else (lambda b, m=member_set(pool // 64, which): m)
    env = members_env(bk, torch, B, T, pool, members_of(0), tick, n_ext=4)
    env.set_agents_per_book([members_of(b) for b in range(B)]) if which == "table" else env.set_agents(members_of(0))
    run = FedRun(env, torch, members_of, tick)
    rng = np.random.default_rng(40 + pool + tick)
    for _ in range(T):
        run.update()
        run.submit(*thin_flow(rng, B, 3, tick))
        run.step()
        assert not env.flags().any(), (run.steps, env.flags())
    print(f"{which}, pool {pool}, tick {tick}: {run.orders} orders, at most {run.max_live} live, busy counts {run.busy.count}")
    run.busy.assert_busy(momentum_signs=which != "mixed")
    env.close()


def test_update_members_off_the_tick_grid_equals_the_model(bk):
    """every sell limit lands on the 2^32 - 1 clamp, which the book's tick 2 does not divide: PRICE_TICK is flagged and
    nothing is created - no order, no id, no list entry - and the book stays the model's"""
    import torch

    B, T = 33, 5
    far = [("noise", 0, 16, dict(NOISE, p_limit=1.0, price_dist_mu=25.0, price_dist_sigma=0.0))]
    env = ingress_env(bk, torch, B, T, 128, 0, 64, strict=False, n_orders=64 * T)
    env.set_agents(far)
    run = FedRun(env, torch, lambda b: far, 2)
    for _ in range(T):
        run.update()
        run.step()
    flags = env.flags()
    assert (flags & bk._lib.FLAG_PRICE_TICK).all() and not (flags & ~np.uint32(bk._lib.FLAG_PRICE_TICK)).any(), flags
    assert run.off_grid > 0 and run.orders > 0
    for b in range(B):
        o = env.orders(b)
        assert not ((o["side"] == 0) & (o["price"] != 0)).any(), b  # no sell limit order exists
    env.close()


@pytest.mark.parametrize("pool", [256, 512])
@pytest.mark.parametrize("which", ["noise", "momentum"])
def test_members_wider_than_a_wave_equal_the_model(bk, which, pool):
    import torch

    B, T = 33, WIDE_STEPS
    members = wide_set(which)
    env = members_env(bk, torch, B, T, pool, members, 1, n_ext=4)
    env.set_agents(members)
    run = FedRun(env, torch, lambda b: members, 1)
    for s in range(T):
        env.enable_trading() if wide_trading(which, s) else env.disable_trading()
        run.update()
        run.submit(*wide_flow(which, pool, s, B, lambda b: run.models[b].order_list(0)))
        run.step()
        assert not env.flags().any(), (s, env.flags())
    print(f"{which}, pool {pool}: longest list of Active ids {run.busy.longest_list}, largest New batch {run.busy.largest_batch}, "
          f"at most {run.max_live} live, busy counts {run.busy.count}")
    run.busy.assert_busy()
    assert run.busy.longest_list > 128 and run.busy.largest_batch == 2 * members[0][2], (run.busy.longest_list, run.busy.largest_batch)
    assert run.max_live < pool, run.max_live
    env.close()


# --------------------------------------------------------------------------------------- b. bk_run's pipelines, resting
REST_BOOKS, REST_SEED, REST_STEP, REST_POOL = 67, 101, 1_000_000, 512
# (offsets of e^3 = 20 and more: few orders near the empty book's mid price, so the touch - the Noise orders alone move it, with
# trading off - shifts from step to step and the momentum takes both signs)
REST_MEMBERS = [("noise", 0, 70, dict(NOISE, p_limit=0.8, p_cancel=0.3, price_dist_mu=3.0, price_dist_sigma=1.5)),
                ("momentum", 100, 20, dict(MOM, demand=40.0, decay=0.5, p_cancel=0.3, price_dist_sigma=2.0))]


def _rest_row(b):
    r = np.random.default_rng(900 + b)
    return [("noise", 0, 70, dict(NOISE, p_limit=float(np.float32(r.uniform(0.7, 0.95))), p_cancel=0.3,
                                  price_dist_mu=float(r.uniform(2.0, 4.0)), price_dist_sigma=float(r.uniform(0.5, 2.0)))),
            ("momentum", 100, 20, dict(MOM, demand=float(r.uniform(20.0, 60.0)), decay=float(r.uniform(0.3, 1.0)), p_cancel=0.3,
                                       price_dist_mu=float(r.uniform(0.0, 1.0)), price_dist_sigma=float(r.uniform(1.0, 4.0))))]


def _resting_model(members_of, n_steps):
    """the expected side, computed once per member table: one RestingBook per book"""
    books = []
    for b in range(REST_BOOKS):
        book, agents = M.RestingBook(REST_SEED + b, 0, 1, REST_STEP), M.AgentSet(members_of(b))
        book.m_pos = book.mom_market = book.noise_market = 0
        for _ in range(n_steps):
            view = book.update(agents)
            book.m_pos += agents.members[1].momentum > 0.0
            for e in view.events:
                if e[0] == "new" and e[5] == (M.MAX_PRICE if e[2] == M.BID else 0):
                    if e[4] >= 100:
                        book.mom_market += 1
                    else:
                        book.noise_market += 1
            book.step()
        books.append(book)
    return books


@pytest.fixture(scope="module")
def resting():
    cache = {}

    def get(table):
        if table not in cache:
            cache[table] = _resting_model(_rest_row if table else (lambda b: REST_MEMBERS), 6)
        return cache[table]

    return get


@pytest.mark.parametrize("pipeline,table", [("fused", False), ("split", False), ("split_wave", False), ("wave_split", False),
                                            ("auto", True)])
def test_run_pipelines_with_trading_off_equal_the_model(bk, resting, pipeline, table):
    books = resting(table)
    # the condition on the model, before any comparison
    peak = max(k.peak_live for k in books)
    assert 128 < peak < REST_POOL, peak
    assert sum(k.m_pos for k in books) > 0 and sum(k.mom_market for k in books) > 0 and sum(k.noise_market for k in books) > 0
    assert all(k.rejected == k.mom_market + k.noise_market for k in books)
    print(f"{pipeline}: peak resting count {peak}, {sum(k.noise_market for k in books)} Noise and "
          f"{sum(k.mom_market for k in books)} Momentum market orders Rejected, momentum > 0 in {sum(k.m_pos for k in books)} updates")

    env = bk.ManyBookEnv(REST_BOOKS, REST_SEED, 0, 1, REST_STEP, True, levels=10, max_live_orders=REST_POOL, trade_capacity=64,
                         history_capacity=6)
    env.set_agents_per_book([_rest_row(b) for b in range(REST_BOOKS)]) if table else env.set_agents(REST_MEMBERS)
    env.disable_trading()
    env.set_pipeline(pipeline)
    env.run(2)
    env.run(4)
    flags = env.flags()
    assert not flags.any(), flags  # every bit, FLAG_DECODE_LOOKAHEAD (256, the wave decode's look-ahead) among them
    assert int(env.trade_counts().sum()) == 0
    hist = env.history()
    for b, book in enumerate(books):
        assert env.rng_state(b) == book.rng.state(), f"book {b}: rng {env.rng_state(b)} vs {book.rng.state()}"
        live = env.live_orders(b)
        for side in (M.BID, M.ASK):
            mine = live[live["side"] == side]
            got = list(zip(mine["order_id"].tolist(), mine["price"].tolist(), mine["vol"].tolist()))
            want = book.live(side)
            assert got == want, (f"book {b}, side {side}: live (id, price, vol) differ first at "
                                 f"{next((k for k, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))}",
                                 len(got), len(want))
        got = [tuple(int(x) for x in hist[s, b, 1:5]) for s in range(6)]
        assert got == book.history, f"book {b}: (bid, ask, ask vol, bid vol) per step {got} vs {book.history}"
    env.close()
