"""The CPU oracle's Noise / Momentum agents against tests/agents_model.py, a model that shares no code with it.

The oracle's sampling chain (oracle/bourse_oracle_agents.cpp over oracle/pm_math.hpp and the ziggurat tables) is the same
text as the kernels', so the GPU suite's bit parity with the oracle shows that the two keep one control flow and rounding
order - not that either is right.  Here the oracle is held, exactly, to a plain-Python restatement of the reference's Rust
and of rand / rand_xoshiro / rand_distr with libm's exp / log / tanh:

* sampling: every standard normal bit for bit (a zero_case value within 4 ulp: pm::log is within 3 ulp of libm, plus one
  division), every generator state, every rounded log-normal price, the clamps at 0 and 2^32 - 1;
* the agents, fed mode: oracle.StepEnv + oracle.AgentSet beside the model's AgentSet, which is given the oracle book's
  statuses and touch before every update - every generator state, created order and member list, through the step's
  shuffle, with trading on.

EXACTNESS.  Equality is exact, with no excluded samples.  libm against pm_math can move a price only when the offset lies
within a few ulp of a tick boundary, about 1e-12 per order.  Should a seed ever hit one, the failure message prints the
offset recomputed with mpmath at 50 digits and its distance to the boundary: a boundary case is answered with another seed
and a comment, never with a tolerance.
"""
import struct

import numpy as np
import pytest

import agents_model as M
from ingress_support import (SEED, STEP, WIDE_STEPS, BusyCounts, apply_oracle, thin_flow, wide_flow, wide_set,
                             wide_trading)
from members_ingress_cases import MOM, NOISE, member_set


def _ordered(x):
    """the double's position in the ordering of all doubles"""
    (i,) = struct.unpack("<q", struct.pack("<d", x))
    return i if i >= 0 else -(i & 0x7FFFFFFFFFFFFFFF)


# ------------------------------------------------------------------------------------------------------- 1. sampling
def test_the_generator_of_the_model_is_the_published_one():
    r = M.Rng(state=(1, 2))  # rand_xoshiro 0.6.0's reference vector for Xoroshiro128StarStar
    assert [r.next_u64() for _ in range(4)] == [5760, 97769243520, 9706862127477703552, 9223447511460779954]
    assert M.Rng(seed=101).state() == (0xD1024A5FAD64D717, 0x0466A7D0954B76A3)


def test_uniform_draws_equal_the_model(oracle):
    a, m = oracle.Rng(seed=77), M.Rng(seed=77)
    for _ in range(500):
        assert float(a.gen_f32()) == m.gen_f32()
        assert a.gen_f64() == m.gen_f64()
        assert a.gen_range(10, 75) == m.gen_range(10, 75)
    assert tuple(int(x) for x in a.st) == m.state()


def test_standard_normal_equals_the_model_bit_for_bit(oracle):
    seeds, draws = 20_000, 40
    worst = zero_cases = wedge_tests = 0
    for seed in range(seeds):
        a, m = oracle.Rng(seed=seed), M.Rng(seed=seed)
        for k in range(draws):
            before = m.zero_cases
            got, want = a.std_normal(), m.std_normal()
            if got != want:
                ulp = abs(_ordered(got) - _ordered(want))
                assert m.zero_cases > before and ulp <= 4, (seed, k, got, want, ulp)
                worst = max(worst, ulp)
        assert tuple(int(x) for x in a.st) == m.state(), seed
        zero_cases, wedge_tests = zero_cases + m.zero_cases, wedge_tests + m.wedge_tests
    print(f"std_normal: {seeds * draws} draws, {zero_cases} zero_case entries (worst {worst} ulp), {wedge_tests} wedge tests")
    assert zero_cases >= 100 and wedge_tests >= 5000, (zero_cases, wedge_tests)


@pytest.mark.parametrize("mu,sigma,tick", [(8.0, 1.0, 1), (0.0, 10.0, 2), (9.0, 1.5, 5)])
def test_lognormal_prices_equal_the_model(oracle, mu, sigma, tick):
    up, down = oracle.lib().orc_round_price_up, oracle.lib().orc_round_price_down
    n = 0
    for mid in (2147483647.5, 1000.5):
        for seed in range(4000):
            a, m = oracle.Rng(seed=10_000 + seed), M.Rng(seed=10_000 + seed)
            for _ in range(5):
                d_a, d_m = abs(a.lognormal(mu, sigma)), abs(m.lognormal(mu, sigma))
                draw = (mid, mu, sigma, m.last_z, float(tick))
                got, want = int(down(mid - d_a, float(tick))), M.round_price_down(mid - d_m, float(tick))
                assert got == want, (seed, got, want, M.explain_price(draw, M.BID))
                got, want = int(up(mid + d_a, float(tick))), M.round_price_up(mid + d_m, float(tick))
                assert got == want, (seed, got, want, M.explain_price(draw, M.ASK))
                assert want % tick == 0 or want == M.MAX_PRICE
                n += 2
            assert tuple(int(x) for x in a.st) == m.state(), seed
    print(f"lognormal({mu}, {sigma}), tick {tick}: {n} prices equal")


def test_price_clamps_equal_the_model(oracle):
    up, down = oracle.lib().orc_round_price_up, oracle.lib().orc_round_price_down
    for tick in (1, 2, 4, 5):
        a, m = oracle.Rng(seed=3), M.Rng(seed=3)
        d_a, d_m = a.lognormal(25.0, 0.0), m.lognormal(25.0, 0.0)  # e^25 = 7.2e10, beyond every price
        for mid in (2147483647.5, 1000.5):
            assert int(down(mid - d_a, float(tick))) == M.round_price_down(mid - d_m, float(tick)) == 0
            assert int(up(mid + d_a, float(tick))) == M.round_price_up(mid + d_m, float(tick)) == M.MAX_PRICE
    # the clamp leaves the tick grid wherever the tick does not divide 2^32 - 1 = 3 * 5 * 17 * 257 * 65537: ticks 2 and 4
    # (tick 5 divides it)
    assert [M.MAX_PRICE % t != 0 for t in (1, 2, 4, 5)] == [False, True, True, False]
    for p, t in ((float("inf"), 2.0), (-float("inf"), 2.0), (float("nan"), 1.0), (-0.5, 1.0), (4294967294.5, 1.0), (7.0, 2.0)):
        assert int(down(p, t)) == M.round_price_down(p, t), (p, t)
        assert int(up(p, t)) == M.round_price_up(p, t), (p, t)
    assert M.round_price_up(7.0, 2.0) == 8 and M.round_price_down(7.0, 2.0) == 6


# ------------------------------------------------------------------------------------------------ 2. agents, fed mode
class FedRun:
    """B oracle StepEnvs with one oracle AgentSet each beside the model's AgentSet and generator per book."""

    def __init__(self, oracle, members_of, B, tick):
        self.B, self.tick = B, tick
        self.refs = [oracle.StepEnv(SEED + b, 0, tick, STEP) for b in range(B)]
        self.sets = [oracle.AgentSet(members_of(b)) for b in range(B)]
        self.rngs = [M.Rng(seed=SEED + b) for b in range(B)]
        self.models = [M.AgentSet(members_of(b)) for b in range(B)]
        self.busy = BusyCounts(members_of(0))
        self.queued = [0] * B
        self.steps = self.orders = self.off_grid = 0
        self.p_market = self.p_limit = 0.0

    def _same_rng(self, b, when):
        got, want = tuple(int(x) for x in self.refs[b].rng_state()), self.rngs[b].state()
        assert got == want, f"book {b}, step {self.steps}, {when}: oracle rng {got} vs model {want}"

    def update(self):
        for b in range(self.B):
            ref, aset, model = self.refs[b], self.sets[b], self.models[b]
            self._same_rng(b, "before the update")
            before = ref.book.orders_array()
            status, n0 = before["status"], len(before)
            bid, ask = ref.book.bid_ask()
            view = M.BookView(lambda i: int(status[i]), bid, ask, n0, self.tick)
            lists0 = {j: aset.order_list(j) for j in self.busy.kinds}
            aset.update(ref)
            model.update(view, self.rngs[b])
            # every order created (id, side, price, vol, trader id), the queue's length, every member's list
            created = ref.book.orders_array()[n0:]
            new = [e for e in view.events if e[0] == "new"]
            assert len(created) == len(new), f"book {b}, step {self.steps}: {len(created)} orders created vs {len(new)}"
            for o, e in zip(created, new):
                got = (int(o["order_id"]), int(o["side"]), int(o["price"]), int(o["vol"]), int(o["trader_id"]))
                want = (e[1], e[2], e[5], e[3], e[4])
                assert got == want, (f"book {b}, step {self.steps}: order (id, side, price, vol, trader) {got} vs {want}",
                                     M.explain_price(view.draws[e[1]], e[2]) if e[1] in view.draws else "a market order")
            self.queued[b] += len(view.events)
            assert ref.n_transactions() == self.queued[b], (b, self.steps, ref.n_transactions(), self.queued[b])
            for j in range(len(aset.members)):
                got = [int(i) for i in _member_ids(ref, aset, j)]
                assert got == model.order_list(j), f"book {b}, step {self.steps}, member {j}: {got} vs {model.order_list(j)}"
            self._same_rng(b, "after the update")
            self.busy.note(b, aset.members, status, n0, lists0, {j: aset.order_list(j) for j in self.busy.kinds}, created,
                           view.mid_price())
            self.orders, self.off_grid = self.orders + len(new), self.off_grid + view.off_grid
            for g in model.members:
                if isinstance(g, M.MomentumAgent):
                    self.p_market, self.p_limit = max(self.p_market, g.p_market), max(self.p_limit, g.p_limit)

    def submit(self, off, ins):
        for b, r in enumerate(self.refs):
            apply_oracle(r, int(off[b]), int(off[b + 1]), ins)
            self.queued[b] += int(off[b + 1] - off[b])

    def trading(self, on):
        for r in self.refs:
            r.enable_trading() if on else r.disable_trading()

    def step(self):
        for b, r in enumerate(self.refs):
            r.step()
            self.rngs[b].shuffle(list(range(self.queued[b])))  # Env::step's shuffle of the queue (env.rs:121)
            self.queued[b] = 0
            self._same_rng(b, "after the step's shuffle")
        self.steps += 1

    def assert_busy(self, momentum_signs=True):
        self.busy.assert_busy(momentum_signs)
        trades = sum(r.book.n_trades() for r in self.refs)
        assert trades > self.B * self.steps, (trades, self.B * self.steps)


def _member_ids(ref, aset, j):
    if aset.members[j][0] != "random":
        return aset.order_list(j)
    import ctypes as C
    import pyoracle

    out = np.zeros(aset.members[j][1], dtype=np.uint64)
    pyoracle.lib().orc_agents_held_ids(aset._a, j, out.ctypes.data_as(C.POINTER(C.c_uint64)))
    return out


@pytest.mark.parametrize("which", ["noise", "momentum", "mixed", "mixed_reversed"])
@pytest.mark.parametrize("R", [1, 4])
def test_the_sets_of_the_ingress_cases_equal_the_model(oracle, R, which):
    B, T = 8, 30
    members = member_set(R, which)
    run = FedRun(oracle, lambda b: members, B, 1)
    rng = np.random.default_rng(100 + R)
    for _ in range(T):
        run.update()
        if which == "momentum":  # alone on a book whose mid price stands still it never starts
            run.submit(*thin_flow(rng, B, 4, 1))
        run.step()
    print(f"R = {R}, {which}: {run.orders} orders, busy counts {run.busy.count}")
    run.assert_busy()


@pytest.mark.parametrize("order_ratio", [0.5, 3.0])
@pytest.mark.parametrize("decay", [0.3, 1.0])
@pytest.mark.parametrize("tick", [1, 2, 5])
def test_a_parameter_sweep_equals_the_model(oracle, tick, decay, order_ratio):
    """ticks 1, 2 and 5 (the book's and the agents'), a momentum that remembers (decay 0.3) and one that does not, p_limit
    below and above p_market, and a demand under which p_market passes 1: every trader of the member then trades"""
    B, T = 8, 30
    members = [("noise", 0, 12, dict(NOISE, tick_size=tick, p_limit=0.4, p_cancel=0.2, price_dist_sigma=1.5,
                                     price_dist_mu=float(np.log(tick)))),
               ("momentum", 100, 10, dict(MOM, tick_size=tick, demand=40.0, decay=decay, order_ratio=order_ratio,
                                          scale=0.5 / tick, p_cancel=0.2, price_dist_mu=float(np.log(2 * tick)),
                                          price_dist_sigma=1.0))]
    run = FedRun(oracle, lambda b: members, B, tick)
    rng = np.random.default_rng(7 * tick)
    for _ in range(T):
        run.update()
        run.submit(*thin_flow(rng, B, 3, tick))
        run.step()
    print(f"tick {tick}, decay {decay}, order_ratio {order_ratio}: {run.orders} orders, largest p_market {run.p_market:.3f}, "
          f"p_limit {run.p_limit:.3f}, busy counts {run.busy.count}")
    run.assert_busy()
    assert run.p_market >= 1.0 and (order_ratio < 1.0 or run.p_limit > 1.0), (run.p_market, run.p_limit)
    assert run.off_grid == 0


@pytest.mark.parametrize("pool", [256, 512])
@pytest.mark.parametrize("which", ["noise", "momentum"])
def test_members_wider_than_a_wave_equal_the_model(oracle, which, pool):
    """the sets tests/test_gpu_members_with_ingress.py and tests/test_gpu_agents_model.py give ingress::k_update_members
    (the pool only picks the script of the external flow here)"""
    B = 6
    members = wide_set(which)
    run = FedRun(oracle, lambda b: members, B, 1)
    for s in range(WIDE_STEPS):
        run.trading(wide_trading(which, s))
        run.update()
        run.submit(*wide_flow(which, pool, s, B, lambda b: run.sets[b].order_list(0)))
        run.step()
    live = max(int((r.book.orders_array()["status"] == 1).sum()) for r in run.refs)
    print(f"{which}, pool {pool}: longest list of Active ids {run.busy.longest_list}, largest New batch {run.busy.largest_batch}, "
          f"{live} live orders at the end, busy counts {run.busy.count}")
    run.assert_busy()
    assert run.busy.longest_list > 128 and run.busy.largest_batch == 2 * members[0][2], (run.busy.longest_list, run.busy.largest_batch)
    if which == "momentum":
        assert run.p_market >= 1.0 and run.p_limit >= 1.0


def test_an_off_grid_limit_price_creates_nothing(oracle):
    """every sell limit lands on the 2^32 - 1 clamp, which the book's tick 2 does not divide: no order, no id, no list entry
    (the project's choice where the reference panics), and both sides go on equal"""
    far = [("noise", 0, 16, dict(NOISE, p_limit=1.0, price_dist_mu=25.0, price_dist_sigma=0.0))]
    run = FedRun(oracle, lambda b: far, 4, 2)
    for _ in range(6):
        run.update()
        run.step()
    assert run.off_grid > 0 and run.orders > 0
    for r in run.refs:
        o = r.book.orders_array()
        assert not ((o["side"] == 0) & (o["price"] != 0)).any()


def test_a_draw_equal_to_p_cancel_cancels(oracle):
    """common.rs:68 keeps an order when `gen::<f32>() > p_cancel`: on equality it goes.  No f32 draw (a multiple of 2^-24)
    can equal the suites' p_cancel values, so this case is built: the second update's first draw is for the list's first
    id, and nothing before it depends on p_cancel (the first update's list is empty) - that draw is read off a first run
    and made the p_cancel of a second."""
    def run_two(p_cancel):
        run = FedRun(oracle, lambda b: [("noise", 0, 8, dict(NOISE, p_limit=1.0, p_market=0.0, p_cancel=p_cancel))], 1, 1)
        run.trading(False)
        run.update()
        run.step()
        first = int(run.sets[0].order_list(0)[0])
        draw = M.Rng(state=run.rngs[0].state()).gen_f32()
        run.update()
        return draw, first not in run.models[0].order_list(0)

    draw, _ = run_two(0.5)
    assert 0.0 < draw < 1.0 and M.f32(draw) == draw
    assert run_two(draw) == (draw, True)                         # equal: cancelled
    assert run_two(draw - 2.0 ** -24) == (draw, False)           # the draw is larger: kept
