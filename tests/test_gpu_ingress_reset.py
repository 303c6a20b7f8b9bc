"""Per-book reset of a DEVICE-INGRESS env to a device-resident snapshot (bk_ingress_snapshot_save / bk_ingress_reset_books*
through ManyBookEnv.save_ingress_snapshot / reset_ingress_books and ManyMarketEnv.reset_ingress_markets), bit for bit
against the CPU oracle.

The oracle cannot be cloned or reseeded, so the expected side is a REPLAY.  `Sim` drives the device env and one
oracle.StepEnv(SEED + b) (+ agent set) per book with the same calls, and records every call per book: trading flag,
update, submitted instructions, step.  The schedule is n steps, save, m steps, reset, k steps.  A book that was never reset
is its oracle after all n + m + k steps; a reset book is a FRESH oracle env and agent set given the first n steps' calls
again, and then the last k steps' calls.  The instructions after a reset are drawn against the expected side's ids, so the
ids a reset hands out again are really targeted.  Compared per book: the level-2 history (the last k rows of a reset
book), trades (of a reset book: the oracle's from the snapshot's count on, and trade_count = (total, that count)), live
orders in priority order, the whole order log with one order_status and the keys, the RNG state and the clock - through
tests/ingress_support.py::check for the books that were never reset and the same tests/oracle_parity.py calls for the others.

The device has no reader for the held ids of bk_update_agents (the RandomAgents groups' case): they are observed through
the orders the agents cancel and place in the k steps after the reset - a wrong held id changes the next update's
cancellations, which the order log and the RNG state then show.  bk_update_members' lists are read (env.member_orders)."""
import ctypes as C

import numpy as np
import pytest

import oracle_parity as P
from ingress_support import MOD, SEED, STEP, BusyCounts, apply_oracle, check, ingress_env, members_env, submit
from members_ingress_cases import NOISE, member_set

pytestmark = pytest.mark.gpu
U64_MAX = 0xFFFFFFFFFFFFFFFF
MASKS = ("none", "all", "first", "last", "alternate")


@pytest.fixture(scope="module")
def bk():
    import bourse_amd

    return bourse_amd


def make_mask(name, B):
    m = np.zeros(B, dtype=bool)
    if name == "all":
        m[:] = True
    elif name == "first":
        m[0] = True
    elif name == "last":
        m[B - 1] = True
    elif name == "alternate":
        m[::2] = True
    elif name == "third":
        m[1::3] = True
    return m


def as_kind(torch, mask, kind, seeds=None):
    """The mask (and seeds) as the host arrays they are, or as torch CUDA tensors written on the current stream."""
    if kind == "host":
        return mask, seeds
    return (torch.tensor(mask, device="cuda"),
            None if seeds is None else torch.tensor(np.asarray(seeds, dtype=np.uint64).view(np.int64), device="cuda"))


def slice_ins(ins, lo, hi):
    return tuple(x[lo:hi].copy() for x in ins)


class Sim:
    """The device env and its expected side: one oracle StepEnv per book, with `sets(b)` -> (kind, agent set) if agents
    run on the device ("random": oracle.RandomAgentSet via update_agents, "members": oracle.AgentSet via update_members)."""

    def __init__(self, oracle, torch, env, B, tick, kind=None, agents_of=None, seed=SEED):
        self.oracle, self.torch, self.env, self.B, self.tick, self.kind, self.agents_of = oracle, torch, env, B, tick, kind, agents_of
        self.seeds = [seed + b for b in range(B)]
        self.refs = [oracle.StepEnv(s, 0, tick, STEP) for s in self.seeds]
        self.sets = [self._new_set(b) for b in range(B)]
        self.log = [[] for _ in range(B)]      # the calls of each book's current line
        self.saved = {}                        # slot -> what the expected side was at the save
        self.snap_trades = [-1] * B            # the trade count of the snapshot a book was last reset to (-1: never)
        self.since_reset = [None] * B          # steps since the book's last reset
        self.steps = 0
        self.busy = BusyCounts(self.sets[0].members) if kind == "members" else None

    def _new_set(self, b):
        if self.kind == "random":
            return self.oracle.RandomAgentSet(self.agents_of(b))
        if self.kind == "members":
            return self.oracle.AgentSet(self.agents_of(b))
        return None

    # ---- one call on one book of the expected side
    def _apply(self, b, ref, aset, op, note=True):
        if op[0] == "trading":
            ref.enable_trading() if op[1] else ref.disable_trading()
        elif op[0] == "update":
            if self.kind == "members" and note:
                traded = [j for j, m in enumerate(aset.members) if m[0] != "random"]
                before = ref.book.orders_array()
                lists0 = {j: aset.order_list(j) for j in traded}
                mid = ref.book.mid_price()
                aset.update(ref)
                self.busy.note(b, aset.members, before["status"], len(before), lists0, {j: aset.order_list(j) for j in traded},
                               ref.book.orders_array()[len(before):], mid)
            else:
                aset.update(ref)
        elif op[0] == "ins":
            apply_oracle(ref, 0, len(op[1][0]), op[1])
        else:
            ref.step()

    def _all(self, op_of):
        for b in range(self.B):
            op = op_of(b)
            self._apply(b, self.refs[b], self.sets[b], op)
            self.log[b].append(op)

    # ---- the calls
    def trading(self, on):
        self.env.enable_trading() if on else self.env.disable_trading()
        self._all(lambda b: ("trading", on))

    def update(self):
        self.env.update_agents(sync=False) if self.kind == "random" else self.env.update_members(sync=False)
        self._all(lambda b: ("update",))

    def submit(self, off, ins):
        submit(self.torch, self.env, off, ins)
        self._all(lambda b: ("ins", slice_ins(ins, int(off[b]), int(off[b + 1]))))

    def step(self):
        self.env.step(sync=False)
        self._all(lambda b: ("step",))
        self.steps += 1
        self.since_reset = [None if s is None else s + 1 for s in self.since_reset]

    def save(self, slot=0):
        self.env.save_ingress_snapshot(slot)
        self.saved[slot] = dict(log=[list(l) for l in self.log], trades=[r.book.n_trades() for r in self.refs],
                                orders=[r.book.n_orders() for r in self.refs], seeds=list(self.seeds),
                                mom=dict(self.busy.mom) if self.busy else None)

    def reset(self, mask, kind="host", seeds=None, slot=0):
        m, s = as_kind(self.torch, mask, kind, seeds)
        self.env.reset_ingress_books(m, seeds=s, slot=slot, sync=(kind == "host"))
        snap = self.saved[slot]
        for b in np.flatnonzero(mask):
            self.seeds[b] = int(seeds[b]) if seeds is not None else snap["seeds"][b]
            # (a reseeded book replays the snapshot's calls too: the tests reseed where the snapshot's calls drew nothing)
            ref, aset = self.oracle.StepEnv(self.seeds[b], 0, self.tick, STEP), self._new_set(b)
            for op in snap["log"][b]:
                self._apply(b, ref, aset, op, note=False)
            self.refs[b], self.sets[b], self.log[b] = ref, aset, list(snap["log"][b])
            self.snap_trades[b], self.since_reset[b] = snap["trades"][b], 0
            if self.busy:
                for key in [k for k in self.busy.mom if k[0] == b]:
                    del self.busy.mom[key]
                self.busy.mom.update({k: v for k, v in snap["mom"].items() if k[0] == b})

    # ---- the comparison
    def member_ids(self, b, j):
        aset = self.sets[b]
        m = aset.members[j]
        if m[0] != "random":
            return aset.order_list(j)
        out = np.zeros(m[1], dtype=np.uint64)
        self.oracle.lib().orc_agents_held_ids(aset._a, j, out.ctypes.data_as(C.POINTER(C.c_uint64)))
        return out

    def check_members(self):
        for b in range(self.B):
            for j in range(len(self.sets[b].members)):
                got, want = self.env.member_orders(b, j), self.member_ids(b, j)
                assert np.array_equal(got, want), (b, j, got, want)

    def check(self, allow_flags=0):
        env = self.env
        env.sync()
        P.no_flags(env, allow=allow_flags)
        kept = [b for b in range(self.B) if self.snap_trades[b] < 0]
        check(env, self.refs, kept)
        hist = env.history()
        assert len(hist) == self.steps
        for b in range(self.B):
            ref, view = self.refs[b], self.refs[b].book
            assert env.time(b) == view.get_time(), (b, env.time(b), view.get_time())
            if b in kept:
                assert env.trade_count(b) == (view.n_trades(), 0), b
                continue
            tag, k = (b, "reset"), self.since_reset[b]
            if k:
                P.same_history(hist[len(hist) - k:, b], ref.history()[-k:], f"{tag}: L2 history tail")
            assert env.trade_count(b) == (view.n_trades(), self.snap_trades[b]), (tag, env.trade_count(b))
            P.same_records(env.trades(b), view.trades_array()[self.snap_trades[b]:], tag, "retained trade")
            P.same_live(env, b, view, tag)
            P.same_orders(env, b, view, tag)
            P.same_keys(env, b, view, tag)
            got, want = env.rng_state(b), tuple(int(x) for x in ref.rng_state())
            assert got == want, f"{tag}: rng state {got} vs {want}"
        if self.kind == "members":
            self.check_members()


def flow(rng, sim, n_b, force=None):
    """One step's instructions, n_b[b] for book b: limit and market orders, cancellations and modifications of the ids the
    expected side's book has now - half of them among the ids the agents hold, if any; force[b] = ids that get a
    cancellation or a modification each, whatever else is drawn."""
    B, tick = sim.B, sim.tick
    n0 = [r.book.n_orders() for r in sim.refs]
    forced = [[int(i) for i in (force[b] if force else []) if 0 <= i < n0[b]] for b in range(B)]
    n_b = np.asarray(n_b) + np.array([len(f) for f in forced])
    off = np.zeros(B + 1, dtype=np.int64)
    off[1:] = np.cumsum(n_b)
    n = int(off[-1])
    action = rng.choice([1, 2, MOD], size=n, p=[0.6, 0.2, 0.2]).astype(np.uint32)
    bid = rng.integers(0, 2, size=n).astype(np.uint8)
    has_p, has_v = rng.integers(0, 2, size=n).astype(np.uint8), rng.integers(0, 2, size=n).astype(np.uint8)
    vol = rng.integers(1, 40, size=n).astype(np.uint32)
    trader = rng.integers(5000, 6000, size=n).astype(np.uint32)
    price = (rng.integers(30, 68, size=n) * tick).astype(np.uint32)
    order_id = np.zeros(n, dtype=np.uint64)
    for b in range(B):
        held = np.zeros(0, dtype=np.uint64)
        if sim.kind == "random":
            held = np.concatenate([sim.sets[b].held_ids(g) for g in range(len(sim.sets[b].groups))])
        elif sim.kind == "members":
            held = np.concatenate([sim.member_ids(b, j) for j in range(len(sim.sets[b].members))])
        held = held[held < n0[b]]
        for q, i in enumerate(range(int(off[b]), int(off[b + 1]))):
            if q < len(forced[b]):
                action[i], order_id[i] = (2 if q % 2 else MOD), forced[b][q]
            elif action[i] == 1:
                continue
            elif n0[b] == 0:
                action[i] = 0  # nothing to target yet: a no-op
            elif len(held) and rng.random() < 0.5:
                order_id[i] = held[rng.integers(0, len(held))]
            else:
                order_id[i] = rng.integers(0, n0[b])
    side = np.where(action == MOD, (has_p << 1) | (has_v << 2), bid).astype(np.uint8)
    market = (action == 1) & (rng.random(n) < 0.15) & (tick == 1)
    price[market] = np.where(bid[market] == 1, 0xFFFFFFFF, 0)  # a market order: the extreme prices (tick 1)
    return off, (action, side, vol, trader, price, order_id)


# ------------------------------------------------------------------ 1. plain ingress, every mask, both kinds
@pytest.mark.parametrize("kind", ["host", "device"])
@pytest.mark.parametrize("pool", [64, 512])
def test_masked_books_rewind_their_records_and_the_others_carry_on(bk, oracle, pool, kind):
    import torch

    B, (n, m, k) = 7, (4, 3, 4)
    per_book = np.array([12, 2, 7, 1, 9, 4, 5])  # n_keep is book 0's: it exceeds every other book's own keep_b
    for mask_name in MASKS:
        mask = make_mask(mask_name, B)
        env = ingress_env(bk, torch, B, n + m + k, pool, 0, 32, tick=1, n_orders=16 * (n + m + k))
        sim = Sim(oracle, torch, env, B, 1)
        rng = np.random.default_rng(3)
        for s in range(n + m + k):
            if s == n:
                assert sim.refs[B - 1].book.n_orders() == 0 and sim.refs[0].book.n_orders() > 2 * sim.refs[1].book.n_orders()
                sim.save()
            if s == n + m:
                sim.reset(mask, kind)
            n_b = per_book.copy()
            n_b[B - 1] = 0 if s < n else 6  # the last book has no order at the save: keep_b = 0
            # after the reset: ids just below and AT the snapshot's next id (handed out again by then) are targeted
            force = [(sim.saved[0]["orders"][b] - 1, sim.saved[0]["orders"][b]) for b in range(B)] if s > n + m else None
            sim.submit(*flow(rng, sim, n_b, force))
            sim.step()
        sim.check()
        if mask.any():
            b = int(np.flatnonzero(mask)[0])
            assert sim.refs[b].book.n_orders() > sim.saved[0]["orders"][b]  # the snapshot's next id was handed out again
        env.close()


# ------------------------------------------------------------------ 2. RandomAgents via update_agents
@pytest.mark.parametrize("save_before_first_update", [False, True])
def test_random_agents_held_ids_rewind(bk, oracle, save_before_first_update):
    import torch

    B, pool, NX = 8, 64, 4
    n, m, k = (0, 5, 6) if save_before_first_update else (4, 3, 4)
    groups = [(pool // 2, (32, 64), (10, 20), 2, 0.8), (pool // 4, (30, 66), (50, 70), 2, 0.3)]
    na = sum(g[0] for g in groups)
    env = ingress_env(bk, torch, B, n + m + k, pool, na, na + NX + 2, tick=2, n_ext=NX + 2)
    env.set_random_agents(groups)
    sim = Sim(oracle, torch, env, B, 2, "random", lambda b: groups)
    rng = np.random.default_rng(17)
    mask = make_mask("alternate", B)
    for s in range(n + m + k):
        if s == n:
            sim.save()  # (n = 0: no update_agents has run - the env has not made the held ids yet)
        if s == n + m:
            sim.reset(mask, "device" if s % 2 else "host")
            for b in np.flatnonzero(mask):  # the replay's agents right after the reset
                held = np.concatenate([sim.sets[b].held_ids(g) for g in range(len(groups))])
                assert (held == U64_MAX).all() if save_before_first_update else (held != U64_MAX).any(), b
        sim.update()
        sim.submit(*flow(rng, sim, rng.integers(0, NX + 1, size=B)))
        sim.step()
    sim.check()
    assert sum(r.book.n_trades() for r in sim.refs) > B * k
    env.close()


# ------------------------------------------------------------------ 3. Noise + Momentum + RandomAgents members
@pytest.mark.parametrize("R", [1, 4])
def test_members_lists_and_momentum_rewind(bk, oracle, R):
    import torch

    B, (n, m, k), NX = 8, (6, 3, 5), 3
    members = member_set(R, "mixed")
    env = members_env(bk, torch, B, n + m + k, 64 * R, members, 1, n_ext=NX)
    env.set_agents(members)
    sim = Sim(oracle, torch, env, B, 1, "members", lambda b: members)
    rng = np.random.default_rng(29 + R)
    mask = make_mask("alternate", B)
    for s in range(n + m + k):
        if s < 2:  # the first step without trading: the RandomAgents' orders all rest
            sim.trading(s == 1)
        if s == n:
            sim.save()
        if s == n + m:
            sim.reset(mask, "device")
            sim.check_members()  # the lists right after the reset are the replay's
        sim.update()  # (the momentum state is observed through this update's orders)
        sim.submit(*flow(rng, sim, rng.integers(0, NX + 1, size=B)))
        sim.step()
    sim.busy.assert_busy()
    trades = sum(r.book.n_trades() for r in sim.refs)
    assert trades > B * sim.steps, (trades, B * sim.steps)
    sim.check()
    env.close()


def test_members_saved_before_their_first_update_start_empty_again(bk, oracle):
    import torch

    B, (m, k) = 6, (4, 4)
    members = member_set(1, "mixed")
    env = members_env(bk, torch, B, m + k, 64, members, 1)
    env.set_agents(members)
    sim = Sim(oracle, torch, env, B, 1, "members", lambda b: members)
    mask = make_mask("alternate", B)
    sim.save()  # member_lists_stale: no buffers yet
    for s in range(m + k):
        if s == m:
            assert any(len(env.member_orders(b, 1)) for b in np.flatnonzero(mask))
            sim.reset(mask)
            for b in np.flatnonzero(mask):
                assert (env.member_orders(b, 0) == U64_MAX).all() and len(env.member_orders(b, 1)) == 0 == len(env.member_orders(b, 2))
        sim.update()
        sim.step()
    sim.check()
    env.close()


# ------------------------------------------------------------------ 4. a reset with a non-empty queue
def test_a_reset_empties_the_queue(bk, oracle):
    import torch

    B, n = 8, 5
    members = member_set(1, "mixed")
    env = members_env(bk, torch, B, n + 1, 64, members, 1, n_ext=4)
    env.set_agents(members)
    sim = Sim(oracle, torch, env, B, 1, "members", lambda b: members)
    rng = np.random.default_rng(41)
    for s in range(n):
        sim.update()
        sim.submit(*flow(rng, sim, np.full(B, 3)))
        sim.step()
    sim.save()
    mask = make_mask("alternate", B)
    env.sync()
    l2_at_save, t_at_save = env.level2(), [env.time(b) for b in range(B)]
    # queued for EVERY book, then half of them are reset: what they had queued is dropped
    sim.update()
    sim.submit(*flow(rng, sim, np.full(B, 4)))
    sim.reset(mask)
    sim.step()
    sim.check()
    hist = env.history()
    for b in range(B):
        if mask[b]:  # an empty queue was stepped: the snapshot's level-2 record again, the clock one step on
            assert np.array_equal(hist[-1, b, 1:], l2_at_save[b, 1:]) and env.time(b) == t_at_save[b] + STEP, b
            assert env.order_count(b) == sim.saved[0]["orders"][b], b
        else:
            assert env.order_count(b) > sim.saved[0]["orders"][b], b
    assert sum(r.book.n_trades() for b, r in enumerate(sim.refs) if not mask[b]) > sum(sim.saved[0]["trades"][b] for b in range(B) if not mask[b])
    env.close()


# ------------------------------------------------------------------ 5. reseed
@pytest.mark.parametrize("kind", ["host", "device"])
def test_reseed_from_the_empty_book(bk, oracle, kind):
    import torch

    B, (m, k), S = 9, (5, 6), 9_000_000_019
    groups = [(32, (32, 64), (10, 20), 2, 0.8), (16, (30, 66), (50, 70), 2, 0.3)]
    env = ingress_env(bk, torch, B, m + k, 64, 48, 48, tick=2)
    env.set_random_agents(groups)
    sim = Sim(oracle, torch, env, B, 2, "random", lambda b: groups)
    mask = make_mask("third", B)
    seeds = (S + np.arange(B)).astype(np.uint64)
    sim.save()  # step 0, the empty books
    for s in range(m + k):
        if s == m:
            sim.reset(mask, kind, seeds=seeds)
        sim.update()
        sim.step()
    sim.check()  # a reseeded book is a fresh oracle env with the new seed after k steps
    env.close()


def test_reseed_on_a_non_empty_snapshot_sets_the_rng_words(bk, oracle):
    import torch

    B, S = 9, 77_000
    env = ingress_env(bk, torch, B, 8, 64, 0, 16, tick=1, n_orders=128)
    sim = Sim(oracle, torch, env, B, 1)
    rng = np.random.default_rng(5)
    for _ in range(3):
        sim.submit(*flow(rng, sim, np.full(B, 5)))
        sim.step()
    env.save_ingress_snapshot()
    orders = [env.orders(b) for b in range(B)]
    sim.submit(*flow(rng, sim, np.full(B, 5)))
    sim.step()
    env.sync()
    before = [env.rng_state(b) for b in range(B)]
    mask = make_mask("third", B)
    env.reset_ingress_books(mask, seeds=(S + np.arange(B)).astype(np.uint64))
    for b in range(B):
        want = tuple(int(x) for x in oracle.Rng(seed=S + b).st) if mask[b] else before[b]
        assert env.rng_state(b) == want, b
        if mask[b]:
            P.same_records(env.orders(b), orders[b], b, "order")
    env.close()


# ------------------------------------------------------------------ 6. order-log capacity
def new_orders(rng, B, n, tick=1):
    """n new limit orders for every book, in a band of prices where bids and asks cross"""
    N = B * n
    return np.arange(B + 1, dtype=np.int64) * n, (
        np.ones(N, np.uint32), rng.integers(0, 2, size=N).astype(np.uint8), rng.integers(1, 40, size=N).astype(np.uint32),
        rng.integers(5000, 6000, size=N).astype(np.uint32), (rng.integers(30, 68, size=N) * tick).astype(np.uint32),
        np.zeros(N, np.uint64))


def test_ids_beyond_the_order_log_capacity(bk, oracle):
    import torch

    B, CAP = 6, 16  # max_orders = 16: the books hand out 24 ids before the save (the log keeps the first 16)
    env = ingress_env(bk, torch, B, 8, 64, 0, 16, tick=1, n_orders=CAP, strict=False)
    rng = np.random.default_rng(9)
    for _ in range(3):
        submit(torch, env, *new_orders(rng, B, 8))
        env.step(sync=False)
    env.sync()
    counts = [env.order_count(b) for b in range(B)]
    assert all(c > CAP for c in counts), counts
    env.save_ingress_snapshot()
    assert env.ingress_snapshot_bytes() == B * (env.state_bytes_per_book() + 4 * env.width + CAP * 80)  # n_keep = max_orders
    status = [[env.order_status(b, i) for i in range(CAP)] for b in range(B)]
    live = [env.live_orders(b) for b in range(B)]
    submit(torch, env, *new_orders(rng, B, 8))
    env.step()
    changed = [b for b in range(B) if [env.order_status(b, i) for i in range(CAP)] != status[b]]
    mask = make_mask("alternate", B)
    assert set(changed) & set(np.flatnonzero(mask).tolist()), "the step was meant to change a logged order of a masked book"
    env.reset_ingress_books(mask)
    P.no_flags(env, allow=bk._lib.FLAG_ORDER_LOG_FULL)
    for b in range(B):
        if mask[b]:  # the records below max_orders are the snapshot's; order_count is the snapshot's next id
            assert env.order_count(b) == counts[b], b
            assert [env.order_status(b, i) for i in range(CAP)] == status[b], b
            P.same_records(env.live_orders(b), live[b], b, "live order")
        else:
            assert env.order_count(b) > counts[b], b
    env.step()
    env.close()


# ------------------------------------------------------------------ 7. markets
class MarketSim:
    """ManyMarketEnv(2 assets) with the device ingress against one oracle.ManyMarkets(1, SEED + market) per market, replayed
    for a reset market as Sim replays a book.  A step's instructions are new orders and cancellations of the book's own ids."""
    TICKS = [1, 2]

    def __init__(self, oracle, torch, env, NM, seed=SEED):
        self.oracle, self.torch, self.env, self.NM, self.A = oracle, torch, env, NM, 2
        self.seeds = [seed + mk for mk in range(NM)]
        self.refs = [self._new(s) for s in self.seeds]
        self.log = [[] for _ in range(NM)]
        self.saved, self.snap_trades, self.since_reset, self.steps = None, [None] * NM, [None] * NM, 0

    def _new(self, seed):
        return self.oracle.ManyMarkets(1, seed, 0, self.TICKS, STEP, True, 10)

    def _apply(self, ref, op):
        if op[0] == "step":
            ref.step()
            return
        for a, (action, side, vol, trader, price, order_id) in enumerate(op[1]):
            for i in range(len(action)):
                if action[i] == 1:
                    ref.place_order(0, a, bool(side[i] & 1), int(vol[i]), int(trader[i]), price=int(price[i]))
                elif action[i] == 2:
                    ref.cancel_order(0, a, int(order_id[i]))

    def submit(self, rng, n_max):
        B = self.NM * self.A
        n_b = rng.integers(1, n_max + 1, size=B)
        off = np.zeros(B + 1, dtype=np.int64)
        off[1:] = np.cumsum(n_b)
        n = int(off[-1])
        action = rng.choice([1, 2], size=n, p=[0.75, 0.25]).astype(np.uint32)
        bid = rng.integers(0, 2, size=n).astype(np.uint8)
        order_id = np.zeros(n, dtype=np.uint64)
        for b in range(B):
            n0 = self.refs[b // self.A].book(0, b % self.A).n_orders()
            for i in range(int(off[b]), int(off[b + 1])):
                if action[i] == 2:
                    if n0 == 0:
                        action[i] = 0
                    else:
                        order_id[i] = rng.integers(0, n0)
        ins = (action, bid, rng.integers(1, 40, size=n).astype(np.uint32), rng.integers(5000, 6000, size=n).astype(np.uint32),
               (rng.integers(30, 68, size=n) * 2).astype(np.uint32), order_id)
        submit(self.torch, self.env, off, ins)
        for mk in range(self.NM):
            op = ("ins", [slice_ins(ins, int(off[mk * self.A + a]), int(off[mk * self.A + a + 1])) for a in range(self.A)])
            self._apply(self.refs[mk], op)
            self.log[mk].append(op)

    def step(self):
        self.env.step(sync=False)
        for mk in range(self.NM):
            self._apply(self.refs[mk], ("step",))
            self.log[mk].append(("step",))
        self.steps += 1
        self.since_reset = [None if s is None else s + 1 for s in self.since_reset]

    def save(self):
        self.env.save_ingress_snapshot()
        self.saved = dict(log=[list(l) for l in self.log],
                          trades=[[r.book(0, a).n_trades() for a in range(self.A)] for r in self.refs])

    def reset(self, mask, kind, seeds=None):
        m, s = as_kind(self.torch, mask, kind, seeds)
        self.env.reset_ingress_markets(m, seeds=s, sync=(kind == "host"))
        for mk in np.flatnonzero(mask):
            if seeds is not None:
                self.seeds[mk] = int(seeds[mk])
            ref = self._new(self.seeds[mk])
            for op in self.saved["log"][mk]:
                self._apply(ref, op)
            self.refs[mk], self.log[mk] = ref, list(self.saved["log"][mk])
            self.snap_trades[mk], self.since_reset[mk] = self.saved["trades"][mk], 0

    def check(self):
        env = self.env
        env.sync()
        P.no_flags(env)
        hist = env.history()
        for mk in range(self.NM):
            ref = self.refs[mk]
            k = self.steps if self.since_reset[mk] is None else self.since_reset[mk]
            for a in range(self.A):
                b, view, tag = mk * self.A + a, ref.book(0, a), (mk, a, "kept" if self.snap_trades[mk] is None else "reset")
                if k:
                    P.same_history(hist[len(hist) - k:, b], ref.history()[-k:, a], f"{tag}: L2 history tail")
                assert env.rng_state(b) == tuple(int(x) for x in ref.rng_states()[0]), tag
                assert env.time(b) == view.get_time(), tag
                base = 0 if self.snap_trades[mk] is None else self.snap_trades[mk][a]
                assert env.trade_count(b) == (view.n_trades(), base), tag
                P.same_records(env.trades(b), view.trades_array()[base:], tag, "retained trade")
                P.same_live(env, b, view, tag)
                P.same_orders(env, b, view, tag)
                P.same_keys(env, b, view, tag)


@pytest.mark.parametrize("reseed", [False, True])
def test_markets_rewind_both_books_and_their_queue(bk, oracle, reseed):
    import torch

    NM, (n, m, k), S = 7, (0 if reseed else 4, 3, 4), 55_000
    env = bk.ManyMarketEnv(NM, SEED, 0, MarketSim.TICKS, STEP, levels=10, max_live_orders=64, max_orders=256, trade_capacity=512,
                           history_capacity=n + m + k, stream=torch.cuda.current_stream().cuda_stream)
    env.enable_device_ingress(32)
    sim = MarketSim(oracle, torch, env, NM)
    rng = np.random.default_rng(13)
    mask = make_mask("alternate", NM)
    for s in range(n + m + k):
        if s == n:
            sim.save()
        if s == n + m:
            sim.submit(rng, 4)  # queued for every market: a reset market's queue is emptied
            for mk in np.flatnonzero(mask):
                sim.log[mk].pop()
            sim.reset(mask, "device" if reseed else "host", seeds=(S + np.arange(NM)).astype(np.uint64) if reseed else None)
            if reseed:
                for mk in np.flatnonzero(mask):
                    want = tuple(int(x) for x in oracle.Rng(seed=S + int(mk)).st)
                    assert env.rng_state(2 * mk) == env.rng_state(2 * mk + 1) == want, mk
        else:
            sim.submit(rng, 6)
        sim.step()
    sim.check()
    assert sum(r.book(0, a).n_trades() for r in sim.refs for a in range(2)) > 0
    env.close()


# ------------------------------------------------------------------ 8. two slots, re-save and drop
def test_two_slots_resave_and_drop(bk, oracle):
    import torch

    B = 8
    env = ingress_env(bk, torch, B, 14, 64, 0, 16, tick=1, n_orders=256)
    sim = Sim(oracle, torch, env, B, 1)
    rng = np.random.default_rng(21)

    def run(steps):
        for _ in range(steps):
            sim.submit(*flow(rng, sim, np.full(B, 6)))
            sim.step()

    assert env.ingress_snapshot_bytes(0) == 0 == env.ingress_snapshot_bytes(1)
    run(2)
    sim.save(0)
    run(3)
    sim.save(1)
    state_bytes = B * (env.state_bytes_per_book() + 4 * env.width)
    keep0, keep1 = max(sim.saved[0]["orders"]), max(sim.saved[1]["orders"])
    assert keep1 > keep0
    assert env.ingress_snapshot_bytes(0) == state_bytes + B * keep0 * 80
    assert env.ingress_snapshot_bytes(1) == state_bytes + B * keep1 * 80
    run(2)
    m0, m1 = np.zeros(B, dtype=bool), np.zeros(B, dtype=bool)
    m0[:3], m1[3:6] = True, True
    sim.reset(m0, slot=0)
    sim.reset(m1, "device", slot=1)
    run(3)
    sim.check()
    # a re-save of slot 0 with more ids per book reallocates, and changes what a reset from it restores
    sim.save(0)
    assert env.ingress_snapshot_bytes(0) == state_bytes + B * max(sim.saved[0]["orders"]) * 80 > state_bytes + B * keep0 * 80
    run(2)
    m2 = np.zeros(B, dtype=bool)
    m2[[0, 4, 7]] = True
    sim.reset(m2, slot=0)
    run(2)
    sim.check()
    env.drop_ingress_snapshot(0)
    assert env.ingress_snapshot_bytes(0) == 0 and env.ingress_snapshot_bytes(1) > 0
    before = P.snapshot(env, books=[6])  # (a book that was never reset: all its trades are retained)
    with pytest.raises(bk.BourseError, match="empty"):
        env.reset_ingress_books(m2, slot=0)
    P.assert_same(before, P.snapshot(env, books=[6]))
    env.drop_ingress_snapshot(0)  # (dropping an empty slot is not an error)
    env.reset_ingress_books(m1, slot=1)  # the other slot is still there
    env.close()


# ------------------------------------------------------------------ 9. the header fix-ups
def test_a_sticky_flag_survives_the_reset(bk, oracle):
    import torch

    B = 6
    env = bk.ManyBookEnv(B, SEED, 0, 1, STEP, levels=10, max_live_orders=64, max_orders=256, trade_capacity=4, history_capacity=8,
                         strict=False, stream=torch.cuda.current_stream().cuda_stream)
    env.enable_device_ingress(32)
    env.save_ingress_snapshot()  # (of the empty books: no flag in the snapshot)
    assert not env.flags().any()
    n = 24
    cross = (np.ones(n, np.uint32), (np.arange(n) % 2).astype(np.uint8), np.full(n, 5, np.uint32), np.full(n, 7, np.uint32),
             np.full(n, 100, np.uint32), np.zeros(n, np.uint64))  # bids and asks at one price: every pair trades
    off = np.arange(B + 1, dtype=np.int64) * n
    for _ in range(2):
        submit(torch, env, off, tuple(np.tile(x, B) for x in cross))
        env.step()
    flagged = env.flags()
    assert (flagged & bk._lib.FLAG_TRADE_OVERFLOW).all(), "4 records per book were meant to overflow"
    env.reset_ingress_books(np.ones(B, dtype=bool))
    assert np.array_equal(env.flags(), flagged)
    assert all(env.order_count(b) == 0 and env.trade_count(b) == (0, 0) for b in range(B))
    env.clear_flags()
    assert not env.flags().any()
    env.close()


def test_reset_books_take_the_envs_current_trading_flag(bk, oracle):
    import torch

    B, (n, m, k) = 8, (3, 2, 3)
    env = ingress_env(bk, torch, B, n + m + k, 64, 0, 16, tick=1, n_orders=256)
    sim = Sim(oracle, torch, env, B, 1)
    rng = np.random.default_rng(33)
    mask = make_mask("alternate", B)
    for s in range(n + m + k):
        if s == n:
            sim.save()  # the snapshot's books trade
        if s == n + m:
            sim.trading(False)
            sim.reset(mask)
            for b in np.flatnonzero(mask):  # (the replay: the snapshot's calls, then trading off)
                sim._apply(b, sim.refs[b], None, ("trading", False))
                sim.log[b].append(("trading", False))
        sim.submit(*flow(rng, sim, np.full(B, 6)))
        sim.step()
    sim.check()
    for b in np.flatnonzero(mask):  # no trade after the reset
        assert env.trade_count(b)[0] == sim.saved[0]["trades"][b], b
    env.close()


def test_trade_count_after_a_reset_is_the_snapshots(bk, oracle):
    import torch

    B = 8
    env = ingress_env(bk, torch, B, 8, 64, 0, 16, tick=1, n_orders=256)
    sim = Sim(oracle, torch, env, B, 1)
    rng = np.random.default_rng(37)
    for s in range(7):
        if s == 4:
            sim.save()
            at_save = [env.trade_count(b) for b in range(B)]
            assert at_save == [(r.book.n_trades(), 0) for r in sim.refs] and sum(t for t, _ in at_save) > 0
        sim.submit(*flow(rng, sim, np.full(B, 8)))
        sim.step()
    mask = make_mask("alternate", B)
    env.reset_ingress_books(mask)
    for b in range(B):
        total, first = env.trade_count(b)
        if mask[b]:
            assert (total, first) == (at_save[b][0], at_save[b][0]) and len(env.trades(b)) == 0, b
        else:
            assert first == 0 and total == sim.refs[b].book.n_trades(), b
    env.close()


# ------------------------------------------------------------------ 10. refusals leave the env as it was
def test_refusals_leave_the_env_unchanged(bk, oracle):
    import torch

    B = 6
    members = member_set(1, "mixed")
    env = members_env(bk, torch, B, 8, 64, members, 1)
    env.set_agents(members)
    for _ in range(3):
        env.update_members(sync=False)
        env.step(sync=False)
    env.save_ingress_snapshot(1)
    env.update_members(sync=False)
    env.step()
    before = P.snapshot(env)
    mask = make_mask("alternate", B)
    L = bk._lib.load()
    for entry in (L.bk_ingress_snapshot_save, L.bk_ingress_snapshot_drop):
        assert entry(None, 0) == bk._lib.BK_INVALID
    assert L.bk_ingress_reset_books(None, 0, mask.astype(np.uint8).ctypes.data_as(C.c_void_p), None) == bk._lib.BK_INVALID
    with pytest.raises(bk.BourseError, match="empty"):
        env.reset_ingress_books(mask, slot=0)
    with pytest.raises(bk.BourseError, match="slot"):
        env.reset_ingress_books(mask, slot=4)
    with pytest.raises(bk.BourseError, match="slot"):
        env.save_ingress_snapshot(4)
    assert L.bk_ingress_reset_books(env._h, 1, None, None) == bk._lib.BK_INVALID and b"null mask" in L.bk_last_error()
    assert L.bk_ingress_reset_books_device(env._h, 1, None, None) == bk._lib.BK_INVALID
    with pytest.raises(ValueError):
        env.reset_ingress_books(mask[:-1], slot=1)
    with pytest.raises(ValueError):
        env.reset_ingress_books(mask, seeds=torch.zeros(B, dtype=torch.int64, device="cuda"), slot=1)
    # the entries of the other kind of env stay refused here, in their own words
    with pytest.raises(bk.BourseError, match="checkpoints"):
        env.save_snapshot()
    with pytest.raises(bk.BourseError, match="checkpoints"):
        env.reset_books(mask)
    with pytest.raises(bk.BourseError):
        env.checkpoint()
    with pytest.raises(bk.BourseError, match="bk_run cannot be mixed"):
        env.run(1)
    P.assert_same(before, P.snapshot(env))
    # other agents since the save
    env.set_agents([("noise", 0, 8, NOISE)])
    with pytest.raises(bk.BourseError, match="install the same agents first"):
        env.reset_ingress_books(mask, slot=1)
    # the same agents again: the slot's held ids and lists are no longer the env's - save again
    env.set_agents(members)
    with pytest.raises(bk.BourseError, match="bk_ingress_snapshot_save again"):
        env.reset_ingress_books(mask, slot=1)
    P.assert_same(before, P.snapshot(env))
    env.save_ingress_snapshot(1)
    env.reset_ingress_books(mask, slot=1)
    env.update_members()
    env.step()
    env.close()

    # an env without the device ingress: its entries are bk_snapshot_save / bk_reset_books
    plain = bk.ManyBookEnv(B, SEED, 0, 2, STEP, max_live_orders=64, history_capacity=4)
    plain.set_random_agents([(32, (40, 56), (10, 20), 2, 0.8)])
    plain.run(2)
    before = P.snapshot(plain)
    with pytest.raises(bk.BourseError, match="bk_snapshot_save / bk_reset_books"):
        plain.save_ingress_snapshot()
    with pytest.raises(bk.BourseError, match="bk_snapshot_save / bk_reset_books"):
        plain.reset_ingress_books(mask)
    with pytest.raises(bk.BourseError, match="bk_snapshot_save / bk_reset_books"):
        plain.drop_ingress_snapshot()
    assert plain.ingress_snapshot_bytes() == 0
    P.assert_same(before, P.snapshot(plain))
    plain.save_snapshot()
    plain.reset_books(mask)
    plain.close()
