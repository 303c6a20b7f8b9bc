"""bk_ingress_snapshot_save / bk_ingress_reset_books* (bourse_amd/csrc/ingress_reset.hpp) at the shapes where
their indexing changes: more (list entry x asset x segment) work items than k_reset_records' fixed grid has waves, several
waves and blocks of k_collect_units and k_max_keep, held-id rows and markets' books of more than one segment, a slot that was
re-saved with fewer ids than its arrays hold, and the accounts / open-order tails behind a reset over many blocks.

The expected side is the REPLAY of tests/test_gpu_ingress_reset.py - its Sim, MarketSim, flow, make_mask and as_kind, one
oracle.StepEnv(SEED + b) per book, a reset book a fresh oracle given the snapshot's calls again - and the models of
tests/accounts_model.py and tests/open_orders_model.py.  Every case counts the conditions it was written for on the expected
side (and the grid's waves from the device's properties) and asserts them before anything is compared.  The layout constants
below are DESIGN.md 2.15's, written out here: nothing is read from the library."""
import numpy as np
import pytest

import accounts_model as AM
import oracle_parity as P
from ingress_support import SEED, STEP, ingress_env, submit
from test_gpu_ingress_reset import U64_MAX, MarketSim, Sim, flow, make_mask, slice_ins
from test_gpu_open_orders import model_rows, only_new, pick
from test_gpu_open_orders import same_rows as same_open_rows

pytestmark = pytest.mark.gpu

ORD_V, LOG_V = 2, 3   # 16-byte vectors per order id in the order records / the order log
SEG_V = 256           # vectors per segment of the order records
SEG_DW = 256          # dwords per segment of a dword row
WAVES_PER_CU = 16     # k_reset_records' grid: 4 blocks x 4 waves per CU
COLLECT_BLOCK = 256   # units per block of k_collect_units (books per block of k_max_keep), 64 per wave
RECORD_BYTES = 16 * (ORD_V + LOG_V)


@pytest.fixture(scope="module")
def bk():
    import bourse_amd

    return bourse_amd


def segs(n, per):
    return -(-n // per)


def grid_waves(torch):
    return WAVES_PER_CU * torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def crossing_orders(rng, n_b, tick=1):
    """n_b[b] new limit orders for book b, in a band of prices where bids and asks cross (every one takes an id)"""
    off = np.zeros(len(n_b) + 1, dtype=np.int64)
    off[1:] = np.cumsum(n_b)
    n = int(off[-1])
    return off, (np.ones(n, np.uint32), rng.integers(0, 2, size=n).astype(np.uint8), rng.integers(1, 40, size=n).astype(np.uint32),
                 rng.integers(5000, 6000, size=n).astype(np.uint32), (rng.integers(30, 68, size=n) * tick).astype(np.uint32),
                 np.zeros(n, np.uint64))


def per_wave(mask):
    """masked units in each 64-unit wave of k_collect_units"""
    return np.add.reduceat(mask.astype(np.int64), np.arange(0, len(mask), 64))


# ------------------------------------------------------------------ 1. more work items than waves; a multi-block collect
def test_more_work_items_than_the_grid_has_waves(bk, oracle):
    """1100 books (four full blocks of k_collect_units / k_max_keep, a fifth with one full wave and one of 12 lanes) whose
    keep_b at the save runs from 0 to 240: n_keep = 240 is 2 segments of order records and 3 of the log, 5 work items per
    book, 5500 in the save against 4096 waves.  Then three resets on the one env, a step between them: a dense mask (935
    units, 4675 work items: a second, ragged trip of the stride loop), every 67th unit from the host (no wave of the collect
    holds two, the last holds none and returns), and two whole waves (units 64..127, the ragged 1088..1099)."""
    import torch

    B, pool, PRE = 1100, 256, 3
    n_waves = grid_waves(torch)
    rng = np.random.default_rng(101)
    total = rng.integers(1, 241, size=B)
    total[[3, 64, 511, 1024, 1099]] = 0   # no id at the save: keep_b = 0
    total[[0, 700, 1087]] = 240           # n_keep
    third = total // 3
    pre = [third, (total - third) // 2, total - third - (total - third) // 2]
    assert max(int(p.max()) for p in pre) <= 80

    env = ingress_env(bk, torch, B, PRE + 6, pool, 0, 96, tick=1, n_orders=320)
    sim = Sim(oracle, torch, env, B, 1)
    for n_b in pre:
        sim.submit(*crossing_orders(rng, n_b))
        sim.step()
    keep = np.array([r.book.n_orders() for r in sim.refs])
    n_keep = int(keep.max())
    assert np.array_equal(keep, total) and 171 <= n_keep <= 256
    s_book = segs(n_keep * ORD_V, SEG_V) + segs(n_keep * LOG_V, SEG_V)
    assert (segs(n_keep * ORD_V, SEG_V), segs(n_keep * LOG_V, SEG_V)) == (2, 3)
    assert B * s_book > n_waves, "the save takes no second trip of the stride loop"
    assert (keep == 0).sum() >= 5
    # rows that end inside their first segment: of the log (and the order records), of the order records only
    assert ((keep > 0) & (keep * LOG_V < SEG_V)).sum() > 100 and ((keep * LOG_V > SEG_V) & (keep * ORD_V < SEG_V)).sum() > 100
    assert segs(B, COLLECT_BLOCK) == 5 and B % COLLECT_BLOCK == 64 + 12
    sim.save()
    assert env.ingress_snapshot_bytes() == B * (env.state_bytes_per_book() + 4 * env.width + n_keep * RECORD_BYTES)

    dense = np.zeros(B, dtype=bool)
    free = np.setdiff1d(np.arange(B), [3, 64])   # of the books without an id, book 3 is masked and book 64 is not
    dense[np.random.default_rng(7).choice(free, 934, replace=False)] = True
    dense[3] = True
    assert dense.sum() == 935   # 85 % of the units
    sparse = np.zeros(B, dtype=bool)
    sparse[::67] = True
    waves = np.zeros(B, dtype=bool)
    waves[64:128], waves[1088:] = True, True
    assert dense.sum() * s_book > n_waves and dense.sum() * s_book % n_waves != 0, "no ragged second trip in the reset"
    assert set(per_wave(sparse).tolist()) == {0, 1} and sparse[0] and sparse.sum() == 17
    assert per_wave(waves).tolist() == [0, 64] + [0] * 15 + [12] and len(per_wave(waves)) == 18
    assert (keep[dense] == 0).any() and (keep[~dense] == 0).any() and keep[dense].max() == n_keep
    assert keep[waves].max() * ORD_V > SEG_V and keep[sparse].max() * ORD_V > SEG_V

    resets = {PRE + 2: (dense, "device"), PRE + 3: (sparse, "host"), PRE + 4: (waves, "device")}
    at_save = sim.saved[0]["orders"]
    for s in range(PRE, PRE + 6):
        if s in resets:
            sim.reset(*resets[s])
        # after the first reset: ids just below and AT the snapshot's next id (handed out again by then) are targeted
        force = [(at_save[b] - 1, at_save[b]) for b in range(B)] if s > PRE + 2 else None
        sim.submit(*flow(rng, sim, rng.integers(0, 4, size=B), force))
        sim.step()
    for mask in (dense, sparse, waves):   # the snapshot's next id was handed out again
        assert any(sim.refs[b].book.n_orders() > at_save[b] for b in np.flatnonzero(mask))
    assert (np.array(sim.snap_trades) < 0).sum() > 100, "books that were never reset"
    sim.check()
    env.close()


# ------------------------------------------------------------------ 2. held ids over more than one dword segment
@pytest.mark.parametrize("save_before_first_update", [False, True])
def test_held_ids_of_two_dword_segments_rewind(bk, oracle, save_before_first_update):
    """331 RandomAgents per book through update_agents: a held-id row is two dword segments, the second 75 dwords long (no
    multiple of 4); 70 books are two waves of the collect, the second of 6 lanes.  Saved after four updates the snapshot's
    ids come back, saved before the first every entry is None again - seen, as in test_random_agents_held_ids_rewind,
    through what the agents cancel and place in the updates after the reset."""
    import torch

    B, pool, NX = 70, 512, 4
    n, m, k = (0, 5, 6) if save_before_first_update else (4, 3, 4)
    groups = [(200, (32, 64), (10, 20), 2, 0.8), (131, (30, 66), (50, 70), 2, 0.3)]
    na = sum(g[0] for g in groups)
    assert na > SEG_DW and segs(na, SEG_DW) == 2 and (na - SEG_DW) % 4 != 0
    assert segs(B, 64) == 2 and B % 64 == 6
    env = ingress_env(bk, torch, B, n + m + k, pool, na, na + NX + 2, tick=2, n_ext=NX + 2)
    env.set_random_agents(groups)
    sim = Sim(oracle, torch, env, B, 2, "random", lambda b: groups)
    rng = np.random.default_rng(17)
    mask = make_mask("alternate", B)
    assert mask[64:].any() and not mask[64:].all()

    def held(b):
        return np.concatenate([sim.sets[b].held_ids(g) for g in range(len(groups))])

    for s in range(n + m + k):
        if s == n:
            if not save_before_first_update:  # a masked book holds a resting order at an agent index of the second segment
                live_beyond = 0
                for b in np.flatnonzero(mask):
                    ids, status = held(b)[SEG_DW:], sim.refs[b].book.orders_array()["status"]
                    live_beyond += int((status[ids[ids != U64_MAX].astype(np.int64)] == 1).sum())
                assert live_beyond > 0
            sim.save()  # (n = 0: no update_agents has run - the env has not made the held ids yet)
        if s == n + m:
            changed = sum(int((held(b)[SEG_DW:] != U64_MAX).sum()) for b in np.flatnonzero(mask))
            assert changed > 0, "no held id in the second segment before the reset"
            sim.reset(mask, "device" if s % 2 else "host")
            for b in np.flatnonzero(mask):  # the replay's agents right after the reset
                h = held(b)
                assert (h == U64_MAX).all() if save_before_first_update else (h[SEG_DW:] != U64_MAX).any(), b
        sim.update()
        sim.submit(*flow(rng, sim, rng.integers(0, NX + 1, size=B)))
        sim.step()
    assert sum(r.book.n_trades() for r in sim.refs) > B * k
    sim.check()
    env.close()


# ------------------------------------------------------------------ 3. markets whose books take several segments
class SkewedMarketSim(MarketSim):
    """MarketSim whose caller chooses every book's number of instructions: its mix (3 new orders to 1 cancellation of an id
    the book has handed out), prices and volumes."""

    def submit_counts(self, rng, n_b):
        B = self.NM * self.A
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


@pytest.mark.parametrize("reseed", [False, True])
def test_markets_of_several_segments_per_book_rewind(bk, oracle, reseed):
    """300 markets of 2 assets (600 books, two blocks of the collect, the second of 44 units).  Four busy / thin steps: in
    an even market asset 0 takes 60 instructions a step and asset 1 at most 3, in an odd market the reverse - n_keep >= 129
    is at least 4 segments per book, and every market pairs a book of several segments with one of fewer than 20 ids, so
    the asset of a work item and its segment both matter.  As in test_markets_rewind_both_books_and_their_queue the reseeded
    run saves the EMPTY books (a replay with another seed needs a snapshot whose calls drew nothing) and runs the busy /
    thin steps between the save and the reset: there n_keep = 0, the record kernel has nothing to move, and what the run
    adds is the reseeding of 600 books from a two-block collect."""
    import torch

    NM, A, BUSY, S = 300, 2, 4, 55_000
    n, m, k = (0, BUSY, 3) if reseed else (BUSY, 2, 3)
    env = bk.ManyMarketEnv(NM, SEED, 0, MarketSim.TICKS, STEP, levels=10, max_live_orders=256, max_orders=512, trade_capacity=1024,
                           history_capacity=n + m + k, stream=torch.cuda.current_stream().cuda_stream)
    env.enable_device_ingress(64)
    sim = SkewedMarketSim(oracle, torch, env, NM)
    rng = np.random.default_rng(13)
    mask = np.random.default_rng(5).random(NM) < 0.5
    assert segs(NM, COLLECT_BLOCK) == 2 and mask[:256].any() and mask[256:].any() and not mask.all()
    busy_asset = np.arange(NM) % 2  # the asset that is busy in the first four steps
    even, odd = (int(np.flatnonzero(mask & (busy_asset == a))[0]) for a in (0, 1))
    for s in range(n + m + k):
        if s == n:
            keep = np.array([[r.book(0, a).n_orders() for a in range(A)] for r in sim.refs])
            n_keep = int(keep.max())
            if reseed:
                assert n_keep == 0
            else:
                s_book = segs(n_keep * ORD_V, SEG_V) + segs(n_keep * LOG_V, SEG_V)
                assert n_keep >= 129 and s_book >= 4
                rows = np.arange(NM)
                assert (keep[rows, busy_asset] * ORD_V > SEG_V).all() and (keep[rows, 1 - busy_asset] < 20).all(), keep
                assert keep[even, 0] > 128 > 20 > keep[even, 1] and keep[odd, 1] > 128 > 20 > keep[odd, 0], (keep[even], keep[odd])
            sim.save()
        if s < BUSY:
            n_b = rng.integers(1, 4, size=NM * A)
            n_b[2 * np.arange(NM) + busy_asset] = 60
            sim.submit_counts(rng, n_b)
        elif s == n + m:
            sim.submit(rng, 4)  # queued for every market: a reset market's queue is emptied
            for mk in np.flatnonzero(mask):
                sim.log[mk].pop()
            sim.reset(mask, "device", seeds=(S + np.arange(NM)).astype(np.uint64) if reseed else None)
            if reseed:
                for mk in np.flatnonzero(mask):
                    want = tuple(int(x) for x in oracle.Rng(seed=S + int(mk)).st)
                    assert env.rng_state(2 * mk) == env.rng_state(2 * mk + 1) == want, mk
        else:
            sim.submit(rng, 6)
        sim.step()
    assert all(sum(r.book(0, a).n_trades() for a in range(A)) > 0 for r, on in zip(sim.refs, mask) if not (on and reseed))
    sim.check()
    env.close()


# ------------------------------------------------------------------ 4. a re-save into a slot that holds more than it needs
def test_a_slot_saved_again_with_fewer_ids(bk, oracle):
    """Slot 1 is saved after six steps, every book goes back to slot 0 (two steps), and slot 1 is saved again after one more:
    its arrays keep the first save's size and hold rows of the smaller n_keep, packed at that stride.  A reset from it, and
    include/bourse_amd.h's word on bk_ingress_snapshot_bytes: the size of the slot's arrays, which never shrink."""
    import torch

    B = 8
    per_book = np.array([12, 2, 7, 1, 9, 4, 5, 10])
    env = ingress_env(bk, torch, B, 12, 64, 0, 16, tick=1, n_orders=256)
    sim = Sim(oracle, torch, env, B, 1)
    rng = np.random.default_rng(21)

    def run(steps):
        for _ in range(steps):
            sim.submit(*flow(rng, sim, per_book))
            sim.step()

    run(2)
    sim.save(0)
    run(4)
    sim.save(1)
    state_bytes = B * (env.state_bytes_per_book() + 4 * env.width)
    first = list(sim.saved[1]["orders"])
    assert env.ingress_snapshot_bytes(1) == state_bytes + B * max(first) * RECORD_BYTES
    sim.reset(np.ones(B, dtype=bool), slot=0)
    run(1)
    sim.save(1)
    again = list(sim.saved[1]["orders"])
    assert 0 < max(again) < max(first) and len(set(again)) > 4, (again, first)
    assert env.ingress_snapshot_bytes(1) == state_bytes + B * max(first) * RECORD_BYTES  # the arrays it holds: they do not shrink
    run(3)
    mask = np.zeros(B, dtype=bool)
    mask[[0, 4, 7]] = True
    # rows beyond book 0's lie where the smaller stride puts them, and the masked books have moved on since
    assert all(sim.refs[b].book.n_orders() > again[b] > 0 for b in np.flatnonzero(mask))
    sim.reset(mask, "device", slot=1)
    run(2)
    sim.check()
    env.close()


# ------------------------------------------------------------------ 5. the tails behind a reset, across blocks
def test_accounts_and_open_orders_behind_a_reset_of_many_blocks(bk, oracle):
    """330 books with accounts and the open-order view: accounts::k_clear and open_orders::k_refresh run over the reset's
    mask with 4 books per block - 83 blocks, the last of two books, one of them masked.  Traders 0..4 have rows, 5 and 6
    trade without one.  Three steps, save, two steps, a reset from a random device mask: at once the masked books show the
    snapshot's resting orders and zero accounts and the others what they showed before; after two more steps both tables
    are their models over the replayed (masked) and the books' own (other) oracles."""
    import torch

    B, tick, NT, depth, T = 330, 2, 5, 2, 7
    assert segs(B, 4) == 83 and B % 4 == 2
    mask = np.random.default_rng(9).random(B) < 0.5
    mask[B - 2], mask[B - 1] = True, False
    on, other = np.flatnonzero(mask), np.flatnonzero(~mask)
    env = ingress_env(bk, torch, B, T, 128, 0, 16, tick=tick, n_ext=12)
    env.enable_accounts(NT)
    env.enable_open_orders(NT, depth)
    sim = Sim(oracle, torch, env, B, tick)
    rng = np.random.default_rng(60)

    def run(steps):
        for _ in range(steps):
            sim.submit(*only_new(rng, B, tick, 6, 12))  # traders 0..6
            sim.step()

    def accounts(books):
        return np.stack([AM.fold(sim.refs[b].book.trades_array(), sim.refs[b].book.orders_array(), NT, max(sim.snap_trades[b], 0))
                         for b in books])

    def same_accounts(got, want, tag):
        assert got.shape == want.shape and got.dtype == want.dtype == AM.ACCOUNT_DTYPE, tag
        for f in want.dtype.names:
            P.same_array(got[f], want[f], tag, f"account field {f}")

    def open_rows():
        return model_rows([r.book for r in sim.refs], NT, depth)

    run(3)
    sim.save()
    run(2)
    at_save = sim.saved[0]["trades"]
    since = np.stack([AM.fold(sim.refs[b].book.trades_array(), sim.refs[b].book.orders_array(), NT, at_save[b]) for b in on])
    assert since["fills"].any(axis=1).sum() > len(on) // 2, "masked books whose traders traded between the save and the reset"
    before_open, before_acct = open_rows(), accounts(range(B))
    assert before_acct["fills"][on].any() and before_acct["fills"][other].any()
    same_open_rows(env.open_orders(), before_open, "before the reset")
    same_accounts(env.accounts(), before_acct, "before the reset")

    sim.reset(mask, "device")  # no step in between: sim.refs of a masked book is its replay at the snapshot
    snap_open = open_rows()
    resting = snap_open[0]["n_bid"].astype(np.int64) + snap_open[0]["n_ask"]
    assert resting[on].any(axis=1).sum() > len(on) // 2, "masked books that rest orders at the snapshot"
    assert sum(snap_open[0][b].tolist() != before_open[0][b].tolist() for b in on) > len(on) // 2
    now_open, now_acct = env.open_orders(), env.accounts()
    same_open_rows(pick(now_open, on), pick(snap_open, on), "masked books: the snapshot's resting orders")
    same_open_rows(pick(now_open, other), pick(before_open, other), "the other books: their rows as they were")
    assert not now_acct[on].view(np.uint64).any(), "the masked books' accounts read zero at once"
    same_accounts(now_acct[other], before_acct[other], "the other books: their accounts as they were")

    run(2)
    assert sum(sim.refs[b].book.n_trades() - at_save[b] for b in on) > len(on)
    same_open_rows(env.open_orders(), open_rows(), "two steps after the reset")
    same_accounts(env.accounts(), accounts(range(B)), "two steps after the reset: reset books count from the snapshot's trades")
    sim.check()
    env.close()
