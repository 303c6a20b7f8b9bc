"""What the device-ingress tests with on-device agents share: the env they build, how one step's instructions reach the
device and the oracle, the comparison of every book with its own oracle.StepEnv (tests/oracle_parity.py), the thin flow of
external orders a Momentum member needs to start, and the busy conditions no Noise / Momentum case may pass without."""
import numpy as np

import oracle_parity as P
from members_ingress_cases import NOISE

MOD = 0x80000003  # BK_ACTION_MODIFY
SEED, STEP = 31, 100_000


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ingress_env(bk, torch, B, T, pool, n_agents, qcap, tick=2, n_ext=0, levels=10, strict=True, n_orders=None):
    n_orders = n_orders or (2 * n_agents + n_ext) * T + 16
    env = bk.ManyBookEnv(B, SEED, 0, tick, STEP, levels=levels, max_live_orders=pool, max_orders=n_orders,
                         trade_capacity=2 * n_orders, history_capacity=T, strict=strict,
                         stream=torch.cuda.current_stream().cuda_stream)
    env.enable_device_ingress(queue_capacity=qcap)
    return env


def members_env(bk, torch, B, T, pool, members, tick, n_ext=0, updates=1, strict=True):
    """an env whose queue takes `updates` updates of the set (every agent's orders, and a cancellation for every order
    that can rest) and n_ext instructions per step, and whose order log takes the run's orders"""
    per_update = sum(m[1] if m[0] == "random" else 2 * m[2] for m in members)
    return ingress_env(bk, torch, B, T, pool, 0, (per_update + pool) * updates + n_ext, tick=tick, strict=strict,
                       n_orders=(per_update * updates + n_ext) * T + 16)


def check(env, refs, books=None):
    """Every book (or ``books``) against its oracle StepEnv: level-2 history, trades, live orders in priority order, the
    order log with one order_status, the order keys and the RNG state."""
    env.sync()
    hist = env.history()
    for b in (range(env.n_books) if books is None else books):
        ref = refs[b]
        P.same_history(hist[:, b], ref.history(), f"L2 history of book {b}")
        P.same_book(env, b, ref.book, orders=True, keys=True)
        got, want = env.rng_state(b), tuple(int(x) for x in ref.rng_state())
        assert got == want, f"book {b}: rng state {got} vs {want}"


def apply_oracle(ref, lo, hi, ins):
    action, side, vol, trader, price, order_id = ins
    for i in range(lo, hi):
        a = int(action[i])
        if a == 1:
            ref.place_order(bool(side[i] & 1), int(vol[i]), int(trader[i]), price=int(price[i]))
        elif a == 2:
            ref.cancel_order(int(order_id[i]))
        elif a == MOD:
            ref.modify_order(int(order_id[i]), new_price=int(price[i]) if side[i] & 2 else None,
                             new_vol=int(vol[i]) if side[i] & 4 else None)


def submit(torch, env, off, ins):
    if len(ins[0]):
        env.submit_instructions_device(dev(torch, off), *[dev(torch, x) for x in ins])


def thin_flow(rng, B, n_max, tick):
    """new orders only: a few limit orders in a band of prices and now and then a market order, for every book"""
    n_b = rng.integers(0, n_max + 1, size=B)
    off = np.zeros(B + 1, dtype=np.int64)
    off[1:] = np.cumsum(n_b)
    n = int(off[-1])
    bid = rng.integers(0, 2, size=n).astype(np.uint8)
    price = (rng.integers(40, 60, size=n) * tick).astype(np.uint32)
    if tick == 1:
        market = rng.random(n) < 0.1
        price[market] = np.where(bid[market] == 1, 0xFFFFFFFF, 0)
    return off, (np.ones(n, np.uint32), bid, rng.integers(20, 200, size=n).astype(np.uint32),
                 rng.integers(5000, 6000, size=n).astype(np.uint32), price, np.zeros(n, np.uint64))


class BusyCounts:
    """The conditions under which a Noise / Momentum comparison says something, counted on the EXPECTED side (the oracle's
    or the model's) while it runs, from its orders and order lists alone, and asserted before anything is compared: per
    Noise / Momentum member a cancellation queued by cancel_live_orders, a limit order, a market order and a list entry
    dropped as not Active; a Momentum member's momentum (the recursion of momentum_agent.rs:152-158 over the expected
    side's mid prices) both above and below 0."""

    def __init__(self, members):
        self.kinds = {j: m[0] for j, m in enumerate(members) if m[0] != "random"}
        self.count = {j: dict(cancel=0, limit=0, market=0, dropped=0, m_pos=0, m_neg=0) for j in self.kinds}
        self.mom = {}  # (book, member) -> (momentum, last mid)
        self.longest_list = self.largest_batch = 0  # most Active ids one list held at an update; most orders of one update

    def note(self, b, members, status, n0, lists0, lists1, created, mid):
        """one update of book b: `status` of the n0 orders it had before, the members' lists before and after (by member
        index), the orders it `created` (fields trader_id, side, price) and the mid price the members saw"""
        trader, side, price = (np.asarray(created[k]) for k in ("trader_id", "side", "price"))
        self.largest_batch = max(self.largest_batch, len(trader))
        for j in self.kinds:
            kind, start, n, p = members[j]
            c = self.count[j]
            kept = set(int(i) for i in lists1[j])
            self.longest_list = max(self.longest_list, sum(1 for i in lists0[j] if status[int(i)] == 1))
            for i in lists0[j]:
                if status[int(i)] != 1:
                    c["dropped"] += 1  # not Status::Active: no draw, gone from the list
                elif int(i) not in kept:
                    c["cancel"] += 1   # Active and not kept: its cancellation was queued
            mine = (trader >= start) & (trader < start + n)
            market = ((side == 1) & (price == 0xFFFFFFFF)) | ((side == 0) & (price == 0))
            # (the sets of one run use disjoint trader id ranges above the RandomAgents members' indices)
            c["market"] += int((mine & market).sum())
            c["limit"] += int(sum(1 for i in kept if i >= n0))
            if kind == "momentum":
                m = 0.0
                if (b, j) in self.mom:
                    m0, last = self.mom[(b, j)]
                    m = m0 * (1.0 - p["decay"]) + p["decay"] * (mid - last)
                c["m_pos"] += m > 0.0
                c["m_neg"] += m < 0.0
                self.mom[(b, j)] = (m, mid)

    def assert_busy(self, momentum_signs=True):
        for j, kind in self.kinds.items():
            c = self.count[j]
            for k in ("cancel", "limit", "market", "dropped"):
                assert c[k] > 0, (j, k, c)
            if kind == "momentum" and momentum_signs:
                assert c["m_pos"] > 0 and c["m_neg"] > 0, (j, c)


# --------------------------------------------------------------------- members wider than a wave (more than 64 traders)
# One Noise member of 70 traders who all place a limit and a market order in every update (140 New events: place_new
# flushes its 64-entry batch twice inside the loop), and one Momentum member of 130 traders whose p_limit and p_market
# pass 1 as soon as the mid price rose (260 New events).  The orders must pile up for the cancel filter to take a second
# and a third 64-entry pass over a list:
# * the Noise member's steps 0-2 run with trading off (its bids <= mid <= asks never cross), so its list holds about 70,
#   126 and 171 Active ids at updates 1-3;
# * the Momentum member's limit orders lie about e^5 = 150 below the mid price, behind the touch, and only a rise of the
#   mid price (momentum > 0) makes it trade at all: demand * tanh(..) is negative below 0.  wide_flow scripts the touch with
#   external orders of a volume no market order dents: two rises a step apart (about 213 Active ids) for a 256-slot pool, three in a row for
#   512 slots, and two listed ids cancelled from outside so that the next filter drops them as not Active.
WIDE_STEPS, WIDE_P_CANCEL = 8, 0.2
_WIDE_RISES = {256: (1, 3), 512: (1, 2, 3, 6)}


def wide_set(which):
    if which == "noise":
        return [("noise", 0, 70, dict(NOISE, p_limit=1.0, p_market=1.0, p_cancel=WIDE_P_CANCEL))]
    assert which == "momentum", which
    return [("momentum", 0, 130, dict(tick_size=1, p_cancel=WIDE_P_CANCEL, trade_vol=1, decay=1.0, demand=200.0, scale=0.5,
                                      order_ratio=1.5, price_dist_mu=5.0, price_dist_sigma=0.25))]


def wide_trading(which, s):
    """whether step s trades"""
    return which != "noise" or s >= 3


def wide_flow(which, pool, s, B, listed):
    """step s's external instructions for every book (the same for each; `listed(b)`: the member's current list on the
    expected side), as (offsets, arrays) in submit's / apply_oracle's format"""
    rows = []  # (action, bid, vol, price, order ids wanted)
    if which == "momentum":
        rises = _WIDE_RISES[pool]
        if s == 0:
            rows += [(1, 1, 1_000_000, 1000, None), (1, 0, 1_000_000, 1100, None)]
        elif s in rises:
            rows.append((1, 1, 1_000_000, 1000 + 10 * (rises.index(s) + 1), None))  # the best bid, and the mid, rise
        elif s % 2 == 0:
            rows.append((1, 0, 1_000_000, 1100 - 5 * s, None))                     # the best ask, and the mid, fall
        if s == 4:
            rows += [(2, 0, 0, 0, 0), (2, 0, 0, 0, 1)]                             # cancel the list's first two ids
    per_book = []
    for b in range(B):
        ids = listed(b) if any(r[0] == 2 for r in rows) else []
        per_book.append([r if r[0] == 1 else r[:4] + (int(ids[r[4]]),) for r in rows if r[0] == 1 or r[4] < len(ids)])
    off = np.zeros(B + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(r) for r in per_book])
    flat = [r for rs in per_book for r in rs]
    col = lambda k, dt: np.array([r[k] or 0 for r in flat], dtype=dt)
    return off, (col(0, np.uint32), col(1, np.uint8), col(2, np.uint32), np.full(len(flat), 5000, np.uint32),
                 col(3, np.uint32), col(4, np.uint64))
