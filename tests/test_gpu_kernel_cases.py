"""Every shipped kernel instantiation against the CPU oracle, one case each (tests/kernel_cases.py): the configuration that
launches it, at the kernel's edges - two launches of different lengths, a last workgroup left partial, uneven parts, a small
look-ahead on some wave-decode cases, a pool filled into its last register - compared bit for bit (level-2 history of every
step and book, trade records, live orders in price-time order, RNG states, clocks, trade counts, the order log and its keys
where one is kept, flags), with the path it took read back: pipeline(), the per-kind launch counts of profile(1), and the
keyed-step counter of the host-driven steps."""
import numpy as np
import pytest

import oracle_parity as P

from kernel_cases import CASES, TICKS, market_members, members, random_groups, random_market_groups

pytestmark = pytest.mark.gpu

SEED, STEP, LEVELS, THREADS = 101, 100_000, 10, 16


@pytest.fixture(scope="module")
def bk():
    import bourse_amd

    return bourse_amd


def _live(view):
    return int((view.orders_array()["status"] == 1).sum())


class _Refs:
    """The oracle of a case: one ManyBooks / ManyMarkets per row of the agents' table (unit u runs row u % rows)."""

    def __init__(self, oracle, case, tick, step):
        self.o, self.mkt, self.U = oracle, case["markets"], case["units"]
        self.A = len(TICKS) if self.mkt else 1
        R, ag = case["R"], case["agents"]
        self.rows = 2 if ag.endswith("_table") else 1
        self.refs = []
        for v in range(self.rows):
            if self.mkt:
                kw = dict(members=market_members(R, v)) if ag.startswith("members") else dict(groups=random_market_groups(R, v))
                self.refs.append(oracle.ManyMarkets(self.U, SEED, 0, TICKS, step, True, LEVELS, **kw))
            else:
                kw = dict(members=members(R, v)) if ag.startswith("members") else dict(groups=random_groups(R, v))
                self.refs.append(oracle.ManyBooks(self.U, SEED, 0, tick, step, True, LEVELS, **kw))

    def _ref(self, b):
        return self.refs[(b // self.A) % self.rows]

    def run(self, n):
        for r in self.refs:
            r.run(n, n_threads=THREADS)

    def set_trading(self, on):
        for r in self.refs:
            if self.mkt:
                r.set_trading(on)
            else:
                for b in range(self.U):
                    self.o.lib().orc_book_set_trading(r.book(b)._b, int(on))

    def view(self, b):
        r = self._ref(b)
        return r.book(b // self.A, b % self.A) if self.mkt else r.book(b)

    def history(self):
        hs = [r.history() for r in self.refs]
        h = hs[0].copy()
        for b in range(self.U * self.A):
            h[:, b] = hs[(b // self.A) % self.rows][:, b]
        return h

    def rngs(self):
        st = [r.rng_states() for r in self.refs]
        return [tuple(int(x) for x in st[(b // self.A) % self.rows][b // self.A]) for b in range(self.U * self.A)]


def _expected_launches(case, n, parts):
    """profile_read_kind(0..3) launch counts of one run(n): 0 the fused kernel, 1 the agents kernel, 2 the event kernel
    of the split kinds (k_step_batch / k_step_batch_log / k_step_decode), 3 k_step_events"""
    if case["kind"] in ("fused", "wave"):
        return [1, 0, 0, 0]
    agents = parts if case["knobs"].get("BOURSE_AMD_STEP_DECODE") == "1" else n * parts
    return [0, agents, n * parts, 0]


def _launch_counts(env):
    c = [env.profile_read_kind(k)[1] for k in range(4)]
    env.profile_read(reset=True)
    return c


def _run_flow(bk, oracle, case):
    R, pool, U, mkt = case["R"], case["pool"], case["units"], case["markets"]
    A = len(TICKS) if mkt else 1
    NB = U * A
    tick, step = (2, STEP) if case["agents"].startswith("random") else (1, 1_000_000)
    T = sum(case["launches"])
    cap = dict(levels=LEVELS, max_live_orders=pool, max_orders=(2 * pool * T + 64) if case["log"] else 0,
               trade_capacity=4 * pool * T + 64, history_capacity=T)
    env = (bk.ManyMarketEnv(U, SEED, 0, TICKS, step, True, **cap) if mkt
           else bk.ManyBookEnv(U, SEED, 0, tick, step, True, **cap))
    ag = case["agents"]
    if ag == "random":
        env.set_random_market_agents(random_market_groups(R)) if mkt else env.set_random_agents(random_groups(R))
    elif ag == "random_table":
        if mkt:
            env.set_random_market_agents_per_market([random_market_groups(R, u % 2) for u in range(U)])
        else:
            env.set_random_agents_per_book([random_groups(R, u % 2) for u in range(U)])
    elif ag == "members":
        env.set_market_agents(market_members(R)) if mkt else env.set_agents(members(R))
    else:
        if mkt:
            env.set_market_agents_per_market([market_members(R, u % 2) for u in range(U)])
        else:
            env.set_agents_per_book([members(R, u % 2) for u in range(U)])
    if case["log"]:
        env.enable_agent_order_log()
    if case["pipeline"]:
        env.set_pipeline(case["pipeline"])
    if case["split_parts"]:
        env.set_split_parts(*case["split_parts"])
    if case["wave_options"]:
        env.set_wave_options(*case["wave_options"])
    assert env.pipeline() == (case["kind"], case["parts"])
    ref = _Refs(oracle, case, tick, step)
    env.profile(1)
    fill = 0
    for i, n in enumerate(case["launches"]):
        # the first launch (an odd number of steps) with trading off leaves every filler agent's order resting
        trading = i > 0
        (env.enable_trading if trading else env.disable_trading)()
        ref.set_trading(trading)
        env.run(n)
        ref.run(n)
        assert _launch_counts(env) == _expected_launches(case, n, case["parts"]), (i, n)
        P.no_flags(env)
        tc, rngs = env.trade_counts(), ref.rngs()
        for b in range(NB):
            view = ref.view(b)
            assert env.rng_state(b) == rngs[b], (i, b)
            assert env.time(b) == view.get_time(), (i, b)
            assert int(tc[b]) == len(view.trades_array()), (i, b)
            live = _live(view)
            assert len(env.live_orders(b)) == live, (i, b)
            fill = max(fill, live)
    hist = env.history()
    P.same_history(hist, ref.history())
    assert np.array_equal(env.level2(), hist[-1])
    for b in range(NB):
        view = ref.view(b)
        P.same_book(env, b, view, orders=case["log"], keys=case["log"])
    assert int(env.trade_counts().sum()) > 0
    env.close()
    return fill


# ------------------------------------------------------------------------------------------------- host-driven steps
def _host_flow(bk, oracle, case):
    R, pool, U, mkt = case["R"], case["pool"], case["units"], case["markets"]
    A = len(TICKS) if mkt else 1
    NB, T = U * A, sum(case["launches"])
    n_fill = 64 * (R - 1) + 8 if R > 1 else 40
    cap = dict(levels=LEVELS, max_live_orders=pool, max_orders=(64 * R + 24) * T + 64, trade_capacity=8 * 64 * R * T,
               history_capacity=T)
    if mkt:
        env = bk.ManyMarketEnv(U, SEED, 0, TICKS, STEP, True, **cap)
        ref = oracle.ManyMarkets(U, SEED, 0, TICKS, STEP, True, LEVELS)
        views = [ref.book(b // A, b % A) for b in range(NB)]
    else:
        env = bk.ManyBookEnv(U, SEED, 0, 1, STEP, True, **cap)
        refs = [oracle.StepEnv(SEED + b, 0, 1, STEP, True, LEVELS) for b in range(U)]
        views = [r.book for r in refs]
    ticks = TICKS if mkt else (1,)

    def call(f, b, *args):
        u, a = divmod(b, A)
        if mkt:
            got, want = getattr(env, f)(u, a, *args), getattr(ref, f)(u, a, *args)
        else:
            got, want = getattr(env, f)(b, *args), getattr(refs[b], f)(*args)
        if f == "place_order":
            assert got == want, (f, b, args)

    rng = np.random.default_rng(case["R"] * 7 + len(case["name"]))
    made = np.zeros(NB, dtype=np.int64)
    env.profile(1)
    keyed_before, s, fill = 0, 0, 0
    first_mod, longest = None, []
    for i, n_steps in enumerate(case["launches"]):
        for _ in range(n_steps):
            queue = np.zeros(U, dtype=np.int64)
            mods = case["mods_from"] is not None and s >= case["mods_from"]
            for u in range(U):
                if s == 0:  # resting orders on both sides of 100 that do not cross: the pool's last register in use
                    for k in range(n_fill):
                        bid = k % 2 == 0
                        price = int(rng.integers(60, 90)) if bid else int(rng.integers(111, 141))
                        call("place_order", u * A, bid, int(rng.integers(1, 31)), k, price * ticks[0])
                    made[u * A] += n_fill
                    queue[u] += n_fill
                    continue
                burst = case["chunks"] and s in (1, T - 1)
                n_ops = 64 * R + 8 + int(rng.integers(0, 9)) if burst else int(rng.integers(20, 41))
                budget = [pool - 4 - _live(views[u * A + a]) for a in range(A)]
                for _ in range(n_ops):
                    a = int(rng.integers(0, A))
                    b, tk = u * A + a, ticks[a]
                    x = rng.random()
                    if x < 0.15 and mods and made[b]:
                        oid = int(rng.integers(0, made[b]))
                        new_p = int(rng.integers(88, 113)) * tk if rng.random() < 0.6 else None
                        new_v = int(rng.integers(1, 31)) if (new_p is None or rng.random() < 0.5) else None
                        call("modify_order", b, oid, new_p, new_v)
                        first_mod = s if first_mod is None else first_mod
                    elif x < 0.25:
                        call("place_order", b, bool(rng.integers(0, 2)), int(rng.integers(1, 6)), 1, None)
                        made[b] += 1
                    elif x < 0.6 and budget[a] > 0:
                        call("place_order", b, bool(rng.integers(0, 2)), int(rng.integers(1, 21)), 2,
                             int(rng.integers(85, 116)) * tk)
                        made[b] += 1
                        budget[a] -= 1
                    elif made[b]:
                        call("cancel_order", b, int(rng.integers(0, made[b])))
                    else:
                        continue
                    queue[u] += 1
            longest.append(int(queue.max()))
            env.step()
            if mkt:
                ref.step()
            else:
                for r in refs:
                    r.step()
            s += 1
        # a checked point
        assert _launch_counts(env) == [0, 0, 0, n_steps], i
        P.no_flags(env)
        for b in range(NB):
            live = _live(views[b])
            assert len(env.live_orders(b)) == live, (i, b)
            fill = max(fill, live)
        keyed = int(env.event_steps_keyed().sum())
        assert keyed > keyed_before, "no step of this launch ran on the keyed event loop"
        keyed_before = keyed
    # the case's own input meets the instantiation's precondition
    if case["chunks"]:
        assert max(longest) > 64 * R, longest
    else:
        assert max(longest) <= 64 * R, longest
    if R == 8 and not case["chunks"]:
        assert first_mod == case["mods_from"] and max(longest[:first_mod]) <= 64 * R, (first_mod, longest)
    hist = env.history()
    if mkt:
        P.same_history(hist, ref.history())
    else:
        for b, r in enumerate(refs):
            P.same_history(hist[:, b], r.history(), f"L2 history of book {b}")
    assert np.array_equal(env.level2(), hist[-1])
    tc = env.trade_counts()
    for b in range(NB):
        view = views[b]
        want_rng = tuple(int(x) for x in ref.rng_states()[b // A]) if mkt else tuple(int(x) for x in refs[b].rng_state())
        assert env.rng_state(b) == want_rng, b
        assert env.time(b) == view.get_time(), b
        assert int(tc[b]) == len(view.trades_array()), b
        P.same_book(env, b, view, orders=True, keys=True)
    assert int(tc.sum()) > 0
    env.close()
    return fill


# --------------------------------------------------------------------------------------- agents into the device queues
def _update_flow(bk, oracle, case):
    R, pool, B = case["R"], case["pool"], case["units"]
    groups = random_groups(R)
    na = sum(g[0] for g in groups)
    T = sum(case["launches"])
    env = bk.ManyBookEnv(B, SEED, 0, 2, STEP, levels=LEVELS, max_live_orders=pool, max_orders=na * T + 16,
                         trade_capacity=2 * na * T + 64, history_capacity=T)
    env.enable_device_ingress(queue_capacity=na)
    env.set_random_agents(groups)
    refs = [oracle.StepEnv(SEED + b, 0, 2, STEP, True, LEVELS) for b in range(B)]
    agents = [oracle.RandomAgentSet(groups) for _ in range(B)]
    env.profile(1)
    fill = 0
    for i, n in enumerate(case["launches"]):
        trading = i > 0  # (the first launch, an odd number of steps, with trading off: every filler agent's order rests)
        (env.enable_trading if trading else env.disable_trading)()
        for r in refs:
            (r.enable_trading if trading else r.disable_trading)()
        for _ in range(n):
            env.update_agents(sync=False)
            env.step(sync=False)
            for r, a in zip(refs, agents):
                a.update(r)
                r.step()
        env.sync()
        assert _launch_counts(env) == [0, 0, 0, n], i
        P.no_flags(env)
        for b in range(B):
            live = _live(refs[b].book)
            assert len(env.live_orders(b)) == live, (i, b)
            fill = max(fill, live)
    assert na <= 64 * R  # (the queue's capacity is the longest queue: no chunks)
    hist = env.history()
    for b, r in enumerate(refs):
        P.same_history(hist[:, b], r.history(), f"L2 history of book {b}")
        assert env.rng_state(b) == tuple(int(x) for x in r.rng_state()), b
        assert env.time(b) == r.book.get_time(), b
        P.same_book(env, b, r.book, orders=True, keys=True)
    assert np.array_equal(env.level2(), hist[-1])
    assert int(env.trade_counts().sum()) > 0
    env.close()
    return fill


FLOWS = {"run": _run_flow, "host": _host_flow, "update": _update_flow}


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_case(bk, oracle, monkeypatch, name):
    case = CASES[name]
    assert case["unreachable"] is None, case["unreachable"]
    for k, v in case["knobs"].items():  # (read when the env is created)
        monkeypatch.setenv(k, v)
    assert len(set(case["launches"])) >= 2
    fill = FLOWS[case["flow"]](bk, oracle, case)
    R = case["R"]
    if R >= 2:  # a bug confined to the pool's upper registers cannot pass unseen
        assert fill > 64 * (R - 1), (fill, 64 * (R - 1))
