"""The retune (bk_retune_* / ManyBookEnv.retune_random_agents, retune_agents, ManyMarketEnv.retune_*): the parameter records
of chosen units of the installed per-unit table rewritten in place on the device, with everything the agents hold kept.

1. identities against the existing pipelines with trading on: a retune with the installed rows changes nothing, an env
   installed with T0 and retuned to T equals an env installed with T, and under a mask the unmasked books equal a control
   bit for bit while the masked ones differ;
2. the ingress path against tests/agents_model.py, fed mode (FedRun of tests/test_gpu_agents_model.py for the members, a
   loop of its own for RandomAgents groups): the model's agents get their attributes assigned, the env is retuned from a
   torch tensor, and the generator, the appended orders and the members' lists stay the model's - with orders from before
   the retune kept and cancelled after it;
3. bk_run's pipelines with trading off against the model's RestingBook, retuned between two runs;
4. the oracle's one in-place assignment (AgentSet.set_noise_prob) under bk_run and on the ingress path;
5. cross-path: bk_run against update_agents + step given the same retune;
6. refusals inside the kernel: status pairs and the counter are tests/retune_model.py's, refused units keep their rows;
7. markets; 8. with the masked reset, in one stream order, and across a checkpoint; 8b. the host entry's staging made and
grown, against the device entry; 9. no wait on the device path; 10. the API's refusals.
The expected sides share no text with the kernel."""
import numpy as np
import pytest

import agents_model as M
import oracle_parity as P
import retune_model as RM
from ingress_support import members_env, thin_flow
from members_ingress_cases import MOM, NOISE
from test_gpu_agents_model import FedRun

pytestmark = pytest.mark.gpu

SEED, STEP, LEVELS = 101, 100_000, 10
B70, K, N = 70, 7, 20
SIZES = (50, 41, 30)


@pytest.fixture(scope="module")
def bk():
    import bourse_amd

    return bourse_amd


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def raw(torch, arr):
    """a structured numpy table as the int32 tensor [units, width, words] of its raw rows"""
    arr = np.ascontiguousarray(arr)
    t = torch.from_numpy(arr.view(np.int32).reshape(arr.shape + (arr.dtype.itemsize // 4,)).copy()).cuda()
    torch.cuda.synchronize()
    return t


def dev(torch, a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def group_rows(n_units, seed, sizes=SIZES, tick=2):
    r = np.random.default_rng(seed)
    rows = []
    for _ in range(n_units):
        row = []
        for n in sizes:
            tlo = int(r.integers(20, 200))
            tw = int(r.choice([1, int(r.integers(2, 40)), int(r.integers(100, 900))]))
            vlo = int(r.integers(1, 60))
            vw = int(r.choice([1, int(r.integers(2, 30)), int(r.integers(200, 2000))]))
            row.append((n, (tlo, tlo + tw), (vlo, vlo + vw), tick * int(r.integers(1, 5)), float(r.uniform(0.2, 0.9))))
        rows.append(row)
    return rows


def group_table(bk, rows):
    from bourse_amd import env as E

    return E._agents_table(rows, len(rows), lambda g: g)


def member_rows(n_units, seed, n_noise=40, n_mom=20):
    r = np.random.default_rng(seed)
    return [[("noise", 0, n_noise, dict(NOISE, p_limit=float(np.float32(r.uniform(0.2, 0.6))), p_cancel=float(np.float32(r.uniform(0.1, 0.4))),
                                        price_dist_mu=float(r.uniform(-0.5, 1.0)), price_dist_sigma=float(r.uniform(0.5, 2.0)))),
             ("momentum", 1000, n_mom, dict(MOM, demand=float(r.uniform(4.0, 30.0)), decay=float(r.uniform(0.3, 1.0)),
                                            price_dist_mu=float(r.uniform(0.0, 1.0)), price_dist_sigma=float(r.uniform(1.0, 8.0))))]
            for _ in range(n_units)]


def member_table(rows):
    from bourse_amd import env as E

    return E._members_rows(rows, len(rows))


def book_env(bk, B=B70, pool=128, **kw):
    return bk.ManyBookEnv(B, SEED, 0, 2, STEP, True, levels=LEVELS, max_live_orders=pool, trade_capacity=3 * pool * N,
                          history_capacity=N, **kw)


def differs(x, y, b):
    return not np.array_equal(x["history"][:, b], y["history"][:, b]) or x["rng"][b] != y["rng"][b]


def identities(bk, torch, make, install, retune, t0, t, t2, mode):
    """1a - 1c for one kind of table: `make()` an env, `install(env, rows)`, `retune(env, table, mask, dev)`"""
    mask = np.zeros(B70, dtype=np.uint8)
    mask[[0, 5, 8, 31, 63, 64, 69]] = 1

    def run(first, *then):
        env = make()
        install(env, first)
        env.set_pipeline(mode)
        for f in then:
            f(env)
        snap = P.snapshot(env)
        P.no_flags(env)
        env.close()
        return snap

    control = run(t, lambda e: e.run(K), lambda e: e.run(N - K))
    assert int(control["trade_counts"].sum()) > 0  # trading is on and trades happen
    # a. the installed rows again, at step 0 (device entry) and in the middle of the run (host entry): nothing changes
    same = run(t, lambda e: retune(e, t, None, True), lambda e: e.run(K), lambda e: retune(e, t, mask, False),
               lambda e: e.run(N - K), lambda e: retune(e, t, None, True))
    P.assert_same(control, same)
    # b. installed with T0, retuned to T before the first step
    for on_dev in (True, False):
        P.assert_same(control, run(t0, lambda e: retune(e, t, None, on_dev), lambda e: e.run(K), lambda e: e.run(N - K)))
    # c. a mask in the middle of the run: the others carry on, the masked books change
    for on_dev in (True, False):
        got = run(t, lambda e: e.run(K), lambda e: retune(e, t2, mask, on_dev), lambda e: e.run(N - K))
        for b in range(B70):
            if mask[b]:
                assert differs(got, control, b), f"book {b} was retuned and runs as before"
                assert np.array_equal(got["history"][:K, b], control["history"][:K, b]), b
            else:
                assert np.array_equal(got["history"][:, b], control["history"][:, b]), b
                assert got["rng"][b] == control["rng"][b] and int(got["trade_counts"][b]) == int(control["trade_counts"][b]), b
                P.same_records(got["trades"][b], control["trades"][b], b, "trade")
                P.same_records(got["live"][b], control["live"][b], b, "live order")


# ------------------------------------------------------------------ 1. identities, every bk_run pipeline with a PB form
@pytest.mark.parametrize("mode", ["auto", "split", "wave_split", "wave"])
def test_random_agents_identities(bk, torch, mode):
    t0, t = group_rows(B70, 1), group_rows(B70, 2)
    t2 = [[(n, (tr[0] + 300, tr[1] + 400), (vr[0] + 5, vr[1] + 9), 2, 1.0) for n, tr, vr, ts, rate in row] for row in t]

    def retune(env, rows, mask, on_dev):
        tab = group_table(bk, rows)
        if on_dev:
            env.retune_random_agents(raw(torch, tab), None if mask is None else dev(torch, mask))
        else:
            env.retune_random_agents(rows if mask is None else tab, mask)
        assert env.retune_rejected() == 0

    identities(bk, torch, lambda: book_env(bk), lambda e, r: e.set_random_agents_per_book(r), retune, t0, t, t2, mode)


@pytest.mark.parametrize("mode", ["auto", "fused", "split", "split_wave", "wave_split"])
def test_members_identities(bk, torch, mode):
    t0, t = member_rows(B70, 3), member_rows(B70, 4)
    t2 = [[("noise", 0, 40, dict(NOISE, p_limit=0.9, p_market=0.05, p_cancel=0.5, price_dist_mu=2.0, price_dist_sigma=0.25, trade_vol=37)),
           ("momentum", 1000, 20, dict(MOM, demand=50.0, decay=0.5, scale=0.1, order_ratio=3.0, price_dist_sigma=2.0))] for _ in t]

    def retune(env, rows, mask, on_dev):
        if on_dev:
            env.retune_agents(raw(torch, member_table(rows)), None if mask is None else dev(torch, mask))
        else:
            env.retune_agents(rows, mask)
        assert env.retune_rejected() == 0

    identities(bk, torch, lambda: book_env(bk, pool=512), lambda e, r: e.set_agents_per_book(r), retune, t0, t, t2, mode)


# ------------------------------------------------------------------ 2. the ingress path against the agents model, fed
def assign(member, m):
    """the reference's field assignment on a model agent, from a member tuple"""
    if m[0] == "random":
        _, n, tr, vr, ts, rate = m
        member.tick_range, member.vol_range, member.tick_size, member.rate = tr, vr, ts, M.f32(rate)
        return
    p = m[3]
    member.tick_size, member.trade_vol, member.p_cancel = float(p["tick_size"]), p["trade_vol"], M.f32(p["p_cancel"])
    member.mu, member.sigma = p["price_dist_mu"], p["price_dist_sigma"]
    if m[0] == "noise":
        member.p_limit, member.p_market = M.f32(p["p_limit"]), M.f32(p["p_market"])
    else:
        member.decay, member.demand, member.scale, member.order_ratio = p["decay"], p["demand"], p["scale"], p["order_ratio"]


def fed_rows(b, width, new):
    r = np.random.default_rng((7000 if new else 6000) + b)
    rnd = ("random", 12, (900, 940) if new else (32, 64), (500, 520) if new else (10, 20), 2 if new else 1, 0.95 if new else 0.9)
    noise = ("noise", 100, 10, dict(NOISE, tick_size=1, p_limit=float(np.float32(r.uniform(0.3, 0.6))),
                                    p_cancel=0.6 if new else 0.15, trade_vol=777 if new else 100,
                                    price_dist_mu=float(r.uniform(-0.5, 1.0)), price_dist_sigma=float(r.uniform(0.5, 2.0))))
    mom = ("momentum", 200, 8, dict(MOM, tick_size=1, decay=float(r.uniform(0.3, 0.9)), demand=float(r.uniform(10.0, 30.0)),
                                    scale=float(r.uniform(0.6, 1.5)) if new else 0.5, order_ratio=float(r.uniform(1.5, 3.0)) if new else 1.0,
                                    p_cancel=0.5 if new else 0.1, trade_vol=555 if new else 100, price_dist_sigma=float(r.uniform(1.0, 8.0))))
    if width == 2:
        return [noise, mom]
    extra = [("noise", 300 + 20 * i, 4, dict(NOISE, tick_size=1, p_limit=0.3 + 0.1 * i + (0.05 if new else 0.0))) for i in range(2)]
    return [rnd, noise, mom] + extra  # width 5: above MAX_MEMBERS, ingress only


@pytest.mark.parametrize("width", [2, 5])
def test_update_members_after_a_retune_equals_the_model(bk, torch, width):
    B, T, k = 33, 9, 4
    mask = np.zeros(B, dtype=np.uint8)
    mask[[0, 3, 7, 8, 20, 31, 32]] = 1
    old = [fed_rows(b, width, False) for b in range(B)]
    new = [fed_rows(b, width, True) if mask[b] else old[b] for b in range(B)]
    env = members_env(bk, torch, B, T, 256, old[0], 1, n_ext=4)
    env.set_agents_per_book(old)
    run = FedRun(env, torch, lambda b: old[b], 1)
    rng = np.random.default_rng(77)
    n_mom = 1 if width == 2 else 2
    # the conditions, per member, all counted on the model's side (its lists and the events of its views)
    kept, cancelled_old, new_range = [0] * width, [0] * width, [0] * width
    mom_nonzero = mom_orders_after = 0
    for s in range(T):
        if s == k:
            before = {b: [list(run.models[b].order_list(j)) for j in range(width)] for b in range(B) if mask[b]}
            for b in np.flatnonzero(mask):
                mom_nonzero += run.models[b].members[n_mom].momentum != 0.0
                for member, m in zip(run.models[b].members, new[b]):
                    assign(member, m)
                run.members[b] = new[b]
            status = torch.full((B, 2), 99, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            # (rows of unmasked books are not read: poison them)
            tab = member_table([new[b] if mask[b] else [("noise", 0, 0, dict(NOISE, tick_size=0))] * width for b in range(B)])
            env.retune_agents(raw(torch, tab), dev(torch, mask), status)
            assert status.cpu().numpy().tolist() == [[0, 0]] * B and env.retune_rejected() == 0
        lists0 = {b: [list(run.models[b].order_list(j)) for j in range(width)] for b in np.flatnonzero(mask)} if s >= k else {}
        run.update()  # generator, appended orders and every member's list against the model, exactly
        for b in lists0:
            for j in range(width):
                now = run.models[b].order_list(j)
                fresh = [i for i in now if i != M.M64 and i not in lists0[b][j]]  # the member's orders of this update
                if s == k:
                    kept[j] += sum(1 for i in now if i != M.M64 and i in before[b][j])
                    cancelled_old[j] += sum(1 for i in before[b][j] if i != M.M64 and i not in now)
                kind = new[b][j][0]
                if kind == "momentum":
                    mom_orders_after += len(fresh)
                # (an order only the new parameters allow: the model's own record of what it placed is its list entry, whose
                #  volume is the member's trade_vol - 777 / 555 - or lies in the RandomAgents member's new vol_range)
                new_range[j] += len(fresh) if kind != "noise" or new[b][j][3]["trade_vol"] == 777 else 0
        run.submit(*thin_flow(rng, B, 3, 1))
        run.step()
        assert not env.flags().any(), (s, env.flags())
    print(f"width {width}: kept {kept}, cancelled from before {cancelled_old}, new-parameter orders {new_range}, "
          f"momentum non-zero at the retune in {mom_nonzero} books, {mom_orders_after} momentum limit orders after it")
    j_noise = 0 if width == 2 else 1
    assert kept[j_noise] > 0 and cancelled_old[j_noise] > 0 and new_range[j_noise] > 0, (kept, cancelled_old, new_range)
    if width == 5:  # the RandomAgents member itself: an agent cancels the order it held from before the retune, others place anew
        assert cancelled_old[0] > 0 and new_range[0] > 0, (cancelled_old, new_range)
    assert mom_nonzero > 0 and mom_orders_after > 0, (mom_nonzero, mom_orders_after)  # (scale and order_ratio are in use)
    env.close()


def fed_groups(b, new):
    r = np.random.default_rng((7500 if new else 6500) + b)
    lo = int(r.integers(900, 940)) if new else int(r.integers(30, 40))
    return [("random", 12, (lo, lo + 30), (500, 520) if new else (10, 20), 2 if new else 1, 0.95 if new else 0.9),
            ("random", 9, (lo + 3, lo + 4), (1, 2), 1, float(r.uniform(0.3, 0.8))),
            ("random", 5, (lo, lo + 60), (3, 9), 3 if new else 1, 1.0)]


def test_update_agents_after_a_retune_equals_the_model(bk, torch):
    """RandomAgents groups through bk_update_agents, fed mode: the model's view is the device book's order statuses; the
    generator and the appended orders stay the model's after the groups' attributes were assigned and the env retuned -
    which they can only do if the held ids survived (an agent holding an Active order cancels it and draws nothing more)"""
    from ingress_support import SEED as ISEED, STEP as ISTEP, ingress_env

    B, T, k = 33, 9, 4
    mask = np.zeros(B, dtype=np.uint8)
    mask[[0, 3, 7, 8, 20, 31, 32]] = 1
    old = [fed_groups(b, False) for b in range(B)]
    new = [fed_groups(b, True) if mask[b] else old[b] for b in range(B)]
    n_agents = sum(g[1] for g in old[0])
    env = ingress_env(bk, torch, B, T, 128, n_agents, 2 * n_agents + 8, tick=1)
    env.set_random_agents_per_book([[g[1:] for g in row] for row in old])
    models, rngs = [M.AgentSet(old[b]) for b in range(B)], [M.Rng(seed=ISEED + b) for b in range(B)]
    cancelled_old = new_range = 0
    for s in range(T):
        if s == k:
            env.sync()
            ids_at_retune = [len(env.orders(b)) for b in range(B)]
            for b in np.flatnonzero(mask):
                for member, m in zip(models[b].members, new[b]):
                    assign(member, m)
            status_d = torch.full((B, 2), 99, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            env.retune_random_agents(raw(torch, group_table(bk, [[g[1:] for g in row] for row in new])), dev(torch, mask), status_d)
            assert status_d.cpu().numpy().tolist() == [[0, 0]] * B
        env.sync()
        before = [env.orders(b) for b in range(B)]
        env.update_agents()
        queued = []
        for b in range(B):
            o = before[b]
            status, n0 = o["status"], len(o)
            view = M.BookView(lambda i, status=status: int(status[i]), 0, M.MAX_PRICE, n0, 1)
            models[b].update(view, rngs[b])
            assert env.rng_state(b) == rngs[b].state(), f"book {b}, step {s}: rng after the update"
            created = env.orders(b)[n0:]
            fresh = [e for e in view.events if e[0] == "new"]
            assert len(created) == len(fresh), f"book {b}, step {s}: {len(created)} orders appended vs {len(fresh)}"
            for o1, e in zip(created, fresh):
                got = tuple(int(o1[f]) for f in ("order_id", "side", "price", "vol", "trader_id", "arr_time", "status"))
                assert got == (e[1], e[2], e[5], e[3], e[4], s * ISTEP, M.NEW), f"book {b}, step {s}: order {got} vs {e}"
            if s >= k and mask[b]:  # (the conditions, from the model's events)
                cancelled_old += sum(1 for e in view.events if e[0] == "cancel" and e[1] < ids_at_retune[b])
                new_range += sum(1 for e in fresh if e[3] >= 500)
            queued.append(len(view.events))
        env.step()
        for b in range(B):
            rngs[b].shuffle(list(range(queued[b])))
            assert env.rng_state(b) == rngs[b].state(), f"book {b}, step {s}: rng after the step's shuffle"
        assert not env.flags().any(), (s, env.flags())
    assert cancelled_old > 0 and new_range > 0, (cancelled_old, new_range)
    assert int(env.trade_counts().sum()) > 0
    env.close()


# ------------------------------------------------------------------ 3. bk_run with trading off against the model
REST_B, REST_SEED, REST_STEP = 33, 101, 1_000_000


def rest_members(b, new):
    r = np.random.default_rng((950 if new else 900) + b)
    return [("noise", 0, 70, dict(NOISE, tick_size=1, p_limit=float(np.float32(r.uniform(0.7, 0.95))), p_cancel=0.5 if new else 0.3,
                                  trade_vol=321 if new else 100, price_dist_mu=float(r.uniform(2.0, 4.0)),
                                  price_dist_sigma=float(r.uniform(0.5, 2.0)))),
            ("momentum", 100, 20, dict(MOM, tick_size=1, demand=float(r.uniform(20.0, 60.0)), decay=float(r.uniform(0.3, 1.0)),
                                       p_cancel=0.3, trade_vol=123 if new else 100, price_dist_mu=float(r.uniform(0.0, 1.0)),
                                       price_dist_sigma=float(r.uniform(1.0, 4.0))))]


def rest_groups(b, new):
    r = np.random.default_rng((850 if new else 800) + b)
    lo = int(r.integers(2000, 2100)) if new else int(r.integers(20, 60))
    return [("random", 50, (lo, lo + 40), (700, 720) if new else (10, 20), 3 if new else 1, float(r.uniform(0.5, 0.9))),
            ("random", 30, (lo + 5, lo + 6), (1, 2), 1, 1.0 if new else 0.4)]


REST_MASK = np.zeros(REST_B, dtype=np.uint8)
REST_MASK[[0, 1, 7, 8, 15, 16, 32]] = 1


class GroupsBook(M.RestingBook):
    """RandomAgents never look at the touch, and with trading off their bids and asks cross: the view is given an empty one"""

    def touch(self):
        return 0, M.MAX_PRICE


def resting_model(rows_of, k, n):
    books = []
    for b in range(REST_B):
        book = (GroupsBook if rows_of is rest_groups else M.RestingBook)(REST_SEED + b, 0, 1, REST_STEP)
        agents = M.AgentSet(rows_of(b, False))
        for s in range(n):
            if s == k and REST_MASK[b]:
                book.ids_at_retune = len(book.orders)
                book.live_at_retune = sum(1 for o in book.orders if o[4] == M.ACTIVE)
                for member, m in zip(agents.members, rows_of(b, True)):
                    assign(member, m)
            book.update(agents)
            book.step()
        books.append(book)
    return books


@pytest.fixture(scope="module")
def rest_models():
    return {"members": resting_model(rest_members, 3, 6), "groups": resting_model(rest_groups, 3, 6)}


@pytest.mark.parametrize("kind,pipeline", [("members", "fused"), ("members", "split_wave"), ("groups", "split"), ("groups", "wave")])
def test_run_after_a_retune_with_trading_off_equals_the_model(bk, torch, rest_models, kind, pipeline):
    books = rest_models[kind]
    # the conditions on the model: the masked books held orders at the retune, and orders only the new parameters allow follow
    new_vols = (321, 123) if kind == "members" else tuple(range(700, 720))
    for b in np.flatnonzero(REST_MASK):
        assert books[b].live_at_retune > 0
        assert any(o[2] in new_vols for o in books[b].orders[books[b].ids_at_retune:]), b
    env = bk.ManyBookEnv(REST_B, REST_SEED, 0, 1, REST_STEP, True, levels=10, max_live_orders=512, trade_capacity=64, history_capacity=6)
    rows_of = rest_members if kind == "members" else rest_groups
    old = [rows_of(b, False) for b in range(REST_B)]
    new = [rows_of(b, REST_MASK[b]) for b in range(REST_B)]
    if kind == "members":
        env.set_agents_per_book(old)
    else:
        env.set_random_agents_per_book([[g[1:] for g in row] for row in old])
    env.disable_trading()
    env.set_pipeline(pipeline)
    env.run(3)
    if kind == "members":
        env.retune_agents(raw(torch, member_table(new)), dev(torch, REST_MASK))
    else:
        env.retune_random_agents(raw(torch, group_table(bk, [[g[1:] for g in row] for row in new])), dev(torch, REST_MASK))
    env.run(3)
    assert not env.flags().any(), env.flags()
    assert env.retune_rejected() == 0 and int(env.trade_counts().sum()) == 0
    hist = env.history()
    for b, book in enumerate(books):
        assert env.rng_state(b) == book.rng.state(), f"book {b}: rng {env.rng_state(b)} vs {book.rng.state()}"
        live = env.live_orders(b)
        for side in (M.BID, M.ASK):
            mine = live[live["side"] == side]
            got = list(zip(mine["order_id"].tolist(), mine["price"].tolist(), mine["vol"].tolist()))
            assert got == book.live(side), f"book {b}, side {side}: live (id, price, vol) differ"
        got = [tuple(int(x) for x in hist[s, b, 1:5]) for s in range(6)]
        assert got == book.history, f"book {b}: (bid, ask, ask vol, bid vol) per step {got} vs {book.history}"
    env.close()


# ------------------------------------------------------------------ 4. the oracle's one in-place assignment, trading on
NOISE_NEW = dict(p_limit=0.85, p_market=0.3, p_cancel=0.45)


def noise_retuned(rows, mask):
    return [[("noise", row[0][1], row[0][2], dict(row[0][3], **NOISE_NEW)), row[1]] if mask[b] else row for b, row in enumerate(rows)]


def test_set_noise_prob_under_run_equals_the_oracle(bk, torch, oracle):
    B, T, k = 33, 14, 6
    rows = member_rows(B, 61)
    mask = np.zeros(B, dtype=np.uint8)
    mask[[0, 7, 8, 9, 30, 32]] = 1
    new = noise_retuned(rows, mask)
    env = bk.ManyBookEnv(B, SEED, 0, 2, STEP, True, levels=LEVELS, max_live_orders=512, trade_capacity=8192, history_capacity=T)
    env.set_agents_per_book(rows)
    env.run(k)
    env.retune_agents(raw(torch, member_table(new)), dev(torch, mask))
    env.run(T - k)
    P.no_flags(env)
    hist = env.history()
    changed = 0
    for b in range(B):
        ref, ag = oracle.StepEnv(SEED + b, 0, 2, STEP, True, LEVELS), oracle.AgentSet(rows[b])
        st = oracle.sim_runner(ref, ag, SEED + b, k)
        if mask[b]:
            for which, v in NOISE_NEW.items():
                ag.set_noise_prob(0, which, v)
        st = oracle.sim_runner(ref, ag, 0, T - k, rng_state=st)
        P.same_history(hist[:, b], ref.history(), f"L2 history of book {b}")
        P.same_book(env, b, ref.book)
        assert env.rng_state(b) == tuple(int(x) for x in st), b
        if mask[b]:  # ... and the assignment shows: the untouched set runs differently
            ref0, ag0 = oracle.StepEnv(SEED + b, 0, 2, STEP, True, LEVELS), oracle.AgentSet(rows[b])
            oracle.sim_runner(ref0, ag0, SEED + b, T)
            changed += not np.array_equal(ref0.history(), ref.history())
    assert changed == int(mask.sum())
    env.close()


def test_set_noise_prob_on_the_ingress_path_equals_the_oracle(bk, torch, oracle):
    from ingress_support import SEED as ISEED, STEP as ISTEP, check

    B, T, k = 33, 10, 4
    rows = member_rows(B, 62, n_noise=16, n_mom=8)
    mask = np.zeros(B, dtype=np.uint8)
    mask[[0, 7, 8, 9, 30, 32]] = 1
    new = noise_retuned(rows, mask)
    env = members_env(bk, torch, B, T, 256, rows[0], 2)
    env.set_agents_per_book(rows)
    refs = [oracle.StepEnv(ISEED + b, 0, 2, ISTEP) for b in range(B)]
    agents = [oracle.AgentSet(rows[b]) for b in range(B)]
    for s in range(T):
        if s == k:
            env.retune_agents(raw(torch, member_table(new)), dev(torch, mask), sync=False)
            for b in np.flatnonzero(mask):
                for which, v in NOISE_NEW.items():
                    agents[b].set_noise_prob(0, which, v)
        env.update_members()
        env.step()
        for b in range(B):
            agents[b].update(refs[b])
            refs[b].step()
    check(env, refs)
    for b in range(B):
        for j in range(2):
            assert [int(i) for i in env.member_orders(b, j)] == [int(i) for i in agents[b].order_list(j)], (b, j)
    env.close()


# ------------------------------------------------------------------ 5. cross-path, trading on
def test_run_and_update_agents_agree_after_the_same_retune(bk, torch):
    from ingress_support import SEED as ISEED, STEP as ISTEP, ingress_env

    B, T, k = 33, 14, 6
    t, t2 = group_rows(B, 51), group_rows(B, 52)
    mask = np.zeros(B, dtype=np.uint8)
    mask[[0, 1, 8, 17, 31, 32]] = 1
    tab2, mask_d = raw(torch, group_table(bk, t2)), dev(torch, mask)
    run_env = bk.ManyBookEnv(B, ISEED, 0, 2, ISTEP, True, levels=10, max_live_orders=128, trade_capacity=8192, history_capacity=T)
    run_env.set_random_agents_per_book(t)
    run_env.run(k)
    run_env.retune_random_agents(tab2, mask_d)
    run_env.run(T - k)
    ing = ingress_env(bk, torch, B, T, 128, sum(SIZES), 2 * sum(SIZES) + 8)
    ing.set_random_agents_per_book(t)
    for s in range(T):
        if s == k:
            ing.retune_random_agents(tab2, mask_d, sync=False)
        ing.update_agents()
        ing.step()
    ing.sync()
    P.no_flags(run_env)
    P.no_flags(ing)
    assert int(run_env.trade_counts().sum()) > 0
    P.same_history(ing.history(), run_env.history())
    P.same_array(ing.trade_counts(), run_env.trade_counts(), "books", "trade counts")
    for b in range(B):
        assert ing.rng_state(b) == run_env.rng_state(b), b
        P.same_records(ing.live_orders(b), run_env.live_orders(b), b, "live order")
    run_env.close()
    ing.close()


# ------------------------------------------------------------------ 6. refusals inside the kernel
def test_refusals_inside_the_kernel_groups(bk, torch):
    B = 33
    good = group_rows(B, 11)
    next_rows = group_rows(B, 12)
    inst = group_table(bk, good)
    tab = group_table(bk, next_rows)
    nan, inf = np.float32("nan"), np.float32("inf")
    bad = {  # unit -> (entry, field changes): one bad entry each, the failing index first, in the middle and last
        1: (0, dict(tick_hi=0)), 2: (1, dict(tick_lo=0)), 4: (2, dict(vol_hi=0)), 6: (1, dict(tick_size=3)),
        9: (2, dict(tick_size=2, tick_lo=1, tick_hi=0x80000001)), 12: (0, dict(n_agents=SIZES[0] + 1)),
        17: (2, dict(n_agents=0)), 20: (1, dict(tick_size=1)), 31: (0, dict(tick_lo=5, tick_hi=5)), 32: (2, dict(tick_size=7)),
    }
    fine = {  # not refused: the bound exactly one below, any rate
        3: (0, dict(tick_size=2, tick_lo=1, tick_hi=0x80000000)), 5: (1, dict(activity_rate=nan)), 7: (2, dict(activity_rate=inf)),
        8: (0, dict(activity_rate=np.float32(0.0))), 10: (1, dict(activity_rate=np.float32(1.5))),
    }
    for u, (j, ch) in {**bad, **fine}.items():
        for k, v in ch.items():
            tab[u, j][k] = v
    mask = np.ones(B, dtype=np.uint8)
    mask[[13, 14, 32]] = 0  # (unit 32 is bad but unmasked: not read, not counted)
    as_rows = lambda t: [[tuple(t[u, j].tolist()) for j in range(t.shape[1])] for u in range(t.shape[0])]  # noqa: E731
    want_table, want_status, want_refused = RM.retune_groups(as_rows(inst), as_rows(tab), mask, [2])
    assert want_refused == len(bad) - 1 and [u for u, s in enumerate(want_status) if s[0]] == sorted(set(bad) - {32})
    assert {want_status[u] for u in (6, 20)} == {(RM.NOT_TICK_MULTIPLE, 1)}

    env = book_env(bk, B)
    env.set_random_agents_per_book(inst)
    env.run(K)
    status = torch.full((B, 2), 99, dtype=torch.int32, device="cuda")
    env.retune_random_agents(raw(torch, tab), dev(torch, mask), status)
    assert [tuple(x) for x in status.cpu().numpy().tolist()] == want_status
    assert env.retune_rejected() == want_refused
    env.run(N - K)
    got = P.snapshot(env)
    env.close()
    # the control: installed rows to step K, then the model's table (refused and unmasked units keep theirs) by a fresh install path
    ctl = book_env(bk, B)
    ctl.set_random_agents_per_book(inst)
    ctl.run(N)
    control = P.snapshot(ctl)
    ctl.close()
    applied = [u for u in range(B) if mask[u] and not want_status[u][0]]
    for u in range(B):
        if u in applied:
            assert differs(got, control, u), f"unit {u} was applied and runs as before"
        else:  # byte-identical records: the run equals the control for exactly these books
            assert np.array_equal(got["history"][:, u], control["history"][:, u]) and got["rng"][u] == control["rng"][u], u
            P.same_records(got["live"][u], control["live"][u], u, "live order")
    # the applied units run as an env retuned by the host entry with the model's table does (install T, retune on the host)
    host = book_env(bk, B)
    host.set_random_agents_per_book(inst)
    host.run(K)
    t_ok = np.array([[tuple(x) for x in row] for row in want_table], dtype=bk.RANDOM_AGENTS_DTYPE)
    host.retune_random_agents(t_ok)
    host.run(N - K)
    P.assert_same(got, P.snapshot(host))
    # the host entry with the bad table: the install's status, the unit and entry named, nothing changed
    with pytest.raises(bk.BourseError) as e:
        host.retune_random_agents(tab, mask)
    assert "unit 1, group 0" in str(e.value)
    with pytest.raises(ValueError) as e:  # (the install's status: BK_PRICE_NOT_TICK_MULTIPLE raises as the reference's PriceError)
        host.retune_random_agents(tab, (np.arange(B) == 6).astype(np.uint8))
    assert "unit 6, group 1" in str(e.value) and "multiple" in str(e.value)
    with pytest.raises(bk.BourseError) as e:
        host.retune_random_agents(tab, (np.arange(B) == 12).astype(np.uint8))
    assert "unit 12, group 0" in str(e.value) and "n_agents" in str(e.value)
    assert host.retune_rejected() == 0
    host.run(3)
    ref = book_env(bk, B)
    ref.set_random_agents_per_book(inst)
    ref.run(K)
    ref.retune_random_agents(t_ok)
    ref.run(N - K + 3)
    assert np.array_equal(host.history()[-3:], ref.history()[-3:]) and [host.rng_state(b) for b in range(B)] == [ref.rng_state(b) for b in range(B)]
    host.close()
    ref.close()


def test_refusals_inside_the_kernel_members(bk, torch):
    B = 33
    inst_rows, next_rows = member_rows(B, 21), member_rows(B, 22)
    inst, tab = member_table(inst_rows), member_table(next_rows)
    bad = {
        0: (0, dict(price_dist_sigma=-1.0)), 2: (1, dict(price_dist_sigma=float("nan"))), 5: (0, dict(price_dist_sigma=float("inf"))),
        7: (1, dict(price_dist_mu=float("inf"))), 8: (0, dict(tick_size=0)), 11: (1, dict(tick_size=3)), 15: (0, dict(type=2)),
        16: (1, dict(type=9)), 23: (0, dict(n_agents=41)), 24: (1, dict(agent_id_start=1001)), 32: (1, dict(n_agents=70000)),
    }
    fine = {1: (0, dict(price_dist_sigma=0.0)), 3: (1, dict(p_cancel=np.float32("nan"))), 4: (0, dict(p_limit=np.float32(1.5)))}
    for u, (j, ch) in {**bad, **fine}.items():
        for k, v in ch.items():
            tab[u, j][k] = v
    mask = np.ones(B, dtype=np.uint8)
    mask[[9, 10]] = 0
    as_rows = lambda t: [[{k: t[u, j][k].item() for k in t.dtype.names} for j in range(t.shape[1])] for u in range(t.shape[0])]  # noqa: E731
    _, want_status, want_refused = RM.retune_members(as_rows(inst), as_rows(tab), mask, [2])
    assert want_refused == len(bad) and [u for u, s in enumerate(want_status) if s[0]] == sorted(bad)
    assert want_status[11] == (RM.NOT_TICK_MULTIPLE, 1) and want_status[8] == (RM.NOT_TICK_MULTIPLE, 0)

    env = book_env(bk, B, pool=512)
    env.set_agents_per_book(inst_rows)
    env.run(K)
    status = torch.full((B, 2), 99, dtype=torch.int32, device="cuda")
    env.retune_agents(raw(torch, tab), dev(torch, mask), status)
    assert [tuple(x) for x in status.cpu().numpy().tolist()] == want_status
    assert env.retune_rejected() == want_refused
    env.retune_agents(raw(torch, tab), dev(torch, mask))  # status None is accepted; the counter is cumulative
    assert env.retune_rejected() == 2 * want_refused
    env.run(N - K)
    got = P.snapshot(env)
    env.close()
    ctl = book_env(bk, B, pool=512)
    ctl.set_agents_per_book(inst_rows)
    ctl.run(N)
    control = P.snapshot(ctl)
    applied = [u for u in range(B) if mask[u] and not want_status[u][0]]
    for u in range(B):
        if u in applied:
            assert differs(got, control, u), f"unit {u} was applied and runs as before"
        else:
            assert np.array_equal(got["history"][:, u], control["history"][:, u]) and got["rng"][u] == control["rng"][u], u
    with pytest.raises(bk.BourseError) as e:
        ctl.retune_agents(tab, mask)
    assert "unit 0, member 0" in str(e.value) and "LogNormal" in str(e.value)
    with pytest.raises(bk.BourseError) as e:
        ctl.retune_agents(tab, (np.arange(B) == 24).astype(np.uint8))
    assert "unit 24, member 1" in str(e.value) and "agent_id_start" in str(e.value)
    assert ctl.retune_rejected() == 0
    ctl.close()


# ------------------------------------------------------------------ 7. markets
def market_rows(nm, seed, ticks):
    r = np.random.default_rng(seed)
    A = len(ticks)
    rows = []
    for _ in range(nm):
        row = []
        for i, n in enumerate((40, 33, 20)):
            a = i % A
            tlo = int(r.integers(5, 60))
            row.append((a, n, (tlo, tlo + int(r.choice([1, int(r.integers(2, 300))]))), (1 + i, 9 + int(r.integers(0, 50))),
                        ticks[a] * int(r.integers(1, 4)), float(r.uniform(0.2, 0.9))))
        rows.append(row)
    return rows


def test_markets_random_agents(bk, torch, oracle):
    NM, ticks, T, k = 11, [2, 1, 4], 20, 7
    A = len(ticks)
    t0, t = market_rows(NM, 1, ticks), market_rows(NM, 2, ticks)
    mask = np.zeros(NM, dtype=np.uint8)
    mask[[0, 4, 10]] = 1
    t2 = [[(a, n, (tr[0] + 100, tr[1] + 150), vr, ts, 1.0) for a, n, tr, vr, ts, rate in row] for row in t]

    def make(first):
        env = bk.ManyMarketEnv(NM, SEED, 0, ticks, STEP, True, levels=LEVELS, max_live_orders=128, trade_capacity=4000, history_capacity=T)
        env.set_random_market_agents_per_market(first)
        return env

    strip = lambda rows: group_table(bk, [[g[1:] for g in row] for row in rows])  # noqa: E731
    # b (and a): installed with T0, retuned to T from the device, then T again from the host in the middle - against the oracle
    env = make(t0)
    env.retune_random_market_agents(raw(torch, strip(t)))
    env.run(k)
    env.retune_random_market_agents(t, mask)
    env.run(T - k)
    hist = env.history()
    P.no_flags(env)
    for m in range(NM):
        ref = oracle.ManyMarkets(1, SEED + m, 0, ticks, STEP, True, LEVELS, t[m])
        ref.run(T)
        assert np.array_equal(hist[:, m * A:(m + 1) * A], ref.history()), m
        assert env.rng_state(m * A) == tuple(int(x) for x in ref.rng_states()[0]), m
    # c. a mask per market: the unmasked markets are the oracle's, the masked ones differ from it after step k
    status = torch.full((NM, 2), 99, dtype=torch.int32, device="cuda")
    env2 = make(t)
    env2.run(k)
    env2.retune_random_market_agents(raw(torch, strip(t2)), dev(torch, mask), status)
    env2.run(T - k)
    assert status.cpu().numpy().tolist() == [[0, 0]] * NM and env2.retune_rejected() == 0
    h2 = env2.history()
    for m in range(NM):
        cols = slice(m * A, (m + 1) * A)
        assert np.array_equal(h2[:k, cols], hist[:k, cols]), m
        assert np.array_equal(h2[:, cols], hist[:, cols]) != bool(mask[m]), m
    # a bad row of a masked market: its tick_size is checked against ITS asset's tick (4 for asset 2)
    bad = strip(t2)
    bad[4, 2]["tick_size"] = 6
    env2.retune_random_market_agents(raw(torch, bad), dev(torch, mask), status)
    assert status.cpu().numpy().tolist()[4] == [RM.NOT_TICK_MULTIPLE, 2] and env2.retune_rejected() == 1
    env.close()
    env2.close()


class _Live:
    """the live orders a run left, answering as an env does for oracle_parity.same_live"""

    def __init__(self, live):
        self._live = live

    def live_orders(self, b):
        return self._live


def test_markets_random_agents_on_the_ingress_path(bk, torch):
    """a RandomMarketAgents table retuned and stepped through bk_update_market_agents: identities 1a - 1c against a control
    on the same path, and the control against bk_run's run of the same table (pinned by the oracle above)"""
    from ingress_support import SEED as ISEED, STEP as ISTEP
    from market_ingress_support import market_env

    NM, ticks, T, k = 11, [2, 1, 4], 12, 5
    A = len(ticks)
    t0, t = market_rows(NM, 5, ticks), market_rows(NM, 6, ticks)
    t2 = [[(a, n, (tr[0] + 100, tr[1] + 150), vr, ts, 1.0) for a, n, tr, vr, ts, rate in row] for row in t]
    mask = np.zeros(NM, dtype=np.uint8)
    mask[[0, 4, 10]] = 1
    strip = lambda rows: group_table(bk, [[g[1:] for g in row] for row in rows])  # noqa: E731

    def steps(env, n):
        for _ in range(n):
            env.update_market_agents()
            env.step()

    def run(first, at0=None, at_k=None):
        env = market_env(bk, torch, NM, ticks, T, 128, 256, 200 * T)
        env.set_random_market_agents_per_market(first)
        if at0:
            at0(env)
        steps(env, k)
        if at_k:
            at_k(env)
        steps(env, T - k)
        env.sync()
        P.no_flags(env)
        out = (env.history(), [env.rng_state(b) for b in range(env.n_books)], [env.live_orders(b) for b in range(env.n_books)],
               env.trade_counts())
        env.close()
        return out

    def same(x, y, markets):
        for m in markets:
            cols = slice(m * A, (m + 1) * A)
            P.same_history(x[0][:, cols], y[0][:, cols], f"L2 history of market {m}")
            assert x[1][m * A] == y[1][m * A], m
            for b in range(m * A, (m + 1) * A):
                P.same_records(x[2][b], y[2][b], b, "live order")

    control = run(t)
    assert int(control[3].sum()) > 0
    # the control is bk_run's run of the same table
    ref = bk.ManyMarketEnv(NM, ISEED, 0, ticks, ISTEP, True, levels=LEVELS, max_live_orders=128, trade_capacity=4000, history_capacity=T)
    ref.set_random_market_agents_per_market(t)
    ref.run(T)
    P.same_history(control[0], ref.history())
    assert control[1] == [ref.rng_state(b) for b in range(ref.n_books)]
    ref.close()
    # a. the installed rows again in the middle of the run; b. T0 retuned to T before the first update (device, host)
    same(control, run(t, at_k=lambda e: e.retune_random_market_agents(raw(torch, strip(t)), dev(torch, mask), sync=False)), range(NM))
    same(control, run(t0, at0=lambda e: e.retune_random_market_agents(raw(torch, strip(t)), sync=False)), range(NM))
    same(control, run(t0, at0=lambda e: e.retune_random_market_agents(t)), range(NM))
    # c. a mask per market at step k: the unmasked markets equal the control bit for bit, the masked ones differ after step k
    got = run(t, at_k=lambda e: e.retune_random_market_agents(raw(torch, strip(t2)), dev(torch, mask), sync=False))
    same(control, got, np.flatnonzero(mask == 0))
    for m in np.flatnonzero(mask):
        cols = slice(m * A, (m + 1) * A)
        assert np.array_equal(got[0][:k, cols], control[0][:k, cols]), m
        assert not np.array_equal(got[0][k:, cols], control[0][k:, cols]) and got[1][m * A] != control[1][m * A], m


def market_member_rows(nm, seed):
    r = np.random.default_rng(seed)
    return [[(0, ("random", 30, (20, 60), (10, 20), 2, float(r.uniform(0.5, 0.9)))),
             (2, ("noise", 100, 12, dict(NOISE, tick_size=4, p_limit=float(np.float32(r.uniform(0.2, 0.6))),
                                         price_dist_mu=float(r.uniform(0.0, 1.0))))),
             (1, ("momentum", 200, 8, dict(MOM, tick_size=1, demand=float(r.uniform(5.0, 30.0)), decay=float(r.uniform(0.3, 1.0)))))]
            for _ in range(nm)]


def test_markets_members(bk, torch, oracle):
    """retune_market_agents: identities 1a - 1c under bk_run with the control held against oracle.ManyMarkets(members=...),
    market by market, and the same identities on the ingress path (update_market_members + step) against a control"""
    from market_ingress_support import market_env

    NM, ticks, T, k = 11, [2, 1, 4], 12, 5
    t0, t, t2 = market_member_rows(NM, 1), market_member_rows(NM, 2), market_member_rows(NM, 3)
    mask = np.zeros(NM, dtype=np.uint8)
    mask[[0, 4, 10]] = 1
    strip = lambda rows: member_table([[m for _, m in r] for r in rows])  # noqa: E731

    def run(first, *then, ingress=False):
        if ingress:
            env = market_env(bk, torch, NM, ticks, T, 128, 256, 200 * T)
        else:
            env = bk.ManyMarketEnv(NM, SEED, 0, ticks, STEP, True, levels=LEVELS, max_live_orders=128, trade_capacity=4000, history_capacity=T)
        env.set_market_agents_per_market(first)
        for f in then:
            f(env)
        env.sync()
        P.no_flags(env)
        out = (env.history(), [env.rng_state(b) for b in range(env.n_books)], [env.live_orders(b) for b in range(env.n_books)])
        env.close()
        return out

    def steps(n):
        def go(env):
            for _ in range(n):
                env.update_market_members()
                env.step()
        return go

    for ingress, adv in ((False, lambda n: (lambda e: e.run(n))), (True, steps)):
        control = run(t, adv(k), adv(T - k), ingress=ingress)
        if not ingress:  # what the identities below are held against is the oracle's run of every market's own row
            for m in range(NM):
                ref = oracle.ManyMarkets(1, SEED + m, 0, ticks, STEP, True, LEVELS, members=t[m])
                ref.run(T)
                P.same_history(control[0][:, 3 * m:3 * m + 3], ref.history(), f"L2 history of market {m}")
                assert control[1][3 * m] == tuple(int(x) for x in ref.rng_states()[0]), m
                for a in range(3):
                    P.same_live(_Live(control[2][3 * m + a]), 0, ref.book(0, a), tag=(m, a))
        # a, b. the installed rows again change nothing; T0 retuned to T equals T installed (device and host entry)
        same = run(t, adv(k), lambda e: e.retune_market_agents(raw(torch, strip(t)), dev(torch, mask)), adv(T - k), ingress=ingress)
        on_dev = run(t0, lambda e: e.retune_market_agents(raw(torch, strip(t))), adv(k), adv(T - k), ingress=ingress)
        on_host = run(t0, lambda e: e.retune_market_agents(t), adv(k), adv(T - k), ingress=ingress)
        for got in (same, on_dev, on_host):
            assert np.array_equal(got[0], control[0]) and got[1] == control[1]
            for x, y in zip(got[2], control[2]):
                P.same_records(x, y, "book", "live order")
        # c. a mask per market
        got = run(t, adv(k), lambda e: e.retune_market_agents(raw(torch, strip(t2)), dev(torch, mask)), adv(T - k), ingress=ingress)
        for m in range(NM):
            cols = slice(3 * m, 3 * m + 3)
            assert np.array_equal(got[0][:k, cols], control[0][:k, cols]), m
            same_m = np.array_equal(got[0][:, cols], control[0][:, cols]) and got[1][3 * m] == control[1][3 * m]
            assert same_m != bool(mask[m]), (ingress, m)


# ------------------------------------------------------------------ 8. with the reset, and across a checkpoint
def test_masked_reset_and_retune_in_one_stream_order(bk, torch):
    B = 33
    t, t2 = group_rows(B, 31), group_rows(B, 32)
    mask = np.zeros(B, dtype=np.uint8)
    mask[[0, 8, 9, 32]] = 1
    seeds = (np.arange(B, dtype=np.uint64) + 9000)
    mixed = [t2[b] if mask[b] else t[b] for b in range(B)]
    stream = torch.cuda.current_stream().cuda_stream
    env = book_env(bk, B, stream=stream)
    env.set_random_agents_per_book(t)
    env.run(4)
    env.save_snapshot(0)
    env.run(K)
    # mask, seeds and rows are written on the env's stream; reset + retune + run with no host call in between
    mask_d, seeds_d = torch.from_numpy(mask).cuda(), torch.from_numpy(seeds.view(np.int64)).cuda()
    rows_d = torch.from_numpy(group_table(bk, t2).view(np.int32).reshape(B, len(SIZES), 7).copy()).cuda()
    env.reset_books(mask_d, seeds_d, slot=0, sync=False)
    env.retune_random_agents(rows_d, mask_d, sync=False)
    env.run(5, sync=False)
    env.sync()
    assert env.retune_rejected() == 0
    # the expected side: the new table installed before the snapshot was taken, reset the same way
    ref = book_env(bk, B, stream=stream)
    ref.set_random_agents_per_book(t)
    ref.run(4)
    ref.set_random_agents_per_book(mixed)
    ref.save_snapshot(0)
    ref.run(K)
    ref.reset_books(mask, seeds, slot=0)
    ref.run(5)
    h, hr = env.history(), ref.history()
    for b in range(B):
        assert np.array_equal(h[-5:, b], hr[-5:, b]), b
        assert env.rng_state(b) == ref.rng_state(b), b
        P.same_records(env.live_orders(b), ref.live_orders(b), b, "live order")
    # the slot taken before the retune is still accepted after it
    env.reset_books(mask_d, None, slot=0)
    # a checkpoint saved before a retune restores after it; the restore brings no parameters back
    cp = book_env(bk, B)
    cp.set_random_agents_per_book(t)
    cp.run(4)
    buf = cp.checkpoint()
    cp.retune_random_agents(t2, mask)
    cp.run(3)
    cp.restore(buf)
    cp.run(3)
    cp2 = book_env(bk, B)
    cp2.set_random_agents_per_book(t)
    cp2.run(4)
    cp2.retune_random_agents(t2, mask)
    cp2.run(3)
    assert [cp.rng_state(b) for b in range(B)] == [cp2.rng_state(b) for b in range(B)]
    assert np.array_equal(cp.history()[-3:], cp2.history()[-3:])
    # conversely a checkpoint taken AFTER a retune restores into an env that repeats the original install, and the retuned
    # parameters come back only with a second retune
    buf2 = cp2.checkpoint()
    cp3 = book_env(bk, B)
    cp3.set_random_agents_per_book(t)
    cp3.restore(buf2)
    cp3.retune_random_agents(t2, mask)
    cp3.run(2)
    cp2.run(2)
    assert [cp3.rng_state(b) for b in range(B)] == [cp2.rng_state(b) for b in range(B)]
    assert np.array_equal(cp3.history()[-2:], cp2.history()[-2:])
    for c in (env, ref, cp, cp2, cp3):
        c.close()


def test_ingress_reset_and_retune_in_one_stream_order(bk, torch):
    """the same on a device-ingress env: the ingress slot saved before a retune is accepted after it (a retune is no
    install), and reset + retune run in one stream order; the expected side is retuned by the host entry before its
    snapshot is taken (host and device entries against the installs: the identities above)"""
    from ingress_support import ingress_env

    B, T = 33, 10
    t, t2 = group_rows(B, 71), group_rows(B, 72)
    mask = np.zeros(B, dtype=np.uint8)
    mask[[0, 8, 9, 32]] = 1
    seeds = np.arange(B, dtype=np.uint64) + 4000
    mixed = [t2[b] if mask[b] else t[b] for b in range(B)]

    def steps(env, n):
        for _ in range(n):
            env.update_agents(sync=False)
            env.step()

    env = ingress_env(bk, torch, B, T, 128, sum(SIZES), 2 * sum(SIZES) + 8)
    env.set_random_agents_per_book(t)
    steps(env, 3)
    env.save_ingress_snapshot(0)
    steps(env, 2)
    mask_d, seeds_d = torch.from_numpy(mask).cuda(), torch.from_numpy(seeds.view(np.int64)).cuda()
    rows_d = torch.from_numpy(group_table(bk, t2).view(np.int32).reshape(B, len(SIZES), 7).copy()).cuda()
    env.retune_random_agents(rows_d, mask_d, sync=False)
    env.reset_ingress_books(mask_d, seeds_d, slot=0, sync=False)  # the slot is older than the retune
    steps(env, 4)
    ref = ingress_env(bk, torch, B, T, 128, sum(SIZES), 2 * sum(SIZES) + 8)
    ref.set_random_agents_per_book(t)
    steps(ref, 3)
    ref.retune_random_agents(mixed)
    ref.save_ingress_snapshot(0)
    steps(ref, 2)
    ref.reset_ingress_books(mask, seeds, slot=0)
    steps(ref, 4)
    env.sync()
    ref.sync()
    assert env.retune_rejected() == 0
    h, hr = env.history(), ref.history()
    for b in range(B):
        rows = slice(-4, None) if mask[b] else slice(0, 5)  # (an unmasked book of `ref` ran steps 3, 4 with its own rows too)
        assert np.array_equal(h[rows, b], hr[rows, b]), b
        if mask[b]:
            assert env.rng_state(b) == ref.rng_state(b), b
            P.same_records(env.live_orders(b), ref.live_orders(b), b, "live order")
    for b in np.flatnonzero(mask == 0):
        assert np.array_equal(h[:, b], hr[:, b]) and env.rng_state(b) == ref.rng_state(b), b
    env.close()
    ref.close()


# ------------------------------------------------------------------ 8b. the host entry's staging, made and then grown
def test_host_and_device_entries_agree_as_the_table_widens(bk, torch):
    """Two envs of one seed, retuned with the same rows - one through the host entry, one through the device entry - for a
    one-group table and then, installed again, for a two-group one: the host entry's staging is made by the first retune and
    replaced by a larger one at the second, and both times the kernel reads from it what the device entry is handed."""
    B = 4
    narrow = (group_rows(B, 11, sizes=(20,)), group_rows(B, 12, sizes=(20,)))
    wide = (group_rows(B, 13, sizes=(20, 15)), group_rows(B, 14, sizes=(20, 15)))
    host, device, control = (book_env(bk, B=B, pool=64) for _ in range(3))
    for installed, rows in (narrow, wide):
        tab = group_table(bk, rows)
        for env in (host, device, control):
            env.set_random_agents_per_book(installed)
        host.retune_random_agents(tab)
        device.retune_random_agents(raw(torch, tab))
    for env in (host, device, control):
        env.run(3)
    assert host.retune_rejected() == 0 and device.retune_rejected() == 0
    assert np.array_equal(host.level2(), device.level2())
    assert [host.rng_state(b) for b in range(B)] == [device.rng_state(b) for b in range(B)]
    assert not np.array_equal(host.level2(), control.level2())  # (the retunes took effect: `control` runs the installed rows)
    for env in (host, device, control):
        env.close()


# ------------------------------------------------------------------ 9. no wait on the device path
def test_device_entries_return_with_work_queued(bk, torch):
    B = 4096
    rows = [[(100, (20, 60), (10, 20), 2, 0.9)]] * B
    env = bk.ManyBookEnv(B, SEED, 0, 2, STEP, True, levels=LEVELS, max_live_orders=128, trade_capacity=64, history_capacity=1,
                         stream=torch.cuda.current_stream().cuda_stream)
    env.set_random_agents_per_book(rows)
    env.disable_trading()
    tab = raw(torch, group_table(bk, rows))
    env.retune_random_agents(tab)  # the first call makes the counter
    env.run(1)
    env.run(1000, sync=False)  # a long launch in front
    env.retune_random_agents(tab, None, None, sync=False)  # mask None: every unit; status None is accepted
    done = torch.cuda.Event()
    done.record()  # on the env's stream, behind the retune
    assert not done.query(), "the retune waited for the run queued in front of it"
    env.sync()
    assert done.query() and env.retune_rejected() == 0
    env.close()


# ------------------------------------------------------------------ 10. the API's refusals
def test_api_refusals(bk, torch):
    B = 33
    rows = group_rows(B, 41)
    tab = group_table(bk, rows)
    env = book_env(bk, B)
    with pytest.raises(bk.BourseError, match="per-unit table"):
        env.retune_random_agents(rows)  # nothing installed
    env.set_random_agents(rows[0])
    with pytest.raises(bk.BourseError, match="bk_set_random_agents_per_book"):
        env.retune_random_agents(rows)  # a uniform install
    with pytest.raises(bk.BourseError, match="bk_set_random_agents_per_book"):
        env.retune_random_agents(raw(torch, tab))
    env.set_random_agents_per_book(rows)
    with pytest.raises(bk.BourseError, match="n_groups"):
        env.retune_random_agents(tab[:, :2])  # a width mismatch
    with pytest.raises(bk.BourseError, match="n_groups"):
        env.retune_random_agents(raw(torch, tab[:, :2]))
    with pytest.raises(bk.BourseError):
        env.retune_agents(member_rows(B, 1))  # the wrong kind of table
    with pytest.raises(ValueError):
        env.retune_random_agents(raw(torch, tab), np.ones(B, dtype=np.uint8))  # a host mask with a device table
    with pytest.raises(ValueError):
        env.retune_random_agents(tab, dev(torch, np.ones(B, dtype=np.uint8)))
    with pytest.raises(ValueError):
        env.retune_random_agents(raw(torch, tab), None, np.zeros((B, 2), dtype=np.uint32))
    with pytest.raises(ValueError):
        env.retune_random_agents(raw(torch, tab), dev(torch, np.ones(B + 1, dtype=np.uint8)))
    assert env.retune_rejected() == 0
    env.set_agents(member_rows(1, 1)[0])
    with pytest.raises(bk.BourseError, match="bk_set_agents_per_book"):
        env.retune_agents(member_rows(B, 1))  # a uniform members install
    env.set_agents_per_book(member_rows(B, 1))
    with pytest.raises(bk.BourseError):
        env.retune_random_agents(rows)
    env.retune_agents(member_rows(B, 2))
    env.close()
