"""What the device-ingress tests with on-device agents share: the env they build, how one step's instructions reach the
device and the oracle, and the comparison of every book with its own oracle.StepEnv (tests/oracle_parity.py)."""
import numpy as np

import oracle_parity as P

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
