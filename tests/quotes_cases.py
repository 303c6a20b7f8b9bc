"""What the quote tests share (tests/test_quotes_cpu.py without a GPU, tests/test_gpu_quotes.py on one): the expected side of a
run with bk_submit_quotes in it, made before the device sees anything, and the busy flow with the conditions it must meet.

The expected side is one oracle.StepEnv(SEED + b) per book.  A step is: the background instructions (ingress_support's
format), then the grid tests/quotes_model.py::expand makes from open_orders_model.rows_ints over the oracle's orders_array()
and the step's quote table, both through ingress_support.apply_oracle, then step().  A step's quotes name ids that rest on the
expected side, so it runs first; what happened is counted while it runs."""
import numpy as np
import pytest

import open_orders_model as OM
import oracle_parity as P
import quotes_model as QM
from ingress_support import SEED, STEP, apply_oracle, dev, submit, thin_flow

KEEP = QM.KEEP
NO_ID = 0xFFFFFFFFFFFFFFFF
WORDS = ("cancel", "reduce", "topup", "fresh", "untouched", "keep_side", "pulled_side")


# grid positions as literal tuples (action, side, vol, trader, price, order_id), for the grids worked out by hand
O = (0, 0, 0, 0, 0, 0)  # a position with nothing in it


def cancel(t, oid):
    return (2, 0, 0, t, 0, oid)


def reduce(t, oid, vol):
    return (QM.MOD, 4, vol, t, 0, oid)


def new(t, bid, price, vol):
    return (1, bid, vol, t, price, 0)


def grid_rows(entries, quotes, depth):
    g = QM.expand(entries, quotes, depth)
    return [tuple(int(g[k][i]) for k in range(6)) for i in range(len(g[0]))]


def join(grids):
    """per-book grids as one batch: (book_offsets, the six arrays)"""
    off = np.zeros(len(grids) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(g[0]) for g in grids])
    return off, tuple(np.concatenate([g[k] for g in grids]) for k in range(6))


class QuotePlan:
    def __init__(self, oracle, B, tick, n_traders, depth, seed=SEED):
        self.B, self.tick, self.NT, self.depth, self.G = B, tick, n_traders, depth, depth + 2
        self.refs = [oracle.StepEnv(seed + b, 0, tick, STEP) for b in range(B)]
        self.steps = []  # (background (off, ins) or None, quotes [B, NT, 4] u32, grid (off, ins), expected out_ids [B, NT, 2] u64)
        self.count = {w: 0 for w in WORDS}  # what the quotes did (quotes_model's words), over all books and steps, and:
        self.partial_keepers = 0    # keepers that had traded before the call that kept them
        self.beyond_depth = 0       # traders resting more than `depth` orders at a call that touches them ...
        self.unlisted_stay = 0      # ... whose unlisted orders are Active after the call's events were queued and the step ran
        self.most_live_positions = 0  # most grid positions of one book with an action in one call
        self.most_resting = 0       # most resting orders of one trader with a row
        self.most_live = 0          # most Active orders of one book
        self.rows_after = []        # open_orders_model.rows of every book after each step, stacked as env.open_orders() gives them

    def entries(self):
        return [OM.rows_ints(r.book.orders_array(), self.NT, self.depth)[1] for r in self.refs]

    def expected_ids(self, b, grid):
        """the ids book b's grid creates, as out_ids_dev [NT, 2] holds them: dense in element order from the book's next id"""
        out = np.full((self.NT, 2), NO_ID, dtype=np.uint64)
        next_id = self.refs[b].book.n_orders()
        for i in np.nonzero(grid[0] == 1)[0]:
            t, at = divmod(int(i), self.G)
            out[t, at - self.depth] = next_id
            next_id += 1
        return out

    def step(self, quotes, background=None, run=True, before=None, after=None):
        """one call with `quotes` behind `background`; before(b, ref) / after(b, ref) queue what else the step holds in front of
        both / behind the quotes; run = False leaves the step to the caller (more calls follow)"""
        quotes = np.ascontiguousarray(quotes, dtype=np.uint32).reshape(self.B, self.NT, 4)
        grids, out_ids, unlisted = [], [], []
        for b, (r, entries) in enumerate(zip(self.refs, self.entries())):
            if before is not None:
                before(b, r)
            if background is not None:
                apply_oracle(r, int(background[0][b]), int(background[0][b + 1]), background[1])
            c = {}
            grid = QM.expand(entries, quotes[b].tolist(), self.depth, c)
            for w in WORDS:
                self.count[w] += c.get(w, 0)
            o = r.book.orders_array()
            traded = set(int(i) for i in r.book.trades_array()["passive_id"])
            self.partial_keepers += sum(1 for k in c.get("keepers", []) if k in traded)
            mine = OM.resting(o, self.NT)
            for t, own in mine.items():
                self.most_resting = max(self.most_resting, len(own))
                if len(own) > self.depth and (quotes[b, t, 1] != KEEP or quotes[b, t, 3] != KEEP):
                    self.beyond_depth += 1
                    unlisted += [(b, x[0]) for x in own[self.depth:]]
            self.most_live_positions = max(self.most_live_positions, int((grid[0] != 0).sum()))
            out_ids.append(self.expected_ids(b, grid))
            apply_oracle(r, 0, len(grid[0]), grid)
            if after is not None:
                after(b, r)
            grids.append(grid)
        self.steps.append((background, quotes, join(grids), np.stack(out_ids)))
        if run:
            self.run_step()
            for b, i in unlisted:  # (the quotes cannot name them; only a trade takes them away)
                self.unlisted_stay += int(self.refs[b].book.orders_array()["status"][i]) == 1
        return self.steps[-1]

    def run_step(self):
        for r in self.refs:
            r.step()
            self.most_live = max(self.most_live, int((r.book.orders_array()["status"] == 1).sum()))
        rows = [OM.rows(r.book.orders_array(), self.NT, self.depth) for r in self.refs]
        self.rows_after.append((np.stack([x[0] for x in rows]), np.stack([x[1] for x in rows])))


# ------------------------------------------------------------------------------------------------ the busy flow
BUSY = dict(B=6, T=10, NT=5, depth=3, tick=2)


def draw_quotes(rng, plan, last, lo=48, p_keep=0.12, p_pull=0.08, p_same=0.2):
    """Quotes near the mid for every book and trader: a bid at lo x tick (one time in four a level above) and an ask at
    (lo + 3) x tick (likewise) of a volume from {50, 100, 200, 400} - the background's orders hold 20 .. 199, so a quote is
    often filled in part, and a side that stays at its price is as often topped up as reduced; with probability p_same a side
    repeats the trader's last row, p_keep gives KEEP, p_pull 0."""
    q = np.zeros((plan.B, plan.NT, 4), dtype=np.uint32)
    for b in range(plan.B):
        for t in range(plan.NT):
            for s, base in ((0, lo), (2, lo + 3)):
                u = rng.random()
                if last is not None and u < p_same:
                    q[b, t, s], q[b, t, s + 1] = last[b, t, s], last[b, t, s + 1]
                elif u < p_same + p_keep:
                    q[b, t, s], q[b, t, s + 1] = 0, KEEP
                elif u < p_same + p_keep + p_pull:
                    q[b, t, s], q[b, t, s + 1] = base * plan.tick, 0
                else:
                    q[b, t, s], q[b, t, s + 1] = (base + int(rng.random() < 0.25)) * plan.tick, int(rng.choice([50, 100, 200, 400]))
    return q


def busy_plan(oracle, pool):
    """6 books x 10 steps, 5 traders at depth 3 (G = 5): every step a thin background flow of traders >= 5000 whose prices
    (40 .. 59 x tick) cross the quotes, then the quotes."""
    plan = QuotePlan(oracle, BUSY["B"], BUSY["tick"], BUSY["NT"], BUSY["depth"])
    rng = np.random.default_rng(97 + pool)
    last = None
    for _ in range(BUSY["T"]):
        last = draw_quotes(rng, plan, last)
        plan.step(last, background=thin_flow(rng, plan.B, 4, plan.tick))
    return plan


def shape_plan(oracle, B, NT, depth, T, seed, n_bg=4):
    """the same flow at another shape: B books, NT traders at `depth`, T steps"""
    plan = QuotePlan(oracle, B, BUSY["tick"], NT, depth)
    rng = np.random.default_rng(seed)
    last = None
    for _ in range(T):
        last = draw_quotes(rng, plan, last)
        plan.step(last, background=thin_flow(rng, plan.B, n_bg, plan.tick))
    return plan


def wide_plan(oracle):
    """70 traders at depth 3 on 3 books: 350 grid positions, six passes, G = 5 straddles every pass boundary"""
    return shape_plan(oracle, 3, 70, 3, 4, 211)


def assert_busy(plan, pool):
    """the conditions under which the busy comparison says something, all counted on the expected side"""
    for w in WORDS:
        assert plan.count[w] > 0, (w, plan.count)
    assert plan.partial_keepers > 0 and plan.beyond_depth > 0 and plan.unlisted_stay > 0, vars(plan)
    assert plan.most_live < pool, (plan.most_live, pool)


# ------------------------------------------------------------------------------------------------ on the device
UNTOUCHED = 7  # what out_ids and status hold before a call: neither an id of these runs, nor u64::MAX, nor a status code


def outputs(torch, plan):
    return (torch.full((plan.B, plan.NT, 2), UNTOUCHED, dtype=torch.int64, device="cuda"),
            torch.full((plan.B, 2), UNTOUCHED, dtype=torch.int32, device="cuda"))


def quotes_dev(torch, quotes):
    return dev(torch, np.ascontiguousarray(quotes, dtype=np.uint32).view(np.int32))


# failures, against a twin env that takes the model's grid through submit_instructions_device
def twin_step(torch, twin, plan, s):
    """step s on the twin env: the same background, then the model's grid through submit_instructions_device"""
    bg, _, (off, ins), _ = plan.steps[s]
    if bg is not None:
        submit(torch, twin, *bg)
    n = len(ins[0])
    ids = torch.full((n,), UNTOUCHED, dtype=torch.int64, device="cuda")
    status = torch.full((plan.B, 2), UNTOUCHED, dtype=torch.int32, device="cuda")
    twin.submit_instructions_device(dev(torch, off), *[dev(torch, x) for x in ins], out_ids=ids, status=status)
    twin.step(sync=False)
    new_ids = ids.cpu().numpy().view(np.uint64).reshape(plan.B, plan.NT, plan.G)[:, :, plan.depth:]
    return new_ids, status.cpu().numpy()


def failing_step(torch, env, twin, plan, quotes, stop, code, raises):
    """One more step with `quotes`, which book `stop[0]` stops at grid position `stop[1]` with `code`: the expected side
    applies that book's grid up to there, both device envs must report the same status and ids, and equal the oracle;
    check_status raises `raises` = (exception, message) once the call is queued."""
    quotes = np.ascontiguousarray(quotes, dtype=np.uint32)
    entries = plan.entries()
    grids = [QM.expand(e, q.tolist(), plan.depth) for e, q in zip(entries, quotes)]
    want_ids = []
    for b, (r, g) in enumerate(zip(plan.refs, grids)):
        n = stop[1] if b == stop[0] else len(g[0])
        ids = plan.expected_ids(b, tuple(np.where(np.arange(len(x)) < n, x, 0) for x in g))
        if b == stop[0]:  # from the failing element on, out_ids is not written
            for i in range(n, len(g[0])):
                t, at = divmod(i, plan.G)
                if at >= plan.depth:
                    ids[t, at - plan.depth] = UNTOUCHED
        want_ids.append(ids)
        if b == stop[0] and code == 1:
            with pytest.raises(ValueError):  # the oracle stops at the bad price, as the reference does
                apply_oracle(r, 0, len(g[0]), g)
        else:
            apply_oracle(r, 0, n, g)
        r.step()
    plan.steps.append((None, quotes, join(grids), np.stack(want_ids)))
    s = len(plan.steps) - 1
    ids, status = outputs(torch, plan)
    with pytest.raises(raises[0], match=raises[1]):
        env.submit_quotes(quotes_dev(torch, quotes), ids, status, check_status=True)
    env.step(sync=False)
    got_ids, got_status = ids.cpu().numpy().view(np.uint64), status.cpu().numpy()
    twin_ids, twin_status = twin_step(torch, twin, plan, s)
    want_status = [[code, stop[1]] if b == stop[0] else [0, plan.NT * plan.G] for b in range(plan.B)]
    assert got_status.tolist() == want_status and twin_status.tolist() == want_status, (got_status.tolist(), twin_status.tolist())
    P.same_array(got_ids, twin_ids, "failing step", "out_ids against the twin's")
    P.same_array(got_ids, np.stack(want_ids), "failing step", "out_ids against the expected side's")
    return got_ids
