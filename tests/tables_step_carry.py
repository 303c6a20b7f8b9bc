"""What tests/test_gpu_tables_step_carry.py and tests/test_tables_step_carry_cpu.py share: the scenario's constants, one
adapter per folded table, and the EXPECTED side of every stage - the tables' plain-Python models over the oracle's run of
the same flow, built once per flow and never changed - with the conditions under which the comparison says something.

The scenario (per flow of test_gpu_counter_wrap.E_FLOWS): an env runs n steps, its checkpoint's step counters are moved
(tests/counter_shift.py) to 2^32 - 3, and a fresh env with EVERY folded table on is restored from it: the series with its
depth and candle companions, the lag table, the bin table, the flow table (book flows) or the cross table (the market
flow).  It runs T1 steps over the carry, saves, runs T2 unfolded steps, resets the alternate units - which folds the T2
steps and cuts the masked carries - runs T3 steps, loses one step to the ring, and a third env goes on from the image
taken behind the carry.  Every table's expected words come from the oracle's history()[lo:hi] with first_step = lo + OFF;
only the candle table's words depend on the step number itself, which is why it is folded once more with the steps cut to
32 bits: that table must differ, or a truncation on the device could not show.

Nothing here touches a device; importing it needs numpy and the models alone."""
import numpy as np

import bins_model as BM
import candles_model as CM
import cross_model as XM
import flow_model as FM
import oracle_parity as P
import series_model as SM
import test_gpu_counter_wrap as CW
from hist_tables import BINS, LAGS, SERIES, Table
from test_gpu_candles import CANDLES
from test_gpu_depth import DEPTH
from test_gpu_reset_books import make_mask

M32 = 1 << 32
FLOWS = ("fused", "wave_split", "members", "market")
BOOKS, RING, ASSETS = CW.E_BOOKS, CW.E_CAP, 2  # 6 books (3 markets of 2 assets), a ring of 12 slots: 2^32 % 12 = 4
# The steps run before the checkpoint, per flow.  The members' books (Noise + Momentum, levels 10, tick 1) are sparse: on the
# oracle books 0, 2 and 4 - the ones the alternate mask resets - are two-sided together only at steps 22 .. 30, and a cut shows in
# a book only if the step in front of it (n + T1 + T2 - 1) and the first replayed step (n + T1) both are.  n = 17 with T2 = 3 puts
# them at 29 and 27, keeps four books with pairs and a lag-4 return inside [17, 27), and leaves the cut in the middle of a bar.
N_OF = {"fused": 5, "wave_split": 5, "members": 17, "market": 5}
T1, T2, T3 = 10, 3, 7  # over the carry in chunks of 2; unfolded in front of the reset; behind it
LOST = RING + 1        # steps run without a fold: one of them falls out of the ring
START = M32 - 3        # steps_done of the restored env
CANDLE_W, CANDLE_N = 3, 4  # 2^32 % 3 = 1, 2^32 % 12 = 4: a truncated step changes bar, phase and slot
CFG = {"series": None, "depth": None, "candles": CM.config(CANDLE_W, CANDLE_N), "lags": 4, "bins": BM.config((1, 4), 64), "cross": (1, 3)}
FLOW_K = 4
BAR_STARTS = [M32 - 3, M32 - 1, M32 + 2, M32 + 5]  # the bars of steps [2^32 - 3, 2^32 + 7) at W = 3


class Cross(Table):
    """the per-market cross table as tests/hist_tables.py sees a table: its unit is the market, [steps, A, W] of the history"""
    name, noun, dtype = "cross", "cross table", XM.CROSS_DTYPE

    def rows(self, hist, spans, **kw):
        return XM.rows(hist, spans, ASSETS, **kw)

    def fold_model(self, h, spans=None, **kw):
        return XM.fold(h, **kw) if "into" in kw else XM.fold(h, spans, ASSETS, **kw)

    def table(self, s):
        return XM.table(s)

    def cleared(self, NM, spans):
        return np.zeros((NM, len(spans), ASSETS, ASSETS), dtype=XM.CROSS_DTYPE)

    def same(self, got, want, tag):
        assert got.dtype == want.dtype == XM.CROSS_DTYPE, (got.dtype, want.dtype)
        assert got.shape == want.shape, f"{tag}: rows {got.shape} vs {want.shape}"
        for f in XM.FIELDS:
            P.same_array(got[f], want[f], tag, f"cross word {f}")


CROSS = Cross()
RING_TABLES = {"series": SERIES, "depth": DEPTH, "candles": CANDLES, "lags": LAGS, "bins": BINS, "cross": CROSS}
FOLDS = {"series": "series", "lags": "lag table", "bins": "bin table", "cross": "cross table"}  # fold_<name>: the noun of its lost steps


def tables_of(flow):
    """the names of the tables folded from the history ring that the flow's env has on"""
    return [n for n in RING_TABLES if n != "cross" or flow == "market"]


def has_flow(flow):
    return flow != "market"


def tape_of(view):
    """an oracle book's trades as flow_model's tape: (price, vol, side_is_bid) in record order"""
    t = view.trades_array()
    return list(zip(t["price"].tolist(), t["vol"].tolist(), t["side"].tolist()))


class Plan:
    """The expected side of one flow.  ``want[table][stage]`` for the stages "cleared", "T1" (steps [n, L1)), "at_reset"
    (steps [n, L2), the masked units' carry cut), "T3" (the end of step 5), "uncut" (the same without the cut), "third" (the third
    env's steps [L1, L2)) and "T1_cut_to_32_bits" / "third_cut_to_32_bits" (the same records, every step number reduced modulo
    2^32).  ``flow[stage]`` holds the flow table's models of the same stages."""

    def __init__(self, oracle, name):
        self.name, self.F = name, CW._EFlow(None, oracle, name)
        n = self.n = N_OF[name]
        self.L1, self.L2, self.L3 = n + T1, n + T1 + T2, n + T1 + T2 + T3
        self.off = START - n
        self.hist, self.views = self.F.ref(self.L3)
        assert self.hist.shape[:2] == (self.L3, BOOKS)
        self.hist.flags.writeable = False
        self.levels = (self.hist.shape[2] - 5) // 4
        self.market = self.F.kind == "market"
        self.units = BOOKS // ASSETS if self.market else BOOKS  # what a reset's mask counts
        self.mask = make_mask("alternate", self.units)
        self.per_book = np.repeat(self.mask, BOOKS // self.units)
        self.want = {t: self._ring_table(RING_TABLES[t], CFG[t]) for t in tables_of(name)}
        self.flow = self._flow_table() if has_flow(name) else None

    # ---- the tables folded from the history ring
    def slices(self, T):
        """the history of each of the table's units: a book, or for the cross table a market's books"""
        if T is CROSS:
            return [self.hist[:, m * ASSETS:(m + 1) * ASSETS] for m in range(BOOKS // ASSETS)]
        return [self.hist[:, b] for b in range(BOOKS)]

    def unit_mask(self, T):
        return self.mask if T is CROSS and self.market else self.per_book

    def _fold(self, T, cfg, u, lo, hi, step_of=None):
        """the model's state over the oracle's steps [lo, hi) of one unit, step i standing at lo + off - or, record by record,
        at step_of(i)"""
        if step_of is None:
            return T.fold_model(u[lo:hi], cfg, first_step=lo + self.off)
        s = T.fold_model(u[lo:lo + 1], cfg, first_step=step_of(lo))
        for i in range(lo + 1, hi):
            T.fold_model(u[i:i + 1], first_step=step_of(i), into=s)
        return s

    def _ring_table(self, T, cfg):
        n, L1, L2, L3, off = self.n, self.L1, self.L2, self.L3, self.off
        us, mask = self.slices(T), self.unit_mask(T)
        cut_at = L2 + off  # the reset stands in front of this step
        w = {"cleared": T.cleared(len(us), self.levels if T is DEPTH else cfg)}
        w["T1"] = T.stack([T.table(self._fold(T, cfg, u, n, L1)) for u in us])
        at_reset, t3, uncut = [], [], []
        for u, m in zip(us, mask):
            s = self._fold(T, cfg, u, n, L2)
            at_reset.append(T.table(SM.cut(s) if (T is SERIES and m) else s))
            if m:  # a reset unit replays the oracle's steps L1 .. L1 + T3 behind the cut, at the env's step numbers
                t3.append(T.table(T.fold_model(u[L1:L1 + T3], cuts=[cut_at], first_step=cut_at, into=self._fold(T, cfg, u, n, L2))))
                uncut.append(T.table(T.fold_model(u[L1:L1 + T3], first_step=cut_at, into=self._fold(T, cfg, u, n, L2))))
            else:
                t3.append(T.table(self._fold(T, cfg, u, n, L3)))
                uncut.append(t3[-1])
        w["at_reset"], w["T3"], w["uncut"] = T.stack(at_reset), T.stack(t3), T.stack(uncut)
        w["third"] = T.stack([T.table(self._fold(T, cfg, u, L1, L2)) for u in us])
        cut32 = lambda i: (i + off) % M32  # noqa: E731
        w["T1_cut_to_32_bits"] = T.stack([T.table(self._fold(T, cfg, u, n, L1, cut32)) for u in us])
        w["third_cut_to_32_bits"] = T.stack([T.table(self._fold(T, cfg, u, L1, L2, cut32)) for u in us])
        # the record-by-record fold at the true steps is the one-pass fold: the models are split-invariant
        for stage, (lo, hi) in (("T1", (n, L1)), ("third", (L1, L2))):
            again = T.stack([T.table(self._fold(T, cfg, u, lo, hi, lambda i: i + off)) for u in us])
            T.same(again, w[stage], f"{T.name}: the model of {stage}, record by record")
        return w

    # ---- the flow table: the oracle's trade tape, the way tests/test_gpu_flow.py builds its expected rows
    def _flow_table(self):
        F, n, L1, L2, L3 = self.F, self.n, self.L1, self.L2, self.L3
        tc = {L: F.counts(L) for L in (n, L1, L2, L3, L1 + T3)}
        kept, back = [tape_of(v) for v in F.ref(L3)[1]], [tape_of(v) for v in F.ref(L1 + T3)[1]]
        for b in range(BOOKS):  # a reset book trades the oracle's records of the shorter run, the same up to the snapshot
            assert kept[b][:tc[L1][b]] == back[b][:tc[L1][b]] and len(kept[b]) == tc[L3][b] and len(back[b]) == tc[L1 + T3][b]
        out = {"counts": tc, "T1": [], "at_reset": [], "T3": [], "uncut": [], "third": []}
        for b in range(BOOKS):
            md = FM.FlowModel(FLOW_K, tc[n][b])
            md.fold(kept[b], tc[L1][b])
            out["T1"].append((md.words(), md.carry(), md.seen))
            md.fold(kept[b], tc[L2][b])
            if self.per_book[b]:
                joined = FM.FlowModel(FLOW_K, tc[n][b])
                joined.fold(kept[b][:tc[L2][b]] + back[b][tc[L1][b]:], tc[L2][b] + tc[L1 + T3][b] - tc[L1][b])
                out["uncut"].append((joined.words(), None, None))
                md.cut(tc[L1][b])
                out["at_reset"].append((md.words(), md.carry(), md.seen))
                md.fold(back[b], tc[L1 + T3][b])
            else:
                out["at_reset"].append((md.words(), md.carry(), md.seen))
                md.fold(kept[b], tc[L3][b])
            out["T3"].append((md.words(), md.carry(), md.seen))
            if not self.per_book[b]:
                out["uncut"].append(out["T3"][-1])
            third = FM.FlowModel(FLOW_K, tc[L1][b])
            third.fold(kept[b], tc[L2][b])
            out["third"].append((third.words(), third.carry(), third.seen))
        return out

    def flow_rows(self, stage):
        return FM.rows_of([w for w, _, _ in self.flow[stage]], FLOW_K)

    def flow_state(self, stage):
        """(carry [B, K], cursors [B]) as env.flow_state() reports them"""
        return (np.array([c for _, c, _ in self.flow[stage]], dtype=np.uint64), np.array([s for _, _, s in self.flow[stage]], dtype=np.uint64))

    # ---- what must hold of the expected side for the comparison to say anything
    def conditions(self):
        n, L1, L2, off = self.n, self.L1, self.L2, self.off
        w = self.want
        assert n + off == START < M32 <= L1 + off and (n + off) % RING != n % RING
        assert (w["series"]["T1"]["n_steps"] == T1).all(), w["series"]["T1"]["n_steps"]
        lag = w["lags"]["T1"]
        live = (lag[:, 0]["n_pairs"] > 0) & (lag[:, CFG["lags"] - 1]["n_h"] > 0)
        assert live.sum() >= 4, (lag[:, 0]["n_pairs"], lag[:, CFG["lags"] - 1]["n_h"])
        assert (w["bins"]["T1"][live][:, 1].sum(axis=1) > 0).all(), "span-4 totals of the same books"
        # the bars: T1 = 10 steps from 2^32 - 3 on are four bars of 2, 3, 3 and 2 steps, on both sides of 2^32, a slot each
        bars = w["candles"]["T1"]
        assert (np.sort(bars["first_step"], axis=1) == np.array(BAR_STARTS, dtype=np.uint64)).all(), bars["first_step"]
        assert (bars["n_steps"] > 0).sum(axis=1).min() >= 3 and (bars["first_step"] < M32).any() and (bars["first_step"] >= M32).any()
        for b in range(BOOKS):
            assert sorted(zip(bars[b]["first_step"].tolist(), bars[b]["n_steps"].tolist())) == list(zip(BAR_STARTS, [2, 3, 3, 2])), b
            assert [int(x) // CANDLE_W % CANDLE_N for x in bars[b]["first_step"]] == list(range(CANDLE_N)), "bar j in slot j % N"
        # the cut stands in the middle of a bar, and so does the third env's first step
        assert (L2 + off) % CANDLE_W and (L1 + off) % CANDLE_W and L1 + off > M32
        if self.market:
            x = w["cross"]["T1"]
            assert (x["n"][:, 0] > 0).all(), x["n"][:, 0]
            assert (x["n_lead"][:, 1] > 0).all(axis=(1, 2)).any(), x["n_lead"][:, 1]
        # the cut of step 4 shows in every table of every masked unit
        for t in tables_of(self.name):
            m = self.unit_mask(RING_TABLES[t])
            for u in np.flatnonzero(m):
                assert w[t]["T3"][u].tobytes() != w[t]["uncut"][u].tobytes(), f"the cut would not show in {t} of unit {u}"
            for u in np.flatnonzero(~m):
                assert w[t]["T3"][u].tobytes() == w[t]["uncut"][u].tobytes()
        if self.flow:
            for b in np.flatnonzero(self.per_book):
                assert self.flow["T3"][b][0] != self.flow["uncut"][b][0], f"the cut would not show in the flow table of book {b}"
            t1 = self.flow_rows("T1")
            assert (t1["n_trades"] > FLOW_K).all() and (t1["lags"][:, FLOW_K - 1, 0] > 0).all(), t1["n_trades"]
            assert ((t1["n_buy"] > 0) & (t1["n_buy"] < t1["n_trades"])).all() and not self.flow_rows("T3")["n_lost"].any()
        # a step number cut to 32 bits gives another candle table, on both sides of the carry and wholly behind it
        for stage in ("T1", "third"):
            assert w["candles"][stage].tobytes() != w["candles"][stage + "_cut_to_32_bits"].tobytes(), f"candles, {stage}: a truncated step would not show"

    def step_free(self):
        """the tables whose words do not depend on the step number: their models cut to 32 bits give the same table"""
        return [t for t in tables_of(self.name) if all(self.want[t][s].tobytes() == self.want[t][s + "_cut_to_32_bits"].tobytes() for s in ("T1", "third"))]


_plans = {}


def plan(oracle, name):
    """the flow's expected side: built once, shared by every test, never changed"""
    if name not in _plans:
        _plans[name] = Plan(oracle, name)
    return _plans[name]
