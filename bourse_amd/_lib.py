"""ctypes binding of the C ABI declared in include/bourse_amd.h.

The HIP extension is the only execution path: if libbourse_amd.so is missing this raises,
and if no GPU is usable every env-creating call raises ``NoDeviceError``.  There is no CPU
fallback (the CPU oracle under oracle/ is test infrastructure and is never imported here).
"""
import ctypes as C
import os

import numpy as np

from . import _build

BK_OK, BK_PRICE, BK_UNKNOWN_ORDER, BK_CAPACITY, BK_STEP_SIZE, BK_INVALID, BK_HIP, BK_NO_DEVICE = range(8)

FLAG_POOL_OVERFLOW, FLAG_TRADE_OVERFLOW, FLAG_STEP_SIZE, FLAG_ORDER_LOG_FULL = 1, 2, 4, 8
FLAG_UNKNOWN_ORDER, FLAG_HIST_OVERFLOW, FLAG_PRICE_TICK, FLAG_EVENT_OVERFLOW = 16, 32, 64, 128
FLAG_DECODE_LOOKAHEAD = 256
FLAG_ACCOUNTS_INEXACT = 512
ACTION_MODIFY = 0x80000003  # BK_ACTION_MODIFY: the one extension of submit_instructions' action codes (0 / 1 / 2)
FLAG_NAMES = {1: "POOL_OVERFLOW (live-order pool full: a resting order was dropped)",
              2: "TRADE_OVERFLOW (trade_capacity exceeded: records dropped, counts exact)",
              4: "STEP_SIZE (a step queued >= step_size events)",
              8: "ORDER_LOG_FULL (order id beyond max_orders)",
              16: "UNKNOWN_ORDER", 32: "HIST_OVERFLOW",
              64: "PRICE_TICK (a Noise/Momentum limit price clamped to u32::MAX was not a tick multiple)",
              128: "EVENT_OVERFLOW (a market queued more events in one step than its shared list holds)",
              256: "DECODE_LOOKAHEAD (a ziggurat rejection loop outran the members' decode's 128-draw look-ahead)",
              512: "ACCOUNTS_INEXACT (a trade record could not be folded into the trader accounts: dropped beyond "
                   "trade_capacity, or an order id beyond max_orders)"}
# (ACCOUNTS_INEXACT comes of the same two capacities as TRADE_OVERFLOW and ORDER_LOG_FULL)
CAPACITY_FLAGS = (FLAG_POOL_OVERFLOW | FLAG_TRADE_OVERFLOW | FLAG_ORDER_LOG_FULL | FLAG_EVENT_OVERFLOW |
                  FLAG_ACCOUNTS_INEXACT)


class BourseError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"bourse_amd status {code}: {msg}")
        self.code = code


class NoDeviceError(BourseError):
    pass


class CapacityError(BourseError):
    pass


class Config(C.Structure):
    _fields_ = [
        ("n_books", C.c_uint32), ("levels", C.c_uint32), ("start_time", C.c_uint64),
        ("tick_size", C.c_uint32), ("trading", C.c_uint32), ("step_size", C.c_uint64),
        ("seed", C.c_uint64), ("book_offset", C.c_uint64), ("max_live_orders", C.c_uint32),
        ("max_orders", C.c_uint32), ("trade_capacity", C.c_uint32), ("history_capacity", C.c_uint32),
        ("device", C.c_int32), ("assets", C.c_uint32),
    ]


class RandomAgentsCfg(C.Structure):
    _fields_ = [
        ("n_agents", C.c_uint32), ("tick_lo", C.c_uint32), ("tick_hi", C.c_uint32),
        ("vol_lo", C.c_uint32), ("vol_hi", C.c_uint32), ("tick_size", C.c_uint32),
        ("activity_rate", C.c_float),
    ]


class AgentDesc(C.Structure):
    _fields_ = [
        ("type", C.c_uint32), ("n_agents", C.c_uint32), ("tick_lo", C.c_uint32), ("tick_hi", C.c_uint32),
        ("vol_lo", C.c_uint32), ("vol_hi", C.c_uint32), ("tick_size", C.c_uint32), ("activity_rate", C.c_float),
        ("agent_id_start", C.c_uint32), ("p_limit", C.c_float), ("p_market", C.c_float), ("p_cancel", C.c_float),
        ("trade_vol", C.c_uint32), ("reserved", C.c_uint32), ("price_dist_mu", C.c_double),
        ("price_dist_sigma", C.c_double), ("decay", C.c_double), ("demand", C.c_double), ("scale", C.c_double),
        ("order_ratio", C.c_double),
    ]


class Stats(C.Structure):
    _fields_ = [
        ("n_books", C.c_uint64), ("sum_trade_vol", C.c_uint64), ("sum_trades", C.c_uint64),
        ("sum_events", C.c_uint64), ("sum_bid_vol", C.c_uint64), ("sum_ask_vol", C.c_uint64),
        ("min_bid", C.c_uint32), ("max_bid", C.c_uint32), ("min_ask", C.c_uint32), ("max_ask", C.c_uint32),
    ]


TRADE_DTYPE = np.dtype(
    {"names": ["t", "side", "price", "vol", "active_id", "passive_id"],
     "formats": ["<u8", "<u4", "<u4", "<u4", "<u8", "<u8"], "offsets": [0, 8, 12, 16, 24, 32], "itemsize": 40})
ORDER_DTYPE = np.dtype(
    {"names": ["side", "status", "arr_time", "end_time", "vol", "start_vol", "price", "trader_id", "order_id"],
     "formats": ["u1", "u1", "<u8", "<u8", "<u4", "<u4", "<u4", "<u4", "<u8"],
     "offsets": [0, 1, 8, 16, 24, 28, 32, 36, 40], "itemsize": 48})

# bk_account: one trader's row of the accounts table (ManyBookEnv.accounts)
ACCOUNT_DTYPE = np.dtype(
    {"names": ["position", "cash", "volume", "fills"], "formats": ["<i8", "<i8", "<u8", "<u8"],
     "offsets": [0, 8, 16, 24], "itemsize": 32})

# bk_trade_bar: one book's bar of one step (ManyBookEnv.trade_bars)
TRADE_BAR_DTYPE = np.dtype(
    {"names": ["open", "high", "low", "close", "buy_vol", "sell_vol", "notional", "n_buy", "n_sell"],
     "formats": ["<u4", "<u4", "<u4", "<u4", "<u8", "<u8", "<u8", "<u4", "<u4"],
     "offsets": [0, 4, 8, 12, 16, 24, 32, 40, 44], "itemsize": 48})

# bk_series_row: one book's series moments of the level-2 history (ManyBookEnv.series), 24 words of 8 bytes
SERIES_FIELDS = ("n_steps", "n_two_sided", "sum_m", "sum_spread", "sum_spread_sq", "sum_bid_vol", "sum_ask_vol", "sum_trade_vol",
                 "sum_trade_vol_sq", "n_trade_steps", "n_ret", "sum_d", "sum_abs_d", "sum_d2", "sum_d4_lo", "sum_d4_hi", "max_abs_d",
                 "n_pairs", "sum_dd", "sum_abs_dd", "min_m", "max_m", "carry_m", "carry_d")
SERIES_SIGNED = ("sum_d", "sum_dd", "carry_d")
SERIES_DTYPE = np.dtype(
    {"names": list(SERIES_FIELDS), "formats": ["<i8" if n in SERIES_SIGNED else "<u8" for n in SERIES_FIELDS],
     "offsets": [8 * i for i in range(24)], "itemsize": 192})

SERIES_MOMENTS_DTYPE = np.dtype([(n, "<f8") for n in (
    "mean_mid", "mean_spread", "var_spread", "mean_return", "var_return", "kurtosis_return", "acf1_return", "acf1_abs_return",
    "mean_trade_vol", "mean_bid_vol", "mean_ask_vol")])


def series_moments(rows) -> np.ndarray:
    """``SERIES_DTYPE`` rows (``ManyBookEnv.series()``) -> float64 moments per book (``SERIES_MOMENTS_DTYPE``), computed
    exactly in Python integers and rounded once.  With ``d`` the step-to-step change of TWICE the mid between consecutive
    two-sided steps (a return of the mid is ``d / 2``):

    ``mean_mid`` = sum_m / (2 n_two_sided); ``mean_spread``, ``var_spread`` (population variance) over two-sided steps;
    ``mean_return`` = sum_d / (2 n_ret); ``var_return`` = (sum_d2 / n_ret - (sum_d / n_ret)^2) / 4;
    ``kurtosis_return`` = n_ret sum_d4 / sum_d2^2 - 3, the excess kurtosis ABOUT ZERO (the row keeps no third power);
    ``acf1_return`` = (sum_dd / n_pairs - mean_d^2) / var_d and ``acf1_abs_return`` the same of ``|d|`` - lag-1
    autocorrelations with the moments of all returns for both factors; ``mean_trade_vol``, ``mean_bid_vol``,
    ``mean_ask_vol`` (the touch volumes) per step.  A division by a zero count or a zero variance gives NaN.  The words
    are read as they are: a sum that has wrapped modulo 2^64 is not detected (the counts and ``max_abs_d`` bound them)."""
    from fractions import Fraction as F

    rows = np.atleast_1d(np.asarray(rows))
    if rows.dtype != SERIES_DTYPE:
        raise ValueError("series_moments needs SERIES_DTYPE rows")
    out = np.full(rows.shape, np.nan, dtype=SERIES_MOMENTS_DTYPE)

    def div(a, b):
        return F(a, b) if b else None

    def put(o, name, x):
        o[name] = np.nan if x is None else float(x)

    for r, o in zip(rows.reshape(-1), out.reshape(-1)):
        w = {n: int(r[n]) for n in SERIES_FIELDS}
        n2, nr, npair, ns = w["n_two_sided"], w["n_ret"], w["n_pairs"], w["n_steps"]
        d4 = w["sum_d4_lo"] | (w["sum_d4_hi"] << 64)
        put(o, "mean_mid", div(w["sum_m"], 2 * n2))
        ms = div(w["sum_spread"], n2)
        put(o, "mean_spread", ms)
        put(o, "var_spread", None if ms is None else F(w["sum_spread_sq"], n2) - ms * ms)
        md, mabs = div(w["sum_d"], nr), div(w["sum_abs_d"], nr)
        put(o, "mean_return", None if md is None else md / 2)
        var_d = None if md is None else F(w["sum_d2"], nr) - md * md
        var_abs = None if mabs is None else F(w["sum_d2"], nr) - mabs * mabs
        put(o, "var_return", None if var_d is None else var_d / 4)
        put(o, "kurtosis_return", None if not w["sum_d2"] else F(nr * d4, w["sum_d2"] ** 2) - 3)
        put(o, "acf1_return", None if not npair or not var_d else (F(w["sum_dd"], npair) - md * md) / var_d)
        put(o, "acf1_abs_return", None if not npair or not var_abs else (F(w["sum_abs_dd"], npair) - mabs * mabs) / var_abs)
        put(o, "mean_trade_vol", div(w["sum_trade_vol"], ns))
        put(o, "mean_bid_vol", div(w["sum_bid_vol"], ns))
        put(o, "mean_ask_vol", div(w["sum_ask_vol"], ns))
    return out


# the depth table (ManyBookEnv.depth): per book levels + 1 rows of 16 words of 8 bytes - a level's row, and the header's
DEPTH_FIELDS = ("sum_bid_vol", "sum_ask_vol", "sum_bid_vol_sq", "sum_ask_vol_sq", "sum_bid_orders", "sum_ask_orders", "n_bid_steps",
                "n_ask_steps", "sum_imb", "sum_imb_sq", "n_signed", "sum_sign_d", "n_agree", "sum_imb_d", "n_move", "sum_abs_imb")
DEPTH_HEADER_FIELDS = ("n_steps", "n_two_sided", "n_pairs", "sum_d", "sum_abs_d", "n_up", "n_down", "n_bid_side", "n_ask_side")
DEPTH_SIGNED = ("sum_imb", "sum_sign_d", "sum_imb_d")
DEPTH_ROW_WORDS = 16

DEPTH_MOMENTS_DTYPE = np.dtype([(n, "<f8") for n in (
    "mean_bid_vol", "mean_ask_vol", "var_bid_vol", "var_ask_vol", "mean_bid_orders", "mean_ask_orders", "bid_occupancy",
    "ask_occupancy", "mean_imb", "var_imb", "response", "hit_rate", "slope")])


def depth_moments(rows) -> np.ndarray:
    """Depth rows ``[n_books, L + 1, 16]`` (``ManyBookEnv.depth()``; one book's ``[L + 1, 16]`` too) -> float64 moments per
    book and level, ``[n_books, L]`` (``DEPTH_MOMENTS_DTYPE``).  Per step, from the header's ``n_steps``: ``mean_bid_vol``,
    ``mean_ask_vol``, ``var_bid_vol``, ``var_ask_vol`` (population variances), ``mean_bid_orders``, ``mean_ask_orders`` and
    the share of steps at which the level held an order, ``bid_occupancy``, ``ask_occupancy``.  Over two-sided steps
    (``n_two_sided``): ``mean_imb`` and ``var_imb`` of the cumulative imbalance ``I_q``.  Over pairs of consecutive two-sided
    steps, with ``J`` the imbalance of the first and ``d`` the change of TWICE the mid: ``response`` = sum_sign_d / n_signed
    / 2, the mean move of the mid in the direction the imbalance pointed, in mid-price units; ``hit_rate`` = n_agree /
    n_move, how often a move went that way; ``slope`` = sum_imb_d / sum_imb_sq, the regression of ``d`` on ``J`` through
    the origin.  NaN where a count or a denominator is 0.  The words are read as they are: a sum that has wrapped modulo
    2^64 is not detected."""
    rows = np.asarray(rows)
    if rows.ndim == 2:
        rows = rows[None]
    if rows.ndim != 3 or rows.shape[1] < 2 or rows.shape[2] != DEPTH_ROW_WORDS or rows.dtype.kind not in "iu" or rows.dtype.itemsize != 8:
        raise ValueError("depth_moments needs 64-bit integer rows [n_books, levels + 1, 16]")
    u = np.ascontiguousarray(rows).view(np.uint64)
    w = {n: (u[:, :-1, i].view(np.int64) if n in DEPTH_SIGNED else u[:, :-1, i]).astype(np.float64) for i, n in enumerate(DEPTH_FIELDS)}
    h = {n: u[:, -1:, i].astype(np.float64) for i, n in enumerate(DEPTH_HEADER_FIELDS)}
    out = np.full((u.shape[0], u.shape[1] - 1), np.nan, dtype=DEPTH_MOMENTS_DTYPE)

    def div(a, b):
        b = np.broadcast_to(b, a.shape)
        return np.divide(a, b, out=np.full(a.shape, np.nan), where=b != 0)

    ns, n2 = h["n_steps"], h["n_two_sided"]
    for side in ("bid", "ask"):
        mean = div(w[f"sum_{side}_vol"], ns)
        out[f"mean_{side}_vol"] = mean
        out[f"var_{side}_vol"] = div(w[f"sum_{side}_vol_sq"], ns) - mean * mean
        out[f"mean_{side}_orders"] = div(w[f"sum_{side}_orders"], ns)
        out[f"{side}_occupancy"] = div(w[f"n_{side}_steps"], ns)
    mean = div(w["sum_imb"], n2)
    out["mean_imb"] = mean
    out["var_imb"] = div(w["sum_imb_sq"], n2) - mean * mean
    out["response"] = div(w["sum_sign_d"], w["n_signed"]) / 2.0
    out["hit_rate"] = div(w["n_agree"], w["n_move"])
    out["slope"] = div(w["sum_imb_d"], w["sum_imb_sq"])
    return out


# the candle table (ManyBookEnv.candles): per book n_candles rows of 16 words of 8 bytes, one bar of `width` steps each
CANDLE_FIELDS = ("first_step", "n_steps", "n_two_sided", "open_m", "high_m", "low_m", "close_m", "sum_m", "sum_spread", "sum_trade_vol",
                 "n_trade_steps", "n_ret", "sum_d", "sum_abs_d", "sum_d2", "max_abs_d")
CANDLE_SIGNED = ("sum_d",)
CANDLE_ROW_WORDS = 16
CANDLE_DTYPE = np.dtype({"names": list(CANDLE_FIELDS), "formats": ["<i8" if n in CANDLE_SIGNED else "<u8" for n in CANDLE_FIELDS],
                         "offsets": [8 * i for i in range(CANDLE_ROW_WORDS)], "itemsize": 8 * CANDLE_ROW_WORDS})

CANDLE_SERIES_DTYPE = np.dtype([(n, "<f8") for n in ("open", "high", "low", "close", "twap", "mean_spread", "volume", "trade_share",
                                                     "realized_var")] + [("bar", "<i8"), ("complete", "?")])


def candle_series(rows, width: int) -> np.ndarray:
    """``CANDLE_DTYPE`` rows ``[n_books, N]`` (``ManyBookEnv.candles()``; one book's ``[N]`` too) of bars of ``width`` steps
    -> per book the bars ordered OLDEST TO NEWEST, ``[n_books, N]`` (``CANDLE_SERIES_DTYPE``), empty slots first.  In
    mid-price units: ``open``, ``high``, ``low``, ``close`` (the words over 2), ``twap`` = sum_m / (2 n_two_sided),
    ``mean_spread`` = sum_spread / n_two_sided, ``realized_var`` = sum_d2 / 4 (the sum of the squared changes of the mid
    whose later step lies in the bar).  ``volume`` = sum_trade_vol, ``trade_share`` = n_trade_steps / n_steps.  ``bar`` is
    the bar's index first_step // width, -1 for a slot that holds no bar; ``complete`` = n_steps == width (the newest bar,
    and the first behind an enable or a clear, may be partial).  A value is NaN where its count is 0.  The words are read as
    they are: a sum that has wrapped modulo 2^64 is not detected."""
    rows = np.asarray(rows)
    if rows.dtype != CANDLE_DTYPE:
        raise ValueError("candle_series needs CANDLE_DTYPE rows")
    width = int(width)
    if width < 1:
        raise ValueError("width must be >= 1")
    if rows.ndim == 1:
        rows = rows[None]
    if rows.ndim != 2:
        raise ValueError("candle_series needs rows [n_books, n_candles]")
    n_steps = rows["n_steps"]
    bar = np.where(n_steps > 0, (rows["first_step"] // np.uint64(width)).astype(np.int64), np.int64(-1))
    order = np.argsort(bar, axis=1, kind="stable")
    rows, bar = np.take_along_axis(rows, order, axis=1), np.take_along_axis(bar, order, axis=1)
    out = np.zeros(rows.shape, dtype=CANDLE_SERIES_DTYPE)

    def div(a, b):
        a, b = a.astype(np.float64), b.astype(np.float64)
        return np.divide(a, b, out=np.full(a.shape, np.nan), where=b != 0)

    n2, ns = rows["n_two_sided"], rows["n_steps"]
    one = np.ones(rows.shape)
    for name, word in (("open", "open_m"), ("high", "high_m"), ("low", "low_m"), ("close", "close_m")):
        out[name] = div(rows[word], (n2 > 0) * one) / 2.0
    out["twap"] = div(rows["sum_m"], n2) / 2.0
    out["mean_spread"] = div(rows["sum_spread"], n2)
    out["volume"] = div(rows["sum_trade_vol"], (ns > 0) * one)
    out["trade_share"] = div(rows["n_trade_steps"], ns)
    out["realized_var"] = div(rows["sum_d2"], (rows["n_ret"] > 0) * one) / 4.0
    out["bar"] = bar
    out["complete"] = ns == np.uint64(width)
    return out


# bk_lag_row: one book's row of one lag of the lag table (ManyBookEnv.lags), 10 words of 8 bytes
LAG_FIELDS = ("n_pairs", "sum_dd", "sum_abs_dd", "n_h", "sum_h", "sum_abs_h", "sum_h2", "sum_h4_lo", "sum_h4_hi", "max_abs_h")
LAG_SIGNED = ("sum_dd", "sum_h")
LAG_DTYPE = np.dtype(
    {"names": list(LAG_FIELDS), "formats": ["<i8" if n in LAG_SIGNED else "<u8" for n in LAG_FIELDS],
     "offsets": [8 * i for i in range(10)], "itemsize": 80})
MAX_LAGS = 64

LAG_MOMENTS_DTYPE = np.dtype([(n, "<f8") for n in ("acf_return", "acf_abs_return", "var_h", "kurtosis_h", "variance_ratio")])


def lag_moments(rows) -> np.ndarray:
    """``LAG_DTYPE`` rows ``[..., n_lags]`` (``ManyBookEnv.lags()``) -> float64 moments of the same shape
    (``LAG_MOMENTS_DTYPE``), computed exactly in Python integers and rounded once.  The last axis is the lag: index ``k - 1``
    is lag / span ``k``.  With ``d`` the step-to-step change of TWICE the mid and ``h`` its change over ``k`` steps:

    ``acf_return[k]`` = (sum_dd / n_pairs - mu^2) / var, with ``mu`` and ``var`` of ``d`` from row 0's span words (the
    moments of all returns for both factors, as ``series_moments``' ``acf1_return``, which ``k = 1`` equals bit for bit);
    ``acf_abs_return[k]`` the same of ``|d|``; ``var_h[k]`` = (sum_h2 / n_h - (sum_h / n_h)^2) / 4, the variance of the
    mid's change over ``k`` steps; ``kurtosis_h[k]`` = n_h sum_h4 / sum_h2^2 - 3, the excess kurtosis ABOUT ZERO;
    ``variance_ratio[k]`` = var_h[k] / (k var_h[1]).  A division by a zero count or a zero variance gives NaN.  The words
    are read as they are: a sum that has wrapped modulo 2^64 is not detected."""
    from fractions import Fraction as F

    rows = np.asarray(rows)
    if rows.dtype != LAG_DTYPE or rows.ndim < 1:
        raise ValueError("lag_moments needs LAG_DTYPE rows of shape [..., n_lags]")
    out = np.full(rows.shape, np.nan, dtype=LAG_MOMENTS_DTYPE)
    K = rows.shape[-1]

    def put(o, name, x):
        o[name] = np.nan if x is None else float(x)

    for table, o in zip(rows.reshape(-1, K), out.reshape(-1, K)):
        w = [{n: int(r[n]) for n in LAG_FIELDS} for r in table]
        nr = w[0]["n_h"]  # row 0's spans are the returns themselves
        md = F(w[0]["sum_h"], nr) if nr else None
        mabs = F(w[0]["sum_abs_h"], nr) if nr else None
        var_d = None if md is None else F(w[0]["sum_h2"], nr) - md * md
        var_abs = None if mabs is None else F(w[0]["sum_h2"], nr) - mabs * mabs
        var_h = []
        for r in w:
            mh = F(r["sum_h"], r["n_h"]) if r["n_h"] else None
            var_h.append(None if mh is None else (F(r["sum_h2"], r["n_h"]) - mh * mh) / 4)
        for k, r in enumerate(w):
            npair, h4 = r["n_pairs"], r["sum_h4_lo"] | (r["sum_h4_hi"] << 64)
            put(o[k], "acf_return", None if not npair or not var_d else (F(r["sum_dd"], npair) - md * md) / var_d)
            put(o[k], "acf_abs_return", None if not npair or not var_abs else (F(r["sum_abs_dd"], npair) - mabs * mabs) / var_abs)
            put(o[k], "var_h", var_h[k])
            put(o[k], "kurtosis_h", None if not r["sum_h2"] else F(r["n_h"] * h4, r["sum_h2"] ** 2) - 3)
            put(o[k], "variance_ratio", None if var_h[k] is None or not var_h[0] else var_h[k] / ((k + 1) * var_h[0]))
    return out


# one book of the flow table (ManyBookEnv.flow): eight base words, then n_lags rows of six words (BK_FLOW_* in the header)
FLOW_BASE_FIELDS = ("n_trades", "n_buy", "sum_vol", "buy_vol", "sum_vol_sq", "notional", "max_vol", "n_lost")
FLOW_LAG_FIELDS = ("n_pairs", "sum_ss", "sum_resp", "sum_back", "sum_abs_dp", "sum_dp2")
FLOW_LAG_SIGNED = ("sum_ss", "sum_resp", "sum_back")


def flow_dtype(n_lags: int) -> np.dtype:
    """One book's row of a flow table with ``n_lags`` lags, ``8 * (8 + 6 * n_lags)`` bytes: the base words as u64 fields, then
    ``lags``, an int64 ``(n_lags, 6)`` sub-array whose row ``k - 1`` holds ``FLOW_LAG_FIELDS`` of lag ``k`` (the unsigned
    words read as int64: the same bits)."""
    K = int(n_lags)
    if not 1 <= K <= MAX_LAGS:
        raise ValueError("n_lags must be in 1..64")
    return np.dtype({"names": list(FLOW_BASE_FIELDS) + ["lags"], "formats": ["<u8"] * 8 + [("<i8", (K, 6))],
                     "offsets": [8 * i for i in range(9)], "itemsize": 8 * (8 + 6 * K)})


FLOW_DTYPE = flow_dtype(16)  # (enable_flow's default n_lags; an env's own is ManyBookEnv.flow_dtype())
FLOW_MOMENTS_BASE = ("buy_share", "sign_mean", "mean_vol", "var_vol", "vwap", "lost_share")
FLOW_MOMENTS_LAG = ("sign_acf", "response", "back_response", "mean_abs_dp", "variogram")


def flow_moments(rows) -> np.ndarray:
    """``flow_dtype(K)`` rows of any shape (``ManyBookEnv.flow()``) -> float64 moments of the same shape, computed exactly in
    Python integers and rounded once: the fields ``FLOW_MOMENTS_BASE`` and, each a ``(K,)`` sub-array with index ``k - 1``
    for lag ``k`` in TRADE time, ``FLOW_MOMENTS_LAG``.

    ``buy_share`` = n_buy / n_trades; ``sign_mean`` = 2 buy_share - 1; ``mean_vol``, ``var_vol`` the mean and variance of the
    trade size; ``vwap`` = notional / sum_vol; ``lost_share`` = n_lost / (n_trades + n_lost).  Per lag, over its n_pairs:
    ``sign_acf`` = (sum_ss / n - sign_mean^2) / (1 - sign_mean^2); ``response`` = sum_resp / n, the mean price change k trades
    AFTER a trade in the direction of that trade; ``back_response`` = sum_back / n, the same before it; ``mean_abs_dp`` =
    sum_abs_dp / n; ``variogram`` = sum_dp2 / n.  A value is NaN where a count or a denominator is 0.  The words are read
    as they are: a sum that has wrapped modulo 2^64 is not detected."""
    from fractions import Fraction as F

    rows = np.asarray(rows)
    names = rows.dtype.names or ()
    if tuple(names) != FLOW_BASE_FIELDS + ("lags",) or rows.dtype["lags"].shape[1:] != (6,):
        raise ValueError("flow_moments needs flow_dtype(K) rows")
    K = rows.dtype["lags"].shape[0]
    out = np.full(rows.shape, np.nan, dtype=np.dtype([(n, "<f8") for n in FLOW_MOMENTS_BASE] + [(n, "<f8", (K,)) for n in FLOW_MOMENTS_LAG]))
    M = (1 << 64) - 1
    flat_in, flat_out = rows.reshape(-1), out.reshape(-1)
    for i in range(flat_in.size):
        r, o = flat_in[i], flat_out[i]
        w = {n: int(r[n]) for n in FLOW_BASE_FIELDS}
        n, lost = w["n_trades"], w["n_lost"]
        mean = None
        if n:
            mean = F(2 * w["n_buy"], n) - 1
            o["buy_share"], o["sign_mean"] = float(F(w["n_buy"], n)), float(mean)
            mv = F(w["sum_vol"], n)
            o["mean_vol"], o["var_vol"] = float(mv), float(F(w["sum_vol_sq"], n) - mv * mv)
        if w["sum_vol"]:
            o["vwap"] = float(F(w["notional"], w["sum_vol"]))
        if n + lost:
            o["lost_share"] = float(F(lost, n + lost))
        for k in range(K):
            lw = dict(zip(FLOW_LAG_FIELDS, (int(x) for x in r["lags"][k])))
            npair = lw["n_pairs"] & M
            if not npair:
                continue
            if mean is not None and mean * mean != 1:
                o["sign_acf"][k] = float((F(lw["sum_ss"], npair) - mean * mean) / (1 - mean * mean))
            o["response"][k] = float(F(lw["sum_resp"], npair))
            o["back_response"][k] = float(F(lw["sum_back"], npair))
            o["mean_abs_dp"][k] = float(F(lw["sum_abs_dp"] & M, npair))
            o["variogram"][k] = float(F(lw["sum_dp2"] & M, npair))
    return out


# bk_cross_row: one market's row of one span and one ordered pair of assets of the cross table (ManyMarketEnv.cross), 8 words
# of 8 bytes; bk_cross_config: n_spans and four spans, five u32
CROSS_FIELDS = ("n", "sum_x", "sum_y", "sum_xx", "sum_yy", "sum_xy", "n_lead", "sum_lead")
CROSS_SIGNED = ("sum_x", "sum_y", "sum_xy", "sum_lead")
CROSS_DTYPE = np.dtype(
    {"names": list(CROSS_FIELDS), "formats": ["<i8" if n in CROSS_SIGNED else "<u8" for n in CROSS_FIELDS],
     "offsets": [8 * i for i in range(8)], "itemsize": 64})
CROSS_CONFIG_DTYPE = np.dtype({"names": ["n_spans", "spans"], "formats": ["<u4", ("<u4", (4,))], "offsets": [0, 4], "itemsize": 20})
CROSS_MOMENTS_DTYPE = np.dtype([(n, "<f8") for n in ("n", "cov", "corr", "beta", "lead_corr")])


def cross_moments(rows) -> np.ndarray:
    """``CROSS_DTYPE`` rows of any shape (``ManyMarketEnv.cross()``: ``[markets, spans, a, b]``) -> float64 moments of the
    same shape (``CROSS_MOMENTS_DTYPE``), computed exactly in Python integers and rounded once.  With ``x`` and ``y`` the
    changes of TWICE the mid of assets ``a`` and ``b`` over the row's span, counted where both are defined:

    ``n`` the count; ``cov`` = (sum_xy / n - mean_x mean_y) / 4, the covariance of the two MID changes (each factor halved);
    ``corr`` = cov / sqrt(var_x var_y); ``beta`` = cov / var_y, the slope of a's change on b's; ``lead_corr`` =
    (sum_lead / n_lead - mean_x mean_y) / (4 sqrt(var_x var_y)), the correlation of a's change with b's PREVIOUS one - its
    normalisation borrows the contemporaneous means and standard deviations, those of the ``n`` steps, not of the ``n_lead``
    steps the product was summed over.  A division by a zero count or a zero variance gives NaN.  The words are read as they
    are: a sum that has wrapped modulo 2^64 is not detected."""
    from fractions import Fraction as F
    from math import sqrt

    rows = np.asarray(rows)
    if rows.dtype != CROSS_DTYPE:
        raise ValueError("cross_moments needs CROSS_DTYPE rows")
    out = np.full(rows.shape, np.nan, dtype=CROSS_MOMENTS_DTYPE)
    for r, o in zip(rows.reshape(-1), out.reshape(-1)):
        w = {n: int(r[n]) for n in CROSS_FIELDS}
        n = w["n"]
        o["n"] = float(n)
        if not n:
            continue
        mx, my = F(w["sum_x"], n), F(w["sum_y"], n)
        cov = (F(w["sum_xy"], n) - mx * my) / 4
        var_x, var_y = (F(w["sum_xx"], n) - mx * mx) / 4, (F(w["sum_yy"], n) - my * my) / 4
        o["cov"] = float(cov)
        if var_y:
            o["beta"] = float(cov / var_y)
        if var_x and var_y:
            sd = sqrt(float(var_x)) * sqrt(float(var_y))
            o["corr"] = float(cov) / sd
            if w["n_lead"]:
                o["lead_corr"] = float((F(w["sum_lead"], w["n_lead"]) - mx * my) / 4) / sd
    return out


# bk_bins_config: the configuration of the bin table (ManyBookEnv.enable_bins), nine u32
BINS_CONFIG_DTYPE = np.dtype(
    {"names": ["n_bins", "n_spans", "spans", "ret_width", "spread_width", "vol_width"],
     "formats": ["<u4", "<u4", ("<u4", (4,)), "<u4", "<u4", "<u4"], "offsets": [0, 4, 8, 24, 28, 32], "itemsize": 36})

def _bins_cfg(cfg):
    """(n_bins, spans, ret_width, spread_width, vol_width) of a ``BINS_CONFIG_DTYPE`` record or of a mapping with its names"""
    names = cfg.dtype.names if getattr(cfg, "dtype", None) is not None else tuple(cfg)
    spans = [int(k) for k in np.asarray(cfg["spans"]).reshape(-1)]
    if "n_spans" in names:  # (the record's four slots: only the first n_spans are used)
        spans = spans[:int(cfg["n_spans"])]
    return int(cfg["n_bins"]), tuple(spans), int(cfg["ret_width"]), int(cfg["spread_width"]), int(cfg["vol_width"])


def bin_edges(cfg) -> np.ndarray:
    """The LOWER edges of the bins of every channel of a bin table, float64 ``[n_spans + 2, n_bins]``; ``cfg`` is
    ``ManyBookEnv.bins_config()`` (a ``BINS_CONFIG_DTYPE`` record) or a mapping with ``n_bins``, ``spans``, ``ret_width``,
    ``spread_width`` and ``vol_width``.  A return channel's edges are in MID-PRICE units: bin ``i`` starts at
    ``(i - n_bins / 2) * ret_width / 2`` (the table counts the change of twice the mid); the spread's and the volume's bin
    ``i`` starts at ``i * width``.  Every bin is ``width`` wide (a return's ``ret_width / 2``), half-open at its upper edge;
    the first return bin also holds everything below it and the last bin of every channel everything above."""
    B, spans, rw, sw, vw = _bins_cfg(cfg)
    i = np.arange(B, dtype=np.float64)
    return np.stack([(i - B // 2) * rw / 2.0] * len(spans) + [i * float(sw), i * float(vw)])


def bin_quantiles(counts, edges, width, q) -> np.ndarray:
    """Quantiles of binned values: per row of ``counts [..., n_bins]`` and per ``q`` (a scalar or a sequence, each in
    (0, 1]) the UPPER edge ``edges[i] + width`` of the first bin ``i`` at which the cumulative share of the counts reaches
    ``q`` - so the ``inverted_cdf`` quantile of the values lies in ``[that - width, that)`` unless it was clamped into an end
    bin.  ``edges`` are the channel's lower edges (``bin_edges(cfg)[c]``), ``width`` its bin width in the same units
    (``ret_width / 2`` for a return channel).  Shape ``counts.shape[:-1] + np.shape(q)``; NaN where the total is zero.  The
    counts are summed in Python integers; ``q * total`` is one float product, as ``numpy.quantile`` forms its index."""
    counts = np.asarray(counts)
    edges = np.asarray(edges, dtype=np.float64)
    if counts.ndim < 1 or edges.shape != counts.shape[-1:]:
        raise ValueError("bin_quantiles needs counts [..., n_bins] and edges [n_bins]")
    qs = np.atleast_1d(np.asarray(q, dtype=np.float64))
    if ((qs <= 0) | (qs > 1)).any():
        raise ValueError("bin_quantiles needs 0 < q <= 1")
    out = np.full((int(np.prod(counts.shape[:-1], dtype=np.int64)), qs.size), np.nan)
    for r, row in enumerate(counts.reshape(-1, counts.shape[-1])):
        c = [int(x) for x in row]
        total = sum(c)
        if not total:
            continue
        for k, qq in enumerate(qs.reshape(-1)):
            need, cum = float(qq) * total, 0
            for i, x in enumerate(c):
                cum += x
                if cum >= need:
                    out[r, k] = edges[i] + width
                    break
    return out.reshape(counts.shape[:-1] + np.shape(q))


# bk_open_summary / bk_open_order: one trader's rows of the open-order tables (ManyBookEnv.open_orders)
OPEN_SUMMARY_DTYPE = np.dtype(
    {"names": ["bid_vol", "ask_vol", "n_bid", "n_ask", "best_bid", "best_ask"], "formats": ["<u8", "<u8", "<u4", "<u4", "<u4", "<u4"],
     "offsets": [0, 8, 16, 20, 24, 28], "itemsize": 32})
OPEN_ORDER_DTYPE = np.dtype(
    {"names": ["order_id", "price", "vol", "side_is_bid"], "formats": ["<u4", "<u4", "<u4", "<u4"],
     "offsets": [0, 4, 8, 12], "itemsize": 16})

# bk_open_queue: the queue position of one entry of the open-order tables (ManyBookEnv.open_queue)
OPEN_QUEUE_DTYPE = np.dtype(
    {"names": ["ahead_vol", "level_ahead_vol", "level_vol", "ahead_orders", "level_ahead_orders"],
     "formats": ["<u8", "<u8", "<u8", "<u4", "<u4"], "offsets": [0, 8, 16, 24, 28], "itemsize": 32})


class OpenQueue(C.Structure):
    """bk_open_queue: one row of the queue table."""
    _fields_ = [("ahead_vol", C.c_uint64), ("level_ahead_vol", C.c_uint64), ("level_vol", C.c_uint64),
                ("ahead_orders", C.c_uint32), ("level_ahead_orders", C.c_uint32)]


# bk_quote: one trader's row of ManyBookEnv.submit_quotes' table; QUOTE_KEEP (BK_QUOTE_KEEP) as a side's vol leaves it alone
QUOTE_DTYPE = np.dtype(
    {"names": ["bid_price", "bid_vol", "ask_price", "ask_vol"], "formats": ["<u4", "<u4", "<u4", "<u4"],
     "offsets": [0, 4, 8, 12], "itemsize": 16})
QUOTE_KEEP = 0xFFFFFFFF


class Quote(C.Structure):
    """bk_quote: one row of the quote table."""
    _fields_ = [("bid_price", C.c_uint32), ("bid_vol", C.c_uint32), ("ask_price", C.c_uint32), ("ask_vol", C.c_uint32)]


# bk_random_agents (RandomAgentsCfg) as a numpy structured dtype: the rows of ManyBookEnv.set_random_agents_per_book's table
RANDOM_AGENTS_DTYPE = np.dtype(
    {"names": ["n_agents", "tick_lo", "tick_hi", "vol_lo", "vol_hi", "tick_size", "activity_rate"],
     "formats": ["<u4", "<u4", "<u4", "<u4", "<u4", "<u4", "<f4"], "offsets": [0, 4, 8, 12, 16, 20, 24], "itemsize": 28})

# bk_agent_desc (AgentDesc) the same way: the rows of ManyBookEnv.retune_agents' table; as 4-byte words a row is 26 of them,
# so device code can address the fields of an int32 [n_units, n_members, 26] tensor (word = offset // 4)
AGENT_DESC_DTYPE = np.dtype(
    {"names": ["type", "n_agents", "tick_lo", "tick_hi", "vol_lo", "vol_hi", "tick_size", "activity_rate", "agent_id_start",
               "p_limit", "p_market", "p_cancel", "trade_vol", "reserved", "price_dist_mu", "price_dist_sigma", "decay",
               "demand", "scale", "order_ratio"],
     "formats": ["<u4", "<u4", "<u4", "<u4", "<u4", "<u4", "<u4", "<f4", "<u4", "<f4", "<f4", "<f4", "<u4", "<u4", "<f8", "<f8",
                 "<f8", "<f8", "<f8", "<f8"],
     "offsets": [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44, 48, 52, 56, 64, 72, 80, 88, 96], "itemsize": 104})


class IngressArrays(C.Structure):
    """bk_ingress_arrays: the pinned staging arrays of the next bk_submit_instructions_host call."""
    _fields_ = [("capacity", C.c_uint64), ("book_offsets", C.c_void_p), ("action", C.c_void_p), ("side", C.c_void_p),
                ("vol", C.c_void_p), ("trader_id", C.c_void_p), ("price", C.c_void_p), ("order_id", C.c_void_p)]


# every symbol include/bourse_amd.h declares: name -> (restype, argtypes)
_u64, _u32, _i32, _vp, _sz = C.c_uint64, C.c_uint32, C.c_int, C.c_void_p, C.c_size_t
_p64, _p32, _p8 = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
SIGNATURES = {
    "bk_last_error": (C.c_char_p, []),
    "bk_hip_versions": (_i32, [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "bk_device_count": (_i32, [C.POINTER(C.c_int)]),
    "bk_env_create": (_i32, [C.POINTER(Config), C.POINTER(_vp)]),
    "bk_env_destroy": (None, [_vp]),
    "bk_env_set_stream": (_i32, [_vp, _vp]),
    "bk_env_sync": (_i32, [_vp]),
    "bk_place_order": (_i32, [_vp, _u32, _i32, _u32, _u32, _i32, _u32, _p64]),
    "bk_cancel_order": (_i32, [_vp, _u32, _u64]),
    "bk_modify_order": (_i32, [_vp, _u32, _u64, _i32, _u32, _i32, _u32]),
    "bk_submit_instructions": (_i32, [_vp, _u32, _sz, _p32, _p8, _p32, _p32, _p32, _p64, _p64, C.POINTER(_sz)]),
    "bk_submit_instructions_csr": (_i32, [_vp, _p64, _p32, _p8, _p32, _p32, _p32, _p64, _p64, C.POINTER(_sz)]),
    "bk_enable_trading": (_i32, [_vp, _i32]),
    "bk_step": (_i32, [_vp]),
    "bk_device_ingress_enable": (_i32, [_vp, _u32]),
    "bk_submit_instructions_device": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "bk_step_async": (_i32, [_vp]),
    "bk_update_agents": (_i32, [_vp]),
    "bk_update_members": (_i32, [_vp]),
    "bk_update_market_agents": (_i32, [_vp]),
    "bk_update_market_members": (_i32, [_vp]),
    "bk_member_orders": (_i32, [_vp, _u32, _u32, _u32, _p64, _p32]),
    "bk_ingress_staging": (_i32, [_vp, _u64, C.POINTER(IngressArrays)]),
    "bk_submit_instructions_host": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _p64]),
    "bk_submit_result": (_i32, [_vp, _u64, _vp, _vp, _p32]),
    "bk_submit_result_view": (_i32, [_vp, _u64, C.POINTER(_vp), C.POINTER(_vp), _p32]),
    "bk_order_status": (_i32, [_vp, _u32, _u64, _p8]),
    "bk_order_count": (_i32, [_vp, _u32, _p64]),
    "bk_get_orders": (_i32, [_vp, _u32, _u64, _u64, _vp]),
    "bk_get_order_keys": (_i32, [_vp, _u32, _u64, _u64, _p32, _p64]),
    "bk_load_book": (_i32, [_vp, _u32, _u64, _u32, _u64, _vp, _p32, _p64, _u64, _vp]),
    "bk_set_random_agents": (_i32, [_vp, _u32, C.POINTER(RandomAgentsCfg)]),
    "bk_set_tick_sizes": (_i32, [_vp, _u32, _p32]),
    "bk_set_random_market_agents": (_i32, [_vp, _u32, C.POINTER(RandomAgentsCfg), _p32]),
    "bk_set_random_agents_per_book": (_i32, [_vp, _u32, _vp, _p32]),
    "bk_set_agents": (_i32, [_vp, _u32, C.POINTER(AgentDesc)]),
    "bk_set_agents_per_book": (_i32, [_vp, _u32, C.POINTER(AgentDesc), _p32]),
    "bk_retune_random_agents_device": (_i32, [_vp, _u32, _vp, _vp, _vp]),
    "bk_retune_random_agents": (_i32, [_vp, _u32, _vp, _vp]),
    "bk_retune_agents_device": (_i32, [_vp, _u32, _vp, _vp, _vp]),
    "bk_retune_agents": (_i32, [_vp, _u32, _vp, _vp]),
    "bk_retune_rejected": (_i32, [_vp, _p64]),
    "bk_set_market_agents": (_i32, [_vp, _u32, C.POINTER(AgentDesc), _p32]),
    "bk_run": (_i32, [_vp, _u64]),
    "bk_l2_width": (_u32, [_vp]),
    "bk_level2": (_i32, [_vp, _u32, _u32, _p32]),
    "bk_history_len": (_i32, [_vp, _p64, _p64]),
    "bk_history": (_i32, [_vp, _u64, _u64, _u32, _u32, _p32]),
    "bk_clear_history": (_i32, [_vp]),
    "bk_history_copy_async": (_i32, [_vp, _u64, _u64, _u32, _u32, _p32, _vp]),
    "bk_stream_create": (_i32, [C.POINTER(_vp)]),
    "bk_stream_sync": (_i32, [_vp]),
    "bk_stream_destroy": (_i32, [_vp]),
    "bk_pinned_alloc": (_i32, [_u64, C.POINTER(_vp)]),
    "bk_pinned_free": (_i32, [_vp]),
    "bk_trade_count": (_i32, [_vp, _u32, _p64, _p64]),
    "bk_trade_counts": (_i32, [_vp, _p64]),
    "bk_get_trades": (_i32, [_vp, _u32, _u64, _u64, _vp]),
    "bk_clear_trades": (_i32, [_vp]),
    "bk_trades_compact": (_i32, [_vp, _p64]),
    "bk_trades_compact_copy_async": (_i32, [_vp, _vp, _p64, _vp]),
    "bk_time": (_i32, [_vp, _u32, _p64]),
    "bk_set_time": (_i32, [_vp, _u32, _u64]),
    "bk_trade_vol": (_i32, [_vp, _u32, _p32]),
    "bk_steps_done": (_i32, [_vp, _p64]),
    "bk_book_flags": (_i32, [_vp, _p32]),
    "bk_clear_flags": (_i32, [_vp, _u32]),
    "bk_flags_summary": (_i32, [_vp, _p32, _p64]),
    "bk_warm": (_i32, [_vp, _u64]),
    "bk_set_agent_order_log": (_i32, [_vp, _i32]),
    "bk_rng_state": (_i32, [_vp, _u32, _p64]),
    "bk_live_orders": (_i32, [_vp, _u32, _u32, _vp, _p32]),
    "bk_stats_compute": (_i32, [_vp, C.POINTER(Stats)]),
    "bk_stats_device_ptr": (_i32, [_vp, C.POINTER(_vp)]),
    "bk_level2_device_ptr": (_i32, [_vp, C.POINTER(_vp)]),
    "bk_profile_enable": (_i32, [_vp, _i32]),
    "bk_profile_read": (_i32, [_vp, C.POINTER(C.c_double), _p64, _i32]),
    "bk_profile_read_kind": (_i32, [_vp, _i32, C.POINTER(C.c_double), _p64]),
    "bk_set_pipeline": (_i32, [_vp, _i32]),
    "bk_get_pipeline": (_i32, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "bk_state_bytes_per_book": (_u64, [_vp]),
    "bk_set_split_parts": (_i32, [_vp, _i32, _u32]),
    "bk_get_split_parts": (_i32, [_vp, C.POINTER(C.c_int), _p32]),
    "bk_set_wave_options": (_i32, [_vp, _u32, _i32]),
    "bk_pipeline_fallbacks": (_i32, [_vp, _p64]),
    "bk_order_counts": (_i32, [_vp, _p64]),
    "bk_event_steps_keyed": (_i32, [_vp, _p64]),
    "bk_stamp_compactions": (_i32, [_vp, _p64]),
    "bk_checkpoint_bytes": (_u64, [_vp]),
    "bk_checkpoint_save": (_i32, [_vp, _vp, _u64]),
    "bk_checkpoint_load": (_i32, [_vp, _vp, _u64]),
    "bk_snapshot_bytes": (_u64, [_vp]),
    "bk_snapshot_save": (_i32, [_vp, _u32]),
    "bk_snapshot_drop": (_i32, [_vp, _u32]),
    "bk_reset_books_device": (_i32, [_vp, _u32, _vp, _vp]),
    "bk_reset_books": (_i32, [_vp, _u32, _vp, _vp]),
    "bk_ingress_snapshot_save": (_i32, [_vp, _u32]),
    "bk_ingress_snapshot_drop": (_i32, [_vp, _u32]),
    "bk_ingress_snapshot_bytes": (_u64, [_vp, _u32]),
    "bk_ingress_reset_books_device": (_i32, [_vp, _u32, _vp, _vp]),
    "bk_ingress_reset_books": (_i32, [_vp, _u32, _vp, _vp]),
    "bk_accounts_enable": (_i32, [_vp, _u32, _i32]),
    "bk_accounts_device_ptr": (_i32, [_vp, C.POINTER(_vp)]),
    "bk_get_accounts": (_i32, [_vp, _u32, _u32, _vp]),
    "bk_accounts_clear": (_i32, [_vp, _vp]),
    "bk_accounts_clear_device": (_i32, [_vp, _vp]),
    "bk_trade_bars_enable": (_i32, [_vp, _u32, _i32]),
    "bk_trade_bars_device_ptr": (_i32, [_vp, C.POINTER(_vp)]),
    "bk_trade_bars_slot": (_i32, [_vp, C.POINTER(_u32)]),
    "bk_get_trade_bars": (_i32, [_vp, _u32, _u32, _vp]),
    "bk_trade_bars_clear": (_i32, [_vp, _vp]),
    "bk_trade_bars_clear_device": (_i32, [_vp, _vp]),
    "bk_series_enable": (_i32, [_vp]),
    "bk_series_fold": (_i32, [_vp]),
    "bk_series_clear": (_i32, [_vp, _vp]),
    "bk_series_clear_device": (_i32, [_vp, _vp]),
    "bk_series_device_ptr": (_i32, [_vp, C.POINTER(_vp)]),
    "bk_get_series": (_i32, [_vp, _u32, _u32, _vp]),
    "bk_depth_enable": (_i32, [_vp]),
    "bk_depth_device_ptr": (_i32, [_vp, C.POINTER(_vp)]),
    "bk_get_depth": (_i32, [_vp, _u32, _u32, _vp]),
    "bk_candles_enable": (_i32, [_vp, _u32, _u32]),
    "bk_candles_config_get": (_i32, [_vp, C.POINTER(_u32)]),
    "bk_candles_device_ptr": (_i32, [_vp, C.POINTER(_vp)]),
    "bk_get_candles": (_i32, [_vp, _u32, _u32, _vp]),
    "bk_lags_enable": (_i32, [_vp, _u32]),
    "bk_lags_fold": (_i32, [_vp]),
    "bk_lags_clear": (_i32, [_vp, _vp]),
    "bk_lags_clear_device": (_i32, [_vp, _vp]),
    "bk_lags_device_ptr": (_i32, [_vp, C.POINTER(_vp)]),
    "bk_get_lags": (_i32, [_vp, _u32, _u32, _vp]),
    "bk_bins_enable": (_i32, [_vp, _vp]),
    "bk_bins_config_get": (_i32, [_vp, _vp]),
    "bk_bins_fold": (_i32, [_vp]),
    "bk_bins_clear": (_i32, [_vp, _vp]),
    "bk_bins_clear_device": (_i32, [_vp, _vp]),
    "bk_bins_device_ptr": (_i32, [_vp, C.POINTER(_vp)]),
    "bk_get_bins": (_i32, [_vp, _u32, _u32, _vp]),
    "bk_cross_enable": (_i32, [_vp, _vp]),
    "bk_cross_config_get": (_i32, [_vp, _vp]),
    "bk_cross_fold": (_i32, [_vp]),
    "bk_cross_clear": (_i32, [_vp, _vp]),
    "bk_cross_clear_device": (_i32, [_vp, _vp]),
    "bk_cross_device_ptr": (_i32, [_vp, C.POINTER(_vp)]),
    "bk_get_cross": (_i32, [_vp, _u32, _u32, _vp]),
    "bk_flow_enable": (_i32, [_vp, _u32, _i32]),
    "bk_flow_fold": (_i32, [_vp]),
    "bk_flow_clear": (_i32, [_vp, _vp]),
    "bk_flow_clear_device": (_i32, [_vp, _vp]),
    "bk_flow_device_ptr": (_i32, [_vp, C.POINTER(_vp)]),
    "bk_flow_lags": (_i32, [_vp, _p32]),
    "bk_get_flow": (_i32, [_vp, _u32, _u32, _vp]),
    "bk_get_flow_state": (_i32, [_vp, _u32, _u32, _vp, _vp]),
    "bk_open_orders_enable": (_i32, [_vp, _u32, _u32]),
    "bk_open_orders_refresh": (_i32, [_vp]),
    "bk_open_orders_device_ptrs": (_i32, [_vp, C.POINTER(_vp), C.POINTER(_vp)]),
    "bk_get_open_orders": (_i32, [_vp, _u32, _u32, _vp, _vp]),
    "bk_open_queue_enable": (_i32, [_vp]),
    "bk_open_queue_device_ptr": (_i32, [_vp, C.POINTER(_vp)]),
    "bk_get_open_queue": (_i32, [_vp, _u32, _u32, _vp]),
    "bk_submit_quotes_device": (_i32, [_vp, _vp, _vp, _vp]),
    "bk_submit_quotes": (_i32, [_vp, _vp, _vp, _vp]),
}

_lib = None


def lib_path() -> str:
    return _build.LIB


def _share_torch_hip_runtime():
    """PyTorch's ROCm wheels bundle their own libamdhip64.so.7 - the SONAME of /opt/rocm's, which this library links.  A process
    gets ONE of the two (the first loaded), and torch does not find the GPU on the system's copy ("No HIP GPUs are available"
    when `import torch` comes AFTER this library's first use; the other order has always worked, and is what bench.py and the
    tests do).  So when torch is installed but not imported yet, its copy of the runtime is loaded first - without importing
    torch.  BOURSE_AMD_OWN_HIP_RUNTIME=1 skips this (a process that never imports torch then runs on /opt/rocm's runtime, as a
    plain C client of the library does)."""
    import importlib.util
    import sys

    if "torch" in sys.modules or os.environ.get("BOURSE_AMD_OWN_HIP_RUNTIME") == "1":
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    if not spec or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
            _note(f"HIP runtime: torch's bundled copy pre-loaded ({cand}); BOURSE_AMD_OWN_HIP_RUNTIME=1 keeps /opt/rocm's")
        except OSError as e:
            # (not loadable here: the library's own dependency resolves as before)
            _note(f"HIP runtime: torch's bundled copy could not be loaded ({e}); the library binds to its own dependency")


def _note(msg: str):
    if os.environ.get("BOURSE_AMD_VERBOSE"):
        import sys

        print("[bourse_amd] " + msg, file=sys.stderr)


def _check_runtime_version(L):
    """Which HIP runtime did the library bind to, and is it the major version it was built against?  (the
    pre-load above silently changes the runtime of every process that has torch installed.)  A mismatch of the major
    version warns; BOURSE_AMD_VERBOSE=1 prints both versions and the runtime's path."""
    try:
        built, run = C.c_int(0), C.c_int(0)
        if L.bk_hip_versions(C.byref(built), C.byref(run)) != 0:
            return
        path = "?"
        try:
            for line in open("/proc/self/maps"):
                if "libamdhip64" in line:
                    path = line.split()[-1]
                    break
        except OSError:
            pass
        _note(f"HIP runtime bound: version {run.value} at {path}; library built against {built.value}")
        if built.value // 10_000_000 != run.value // 10_000_000:
            import warnings

            warnings.warn(f"bourse_amd: built against HIP {built.value} but running on HIP runtime {run.value} ({path}); set "
                          f"BOURSE_AMD_OWN_HIP_RUNTIME=1 to keep the system runtime", RuntimeWarning)
    except Exception:  # noqa: BLE001  (diagnostics must never stop a load)
        pass


def load() -> C.CDLL:
    """Load libbourse_amd.so (building it first if hipcc is here and the sources are newer)."""
    global _lib
    if _lib is not None:
        return _lib
    _share_torch_hip_runtime()
    path = _build.LIB
    override = os.environ.get("BOURSE_AMD_LIBRARY")  # a variant build (scripts/asm_ab.sh); never rebuilt implicitly
    if override:
        if not os.path.exists(override):
            raise ImportError(f"bourse_amd: BOURSE_AMD_LIBRARY={override} does not exist")
        path = override
    elif _build.is_stale():
        try:
            _build.build()
        except Exception as e:  # no toolchain on this machine
            if not os.path.exists(path):
                raise ImportError(
                    f"bourse_amd: HIP extension {path} is missing and could not be built ({e}). "
                    "There is no CPU fallback."
                ) from e
    L = C.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(L, name)  # AttributeError = header/library mismatch: fail loudly
        fn.restype = res
        fn.argtypes = args
    L.bk_selftest_reduce.restype = _i32
    L.bk_selftest_reduce.argtypes = [_p32, _u32, _p32]
    L.bk_selftest_math.restype = _i32
    L.bk_selftest_math.argtypes = [_i32, C.POINTER(C.c_double), _u64, C.POINTER(C.c_double)]
    _lib = L
    _check_runtime_version(L)
    return L


def check(rc: int):
    if rc == BK_OK:
        return
    msg = load().bk_last_error().decode()
    if rc == BK_PRICE:
        raise ValueError(msg)  # reference: PyValueError(e.to_string()), rust/src/step_sim.rs:239-242
    if rc == BK_NO_DEVICE:
        raise NoDeviceError(rc, msg)
    if rc == BK_CAPACITY:
        raise CapacityError(rc, msg)
    if rc == BK_UNKNOWN_ORDER:
        raise IndexError(msg)
    raise BourseError(rc, msg)


def p32(a):
    return a.ctypes.data_as(_p32)


def p64(a):
    return a.ctypes.data_as(_p64)


def p8(a):
    return a.ctypes.data_as(_p8)
