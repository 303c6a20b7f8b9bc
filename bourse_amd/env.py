"""``ManyBookEnv``: B independent ``bourse_de::Env`` instances stepped in lockstep on one MI355X.

Host-side mirror of the reference's Rust surface for the hot path
(``Env`` crates/step_sim/src/env.rs:58-295, ``RandomAgents`` agents/random_agent.rs:48-120,
``sim_runner`` runner.rs:46-69), calling the HIP kernels through the C ABI
(include/bourse_amd.h).  Book ``b`` owns the RNG stream
``Xoroshiro128StarStar::seed_from_u64(seed + book_offset + b)``.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Iterable, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import AgentDesc, Config, RandomAgentsCfg, Stats, check

MAX_PRICE = 2**32 - 1


@dataclass(frozen=True)
class RandomAgents:
    """``RandomAgents::new(n_agents, tick_range, vol_range, tick_size, activity_rate)``
    (ref agents/random_agent.rs:67-81).  One instance describes one group, replicated per book."""

    n_agents: int
    tick_range: Tuple[int, int]
    vol_range: Tuple[int, int]
    tick_size: int
    activity_rate: float

    def as_tuple(self):
        return (self.n_agents, tuple(self.tick_range), tuple(self.vol_range), self.tick_size, self.activity_rate)


@dataclass(frozen=True)
class RandomMarketAgents:
    """``RandomMarketAgents::new(asset, n_agents, tick_range, vol_range, tick_size, activity_rate)``
    (ref agents/random_agent.rs:185-201): a RandomAgents group trading one asset of a market."""

    asset: int
    n_agents: int
    tick_range: Tuple[int, int]
    vol_range: Tuple[int, int]
    tick_size: int
    activity_rate: float

    def as_tuple(self):
        return (self.asset, self.n_agents, tuple(self.tick_range), tuple(self.vol_range), self.tick_size,
                self.activity_rate)


@dataclass(frozen=True)
class NoiseAgentParams:
    """ref crates/step_sim/src/agents/noise_agent.rs:24-46"""

    tick_size: int
    p_limit: float
    p_market: float
    p_cancel: float
    trade_vol: int
    price_dist_mu: float
    price_dist_sigma: float


@dataclass(frozen=True)
class NoiseAgent:
    """``NoiseAgent::new(agent_id_start, n_agents, params)`` (ref noise_agent.rs:110-123)."""

    agent_id_start: int
    n_agents: int
    params: NoiseAgentParams

    def as_tuple(self):
        return ("noise", self.agent_id_start, self.n_agents, dict(self.params.__dict__))


@dataclass(frozen=True)
class MomentumParams:
    """ref crates/step_sim/src/agents/momentum_agent.rs:24-60"""

    tick_size: int
    p_cancel: float
    trade_vol: int
    decay: float
    demand: float
    scale: float
    order_ratio: float
    price_dist_mu: float
    price_dist_sigma: float


@dataclass(frozen=True)
class MomentumAgent:
    """``MomentumAgent::new(agent_id_start, n_agents, params)`` (ref momentum_agent.rs:128-142)."""

    agent_id_start: int
    n_agents: int
    params: MomentumParams

    def as_tuple(self):
        return ("momentum", self.agent_id_start, self.n_agents, dict(self.params.__dict__))


_STICKY_MAGIC = b"BKSTICKY"  # trailer of ManyBookEnv.checkpoint(): flag bits already reported to a strict caller


# ---------------------------------------------------------------- what the entries ask of their arguments
def _is_dev(x) -> bool:
    """A device object - a torch tensor or anything with ``__cuda_array_interface__`` - and not a host array."""
    return hasattr(x, "data_ptr") or hasattr(x, "__cuda_array_interface__")


def _dev_count(x) -> int:
    """Elements of a device object."""
    return int(x.numel()) if hasattr(x, "numel") else int(np.prod(x.__cuda_array_interface__["shape"]))


def _dev_bytes(x) -> int:
    """Bytes of a device object, whatever its element type."""
    if hasattr(x, "data_ptr"):
        return _dev_count(x) * int(x.element_size())
    return _dev_count(x) * np.dtype(x.__cuda_array_interface__["typestr"]).itemsize


def _host_mask(mask, n: int, per: str, name: str = "mask") -> np.ndarray:
    """A host mask as the library reads it: contiguous uint8, ``n`` entries (``per``: what an entry stands for)."""
    m = np.ascontiguousarray(np.asarray(mask))
    if m.dtype != np.bool_ and m.dtype != np.uint8:
        raise ValueError("mask: a bool or uint8 array is needed")
    m = m.astype(np.uint8, copy=False)
    if m.shape != (n,):
        raise ValueError(f"{name}: {n} elements are needed ({per})")
    return m


def _raise_on_status(status, unit: str):
    """``check_status=True``: raise for the first book whose ``status`` pair ``{code, units applied}`` reports a failure -
    the reference's ``ValueError`` at a bad price, ``CapacityError`` otherwise.  ``unit`` words the message: ``"element"``
    of a batch (``submit_instructions_device``) or ``"grid position"`` (``submit_quotes``)."""
    st = status.cpu().numpy() if hasattr(status, "cpu") else np.asarray(status)
    st = st.reshape(-1, 2).view(np.uint32) if st.dtype.itemsize == 4 else st.reshape(-1, 2)
    bad = np.nonzero(st[:, 0])[0]
    if len(bad):
        b, code, applied = int(bad[0]), int(st[bad[0], 0]), int(st[bad[0], 1])
        if code == _lib.BK_PRICE:
            price = "a price of its batch" if unit == "element" else "a quoted price"
            raise ValueError(f"book {b}: {price} was not a multiple of the tick size "
                             f"({unit} {applied} of the book's batch; earlier {unit.split()[-1]}s are queued)")
        raise _lib.CapacityError(code, f"book {b}: event queue / id space exhausted after {applied} {unit}s")


class ManyBookEnv:
    """B books on one GPU.  ``Env::new(start_time, tick_size, step_size, trading)`` per book."""

    def __init__(self, n_books: int, seed: int, start_time: int, tick_size: int, step_size: int, trading: bool = True,
                 levels: int = 10, max_live_orders: int = 128, max_orders: int = 0, trade_capacity: int = 4096,
                 history_capacity: int = 0, book_offset: int = 0, device: int = 0, stream: Optional[int] = None,
                 assets: int = 1, tick_sizes: Optional[Sequence[int]] = None, strict: bool = True):
        self._L = _lib.load()
        # strict: step() and synchronous run() raise when a book NEWLY reports a capacity flag.  The reference's book is
        # unbounded (crates/order_book/src/orderbook.rs:113-115); here pool / trade-record / order-log capacities are
        # fixed, and an overflow must never pass silently.  strict=False leaves the sticky flags to flags().
        # The device flags stay sticky (flags() is the record); the exception reports each bit of each book ONCE: a
        # caller that catches it can keep stepping (clear_flags() re-arms it).  BK_FLAG_STEP_SIZE is a warning, not an
        # error: the reference's Env::step never checks the event count against step_size (env.rs:116-134).
        self.strict = bool(strict)
        self._flags_sticky = None    # per-book bits a strict check has reported and moved off the device (see raise_on_flags)
        self._warned_bits = 0        # warning-only bits (STEP_SIZE) already warned about: left on the device, not re-polled
        self.last_retained_trades = 0  # largest number of records a book retained at the last strict check
        cfg = Config()
        cfg.assets = int(assets)
        self.assets = max(1, int(assets))
        cfg.n_books, cfg.levels = int(n_books), int(levels)
        cfg.start_time, cfg.tick_size, cfg.step_size = int(start_time), int(tick_size), int(step_size)
        cfg.trading, cfg.seed, cfg.book_offset = int(bool(trading)), int(seed) & (2**64 - 1), int(book_offset)
        cfg.max_live_orders, cfg.max_orders = int(max_live_orders), int(max_orders)
        cfg.trade_capacity, cfg.history_capacity, cfg.device = int(trade_capacity), int(history_capacity), int(device)
        self.history_capacity = int(history_capacity)
        self._h = C.c_void_p()
        self.n_books, self.levels, self.tick_size = int(n_books), int(levels), int(tick_size)
        self.step_size, self.start_time = int(step_size), int(start_time)
        check(self._L.bk_env_create(C.byref(cfg), C.byref(self._h)))
        self.width = int(self._L.bk_l2_width(self._h))
        self._stream = None if stream is None else int(stream)  # (None: the env's own stream, which Python never sees)
        # the device-resident tables this env has enabled (0 / None / False: not enabled)
        self._n_traders = 0       # enable_accounts
        self._bars_window = 0     # enable_trade_bars
        self._series = False      # enable_series
        self._candles = None      # enable_candles: width, n_candles and where the series' cursor stood / stands
        self._n_lags = 0          # enable_lags
        self._flow_lags = 0       # enable_flow
        self._bins_shape = None   # enable_bins: (n_spans + 2, n_bins)
        self._cross_spans = 0     # ManyMarketEnv.enable_cross: n_spans
        self._open_shape = None   # enable_open_orders: (n_traders, depth)
        self._open_queue = False  # enable_open_queue: the queue table beside the open-order entries exists
        if stream is not None:
            check(self._L.bk_env_set_stream(self._h, C.c_void_p(stream)))
        if tick_sizes is not None:
            tk = np.asarray(list(tick_sizes), dtype=np.uint32)
            check(self._L.bk_set_tick_sizes(self._h, len(tk), _lib.p32(tk)))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._L.bk_env_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------ host-driven flow (Env methods)
    def place_order(self, book: int, bid: bool, vol: int, trader_id: int, price: Optional[int] = None) -> int:
        """``Env::place_order`` (env.rs:166-176); raises ValueError on a non-tick-multiple price."""
        out = C.c_uint64(0)
        check(self._L.bk_place_order(self._h, book, int(bool(bid)), int(vol), int(trader_id), int(price is not None),
                                     int(price if price is not None else 0), C.byref(out)))
        return int(out.value)

    def cancel_order(self, book: int, order_id: int):
        check(self._L.bk_cancel_order(self._h, book, int(order_id)))

    def modify_order(self, book: int, order_id: int, new_price: Optional[int] = None, new_vol: Optional[int] = None):
        check(self._L.bk_modify_order(self._h, book, int(order_id), int(new_price is not None), int(new_price or 0),
                                      int(new_vol is not None), int(new_vol or 0)))

    def submit_instructions(self, book: int, instructions) -> np.ndarray:
        """``StepEnvNumpy.submit_instructions`` (rust/src/step_sim_numpy.rs:233-275)."""
        action, sides, vols, traders, prices, order_ids = instructions
        action = np.ascontiguousarray(action, dtype=np.uint32)
        sides = np.ascontiguousarray(np.asarray(sides).astype(np.uint8))
        vols = np.ascontiguousarray(vols, dtype=np.uint32)
        traders = np.ascontiguousarray(traders, dtype=np.uint32)
        prices = np.ascontiguousarray(prices, dtype=np.uint32)
        order_ids = np.ascontiguousarray(order_ids, dtype=np.uint64)
        n = len(action)
        out = np.full(n, 2**64 - 1, dtype=np.uint64)
        done = C.c_size_t(0)
        check(self._L.bk_submit_instructions(self._h, book, n, _lib.p32(action), _lib.p8(sides), _lib.p32(vols),
                                             _lib.p32(traders), _lib.p32(prices), _lib.p64(order_ids),
                                             _lib.p64(out), C.byref(done)))
        return out

    def _host_batch(self, book_offsets, instructions):
        action, sides, vols, traders, prices, order_ids = instructions
        off = np.ascontiguousarray(book_offsets, dtype=np.uint64)
        if len(off) != self.n_books + 1:
            raise ValueError("book_offsets needs n_books + 1 entries")
        action = np.ascontiguousarray(action, dtype=np.uint32)
        sides = np.asarray(sides)
        sides = np.ascontiguousarray(sides if sides.dtype == np.uint8 else sides.astype(np.uint8))
        vols = np.ascontiguousarray(vols, dtype=np.uint32)
        traders = np.ascontiguousarray(traders, dtype=np.uint32)
        prices = np.ascontiguousarray(prices, dtype=np.uint32)
        order_ids = np.ascontiguousarray(order_ids, dtype=np.uint64)
        if not (len(action) == len(sides) == len(vols) == len(traders) == len(prices) == len(order_ids) == int(off[-1])):
            raise ValueError("instruction arrays must all have book_offsets[-1] elements")
        return off, action, sides, vols, traders, prices, order_ids

    def submit_instructions_all(self, book_offsets, instructions) -> np.ndarray:
        """``submit_instructions`` (rust/src/step_sim_numpy.rs:233-275) for every book in one call: book b's instructions
        are elements ``[book_offsets[b], book_offsets[b + 1])`` of the six HOST arrays; returns the ids (``2**64 - 1``
        for elements that created nothing).  On a device-ingress env the arrays travel pinned staging -> async upload ->
        ``k_ingest`` (``bk_submit_instructions_host``), and a book whose batch stopped at a bad price raises the
        reference's ``ValueError`` AFTER every book has been applied (books are independent; earlier elements of the failing
        book stay queued, as in the reference); otherwise the host half of ``Env`` walks them
        (``bk_submit_instructions_csr``: stops at the first bad price of any book)."""
        if getattr(self, "_device_ingress", False):
            out, status, bad = self.submit_result(self.submit_instructions_all_async(book_offsets, instructions))
            if bad is not None:  # (the lowest book with a code in `status`)
                _raise_on_status(status, "element")
            return out
        off, action, sides, vols, traders, prices, order_ids = self._host_batch(book_offsets, instructions)
        out = np.full(len(action), 2**64 - 1, dtype=np.uint64)
        done = C.c_size_t(0)
        check(self._L.bk_submit_instructions_csr(self._h, _lib.p64(off), _lib.p32(action), _lib.p8(sides), _lib.p32(vols),
                                                 _lib.p32(traders), _lib.p32(prices), _lib.p64(order_ids), _lib.p64(out),
                                                 C.byref(done)))
        return out

    def submit_instructions_all_async(self, book_offsets, instructions) -> int:
        """Device-ingress env: queue the host arrays (``bk_submit_instructions_host``) and return a TICKET at once; the ids
        and the per-book status are fetched later with ``submit_result(ticket)`` (two tickets may be in flight: the upload
        of one runs under the step kernel of the other).  Arrays obtained from ``ingress_staging()`` are uploaded in
        place, anything else is first copied to pinned memory by the library's host threads."""
        off, action, sides, vols, traders, prices, order_ids = self._host_batch(book_offsets, instructions)
        t = C.c_uint64(0)
        vp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
        check(self._L.bk_submit_instructions_host(self._h, vp(off), vp(action), vp(sides), vp(vols), vp(traders), vp(prices),
                                                  vp(order_ids), C.byref(t)))
        self._ticket_n = getattr(self, "_ticket_n", {})
        self._ticket_n[int(t.value)] = len(action)
        self._ticket_n.pop(int(t.value) - 2, None)
        return int(t.value)

    def submit_result(self, ticket: int, ids: bool = True, out: Optional[np.ndarray] = None, status: Optional[np.ndarray] = None,
                      view: bool = False):
        """(ids u64[n] or None, status u32[n_books, 2] = {code, elements applied}, lowest failing book or None) of a ticket.
        ``out`` / ``status``: arrays to fill instead of fresh ones (a loop that fetches every step saves their page faults).
        ``view=True``: no copy at all - read-only numpy views of the library's pinned staging, valid until two more submits."""
        n = getattr(self, "_ticket_n", {}).get(int(ticket))
        if n is None:  # not a ticket of this env, or two submits old: the library says which
            check(self._L.bk_submit_result(self._h, int(ticket), None, None, None))
            raise _lib.BourseError(_lib.BK_INVALID, f"ticket {ticket}: its element count is no longer known")
        if view:
            pi, ps, bad = C.c_void_p(0), C.c_void_p(0), C.c_uint32(0)
            check(self._L.bk_submit_result_view(self._h, int(ticket), C.byref(pi), C.byref(ps), C.byref(bad)))

            def ro(ptr, dtype, count, shape):
                if count == 0:
                    return np.zeros(shape, dtype=dtype)
                a = np.frombuffer((C.c_char * (count * np.dtype(dtype).itemsize)).from_address(ptr), dtype=dtype, count=count).reshape(shape)
                a.flags.writeable = False
                return a

            return ((ro(pi.value, np.uint64, n, (n,)) if ids else None), ro(ps.value, np.uint32, 2 * self.n_books, (self.n_books, 2)),
                    (None if bad.value == 0xFFFFFFFF else int(bad.value)))
        if ids:
            if out is None:
                out = np.empty(n, dtype=np.uint64)
            elif out.dtype != np.uint64 or not out.flags.c_contiguous or len(out) < n:
                raise ValueError("out: a contiguous uint64 array of at least the ticket's element count")
        if status is None:
            status = np.empty((self.n_books, 2), dtype=np.uint32)
        elif status.dtype != np.uint32 or not status.flags.c_contiguous or status.size != 2 * self.n_books:
            raise ValueError("status: a contiguous uint32 array of 2 x n_books")
        bad = C.c_uint32(0)
        check(self._L.bk_submit_result(self._h, int(ticket), C.c_void_p(out.ctypes.data) if ids and n else None,
                                       C.c_void_p(status.ctypes.data), C.byref(bad)))
        return (out[:n] if ids else None), status, (None if bad.value == 0xFFFFFFFF else int(bad.value))

    def ingress_staging(self, min_elements: int) -> dict:
        """Pinned staging arrays of the NEXT ``submit_instructions_all(_async)`` call (``bk_ingress_staging``), as numpy
        views: ``book_offsets`` u64[n_books + 1], ``action`` / ``vol`` / ``trader_id`` / ``price`` u32, ``side`` u8,
        ``order_id`` u64, each of ``capacity >= min_elements`` elements.  Fill them in place and pass slices of THESE arrays
        to the submit call: they are uploaded without a host copy.  Valid until that submit returns."""
        a = _lib.IngressArrays()
        check(self._L.bk_ingress_staging(self._h, int(min_elements), C.byref(a)))
        cap = int(a.capacity)

        def view(ptr, dtype, n):
            buf = (C.c_char * (n * np.dtype(dtype).itemsize)).from_address(ptr)
            return np.frombuffer(buf, dtype=dtype, count=n)

        return {"capacity": cap, "book_offsets": view(a.book_offsets, np.uint64, self.n_books + 1),
                "action": view(a.action, np.uint32, cap), "side": view(a.side, np.uint8, cap),
                "vol": view(a.vol, np.uint32, cap), "trader_id": view(a.trader_id, np.uint32, cap),
                "price": view(a.price, np.uint32, cap), "order_id": view(a.order_id, np.uint64, cap)}

    def enable_trading(self):
        check(self._L.bk_enable_trading(self._h, 1))

    def disable_trading(self):
        check(self._L.bk_enable_trading(self._h, 0))

    def step(self, sync: bool = True):
        """``Env::step`` (env.rs:116-135) for every book over the queued events.  ``sync=False`` (device-resident
        ingress only): queue the step on the env's stream and return (no flag check)."""
        if not sync:
            check(self._L.bk_step_async(self._h))
            return
        check(self._L.bk_step(self._h))
        if self.strict:
            self.raise_on_flags()

    def update_agents(self, sync: bool = True):
        """``agents.update(env, rng)`` (random_agent.rs:85-119) of the installed RandomAgents for every book into the
        device-resident queues (``bk_update_agents``): the agents' placements and cancellations join the submitted
        instructions in call order, drawn from the book's own RNG, and the next ``step()`` trades all of it.  Needs
        ``enable_device_ingress()`` first, then ``set_random_agents`` / ``set_random_agents_per_book``.  ``sync=False``:
        queue it on the env's stream and return (no flag check), like ``step(sync=False)``."""
        check(self._L.bk_update_agents(self._h))
        if sync:
            self.sync()
            if self.strict:
                self.raise_on_flags()

    def update_members(self, sync: bool = True):
        """``agents.update(env, rng)`` of the installed AgentSet - NoiseAgent / MomentumAgent members (noise_agent.rs:127-176,
        momentum_agent.rs:146-208), with or without RandomAgents members, in declaration order - for every book into the
        device-resident queues (``bk_update_members``): the members' placements and cancellations join the submitted
        instructions in call order, drawn from the book's own RNG, and the next ``step()`` trades all of it.  Needs
        ``enable_device_ingress()`` first, then ``set_agents`` / ``set_agents_per_book`` (an all-RandomAgents set is
        ``update_agents``').  ``sync=False``: queue it on the env's stream and return (no flag check)."""
        check(self._L.bk_update_members(self._h))
        if sync:
            self.sync()
            if self.strict:
                self.raise_on_flags()

    def update_market_agents(self, sync: bool = True):
        """``RandomMarketAgents::update`` (random_agent.rs:204-245) of the groups of ``set_random_market_agents`` /
        ``set_random_market_agents_per_market`` for every market into the market's device-resident queue
        (``bk_update_market_agents``): a group of asset ``a`` cancels and places on book ``market * assets + a``, with the
        market's own RNG, and its events join the submitted instructions in call order; the next ``step()`` trades all of
        it.  Needs ``enable_device_ingress()`` first, then the agents.  On an env of one asset it shares the held ids with
        ``update_agents``.  ``sync=False``: queue it on the env's stream and return (no flag check)."""
        check(self._L.bk_update_market_agents(self._h))
        if sync:
            self.sync()
            if self.strict:
                self.raise_on_flags()

    def update_market_members(self, sync: bool = True):
        """``MarketAgent::update`` of the set of ``set_market_agents`` / ``set_market_agents_per_market`` - NoiseMarketAgent
        (noise_agent.rs:226-340), MomentumMarketAgent (momentum_agent.rs:282-397) and RandomMarketAgents members, in
        declaration order - for every market into the market's device-resident queue (``bk_update_market_members``), each
        member on the book of its asset.  Needs ``enable_device_ingress()`` first, then the set (an all-RandomAgents set is
        ``update_market_agents``').  On an env of one asset it shares the lists and the momentum state with
        ``update_members``.  ``sync=False``: queue it on the env's stream and return (no flag check)."""
        check(self._L.bk_update_market_members(self._h))
        if sync:
            self.sync()
            if self.strict:
                self.raise_on_flags()

    def member_orders(self, book: int, member: int) -> np.ndarray:
        """Member ``member``'s ``orders`` vector of one book after the last ``update_members`` (``bk_member_orders``), u64
        in list order; for a RandomAgents member the ids its agents hold, ``2**64 - 1`` for None.  On a market it is the
        list of market ``book // assets``, whose ids are ids of the member's asset's book."""
        n = C.c_uint32(0)
        check(self._L.bk_member_orders(self._h, int(book), int(member), 0, None, C.byref(n)))
        out = np.zeros(max(int(n.value), 1), dtype=np.uint64)
        check(self._L.bk_member_orders(self._h, int(book), int(member), int(n.value), _lib.p64(out), C.byref(n)))
        return out[:int(n.value)]

    # ------------------------------------------------------------ device-resident instruction ingress
    def enable_device_ingress(self, queue_capacity: int = 256):
        """Switch this (fresh) env to instructions submitted FROM DEVICE MEMORY (``bk_device_ingress_enable``): at most
        ``queue_capacity`` events per book (market) and step."""
        check(self._L.bk_device_ingress_enable(self._h, int(queue_capacity)))
        self._device_ingress = True

    @staticmethod
    def _dev_ptr(x, itemsize, name):
        """Device pointer of a torch CUDA tensor / anything with ``__cuda_array_interface__`` (contiguous, right width)."""
        if x is None:
            return None
        if hasattr(x, "data_ptr"):  # torch
            if not x.is_cuda or not x.is_contiguous() or x.element_size() != itemsize:
                raise ValueError(f"{name}: a contiguous CUDA tensor of {itemsize}-byte elements is needed")
            return C.c_void_p(x.data_ptr())
        cai = getattr(x, "__cuda_array_interface__", None)
        if cai is None or cai.get("strides") or np.dtype(cai["typestr"]).itemsize != itemsize:
            raise ValueError(f"{name}: a contiguous device array of {itemsize}-byte elements is needed")
        return C.c_void_p(cai["data"][0])

    def _device_ptr(self, entry) -> int:
        """The device address a ``bk_*_device_ptr`` entry hands out."""
        out = C.c_void_p()
        check(entry(self._h, C.byref(out)))
        return int(out.value)

    def _book_range(self, first_book: int, n_books: Optional[int]) -> Tuple[int, int]:
        """``(first, n)`` of the readers' book range; ``n_books=None``: to the last book.  (The library checks the end.)"""
        first = int(first_book)
        n = self.n_books - first if n_books is None else int(n_books)
        if first < 0 or n < 0:
            raise ValueError("book range out of bounds")
        return first, n

    def _book_rows(self, entry, first_book: int, n_books: Optional[int], *tables):
        """The rows of a book range from a ``bk_get_*`` entry: one zeroed array ``[n, *shape]`` per ``(shape, dtype)`` of
        ``tables`` for the entry to fill (``None``: a table this env does not keep - the entry is handed a null pointer)."""
        first, n = self._book_range(first_book, n_books)
        outs = [None if t is None else np.zeros((n,) + tuple(t[0]), dtype=t[1]) for t in tables]
        check(entry(self._h, first, n, *(None if o is None else o.ctypes.data_as(C.c_void_p) for o in outs)))
        return outs

    def _masked_clear(self, device_entry, host_entry, mask, sync, n: Optional[int] = None, per: str = "one per book"):
        """``clear_accounts``' ``mask`` / ``sync`` for any per-book table: ``None``, a device object or a host array
        (``n``, ``per``: the entries of a table whose unit is not the book)."""
        n = self.n_books if n is None else n
        if mask is None:
            check(device_entry(self._h, None))
        elif _is_dev(mask):
            if _dev_count(mask) != n:
                raise ValueError(f"mask: {n} elements are needed ({per})")
            check(device_entry(self._h, self._dev_ptr(mask, 1, "mask")))
        else:
            m = _host_mask(mask, n, per)
            check(host_entry(self._h, m.ctypes.data_as(C.c_void_p)))
        if sync:
            self.sync()

    def submit_instructions_device(self, book_offsets, action, side, vol, trader_id, price, order_id, out_ids=None,
                                   status=None, check_status: bool = False):
        """``submit_instructions`` (rust/src/step_sim_numpy.rs:233-275) for every book from DEVICE arrays, nothing passing
        through the host: book ``b``'s instructions are elements ``[book_offsets[b], book_offsets[b+1])``.  Arguments are
        torch CUDA tensors (or any ``__cuda_array_interface__`` object): ``book_offsets`` 8-byte ints (n_books + 1),
        ``action`` / ``vol`` / ``trader_id`` / ``price`` 4-byte ints, ``side`` 1-byte (bool / uint8), ``order_id`` 8-byte.
        ``out_ids`` (8-byte, one per element) receives the created ids (2**64 - 1 elsewhere), ``status`` (4-byte,
        2 per book) ``{code, elements applied}``.  Queued on the env's stream - which must be the stream the arrays were
        written on (``ManyBookEnv(stream=torch.cuda.current_stream().cuda_stream)``).  ``check_status=True`` waits and
        raises the reference's ``ValueError`` for the first book whose batch stopped at a bad price."""
        P = self._dev_ptr
        off_ptr = P(book_offsets, 8, "book_offsets")  # (validates the first argument before anything is looked at)
        if action is None:
            raise ValueError("action: a contiguous CUDA tensor of 4-byte elements is needed")
        if _dev_count(action) == 0:  # nothing to submit for any book (an empty device array has no address to hand over)
            if status is not None and hasattr(status, "zero_"):
                status.zero_()
            return out_ids, status
        check(self._L.bk_submit_instructions_device(self._h, off_ptr, P(action, 4, "action"),
                                                    P(side, 1, "side"), P(vol, 4, "vol"), P(trader_id, 4, "trader_id"),
                                                    P(price, 4, "price"), P(order_id, 8, "order_id"), P(out_ids, 8, "out_ids"),
                                                    P(status, 4, "status")))
        if check_status:
            if status is None:
                raise ValueError("check_status needs a status array")
            self.sync()
            _raise_on_status(status, "element")
        return out_ids, status

    def flags_summary(self) -> Tuple[int, int]:
        """(OR of every book's sticky flags, largest number of trade records a book retains): one small reduction on
        the device and an 8-byte copy - what the strict checks poll instead of the per-book array."""
        f, r = C.c_uint32(0), C.c_uint64(0)
        check(self._L.bk_flags_summary(self._h, C.byref(f), C.byref(r)))
        return int(f.value), int(r.value)

    def clear_flags(self, mask: int = 0xFFFFFFFF):
        """Clear sticky flag bits (on the device and in the host-side record of the bits already reported)."""
        check(self._L.bk_clear_flags(self._h, int(mask) & 0xFFFFFFFF))
        if self._flags_sticky is not None:
            self._flags_sticky &= np.uint32(~int(mask) & 0xFFFFFFFF)
        self._warned_bits &= ~int(mask) & 0xFFFFFFFF

    def raise_on_flags(self, mask: Optional[int] = None):
        """Raise ``CapacityError`` (capacity bits) / ``BourseError`` (price-tick) for flag bits in ``mask`` that a book
        carries (default mask: every flag except UNKNOWN_ORDER, which ``step`` reports itself).  A STEP_SIZE bit alone
        only warns: the reference tolerates such a step.  Reported bits MOVE from the device to a host-side sticky record
        (``flags()`` returns both): the two-word summary reads 0 again, so the next check stays cheap, and a book that
        overflows AGAIN after the caller caught the error is reported again instead of passing silently."""
        import warnings

        m = (~_lib.FLAG_UNKNOWN_ORDER & 0xFFFFFFFF) if mask is None else (int(mask) & 0xFFFFFFFF)
        # The warning-only STEP_SIZE bit STAYS on the device once it has been warned about: a workload that regularly queues
        # >= step_size events (which the reference tolerates) would otherwise re-set it every step, and every strict step
        # would fetch the per-book array, launch the clear kernel and warn again.  clear_flags() re-arms the warning.
        m &= ~self._warned_bits & 0xFFFFFFFF
        any_or, self.last_retained_trades = self.flags_summary()
        if not (any_or & m):
            return  # nothing set anywhere (the common case): the per-book array is not fetched
        f = np.zeros(self.n_books, dtype=np.uint32)
        check(self._L.bk_book_flags(self._h, _lib.p32(f)))
        new = f & np.uint32(m)
        if not new.any():
            return
        bits = int(np.bitwise_or.reduce(new))
        self._warned_bits |= bits & _lib.FLAG_STEP_SIZE
        moved = bits & ~_lib.FLAG_STEP_SIZE & 0xFFFFFFFF  # error bits move to the host-side record; the warning bit does not
        if moved:
            if self._flags_sticky is None:
                self._flags_sticky = np.zeros_like(f)
            self._flags_sticky |= new & np.uint32(moved)
            check(self._L.bk_clear_flags(self._h, moved))
        books = np.nonzero(new)[0]
        names = "; ".join(n for b, n in _lib.FLAG_NAMES.items() if bits & b)
        msg = f"{len(books)} book(s) flagged (first: book {int(books[0])}): {names}"
        if bits & _lib.CAPACITY_FLAGS:
            raise _lib.CapacityError(_lib.BK_CAPACITY, msg)
        if bits & ~_lib.FLAG_STEP_SIZE:
            raise _lib.BourseError(_lib.BK_INVALID, msg)
        warnings.warn(f"bourse_amd: {msg} (price-time keys of that step may collide; the reference does not check this)",
                      RuntimeWarning, stacklevel=3)

    def order_status(self, book: int, order_id: int) -> int:
        out = C.c_uint8(0)
        check(self._L.bk_order_status(self._h, book, int(order_id), C.byref(out)))
        return int(out.value)

    def order_count(self, book: int) -> int:
        out = C.c_uint64(0)
        check(self._L.bk_order_count(self._h, book, C.byref(out)))
        return int(out.value)

    def orders(self, book: int) -> np.ndarray:
        n = self.order_count(book)
        a = np.zeros(n, dtype=_lib.ORDER_DTYPE)
        if n:
            check(self._L.bk_get_orders(self._h, book, 0, n, a.ctypes.data_as(C.c_void_p)))
        return a

    def order_keys(self, book: int) -> Tuple[np.ndarray, np.ndarray]:
        """``OrderEntry.key`` of every order (orderbook.rs:34-39) as (key price, key time)."""
        n = self.order_count(book)
        kp, kt = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint64)
        if n:
            check(self._L.bk_get_order_keys(self._h, book, 0, n, _lib.p32(kp), _lib.p64(kt)))
        return kp, kt

    # ------------------------------------------------------------ JSON snapshots (serde layout of the reference)
    def book_state(self, book: int, trading: bool = True, trade_vol: Optional[int] = None, trades=None) -> dict:
        """The book as ``serde_json`` serialises ``OrderBook`` (orderbook.rs:93-112: t, tick_size, trade_vol, orders
        [{order, key}], trades, trading; ask_side / bid_side are skipped and rebuilt on load, :891-918)."""
        side = {1: "Bid", 0: "Ask"}
        status = ["New", "Active", "Filled", "Cancelled", "Rejected"]  # types.rs:51-63
        o, (kp, kt) = self.orders(book), self.order_keys(book)
        orders = []
        for r, p, t in zip(o, kp.tolist(), kt.tolist()):
            bid = int(r["side"])
            orders.append({
                "order": {"side": side[bid], "status": status[int(r["status"])], "arr_time": int(r["arr_time"]),
                          "end_time": int(r["end_time"]), "vol": int(r["vol"]), "start_vol": int(r["start_vol"]),
                          "price": int(r["price"]), "trader_id": int(r["trader_id"]), "order_id": int(r["order_id"])},
                "key": [side[bid], (MAX_PRICE - p) if bid else p, t],  # price_key, side.rs:300-313
            })
        trades = [{"t": int(r["t"]), "side": side[int(r["side"])], "price": int(r["price"]), "vol": int(r["vol"]),
                   "active_order_id": int(r["active_id"]), "passive_order_id": int(r["passive_id"])}
                  for r in (self.trades(book, first=0) if trades is None else trades)]
        tick = self.tick_sizes[book % self.assets] if hasattr(self, "tick_sizes") else self.tick_size
        return {"t": self.time(book), "tick_size": int(tick),
                "trade_vol": self.trade_vol(book) if trade_vol is None else int(trade_vol), "orders": orders,
                "trades": trades, "trading": bool(trading)}

    def load_book_state(self, book: int, state: dict):
        """``TryFrom<OrderBookState>`` (orderbook.rs:891-918) for one book of this env (same tick size)."""
        side = {"Bid": 1, "Ask": 0}
        status = {"New": 0, "Active": 1, "Filled": 2, "Cancelled": 3, "Rejected": 4}
        tick = self.tick_sizes[book % self.assets] if hasattr(self, "tick_sizes") else self.tick_size
        if int(state["tick_size"]) != tick:
            raise ValueError("snapshot tick_size differs from the book's")
        n = len(state["orders"])
        o = np.zeros(n, dtype=_lib.ORDER_DTYPE)
        kp, kt = np.zeros(max(n, 1), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.uint64)
        for i, e in enumerate(state["orders"]):
            r, k = e["order"], e["key"]
            bid = side[r["side"]]
            o[i] = (bid, status[r["status"]], r["arr_time"], r["end_time"], r["vol"], r["start_vol"], r["price"],
                    r["trader_id"], r["order_id"])
            kp[i] = (MAX_PRICE - k[1]) if side[k[0]] else k[1]
            kt[i] = k[2]
        t = np.zeros(len(state["trades"]), dtype=_lib.TRADE_DTYPE)
        for i, r in enumerate(state["trades"]):
            t[i] = (r["t"], side[r["side"]], r["price"], r["vol"], r["active_order_id"], r["passive_order_id"])
        check(self._L.bk_load_book(self._h, book, int(state["t"]), int(state["trade_vol"]), n,
                                   o.ctypes.data_as(C.c_void_p), _lib.p32(kp), _lib.p64(kt), len(t),
                                   t.ctypes.data_as(C.c_void_p)))

    # ------------------------------------------------------------ on-device flow
    def set_random_agents(self, groups: Iterable[RandomAgents | tuple]):
        gs = [g.as_tuple() if isinstance(g, RandomAgents) else g for g in groups]
        arr = (RandomAgentsCfg * max(len(gs), 1))()
        for i, (n, tr, vr, ts, rate) in enumerate(gs):
            arr[i].n_agents, arr[i].tick_lo, arr[i].tick_hi = int(n), int(tr[0]), int(tr[1])
            arr[i].vol_lo, arr[i].vol_hi, arr[i].tick_size = int(vr[0]), int(vr[1]), int(ts)
            arr[i].activity_rate = float(np.float32(rate))
        check(self._L.bk_set_random_agents(self._h, len(gs), arr))
        self.groups = gs

    def set_random_market_agents(self, groups: Iterable["RandomMarketAgents | tuple"]):
        """A ``MarketAgentSet`` of ``RandomMarketAgents`` groups ``(asset, n, tick_range, vol_range, tick_size, rate)``,
        identical for every market (needs ``assets > 1`` books per market)."""
        gs = [g.as_tuple() if isinstance(g, RandomMarketAgents) else g for g in groups]
        arr = (RandomAgentsCfg * max(len(gs), 1))()
        assets = np.zeros(max(len(gs), 1), dtype=np.uint32)
        for i, (asset, n, tr, vr, ts, rate) in enumerate(gs):
            assets[i] = int(asset)
            arr[i].n_agents, arr[i].tick_lo, arr[i].tick_hi = int(n), int(tr[0]), int(tr[1])
            arr[i].vol_lo, arr[i].vol_hi, arr[i].tick_size = int(vr[0]), int(vr[1]), int(ts)
            arr[i].activity_rate = float(np.float32(rate))
        check(self._L.bk_set_random_market_agents(self._h, len(gs), arr, _lib.p32(assets)))
        self.groups = gs

    def set_random_agents_per_book(self, table):
        """RandomAgents groups whose parameters differ per book (``bk_set_random_agents_per_book``): book ``b`` steps as
        book ``b`` of an env given ``set_random_agents(table[b])`` does, bit for bit.  ``table`` is a sequence of
        ``n_books`` group lists shaped like ``set_random_agents``' argument, or a numpy structured array
        ``(n_books, n_groups)`` of ``RANDOM_AGENTS_DTYPE``.  ``n_agents`` must be the same in every book; tick and
        volume ranges, tick size and activity rate may differ.  A later ``set_random_agents`` / ``set_agents`` replaces
        the table."""
        if self.assets > 1:
            raise ValueError("markets take set_random_market_agents_per_market")
        arr = _agents_table(table, self.n_books, lambda g: g.as_tuple() if isinstance(g, RandomAgents) else g)
        check(self._L.bk_set_random_agents_per_book(self._h, arr.shape[1], arr.ctypes.data_as(C.c_void_p), None))
        self.groups = None

    def set_agents(self, members, assets=None):
        """A ``#[derive(AgentSet)]`` struct: members updated in declaration order (ref crates/macros/src/lib.rs:57-73).
        Each member is a RandomAgents / NoiseAgent / MomentumAgent instance or the equivalent tuple
        ``("random", n, tick_range, vol_range, tick_size, rate)`` / ``("noise"|"momentum", id_start, n, params_dict)``."""
        ms = [_member_tuple(m) for m in members]
        arr = (AgentDesc * max(len(ms), 1))()
        for i, m in enumerate(ms):
            _fill_agent_desc(arr[i], m)
        if assets is not None:
            as_arr = np.asarray(list(assets), dtype=np.uint32)
            check(self._L.bk_set_market_agents(self._h, len(ms), arr, _lib.p32(as_arr)))
        else:
            check(self._L.bk_set_agents(self._h, len(ms), arr))
        self.members = ms

    def set_agents_per_book(self, table):
        """AgentSet members whose parameters differ per book (``bk_set_agents_per_book``): book ``b`` steps as book ``b``
        of an env given ``set_agents(table[b])`` does, bit for bit.  ``table`` holds ``n_books`` member lists in
        ``set_agents``' tuple or instance format.  The members' kinds and ``n`` must be the same in every book; every
        other parameter may differ.  A later ``set_agents`` / ``set_random_agents`` / ``set_random_agents_per_book``
        replaces the table."""
        if self.assets > 1:
            raise ValueError("markets take set_market_agents_per_market")
        self._set_members_table(table, self.n_books, None)

    def _set_members_table(self, table, n_units: int, assets):
        rows = [[_member_tuple(m) for m in row] for row in table]
        if len(rows) != n_units:
            raise ValueError(f"the table needs one row of members per unit: {n_units} rows, got {len(rows)}")
        n = len(rows[0]) if rows else 0
        if n == 0 or any(len(r) != n for r in rows):
            raise ValueError("every row of the table needs the same number (>= 1) of members")
        arr = _members_array(rows, n_units)
        as_arr = None if assets is None else np.asarray(assets, dtype=np.uint32)
        check(self._L.bk_set_agents_per_book(self._h, n, arr, None if as_arr is None else _lib.p32(as_arr)))
        self.members = None

    # ------------------------------------------------------------ retune: the installed per-unit table, in place
    def retune_random_agents(self, table, mask=None, status=None, sync: bool = True):
        """Replace the RandomAgents parameters of the books ``mask`` names in the table ``set_random_agents_per_book``
        installed, in place on the device (``bk_retune_random_agents`` / ``bk_retune_random_agents_device``): the same
        agents, holding the same resting orders, draw from the new ``activity_rate``, ranges and tick size from the next
        ``run`` / ``update_agents`` on.  Nothing else changes - books, RNG states, held ids, snapshots and checkpoints (which
        hold no parameters: a reset or restore brings none back).  ``n_agents`` must stay what was installed.

        ``table``: what ``set_random_agents_per_book`` takes (the host entry: every masked book is checked first, and
        on the first bad entry nothing changes and the install's error is raised) - or a torch CUDA tensor /
        ``__cuda_array_interface__`` object of the raw ``RANDOM_AGENTS_DTYPE`` rows ``[n_books, n_groups]`` (28 B each,
        e.g. an int32 ``[n_books, n_groups, 7]`` tensor) written on the env's stream (the device entry: nothing passes
        through the host, a book with a bad entry keeps its whole row).  ``mask`` (bool / uint8 per book, ``None`` = every
        book) and ``status`` (4-byte ints, 2 per book: ``{code, first failing group}``) must be the same kind of object as
        the table.  ``retune_rejected()`` counts the refused books.  Queued on the env's stream; ``sync`` waits for it."""
        if self.assets > 1:
            raise ValueError("markets take retune_random_market_agents")
        self._retune(False, table, mask, status, sync,
                     lambda t: _agents_table(t, self.n_books, lambda g: g.as_tuple() if isinstance(g, RandomAgents) else g))

    def retune_agents(self, table, mask=None, status=None, sync: bool = True):
        """``retune_random_agents`` for the members' table ``set_agents_per_book`` installed (``bk_retune_agents`` /
        ``bk_retune_agents_device``): the masked books' Noise / Momentum / RandomAgents members keep their order lists and
        momentum state and take the new parameters.  A member's kind, ``n`` and ``agent_id_start`` must stay what was
        installed.  ``table``: ``n_books`` member lists as ``set_agents_per_book`` takes them or a structured array of
        ``AGENT_DESC_DTYPE`` (host), or a device object of the raw rows ``[n_books, n_members]`` (104 B each, e.g. an int32
        ``[n_books, n_members, 26]`` tensor)."""
        if self.assets > 1:
            raise ValueError("markets take retune_market_agents")
        self._retune(True, table, mask, status, sync, lambda t: _members_rows(t, self.n_books))

    def retune_rejected(self) -> int:
        """Units (books, or markets) the retunes of this env have refused so far (``bk_retune_rejected``); waits for the
        env's stream."""
        n = C.c_uint64(0)
        check(self._L.bk_retune_rejected(self._h, C.byref(n)))
        return int(n.value)

    def _retune(self, members: bool, table, mask, status, sync, host_rows):
        n_units = self.n_books // self.assets
        itemsize = 104 if members else 28
        dev_entry = self._L.bk_retune_agents_device if members else self._L.bk_retune_random_agents_device
        host_entry = self._L.bk_retune_agents if members else self._L.bk_retune_random_agents

        def block(x, name):  # (a device object of any element width: its address and its size in bytes)
            if hasattr(x, "data_ptr"):
                if not x.is_cuda or not x.is_contiguous():
                    raise ValueError(f"{name}: a contiguous CUDA tensor is needed")
                return C.c_void_p(x.data_ptr()), _dev_bytes(x)
            cai = x.__cuda_array_interface__
            if cai.get("strides"):
                raise ValueError(f"{name}: a contiguous device array is needed")
            return C.c_void_p(cai["data"][0]), _dev_bytes(x)

        for name, x in (("mask", mask), ("status", status)):
            if x is not None and _is_dev(x) != _is_dev(table):
                raise ValueError(f"table and {name} must both be host arrays or both be device arrays")
        if _is_dev(table):
            ptr, nbytes = block(table, "table")
            if nbytes == 0 or nbytes % (n_units * itemsize):
                raise ValueError(f"table: {n_units} x width rows of {itemsize} bytes are needed, got {nbytes} bytes")
            width = nbytes // (n_units * itemsize)
            m_ptr = s_ptr = None
            if mask is not None:
                m_ptr, mb = block(mask, "mask")
                if mb != n_units:
                    raise ValueError(f"mask: {n_units} one-byte elements are needed (one per book, or per market)")
            if status is not None:
                s_ptr, sb = block(status, "status")
                if sb != n_units * 8:
                    raise ValueError(f"status: {2 * n_units} four-byte elements are needed (two per book, or per market)")
            check(dev_entry(self._h, width, ptr, m_ptr, s_ptr))
        else:
            arr = host_rows(table)
            m = None if mask is None else _host_mask(mask, n_units, "one per book, or per market")
            if status is not None and (not isinstance(status, np.ndarray) or status.size != 2 * n_units):
                raise ValueError(f"status: a numpy array of {2 * n_units} elements is needed")
            check(host_entry(self._h, arr.shape[1], arr.ctypes.data_as(C.c_void_p),
                             None if m is None else m.ctypes.data_as(C.c_void_p)))
            if status is not None:
                status[...] = 0  # (the host entry applies every masked unit or raises)
        if sync:
            self.sync()

    def set_market_agents(self, members):
        """A ``#[derive(MarketAgentSet)]`` struct: ``[(asset, member), ...]`` with members as in ``set_agents`` — the
        multi-asset twins RandomMarketAgents / NoiseMarketAgent / MomentumMarketAgent (needs ``assets > 1``)."""
        members = list(members)
        self.set_agents([m for _, m in members], assets=[int(a) for a, _ in members])

    def run(self, n_steps: int, sync: bool = True):
        """``sim_runner``'s loop body ``n_steps`` times in ONE kernel launch (runner.rs:53-68)."""
        check(self._L.bk_run(self._h, int(n_steps)))
        if sync:
            self.sync()
            if self.strict:
                self.raise_on_flags()

    def enable_agent_order_log(self):
        """Record the orders ``run``'s RandomAgents create (``bk_set_agent_order_log``): ``orders`` / ``order_status`` /
        ``order_keys`` / ``book_state`` then answer for them as ``Env::get_orders`` / ``order_status`` do after
        ``sim_runner`` (env.rs:253-290).  Needs ``max_orders > 0`` (the log's capacity per book, 80 B per order) and must be
        called before the first ``run``; the env then runs the split pipelines with the logging event kernel."""
        check(self._L.bk_set_agent_order_log(self._h, 1))

    def warm(self, n_steps: int = 100):
        """``bk_warm``: ``n_steps`` of this env's own kernels on its own books, then everything is put back (state,
        level-2 records, step counter; no history slot or trade record is written).  Brings the GPU's clocks up and
        pays the pipeline's one-off set-up before a short, latency-sensitive ``run``."""
        check(self._L.bk_warm(self._h, int(n_steps)))

    def sync(self):
        check(self._L.bk_env_sync(self._h))

    # ------------------------------------------------------------ readers
    def level2(self, first_book: int = 0, n_books: Optional[int] = None) -> np.ndarray:
        """u32[n_books, 5+4L]: end-of-step snapshot, numpy ``level_2_data`` layout."""
        n = self.n_books - first_book if n_books is None else n_books
        out = np.zeros((n, self.width), dtype=np.uint32)
        check(self._L.bk_level2(self._h, first_book, n, _lib.p32(out)))
        return out

    def history_len(self) -> Tuple[int, int]:
        a, b = C.c_uint64(0), C.c_uint64(0)
        check(self._L.bk_history_len(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def history(self, first_step: Optional[int] = None, n_steps: Optional[int] = None, first_book: int = 0,
                n_books: Optional[int] = None) -> np.ndarray:
        """u32[n_steps, n_books, 5+4L] (Level2DataRecords + trade_vols, data.rs:9-57)."""
        f, n = self.history_len()
        first_step = f if first_step is None else first_step
        n_steps = (f + n - first_step) if n_steps is None else n_steps
        nb = self.n_books - first_book if n_books is None else n_books
        out = np.zeros((n_steps, nb, self.width), dtype=np.uint32)
        if n_steps and nb:
            check(self._L.bk_history(self._h, first_step, n_steps, first_book, nb, _lib.p32(out)))
        return out

    def stream_history(self, n_steps: int, chunk: int, on_chunk=None, trades: bool = False,
                       trade_records_per_chunk: Optional[int] = None) -> dict:
        """Run ``n_steps`` in chunks while the previous chunk's L2 records stream to pinned host memory on a copy
        stream (double-buffered; needs history_capacity >= 2 * chunk).  ``on_chunk(first_step, l2[chunk, B, W])`` is
        called once a chunk has landed (the arrays are reused two chunks later).  With ``trades=True`` the chunk's trade
        records travel too, compacted on the device into one dense stream (``bk_trades_compact``):
        ``on_chunk(first_step, l2, (offsets[B+1], records))``; needs trade_capacity >= the trades of one chunk per
        book.  Returns timing figures."""
        import time

        if chunk < 1 or self.history_capacity < 2 * chunk:
            raise ValueError("stream_history needs history_capacity >= 2 * chunk")
        L, W, B = self._L, self.width, self.n_books
        out_t = C.POINTER(C.c_uint32)
        tcap = int(trade_records_per_chunk or 64 * chunk * B) if trades else 0
        streams, bufs, tbufs = [], [], []
        for _ in range(2):  # chunk k uses stream/buffer k % 2: copy k overlaps run k+1, and is awaited before run k+2
            cs, p = C.c_void_p(), C.c_void_p()
            check(L.bk_stream_create(C.byref(cs)))
            check(L.bk_pinned_alloc(chunk * B * W * 4, C.byref(p)))
            streams.append(cs)
            bufs.append((p, np.ctypeslib.as_array(C.cast(p, out_t), shape=(chunk, B, W))))
            if trades:
                pr, po = C.c_void_p(), C.c_void_p()
                check(L.bk_pinned_alloc(tcap * 40, C.byref(pr)))
                check(L.bk_pinned_alloc((B + 1) * 8, C.byref(po)))
                rec = np.ctypeslib.as_array(C.cast(pr, C.POINTER(C.c_uint8)), shape=(tcap * 40,)).view(_lib.TRADE_DTYPE)
                off = np.ctypeslib.as_array(C.cast(po, C.POINTER(C.c_uint64)), shape=(B + 1,))
                tbufs.append((pr, po, rec, off))
        inflight = [None, None]  # per buffer: (first_step, n_steps, n_trade_records)

        def land(i):
            if inflight[i] is not None:
                check(L.bk_stream_sync(streams[i]))
                if on_chunk is not None:
                    first, c, nt = inflight[i]
                    if trades:
                        on_chunk(first, bufs[i][1][:c], (tbufs[i][3], tbufs[i][2][:nt]))
                    else:
                        on_chunk(first, bufs[i][1][:c])
                inflight[i] = None

        done, k, nbytes = 0, 0, 0
        t0 = time.perf_counter()
        try:
            while done < n_steps:
                c = min(chunk, n_steps - done)
                i = k % 2
                land(i)  # chunk k-2 has left the ring and its host buffer has been consumed
                first = self.steps_done()
                self.run(c, sync=False)
                check(L.bk_history_copy_async(self._h, first, c, 0, B, C.cast(bufs[i][0], out_t), streams[i]))
                nt = 0
                if trades:
                    check(L.bk_stream_sync(streams[1 - i]))  # the device's dense buffer is still being copied out
                    total = C.c_uint64(0)
                    check(L.bk_trades_compact(self._h, C.byref(total)))
                    nt = int(total.value)
                    if nt > tcap:
                        raise _lib.CapacityError(f"{nt} trade records in one chunk exceed trade_records_per_chunk={tcap}")
                    check(L.bk_trades_compact_copy_async(self._h, tbufs[i][0], C.cast(tbufs[i][1], C.POINTER(C.c_uint64)),
                                                         streams[i]))
                    nbytes += nt * 40 + (B + 1) * 8
                inflight[i] = (first, c, nt)
                nbytes += c * B * W * 4
                done += c
                k += 1
            land(k % 2)
            land((k + 1) % 2)
            self.sync()
            dt = time.perf_counter() - t0
        finally:
            for cs, (p, _) in zip(streams, bufs):
                L.bk_stream_sync(cs)
                L.bk_pinned_free(p)
                L.bk_stream_destroy(cs)
            for pr, po, _, _ in tbufs:
                L.bk_pinned_free(pr)
                L.bk_pinned_free(po)
        return {"seconds": dt, "book_steps_per_s": B * n_steps / dt, "d2h_gb_per_s": nbytes / dt / 1e9, "bytes": nbytes}

    def clear_history(self):
        check(self._L.bk_clear_history(self._h))

    def trade_count(self, book: int) -> Tuple[int, int]:
        a, b = C.c_uint64(0), C.c_uint64(0)
        check(self._L.bk_trade_count(self._h, book, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def trade_counts(self) -> np.ndarray:
        out = np.zeros(self.n_books, dtype=np.uint64)
        check(self._L.bk_trade_counts(self._h, _lib.p64(out)))
        return out

    def trades(self, book: int, first: Optional[int] = None, n: Optional[int] = None) -> np.ndarray:
        total, base = self.trade_count(book)
        first = base if first is None else first
        n = total - first if n is None else n
        a = np.zeros(n, dtype=_lib.TRADE_DTYPE)
        if n:
            check(self._L.bk_get_trades(self._h, book, first, n, a.ctypes.data_as(C.c_void_p)))
        return a

    def drain_trades(self) -> Tuple[np.ndarray, np.ndarray]:
        """All retained trade records of all books as ONE dense array + CSR offsets (book b: ``rec[off[b]:off[b+1]]``),
        compacted on the device; the records are then consumed (like ``clear_trades``)."""
        total = C.c_uint64(0)
        check(self._L.bk_trades_compact(self._h, C.byref(total)))
        rec = np.zeros(int(total.value), dtype=_lib.TRADE_DTYPE)
        off = np.zeros(self.n_books + 1, dtype=np.uint64)
        check(self._L.bk_trades_compact_copy_async(self._h, rec.ctypes.data_as(C.c_void_p), _lib.p64(off), None))
        return off, rec

    def clear_trades(self):
        check(self._L.bk_clear_trades(self._h))

    def order_counts(self) -> np.ndarray:
        """Orders created so far per book by the on-device agents (``orders.len()``, orderbook.rs:327-329)."""
        out = np.zeros(self.n_books, dtype=np.uint64)
        check(self._L.bk_order_counts(self._h, _lib.p64(out)))
        return out

    def event_steps_keyed(self) -> np.ndarray:
        """Per book: how many host-driven / ingress steps ran on the keyed event loop (a diagnostic; ``bk_event_steps_keyed``)."""
        out = np.zeros(self.n_books, dtype=np.uint64)
        check(self._L.bk_event_steps_keyed(self._h, _lib.p64(out)))
        return out

    def stamp_compactions(self) -> int:
        """How many times this env has queued the stamp compaction (a diagnostic; ``bk_stamp_compactions``)."""
        out = C.c_uint64(0)
        check(self._L.bk_stamp_compactions(self._h, C.byref(out)))
        return int(out.value)

    def time(self, book: int = 0) -> int:
        out = C.c_uint64(0)
        check(self._L.bk_time(self._h, book, C.byref(out)))
        return int(out.value)

    def set_time(self, book: int, t: int):
        """``OrderBook::set_time`` (orderbook.rs:183-185) — host-driven path."""
        check(self._L.bk_set_time(self._h, book, int(t)))

    def trade_vol(self, book: int = 0) -> int:
        out = C.c_uint32(0)
        check(self._L.bk_trade_vol(self._h, book, C.byref(out)))
        return int(out.value)

    def steps_done(self) -> int:
        out = C.c_uint64(0)
        check(self._L.bk_steps_done(self._h, C.byref(out)))
        return int(out.value)

    def flags(self) -> np.ndarray:
        """Every book's sticky flag word: the device's bits OR the ones a strict check has already reported."""
        out = np.zeros(self.n_books, dtype=np.uint32)
        check(self._L.bk_book_flags(self._h, _lib.p32(out)))
        if self._flags_sticky is not None:
            out |= self._flags_sticky
        return out

    def rng_state(self, book: int) -> Tuple[int, int]:
        out = np.zeros(2, dtype=np.uint64)
        check(self._L.bk_rng_state(self._h, book, _lib.p64(out)))
        return int(out[0]), int(out[1])

    def live_orders(self, book: int) -> np.ndarray:
        cap = 1024
        a = np.zeros(cap, dtype=_lib.ORDER_DTYPE)
        n = C.c_uint32(0)
        check(self._L.bk_live_orders(self._h, book, cap, a.ctypes.data_as(C.c_void_p), C.byref(n)))
        return a[: n.value].copy()

    def stats(self) -> dict:
        s = Stats()
        check(self._L.bk_stats_compute(self._h, C.byref(s)))
        return {k: int(getattr(s, k)) for k, _ in Stats._fields_}

    def stats_device_ptr(self) -> int:
        return self._device_ptr(self._L.bk_stats_device_ptr)

    def level2_device_ptr(self) -> int:
        """Device address of the latest level-2 records, u32[n_books][width] (for on-device consumers)."""
        return self._device_ptr(self._L.bk_level2_device_ptr)

    def stats_compute_async(self):
        check(self._L.bk_stats_compute(self._h, None))

    # ------------------------------------------------------------ measurement
    def profile(self, every: int):
        """HIP-event timing of the step kernels: 0 off, N >= 1 = time the kernels of every Nth step."""
        check(self._L.bk_profile_enable(self._h, int(every)))

    def profile_read(self, reset: bool = True) -> Tuple[float, int]:
        ms, n = C.c_double(0), C.c_uint64(0)
        check(self._L.bk_profile_read(self._h, C.byref(ms), C.byref(n), int(reset)))
        return float(ms.value), int(n.value)

    def profile_read_kind(self, kind: int) -> Tuple[float, int]:
        """kind: 0 k_run_random, 1 k_agents_fsm, 2 k_step_batch, 3 k_step_events (call before profile_read(reset))."""
        ms, n = C.c_double(0), C.c_uint64(0)
        check(self._L.bk_profile_read_kind(self._h, int(kind), C.byref(ms), C.byref(n)))
        return float(ms.value), int(n.value)

    def set_pipeline(self, mode: str):
        """'auto' | 'fused' | 'split' | 'split_wave' | 'wave_split' | 'wave' — kernel pipeline of run(); results are
        identical.  ('wave' / 'wave_split': RandomAgents books, the RNG-serial phases one wave per book with a
        wave-parallel stream decode, fused with the event phase in one persistent kernel / as a kernel of its own;
        'wave_split' on an AgentSet of Noise / Momentum members: their update one wave per book with the same kind of
        decode - k_agents_mixed_wave - in front of the event kernel, the auto choice from 512 books.)  ('split_wave':
        AgentSets with Noise/Momentum members keep their update one wave per book as scalar code; for RandomAgents it
        equals 'split'.)"""
        check(self._L.bk_set_pipeline(self._h, {"auto": 0, "fused": 1, "split": 2, "split_wave": 3, "wave_split": 4, "wave": 5}[mode]))

    def set_wave_options(self, lookahead: int = 64, parts: int = 0):
        """'wave' pipeline knobs: look-ahead of the vector decode path (1..64; small = exercise the scalar slow path)
        and the number of parts the batch is cut in (0 = default)."""
        check(self._L.bk_set_wave_options(self._h, int(lookahead), int(parts)))

    def set_split_parts(self, n_parts: int, min_part: int = 4096):
        """Split pipeline: cut the batch in ``min(n_parts, books / min_part)`` parts on separate streams."""
        check(self._L.bk_set_split_parts(self._h, int(n_parts), int(min_part)))

    def split_parts(self) -> Tuple[int, int]:
        """(n_parts, min_part) as set (``bk_get_split_parts``); ``pipeline()`` reports the effective number of parts."""
        a, b = C.c_int(0), C.c_uint32(0)
        check(self._L.bk_get_split_parts(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def pipeline_fallbacks(self) -> int:
        """Rounds 1-2: bk_run launches the auto pipeline rolled back and redid on the fused kernel.  Always 0 since round
        3 (the auto choice frees pool slots like the fused kernel; nothing is left to roll back)."""
        out = C.c_uint64(0)
        check(self._L.bk_pipeline_fallbacks(self._h, C.byref(out)))
        return int(out.value)

    def pipeline(self) -> Tuple[str, int]:
        """('fused' | 'split' | 'wave_split' | 'wave', number of book parts on separate streams) that run() will use."""
        a, b = C.c_int(0), C.c_int(1)
        check(self._L.bk_get_pipeline(self._h, C.byref(a), C.byref(b)))
        return ("fused", "split", "wave_split", "wave")[a.value], int(b.value)

    def checkpoint(self) -> np.ndarray:
        """Complete simulation state (pool, clock, counters, RNG of every book) as a byte array."""
        n = int(self._L.bk_checkpoint_bytes(self._h))
        # The flag bits a strict check has already reported live on the host (raise_on_flags moves them off the device):
        # they travel as a trailer behind the library's image, so that flags() reads the same after a restore.
        tail = 0 if self._flags_sticky is None else 16 + 4 * self.n_books
        buf = np.zeros(n + tail, dtype=np.uint8)
        check(self._L.bk_checkpoint_save(self._h, buf.ctypes.data_as(C.c_void_p), n))
        if tail:
            buf[n:n + 16] = np.frombuffer(_STICKY_MAGIC + np.uint64(self.n_books).tobytes(), dtype=np.uint8)
            buf[n + 16:] = self._flags_sticky.view(np.uint8)
        return buf

    def restore(self, buf: np.ndarray):
        """Load a checkpoint taken from an env of the same shape; the run continues bit-identically."""
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        n = int(self._L.bk_checkpoint_bytes(self._h))
        # exactly the library's image, or the image + the sticky-flags trailer of checkpoint() with its magic and this env's
        # book count; anything else - a checkpoint of another shape, a truncated or padded file - is refused, not loaded in part
        tail = 16 + 4 * self.n_books
        has_tail = buf.nbytes == n + tail
        if has_tail and not (buf[n:n + 8].tobytes() == _STICKY_MAGIC and
                             int(np.frombuffer(buf[n + 8:n + 16].tobytes(), dtype=np.uint64)[0]) == self.n_books):
            raise _lib.BourseError(_lib.BK_INVALID, "restore: the checkpoint's trailer is not this env's (magic / book count)")
        if not has_tail and buf.nbytes != n:
            raise _lib.BourseError(_lib.BK_INVALID, f"restore: {buf.nbytes} bytes is not a checkpoint of this env's shape ({n} bytes, "
                                                   f"or {n + tail} with the reported-flags trailer)")
        check(self._L.bk_checkpoint_load(self._h, buf.ctypes.data_as(C.c_void_p), n))
        self._candles_folded(restart=True)
        self._flags_sticky, self._warned_bits = None, 0
        if has_tail:
            self._flags_sticky = buf[n + 16:].view(np.uint32).copy()

    def state_bytes_per_book(self) -> int:
        return int(self._L.bk_state_bytes_per_book(self._h))

    # ------------------------------------------------------------ per-book reset to a device-resident snapshot
    def snapshot_bytes(self) -> int:
        """Device bytes one snapshot slot costs."""
        return int(self._L.bk_snapshot_bytes(self._h))

    def save_snapshot(self, slot: int = 0):
        """``bk_snapshot_save``: a device-resident copy of every book's state (pool, clock, counters, RNG, level-2 record)
        in ``slot`` (0 .. 3), queued on the env's stream; a later save of the slot overwrites it.  The reference has no
        counterpart."""
        check(self._L.bk_snapshot_save(self._h, int(slot)))

    def drop_snapshot(self, slot: int = 0):
        """Free the slot's device memory (``bk_snapshot_drop``)."""
        check(self._L.bk_snapshot_drop(self._h, int(slot)))

    def reset_books(self, mask, seeds=None, slot: int = 0, sync: bool = True):
        """Books ``b`` with ``mask[b]`` set go back to their state in snapshot ``slot`` while the others carry on
        (``bk_reset_books`` / ``bk_reset_books_device``); on a market env the mask is over markets and every book of a
        masked market goes back.  ``mask``: bool / uint8, one per book (market) - a host array, or a torch CUDA tensor /
        ``__cuda_array_interface__`` object written on the env's stream, which then never passes through the host.
        ``seeds`` (uint64, same length, the same kind of object as the mask): the reset books start a new RNG stream,
        seeded as a fresh env's book with that seed is.  A reset book keeps its sticky flags and takes the env's current
        trading flag; no trade of the run it abandons stays retained; the env's step counter and history ring go on
        (``history()`` rows of a reset book continue at the env's step index).  Queued on the env's stream; ``sync``
        waits for it."""
        self._masked_reset(self._L.bk_reset_books_device, self._L.bk_reset_books, mask, seeds, slot, sync)

    def _masked_reset(self, device_entry, host_entry, mask, seeds, slot, sync):
        n_units = self.n_books // self.assets
        per = "one per book, or per market"
        if mask is None:
            raise ValueError("mask: one bool / uint8 per book (market) is needed")
        if seeds is not None and _is_dev(mask) != _is_dev(seeds):
            raise ValueError("mask and seeds must both be host arrays or both be device arrays")
        if _is_dev(mask):
            if _dev_count(mask) != n_units or (seeds is not None and _dev_count(seeds) != n_units):
                raise ValueError(f"mask / seeds: {n_units} elements are needed ({per})")
            check(device_entry(self._h, int(slot), self._dev_ptr(mask, 1, "mask"), self._dev_ptr(seeds, 8, "seeds")))
        else:
            m = _host_mask(mask, n_units, per, name="mask / seeds")
            s = None if seeds is None else np.ascontiguousarray(np.asarray(seeds), dtype=np.uint64)
            if s is not None and s.shape != (n_units,):
                raise ValueError(f"mask / seeds: {n_units} elements are needed ({per})")
            check(host_entry(self._h, int(slot), m.ctypes.data_as(C.c_void_p),
                             None if s is None else s.ctypes.data_as(C.c_void_p)))
        self._candles_folded()  # (a reset folds the series' outstanding steps first)
        if sync:
            self.sync()

    # ------------------------------------------------------------ the same for an env with the device ingress
    def ingress_snapshot_bytes(self, slot: int = 0) -> int:
        """Device bytes ingress-snapshot ``slot`` holds (0: empty)."""
        return int(self._L.bk_ingress_snapshot_bytes(self._h, int(slot)))

    def save_ingress_snapshot(self, slot: int = 0):
        """``bk_ingress_snapshot_save``: ``save_snapshot`` for an env with the device ingress, in slots (0 .. 3) of their
        own - besides every book's state, the order records of the ids handed out so far, the held ids of
        ``update_agents`` and the lists and momentum state of ``update_members``.  Waits for the env's stream.  The
        reference has no counterpart."""
        check(self._L.bk_ingress_snapshot_save(self._h, int(slot)))

    def drop_ingress_snapshot(self, slot: int = 0):
        """Free the slot's device memory (``bk_ingress_snapshot_drop``)."""
        check(self._L.bk_ingress_snapshot_drop(self._h, int(slot)))

    def reset_ingress_books(self, mask, seeds=None, slot: int = 0, sync: bool = True):
        """``reset_books`` for an env with the device ingress (``bk_ingress_reset_books`` /
        ``bk_ingress_reset_books_device``), with the same ``mask`` / ``seeds`` / ``sync``: a masked book (market) also gets
        back its order records, its agents' held ids and its members' lists and state, and its queue is emptied - what
        was submitted or queued by an update since the last ``step`` is dropped, so reset right after ``step``.  Refused
        after any ``set_*agents*`` call since the save: ``save_ingress_snapshot`` again."""
        self._masked_reset(self._L.bk_ingress_reset_books_device, self._L.bk_ingress_reset_books, mask, seeds, slot, sync)

    # ------------------------------------------------------------ trader accounts of an env with the device ingress
    ACCOUNT_DTYPE = _lib.ACCOUNT_DTYPE

    def enable_accounts(self, n_traders: int, consume_trades: bool = False):
        """``bk_accounts_enable``: keep ``position`` / ``cash`` / ``volume`` / ``fills`` of traders ``0 .. n_traders - 1``
        per book in device memory, folded from every step's new trade records on the env's stream with no host in the
        loop (trader ids >= ``n_traders`` - background members, say - are left out).  Call after
        ``enable_device_ingress`` and before the first instruction, update or step.  ``consume_trades=True`` marks the
        trade records consumed once folded (as ``clear_trades``), so ``trade_capacity`` only has to hold one step's trades.
        A record that could not be folded sets ``FLAG_ACCOUNTS_INEXACT`` on its book.  The reference has no counterpart."""
        if not 0 <= int(n_traders) <= 0xFFFFFFFF:
            raise ValueError("n_traders out of range")
        check(self._L.bk_accounts_enable(self._h, int(n_traders), int(bool(consume_trades))))
        self._n_traders = int(n_traders)

    def _accounts_traders(self) -> int:
        if not self._n_traders:
            raise _lib.BourseError(_lib.BK_INVALID, "this env has no trader accounts: call enable_accounts first")
        return self._n_traders

    def accounts(self, first_book: int = 0, n_books: Optional[int] = None) -> np.ndarray:
        """The rows of books ``[first_book, first_book + n_books)`` (default: to the last book) as a structured array of
        shape ``[n, n_traders]`` (``ACCOUNT_DTYPE``).  Waits for the env's stream."""
        nt = self._accounts_traders()
        return self._book_rows(self._L.bk_get_accounts, first_book, n_books, ((nt,), _lib.ACCOUNT_DTYPE))[0]

    def accounts_device_ptr(self) -> int:
        """Device address of the table, ``bk_account[n_books][n_traders]`` (for on-device consumers)."""
        return self._device_ptr(self._L.bk_accounts_device_ptr)

    def accounts_view(self) -> "AccountsView":
        """The table in place as an object with ``__cuda_array_interface__``: int64, shape ``(n_books, n_traders, 4)``, the
        last axis ``position, cash, volume, fills`` (the two unsigned words read as int64: the same bits).
        ``torch.as_tensor(env.accounts_view(), device="cuda")`` is a zero-copy tensor that every later step updates; it is
        written on the env's stream, so read it there (or after ``sync()``)."""
        return AccountsView(self, self.accounts_device_ptr(), (self.n_books, self._accounts_traders(), 4), self._stream)

    def clear_accounts(self, mask=None, sync: bool = True):
        """Zero the rows of the books ``b`` with ``mask[b]`` set (``None``: every book); they count from the book's
        current trade count on.  ``mask``: bool / uint8, one per BOOK - a host array (``bk_accounts_clear``), or a torch
        CUDA tensor / ``__cuda_array_interface__`` object written on the env's stream (``bk_accounts_clear_device``: no
        host synchronisation).  ``reset_ingress_books`` clears the books it resets by itself.  ``sync`` waits for it."""
        self._accounts_traders()
        self._masked_clear(self._L.bk_accounts_clear_device, self._L.bk_accounts_clear, mask, sync)

    # ------------------------------------------------------------ per-step trade bars of an env with the device ingress
    TRADE_BAR_DTYPE = _lib.TRADE_BAR_DTYPE

    def enable_trade_bars(self, window: int = 1, consume_trades: bool = False):
        """``bk_trade_bars_enable``: keep, per book, a ring of the last ``window`` steps' bars in device memory - ``open`` /
        ``high`` / ``low`` / ``close`` price, ``buy_vol`` / ``sell_vol`` by the aggressor's side, ``notional`` and the
        record counts ``n_buy`` / ``n_sell`` - folded from every step's new trade records on the env's stream with no host
        in the loop.  The step run while ``steps_done()`` reads ``k`` goes to slot ``k % window``; a book-step without a
        trade carries the previous close and is zero otherwise.  Call after ``enable_device_ingress``, at any time.
        ``consume_trades=True`` marks the trade records consumed once folded (as ``clear_trades``), so ``trade_capacity``
        only has to hold one step's trades.  A record dropped beyond ``trade_capacity`` is left out of its bar; that book carries ``FLAG_TRADE_OVERFLOW``.  The
        reference has no counterpart."""
        if not 0 <= int(window) <= 0xFFFFFFFF:
            raise ValueError("window out of range")
        check(self._L.bk_trade_bars_enable(self._h, int(window), int(bool(consume_trades))))
        self._bars_window = int(window)

    def _trade_bars_window(self) -> int:
        if not self._bars_window:
            raise _lib.BourseError(_lib.BK_INVALID, "this env has no trade bars: call enable_trade_bars first")
        return self._bars_window

    def trade_bars(self, first_book: int = 0, n_books: Optional[int] = None) -> np.ndarray:
        """The rings of books ``[first_book, first_book + n_books)`` (default: to the last book) as a structured array of
        shape ``[n, window]`` (``TRADE_BAR_DTYPE``).  Waits for the env's stream."""
        w = self._trade_bars_window()
        return self._book_rows(self._L.bk_get_trade_bars, first_book, n_books, ((w,), _lib.TRADE_BAR_DTYPE))[0]

    def trade_bars_device_ptr(self) -> int:
        """Device address of the ring, ``bk_trade_bar[n_books][window]`` (for on-device consumers)."""
        return self._device_ptr(self._L.bk_trade_bars_device_ptr)

    def trade_bars_slot(self) -> int:
        """The slot the latest folded step went to, ``(steps_done() - 1) % window``: a host integer, no wait."""
        out = C.c_uint32(0)
        check(self._L.bk_trade_bars_slot(self._h, C.byref(out)))
        return int(out.value)

    def trade_bars_view(self) -> "TradeBarsView":
        """The ring in place as an object with ``__cuda_array_interface__``: int64, shape ``(n_books, window, 6)``.  Word 0
        is ``open | high << 32``, word 1 ``low | close << 32``, words 2..4 ``buy_vol``, ``sell_vol``, ``notional`` (unsigned,
        read as int64: the same bits) and word 5 ``n_buy | n_sell << 32``.  ``torch.as_tensor(env.trade_bars_view(),
        device="cuda")`` is a zero-copy tensor that every later step updates; it is written on the env's stream, so read it
        there (or after ``sync()``)."""
        return TradeBarsView(self, self.trade_bars_device_ptr(), (self.n_books, self._trade_bars_window(), 6), self._stream)

    def clear_trade_bars(self, mask=None, sync: bool = True):
        """Zero all rows of the books ``b`` with ``mask[b]`` set (``None``: every book); their bars count from the book's
        current trade count on and the carried price starts at 0.  ``mask`` / ``sync`` as ``clear_accounts`` takes them
        (``bk_trade_bars_clear`` / ``bk_trade_bars_clear_device``).  ``reset_ingress_books`` clears the books it resets."""
        self._trade_bars_window()
        self._masked_clear(self._L.bk_trade_bars_clear_device, self._L.bk_trade_bars_clear, mask, sync)

    # ------------------------------------------------------------ per-book series moments of the level-2 history
    SERIES_DTYPE = _lib.SERIES_DTYPE

    def enable_series(self):
        """``bk_series_enable``: keep one row of integer sums per book in device memory - over the book's whole series of
        level-2 records: counts, sums of twice the mid, of the spread and its square, of the touch volumes and the traded
        volume, of the mid's step-to-step change ``d`` up to its fourth power, of ``d * d_prev`` and ``|d| * |d_prev|``, and
        the extremes (``SERIES_DTYPE``; include/bourse_amd.h states what one record adds).  ``fold_series()`` folds the
        steps run since the last fold from the history ring, on the env's stream; nothing leaves the device until
        ``series()`` is read.  Needs ``history_capacity > 0``; works with ``run`` on every pipeline, ``step``, the device
        ingress and markets.  Steps before the call are not counted.  The reference has no counterpart."""
        check(self._L.bk_series_enable(self._h))
        self._series = True

    def fold_series(self, sync: bool = False):
        """``bk_series_fold``: queue the fold of every step run since the last fold (no new step: no launch).  Raises if
        one of them is no longer retained by the ring - more than ``history_capacity`` steps since the last fold, or
        ``clear_history()`` - naming how many were lost; rows and cursor are then unchanged and ``clear_series()`` starts
        again."""
        check(self._L.bk_series_fold(self._h))
        self._candles_folded()
        if sync:
            self.sync()

    def series(self, first_book: int = 0, n_books: Optional[int] = None) -> np.ndarray:
        """The rows of books ``[first_book, first_book + n_books)`` (default: to the last book) as a structured array
        (``SERIES_DTYPE``).  Waits for the env's stream; does NOT fold."""
        return self._book_rows(self._L.bk_get_series, first_book, n_books, ((), _lib.SERIES_DTYPE))[0]

    def series_device_ptr(self) -> int:
        """Device address of the table, ``bk_series_row[n_books]`` (for on-device consumers)."""
        return self._device_ptr(self._L.bk_series_device_ptr)

    def series_view(self) -> "SeriesView":
        """The table in place as an object with ``__cuda_array_interface__``: int64, shape ``(n_books, 24)``, the words in
        ``SERIES_DTYPE``'s order (unsigned words read as int64: the same bits).  ``torch.as_tensor(env.series_view(),
        device="cuda")`` is a zero-copy tensor that every later fold updates; it is written on the env's stream, so read
        it there (or after ``sync()``)."""
        return SeriesView(self, self.series_device_ptr(), (self.n_books, 24), self._stream)

    def clear_series(self, mask=None, sync: bool = True):
        """With a ``mask`` (one entry per BOOK): fold what is outstanding (raising as ``fold_series`` does), then clear the
        rows of the books with ``mask[b]`` set, carry included.  ``None``: clear every row and count from the current step
        on without folding - the way on after lost steps.  ``mask`` / ``sync`` as ``clear_accounts`` takes them
        (``bk_series_clear`` / ``bk_series_clear_device``).  ``reset_books`` / ``reset_ingress_books`` fold and then cut only
        the carry of the books they reset: the sums go on across episodes and no return spans a reset."""
        # (no check of its own in front: the library refuses an env without the table)
        self._masked_clear(self._L.bk_series_clear_device, self._L.bk_series_clear, mask, sync)
        self._candles_folded(restart=mask is None)

    def run_series(self, n_steps: int, chunk: Optional[int] = None):
        """``run(c, sync=False); fold_series()`` in chunks of ``chunk <= history_capacity`` steps (default:
        ``history_capacity``) until ``n_steps`` are run: the way to run more steps than the ring holds.  Nothing waits
        between the chunks, or at the end.  With ``enable_lags`` / ``enable_bins`` / ``enable_cross`` those tables are folded
        after every chunk too - and alone if only they are enabled.  So is the flow table of ``enable_flow`` (``fold_flow()``: the chunk's trade
        records; with ``consume_trades`` ``trade_capacity`` then only has to hold one chunk's trades), also as the only table
        of the env: ``fold_series`` and its refusal come only where no table at all is enabled."""
        c = self.history_capacity if chunk is None else int(chunk)
        if not 1 <= c <= self.history_capacity:
            raise ValueError("run_series needs 1 <= chunk <= history_capacity")
        folds = ([self.fold_lags] if self._n_lags else []) + ([self.fold_bins] if self._bins_shape else [])
        folds += [self.fold_cross] if self._cross_spans else []  # (ManyMarketEnv.enable_cross)
        folds += [self.fold_flow] if self._flow_lags else []  # (enable_flow: the chunk's trade records as well)
        if self._series or not folds:  # (neither table: fold_series raises the library's refusal, as ever)
            folds.insert(0, self.fold_series)
        for fold in folds:
            fold()  # (steps run before the call are not pushed out of the ring by the first chunk)
        left = int(n_steps)
        while left > 0:
            n = min(c, left)
            self.run(n, sync=False)
            for fold in folds:
                fold()
            left -= n

    # ------------------------------------------------------------ per-level depth table, the series moments' companion
    def enable_depth(self):
        """``bk_depth_enable``: beside the series moments keep ``levels + 1`` rows of sixteen integer sums per book in
        device memory, folded from the LADDER of the level-2 records - per level the sums of the resting volume, its
        square and the order count on either side and how often the level was occupied, the sums of the cumulative depth
        imbalance ``I_q``, and of the next move of the mid against it (``bourse_amd.DEPTH_FIELDS``); in the last row the
        header (``DEPTH_HEADER_FIELDS``).  Needs ``enable_series()`` first and shares its cursor: ``fold_series``,
        ``clear_series``, ``run_series``, the resets (which cut the carry) and ``restore`` (which clears) act on both
        tables.  Folds the series' outstanding steps first - and refuses as ``fold_series`` does if steps were lost - so
        the depth rows count from the current step on.  ``depth_moments`` turns the rows into moments.  The reference has
        no counterpart."""
        check(self._L.bk_depth_enable(self._h))

    def depth(self, first_book: int = 0, n_books: Optional[int] = None) -> np.ndarray:
        """The rows of books ``[first_book, first_book + n_books)`` (default: to the last book) as a uint64 array of
        shape ``[n, levels + 1, 16]``.  Waits for the env's stream; does NOT fold (``fold_series`` folds both tables)."""
        return self._book_rows(self._L.bk_get_depth, first_book, n_books, ((self.levels + 1, _lib.DEPTH_ROW_WORDS), np.uint64))[0]

    def depth_device_ptr(self) -> int:
        """Device address of the table, ``uint64_t[n_books][levels + 1][16]`` (for on-device consumers)."""
        return self._device_ptr(self._L.bk_depth_device_ptr)

    def depth_view(self) -> "DepthView":
        """The table in place as an object with ``__cuda_array_interface__``: int64, shape ``(n_books, levels + 1, 16)``
        (unsigned words read as int64: the same bits).  ``torch.as_tensor(env.depth_view(), device="cuda")`` is a zero-copy
        tensor that every later fold updates; it is written on the env's stream, so read it there (or after ``sync()``)."""
        return DepthView(self, self.depth_device_ptr(), (self.n_books, self.levels + 1, _lib.DEPTH_ROW_WORDS), self._stream)

    # ------------------------------------------------------------ per-book candle table, the series moments' other companion
    CANDLE_DTYPE = _lib.CANDLE_DTYPE

    def enable_candles(self, width: int, n_candles: int):
        """``bk_candles_enable``: beside the series moments keep per book a ring of the last ``n_candles`` (1 .. 65536) bars
        of ``width`` (1 .. 1048576) steps each in device memory, sixteen integer words a bar, folded from the same level-2
        records: open / high / low / close of twice the mid, the sums behind the time-weighted mid and spread, the traded
        volume, and the returns' sums up to the realised variance (``bourse_amd.CANDLE_FIELDS`` / ``CANDLE_DTYPE``;
        include/bourse_amd.h states what one record adds).  Bars are aligned to the env's absolute step count, the same
        for every book: step ``s`` is of bar ``s // width`` in slot ``(s // width) % n_candles``.  Needs ``enable_series()``
        first and shares its cursor: ``fold_series``, ``clear_series``, ``run_series``, the resets (which cut the carry)
        and ``restore`` (which clears) act on it too; ``enable_depth`` may stand beside it, in either order.  Folds the
        series' outstanding steps first - and refuses as ``fold_series`` does if steps were lost - so the bars count from
        the current step on.  ``candle_series`` turns the rows into prices.  The reference has no counterpart."""
        for name, x in (("width", width), ("n_candles", n_candles)):
            if not 0 <= int(x) <= 0xFFFFFFFF:
                raise ValueError(f"{name} out of range")
        check(self._L.bk_candles_enable(self._h, int(width), int(n_candles)))
        done = self.steps_done()
        self._candles = {"width": int(width), "n": int(n_candles), "start": done, "seen": done}

    def _candles_folded(self, restart: bool = False):
        """a call that folded the series' outstanding steps has returned: the candle table stands at ``steps_done`` too
        (``restart``: its rows were cleared as well)"""
        c = getattr(self, "_candles", None)
        if c is not None:
            c["seen"] = self.steps_done()
            if restart:
                c["start"] = c["seen"]

    def candles_config(self) -> Tuple[int, int]:
        """``bk_candles_config_get``: ``(width, n_candles)`` as enabled."""
        out = (C.c_uint32 * 2)()
        check(self._L.bk_candles_config_get(self._h, out))
        return int(out[0]), int(out[1])

    def candles(self, first_book: int = 0, n_books: Optional[int] = None) -> np.ndarray:
        """The bars of books ``[first_book, first_book + n_books)`` (default: to the last book) as a structured array of
        shape ``[n, n_candles]`` (``CANDLE_DTYPE``), slot by slot: bar ``j`` in slot ``j % n_candles``, ``n_steps == 0``
        where a slot holds no bar.  Waits for the env's stream; does NOT fold (``fold_series`` folds both tables)."""
        return self._book_rows(self._L.bk_get_candles, first_book, n_books, ((self.candles_config()[1],), _lib.CANDLE_DTYPE))[0]

    def candles_device_ptr(self) -> int:
        """Device address of the table, ``uint64_t[n_books][n_candles][16]`` (for on-device consumers)."""
        return self._device_ptr(self._L.bk_candles_device_ptr)

    def candles_view(self) -> "CandlesView":
        """The table in place as an object with ``__cuda_array_interface__``: int64, shape ``(n_books, n_candles, 16)``
        (unsigned words read as int64: the same bits).  ``torch.as_tensor(env.candles_view(), device="cuda")`` is a
        zero-copy tensor that every later fold updates; it is written on the env's stream, so read it there (or after
        ``sync()``)."""
        ptr = self.candles_device_ptr()
        return CandlesView(self, ptr, (self.n_books, self.candles_config()[1], _lib.CANDLE_ROW_WORDS), self._stream)

    def candles_latest(self) -> Optional[Tuple[int, int]]:
        """``(bar, slot)`` of the newest folded bar - that of the last step in front of the series' cursor, the same for
        every book - from host integers, with no wait; ``None`` while no step is folded since the enable, a full clear or
        a restore."""
        width, n = self.candles_config()
        c = self._candles
        if c["seen"] <= c["start"]:
            return None
        bar = (c["seen"] - 1) // width
        return bar, bar % n

    # ------------------------------------------------------------ per-book lag table of the level-2 history
    LAG_DTYPE = _lib.LAG_DTYPE

    def enable_lags(self, n_lags: int):
        """``bk_lags_enable``: keep ``n_lags`` rows (1 .. 64) of integer sums per book in device memory, row ``k - 1`` for
        lag / span ``k``: the count and sums of ``d_s * d_{s-k}`` and ``|d_s| * |d_{s-k}|`` (``d`` the step-to-step change
        of twice the mid), and count, sum, absolute sum, second and fourth power and maximum of the change over ``k`` steps
        (``LAG_DTYPE``; include/bourse_amd.h states what one record adds).  ``fold_lags()`` folds the steps run since the
        last fold from the history ring, on the env's stream; nothing leaves the device until ``lags()`` is read.  Needs
        ``history_capacity > 0``; works with ``run`` on every pipeline, ``step``, the device ingress and markets, with or
        without ``enable_series``.  Steps before the call are not counted.  The reference has no counterpart."""
        if not 0 <= int(n_lags) <= 0xFFFFFFFF:
            raise ValueError("n_lags out of range")
        check(self._L.bk_lags_enable(self._h, int(n_lags)))
        self._n_lags = int(n_lags)

    def _lags_count(self) -> int:
        if not self._n_lags:
            raise _lib.BourseError(_lib.BK_INVALID, "this env has no lag table: call enable_lags (bk_lags_enable) first")
        return self._n_lags

    def fold_lags(self, sync: bool = False):
        """``bk_lags_fold``: queue the fold of every step run since the last fold (no new step: no launch).  Raises if one
        of them is no longer retained by the ring - more than ``history_capacity`` steps since the last fold, or
        ``clear_history()`` - naming how many were lost; rows, carry and cursor are then unchanged and ``clear_lags()``
        starts again."""
        check(self._L.bk_lags_fold(self._h))
        if sync:
            self.sync()

    def lags(self, first_book: int = 0, n_books: Optional[int] = None) -> np.ndarray:
        """The rows of books ``[first_book, first_book + n_books)`` (default: to the last book) as a structured array of
        shape ``[n, n_lags]`` (``LAG_DTYPE``).  Waits for the env's stream; does NOT fold."""
        return self._book_rows(self._L.bk_get_lags, first_book, n_books, ((self._lags_count(),), _lib.LAG_DTYPE))[0]

    def lags_device_ptr(self) -> int:
        """Device address of the table, ``bk_lag_row[n_books][n_lags]`` (for on-device consumers)."""
        return self._device_ptr(self._L.bk_lags_device_ptr)

    def lags_view(self) -> "LagsView":
        """The table in place as an object with ``__cuda_array_interface__``: int64, shape ``(n_books, n_lags, 10)``, the
        words in ``LAG_DTYPE``'s order (unsigned words read as int64: the same bits).  ``torch.as_tensor(env.lags_view(),
        device="cuda")`` is a zero-copy tensor that every later fold updates; it is written on the env's stream, so read
        it there (or after ``sync()``)."""
        return LagsView(self, self.lags_device_ptr(), (self.n_books, self._lags_count(), 10), self._stream)

    def clear_lags(self, mask=None, sync: bool = True):
        """With a ``mask`` (one entry per BOOK): fold what is outstanding (raising as ``fold_lags`` does), then clear the
        rows and the carry of the books with ``mask[b]`` set.  ``None``: clear everything and count from the current step
        on without folding - the way on after lost steps.  ``mask`` / ``sync`` as ``clear_accounts`` takes them
        (``bk_lags_clear`` / ``bk_lags_clear_device``).  ``reset_books`` / ``reset_ingress_books`` fold and then cut only
        the carry of the books they reset: the sums go on across episodes and no span or pair reaches over a reset."""
        # (no check of its own in front: the library refuses an env without the table)
        self._masked_clear(self._L.bk_lags_clear_device, self._L.bk_lags_clear, mask, sync)

    # ------------------------------------------------------------ per-book flow table of the trade records
    FLOW_DTYPE = _lib.FLOW_DTYPE

    def enable_flow(self, n_lags: int = 16, consume_trades: bool = False):
        """``bk_flow_enable``: keep ``8 + 6 * n_lags`` integer sums per book in device memory, over the book's TRADE RECORDS
        in record order - counts, volumes and notional of all trades and of the buys, and at lags ``1 .. n_lags`` (1 .. 64)
        in trade time the sums behind the sign autocorrelation, the response function and the price variogram
        (``flow_dtype(n_lags)``; include/bourse_amd.h states what one record and one pair add).  ``fold_flow()`` folds every
        book's new records on the env's stream; a device-ingress env also folds behind every ``step``; nothing leaves the
        device until ``flow()`` is read.  Needs ``trade_capacity > 0``; works with ``run`` on every pipeline, ``step``, the
        device ingress, markets and Noise / Momentum members.  ``consume_trades=True`` marks the records consumed by the
        fold (as ``clear_trades``), so ``trade_capacity`` only has to hold what is written between two folds.  A record the
        table could not read - dropped beyond ``trade_capacity``, or cleared / drained before the fold - counts in
        ``n_lost`` and forms no pair.  Records before the call are not counted.  The reference has no counterpart."""
        if not 0 <= int(n_lags) <= 0xFFFFFFFF:
            raise ValueError("n_lags out of range")
        check(self._L.bk_flow_enable(self._h, int(n_lags), 1 if consume_trades else 0))
        self._flow_lags = int(n_lags)

    def _flow_count(self) -> int:
        if not self._flow_lags:
            raise _lib.BourseError(_lib.BK_INVALID, "this env has no flow table: call enable_flow (bk_flow_enable) first")
        return self._flow_lags

    def flow_dtype(self) -> np.dtype:
        """``flow_dtype(n_lags)`` of this env's table."""
        return _lib.flow_dtype(self._flow_count())

    def fold_flow(self, sync: bool = False):
        """``bk_flow_fold``: queue one launch that folds every book's trade records since its cursor (a book without a new
        record returns at once)."""
        check(self._L.bk_flow_fold(self._h))
        if sync:
            self.sync()

    def flow(self, first_book: int = 0, n_books: Optional[int] = None) -> np.ndarray:
        """The rows of books ``[first_book, first_book + n_books)`` (default: to the last book) as a structured array
        (``flow_dtype()``): the eight base fields and ``lags``, an int64 ``(n_lags, 6)`` sub-array.  Waits for the env's
        stream; does NOT fold."""
        return self._book_rows(self._L.bk_get_flow, first_book, n_books, ((), self.flow_dtype()))[0]

    def flow_state(self, first_book: int = 0, n_books: Optional[int] = None):
        """``(carry [n, n_lags] uint64, cursors [n] uint64)`` of the same books, for tests and debugging
        (``bk_get_flow_state``)."""
        return tuple(self._book_rows(self._L.bk_get_flow_state, first_book, n_books, ((self._flow_count(),), np.uint64),
                                     ((), np.uint64)))

    def flow_device_ptr(self) -> int:
        """Device address of the table, ``uint64_t[n_books][8 + 6 * n_lags]`` (for on-device consumers)."""
        return self._device_ptr(self._L.bk_flow_device_ptr)

    def flow_view(self) -> "FlowView":
        """The table in place as an object with ``__cuda_array_interface__``: int64, shape ``(n_books, 8 + 6 * n_lags)``,
        the words in ``flow_dtype()``'s order (unsigned words read as int64: the same bits).  ``torch.as_tensor(
        env.flow_view(), device="cuda")`` is a zero-copy tensor that every later fold updates; it is written on the env's
        stream, so read it there (or after ``sync()``)."""
        return FlowView(self, self.flow_device_ptr(), (self.n_books, 8 + 6 * self._flow_count()), self._stream)

    def clear_flow(self, mask=None, sync: bool = True):
        """With a ``mask`` (one entry per BOOK): fold, then zero the words, invalidate the carry and move the cursor to the
        trade count of the books with ``mask[b]`` set.  ``None``: the same for every book without folding.  ``mask`` /
        ``sync`` as ``clear_accounts`` takes them (``bk_flow_clear`` / ``bk_flow_clear_device``).  ``reset_books`` /
        ``reset_ingress_books`` fold and then only cut the books they reset: the sums go on across episodes and no pair
        reaches over a reset."""
        self._masked_clear(self._L.bk_flow_clear_device, self._L.bk_flow_clear, mask, sync)

    # ------------------------------------------------------------ per-book bin table of the level-2 history
    BINS_CONFIG_DTYPE = _lib.BINS_CONFIG_DTYPE

    def enable_bins(self, spans=(1,), n_bins: int = 64, ret_width: int = 1, spread_width: int = 1, vol_width: int = 1):
        """``bk_bins_enable``: keep ``len(spans) + 2`` rows of ``n_bins`` u64 counts per book in device memory - channel
        ``j`` the change of twice the mid over ``spans[j]`` steps (1 .. 64 each, at most four, any order) in bins of
        ``ret_width`` centred on zero, then the spread in bins of ``spread_width`` and the traded volume per step in bins of
        ``vol_width``, both from zero; the end bins hold everything beyond them (include/bourse_amd.h states what one record
        adds; ``bourse_amd.bin_edges`` gives the edges).  ``n_bins`` is even and in 2 .. 256.  ``fold_bins()`` folds the
        steps run since the last fold from the history ring, on the env's stream; nothing leaves the device until ``bins()``
        is read.  Needs ``history_capacity > 0``; works with ``run`` on every pipeline, ``step``, the device ingress and
        markets, with or without ``enable_series`` / ``enable_lags``.  Steps before the call are not counted.  The reference
        has no counterpart."""
        spans = tuple(int(k) for k in spans)
        slots = (spans + (0, 0, 0, 0))[:4]  # (more than four spans: the library refuses n_spans)
        words = [int(n_bins), len(spans), *slots, int(ret_width), int(spread_width), int(vol_width)]
        if any(not 0 <= w <= 0xFFFFFFFF for w in words + list(spans)):
            raise ValueError("enable_bins: every value is a 32-bit unsigned integer")
        cfg = np.array(words, dtype=np.uint32)
        check(self._L.bk_bins_enable(self._h, cfg.ctypes.data_as(C.c_void_p)))
        self._bins_shape = (len(spans) + 2, int(n_bins))

    def _bins_dims(self) -> Tuple[int, int]:
        if not self._bins_shape:
            raise _lib.BourseError(_lib.BK_INVALID, "this env has no bin table: call enable_bins (bk_bins_enable) first")
        return self._bins_shape

    def bins_config(self) -> np.ndarray:
        """``bk_bins_config_get``: the configuration the table was enabled with, a ``BINS_CONFIG_DTYPE`` record (what
        ``bourse_amd.bin_edges`` takes)."""
        self._bins_dims()
        cfg = np.zeros((), dtype=_lib.BINS_CONFIG_DTYPE)
        check(self._L.bk_bins_config_get(self._h, cfg.ctypes.data_as(C.c_void_p)))
        return cfg

    def fold_bins(self, sync: bool = False):
        """``bk_bins_fold``: queue the fold of every step run since the last fold (no new step: no launch).  Raises if one
        of them is no longer retained by the ring - more than ``history_capacity`` steps since the last fold, or
        ``clear_history()`` - naming how many were lost; table, carry and cursor are then unchanged and ``clear_bins()``
        starts again."""
        check(self._L.bk_bins_fold(self._h))
        if sync:
            self.sync()

    def bins(self, first_book: int = 0, n_books: Optional[int] = None) -> np.ndarray:
        """The counts of books ``[first_book, first_book + n_books)`` (default: to the last book) as a uint64 array of
        shape ``[n, n_spans + 2, n_bins]``.  Waits for the env's stream; does NOT fold."""
        return self._book_rows(self._L.bk_get_bins, first_book, n_books, (self._bins_dims(), np.uint64))[0]

    def bins_device_ptr(self) -> int:
        """Device address of the table, ``uint64_t[n_books][n_spans + 2][n_bins]`` (for on-device consumers)."""
        return self._device_ptr(self._L.bk_bins_device_ptr)

    def bins_view(self) -> "BinsView":
        """The table in place as an object with ``__cuda_array_interface__``: int64, shape ``(n_books, n_spans + 2,
        n_bins)`` (the unsigned counts read as int64: the same bits).  ``torch.as_tensor(env.bins_view(), device="cuda")``
        is a zero-copy tensor that every later fold updates; it is written on the env's stream, so read it there (or after
        ``sync()``)."""
        return BinsView(self, self.bins_device_ptr(), (self.n_books,) + self._bins_dims(), self._stream)

    def clear_bins(self, mask=None, sync: bool = True):
        """With a ``mask`` (one entry per BOOK): fold what is outstanding (raising as ``fold_bins`` does), then clear the
        counts and the carry of the books with ``mask[b]`` set.  ``None``: clear everything and count from the current step
        on without folding - the way on after lost steps.  ``mask`` / ``sync`` as ``clear_accounts`` takes them
        (``bk_bins_clear`` / ``bk_bins_clear_device``).  ``reset_books`` / ``reset_ingress_books`` fold and then cut only
        the carry of the books they reset: the counts go on across episodes and no span reaches over a reset."""
        # (no check of its own in front: the library refuses an env without the table)
        self._masked_clear(self._L.bk_bins_clear_device, self._L.bk_bins_clear, mask, sync)

    # ------------------------------------------------------------ open orders of an env with the device ingress
    OPEN_SUMMARY_DTYPE = _lib.OPEN_SUMMARY_DTYPE
    OPEN_ORDER_DTYPE = _lib.OPEN_ORDER_DTYPE

    def enable_open_orders(self, n_traders: int, depth: int = 8):
        """``bk_open_orders_enable``: keep, per book and for traders ``0 .. n_traders - 1``, a summary row (resting volume
        and order count per side, own best bid and ask) and the ``depth`` oldest resting orders (id, price, remaining
        volume, side) in device memory, recomputed from the pool on the env's stream behind every step and every
        ``reset_ingress_books`` with no host in the loop (trader ids >= ``n_traders`` - background members, say - are left
        out).  Call at any time after ``enable_device_ingress``; ``depth=0`` keeps the summary rows only.  The reference has
        no counterpart."""
        if not 0 <= int(n_traders) <= 0xFFFFFFFF or not 0 <= int(depth) <= 0xFFFFFFFF:
            raise ValueError("n_traders / depth out of range")
        check(self._L.bk_open_orders_enable(self._h, int(n_traders), int(depth)))
        self._open_shape = (int(n_traders), int(depth))

    def _open_orders_shape(self):
        if self._open_shape is None:
            raise _lib.BourseError(_lib.BK_INVALID, "this env has no open-order view: call enable_open_orders first")
        return self._open_shape

    def refresh_open_orders(self):
        """``bk_open_orders_refresh``: recompute every book's rows now (asynchronous on the env's stream), for callers
        that changed a pool outside a step."""
        self._open_orders_shape()
        check(self._L.bk_open_orders_refresh(self._h))

    def open_orders(self, first_book: int = 0, n_books: Optional[int] = None):
        """The rows of books ``[first_book, first_book + n_books)`` (default: to the last book) as of the last refresh:
        ``(summary[n, n_traders]`` of ``OPEN_SUMMARY_DTYPE``, ``entries[n, n_traders, depth]`` of ``OPEN_ORDER_DTYPE``
        or ``None`` with ``depth == 0)``.  A trader's entries are its resting orders in ascending order id; unused slots
        hold ``order_id == 0xFFFFFFFF``.  Waits for the env's stream."""
        nt, depth = self._open_orders_shape()
        summary, entries = self._book_rows(self._L.bk_get_open_orders, first_book, n_books, ((nt,), _lib.OPEN_SUMMARY_DTYPE),
                                           ((nt, depth), _lib.OPEN_ORDER_DTYPE) if depth else None)
        return summary, entries

    def open_orders_device_ptrs(self):
        """Device addresses ``(summary, entries)`` of ``bk_open_summary[n_books][n_traders]`` and
        ``bk_open_order[n_books][n_traders][depth]`` (``entries`` is ``None`` with ``depth == 0``)."""
        summary, entries = C.c_void_p(), C.c_void_p()
        check(self._L.bk_open_orders_device_ptrs(self._h, C.byref(summary), C.byref(entries)))
        return int(summary.value), (int(entries.value) if entries.value else None)

    def open_orders_views(self):
        """The two tables in place as objects with ``__cuda_array_interface__`` (``torch.as_tensor(view, device="cuda")``
        is a zero-copy tensor that every later step updates; written on the env's stream, so read it there or after
        ``sync()``): ``(summary_view, entries_view)``, the second ``None`` with ``depth == 0``.

        ``summary_view``: int64, shape ``(n_books, n_traders, 4)``, the last axis ``bid_vol, ask_vol, counts, best`` (the
        unsigned words read as int64: the same bits).  The last two words pack two ``u32`` each, the first in the low
        half: ``n_bid = counts & 0xFFFFFFFF``, ``n_ask = counts >> 32``, ``best_bid = best & 0xFFFFFFFF``,
        ``best_ask = (best >> 32) & 0xFFFFFFFF``.

        ``entries_view``: int32, shape ``(n_books, n_traders, depth, 4)``, the last axis ``order_id, price, vol,
        side_is_bid`` (the ``u32`` words read as int32: the same bits; an unused slot's ``order_id`` reads -1)."""
        nt, depth = self._open_orders_shape()
        summary, entries = self.open_orders_device_ptrs()
        return (OpenOrdersView(self, summary, (self.n_books, nt, 4), "<i8", self._stream),
                OpenOrdersView(self, entries, (self.n_books, nt, depth, 4), "<i4", self._stream) if depth else None)

    # ------------------------------------------------------------ queue positions of the open orders
    OPEN_QUEUE_DTYPE = _lib.OPEN_QUEUE_DTYPE

    def enable_open_queue(self):
        """``bk_open_queue_enable``: keep, beside every entry of the open-order view, where that resting order stands in
        its book's queue - the volume and the number of orders with priority over it (better-priced, or earlier at its own
        price), the part of both at its own price, and the whole volume of its level - in device memory, recomputed from
        the pool right behind the open-order rows wherever those are refreshed.  Every live order counts, whoever owns
        it.  Call at any time after ``enable_open_orders`` with ``depth > 0``.  The reference has no counterpart."""
        check(self._L.bk_open_queue_enable(self._h))
        self._open_queue = True

    def _open_queue_shape(self):
        if not self._open_queue:
            raise _lib.BourseError(_lib.BK_INVALID, "this env has no queue view: call enable_open_queue first")
        return self._open_orders_shape()

    def open_queue(self, first_book: int = 0, n_books: Optional[int] = None) -> np.ndarray:
        """The rows of books ``[first_book, first_book + n_books)`` (default: to the last book) as of the last refresh, a
        structured array of shape ``[n, n_traders, depth]`` (``OPEN_QUEUE_DTYPE``); row ``[b, t, k]`` belongs to entry
        ``[b, t, k]`` of ``open_orders()``, and an unused entry's row is all zeros.  Waits for the env's stream."""
        nt, depth = self._open_queue_shape()
        return self._book_rows(self._L.bk_get_open_queue, first_book, n_books, ((nt, depth), _lib.OPEN_QUEUE_DTYPE))[0]

    def open_queue_device_ptr(self) -> int:
        """Device address of the table, ``bk_open_queue[n_books][n_traders][depth]`` (for on-device consumers)."""
        self._open_queue_shape()
        return self._device_ptr(self._L.bk_open_queue_device_ptr)

    def open_queue_view(self) -> "OpenOrdersView":
        """The table in place as an object with ``__cuda_array_interface__`` (``torch.as_tensor(view, device="cuda")`` is
        a zero-copy tensor that every later step updates; written on the env's stream, so read it there or after
        ``sync()``): int64, shape ``(n_books, n_traders, depth, 4)``, the last axis ``ahead_vol, level_ahead_vol,
        level_vol, counts`` (the unsigned words read as int64: the same bits) with ``ahead_orders = counts & 0xFFFFFFFF``
        and ``level_ahead_orders = counts >> 32``."""
        nt, depth = self._open_queue_shape()
        return OpenOrdersView(self, self.open_queue_device_ptr(), (self.n_books, nt, depth, 4), "<i8", self._stream)

    # ------------------------------------------------------------ quotes: requote every trader from one dense table
    QUOTE_DTYPE = _lib.QUOTE_DTYPE
    QUOTE_KEEP = _lib.QUOTE_KEEP

    def submit_quotes(self, quotes, out_ids=None, status=None, check_status: bool = False):
        """``bk_submit_quotes_device`` / ``bk_submit_quotes``: one row ``(bid_price, bid_vol, ask_price, ask_vol)`` per
        book and trader of the open-order view, "this trader wants this bid and this ask".  Per side, against the trader's
        listed entries as the last refresh left them: ``vol == QUOTE_KEEP`` leaves the side alone, ``vol == 0`` cancels
        every listed order of it; otherwise the first listed order at the target price keeps (reduced in place when it
        holds more, topped up by a new order behind it when it holds less), every other listed order of the side is
        cancelled, and without a keeper a new limit order is placed.  The result is queued on the env's stream exactly
        as ``submit_instructions_device`` queues the dense grid ``n_traders x (depth + 2)`` (include/bourse_amd.h).

        ``quotes``: a torch CUDA tensor or ``__cuda_array_interface__`` object of 4-byte ints shaped ``(n_books,
        n_traders, 4)``, written on the env's stream (the device entry), or a numpy array of that shape / of
        ``QUOTE_DTYPE`` rows ``(n_books, n_traders)`` (the host entry).  ``out_ids`` (device, 8-byte, ``(n_books, n_traders,
        2)``) receives the ids of the new bid and ask, 2**64 - 1 elsewhere; ``status`` (device, 4-byte, 2 per book)
        ``{code, grid positions applied}``.  ``check_status`` behaves as on ``submit_instructions_device``."""
        if check_status and status is None:
            raise ValueError("check_status needs a status array")
        nt = self._open_shape[0] if self._open_shape else None  # (without the view the library refuses the call and says why)
        P = self._dev_ptr
        if _is_dev(quotes):
            ptr = P(quotes, 4, "quotes")
            if nt is not None and _dev_count(quotes) != self.n_books * nt * 4:
                raise ValueError(f"quotes: shape (n_books, n_traders, 4) = ({self.n_books}, {nt}, 4) is needed")
            check(self._L.bk_submit_quotes_device(self._h, ptr, P(out_ids, 8, "out_ids"), P(status, 4, "status")))
        else:
            if quotes is None:
                host = None
            elif isinstance(quotes, np.ndarray) and quotes.dtype == _lib.QUOTE_DTYPE:
                host = np.ascontiguousarray(quotes)
            else:
                q = np.asarray(quotes)
                if q.dtype.kind not in "iu":
                    raise ValueError("quotes: integers or QUOTE_DTYPE rows are needed")
                if q.size and (q.min() < 0 or q.max() > 0xFFFFFFFF):
                    raise ValueError("quotes: prices and volumes are 32-bit unsigned")
                host = np.ascontiguousarray(q.astype(np.uint32))
            if host is not None and nt is not None and host.nbytes != self.n_books * nt * 16:
                raise ValueError(f"quotes: shape (n_books, n_traders, 4) = ({self.n_books}, {nt}, 4) is needed")
            check(self._L.bk_submit_quotes(self._h, None if host is None else host.ctypes.data_as(C.c_void_p),
                                           P(out_ids, 8, "out_ids"), P(status, 4, "status")))
        if check_status:
            self.sync()
            _raise_on_status(status, "grid position")
        return out_ids, status


class _DeviceTableView:
    """A device-resident table of an env where it lives, for ``torch.as_tensor(view, device="cuda")``, cupy and anything
    else that reads ``__cuda_array_interface__``.  Keeps its env (and so the memory) alive."""

    def __init__(self, env, ptr: int, shape, typestr: str, stream: Optional[int]):
        self._env = env
        # version 3 of the interface: `stream` is the stream the data is written on - None when unknown (an env on its own
        # stream), 1 for the legacy default stream (whose handle 0 the interface disallows), else the handle
        self.__cuda_array_interface__ = {"shape": tuple(int(x) for x in shape), "typestr": typestr, "data": (int(ptr), False),
                                         "version": 3, "strides": None,
                                         "stream": None if stream is None else (stream if stream != 0 else 1)}


class OpenOrdersView(_DeviceTableView):
    """One table of ``ManyBookEnv.open_orders_views()`` where it lives, for ``torch.as_tensor(view, device="cuda")``, cupy
    and anything else that reads ``__cuda_array_interface__``.  Keeps its env (and so the memory) alive."""


class AccountsView(_DeviceTableView):
    """``ManyBookEnv.accounts_view()``: the accounts table where it lives, for ``torch.as_tensor(view, device="cuda")``,
    cupy and anything else that reads ``__cuda_array_interface__``.  Keeps its env (and so the memory) alive."""

    def __init__(self, env, ptr: int, shape, stream: Optional[int]):
        super().__init__(env, ptr, shape, "<i8", stream)


class TradeBarsView(AccountsView):
    """``ManyBookEnv.trade_bars_view()``: the ring of trade bars where it lives, read the same way."""


class SeriesView(AccountsView):
    """``ManyBookEnv.series_view()``: the table of series moments where it lives, read the same way."""


class DepthView(AccountsView):
    """``ManyBookEnv.depth_view()``: the depth table where it lives, read the same way."""


class CandlesView(AccountsView):
    """``ManyBookEnv.candles_view()``: the candle table where it lives, read the same way."""


class LagsView(AccountsView):
    """``ManyBookEnv.lags_view()``: the lag table where it lives, read the same way."""


class FlowView(AccountsView):
    """``ManyBookEnv.flow_view()``: the flow table where it lives, read the same way."""


class BinsView(AccountsView):
    """``ManyBookEnv.bins_view()``: the bin table where it lives, read the same way."""


class CrossView(AccountsView):
    """``ManyMarketEnv.cross_view()``: the cross table where it lives, read the same way."""


def sim_runner(env: ManyBookEnv, agents: Sequence[RandomAgents | tuple], n_steps: int):
    """``sim_runner(env, agents, seed, n_steps, _)`` (ref runner.rs:46-69) for every book of ``env``.

    The seed is the env's (book b: seed + book_offset + b): in the reference the RNG is a local of
    ``sim_runner``; here it is part of the device state so runs can be continued."""
    env.set_random_agents(agents)
    env.run(n_steps)


class ManyMarketEnv(ManyBookEnv):
    """``n_markets`` independent ``MarketEnv<ASSETS>`` (ref crates/step_sim/src/market_env.rs:46-340) in lockstep: the
    ``len(tick_sizes)`` books of a market share one clock, one RNG stream (market m: seed + market_offset + m) and one
    shuffled event queue.  Every ``ManyBookEnv`` reader works on the flat book index ``market * assets + asset``
    (``book()``); the mutators below take ``(market, asset)`` like ``MarketEnv``'s take ``asset`` / ``MarketOrderId``."""

    def __init__(self, n_markets: int, seed: int, start_time: int, tick_sizes: Sequence[int], step_size: int,
                 trading: bool = True, market_offset: int = 0, **kw):
        tick_sizes = [int(t) for t in tick_sizes]
        super().__init__(int(n_markets) * len(tick_sizes), seed, start_time, tick_sizes[0], step_size, trading,
                         book_offset=market_offset, assets=len(tick_sizes), tick_sizes=tick_sizes, **kw)
        self.n_markets, self.tick_sizes = int(n_markets), tick_sizes

    def book(self, market: int, asset: int) -> int:
        if not (0 <= market < self.n_markets and 0 <= asset < self.assets):
            raise IndexError("market / asset out of range")
        return market * self.assets + asset

    def reset_markets(self, mask, seeds=None, slot: int = 0, sync: bool = True):
        """``reset_books`` spelt by market: ``mask`` / ``seeds`` hold one element per market, and every book of a masked
        market goes back to the snapshot (with ``seeds``, all of them on the market's new RNG stream)."""
        self.reset_books(mask, seeds, slot, sync)

    def reset_ingress_markets(self, mask, seeds=None, slot: int = 0, sync: bool = True):
        """``reset_ingress_books`` spelt by market (an env with the device ingress): a masked market's books, and its
        queue, go back."""
        self.reset_ingress_books(mask, seeds, slot, sync)

    # ------------------------------------------------------------ per-market cross table of the level-2 history
    CROSS_DTYPE = _lib.CROSS_DTYPE

    def enable_cross(self, spans=(1,)):
        """``bk_cross_enable``: keep ``len(spans) * assets * assets`` rows of eight integer sums per MARKET in device memory,
        row ``(j, a, b)`` for the ordered pair asset ``a`` against asset ``b`` at span ``spans[j]`` (1 .. 64 steps each, at
        most four, any order): count, sums, squares and cross product of the two assets' changes of twice the mid over the
        span where both are defined, and count and sum of a's change times b's PREVIOUS one (``CROSS_DTYPE`` /
        ``bourse_amd.CROSS_FIELDS``; include/bourse_amd.h states what one step adds).  ``fold_cross()`` folds the steps run
        since the last fold from the history ring, on the env's stream; nothing leaves the device until ``cross()`` is read.
        Needs ``history_capacity > 0`` and ``assets >= 2``; works with ``run`` on every pipeline, ``step`` and the device
        ingress, with or without the per-book tables.  Steps before the call are not counted.  ``bourse_amd.cross_moments``
        turns the rows into covariance, correlation, beta and lead correlation.  The reference has no counterpart."""
        spans = tuple(int(h) for h in spans)
        slots = (spans + (0, 0, 0, 0))[:4]  # (more than four spans: the library refuses n_spans)
        words = [len(spans), *slots]
        if any(not 0 <= w <= 0xFFFFFFFF for w in words + list(spans)):
            raise ValueError("enable_cross: every value is a 32-bit unsigned integer")
        cfg = np.array(words, dtype=np.uint32)
        check(self._L.bk_cross_enable(self._h, cfg.ctypes.data_as(C.c_void_p)))
        self._cross_spans = len(spans)

    def _cross_dims(self) -> Tuple[int, int, int]:
        if not self._cross_spans:
            raise _lib.BourseError(_lib.BK_INVALID, "this env has no cross table: call enable_cross (bk_cross_enable) first")
        return self._cross_spans, self.assets, self.assets

    def cross_config(self) -> np.ndarray:
        """``bk_cross_config_get``: the configuration the table was enabled with, a ``CROSS_CONFIG_DTYPE`` record."""
        self._cross_dims()
        cfg = np.zeros((), dtype=_lib.CROSS_CONFIG_DTYPE)
        check(self._L.bk_cross_config_get(self._h, cfg.ctypes.data_as(C.c_void_p)))
        return cfg

    def fold_cross(self, sync: bool = False):
        """``bk_cross_fold``: queue the fold of every step run since the last fold (no new step: no launch).  Raises if one
        of them is no longer retained by the ring - more than ``history_capacity`` steps since the last fold, or
        ``clear_history()`` - naming how many were lost; rows, carry and cursor are then unchanged and ``clear_cross()``
        starts again."""
        check(self._L.bk_cross_fold(self._h))
        if sync:
            self.sync()

    def cross(self, first_market: int = 0, n_markets: Optional[int] = None) -> np.ndarray:
        """The rows of markets ``[first_market, first_market + n_markets)`` (default: to the last market) as a structured
        array of shape ``[n, n_spans, assets, assets]`` (``CROSS_DTYPE``).  Waits for the env's stream; does NOT fold."""
        dims = self._cross_dims()
        first = int(first_market)
        n = self.n_markets - first if n_markets is None else int(n_markets)
        if first < 0 or n < 0:
            raise ValueError("market range out of bounds")
        out = np.zeros((n,) + dims, dtype=_lib.CROSS_DTYPE)
        check(self._L.bk_get_cross(self._h, first, n, out.ctypes.data_as(C.c_void_p)))
        return out

    def cross_device_ptr(self) -> int:
        """Device address of the table, ``bk_cross_row[n_markets][n_spans][assets][assets]`` (for on-device consumers)."""
        return self._device_ptr(self._L.bk_cross_device_ptr)

    def cross_view(self) -> "CrossView":
        """The table in place as an object with ``__cuda_array_interface__``: int64, shape ``(n_markets, n_spans, assets,
        assets, 8)``, the words in ``CROSS_DTYPE``'s order (unsigned words read as int64: the same bits).
        ``torch.as_tensor(env.cross_view(), device="cuda")`` is a zero-copy tensor that every later fold updates; it is
        written on the env's stream, so read it there (or after ``sync()``)."""
        return CrossView(self, self.cross_device_ptr(), (self.n_markets,) + self._cross_dims() + (8,), self._stream)

    def clear_cross(self, mask=None, sync: bool = True):
        """With a ``mask`` (one entry per MARKET, as ``reset_markets`` takes it): fold what is outstanding (raising as
        ``fold_cross`` does), then clear the rows and the carry of the markets with ``mask[m]`` set.  ``None``: clear
        everything and count from the current step on without folding - the way on after lost steps.  ``mask`` / ``sync`` as
        ``clear_accounts`` takes them (``bk_cross_clear`` / ``bk_cross_clear_device``).  ``reset_markets`` /
        ``reset_ingress_markets`` fold and then cut only the carry of the markets they reset: the sums go on across episodes
        and no span or lead reaches over a reset."""
        # (no check of its own in front: the library refuses an env without the table)
        self._masked_clear(self._L.bk_cross_clear_device, self._L.bk_cross_clear, mask, sync, self.n_markets, "one per market")

    def place_order(self, market: int, asset: int, bid: bool, vol: int, trader_id: int, price: Optional[int] = None):
        """``MarketEnv::place_order(asset, side, vol, trader_id, price)`` (market_env.rs:163-176) -> per-asset order id"""
        return super().place_order(self.book(market, asset), bid, vol, trader_id, price)

    def cancel_order(self, market: int, asset: int, order_id: int):
        super().cancel_order(self.book(market, asset), order_id)

    def modify_order(self, market: int, asset: int, order_id: int, new_price: Optional[int] = None,
                     new_vol: Optional[int] = None):
        super().modify_order(self.book(market, asset), order_id, new_price, new_vol)


    def set_random_market_agents_per_market(self, rows):
        """RandomMarketAgents groups whose parameters differ per market (``bk_set_random_agents_per_book``): ``rows[m]``
        is market ``m``'s list of ``(asset, n, tick_range, vol_range, tick_size, rate)`` (or ``RandomMarketAgents``), as
        ``set_random_market_agents`` takes it; ``asset`` and ``n`` must be the same in every market."""
        rows = [[g.as_tuple() if isinstance(g, RandomMarketAgents) else tuple(g) for g in row] for row in rows]
        if len(rows) != self.n_markets:
            raise ValueError(f"the table needs one row of groups per market: {self.n_markets} rows, got {len(rows)}")
        if not rows or not rows[0] or any(len(r) != len(rows[0]) for r in rows):
            raise ValueError("every row of the table needs the same number (>= 1) of groups")
        assets = np.array([int(g[0]) for g in rows[0]], dtype=np.uint32)
        if any([int(g[0]) for g in r] != list(assets) for r in rows):
            raise ValueError("the groups' assets must be the same in every market")
        arr = _agents_table([[g[1:] for g in r] for r in rows], self.n_markets, lambda g: g)
        check(self._L.bk_set_random_agents_per_book(self._h, arr.shape[1], arr.ctypes.data_as(C.c_void_p), _lib.p32(assets)))
        self.groups = None

    def set_market_agents_per_market(self, rows):
        """MarketAgentSet members whose parameters differ per market (``bk_set_agents_per_book``): ``rows[m]`` is market
        ``m``'s ``[(asset, member), ...]`` list as ``set_market_agents`` takes it; each member's asset, kind and ``n`` must
        be the same in every market."""
        rows = [list(r) for r in rows]
        if len(rows) != self.n_markets:
            raise ValueError(f"the table needs one row of members per market: {self.n_markets} rows, got {len(rows)}")
        if not rows or not rows[0] or any(len(r) != len(rows[0]) for r in rows):
            raise ValueError("every row of the table needs the same number (>= 1) of members")
        assets = [int(a) for a, _ in rows[0]]
        if any([int(a) for a, _ in r] != assets for r in rows):
            raise ValueError("the members' assets must be the same in every market")
        self._set_members_table([[m for _, m in r] for r in rows], self.n_markets, assets)

    def retune_random_market_agents(self, rows, mask=None, status=None, sync: bool = True):
        """``retune_random_agents`` per market, for the table ``set_random_market_agents_per_market`` installed: ``rows[m]``
        as that call takes it (the groups' assets stay what was installed) or a device object of the raw rows
        ``[n_markets, n_groups]``; ``mask`` / ``status`` hold one element / pair per market."""
        if not (_is_dev(rows) or isinstance(rows, np.ndarray)):
            rows = [[(g.as_tuple() if isinstance(g, RandomMarketAgents) else tuple(g))[1:] for g in row] for row in rows]
        self._retune(False, rows, mask, status, sync, lambda t: _agents_table(t, self.n_markets, lambda g: g))

    def retune_market_agents(self, rows, mask=None, status=None, sync: bool = True):
        """``retune_agents`` per market, for the table ``set_market_agents_per_market`` installed: ``rows[m]`` is market
        ``m``'s ``[(asset, member), ...]`` list (the members' assets stay what was installed) or a device object of the raw
        rows ``[n_markets, n_members]``."""
        if not (_is_dev(rows) or isinstance(rows, np.ndarray)):
            rows = [[m for _, m in r] for r in rows]
        self._retune(True, rows, mask, status, sync, lambda t: _members_rows(t, self.n_markets))

    # Market::save_json / load_json (market.rs:367-390): {"order_books": [OrderBook; ASSETS]}
    def market_state(self, market: int, trading: bool = True) -> dict:
        return {"order_books": [self.book_state(self.book(market, a), trading) for a in range(self.assets)]}

    def load_market_state(self, market: int, state: dict):
        if len(state["order_books"]) != self.assets:
            raise ValueError("snapshot holds a different number of assets")
        for a, s in enumerate(state["order_books"]):
            self.load_book_state(self.book(market, a), s)

    def save_json(self, market: int, path: str, pretty: bool = False, trading: bool = True):
        import json

        with open(path, "w") as f:
            json.dump(self.market_state(market, trading), f, **({"indent": 2} if pretty else {"separators": (",", ":")}))

    def load_json(self, market: int, path: str):
        import json

        with open(path) as f:
            self.load_market_state(market, json.load(f))


def _member_tuple(m) -> tuple:
    """An AgentSet member in ``set_agents``' tuple format: ``("random", n, tick_range, vol_range, tick_size, rate)`` or
    ``("noise"|"momentum", id_start, n, params_dict)``."""
    if isinstance(m, RandomAgents):
        return ("random",) + m.as_tuple()
    if isinstance(m, (NoiseAgent, MomentumAgent)):
        return m.as_tuple()
    return tuple(m)


def _fill_agent_desc(d, m: tuple):
    if m[0] == "random":
        _, n, tr, vr, ts, rate = m
        d.type, d.n_agents, d.tick_size, d.activity_rate = 0, int(n), int(ts), float(np.float32(rate))
        d.tick_lo, d.tick_hi, d.vol_lo, d.vol_hi = int(tr[0]), int(tr[1]), int(vr[0]), int(vr[1])
    else:
        kind, start, n, p = m
        d.type = 1 if kind == "noise" else 2
        d.agent_id_start, d.n_agents, d.tick_size = int(start), int(n), int(p["tick_size"])
        d.p_cancel, d.trade_vol = float(np.float32(p["p_cancel"])), int(p["trade_vol"])
        d.price_dist_mu, d.price_dist_sigma = float(p["price_dist_mu"]), float(p["price_dist_sigma"])
        if kind == "noise":
            d.p_limit, d.p_market = float(np.float32(p["p_limit"])), float(np.float32(p["p_market"]))
        else:
            d.decay, d.demand = float(p["decay"]), float(p["demand"])
            d.scale, d.order_ratio = float(p["scale"]), float(p["order_ratio"])


def _members_array(rows, n_units: int):
    """The flat AgentDesc array (unit-major) of ``n_units`` equally long rows of member tuples."""
    n = len(rows[0])
    arr = (AgentDesc * (n_units * n))()
    for u, row in enumerate(rows):
        for i, m in enumerate(row):
            _fill_agent_desc(arr[u * n + i], m)
    return arr


def _members_rows(table, n_units: int) -> np.ndarray:
    """A contiguous (n_units, n_members) AGENT_DESC_DTYPE array from a structured array or per-unit member lists in
    ``set_agents``' format; the shape is checked here (ValueError) before the library sees it."""
    if isinstance(table, np.ndarray) and table.dtype.names is not None:
        if table.ndim != 2 or table.shape[0] != n_units or table.shape[1] == 0:
            raise ValueError(f"the table must be (n_units = {n_units}, n_members >= 1), got {table.shape}")
        if table.dtype != _lib.AGENT_DESC_DTYPE:
            table = table.astype(_lib.AGENT_DESC_DTYPE)
        return np.ascontiguousarray(table)
    rows = [[_member_tuple(m) for m in row] for row in table]
    if len(rows) != n_units:
        raise ValueError(f"the table needs one row of members per unit: {n_units} rows, got {len(rows)}")
    n = len(rows[0]) if rows else 0
    if n == 0 or any(len(r) != n for r in rows):
        raise ValueError("every row of the table needs the same number (>= 1) of members")
    return np.frombuffer(_members_array(rows, n_units), dtype=_lib.AGENT_DESC_DTYPE).reshape(n_units, n).copy()


def _agents_table(table, n_units: int, as_tuple) -> np.ndarray:
    """A contiguous (n_units, n_groups) RANDOM_AGENTS_DTYPE array from a structured array or per-unit group lists of
    ``(n, tick_range, vol_range, tick_size, rate)``; the shape is checked here (ValueError) before the library sees it."""
    if isinstance(table, np.ndarray) and table.dtype.names is not None:
        if table.ndim != 2 or table.shape[0] != n_units or table.shape[1] == 0:
            raise ValueError(f"the table must be (n_units = {n_units}, n_groups >= 1), got {table.shape}")
        if table.dtype != _lib.RANDOM_AGENTS_DTYPE:
            table = table.astype(_lib.RANDOM_AGENTS_DTYPE)
        return np.ascontiguousarray(table)
    rows = [[as_tuple(g) for g in row] for row in table]
    if len(rows) != n_units:
        raise ValueError(f"the table needs one row of groups per unit: {n_units} rows, got {len(rows)}")
    n_groups = len(rows[0]) if rows else 0
    if n_groups == 0 or any(len(r) != n_groups for r in rows):
        raise ValueError("every row of the table needs the same number (>= 1) of groups")
    arr = np.zeros((n_units, n_groups), dtype=_lib.RANDOM_AGENTS_DTYPE)
    for u, row in enumerate(rows):
        for g, (n, tr, vr, ts, rate) in enumerate(row):
            arr[u, g] = (int(n), int(tr[0]), int(tr[1]), int(vr[0]), int(vr[1]), int(ts), np.float32(rate))
    return arr


def market_sim_runner(env: ManyMarketEnv, agents: Sequence[RandomMarketAgents | tuple], n_steps: int):
    """``market_sim_runner(env, agents, seed, n_steps, _)`` (ref runner.rs:108-131) for every market of ``env``."""
    env.set_random_market_agents(agents)
    env.run(n_steps)
