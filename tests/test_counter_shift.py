"""tests/counter_shift.py on a synthetic checkpoint image: the carry into the counters' high words, modulo 2^64, and that
nothing else of the image moves - the other header words, the pool rows, the level-2 records behind the state blocks."""
import numpy as np
import pytest

import counter_shift as CS

M32 = 0xFFFFFFFF


def _image(n_books, pool_slots, w, seed):
    rng = np.random.default_rng(seed)
    stride = CS.stride_of(pool_slots)
    img = rng.integers(0, 256, size=64 + n_books * (stride + w) * 4, dtype=np.uint8)
    return img


def _words(img, n_books, pool_slots):
    return CS.books_view(img.copy(), n_books, pool_slots)


@pytest.mark.parametrize("pool_slots", [64, 128, 256, 512])
def test_the_shift_carries_and_leaves_everything_else(pool_slots):
    B, W = 5, 13
    img = _image(B, pool_slots, W, pool_slots)
    st0 = CS.books_view(img, B, pool_slots)
    # counters whose low words are next to the carry, one book already past it, one that wraps modulo 2^64
    lows = [M32 - 2, M32, 0, 7, M32 - 1]
    highs = [0, 0, 1, M32, M32]
    for w in (CS.H_TRADES, CS.H_EVENTS, CS.H_STEPS, CS.H_TRADE_BASE):
        st0[:, w], st0[:, w + 1] = lows, highs
    st0[:, CS.H_TRADE_BASE] = [5, 6, 0, 1, 2]  # the base trails the count
    head0 = img[:64].view(np.uint64)
    head0[CS.STEPS_DONE] = np.uint64(M32 - 2)
    before = img.copy()
    trades, events, steps = [3, 1, 0, 2 ** 33, 2], [0, 1, M32, 1, 5], 3

    out = CS.shift(img, B, pool_slots, trades=trades, events=events, steps=steps)
    assert np.array_equal(img, before), "the input image is not modified"
    st = _words(out, B, pool_slots)
    was = _words(before, B, pool_slots)
    t0, e0, s0, b0 = (CS.read64(was, w) for w in (CS.H_TRADES, CS.H_EVENTS, CS.H_STEPS, CS.H_TRADE_BASE))
    assert CS.read64(st, CS.H_TRADES) == [(x + a) & CS.M64 for x, a in zip(t0, trades)]
    assert CS.read64(st, CS.H_TRADE_BASE) == [(x + a) & CS.M64 for x, a in zip(b0, trades)]
    assert CS.read64(st, CS.H_EVENTS) == [(x + a) & CS.M64 for x, a in zip(e0, events)]
    assert CS.read64(st, CS.H_STEPS) == [(x + steps) & CS.M64 for x in s0]
    # the carries themselves, spelled out: low word wraps, high word takes the one
    assert (int(st[0, CS.H_TRADES]), int(st[0, CS.H_TRADES + 1])) == (0, 1)
    assert (int(st[1, CS.H_TRADES]), int(st[1, CS.H_TRADES + 1])) == (0, 1)
    assert (int(st[1, CS.H_EVENTS]), int(st[1, CS.H_EVENTS + 1])) == (0, 1)
    assert (int(st[4, CS.H_TRADES]), int(st[4, CS.H_TRADES + 1])) == (0, 0)  # 2^64 - 2 + 2: modulo 2^64
    assert (int(st[0, CS.H_STEPS]), int(st[0, CS.H_STEPS + 1])) == (0, 1)
    assert int(out[:64].view(np.uint64)[CS.STEPS_DONE]) == 2 ** 32
    # untouched: every other header dword, every pool row, the file header's other words, the level-2 records
    moved = {w + k for w in (CS.H_TRADES, CS.H_EVENTS, CS.H_STEPS, CS.H_TRADE_BASE) for k in (0, 1)}
    keep = [i for i in range(CS.stride_of(pool_slots)) if i not in moved]
    assert np.array_equal(st[:, keep], was[:, keep])
    assert np.array_equal(st[:, CS.HDR_DW:], was[:, CS.HDR_DW:])
    h, h_was = out[:64].view(np.uint64), before[:64].view(np.uint64)
    assert [int(x) for i, x in enumerate(h) if i != CS.STEPS_DONE] == [int(x) for i, x in enumerate(h_was) if i != CS.STEPS_DONE]
    tail = 64 + B * CS.stride_of(pool_slots) * 4
    assert np.array_equal(out[tail:], before[tail:]) and len(out) == len(before)


def test_parts_of_the_shift_and_the_header_indices():
    B, P = 3, 64
    img = _image(B, P, 9, 1)
    # nothing asked: a copy
    assert np.array_equal(CS.shift(img, B, P), img)
    only_events = CS.shift(img, B, P, events=[1, 2, 3])
    a, b = _words(only_events, B, P), _words(img, B, P)
    diff = np.flatnonzero((a != b).any(axis=0)).tolist()
    assert set(diff) <= {CS.H_EVENTS, CS.H_EVENTS + 1} and CS.H_EVENTS in diff
    assert np.array_equal(only_events[:64], img[:64])
    # the indices are book_device.hpp's Hdr
    import os
    import re

    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bourse_amd", "csrc", "book_device.hpp")).read()
    body = re.search(r"enum Hdr : int \{(.*?)\};", src, re.S).group(1)
    names = [n for n in re.findall(r"\b(H_\w+)\b(?:\s*=\s*\d+)?\s*,", re.sub(r"//.*", "", body))]
    assert names.index("H_SEQ") == CS.H_SEQ
    assert names.index("H_TRADES_LO") == CS.H_TRADES and names.index("H_TRADES_HI") == CS.H_TRADES + 1
    assert names.index("H_STEPS_LO") == CS.H_STEPS and names.index("H_EVENTS_LO") == CS.H_EVENTS
    assert names.index("H_TRADE_BASE_LO") == CS.H_TRADE_BASE and names.index("H_TRADE_BASE_HI") == CS.H_TRADE_BASE + 1
    with pytest.raises(AssertionError):
        CS.shift(img, B, P, trades=[1, 2])
