"""Move the 64-bit counters of a checkpoint image, so that a restored env starts next to a carry into their high words.

The image is the documented layout (bk_checkpoint_save): an 8 x u64 header with ``steps_done`` in word 1; then per book
``stride = 64 + 320 R`` dwords - 64 header dwords indexed by ``Hdr`` (book_device.hpp), then the pool rows; then the books'
latest level-2 records.  ``shift`` adds, modulo 2^64 and per book,

* ``trades[b]`` to H_TRADES and H_TRADE_BASE together (the retained records' window moves with the count),
* ``events[b]`` to H_EVENTS,
* ``steps`` - one number, the books step together - to every book's H_STEPS and to the header's ``steps_done``,

and touches nothing else.  Plain module next to oracle_parity.py; needs numpy alone.
"""
import numpy as np

HEADER_WORDS = 8          # u64
STEPS_DONE = 1            # header word
HDR_DW = 64
# Hdr (book_device.hpp): the low dword of each two-word counter; the high dword follows
H_SEQ = 7
H_TRADES, H_STEPS, H_EVENTS, H_TRADE_BASE = 8, 12, 14, 17
M64 = (1 << 64) - 1


def stride_of(pool_slots):
    return HDR_DW + 5 * pool_slots


def books_view(img, n_books, pool_slots):
    """[n_books, stride] u32 view of the image's state blocks (writes go through to ``img``)."""
    stride = stride_of(pool_slots)
    assert img.dtype == np.uint8 and img.ndim == 1 and len(img) >= HEADER_WORDS * 8 + n_books * stride * 4
    return img[HEADER_WORDS * 8:HEADER_WORDS * 8 + n_books * stride * 4].view(np.uint32).reshape(n_books, stride)


def read64(st, word):
    """The two-word counter at header dword ``word`` of every book, as Python ints."""
    return [(int(hi) << 32) | int(lo) for lo, hi in zip(st[:, word], st[:, word + 1])]


def _add64(st, word, add):
    for b, a in enumerate(add):
        v = (((int(st[b, word + 1]) << 32) | int(st[b, word])) + int(a)) & M64
        st[b, word], st[b, word + 1] = v & 0xFFFFFFFF, v >> 32


def shift(img, n_books, pool_slots, trades=None, events=None, steps=0):
    """A shifted copy of ``img``."""
    out = np.array(img, dtype=np.uint8, copy=True)
    st = books_view(out, n_books, pool_slots)
    if trades is not None:
        assert len(trades) == n_books
        _add64(st, H_TRADES, trades)
        _add64(st, H_TRADE_BASE, trades)
    if events is not None:
        assert len(events) == n_books
        _add64(st, H_EVENTS, events)
    if steps:
        _add64(st, H_STEPS, [steps] * n_books)
        head = out[:HEADER_WORDS * 8].view(np.uint64)
        head[STEPS_DONE] = np.uint64((int(head[STEPS_DONE]) + int(steps)) & M64)
    return out
