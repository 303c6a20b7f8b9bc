"""The stamp compaction as a plain sort, and what the tests of the stamp wrap need to reason about stamps.

A book's resting orders carry u32 arrival stamps handed out by a counter that grows by one per order that rests (a New that
does not fill at once, a modification that re-keys).  ``compact`` is the rule of bourse_amd/csrc/stamp_rows.hpp restated
without its arithmetic: order the live stamps by when they were handed out - walking BACK from the counter, modulo 2^32 - and
number them 0, 1, 2, ... oldest first; the counter becomes the live count.  Plain module; needs nothing.
"""
M32 = 1 << 32


def compact(seq_ctr, live, seq):
    """(new counter, new stamps): live slots get their rank, dead slots keep their word."""
    idx = [i for i, l in enumerate(live) if l]
    # handed out k rests ago <=> seq == (seq_ctr - k) mod 2^32, k in 1 .. 2^32 (k = 2^32 and k = 0 are the same residue: a
    # live stamp equal to the counter was handed out a full turn ago only if the invariant is already broken)
    back = {i: (seq_ctr - seq[i]) % M32 for i in idx}
    order = sorted(idx, key=lambda i: -back[i])
    out = list(seq)
    for rank, i in enumerate(order):
        out[i] = rank
    return len(idx), out
