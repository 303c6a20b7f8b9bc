"""Oracle RNG restatement vs. the only external anchors available.

PARITY UNPINNED for everything except the generator recurrence: the reference's Rust cannot run
here and none of its tests asserts an RNG-dependent value.
"""
import numpy as np

from agents_model import gen_range as _py_gen_range, shuffle as _py_shuffle


def test_xoroshiro128starstar_known_answer(oracle):
    # Published known-answer vector of xoroshiro128** for state (1, 2)
    # (rand_xoshiro 0.6.0's own reference test for Xoroshiro128StarStar).
    r = oracle.Rng(state=(1, 2))
    expect = [
        5760, 97769243520, 9706862127477703552, 9223447511460779954, 8358291023205304566,
        15695619998649302768, 8517900938696309774, 16586480348202605369, 6959129367028440372,
        16822147227405758281,
    ]
    assert [r.next_u64() for _ in range(10)] == expect


def _splitmix(x):
    M = (1 << 64) - 1
    x = (x + 0x9E3779B97F4A7C15) & M
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    return x, z ^ (z >> 31)


def test_seed_from_u64_is_splitmix64(oracle):
    # rand_xoshiro `from_splitmix!`: s0, s1 = first two SplitMix64 outputs
    for seed in (0, 1, 101, 2**63 + 12345, 2**64 - 1):
        x, a = _splitmix(seed)
        x, b = _splitmix(x)
        st = oracle.Rng(seed=seed).st
        assert (int(st[0]), int(st[1])) == (a, b)
    st = oracle.Rng(seed=101).st
    assert (int(st[0]), int(st[1])) == (0xD1024A5FAD64D717, 0x0466A7D0954B76A3)


def test_next_u32_is_low_half_and_f32_scaling(oracle):
    a, b = oracle.Rng(seed=7), oracle.Rng(seed=7)
    for _ in range(64):
        v = a.next_u64()
        assert b.next_u32() == v & 0xFFFFFFFF
    a, b = oracle.Rng(seed=9), oracle.Rng(seed=9)
    for _ in range(64):
        v = a.next_u32()
        f = b.gen_f32()
        assert f == np.float32(v >> 8) * np.float32(2.0**-24)
        assert 0.0 <= f < 1.0


def test_gen_range_and_shuffle_match_python_restatement(oracle):
    # UniformInt::sample_single + SliceRandom::shuffle restated independently in Python (App. B.3/B.4): tests/agents_model.py
    for lo, hi in ((0, 2), (10, 100), (32, 64), (10, 20), (50, 70), (0, 129), (5, 6)):
        a, b = oracle.Rng(seed=lo * 1000 + hi), oracle.Rng(seed=lo * 1000 + hi)
        for _ in range(200):
            x = a.gen_range(lo, hi)
            assert x == _py_gen_range(b, lo, hi)
            assert lo <= x < hi
        assert tuple(a.st) == tuple(b.st)
    for n in (0, 1, 2, 3, 17, 64, 128, 500):
        a, b = oracle.Rng(seed=n), oracle.Rng(seed=n)
        got = a.shuffle(np.arange(n, dtype=np.uint32))
        ref = _py_shuffle(b, list(range(n)))
        assert got.tolist() == ref
        assert tuple(a.st) == tuple(b.st)
        assert sorted(got.tolist()) == list(range(n))
