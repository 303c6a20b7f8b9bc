"""The expected side of tests/test_gpu_tables_step_carry.py, without a GPU: the oracle's runs and the tables' plain-Python
models only.  What is asserted here keeps the GPU test from passing trivially - every book is busy over the carry, the
candle bars lie on both sides of 2^32 in slots of their own, the reset's cut shows in every table of every masked unit -
and, for the one table whose words depend on the step number, that the model fed step numbers cut to 32 bits gives another
table: a 32-bit cut anywhere between steps_done and the kernel's arguments then cannot go unnoticed.  The GPU test asserts
the same conditions again before it compares anything (tests/tables_step_carry.py::Plan.conditions)."""
import numpy as np
import pytest

pytest.register_assert_rewrite("hist_tables", "tables_step_carry")  # (support modules: their asserts report their values too)

import candles_model as CM  # noqa: E402
import tables_step_carry as SC  # noqa: E402

each_flow = pytest.mark.parametrize("name", SC.FLOWS)


def test_the_constants_put_a_truncated_step_in_another_bar_phase_and_slot():
    assert SC.FLOWS == ("fused", "wave_split", "members", "market") and (SC.BOOKS, SC.RING, SC.ASSETS) == (6, 12, 2)
    assert SC.M32 % SC.RING == 4 and SC.M32 % SC.CANDLE_W == 1 and SC.M32 % (SC.CANDLE_W * SC.CANDLE_N) == 4
    W, N = SC.CANDLE_W, SC.CANDLE_N
    for s in range(SC.M32, SC.START + SC.T1 + SC.T2 + SC.T3 + SC.LOST):  # every step behind the carry, against its low word
        t = s % SC.M32
        assert s % SC.RING != t % SC.RING and s % W != t % W and s // W != t // W and s // W % N != t // W % N, s
    assert max(SC.N_OF.values()) + SC.T1 + SC.T2 + SC.T3 + SC.LOST < 60 and SC.T2 <= SC.RING and SC.LOST == SC.RING + 1
    assert SC.BAR_STARTS == sorted({max(s // W * W, SC.START) for s in range(SC.START, SC.START + SC.T1)})


@each_flow
def test_the_expected_tables_are_busy_over_the_carry_and_the_cut_shows(oracle, name):
    p = SC.plan(oracle, name)
    assert set(p.want) == set(SC.tables_of(name)) and (p.flow is None) == (name == "market") and ("cross" in p.want) == (name == "market")
    p.conditions()
    for t, w in p.want.items():  # no stage is trivially the cleared table, and the stages differ from each other
        for stage in ("T1", "at_reset", "T3", "third"):
            assert w[stage].shape == w["cleared"].shape and w[stage].tobytes() != w["cleared"].tobytes(), (t, stage)
        assert len({w[s].tobytes() for s in ("T1", "at_reset", "T3", "third")}) == 4, t


@each_flow
def test_a_step_number_cut_to_32_bits_changes_the_candle_table_and_no_other(oracle, name):
    """the bars' first_step, bar and slot come from the absolute step: steps 2^32 .. fold into bars 0 .. of the truncated model"""
    p = SC.plan(oracle, name)
    w = p.want["candles"]
    for stage in ("T1", "third"):
        assert w[stage].tobytes() != w[stage + "_cut_to_32_bits"].tobytes(), stage
    cut = w["T1_cut_to_32_bits"]
    assert (cut["first_step"] < SC.M32).all() and (w["T1"]["first_step"] >= SC.M32).any()
    assert (w["third"]["first_step"][w["third"]["n_steps"] > 0] > SC.M32).all()
    assert (w["third_cut_to_32_bits"]["first_step"] < SC.M32).all()
    # the other tables' words hold no step number: they cannot tell, and are held to the device through their sums alone
    assert p.step_free() == [t for t in SC.tables_of(name) if t != "candles"]


@each_flow
def test_the_oracles_shorter_runs_are_prefixes_of_the_long_one(oracle, name):
    """every stage slices ONE history: the oracle after L steps is the first L steps of the oracle after L3"""
    p = SC.plan(oracle, name)
    for L in (p.n, p.L1, p.L2, p.L1 + SC.T3):
        h, _ = p.F.ref(L)
        assert h.shape[0] == L and np.array_equal(h, p.hist[:L]), L


def test_the_candle_model_of_the_first_ten_steps_by_hand():
    """ten records of one two-sided book with mid 100 + i: the bars of steps 2^32 - 3 .. 2^32 + 6 at W = 3, N = 4"""
    hist = np.zeros((SC.T1, 9), dtype=np.uint32)
    hist[:, 1], hist[:, 2] = 99 + np.arange(SC.T1), 101 + np.arange(SC.T1)
    rows = CM.table(CM.fold(hist, SC.CFG["candles"], first_step=SC.START))
    assert rows["first_step"].tolist() == SC.BAR_STARTS and rows["n_steps"].tolist() == [2, 3, 3, 2]
    assert rows["open_m"].tolist() == [200, 204, 210, 216] and rows["n_ret"].tolist() == [1, 3, 3, 2]
