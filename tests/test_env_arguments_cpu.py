"""What ``bourse_amd.env`` asks of the arguments of its masked and device entries, checked without a GPU: the helpers
every ``reset_*`` / ``clear_*`` / ``retune_*`` / ``submit_*`` method shares, driven with numpy arrays and a stub that
carries nothing but a ``__cuda_array_interface__`` dictionary.  Exception types and texts are the public ones."""
import numpy as np
import pytest

from bourse_amd import _lib, env as E


class Stub:
    """A device object as cupy / numba would hand one over (never dereferenced here)."""

    def __init__(self, shape, typestr, strides=None):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (0x1000, False), "version": 3,
                                         "strides": strides}


# ---------------------------------------------------------------- host masks, n = 3
@pytest.mark.parametrize("dtype", [np.bool_, np.uint8])
def test_host_mask_accepts_bool_and_uint8(dtype):
    m = E._host_mask(np.array([1, 0, 1], dtype=dtype), 3, "one per book")
    assert m.dtype == np.uint8 and m.shape == (3,) and m.flags.c_contiguous and m.tolist() == [1, 0, 1]


def test_host_mask_takes_a_list_of_bools():
    assert E._host_mask([True, False, False], 3, "one per book").tolist() == [1, 0, 0]


def test_host_mask_refuses_other_dtypes():
    with pytest.raises(ValueError) as e:
        E._host_mask(np.array([1, 0, 1], dtype=np.int64), 3, "one per book")
    assert str(e.value) == "mask: a bool or uint8 array is needed"


@pytest.mark.parametrize("shape", [(2,), (3, 1)])
@pytest.mark.parametrize("per", ["one per book", "one per book, or per market"])
def test_host_mask_refuses_other_shapes(shape, per):
    with pytest.raises(ValueError) as e:
        E._host_mask(np.zeros(shape, dtype=np.uint8), 3, per)
    assert str(e.value) == f"mask: 3 elements are needed ({per})"


def test_host_mask_of_the_resets_names_mask_and_seeds():
    with pytest.raises(ValueError) as e:
        E._host_mask(np.zeros(2, dtype=np.bool_), 3, "one per book, or per market", name="mask / seeds")
    assert str(e.value) == "mask / seeds: 3 elements are needed (one per book, or per market)"


def test_host_mask_copies_a_strided_view():
    base = np.array([1, 9, 0, 9, 1, 9], dtype=np.uint8)
    view = base[::2]
    assert not view.flags.c_contiguous
    m = E._host_mask(view, 3, "one per book")
    assert m.flags.c_contiguous and m.tolist() == [1, 0, 1] and not np.shares_memory(m, base)


# ---------------------------------------------------------------- device objects
def test_device_objects_are_told_from_host_arrays():
    assert E._is_dev(Stub((3,), "|u1")) and not E._is_dev(np.zeros(3, dtype=np.uint8)) and not E._is_dev([1, 0, 1])


@pytest.mark.parametrize("typestr,width", [("|u1", 1), ("<u8", 8)])
def test_device_element_and_byte_counts(typestr, width):
    x = Stub((4, 3), typestr)
    assert E._dev_count(x) == 12 and E._dev_bytes(x) == 12 * width
    assert E._dev_count(Stub((0,), typestr)) == 0 and E._dev_bytes(Stub((0,), typestr)) == 0
    assert E.ManyBookEnv._dev_ptr(x, width, "x").value == 0x1000
    assert E.ManyBookEnv._dev_ptr(None, width, "x") is None


def test_dev_ptr_refuses_strides():
    with pytest.raises(ValueError) as e:
        E.ManyBookEnv._dev_ptr(Stub((3,), "|u1", strides=(2,)), 1, "mask")
    assert str(e.value) == "mask: a contiguous device array of 1-byte elements is needed"


@pytest.mark.parametrize("typestr,want", [("|u1", 8), ("<u8", 1), ("<i4", 8)])
def test_dev_ptr_refuses_the_wrong_width(typestr, want):
    with pytest.raises(ValueError) as e:
        E.ManyBookEnv._dev_ptr(Stub((3,), typestr), want, "seeds")
    assert str(e.value) == f"seeds: a contiguous device array of {want}-byte elements is needed"


# ---------------------------------------------------------------- the status of check_status=True, three books
def _status(book=None, code=0, applied=0):
    st = np.zeros((3, 2), dtype=np.uint32)
    if book is not None:
        st[book] = (code, applied)
    return st


@pytest.mark.parametrize("unit", ["element", "grid position"])
def test_status_without_a_failure_raises_nothing(unit):
    assert E._raise_on_status(_status(), unit) is None
    assert E._raise_on_status(_status().view(np.int32).reshape(-1), unit) is None  # (as a flat int32 tensor comes back)


def test_status_price_code_of_a_batch():
    with pytest.raises(ValueError) as e:
        E._raise_on_status(_status(1, _lib.BK_PRICE, 5), "element")
    assert str(e.value) == ("book 1: a price of its batch was not a multiple of the tick size "
                            "(element 5 of the book's batch; earlier elements are queued)")


def test_status_price_code_of_quotes():
    with pytest.raises(ValueError) as e:
        E._raise_on_status(_status(1, _lib.BK_PRICE, 5), "grid position")
    assert str(e.value) == ("book 1: a quoted price was not a multiple of the tick size "
                            "(grid position 5 of the book's batch; earlier positions are queued)")


@pytest.mark.parametrize("unit,tail", [("element", "7 elements"), ("grid position", "7 grid positions")])
def test_status_other_code_is_a_capacity_error(unit, tail):
    with pytest.raises(_lib.CapacityError) as e:
        E._raise_on_status(_status(2, _lib.BK_CAPACITY, 7), unit)
    assert e.value.code == _lib.BK_CAPACITY
    assert str(e.value) == f"bourse_amd status {_lib.BK_CAPACITY}: book 2: event queue / id space exhausted after {tail}"


def test_status_reports_the_lowest_failing_book():
    st = _status(2, _lib.BK_CAPACITY, 7)
    st[1] = (_lib.BK_PRICE, 0)
    with pytest.raises(ValueError, match=r"^book 1: .*\(element 0 of"):
        E._raise_on_status(st, "element")
