"""CPU: the guard-band checker of tests/abi_guard.py catches what it is there to catch.

tests/test_gpu_abi_confinement.py trusts it to see a single element written outside the rows a
kernel was given; here such writes are planted by hand, on torch CPU tensors and numpy arrays.
"""
import numpy as np
import pytest
import torch

import abi_guard as ag

ROWS, WIDTH = 5, 12
TORCH_DTYPES = [torch.float32, torch.float64, torch.int32]
NP_DTYPES = [np.float32, np.float64, np.int32, np.uint32]


def _make(kind, dtype, rows=ROWS, width=WIDTH):
    return ag.banded(rows, width, dtype) if kind == "torch" else ag.banded_np(rows, width, dtype)


CASES = [("torch", d) for d in TORCH_DTYPES] + [("numpy", d) for d in NP_DTYPES]
_ids = [f"{k}-{str(d)[6:] if k == 'torch' else np.dtype(d).name}" for k, d in CASES]


@pytest.mark.parametrize("kind,dtype", CASES, ids=_ids)
def test_layout_and_sentinel(kind, dtype):
    whole, view = _make(kind, dtype)
    assert tuple(whole.shape) == (ag.FRONT + ROWS + ag.BACK, WIDTH) and tuple(view.shape) == (ROWS, WIDTH)
    assert (ag.FRONT, ag.BACK) == (16, 64)
    # the view is the middle of the same memory
    item = whole.element_size() if kind == "torch" else whole.itemsize
    ptr = (lambda a: a.data_ptr()) if kind == "torch" else (lambda a: a.ctypes.data)
    assert ptr(view) == ptr(whole) + ag.FRONT * WIDTH * item
    b = ag.bits(whole)
    assert np.all(b == ag.sentinel(whole.dtype))
    if "float" in str(whole.dtype):
        f = whole.numpy() if kind == "torch" else whole
        assert np.isnan(f).all()  # a NaN: no float comparison finds it
        # quiet (the top mantissa bit) and with a payload below it
        mant = 23 if item == 4 else 52
        assert (ag.sentinel(whole.dtype) >> (mant - 1)) & 1 == 1
        assert ag.sentinel(whole.dtype) & ((1 << (mant - 1)) - 1) != 0
    else:
        assert ag.sentinel(whole.dtype) & 1 == 1
    ag.assert_bands_intact(whole, ag.FRONT, ROWS)
    with pytest.raises(AssertionError, match=r"never written, the first at \(row, column\) \(0, 0\)"):
        ag.assert_all_written(view)


@pytest.mark.parametrize("kind,dtype", CASES, ids=_ids)
def test_planted_write_is_reported_where_it_is(kind, dtype):
    """One element at the first and at the last position of each band."""
    total = ag.FRONT + ROWS + ag.BACK
    spots = [(0, 0, "front"), (ag.FRONT - 1, WIDTH - 1, "front"), (ag.FRONT + ROWS, 0, "back"),
             (total - 1, WIDTH - 1, "back")]
    for r, c, band in spots:
        whole, view = _make(kind, dtype)
        view[...] = 0  # the payload written, as a kernel would
        ag.assert_bands_intact(whole, ag.FRONT, ROWS)
        ag.assert_all_written(view)
        whole[r, c] = 1
        with pytest.raises(AssertionError) as ex:
            ag.assert_bands_intact(whole, ag.FRONT, ROWS, what="act")
        msg = str(ex.value)
        assert f"(row {r}, column {c})" in msg and f"{band} band" in msg and msg.startswith("act: 1 element")


@pytest.mark.parametrize("kind,dtype", [c for c in CASES if "float" in str(c[1])],
                         ids=[i for i, c in zip(_ids, CASES) if "float" in str(c[1])])
def test_another_nan_payload_is_caught(kind, dtype):
    """The check is on the bits: a band element replaced by a different NaN (what a kernel that
    computed on the band and stored the result would leave) compares unequal, though both are
    NaN and a float comparison could tell neither from the other."""
    whole, view = _make(kind, dtype)
    view[...] = 0
    r, c = ag.FRONT + ROWS + 3, 7
    whole[r, c] = float("nan")  # the default quiet NaN: payload 0
    f = whole.numpy() if kind == "torch" else whole
    assert np.isnan(f[r, c]) and np.isnan(f[r, c - 1])
    assert ag.bits(whole)[r, c] != ag.sentinel(whole.dtype)
    with pytest.raises(AssertionError, match=rf"\(row {r}, column {c}\)"):
        ag.assert_bands_intact(whole, ag.FRONT, ROWS)
    # ... and the sentinel's own bits back (through the integer view) are what "intact" means
    if kind == "torch":
        whole.view(torch.int64 if whole.element_size() == 8 else torch.int32)[r, c] = ag.sentinel(whole.dtype)
    else:
        whole.view(np.uint64 if whole.itemsize == 8 else np.uint32)[r, c] = ag.sentinel(whole.dtype)
    ag.assert_bands_intact(whole, ag.FRONT, ROWS)


@pytest.mark.parametrize("kind,dtype", CASES, ids=_ids)
def test_untouched_payload_element_fails_all_written(kind, dtype):
    for r, c in [(0, 0), (ROWS - 1, WIDTH - 1), (2, 5)]:
        whole, view = _make(kind, dtype)
        keep = ag.bits(view)[r, c]
        view[...] = 0
        if kind == "torch":
            view.view(torch.int64 if view.element_size() == 8 else torch.int32)[r, c] = int(keep)
        else:
            view.view(np.uint64 if view.itemsize == 8 else np.uint32)[r, c] = keep
        with pytest.raises(AssertionError, match=rf"1 payload element\(s\) never written.*\({r}, {c}\)"):
            ag.assert_all_written(view, what="act")


@pytest.mark.parametrize("kind", ["torch", "numpy"])
@pytest.mark.parametrize("shift", [1, 2, 3])
def test_shifted_payload(kind, shift):
    """An unaligned payload: `shift` elements into the back band. The elements it vacates in
    front are band, the ones it covers behind are payload."""
    whole, _ = _make(kind, torch.float32 if kind == "torch" else np.float32)
    view = ag.shifted(whole, ag.FRONT, ROWS, shift)
    assert tuple(view.shape) == (ROWS, WIDTH)
    ptr = (lambda a: a.data_ptr()) if kind == "torch" else (lambda a: a.ctypes.data)
    assert ptr(view) == ptr(whole) + 4 * (ag.FRONT * WIDTH + shift)
    view[...] = 0
    ag.assert_all_written(view)
    ag.assert_bands_intact(whole, ag.FRONT, ROWS, shift=shift)
    with pytest.raises(AssertionError, match=rf"\(row {ag.FRONT + ROWS}, column 0\)"):
        ag.assert_bands_intact(whole, ag.FRONT, ROWS)  # (the unshifted payload ends `shift` elements sooner)
    whole[ag.FRONT, shift - 1] = 1  # the last element in front of the shifted payload
    with pytest.raises(AssertionError, match=rf"\(row {ag.FRONT}, column {shift - 1}\).*front band"):
        ag.assert_bands_intact(whole, ag.FRONT, ROWS, shift=shift)


@pytest.mark.parametrize("kind", ["torch", "numpy"])
def test_fill_bands_and_bit_equality(kind):
    whole, view = _make(kind, torch.float32 if kind == "torch" else np.float32)
    view[...] = 2
    before = ag.bits(whole)
    ag.assert_bits_equal(whole, before)
    ag.fill_bands(whole, ag.FRONT, ROWS, 1e30)
    f = whole.numpy() if kind == "torch" else whole
    assert np.all(f[:ag.FRONT] == np.float32(1e30)) and np.all(f[ag.FRONT + ROWS:] == np.float32(1e30))
    assert np.all(f[ag.FRONT:ag.FRONT + ROWS] == 2)
    with pytest.raises(AssertionError, match=r"differ bitwise, the first at \(0, 0\)"):
        ag.assert_bits_equal(whole, before, what="obs")
    # -0.0 == 0.0 as floats, not as bits
    a, b = np.zeros((2, 2), np.float32), np.zeros((2, 2), np.float32)
    b[1, 0] = -0.0
    assert np.array_equal(a, b)
    with pytest.raises(AssertionError, match=r"\(1, 0\)"):
        ag.assert_bits_equal(a, b)


def test_status_column():
    """A [B] vector is a banded buffer one element wide."""
    whole, view = ag.banded(7, 1, torch.int32)
    flat = view.view(-1)
    assert flat.data_ptr() == view.data_ptr() and flat.numel() == 7
    flat.zero_()
    ag.assert_all_written(view)
    ag.assert_bands_intact(whole, ag.FRONT, 7)
    whole[ag.FRONT + 7, 0] = 0
    with pytest.raises(AssertionError, match=rf"\(row {ag.FRONT + 7}, column 0\)"):
        ag.assert_bands_intact(whole, ag.FRONT, 7)
