"""Guard bands around the buffers a test hands to the C ABI.

A kernel that writes a row it was not given corrupts a neighbouring tensor of the caller's and
nothing faults. To see such a write, a test passes the middle of a larger allocation it owns:
`front` rows, then the payload, then `back` rows, every element holding a sentinel bit pattern
(a quiet NaN with a payload for float32 / float64, a fixed odd word for the 32-bit integers).
After the call the bands must hold the sentinel still, bit for bit, and the payload must not.

Every comparison is made on an integer view: the float sentinel is a NaN, which a float
comparison can neither find (NaN != NaN) nor tell from another NaN.

torch tensors (CPU or GPU) and numpy arrays are served by the same functions; banded() makes
the former, banded_np() the latter (host buffers: go2pi_run, go2pi_controller_step).
"""
from __future__ import annotations

import numpy as np

FRONT = 16  # rows in front of the payload: one tile
BACK = 64   # rows behind it: four 16-row tiles, so a whole tile of overshoot stays inside the allocation

SENTINEL = {"float32": 0x7FC5A5A5, "float64": 0x7FF8A5A5A5A5A5A5, "int32": 0x5A5A5A5B, "uint32": 0x5A5A5A5B}
_UINT = {4: np.uint32, 8: np.uint64}


def _name(dtype) -> str:
    name = str(dtype).replace("torch.", "")
    if name not in SENTINEL:
        raise TypeError(f"no sentinel for dtype {dtype}")
    return name


def sentinel(dtype) -> int:
    return SENTINEL[_name(dtype)]


def bits(a) -> np.ndarray:
    """The elements of a torch tensor or numpy array as unsigned integers of their width
    (a host copy, same shape)."""
    if not isinstance(a, np.ndarray):
        a = a.detach().cpu().contiguous().numpy()
    a = np.ascontiguousarray(a)
    return a.view(_UINT[a.dtype.itemsize]).copy()


def banded(shape_rows, width, dtype, front=FRONT, back=BACK, device="cpu"):
    """(whole, view): `whole` is one contiguous torch tensor [front + rows + back, width] filled
    with the sentinel of `dtype` (torch.float32 / float64 / int32), `view` its middle rows."""
    import torch
    whole = torch.empty((front + shape_rows + back, width), dtype=dtype, device=device)
    whole.view(torch.int64 if whole.element_size() == 8 else torch.int32).fill_(sentinel(dtype))
    return whole, whole[front:front + shape_rows]


def banded_np(shape_rows, width, dtype, front=FRONT, back=BACK):
    """banded() for host buffers: numpy arrays (np.float32 / float64 / int32 / uint32)."""
    dt = np.dtype(dtype)
    whole = np.empty((front + shape_rows + back, width), dt)
    whole.view(_UINT[dt.itemsize])[...] = sentinel(dt)
    return whole, whole[front:front + shape_rows]


def shifted(whole, front, rows, shift):
    """The payload moved `shift` elements towards the back band (an unaligned pointer into the
    same allocation): a contiguous [rows, width] view that starts shift elements behind row `front`."""
    width = whole.shape[1]
    lo = front * width + shift
    return whole.reshape(-1)[lo:lo + rows * width].reshape(rows, width)


def fill_bands(whole, front, rows, value):
    """Overwrite both bands with `value` (the payload keeps its contents)."""
    whole[:front] = value
    whole[front + rows:] = value


def assert_bands_intact(whole, front, rows, shift=0, what="buffer"):
    """Every element outside the payload (rows [front, front + rows), moved `shift` elements
    back) still holds the sentinel, compared bitwise. Reports the first changed (row, column)
    of `whole`."""
    width = whole.shape[1]
    flat = bits(whole).reshape(-1)
    lo = front * width + shift
    hi = lo + rows * width
    outside = np.ones(flat.size, bool)
    outside[lo:hi] = False
    bad = np.flatnonzero(outside & (flat != flat.dtype.type(sentinel(whole.dtype))))
    if bad.size:
        r, c = divmod(int(bad[0]), width)
        where = "front band" if bad[0] < lo else "back band"
        raise AssertionError(f"{what}: {bad.size} element(s) outside the payload changed, the first at "
                             f"(row {r}, column {c}) of the allocation ({where}; payload rows "
                             f"{front}..{front + rows - 1}): bits {int(flat[bad[0]]):#x}")


def assert_all_written(view, what="buffer"):
    """No element of the payload still holds the sentinel."""
    b = bits(view)
    left = np.argwhere(b == b.dtype.type(sentinel(view.dtype)))
    if left.size:
        raise AssertionError(f"{what}: {len(left)} payload element(s) never written, the first at "
                             f"(row, column) {tuple(int(i) for i in left[0])}")


def assert_bits_equal(got, want, what="buffer"):
    """Two buffers (or a buffer and bits() taken earlier) hold the same bits everywhere."""
    g = bits(got)
    w = want if isinstance(want, np.ndarray) and want.dtype.kind == "u" else bits(want)
    assert g.shape == w.shape, f"{what}: shape {g.shape} != {w.shape}"
    bad = np.argwhere(g != w)
    if bad.size:
        i = tuple(int(k) for k in bad[0])
        raise AssertionError(f"{what}: {len(bad)} element(s) differ bitwise, the first at {i}: "
                             f"{int(g[i]):#x} != {int(w[i]):#x}")
