"""Host-only parts of the grid index (csrc/grid_nn.hip) through the built library: the grid-dimension function and the workspace
sizes.  No GPU is touched: both are pure functions of their arguments."""
import ctypes

import pytest

from pccx import _lib

MAX_CELLS = 1 << 21          # what include/pccx.h promises for pccx_grid_dims
MAX_AXIS = 1024


def dims(N, ex, ey, ez):
    out = (ctypes.c_int32 * 3)()
    cell = ctypes.c_float()
    _lib.call("pccx_grid_dims", int(N), float(ex), float(ey), float(ez), ctypes.addressof(out), ctypes.addressof(cell))
    return tuple(out), cell.value


def test_zero_extent_axes_get_one_cell():
    (gx, gy, gz), cell = dims(100000, 8.0, 5.0, 0.0)
    assert gz == 1 and gx > 1 and gy > 1 and cell > 0
    (gx, gy, gz), _ = dims(100000, 0.0, 5.0, 0.0)
    assert (gx, gz) == (1, 1) and gy > 1
    assert dims(100000, 0.0, 0.0, 0.0)[0] == (1, 1, 1)                     # all points identical: one cell in all
    assert dims(1, 3.0, 2.0, 1.0)[0] == (1, 1, 1)                          # one point: nothing to separate
    for bad in (float("nan"), float("inf"), -1.0):                          # no extent to speak of: treated as zero, never a crash
        g, cell = dims(4096, bad, 1.0, 1.0)
        assert g[0] == 1 and g[1] >= 1 and g[2] >= 1 and cell > 0


def test_cells_follow_the_extents_and_are_cubic():
    (gx, gy, gz), cell = dims(1_000_000, 10.0, 8.0, 3.0)                   # a room: flat box
    assert gx >= gy >= gz > 1
    assert gx == round(10.0 / cell)                                         # the longest axis is cut exactly
    assert abs(gy - 8.0 / cell) <= 1 and abs(gz - 3.0 / cell) <= 1         # the others by the same cell side


@pytest.mark.parametrize("ext", [(1.0, 1.0, 1.0), (10.0, 8.0, 3.0), (1.0, 1.0, 0.0), (5.0, 0.0, 0.0), (1e-3, 1.0, 1e3)])
def test_cell_cap_holds(ext):
    for N in (10 ** 7, 2 ** 31 - 1):
        (gx, gy, gz), _ = dims(N, *ext)
        assert gx * gy * gz <= MAX_CELLS and max(gx, gy, gz) <= MAX_AXIS


@pytest.mark.parametrize("ext", [(1.0, 1.0, 1.0), (10.0, 8.0, 3.0), (7.3, 2.1, 0.0), (0.013, 1.7, 0.4)])
def test_dims_are_monotone_in_n(ext):
    prev = (1, 1, 1)
    for N in (1, 2, 3, 7, 64, 65, 1000, 8192, 40000, 65536, 10 ** 6, 4 * 10 ** 6, 10 ** 7, 10 ** 8):
        g = dims(N, *ext)[0]
        assert all(a >= b for a, b in zip(g, prev)), (N, g, prev)
        assert g[0] * g[1] * g[2] <= max(N, 1)                             # never more cells than points
        prev = g


def test_workspace_sizes():
    lib = _lib.load()
    for fn in (lib.pccx_grid_index_workspace_bytes, lib.pccx_grid_query_workspace_bytes):
        assert fn(0, 8192) == 0 and fn(0, 0) == 0 and fn(4, 0) == 0
        for N in (1, 65, 8192, 10 ** 6):
            sizes = [fn(B, N) for B in (1, 2, 3, 64, 256)]
            assert sizes[0] > 0 and sizes == sorted(sizes), (N, sizes)
        for B in (1, 3, 256):
            sizes = [fn(B, N) for N in (1, 2, 63, 64, 65, 1000, 8192, 40000, 10 ** 6)]
            assert sizes == sorted(sizes), (B, sizes)
    # the index holds at least the points in cell order (12 + 4 bytes each) and the sort's own workspace
    assert lib.pccx_grid_index_workspace_bytes(1, 10 ** 6) >= 16 * 10 ** 6 + lib.pccx_sort_keys_workspace_bytes(10 ** 6)


def test_bad_arguments_are_errors():
    with pytest.raises(_lib.PccxError):
        _lib.call("pccx_grid_dims", 0, 1.0, 1.0, 1.0, ctypes.addressof((ctypes.c_int32 * 3)()), ctypes.addressof(ctypes.c_float()))
    with pytest.raises(_lib.PccxError):
        _lib.call("pccx_grid_dims", 10, 1.0, 1.0, 1.0, None, None)
