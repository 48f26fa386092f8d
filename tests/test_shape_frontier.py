"""CPU leg of the shape frontier (tests/shape_frontier_cases.py; tests/test_gpu_shape_frontier.py runs it on an MI355X):
the heights of the tall cases against their grid.y formulas, the band cap of gs_resize's plan at its two heights, the
whole-array perspective model against the pixel-by-pixel one, and gs_erode / gs_sobel at 16 x 262200 on the emulator.

The emulator enforces no grid limits: it pins the kernels' row arithmetic beyond row 4 x 65535, not the launch."""
import numpy as np
import pytest

import geom_batch_cases as gc
import shape_frontier_cases as sfc
from parity_cases import Mem


@pytest.mark.parametrize("case", sfc.TALL, ids=[c[0] for c in sfc.TALL])
def test_heights_straddle_the_grid_limit(case):
    """`past` makes the case's grid.y exceed 65535, `last` is the largest height that does not"""
    sfc.check_frontier(case)


def test_resize_plan_at_the_band_cap():
    """8 x 1000 -> 8 x 1048560: 65535 bands of 16 rows, not capped; -> 8 x 1048700: 65544 bands of 16 rows would pass
    grid.y's 65535, so bands of ceil(1048700 / 65535) = 17 -> 20 rows, 52435 of them, with the LDS sized for 16 rows"""
    assert gc.plan(8, 1048560, 8, 1000) == (16, 32) and sfc.ceil_div(1048560, 16) == 65535
    assert gc.plan(8, 1048700, 8, 1000) == (20, 32) and sfc.ceil_div(1048700, 16) == 65544 and sfc.ceil_div(1048700, 20) == 52435
    for name, op, w, grid_y, past, last in sfc.TALL_RESIZE:
        for h in (past, last):
            assert grid_y(h) == sfc.ceil_div(h, gc.plan(w, h, 8, 1000)[0]) <= gc.MAX_BANDS


def test_perspective_model_is_the_spec():
    from blob_cases import spec_perspective
    src = sfc.frame(3, 64, 50)
    for (dw, dh), c in (((16, 41), sfc.PERSPECTIVE_CORNERS), ((5, 9), ((60, 70), (0, 0), (49, 0), (2, 63))), ((1, 3), sfc.PERSPECTIVE_CORNERS)):
        assert np.array_equal(sfc.spec_perspective(dw, dh, src, c), spec_perspective(dw, dh, src, c)), (dw, dh)


@pytest.mark.parametrize("name", ["erode", "sobel"])
def test_row_arithmetic_past_row_262140_emulated(emu, reference, name):
    case = [c for c in sfc.TALL_GRID2D if c[0] == name][0]
    sfc.run_tall(emu, [Mem("host")], reference, case, "past")
