"""LBP cascades with large, shared and odd-shaped stages on an MI355X: the cases of tests/lbp_cascade_cases.py against the
oracle, bit for bit -- every named cascade under every kernel choice (key 14 = 0..4, key 4 = 1, key 15 = 241 and 7), every
parameter set, three frames, the integral image in host and in device memory; the batch entry with and without the counting
kernels; single windows.  tests/test_lbp_cascades.py runs a part of the same on the emulator and holds the checks of the
inputs themselves."""
import pytest

import lbp_cascade_cases as lc
from parity_cases import Mem

pytestmark = pytest.mark.gpu
MEMS = [Mem("device"), Mem("host")]


@pytest.mark.parametrize("kv", lc.KEYS, ids=lc.KEY_IDS)
@pytest.mark.parametrize("name", lc.NAMES)
def test_detect(hip, oracle, name, kv):
    lc.check_detect(hip, oracle, MEMS, name, kv[0], kv[1])


@pytest.mark.parametrize("name", lc.NAMES)
def test_batch_and_counting_kernels(hip, oracle, name):
    lc.check_batch(hip, oracle, MEMS[0], name)


@pytest.mark.parametrize("name", lc.NAMES)
def test_single_windows(hip, oracle, name):
    lc.check_windows(hip, oracle, MEMS, name)
