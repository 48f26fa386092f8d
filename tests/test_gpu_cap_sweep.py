"""The cap sweeps of tests/cap_sweep_cases.py on the MI355X, in full: every cap from 1 to T + 2 wherever one uncapped
reference run gives the expected prefix, caps_for() -- every seam, the marks, 200 random caps -- for the LBP scans and the
4200-query matching, every nkps for ORB and every nblobs for the blobs.  What only the GPU has: the emit kernels' real wave
scheduling, the LBP early exit racing real counters, the blob kernels' atomics, the device-side level counts."""
import pytest

import blob_cases as bc
import cap_sweep_cases as cs
from guard_cases import Guarded
from parity_cases import Mem

pytestmark = pytest.mark.gpu

HOST, DEVICE = Mem("host"), Mem("device")
MEMS = {"host": HOST, "device": DEVICE}
MATCH_SMALL = (150, 300, (150, 97, 64))
MATCH_CHUNKS = ((4200, 64, (4200, 4050)), (4200, 1024, (4200, 2049)))


# ---- gs_fast, gsh_fast_batch -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["host", "device"])
@pytest.mark.parametrize("key19", [0, 1])
@pytest.mark.parametrize("name", cs.FAST_SMALL)
def test_fast_every_cap_gpu(hip, oracle, name, key19, kind):
    cs.check_fast(hip, oracle, MEMS[kind], name, key19)


@pytest.mark.parametrize("name", sorted(cs.FAST_TALL))
def test_fast_every_cap_through_chunk_scan_gpu(hip, oracle, name):
    """more than 1024 chunks per frame: k_chunk_scan's second 1024-wide pass carries a non-zero sum into a chunk that emits"""
    cs.check_fast(hip, oracle, DEVICE, name, cs.FAST_TALL[name][2])


@pytest.mark.parametrize("key19", [0, 1])
def test_fast_batch_every_cap_gpu(hip, oracle, key19):
    cs.check_fast_batch(hip, oracle, DEVICE, key19)


# ---- gs_lbp_detect, gsh_lbp_detect_batch ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("key14", [0, 1])
@pytest.mark.parametrize("name", cs.LBP_NAMES)
def test_lbp_caps_gpu(hip, oracle, name, key14):
    cs.check_lbp(hip, oracle, (HOST, DEVICE), name, key14)


@pytest.mark.parametrize("name", cs.LBP_NAMES)
def test_lbp_batch_caps_gpu(hip, oracle, name):
    cs.check_lbp_batch(hip, oracle, DEVICE, name)


# ---- gs_match_orb, gsh_match_orb_dev, gsh_match_orb_batch ------------------------------------------------------------------------
def test_match_every_cap_three_words_gpu(hip, oracle):
    cs.check_match_dropin(hip, oracle, *MATCH_SMALL)
    cs.check_match_dev(hip, oracle, DEVICE, *MATCH_SMALL)
    cs.check_match_batch(hip, oracle, DEVICE, *MATCH_SMALL)


@pytest.mark.parametrize("sizes", MATCH_CHUNKS, ids=lambda s: "%dx%d" % s[:2])
def test_match_caps_three_chunks_gpu(hip, oracle, sizes):
    cs.check_match_dropin(hip, oracle, *sizes)
    cs.check_match_batch(hip, oracle, DEVICE, *sizes)


# ---- nkps of ORB ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["host", "device"])
@pytest.mark.parametrize("w, h", cs.ORB_SHAPES)
def test_orb_every_nkps_gpu(hip, oracle, w, h, kind):
    cs.check_orb_dropin(hip, oracle, MEMS[kind], w, h)


@pytest.mark.parametrize("w, h", cs.ORB_SHAPES)
def test_orb_batch_every_nkps_gpu(hip, oracle, w, h):
    cs.check_orb_batch(hip, oracle, DEVICE, w, h)


@pytest.mark.parametrize("w, h", cs.ORB_SHAPES)
def test_orb_batch_nostdlib_every_nkps_gpu(hip, w, h):
    cs.check_orb_batch_nostdlib(hip, w, h)


@pytest.mark.parametrize("flavour", ["nostdlib", "libm"])
@pytest.mark.parametrize("w, h, levels, sweep", cs.PYRAMID_SWEEPS, ids=lambda v: str(v) if isinstance(v, int) else "nkps%d" % len(v))
def test_pyramid_every_nkps_gpu(hip, w, h, levels, sweep, flavour):
    gd = Guarded("device", seed=8)
    cs.check_pyramid(hip, gd, flavour, w, h, levels, sweep)
    assert gd.checked == 4 * len(sweep)


# ---- gs_blobs, gsh_blobs_batch -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["host", "device"])
@pytest.mark.parametrize("index", range(len(bc.emu_frames())), ids=[name.replace(" ", "_") for name, _ in bc.emu_frames()])
def test_blobs_every_nblobs_gpu(hip, index, kind):
    name, img = cs.blob_frames()[index]
    cs.check_blobs(hip, MEMS[kind], name, img)


@pytest.mark.parametrize("shape", [(70, 23), (64, 64)], ids=str)
def test_blobs_batch_every_nblobs_gpu(hip, shape):
    cs.check_blobs_batch(hip, DEVICE, shape)
