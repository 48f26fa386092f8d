"""gsh_crop_batch, gsh_resize_batch, gsh_resize_nn_batch and gsh_crop_resize_batch on the MI355X: the cases of
tests/geom_batch_cases.py on device memory with thousands of waves in flight where the emulator runs one block at a time,
one full-size check per kind of scale against the oracle, and the chain resize -> crop -> resize enqueued on a caller's
stream with no host sync between the calls."""
import numpy as np
import pytest

import geom_batch_cases as gc
from parity_cases import Mem

pytestmark = pytest.mark.gpu
MEM = Mem("device")


@pytest.fixture(scope="module")
def oracles(oracle):
    from oracle import pyoracle
    return [oracle] + ([pyoracle.Oracle("reference")] if pyoracle.have_reference() else [])


@pytest.mark.parametrize("case", gc.ALL_CHECKS, ids=lambda f: f.__name__[6:])
def test_geom_batch_gpu(hip, oracles, case):
    case(hip, MEM, oracles)


@pytest.mark.parametrize("sw,sh,dw,dh,branch", [
    (1920, 1080, 1280, 720, (16, 388 * 27)),   # downscale 3:2, bands of 16 rows staged
    (3838, 2160, 1279, 719, (16, 0)),          # ragged downscale 3:1, nine source pixels per result pixel: gathered
    (1280, 720, 1920, 1080, (16, 176 * 14)),   # upscale 2:3: every source row is tapped by more than one output row
], ids=["1920x1080_to_1280x720", "3838x2160_to_1279x719", "1280x720_to_1920x1080"])
def test_full_frames_against_the_oracle(hip, oracle, sw, sh, dw, dh, branch):
    import torch
    assert gc.plan(dw, dh, sw, sh) == branch
    src = gc.frames(31, 3, sh, sw)
    s = torch.from_numpy(np.array(src)).cuda()
    d = torch.full((3, dh, dw), gc.FILL, dtype=torch.uint8, device="cuda")
    hip.resize_batch(d, s)
    torch.cuda.synchronize()
    got = d.cpu().numpy()
    for f in range(3):
        want = oracle.resize(src[f], dw, dh)
        assert np.array_equal(got[f], want), "frame %d: %d bytes differ" % (f, np.count_nonzero(got[f] != want))
    assert torch.equal(s.cpu(), torch.from_numpy(np.array(src)))


def test_resize_crop_resize_unsynced_on_a_caller_stream(hip, oracle):
    """resize_batch -> crop_batch -> resize_batch after gsh_set_stream on a torch stream and under gsh_set_async(1) with
    nothing between the calls, compared after ONE sync with the run that synchronised after every call and with the oracle"""
    import torch
    src = gc.frames(32, 3, 360, 1041)
    roi = (33, 21, 500, 131)
    want = np.stack([oracle.resize(oracle.crop(oracle.resize(f, 640, 200), *roi), 333, 77) for f in src])

    def chain(s, sync):
        a = torch.full((3, 200, 640), gc.FILL, dtype=torch.uint8, device="cuda")
        b = torch.full((3, roi[3], roi[2]), gc.FILL, dtype=torch.uint8, device="cuda")
        c = torch.full((3, 77, 333), gc.FILL, dtype=torch.uint8, device="cuda")
        hip.resize_batch(a, s), sync()
        hip.crop_batch(b, a, *roi), sync()
        hip.resize_batch(c, b), sync()
        return c

    synced = chain(torch.from_numpy(np.array(src)).cuda(), torch.cuda.synchronize).cpu().numpy()
    assert np.array_equal(synced, want)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    try:
        hip.set_stream(st.cuda_stream)
        hip.set_async(True)
        with torch.cuda.stream(st):
            out = chain(torch.from_numpy(np.array(src)).cuda(non_blocking=False), lambda: None)
        st.synchronize()
        got = out.cpu().numpy()
    finally:
        hip.set_async(False)
        hip.set_stream(None)
    assert np.array_equal(got, synced)
