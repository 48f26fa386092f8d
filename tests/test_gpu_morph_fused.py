"""gsh_morph_batch on the MI355X: the cases of tests/morph_cases.py with thousands of waves in flight where the emulator
runs one at a time, 1080p and ragged 4K frames against the numpy restatement, and the close chain `dilate 9 -> erode 10`
enqueued on a caller's stream with no host sync between the calls."""
import numpy as np
import pytest

import morph_cases as mc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", mc.ALL_CHECKS, ids=lambda f: f.__name__[6:])
def test_morph_batch_gpu(hip, case):
    case(hip, mc.Device)


@pytest.fixture(scope="module")
def big_frames():
    rng = np.random.default_rng(41)
    out = {}
    for (h, w) in ((1080, 1920), (2160, 3838)):
        a = rng.integers(0, 256, (1, h, w), dtype=np.uint8)
        a[0, h // 3:h // 3 + 40, w // 4:w // 4 + 300] = 0      # plateaus wider than any window: both ops keep structure
        a[0, h // 2:h // 2 + 40, w // 2:w // 2 + 300] = 255
        out[(h, w)] = (a, {(it, dil): mc.spec(a, it, dil) for it in (4, 9) for dil in (True, False)})
    return out


@pytest.mark.parametrize("shape", [(1080, 1920), (2160, 3838)], ids=["1920x1080", "3838x2160"])
def test_full_frames_against_the_restatement(hip, big_frames, shape):
    import torch
    a, want = big_frames[shape]
    src = torch.from_numpy(a).cuda()
    dst, tmp = torch.zeros_like(src), torch.zeros_like(src)
    for (it, dil), w in want.items():
        dst.fill_(0x5a)
        hip.morph_batch(dst, src, it, dil, tmp=tmp)
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        assert np.array_equal(got, w), "%s %d: %d bytes differ" % ("dilate" if dil else "erode", it, np.count_nonzero(got != w))
    assert torch.equal(src.cpu(), torch.from_numpy(a))


def test_close_chain_unsynced_on_a_caller_stream(hip):
    """dilate 9 -> erode 10 after gsh_set_stream on a torch stream and under gsh_set_async(1), tmp supplied (nothing in
    the calls can synchronise), compared after ONE sync with the restatement and with the run that synchronised after
    every call"""
    import torch
    rng = np.random.default_rng(42)
    a = ((rng.integers(0, 1000, (3, 360, 1041)) < 4) * 255).astype(np.uint8)
    want = mc.spec(mc.spec(a, 9, True), 10, False)
    src = torch.from_numpy(a).cuda()
    mid, out, tmp = torch.zeros_like(src), torch.zeros_like(src), torch.zeros_like(src)
    hip.morph_batch(mid, src, 9, True, tmp=tmp), torch.cuda.synchronize()
    hip.morph_batch(out, mid, 10, False, tmp=tmp), torch.cuda.synchronize()
    synced = out.cpu().numpy()
    assert np.array_equal(synced, want) and want.any() and not want.all()
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    try:
        hip.set_stream(st.cuda_stream)
        hip.set_async(True)
        with torch.cuda.stream(st):
            src2 = torch.from_numpy(a).cuda(non_blocking=False)
            mid2, out2, tmp2 = torch.zeros_like(src2), torch.zeros_like(src2), torch.zeros_like(src2)
            hip.morph_batch(mid2, src2, 9, True, tmp=tmp2)
            hip.morph_batch(out2, mid2, 10, False, tmp=tmp2)
        st.synchronize()
        got = out2.cpu().numpy()
    finally:
        hip.set_async(False)
        hip.set_stream(None)
    assert np.array_equal(got, synced)
