"""gsh_match_template_batch, gsh_find_best_match_batch and gsh_locate_template_batch on the MI355X: the cases of
tests/tmatch_batch_cases.py on device memory with every wave of a launch in flight at once (the emulator runs one block at a
time, so only here do the 64-bit atomic maxima of a frame really race), the default tile rule on both sides of its 512-block
limit, a launch that fills the chip, and the chain crop -> locate -> find enqueued on a caller's stream with no host sync
between the calls."""
import numpy as np
import pytest

import tmatch_batch_cases as tc
from parity_cases import Mem

pytestmark = pytest.mark.gpu
MEM = Mem("device")


@pytest.fixture(scope="module")
def oracles(oracle):
    from oracle import pyoracle
    return [oracle] + ([pyoracle.Oracle("reference")] if pyoracle.have_reference() else [])


@pytest.mark.parametrize("case", tc.ALL_CHECKS, ids=lambda f: f.__name__[6:])
def test_tmatch_batch_gpu(hip, oracles, case):
    case(hip, MEM, oracles)


@pytest.mark.parametrize("n, kernel", [(127, "split"), (128, "whole")])
def test_default_rule_on_both_sides_of_512_blocks(hip, oracle, n, kernel):
    """case 3 with no key set: frames of 144 x 96 and a 16 x 32 template have 129 x 65 results, 2 x 2 whole tiles each: 127
    frames are 508 blocks and take the split form, 128 frames are 512 and take whole tiles"""
    img = tc.frames(21, 128, 96, 144)[:n]
    assert tc.plan(144, 96, 16, 32, n) == kernel
    _, best, score = tc.run(hip, MEM, [oracle], ("limit", n), img, np.ascontiguousarray(img[n - 1, 60:92, 125:141]), "%d frames" % n)
    assert tuple(best[n - 1]) == (125, 60) and score[n - 1] == 255


def test_a_launch_that_fills_the_chip(hip, oracle):
    """32 frames of 640 x 360 and one 64 x 64 template: 25 whole tiles a frame, 800 in the launch (alone a frame would take
    100 split tiles).  The first and the last frame against the oracle, all 32 against gs_match_template + gs_find_best_match
    of the same library, frame by frame."""
    import torch
    n = 32
    img = tc.frames(22, n, 360, 640)
    tmpl = np.ascontiguousarray(img[n - 1, 200:264, 333:397])
    assert tc.plan(640, 360, 64, 64, n) == "band" and tc.plan(640, 360, 64, 64, 1) == "split"
    d_img, d_tmpl = torch.from_numpy(np.array(img)).cuda(), torch.from_numpy(tmpl).cuda()
    maps = torch.full((n, 297, 577), tc.FILL, dtype=torch.uint8, device="cuda")
    best = torch.full((2, n, 2), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    score = torch.full((2, n), tc.FILL, dtype=torch.uint8, device="cuda")
    hip.match_template_batch(maps, d_img, d_tmpl)
    hip.find_best_match_batch(maps, best[0], score[0])
    hip.locate_template_batch(d_img, d_tmpl, best[1], score[1])
    torch.cuda.synchronize()
    got, b, s = maps.cpu().numpy(), best.cpu().numpy(), score.cpu().numpy()
    assert np.array_equal(b[0], b[1]) and np.array_equal(s[0], s[1])
    for f in (0, n - 1):
        want = oracle.match_template(img[f], tmpl)
        assert np.array_equal(got[f], want), "frame %d: %d bytes differ" % (f, np.count_nonzero(got[f] != want))
        x, y = oracle.find_best_match(want)
        assert (x, y) == tuple(b[1, f]) and want[y, x] == s[1, f]
    assert tuple(b[1, n - 1]) == (333, 200) and s[1, n - 1] == 255
    one = torch.empty((297, 577), dtype=torch.uint8, device="cuda")
    for f in range(n):
        hip.match_template(d_img[f], d_tmpl, one)
        assert torch.equal(one, maps[f]), f
        assert hip.find_best_match(one) == tuple(b[1, f]), f
    assert torch.equal(d_img.cpu(), torch.from_numpy(np.array(img))) and torch.equal(d_tmpl.cpu(), torch.from_numpy(tmpl))


def test_crop_locate_find_unsynced_on_a_caller_stream(hip, oracle):
    """crop_batch (cut a patch out of frame 1) -> locate_template_batch -> match_template_batch -> find_best_match_batch after
    gsh_set_stream on a torch stream and under gsh_set_async(1) with nothing between the calls, compared after ONE sync with
    the run that synchronised after every call and with the oracle"""
    import torch
    n, roi = 6, (301, 77, 48, 40)
    img = tc.frames(23, n, 240, 500)
    tmpl = oracle.crop(img[1], *roi)
    want_maps = np.stack([oracle.match_template(f, tmpl) for f in img])
    want_best = np.array([oracle.find_best_match(m) for m in want_maps])
    assert tuple(want_best[1]) == roi[:2] and tc.plan(500, 240, 48, 40, n) == "split"  # 16 whole tiles a frame, 96 in the launch

    def chain(s, sync):
        t = torch.full((1, roi[3], roi[2]), tc.FILL, dtype=torch.uint8, device="cuda")
        maps = torch.full((n,) + want_maps.shape[1:], tc.FILL, dtype=torch.uint8, device="cuda")
        best = torch.full((2, n, 2), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        score = torch.full((2, n), tc.FILL, dtype=torch.uint8, device="cuda")
        hip.crop_batch(t, s[1:2], *roi), sync()
        hip.locate_template_batch(s, t[0], best[0], score[0]), sync()
        hip.match_template_batch(maps, s, t[0]), sync()
        hip.find_best_match_batch(maps, best[1], score[1]), sync()
        return maps, best, score

    synced = [a.cpu().numpy() for a in chain(torch.from_numpy(np.array(img)).cuda(), torch.cuda.synchronize)]
    assert np.array_equal(synced[0], want_maps)
    assert np.array_equal(synced[1][0], want_best) and np.array_equal(synced[1][1], want_best)
    assert np.array_equal(synced[2][0], synced[2][1]) and synced[2][0][1] == 255
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    try:
        hip.set_stream(st.cuda_stream)
        hip.set_async(True)
        with torch.cuda.stream(st):
            out = chain(torch.from_numpy(np.array(img)).cuda(non_blocking=False), lambda: None)
        st.synchronize()
        got = [a.cpu().numpy() for a in out]
    finally:
        hip.set_async(False)
        hip.set_stream(None)
    for a, b in zip(got, synced):
        assert np.array_equal(a, b)
