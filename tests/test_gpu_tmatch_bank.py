"""gsh_match_templates_batch and gsh_locate_templates_batch on the MI355X: the cases of tests/tmatch_bank_cases.py on device
memory with every wave of a launch in flight at once (the emulator runs one block at a time, so only here do the 64-bit
atomic maxima of a (frame, template) word really race), a launch that fills the chip, and the chain crop_resize -> locate
enqueued on a caller's stream with no host sync between the calls."""
import numpy as np
import pytest

import tmatch_bank_cases as tb
from parity_cases import Mem

pytestmark = pytest.mark.gpu
MEM = Mem("device")


@pytest.fixture(scope="module")
def oracles(oracle):
    from oracle import pyoracle
    return [oracle] + ([pyoracle.Oracle("reference")] if pyoracle.have_reference() else [])


@pytest.mark.parametrize("key27", tb.BOTH, ids=("bank", "loop"))
@pytest.mark.parametrize("case", tb.ALL_CHECKS, ids=lambda f: f.__name__[6:])
def test_tmatch_bank_gpu(hip, oracles, case, key27):
    case(hip, MEM, oracles, key27)


def test_default_rule_gpu(hip, oracles):
    tb.check_default_rule(hip, MEM, oracles)


def test_a_launch_that_fills_the_chip(hip, oracle):
    """9: four frames of 320 x 180 against 40 templates of 24 x 24 cut from the frames (template t from frame t % 4): result
    297 x 157, 5 x 20 blocks a frame and one group of 64 templates, 400 blocks of four waves in the launch, each sending up to
    40 keys.  Frames 0 and 3 against the oracle for all 40 templates; all maps against the per-template loop of the same
    library; locate equal to find-on-maps."""
    import torch
    n, m, t = 4, 40, 24
    img = tb.frames(51, n, 180, 320)
    rng = np.random.default_rng(52)
    at = list(zip(rng.integers(0, 297, m), rng.integers(0, 157, m)))
    bank = np.stack([img[k % n, y:y + t, x:x + t] for k, (x, y) in enumerate(at)])
    assert tb.takes(t, t)
    d_img, d_bank = torch.from_numpy(np.array(img)).cuda(), torch.from_numpy(bank).cuda()
    maps = torch.full((n, m, 157, 297), tb.FILL, dtype=torch.uint8, device="cuda")
    loop = torch.full((m, n, 157, 297), tb.FILL, dtype=torch.uint8, device="cuda")
    best = torch.full((2, n, m, 2), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    score = torch.full((2, n, m), tb.FILL, dtype=torch.uint8, device="cuda")
    winner = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    with tb.tuned(hip, key27=2):
        hip.match_templates_batch(maps, d_img, d_bank)
        hip.locate_templates_batch(d_img, d_bank, best[0], score[0], winner)
    for k in range(m):
        hip.match_template_batch(loop[k], d_img, d_bank[k])
    hip.find_best_match_batch(maps.view(n * m, 157, 297), best[1].view(n * m, 2), score[1].view(n * m))
    torch.cuda.synchronize()
    assert torch.equal(maps, loop.permute(1, 0, 2, 3))
    assert torch.equal(best[0], best[1]) and torch.equal(score[0], score[1])
    got, b, s, w = maps.cpu().numpy(), best[0].cpu().numpy(), score[0].cpu().numpy(), winner.cpu().numpy()
    for f in (0, 3):
        for k in range(m):
            want = oracle.match_template(img[f], bank[k])
            assert np.array_equal(got[f, k], want), "map (%d, %d): %d bytes differ" % (f, k, np.count_nonzero(got[f, k] != want))
            x, y = oracle.find_best_match(want)
            assert (x, y) == tuple(b[f, k]) and want[y, x] == s[f, k]
    for k, (x, y) in enumerate(at):
        assert tuple(b[k % n, k]) == (x, y) and s[k % n, k] == 255
    assert np.array_equal(w, np.argmax(s, axis=1)) and list(w) == [0, 1, 2, 3]
    assert torch.equal(d_img.cpu(), torch.from_numpy(np.array(img))) and torch.equal(d_bank.cpu(), torch.from_numpy(bank))


def test_crop_resize_locate_unsynced_on_a_caller_stream(hip, oracle):
    """10: crop_resize_batch cuts six 16 x 16 patches at device-side rectangles out of frame 0 -- the bank is born on the device
    -- and locate_templates_batch runs over all frames, after gsh_set_stream on a torch stream and under gsh_set_async(1) with
    nothing between the calls; compared after ONE sync with the run that synchronised after every call and with the oracle"""
    import torch
    n, m = 4, 6
    img = tb.frames(53, n, 120, 200)
    rects = np.array([(0, 0, 16, 16), (184, 104, 16, 16), (64, 8, 16, 16), (33, 77, 16, 16), (101, 50, 16, 16), (150, 3, 16, 16)], np.int32)
    bank = np.stack([oracle.resize(oracle.crop(img[0], *r), 16, 16, nearest=True) for r in rects])
    assert all(np.array_equal(bank[k], img[0, y:y + 16, x:x + 16]) for k, (x, y, _, _) in enumerate(rects))
    want_maps, want_best, want_score, want_winner = tb.expected([oracle], "chain", img, bank)
    assert [tuple(p) for p in want_best[0]] == [tuple(r[:2]) for r in rects] and (want_score[0] == 255).all()

    def chain(s, rois, frame_of, sync):
        t = torch.full((m, 16, 16), tb.FILL, dtype=torch.uint8, device="cuda")
        best = torch.full((n, m, 2), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        score = torch.full((n, m), tb.FILL, dtype=torch.uint8, device="cuda")
        winner = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        hip.crop_resize_batch(t, s, rois, frame_of, nearest=True), sync()
        hip.locate_templates_batch(s, t, best, score, winner), sync()
        return t, best, score, winner

    def inputs():
        return (torch.from_numpy(np.array(img)).cuda(), torch.from_numpy(rects).cuda(), torch.zeros(m, dtype=torch.int32, device="cuda"))

    for key27 in tb.BOTH:
        with tb.tuned(hip, key27=key27):
            synced = [a.cpu().numpy() for a in chain(*inputs(), torch.cuda.synchronize)]
            assert np.array_equal(synced[0], bank)
            assert np.array_equal(synced[1].view(np.uint32), want_best) and np.array_equal(synced[2], want_score)
            assert np.array_equal(synced[3].view(np.uint32), want_winner)
            st = torch.cuda.Stream()
            torch.cuda.synchronize()
            try:
                hip.set_stream(st.cuda_stream)
                hip.set_async(True)
                with torch.cuda.stream(st):
                    out = chain(*inputs(), lambda: None)
                st.synchronize()
                got = [a.cpu().numpy() for a in out]
            finally:
                hip.set_async(False)
                hip.set_stream(None)
            for a, b in zip(got, synced):
                assert np.array_equal(a, b)
