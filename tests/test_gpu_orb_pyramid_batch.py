"""gsh_pyramid_batch and gsh_orb_extract_pyramid_batch_nostdlib on the MI355X: the cases of
tests/orb_pyramid_batch_cases.py on device memory, a batch of more frames than a wave has lanes, and the chain
orb_extract_pyramid_batch_nostdlib -> match_orb_batch enqueued on a caller's stream with no host sync between the calls."""
import numpy as np
import pytest

import orb_pyramid_batch_cases as oc
from grayskull_amd import KEYPOINT_DTYPE
from guard_cases import Guarded

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("w, h, n_levels, L", oc.PYRAMID_CASES, ids=lambda v: str(v))
def test_pyramid_batch_gpu(hip, w, h, n_levels, L):
    gd = Guarded("device", seed=w + h)
    oc.check_pyramid(hip, gd, w, h, n_levels, L)
    assert gd.checked == oc.check_pyramid.checks


def test_pyramid_level_rules_gpu(hip):
    gd = Guarded("device", seed=4)
    oc.check_pyramid_level_rules(hip, gd)
    assert gd.checked == oc.check_pyramid_level_rules.checks


@pytest.mark.parametrize("case", oc.ORB_CHECKS, ids=lambda f: f.__name__[6:])
def test_orb_pyramid_batch_gpu(hip, case):
    gd = Guarded("device", seed=5)
    case(hip, gd)
    assert gd.checked == case.checks


def test_more_frames_than_a_wave_has_lanes(hip):
    """70 frames of 131 x 97, nkps 24, two levels: frames A - D in turn, the seed varied per frame, every frame against the
    oracle (k_orb_select_level takes one frame per block, k_orb_describe_level one frame per grid row)"""
    makers = (oc.frame_a, oc.frame_b, oc.frame_c, oc.frame_d)
    frames = np.stack([makers[f % 4](131, 97, 30 + f) for f in range(70)])
    gd = Guarded("device", seed=7)
    pl = oc.run_orb(hip, gd, "seventy", 108, frames, 24, 3)
    assert gd.checked == 4
    assert len({p[-1][0] for p in pl}) >= 3 and all(len(p) == 2 for p in pl)


def test_extract_then_match_unsynced_on_a_caller_stream(hip):
    """orb_extract_pyramid_batch_nostdlib of one template frame (n = 1) and of six scene windows -> match_orb_batch (the
    template's one set against every scene, counts_dev passed straight through as n1 and n2) after gsh_set_stream on a torch
    stream and under gsh_set_async(1) with nothing between the calls, compared after ONE sync with the run that
    synchronised after every call and with the oracle on the downloaded keypoints"""
    import torch
    from oracle.pyoracle import Oracle
    n, nkps, h, w, levels = 6, 120, 120, 160, 3
    base = Oracle.synth(w + 10, h + 6, 5)
    scenes = np.stack([np.ascontiguousarray(base[f:f + h, 2 * f:2 * f + w]) for f in range(n)])  # the scene, shifted
    tmpl = np.ascontiguousarray(base[None, 3:3 + h, 4:4 + w])

    def chain(sync):
        timg, simg = torch.from_numpy(tmpl).cuda(), torch.from_numpy(scenes).cuda()
        tbuf = torch.zeros(hip.orb_pyramid_batch_buffer_bytes(w, h, levels, 1), dtype=torch.uint8, device="cuda")
        sbuf = torch.zeros(hip.orb_pyramid_batch_buffer_bytes(w, h, levels, n), dtype=torch.uint8, device="cuda")
        tk = torch.zeros((1, nkps, 12), dtype=torch.int32, device="cuda")
        sk = torch.zeros((n, nkps, 12), dtype=torch.int32, device="cuda")
        tc = torch.full((1,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        sc = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        matches = torch.full((n, nkps, 3), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        counts = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        hip.orb_extract_pyramid_batch_nostdlib(timg, tbuf, tk, tc, nkps, 20, levels), sync()
        hip.orb_extract_pyramid_batch_nostdlib(simg, sbuf, sk, sc, nkps, 20, levels), sync()
        hip.match_orb_batch(tk, tc, sk, sc, matches, counts, 60.0), sync()
        return tk, tc, sk, sc, matches, counts

    synced = [a.cpu().numpy() for a in chain(torch.cuda.synchronize)]
    tk, tc, sk, sc, matches, counts = synced
    assert tc[0] > 20 and (sc > 20).all() and (sc <= nkps).all() and counts.sum() > 20
    o = Oracle("port")
    for f in range(n):
        want = o.match_orb(tk[0, :tc[0]].reshape(-1).view(KEYPOINT_DTYPE), sk[f, :sc[f]].reshape(-1).view(KEYPOINT_DTYPE), nkps, 60.0)
        want = want.view(np.uint32).reshape(-1, 3)
        assert counts[f] == len(want) and np.array_equal(matches[f, :counts[f]].view(np.uint32), want), f
        assert (matches[f, counts[f]:].view(np.uint32) == 0x5A5A5A5A).all(), f
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    try:
        hip.set_stream(st.cuda_stream)
        hip.set_async(True)
        with torch.cuda.stream(st):
            out = chain(lambda: None)
        st.synchronize()
        got = [a.cpu().numpy() for a in out]
    finally:
        hip.set_async(False)
        hip.set_stream(None)
    for a, b in zip(got, synced):
        assert np.array_equal(a, b)
