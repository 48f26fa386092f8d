"""gsh_orb_extract_pyramid_batch and gsh_orb_pyramid_buffer_fill_batch on the MI355X: the cases of
tests/orb_pyramid_libm_cases.py on device memory, a batch whose host half runs on the thread pool (more than 4096 kept
keypoints, more frames than a wave has lanes), and the chain extract (template) -> extract (scenes) -> match_orb_batch
enqueued on a caller's stream with no host sync between the calls."""
import numpy as np
import pytest

import orb_pyramid_batch_cases as oc
import orb_pyramid_libm_cases as lc
from grayskull_amd import KEYPOINT_DTYPE
from guard_cases import Guarded

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", lc.ORB_CHECKS, ids=lambda f: f.__name__[6:])
def test_orb_pyramid_libm_batch_gpu(hip, case):
    gd = Guarded("device", seed=5)
    case(hip, gd)
    assert gd.checked == case.checks


@pytest.mark.parametrize("w, h, n_levels, L, n", lc.FILL_CASES, ids=lambda v: str(v))
def test_buffer_fill_gpu(hip, w, h, n_levels, L, n):
    gd = Guarded("device", seed=w + n)
    lc.check_fill(hip, gd, w, h, n_levels, L, n)
    assert gd.checked == lc.check_fill.checks


def test_buffer_fill_writes_nothing_gpu(hip):
    gd = Guarded("device", seed=8)
    lc.check_fill_writes_nothing(hip, gd)
    assert gd.checked == lc.check_fill_writes_nothing.checks


def test_host_half_on_the_thread_pool(hip):
    """72 frames of 203 x 171, frames A, C, D in turn with seeds 30 + f, nkps 90, three levels: some 4900 kept keypoints (4941
    over this test's random score-map frames), above the 4096 from which the host trig is dealt over the pool's threads;
    every frame against the oracle"""
    makers = (oc.frame_a, oc.frame_c, oc.frame_d)
    frames = np.stack([makers[f % 3](203, 171, 30 + f) for f in range(72)])
    gd = Guarded("device", seed=7)
    pl = lc.run_orb(hip, gd, "libm seventy-two", 108, frames, 90, 3)
    assert gd.checked == 4
    assert sum(lc.totals(pl)) > 4096 and len({p[-1][0] for p in pl}) >= 3


def test_times_of_a_profiled_call(hip):
    """under gsh_profile(1) the call records where its time went (gsh_orb_pyramid_batch_times: device before, copy down, host
    trig, copy up, device after) and computes the same bytes"""
    gd = Guarded("device", seed=9)
    hip.profile(True)
    try:
        lc.check_quotas_differ_in_one_batch(hip, gd)
        ms = hip.orb_pyramid_batch_times()
    finally:
        hip.profile(False)
    assert gd.checked == 4 and len(ms) == 5
    assert all(0 < t < 1000 for t in ms), ms


def test_extract_then_match_unsynced_on_a_caller_stream(hip):
    """orb_extract_pyramid_batch of one template frame (n = 1) and of six scene windows -> match_orb_batch (the template's one
    set against every scene, counts passed straight through as n1 and n2) after gsh_set_stream on a torch stream and under
    gsh_set_async(1) with nothing between the calls, compared after ONE sync with the run that synchronised after every call;
    the keypoints are the libm oracle's and the matches the oracle's on them"""
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
        hip.orb_extract_pyramid_batch(timg, tbuf, tk, tc, nkps, 20, levels), sync()
        hip.orb_extract_pyramid_batch(simg, sbuf, sk, sc, nkps, 20, levels), sync()
        hip.match_orb_batch(tk, tc, sk, sc, matches, counts, 60.0), sync()
        return tk, tc, sk, sc, matches, counts

    synced = [a.cpu().numpy() for a in chain(torch.cuda.synchronize)]
    tk, tc, sk, sc, matches, counts = synced
    assert tc[0] > 20 and (sc > 20).all() and (sc <= nkps).all() and counts.sum() > 20
    o = Oracle("port")
    for img, k, c in [(tmpl[0], tk[0], tc[0])] + [(scenes[f], sk[f], sc[f]) for f in range(n)]:
        want = o.orb_extract_pyramid(img, nkps, 20, levels)[0]
        assert c == len(want) and k[:c].reshape(-1).view(KEYPOINT_DTYPE).tobytes() == want.tobytes()
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
