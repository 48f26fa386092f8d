"""gsh_match_orb_batch on the MI355X: the cases of tests/match_batch_cases.py on device memory (the 16 waves of
a block stage their tiles and merge their states side by side only here), a launch that fills
the chip against gsh_match_orb_dev of the same library, and the chain orb_extract_batch_nostdlib -> match_orb_batch
enqueued on a caller's stream with no host sync between the calls."""
import numpy as np
import pytest

import match_batch_cases as mc
from grayskull_amd import KEYPOINT_DTYPE
from parity_cases import Mem

pytestmark = pytest.mark.gpu
MEM = Mem("device")


@pytest.fixture(scope="module")
def oracles(oracle):
    from oracle import pyoracle
    return [oracle] + ([pyoracle.Oracle("reference")] if pyoracle.have_reference() else [])


@pytest.mark.parametrize("case", mc.ALL_CHECKS, ids=lambda f: f.__name__[6:])
def test_match_batch_gpu(hip, oracles, case):
    case(hip, MEM, oracles)


def test_a_launch_that_fills_the_chip(hip, oracle):
    """64 pairs of 500 x 500: 8 blocks of 16 waves a pair, 512 blocks in the launch.  Every pair against gsh_match_orb_dev of
    the same library, pairs 0 and 63 against the oracle."""
    import torch
    n, nk = 64, 500
    sets = [mc.pair(nk, nk, salt=100 + p) for p in range(n)]
    k1 = torch.from_numpy(np.stack([q for q, _ in sets]).view(np.int32)).cuda()
    k2 = torch.from_numpy(np.stack([t for _, t in sets]).view(np.int32)).cuda()
    cnt = torch.full((n,), nk, dtype=torch.int32, device="cuda")
    matches = torch.full((n, nk, 3), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    counts = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    hip.match_orb_batch(k1, cnt, k2, cnt, matches, counts, 60.0)
    one, c1 = torch.empty((nk, 3), dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    got, h = matches.cpu().numpy().view(np.uint32), counts.cpu().numpy()
    for p in range(n):
        one.fill_(0x5A5A5A5A)
        hip.match_orb_dev(k1[p], nk, k2[p], nk, one, c1, nk, 60.0)
        torch.cuda.synchronize()
        assert int(c1[0]) == h[p] and torch.equal(one, matches[p]), p
    for p in (0, n - 1):
        want = oracle.match_orb(mc.records(sets[p][0]), mc.records(sets[p][1]), nk, 60.0).view(np.uint32).reshape(-1, 3)
        assert h[p] == len(want) > 100 and np.array_equal(got[p, :h[p]], want), p
        assert (got[p, h[p]:] == 0x5A5A5A5A).all(), p


def test_extract_then_match_unsynced_on_a_caller_stream(hip):
    """orb_extract_batch_nostdlib -> match_orb_batch (frame f against frame (f + 1) mod n, counts_dev passed straight
    through as n1 and n2) after gsh_set_stream on a torch stream and under gsh_set_async(1) with nothing between the calls,
    compared after ONE sync with the run that synchronised after every call and with the oracle on the downloaded keypoints"""
    import torch
    from oracle.pyoracle import Oracle
    n, nkps, h, w = 6, 120, 120, 160
    base = Oracle.synth(w + 10, h + 6, 5)
    frames = np.stack([np.ascontiguousarray(base[f:f + h, 2 * f:2 * f + w]) for f in range(n)])  # the scene, shifted

    def chain(sync):
        img = torch.from_numpy(frames).cuda()
        sm = torch.zeros_like(img)
        kps = torch.zeros((n, nkps, 12), dtype=torch.int32, device="cuda")
        cnt = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        nxt_k, nxt_c = torch.empty_like(kps), torch.empty_like(cnt)
        matches = torch.full((n, nkps, 3), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        counts = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        hip.orb_extract_batch_nostdlib(img, sm, kps, cnt, nkps, 20), sync()
        nxt_k.copy_(torch.roll(kps, -1, 0)), nxt_c.copy_(torch.roll(cnt, -1, 0))  # torch work on the same stream, no sync
        hip.match_orb_batch(kps, cnt, nxt_k, nxt_c, matches, counts, 60.0), sync()
        return kps, cnt, matches, counts

    synced = [a.cpu().numpy() for a in chain(torch.cuda.synchronize)]
    kps, cnt, matches, counts = synced
    assert (cnt > 20).all() and (cnt <= nkps).all() and counts.sum() > 20
    o = Oracle("port")
    for f in range(n):
        g = (f + 1) % n
        want = o.match_orb(kps[f, :cnt[f]].reshape(-1).view(KEYPOINT_DTYPE), kps[g, :cnt[g]].reshape(-1).view(KEYPOINT_DTYPE), nkps, 60.0)
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
