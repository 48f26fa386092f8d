"""gs_trace_contour on the MI355X: the checks of tests/test_contours.py through the product library -- host and
device pointers of the drop-in call, the batch, 4K frames against the compiled reference (oracle/_ref/libgs_ref.so),
endless walks against the restatement, and the chain threshold -> blobs -> contour starts -> trace device-resident
end to end."""
import os

import numpy as np
import pytest

import blob_cases as bc
import contour_cases as cc
from grayskull_amd import BLOB_DTYPE, CONTOUR_DTYPE
from test_contours import (batch_trace, build_c_program, chain_expected, check_endless, check_family_frames, check_hand_cases,
                           check_split, check_starts_glue, family_frames)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class DeviceTensors:
    """numpy <-> torch tensors on the GPU (int32 / int16 / uint8 views of the records)"""

    @staticmethod
    def dev(a):
        import torch
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    @staticmethod
    def host(t):
        return t.cpu().numpy()

    @staticmethod
    def sync():
        import torch
        torch.cuda.synchronize()


def _ref():
    from oracle import pyoracle
    if not pyoracle.have_reference():
        pytest.skip("oracle/_ref/libgs_ref.so not built")
    return cc.Ref()


def dropin_device_sequence(hip, img, starts):
    """the drop-in call with DEVICE pointers for img.data and visited.data"""
    import torch
    dimg = torch.from_numpy(img).cuda()
    dvis = torch.zeros(img.shape, dtype=torch.uint8, device="cuda")
    got = [cc.rec_tuple(hip.trace_contour(dimg, dvis, s)) for s in starts]
    return got, dvis.cpu().numpy()


def test_hand_derived_cases_gpu(hip):
    check_hand_cases(hip, DeviceTensors)


@pytest.mark.parametrize("w", [63, 65, 200, 1000, 4097])
def test_ending_walks_match_reference_gpu(hip, w):
    ref = _ref()
    rng = np.random.default_rng(w)
    check_family_frames(hip, DeviceTensors, ref, family_frames(rng, 70 + w % 7, w), "w %d" % w, dropin_device=dropin_device_sequence)


def test_4k_frames_match_reference_gpu(hip):
    """4 frames of 3840 x 2160 as one batch and through the drop-in on host and on device pointers.  The disc and
    rectangle frames take every start pixel; on the noise frames one cluster spans the frame and each start pixel on
    its rim walks about 70 000 moves, so "every start pixel" (some 10^5 per frame) would be 10^9 moves and more per
    frame for the restatement that has to decide each walk before the reference may be called: a sample spread over
    the whole frame, at least 12 start pixels, traced in raster order on one plane (cc.sampled_starts)"""
    ref = _ref()
    rng = np.random.default_rng(4)
    h, w = 2160, 3840
    frames = [cc.upscaled_noise(rng, h, w, 3), cc.random_discs(rng, h, w, 400, 5, 90), cc.random_rects(rng, h, w, 400, 3, 200),
              cc.upscaled_noise(rng, h, w, 2)]
    frames[2][::, :] |= bc.spiral(h, w, gap=3) & np.where(np.indices((h, w))[1] < 700, 255, 0).astype(np.uint8)
    check_family_frames(hip, DeviceTensors, ref, frames, "4K", budget=1000000, dropin_device=dropin_device_sequence)


def test_endless_walks_match_restatement_gpu(hip):
    rng = np.random.default_rng(6)
    frames = [cc.random_mask(rng, 128, 96, 0.6)]
    img = bc.blurred_noise(rng, 128, 96, passes=1)
    frames.append(np.where(img > np.median(img), 255, 0).astype(np.uint8))
    check_endless(hip, DeviceTensors, frames, "96 x 128")
    # endless walks that cross many tiles: a 1-px maze and a random mask at 720p, the batch only
    big = [bc.maze(rng, 720, 1280), cc.random_mask(rng, 720, 1280, 0.6)]
    check_endless(hip, DeviceTensors, big, "720p", dropin_stride=10 ** 9, budget=400000)


def test_blob_contour_starts_gpu(hip):
    check_starts_glue(hip, DeviceTensors, np.random.default_rng(21))


def test_frames_per_launch_split_gpu(hip):
    check_split(hip, DeviceTensors)


def test_chain_device_resident_vs_reference(hip):
    """threshold_batch -> blobs_batch(cap 1000) -> blob_contour_starts_batch -> trace_contours_batch on 9 frames of
    1280 x 720 with no host round trip, against the reference's gs_blobs, a host search for each blob's first labelled
    pixel and gs_trace_contour per blob in label order (endless walks: the restatement); counts differ per frame, one
    frame traces nothing, and a second pass without status gives the same records"""
    import torch
    ref = _ref()
    rng = np.random.default_rng(9)
    h, w, cap = 720, 1280, 1000
    doc = np.full((h, w), 40, np.uint8)
    doc[100:620, 300:1000] = 220
    doc[150:200, 350:900] = 30
    doc = np.clip(doc.astype(np.int32) + rng.integers(-25, 25, (h, w)), 0, 255).astype(np.uint8)
    gray = [np.where(cc.upscaled_noise(rng, h, w, 3) > 0, 200, 60).astype(np.uint8) for _ in range(4)]
    gray += [np.where(cc.random_discs(rng, h, w, 60, 4, 60) > 0, 180, 20).astype(np.uint8) for _ in range(3)]
    gray += [doc, np.full((h, w), 10, np.uint8)]  # the last frame has no blob at all: counts[f] = 0
    n = len(gray)
    assert n >= 8
    src = torch.from_numpy(np.stack(gray)).cuda()
    hip.threshold_batch(src, 128)
    lab = torch.zeros(src.shape, dtype=torch.int16, device="cuda")
    blobs = torch.zeros((n, cap, 8), dtype=torch.int32, device="cuda")
    counts = torch.zeros(n, dtype=torch.int32, device="cuda")
    hip.blobs_batch(src, lab, blobs, counts, cap)
    cont = torch.zeros((n, cap, 7), dtype=torch.int32, device="cuda")
    hip.blob_contour_starts_batch(lab, blobs, counts, cont)
    cont2 = cont.clone()
    vis = torch.zeros_like(src)
    st = torch.zeros((n, cap), dtype=torch.uint8, device="cuda")
    hip.trace_contours_batch(src, vis, cont, counts, st)
    vis2 = torch.zeros_like(src)
    hip.trace_contours_batch(src, vis2, cont2, counts, None)  # status == NULL
    torch.cuda.synchronize()
    assert torch.equal(cont, cont2) and torch.equal(vis, vis2)
    binary, cnt = src.cpu().numpy(), counts.cpu().numpy()
    got = cont.cpu().numpy().view(CONTOUR_DTYPE).reshape(n, cap)
    gvis, gst = vis.cpu().numpy(), st.cpu().numpy()
    assert cnt[-1] == 0 and not gvis[-1].any() and len(set(cnt.tolist())) > 3
    total = endless = 0
    for f in range(n):
        assert np.array_equal(binary[f], np.where(gray[f] > 128, 255, 0))
        recs, labels, starts, want, want_vis, e = chain_expected(ref, binary[f], cap)
        assert int(cnt[f]) == len(recs), f
        assert [(int(r["sx"]), int(r["sy"])) for r in got[f, :len(recs)]] == starts, f
        cc.assert_sequence_equal([cc.rec_tuple(r) for r in got[f, :len(recs)]], gvis[f], want, want_vis, "frame %d" % f,
                                 got_status=gst[f])
        total, endless = total + len(recs), endless + e
    assert total > 1000 and endless * 10 <= total


def test_c99_contour_program_against_product_library(tmp_path, hip):
    assert "all passed" in build_c_program(tmp_path, os.path.join(ROOT, "grayskull_amd"), "libgrayskull_hip.so")
