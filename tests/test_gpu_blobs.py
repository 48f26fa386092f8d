"""gs_blobs / gs_blob_corners / gs_perspective_correct on the MI355X: the hand-derived cases, 4K frames against the
compiled reference (oracle/_ref/libgs_ref.so) through the host- and device-pointer drop-in paths and the batches,
and the nanomagick `scan` chain device-resident end to end.  Unlike the emulator, which runs one block at a time,
these runs have thousands of waves racing through the union-find."""
import os

import numpy as np
import pytest

import blob_cases as bc
from grayskull_amd import BLOB_DTYPE
from test_blobs import check_hand_cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ref():
    from oracle import pyoracle
    if not pyoracle.have_reference():
        pytest.skip("oracle/_ref/libgs_ref.so not built")
    return bc.Ref()


def _recs(t):
    """(n, nblobs, 8) int32 tensor -> numpy BLOB_DTYPE records"""
    return t.cpu().numpy().view(BLOB_DTYPE).reshape(t.shape[0], t.shape[1])


def test_hand_derived_cases_gpu(hip):
    check_hand_cases(hip)


def frames_4k(rng, n):
    h, w = 2160, 3840
    out = []
    for i in range(n):
        kind = i % 4
        if kind == 0:
            out.append(bc.random_mask(rng, h, w, 0.59))
        elif kind == 1:
            img = bc.blurred_noise(rng, h, w)
            out.append(np.where(img > np.median(img), 255, 0).astype(np.uint8))
        elif kind == 2:
            out.append(bc.maze(rng, h, w))
        else:
            out.append(bc.spiral(h, w, gap=3) | bc.dots(h, w))
    return out


@pytest.mark.parametrize("cap", [1, 150, 1000, 65534, 65535])
def test_4k_dropin_host_and_device_vs_reference(hip, cap):
    import torch
    ref = _ref()
    rng = np.random.default_rng(cap)
    for img in frames_4k(rng, 4):
        starts = bc.start_count(img)
        if cap >= 65535 and starts > 65535:
            continue  # the reference is undefined there (it writes blobs[-1])
        want = ref.blobs(img, cap)
        bc.assert_blobs_equal(hip.blobs(img, cap), want, "host cap %d" % cap)
        dimg = torch.from_numpy(img).cuda()
        dlab = torch.zeros(img.shape, dtype=torch.int16, device="cuda")
        recs, lab = hip.blobs(dimg, cap, labels=dlab)
        bc.assert_blobs_equal((recs, lab.cpu().numpy().view(np.uint16)), want, "device cap %d" % cap)


def test_checkerboard_and_caps_around_the_start_count(hip):
    ref = _ref()
    chk = bc.checkerboard(250, 517)  # no 4-adjacent pair: every fg pixel is a start pixel (64625 of them)
    starts = bc.start_count(chk)
    assert starts < 65535
    for cap in (1, starts - 1, starts, starts + 1, 65534, 65535):
        bc.assert_blobs_equal(hip.blobs(chk, cap), ref.blobs(chk, cap), "checkerboard cap %d" % cap)
    rng = np.random.default_rng(3)
    for w in (63, 65, 1000, 4097):
        img = bc.random_mask(rng, 71, w, 0.6)
        starts = bc.start_count(img)
        for cap in (1, 150, max(1, starts // 2), starts, starts + 1):
            bc.assert_blobs_equal(hip.blobs(img, cap), ref.blobs(img, cap), "w %d cap %d" % (w, cap))


@pytest.mark.parametrize("n,cap", [(8, 1000), (64, 65534)])
def test_4k_batch_vs_reference_and_dropin(hip, n, cap):
    import torch
    ref = _ref()
    rng = np.random.default_rng(n)
    frames = frames_4k(rng, 4)
    batch = np.stack([frames[i % 4] if i < 4 else np.roll(frames[i % 4], 37 * i, axis=1) for i in range(n)])
    dimg = torch.from_numpy(batch).cuda()
    lab = torch.zeros(batch.shape, dtype=torch.int16, device="cuda")
    blobs = torch.zeros((n, cap, 8), dtype=torch.int32, device="cuda")
    counts = torch.zeros(n, dtype=torch.int32, device="cuda")
    hip.blobs_batch(dimg, lab, blobs, counts, cap)
    torch.cuda.synchronize()
    recs, labs, cnt = _recs(blobs), lab.cpu().numpy().view(np.uint16), counts.cpu().numpy()
    checked = 0
    for f in range(n):
        got = (recs[f, :cnt[f]], labs[f])
        if f < 8:  # the reference costs ~50 ms per 4K frame: check the first eight against it, the rest per call
            bc.assert_blobs_equal(got, ref.blobs(batch[f], cap), "batch frame %d" % f)
        bc.assert_blobs_equal(got, hip.blobs(batch[f], cap), "batch vs drop-in frame %d" % f)
        checked += 1
    assert checked == n


def test_frames_per_launch_split(hip):
    """gsh_tune key 8 lowers the frames per launch: the split must not change any frame's result"""
    import torch
    rng = np.random.default_rng(11)
    batch = np.stack([bc.random_mask(rng, 97, 203, 0.6) for _ in range(7)])
    dimg = torch.from_numpy(batch).cuda()
    outs = []
    for fpl in (0, 3):
        hip.tune(8, fpl)
        try:
            lab = torch.zeros(batch.shape, dtype=torch.int16, device="cuda")
            blobs = torch.zeros((7, 300, 8), dtype=torch.int32, device="cuda")
            counts = torch.zeros(7, dtype=torch.int32, device="cuda")
            hip.blobs_batch(dimg, lab, blobs, counts, 300)
            corners = torch.zeros((7, 4, 2), dtype=torch.int32, device="cuda")
            hip.blob_corners_batch(dimg, lab, blobs[:, 0].contiguous(), corners)
            dst = torch.zeros((7, 40, 30), dtype=torch.uint8, device="cuda")
            hip.perspective_correct_batch(dst, dimg, corners)
            torch.cuda.synchronize()
            outs.append([t.cpu().numpy() for t in (lab, blobs, counts, corners, dst)])
        finally:
            hip.tune(8, 0)
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
    for f in range(7):
        bc.assert_blobs_equal((_recs(torch.from_numpy(outs[0][1]))[f, :outs[0][2][f]], outs[0][0][f].view(np.uint16)),
                              bc.spec_blobs(batch[f], 300), "frame %d" % f)


def _read_pgm(path):
    data = open(path, "rb").read()
    parts = data.split(maxsplit=4)
    w, h = int(parts[1]), int(parts[2])
    return np.frombuffer(parts[4][:w * h], np.uint8).reshape(h, w).copy()


def test_scan_chain_device_resident_vs_reference(hip):
    """nanomagick `scan` (ref nanomagick.c:187-210) on a batch: blur 1 -> Otsu + 10 -> threshold -> gs_blobs(1000)
    -> largest blob (first maximum, torch.argmax) -> corners -> 800 x 1000 perspective, with no host round trip,
    against the reference's functions frame by frame"""
    import torch
    ref = _ref()
    rng = np.random.default_rng(9)
    lena = _read_pgm(os.path.join(ROOT, "tests", "golden", "lena.pgm"))
    h, w = 720, 1280
    frames = [np.pad(lena, ((0, h - lena.shape[0]), (0, w - lena.shape[1])), mode="reflect")]
    frames += [bc.blurred_noise(rng, h, w, passes=p) for p in (1, 3, 6)]
    doc = np.full((h, w), 40, np.uint8)
    doc[100:620, 300:1000] = 220
    doc[150:200, 350:900] = 30
    frames.append(np.clip(doc.astype(np.int32) + rng.integers(-25, 25, (h, w)), 0, 255).astype(np.uint8))
    batch = np.stack(frames)
    n, cap, dw, dh = len(frames), 1000, 800, 1000
    src = torch.from_numpy(batch).cuda()
    tmp = torch.zeros_like(src)
    hip.blur_batch(tmp, src, 1)
    hist = torch.zeros((n, 256), dtype=torch.int32, device="cuda")
    thr = torch.zeros(n, dtype=torch.uint8, device="cuda")
    hip.otsu_batch(tmp, hist, thr)
    thr10 = ((thr.to(torch.int32) + 10) & 255).to(torch.uint8)
    hip.threshold_batch(tmp, thr10)
    lab = torch.zeros(batch.shape, dtype=torch.int16, device="cuda")
    blobs = torch.zeros((n, cap, 8), dtype=torch.int32, device="cuda")
    counts = torch.zeros(n, dtype=torch.int32, device="cuda")
    hip.blobs_batch(tmp, lab, blobs, counts, cap)
    valid = torch.arange(cap, device="cuda")[None, :] < counts[:, None]
    area = torch.where(valid, blobs[:, :, 1].to(torch.int64), torch.full_like(blobs[:, :, 1], -1, dtype=torch.int64))
    largest = torch.argmax(area, dim=1)
    chosen = blobs[torch.arange(n, device="cuda"), largest].contiguous()
    corners = torch.zeros((n, 4, 2), dtype=torch.int32, device="cuda")
    hip.blob_corners_batch(tmp, lab, chosen, corners)
    out = torch.zeros((n, dh, dw), dtype=torch.uint8, device="cuda")
    hip.perspective_correct_batch(out, src, corners)
    torch.cuda.synchronize()
    recs, labs, cnt = _recs(blobs), lab.cpu().numpy().view(np.uint16), counts.cpu().numpy()
    over = 0
    for f in range(n):
        r_tmp, r_recs, r_labels, r_largest, r_corners, r_out = ref.scan(batch[f], cap, dw, dh)
        over += bc.start_count(r_tmp) > cap
        assert np.array_equal(tmp[f].cpu().numpy(), r_tmp), "frame %d: thresholded frame" % f
        bc.assert_blobs_equal((recs[f, :cnt[f]], labs[f]), (r_recs, r_labels), "frame %d" % f)
        assert int(largest[f]) == r_largest, f
        assert [tuple(p) for p in corners[f].cpu().numpy().tolist()] == [tuple(p) for p in r_corners], f
        assert np.array_equal(out[f].cpu().numpy(), r_out), "frame %d: perspective" % f
    assert over >= 1, "no frame exercised the capped path"
