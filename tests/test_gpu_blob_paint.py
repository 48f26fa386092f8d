"""gsh_blob_paint_batch, gsh_blob_largest_batch and gsh_threshold_batch_dev_offset on the MI355X: the cases of
tests/blob_paint_cases.py with thousands of blocks racing where the emulator runs one at a time, 1080p frames against
the numpy restatement, the scan chain through the C entry points against the torch.argmax chain, the same chain with no
host sync on a caller's stream, and the real gsbatch binary against the reference's nanomagick (oracle/_ref/nano_ref,
built beforehand; the reference checkout itself is not read here)."""
import os
import subprocess

import numpy as np
import pytest

import blob_cases as bc
import blob_paint_cases as pc
from grayskull_amd import BLOB_DTYPE

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENA = os.path.join(ROOT, "tests", "golden", "lena.pgm")


def test_hand_cases_gpu(hip):
    pc.check_hand_cases(hip, pc.Device)


def test_shapes_and_band_heights_gpu(hip):
    pc.check_shapes(hip, pc.Device)


def test_batches_gpu(hip):
    pc.check_batches(hip, pc.Device)


def test_largest_gpu(hip):
    pc.check_largest(hip, pc.Device)


def test_threshold_offset_gpu(hip):
    pc.check_threshold_offset(hip, pc.Device)


def _blobs_batch(hip, batch, cap):
    import torch
    n = batch.shape[0]
    dimg = torch.from_numpy(batch).cuda()
    lab = torch.zeros(batch.shape, dtype=torch.int16, device="cuda")
    blobs = torch.zeros((n, cap, 8), dtype=torch.int32, device="cuda")
    counts = torch.zeros(n, dtype=torch.int32, device="cuda")
    hip.blobs_batch(dimg, lab, blobs, counts, cap)
    return dimg, lab, blobs, counts


def _paint_and_check(hip, batch, cap, what):
    """records from gsh_blobs_batch itself (tests/test_gpu_blobs.py pins them to the reference), the picture against
    the restatement; guard bytes around dst stay untouched"""
    import torch
    n, h, w = batch.shape
    dimg, _, blobs, counts = _blobs_batch(hip, batch, cap)
    guard = torch.full((n + 2, h, w), 77, dtype=torch.uint8, device="cuda")
    hip.blob_paint_batch(guard[1:n + 1], dimg, blobs, counts)
    torch.cuda.synchronize()
    out, cnt = guard.cpu().numpy(), counts.cpu().numpy()
    recs = blobs.cpu().numpy().view(BLOB_DTYPE).reshape(n, cap)
    assert (out[0] == 77).all() and (out[n + 1] == 77).all(), "written outside dst"
    for f in range(n):
        pc.assert_label_order(recs[f, :cnt[f]], what)
        want, _ = pc.spec_paint(batch[f], recs[f], int(cnt[f]))
        assert np.array_equal(out[f + 1], want), "%s frame %d: %d bytes differ" % (what, f, np.count_nonzero(out[f + 1] != want))
    return cnt


def test_1080p_one_frame_filling_blob(hip):
    img = np.full((1, 1080, 1920), 255, np.uint8)
    img[0, ::97, ::89] = 128  # still foreground for gs_blobs, grey in the picture
    cnt = _paint_and_check(hip, img, 150, "frame-filling blob")
    assert cnt[0] == 1


def test_1080p_dots_at_cap_65534(hip):
    img = bc.dots(1080, 1920, period=6, size=3)[None]
    cnt = _paint_and_check(hip, img, 65534, "dots")
    assert cnt[0] == 180 * 320


def test_noise_masks_at_cap_150(hip):
    rng = np.random.default_rng(150)
    batch = np.stack([bc.random_mask(rng, 612, 816, d) for d in (0.3, 0.45, 0.55, 0.59, 0.62, 0.7, 0.05, 0.9)])
    cnt = _paint_and_check(hip, batch, 150, "noise")
    assert (cnt <= 150).all() and cnt.max() == 150


def _scan_frames():
    rng = np.random.default_rng(9)
    lena = np.frombuffer(open(LENA, "rb").read()[-128 * 128:], np.uint8).reshape(128, 128)
    h, w = 360, 640
    frames = [np.pad(lena, ((0, h - 128), (0, w - 128)), mode="reflect")]
    frames += [bc.blurred_noise(rng, h, w, passes=p) for p in (1, 3, 6)]
    doc = np.full((h, w), 40, np.uint8)
    doc[50:310, 150:500] = 220
    doc[75:100, 175:450] = 30
    frames.append(np.clip(doc.astype(np.int32) + rng.integers(-25, 25, (h, w)), 0, 255).astype(np.uint8))
    return np.stack(frames)


def _scan_chain(hip, src, c_entry_points, sync):
    """nanomagick's scan on a batch; c_entry_points: threshold offset + largest on the device through the library,
    else the torch.argmax chain of tests/test_gpu_blobs.py.  sync: synchronise after every call."""
    import torch
    n, cap = src.shape[0], 1000
    step = torch.cuda.synchronize if sync else (lambda: None)
    tmp = torch.zeros_like(src)
    hist = torch.zeros((n, 256), dtype=torch.int32, device="cuda")
    thr = torch.zeros(n, dtype=torch.uint8, device="cuda")
    lab = torch.zeros(src.shape, dtype=torch.int16, device="cuda")
    blobs = torch.zeros((n, cap, 8), dtype=torch.int32, device="cuda")
    counts = torch.zeros(n, dtype=torch.int32, device="cuda")
    corners = torch.zeros((n, 4, 2), dtype=torch.int32, device="cuda")
    out = torch.zeros((n, 1000, 800), dtype=torch.uint8, device="cuda")
    index = torch.zeros(n, dtype=torch.int32, device="cuda")
    hip.blur_batch(tmp, src, 1), step()
    hip.otsu_batch(tmp, hist, thr), step()
    if c_entry_points:
        hip.threshold_batch_dev_offset(tmp, thr, 10), step()
    else:
        hip.threshold_batch(tmp, ((thr.to(torch.int32) + 10) & 255).to(torch.uint8)), step()
    hip.blobs_batch(tmp, lab, blobs, counts, cap), step()
    if c_entry_points:
        chosen = torch.zeros((n, 8), dtype=torch.int32, device="cuda")
        hip.blob_largest_batch(blobs, counts, chosen, index), step()
    else:
        valid = torch.arange(cap, device="cuda")[None, :] < counts[:, None]
        area = torch.where(valid, blobs[:, :, 1].to(torch.int64), torch.full_like(blobs[:, :, 1], -1, dtype=torch.int64))
        index = torch.argmax(area, dim=1).to(torch.int32)
        chosen = blobs[torch.arange(n, device="cuda"), index.long()].contiguous()
    hip.blob_corners_batch(tmp, lab, chosen, corners), step()
    hip.perspective_correct_batch(out, src, corners), step()
    return {"tmp": tmp, "counts": counts, "index": index, "chosen": chosen, "corners": corners, "out": out}


def _host(run):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in run.items()}


def test_scan_chain_through_c_entry_points_equals_argmax_chain(hip):
    import torch
    src = torch.from_numpy(_scan_frames()).cuda()
    want, got = _host(_scan_chain(hip, src, False, True)), _host(_scan_chain(hip, src, True, True))
    assert (want["counts"] >= 1).all()
    for k in want:
        assert np.array_equal(want[k], got[k]), k


def test_scan_chain_unsynced_on_a_caller_stream(hip):
    """the chain through the new entry points enqueued with no sync, after gsh_set_stream on a torch stream and under
    gsh_set_async(1): the bytes of the run that synchronised after every call"""
    import torch
    src = torch.from_numpy(_scan_frames()).cuda()
    want = _host(_scan_chain(hip, src, True, True))
    pic_want = torch.zeros_like(src)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    try:
        hip.set_stream(st.cuda_stream)
        hip.set_async(True)
        with torch.cuda.stream(st):
            run = _scan_chain(hip, src, True, False)
            # the paint of the binarised frames from the records still in flight, same stream, no sync
            pic = torch.zeros_like(src)
            blobs_again = _blobs_batch_on(hip, run["tmp"])
            hip.blob_paint_batch(pic, run["tmp"], blobs_again[0], blobs_again[1])
        st.synchronize()
        got = _host(run)
    finally:
        hip.set_async(False)
        hip.set_stream(None)
    for k in want:
        assert np.array_equal(want[k], got[k]), k
    blobs_sync = _blobs_batch_on(hip, run["tmp"])
    torch.cuda.synchronize()
    hip.blob_paint_batch(pic_want, run["tmp"], blobs_sync[0], blobs_sync[1])
    torch.cuda.synchronize()
    assert torch.equal(pic, pic_want) and bool((pic == 128).any())


def _blobs_batch_on(hip, dimg):
    import torch
    n = dimg.shape[0]
    lab = torch.zeros(dimg.shape, dtype=torch.int16, device="cuda")
    blobs = torch.zeros((n, 150, 8), dtype=torch.int32, device="cuda")
    counts = torch.zeros(n, dtype=torch.int32, device="cuda")
    hip.blobs_batch(dimg, lab, blobs, counts, 150)
    return blobs, counts


def test_gsbatch_blobs_and_scan_on_gpu(hip, tmp_path):
    """the real binary: `blobs 150`, the reference Makefile's pipe and `scan` on lena-derived files against the piped
    reference CLI (inputs prepared and checked to drop no index, like tests/test_gsbatch_blobs.py)"""
    from tests.test_gsbatch import chain_args, nano_chain, write_pgm
    from tests.util import read_pgm
    nano = os.path.join(ROOT, "oracle", "_ref", "nano_ref")
    if not os.path.exists(nano):
        pytest.skip("oracle/_ref/nano_ref was not prebuilt")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "grayskull_amd", "csrc"), "tool"])
    exe = os.path.join(ROOT, "grayskull_amd", "gsbatch")
    a = read_pgm(LENA)
    files = []
    for k, img in enumerate((a, np.roll(a, 31, axis=1), np.kron(a, np.ones((3, 5), np.uint8)))):  # 128 x 128 twice, 640 x 384
        img = np.ascontiguousarray(img).copy()
        img[-(img.shape[0] // 3):] = 0
        img[0, 0] = 40
        p = str(tmp_path / ("in%d.pgm" % k))
        write_pgm(p, img)
        files.append(p)
    pipe = [("blur", ["3"]), ("sobel", []), ("threshold", ["otsu"]), ("morph", ["dilate", "9"]), ("morph", ["erode", "10"]),
            ("blobs", ["150"])]
    for c, chain in enumerate(([("blobs", ["150"])], pipe, [("scan", [])])):
        outdir = tmp_path / ("out%d" % c)
        outdir.mkdir()
        r = subprocess.run([exe, "-v", "-o", str(outdir), *chain_args(chain), "--", *files], capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr.decode()[-800:]
        for i, f in enumerate(files):
            if chain[-1][0] == "blobs":
                before = f if len(chain) == 1 else nano_chain(nano, chain[:-1], f, tmp_path, "pre%d_%d" % (c, i))[0]
                img = read_pgm(before)
                recs, _ = hip.blobs(img, 150)
                assert len(recs) >= 1 and pc.spec_paint(img, recs, len(recs))[1].size == 0, "input reaches row h"
            exp, err = nano_chain(nano, chain, f, tmp_path, "ref%d_%d" % (c, i))
            assert exp is not None, err
            assert open(str(outdir / os.path.basename(f)), "rb").read() == open(exp, "rb").read(), (c, f)
