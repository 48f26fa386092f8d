#!/usr/bin/env python3
"""gsh_blobs_batch on 64 x 3840x2160 frames in four input families, per-frame times from device events around a
synchronised, warmed-up batch; the batched `scan` chain (nanomagick.c:187-210) per frame; the reference's CPU time
per frame (oracle/_ref/libgs_ref.so, one thread) and an output check of every timed frame against it.
"single_frame_dropin_us" is one frame through the drop-in gs_blobs on device pointers (wall clock, synchronised).
Per family also gsh_blob_paint_batch (the picture of nanomagick's `blobs` verb) beside gsh_threshold_batch -- the 2 B/px
pointwise pass -- on the same buffers; the scan chain once with torch.argmax and once through the C entry points
(gsh_threshold_batch_dev_offset, gsh_blob_largest_batch); and the wall time of `gsbatch blobs 150` / `gsbatch scan` on
64 4K PGM files.
Prints one JSON line.  BLOBS_FRAMES / BLOBS_REPS override the batch size / timed repetitions; BLOBS_SKIP_REF=1 leaves
out the reference's CPU runs (and the checks against it), BLOBS_GSBATCH=0 the gsbatch runs."""
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import grayskull_amd as gs  # noqa: E402
import blob_cases as bc  # noqa: E402
import blob_paint_cases as bpc  # noqa: E402
from grayskull_amd import BLOB_DTYPE  # noqa: E402

g = gs.lib()
g.use_torch_stream()
n, h, w = int(os.environ.get("BLOBS_FRAMES", 64)), 2160, 3840
reps = int(os.environ.get("BLOBS_REPS", 5))
skip_ref = os.environ.get("BLOBS_SKIP_REF") == "1"
gen = torch.Generator(device="cuda").manual_seed(1234)


def otsu_mask(x):
    hist = torch.zeros((n, 256), dtype=torch.int32, device="cuda")
    thr = torch.zeros(n, dtype=torch.uint8, device="cuda")
    g.otsu_batch(x, hist, thr)
    g.threshold_batch(x, thr)
    return x


def family(name):
    if name == "noise_otsu_cap1000":  # blurred noise thresholded at Otsu: ~10^5 start pixels, the capped path
        noise = torch.randint(0, 256, (n, 1, h, w), generator=gen, device="cuda", dtype=torch.uint8).float()
        return otsu_mask(F.avg_pool2d(noise, 5, stride=1, padding=2).to(torch.uint8)[:, 0].contiguous()), 1000
    if name == "dots16_cap65534":  # 5x5 dots on a 16-px lattice: 32400 blobs, uncapped
        return torch.from_numpy(np.stack([bc.dots(h, w, 16, 5)] * n)).cuda(), 65534
    if name == "document_cap1000":  # heavily blurred noise: a few large blobs
        low = torch.randint(0, 256, (n, 1, h // 90, w // 90), generator=gen, device="cuda", dtype=torch.uint8).float()
        up = F.interpolate(low, size=(h, w), mode="bilinear", align_corners=False).to(torch.uint8)[:, 0].contiguous()
        return otsu_mask(up), 1000
    if name == "all_foreground_cap1000":  # one frame-filling blob: the contention case
        return torch.full((n, h, w), 255, dtype=torch.uint8, device="cuda"), 1000
    raise ValueError(name)


def timed(fn):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3 / n  # us per frame


ref = None if skip_ref else bc.Ref()
mask_files = None  # the noise family's masks, kept for the gsbatch runs
out = {"frames": n, "w": w, "h": h, "families": {}}
for name in ("noise_otsu_cap1000", "dots16_cap65534", "document_cap1000", "all_foreground_cap1000"):
    img, cap = family(name)
    lab = torch.zeros((n, h, w), dtype=torch.int16, device="cuda")
    blobs = torch.zeros((n, cap, 8), dtype=torch.int32, device="cuda")
    counts = torch.zeros(n, dtype=torch.int32, device="cuda")
    us = timed(lambda: g.blobs_batch(img, lab, blobs, counts, cap))
    host = img.cpu().numpy()
    labs, cnt = lab.cpu().numpy().view(np.uint16), counts.cpu().numpy()
    recs = blobs.cpu().numpy().view(BLOB_DTYPE).reshape(n, cap)
    ok, ref_ms, starts = 0, [], []
    for f in range(0 if skip_ref else n):
        t0 = time.perf_counter()
        want = ref.blobs(host[f], cap)
        ref_ms.append((time.perf_counter() - t0) * 1e3)
        try:
            bc.assert_blobs_equal((recs[f, :cnt[f]], labs[f]), want, "%s frame %d" % (name, f))
            ok += 1
        except AssertionError as e:
            print("MISMATCH", e, file=sys.stderr)
        if f < 4:
            starts.append(bc.start_count(host[f]))
    # one frame alone: the drop-in gs_blobs on device pointers (it synchronises and reads m back), wall clock
    one, one_lab = img[0], lab[0]
    g.blobs(one, cap, labels=one_lab)
    t0 = time.perf_counter()
    for _ in range(reps):
        g.blobs(one, cap, labels=one_lab)
    single_us = (time.perf_counter() - t0) / reps * 1e6
    # the picture of the `blobs` verb from these records, and the 2 B/px yardstick on the same buffers
    pic = torch.empty_like(img)
    paint_us = timed(lambda: g.blob_paint_batch(pic, img, blobs, counts))
    want_pic, _ = bpc.spec_paint(host[0], recs[0], int(cnt[0]))
    paint_ok = bool(np.array_equal(pic[0].cpu().numpy(), want_pic))
    thr_us = timed(lambda: g.threshold_batch(pic, 128))
    if name == "noise_otsu_cap1000":
        mask_files = host.copy()
    del pic
    out["families"][name] = {"paint_us_per_frame": round(paint_us, 2), "threshold_us_per_frame": round(thr_us, 2),
                             "paint_over_threshold": round(paint_us / thr_us, 2), "paint_frame0_equals_restatement": paint_ok,
                             "cap": cap, "us_per_frame": round(us, 2), "single_frame_dropin_us": round(single_us, 1),
                             "blobs_frame0": int(cnt[0]),
                             "start_pixels_frames0_3": starts, "ref_cpu_ms_per_frame": round(float(np.median(ref_ms)), 2) if ref_ms else None,
                             "frames_equal_to_reference": "%d/%d" % (ok, len(ref_ms))}
    del lab, blobs, img

# the batched scan chain on the noise family's source frames (blur 1 -> Otsu + 10 -> threshold -> blobs(1000) -> largest
# -> corners -> 800 x 1000 perspective), device resident
noise = torch.randint(0, 256, (n, 1, h, w), generator=gen, device="cuda", dtype=torch.uint8).float()
src = F.avg_pool2d(noise, 9, stride=1, padding=4).to(torch.uint8)[:, 0].contiguous()
del noise
tmp = torch.zeros_like(src)
hist = torch.zeros((n, 256), dtype=torch.int32, device="cuda")
thr = torch.zeros(n, dtype=torch.uint8, device="cuda")
lab = torch.zeros((n, h, w), dtype=torch.int16, device="cuda")
blobs = torch.zeros((n, 1000, 8), dtype=torch.int32, device="cuda")
counts = torch.zeros(n, dtype=torch.int32, device="cuda")
corners = torch.zeros((n, 4, 2), dtype=torch.int32, device="cuda")
dst = torch.zeros((n, 1000, 800), dtype=torch.uint8, device="cuda")
ar = torch.arange(1000, device="cuda")[None, :]
rows = torch.arange(n, device="cuda")


def scan():
    g.blur_batch(tmp, src, 1)
    g.otsu_batch(tmp, hist, thr)
    g.threshold_batch(tmp, ((thr.to(torch.int32) + 10) & 255).to(torch.uint8))
    g.blobs_batch(tmp, lab, blobs, counts, 1000)
    area = torch.where(ar < counts[:, None], blobs[:, :, 1].to(torch.int64), -1)
    chosen = blobs[rows, torch.argmax(area, dim=1)].contiguous()
    g.blob_corners_batch(tmp, lab, chosen, corners)
    g.perspective_correct_batch(dst, src, corners)


one = torch.zeros((n, 8), dtype=torch.int32, device="cuda")


def scan_c():  # the same chain through the C entry points alone: what a C caller (gsbatch scan) runs
    g.blur_batch(tmp, src, 1)
    g.otsu_batch(tmp, hist, thr)
    g.threshold_batch_dev_offset(tmp, thr, 10)
    g.blobs_batch(tmp, lab, blobs, counts, 1000)
    g.blob_largest_batch(blobs, counts, one)
    g.blob_corners_batch(tmp, lab, one, corners)
    g.perspective_correct_batch(dst, src, corners)


scan_us = timed(scan)
host_src, got_dst, got_c = src.cpu().numpy(), dst.cpu().numpy(), corners.cpu().numpy()
dst.zero_(), corners.zero_()
scan_c_us = timed(scan_c)
scan_c_equal = bool(np.array_equal(dst.cpu().numpy(), got_dst) and np.array_equal(corners.cpu().numpy(), got_c))
ok, ref_ms, over = 0, [], 0
for f in range(0 if skip_ref else n):
    t0 = time.perf_counter()
    r_tmp, _, _, _, r_corners, r_out = ref.scan(host_src[f])
    ref_ms.append((time.perf_counter() - t0) * 1e3)
    over += bc.start_count(r_tmp) > 1000
    ok += int([tuple(p) for p in got_c[f].tolist()] == [tuple(p) for p in r_corners] and np.array_equal(got_dst[f], r_out))
out["scan_chain"] = {"us_per_frame": round(scan_us, 2), "c_entry_points_us_per_frame": round(scan_c_us, 2),
                     "c_entry_points_equal_argmax_chain": scan_c_equal,
                     "ref_cpu_ms_per_frame": round(float(np.median(ref_ms)), 2) if ref_ms else None,
                     "frames_equal_to_reference": "%d/%d" % (ok, len(ref_ms)), "frames_over_1000_start_pixels": over}

# gsbatch on n 4K PGM files: wall time of the whole process (read, upload, stages, download, write)
exe = os.path.join(ROOT, "grayskull_amd", "gsbatch")
if os.environ.get("BLOBS_GSBATCH", "1") != "0" and os.path.exists(exe) and mask_files is not None:
    work = tempfile.mkdtemp(prefix="gsbatch_blobs_")
    try:
        walls = {}
        for verb, frames, args in (("blobs", mask_files, ["blobs", "150"]), ("scan", host_src, ["scan"])):
            files = []
            for f in range(n):
                path = os.path.join(work, "%s%03d.pgm" % (verb, f))
                with open(path, "wb") as fp:
                    fp.write(b"P5\n%d %d\n255\n" % (w, h))
                    fp.write(frames[f].tobytes())
                files.append(path)
            outdir = os.path.join(work, "out_" + verb)
            os.mkdir(outdir)
            best = None
            for _ in range(2):  # the second run finds the files in the page cache
                t0 = time.perf_counter()
                r = subprocess.run([exe, "-o", outdir, *args, "--", *files], capture_output=True, timeout=600)
                dt = time.perf_counter() - t0
                best = dt if best is None or dt < best else best
            walls[verb] = {"wall_s": round(best, 3), "exit": r.returncode, "files_written": len(os.listdir(outdir))}
            for path in files:
                os.remove(path)
            shutil.rmtree(outdir)
        out["gsbatch_%d_files_4k" % n] = walls
    finally:
        shutil.rmtree(work, ignore_errors=True)
print(json.dumps(out))
