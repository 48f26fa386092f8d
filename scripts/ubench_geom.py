#!/usr/bin/env python3
"""gsh_resize_batch / gsh_crop_batch / gsh_crop_resize_batch against THE PARENT COMMIT'S PATH: n stream-ordered per-frame
gs_resize / gs_crop calls on device pointers under gsh_set_async(1) (what gsbatch's `resize` and `crop` stages ran), the
parent's per-pixel kernels included.  The parent library is built beside this one:

    git worktree add /tmp/gs_parent HEAD~0     # or: the commit to compare with
    make -C /tmp/gs_parent/grayskull_amd/csrc all && mkdir -p build_variants && \
        cp /tmp/gs_parent/grayskull_amd/libgrayskull_hip.so build_variants/libgs_parent.so
    make -C grayskull_amd/csrc experiment      # build_variants/libgs_experiment.so: gsh_probe_strip_copy, the rate unit
    python scripts/ubench_geom.py [out.json]   # default profiles/geom_batch.json; the log is stdout

Per shape: events around back-to-back calls after a warm-up, ROUNDS rounds with the forms alternating inside every round
(parent per-frame loop, the batch call, the batch call forced into the gather and into the staged form = gsh_tune key 25,
1 and 2), the median with min and max
kept; the outputs of the forms compared byte for byte; the bytes that must move (every source byte the result depends on
once + every result byte once) divided by the time, as a fraction of gsh_probe_strip_copy's rate on this box.  Without
build_variants/libgs_parent.so / libgs_experiment.so the columns that need them are null ("unmeasured")."""
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import grayskull_amd as gs
from grayskull_amd._abi import GsImage, GsRect

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "geom_batch.json")
ROUNDS = 5
g = gs.Grayskull(os.environ["UB_LIB"]) if os.environ.get("UB_LIB") else gs.lib()
g.use_torch_stream()
g.set_async(True)


def raw(path):
    """a library without the new entries (the parent) or with the probe: only the symbols used here are bound"""
    if not os.path.exists(path):
        return None
    c = C.CDLL(path)
    c.gsh_set_stream.argtypes, c.gsh_set_async.argtypes = [C.c_void_p], [C.c_int]
    c.gs_resize.argtypes = c.gs_resize_nn.argtypes = [GsImage, GsImage]
    c.gs_crop.argtypes = [GsImage, GsImage, GsRect]
    for f in (c.gsh_set_stream, c.gsh_set_async, c.gs_resize, c.gs_resize_nn, c.gs_crop):
        f.restype = None
    c.gsh_set_stream(C.c_void_p(torch.cuda.current_stream().cuda_stream))
    c.gsh_set_async(1)
    return c


parent = raw(os.environ.get("UB_PARENT", os.path.join(ROOT, "build_variants", "libgs_parent.so")))
probe = raw(os.environ.get("UB_PROBE", os.path.join(ROOT, "build_variants", "libgs_experiment.so")))
if probe is not None:
    probe.gsh_probe_strip_copy.argtypes, probe.gsh_probe_strip_copy.restype = [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_uint], None


def timeit(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn(); fn(); torch.cuda.synchronize(); e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def rounds(fns, reps):
    out = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            out[k].append(timeit(fn, reps))
    return out


def img(t):
    return GsImage(int(t.shape[1]), int(t.shape[0]), t.data_ptr())


def strip_copy_rate():
    """GB/s of gsh_probe_strip_copy on 64 x 3840x2160 (read + write), the library's access-pattern ceiling"""
    if probe is None:
        return None
    a = torch.empty((64, 2160, 3840), dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    g.synth_batch(a, 77)
    ms = statistics.median(rounds({"p": lambda: probe.gsh_probe_strip_copy(b.data_ptr(), a.data_ptr(), 3840, 2160, 64)}, 10)["p"])
    return 2 * a.numel() / ms / 1e6


# (call, n, sw, sh, result w, result h or roi, kind)
SHAPES = (("resize", 64, 3840, 2160, (1920, 1080), "downscale"),
          ("resize", 64, 3840, 2160, (640, 360), "downscale"),
          ("resize", 64, 3838, 2160, (1279, 719), "downscale, ragged"),
          ("resize", 256, 1280, 720, (1920, 1080), "upscale"),
          ("resize", 512, 612, 816, (300, 400), "downscale"),
          ("resize", 1, 3840, 2160, (1920, 1080), "the drop-in call's case"),
          ("crop", 64, 3840, 2160, (333, 217, 1920, 1080), "strided copy"),
          ("crop_resize", 64, 3840, 2160, (64, 64), "patch extraction, 6400 random in-frame rois"))

copy_rate = strip_copy_rate()
results = {"device": torch.cuda.get_device_name(0), "library": g.version(), "rounds": ROUNDS,
           "parent_path": "n stream-ordered per-frame gs_resize / gs_crop calls under gsh_set_async(1), parent library" if parent is not None else None,
           "strip_copy_GBps": copy_rate, "rows": []}
print("strip copy rate: %s GB/s" % ("%.0f" % copy_rate if copy_rate else "unmeasured"), flush=True)
for (call, n, sw, sh, res, kind) in SHAPES:
    src = torch.empty((n, sh, sw), dtype=torch.uint8, device="cuda")
    g.synth_batch(src, 500 + n)
    fns, npatch = {}, n
    if call == "resize":
        dw, dh = res
        dst, dst_p = (torch.zeros((n, dh, dw), dtype=torch.uint8, device="cuda") for _ in range(2))
        fns["batch"] = lambda: g.resize_batch(dst, src)
        if parent is not None:
            si, di = [img(src[f]) for f in range(n)], [img(dst_p[f]) for f in range(n)]
            fns["parent"] = lambda: [parent.gs_resize(di[f], si[f]) for f in range(n)]
        # bytes that must move: upscales read every source byte, downscales at most 4 taps per result byte
        moved = n * (min(sw * sh, 4 * dw * dh) + dw * dh)
    elif call == "crop":
        x, y, dw, dh = res
        dst, dst_p = (torch.zeros((n, dh, dw), dtype=torch.uint8, device="cuda") for _ in range(2))
        fns["batch"] = lambda: g.crop_batch(dst, src, x, y, dw, dh)
        if parent is not None:
            si, di, roi = [img(src[f]) for f in range(n)], [img(dst_p[f]) for f in range(n)], GsRect(x, y, dw, dh)
            fns["parent"] = lambda: [parent.gs_crop(di[f], si[f], roi) for f in range(n)]
        moved = 2 * n * dw * dh
    else:
        dw, dh = res
        npatch = 6400
        rs = np.random.RandomState(12)
        rw, rh = rs.randint(16, 513, npatch), rs.randint(16, 513, npatch)
        rx, ry = (rs.rand(npatch) * (sw - rw + 1)).astype(np.int64), (rs.rand(npatch) * (sh - rh + 1)).astype(np.int64)
        rois_h = np.stack([rx, ry, rw, rh], 1).astype(np.int32)
        fo_h = rs.randint(0, n, npatch).astype(np.int32)
        rois, fo = torch.from_numpy(rois_h).cuda(), torch.from_numpy(fo_h).cuda()
        dst, dst_p = (torch.zeros((npatch, dh, dw), dtype=torch.uint8, device="cuda") for _ in range(2))
        tmp = torch.zeros(512 * 512, dtype=torch.uint8, device="cuda")
        fns["batch"] = lambda: g.crop_resize_batch(dst, src, rois, fo)
        if parent is not None:
            # the parent's only way: gs_crop into a temporary + gs_resize, per rectangle (the host round trip that brings the
            # rectangles back is NOT in the timed region)
            ci = [GsImage(int(rw[p]), int(rh[p]), tmp.data_ptr()) for p in range(npatch)]
            fi = [img(src[int(fo_h[p])]) for p in range(npatch)]
            ri = [GsRect(int(rx[p]), int(ry[p]), int(rw[p]), int(rh[p])) for p in range(npatch)]
            di = [img(dst_p[p]) for p in range(npatch)]

            def per_patch():
                for p in range(npatch):
                    parent.gs_crop(ci[p], fi[p], ri[p])
                    parent.gs_resize(di[p], ci[p])
            fns["parent"] = per_patch
        moved = int(sum(min(int(rw[p]) * int(rh[p]), 4 * dw * dh) for p in range(npatch))) + npatch * dw * dh

    def forced(form, batch=None):
        def run():
            g.tune(25, form)
            batch()
            g.tune(25, 0)
        return run
    if call != "crop":  # both forms of k_resize_tile whatever the launcher's rule picks (gsh_tune key 25)
        fns["batch_gather_form"] = forced(1, fns["batch"])
        fns["batch_staged_form"] = forced(2, fns["batch"])
    reps = 50 if n == 1 else (3 if call == "crop_resize" else 10)
    r = rounds(fns, reps)
    same = None
    if parent is not None:
        dst.zero_(), dst_p.zero_()
        fns["batch"](), fns["parent"](), torch.cuda.synchronize()
        same = bool(torch.equal(dst, dst_p))
    row = {"call": call, "frames": n, "sw": sw, "sh": sh, "result": list(res), "kind": kind, "bytes_moved": moved, "same_bytes_as_parent": same}
    for k, v in r.items():
        row[k + "_ms"] = statistics.median(v)
        row[k + "_ms_min_max"] = [min(v), max(v)]
    row["batch_GBps"] = moved / row["batch_ms"] / 1e6
    row["fraction_of_strip_copy"] = row["batch_GBps"] / copy_rate if copy_rate else None
    row["batch_over_parent"] = row["batch_ms"] / row["parent_ms"] if "parent_ms" in row else None
    results["rows"].append(row)
    print("%-11s %3d x %dx%d -> %-22s %-26s batch %.4f ms [%.4f, %.4f]  gather form %s  staged form %s  parent %s  batch/parent %s  %.0f GB/s = %s of strip copy  same bytes: %s" % (
        call, n, sw, sh, res, kind, row["batch_ms"], *row["batch_ms_min_max"],
        "%.4f" % row["batch_gather_form_ms"] if "batch_gather_form_ms" in row else "-",
        "%.4f" % row["batch_staged_form_ms"] if "batch_staged_form_ms" in row else "-",
        "%.4f [%.4f, %.4f]" % (row["parent_ms"], *row["parent_ms_min_max"]) if "parent_ms" in row else "unmeasured",
        "%.3f" % row["batch_over_parent"] if row["batch_over_parent"] else "-", row["batch_GBps"],
        "%.2f" % row["fraction_of_strip_copy"] if copy_rate else "unmeasured", same), flush=True)
    del src, dst, dst_p
    torch.cuda.empty_cache()
with open(OUT, "w") as f:
    json.dump(results, f, indent=1)
    f.write("\n")
print("wrote", OUT)
