#!/usr/bin/env python3
"""gsh_orb_extract_pyramid_batch_nostdlib against the loop a caller had to write before it -- gsh_orb_extract_pyramid per
frame -- and gsh_pyramid_batch against gsh_downsample_batch level by level.

    python scripts/ubench_orb_pyramid_batch.py [out.json]   # default profiles/orb_pyramid_batch.json; the log is stdout

nkps 2500, threshold 20, 3 levels (nanomagick's values); frames from gsh_synth_batch.  Per shape (32 and 256 x 720p,
64 x 4K, 1 x 720p), in one process: a warm-up of every form, then ROUNDS rounds with the forms alternating inside every
round, each timed with stream events around as many back-to-back repetitions as fill WINDOW_MS; the median with min and
max kept.
  loop     per frame gsh_orb_extract_pyramid: the LIBM flavour, synchronous, keypoints on the host -- the only pyramid
           the library offered, so the two flavours differ (other angles and descriptors, the same corners)
  batch    gsh_orb_extract_pyramid_batch_nostdlib: GS_NO_STDLIB trig, stream-ordered, keypoints stay on the device
  levels3  the pyramid alone: gsh_downsample_batch twice (level 1 from the frames, level 2 from level 1)
  pyramid  the pyramid alone: gsh_pyramid_batch
The keypoint COUNTS of loop and batch are compared (the selection does not depend on the trig), and the level planes of
levels3 and pyramid byte for byte.  UB_TINY=1: the script's own rehearsal on small frames; UB_LIB: another build of the
library; UB_SHAPES=32x1280x720[,...]: these shapes only (a profiler run)."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import grayskull_amd as gs

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "orb_pyramid_batch.json")
ROUNDS = int(os.environ.get("UB_ROUNDS", "5"))
WINDOW_MS = float(os.environ.get("UB_WINDOW_MS", "100"))
NKPS, THR, LEVELS = 2500, 20, 3
SHAPES = ((32, 1280, 720), (256, 1280, 720), (64, 3840, 2160), (1, 1280, 720))  # (frames, w, h)
if os.environ.get("UB_TINY"):  # rehearsal of the script itself
    SHAPES, NKPS = ((3, 203, 171), (1, 160, 128)), 90  # both have three levels: levels3 writes two planes
if os.environ.get("UB_SHAPES"):  # e.g. UB_SHAPES=32x1280x720 for a profiler run of one shape
    SHAPES = tuple(tuple(int(v) for v in s.split("x")) for s in os.environ["UB_SHAPES"].split(","))
g = gs.Grayskull(os.environ["UB_LIB"]) if os.environ.get("UB_LIB") else gs.lib()
g.use_torch_stream()
g.set_async(True)


def timeit(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


results = {"device": torch.cuda.get_device_name(0), "library": g.version(), "rounds": ROUNDS, "nkps": NKPS, "threshold": THR, "levels": LEVELS,
           "forms": {"loop": "gsh_orb_extract_pyramid per frame (libm flavour, synchronous, host keypoints)",
                     "batch": "gsh_orb_extract_pyramid_batch_nostdlib (GS_NO_STDLIB flavour, stream-ordered, device keypoints)",
                     "levels3": "gsh_downsample_batch twice", "pyramid": "gsh_pyramid_batch"},
           "note": "loop and batch are different trig flavours: counts are compared, not records", "rows": []}
for (n, w, h) in SHAPES:
    frames = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
    g.synth_batch(frames, 40)
    nb1 = g.orb_pyramid_buffer_bytes(w, h, LEVELS)
    buf1 = torch.zeros(nb1, dtype=torch.uint8, device="cuda")
    buf = torch.zeros(g.orb_pyramid_batch_buffer_bytes(w, h, LEVELS, n), dtype=torch.uint8, device="cuda")
    kps = torch.zeros((n, NKPS, 12), dtype=torch.int32, device="cuda")
    counts = torch.zeros(n, dtype=torch.int32, device="cuda")
    loop_counts = np.zeros(n, np.int64)
    l1, l2 = n * (w // 2) * (h // 2), n * (w // 4) * (h // 4)
    planes = {f: torch.zeros(l1 + l2, dtype=torch.uint8, device="cuda") for f in ("levels3", "pyramid")}

    def loop():
        for f in range(n):
            loop_counts[f] = len(g.orb_extract_pyramid_dev(frames[f], buf1, NKPS, THR, LEVELS))

    def batch():
        g.orb_extract_pyramid_batch_nostdlib(frames, buf, kps, counts, NKPS, THR, LEVELS)

    def levels3():
        p = planes["levels3"]
        a = p[:l1].view(n, h // 2, w // 2)
        g.downsample_batch(a, frames)
        g.downsample_batch(p[l1:].view(n, h // 4, w // 4), a)

    def pyramid():
        g.pyramid_batch(planes["pyramid"], frames, LEVELS)

    fns = {"loop": loop, "batch": batch, "levels3": levels3, "pyramid": pyramid}
    for fn in fns.values():  # warm-up: code objects, scratch growth
        fn()
    torch.cuda.synchronize()
    reps = {k: max(2, min(500, int(WINDOW_MS / max(timeit(fn, 2), 1e-3)) + 1)) for k, fn in fns.items()}
    r = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            r[k].append(timeit(fn, reps[k]))
    bc = counts.cpu().numpy()
    row = {"frames": n, "w": w, "h": h, "reps": reps, "keypoints_batch": int(bc.sum()), "keypoints_loop": int(loop_counts.sum()),
           "same_counts": bool(np.array_equal(bc, loop_counts)), "same_planes": bool(torch.equal(planes["levels3"], planes["pyramid"]))}
    for k, v in r.items():
        row[k + "_ms"] = statistics.median(v)
        row[k + "_ms_min_max"] = [min(v), max(v)]
    row["batch_us_per_frame"] = 1e3 * row["batch_ms"] / n
    row["loop_us_per_frame"] = 1e3 * row["loop_ms"] / n
    row["batch_over_loop"] = row["batch_ms"] / row["loop_ms"]
    row["pyramid_over_levels3"] = row["pyramid_ms"] / row["levels3_ms"]
    row["pyramid_GB_s"] = n * w * h * (1 + 1 / 4 + 1 / 16) / row["pyramid_ms"] / 1e6
    results["rows"].append(row)
    print("%3d x %dx%d  loop %9.4f ms [%.4f, %.4f]  batch %8.4f [%.4f, %.4f]  batch/loop %.4f  %.2f us/frame | levels3 %.4f [%.4f, %.4f]  "
          "pyramid %.4f [%.4f, %.4f]  pyramid/levels3 %.3f  %.0f GB/s | keypoints %d / %d  same counts: %s  same planes: %s" % (
              n, w, h, row["loop_ms"], *row["loop_ms_min_max"], row["batch_ms"], *row["batch_ms_min_max"], row["batch_over_loop"],
              row["batch_us_per_frame"], row["levels3_ms"], *row["levels3_ms_min_max"], row["pyramid_ms"], *row["pyramid_ms_min_max"],
              row["pyramid_over_levels3"], row["pyramid_GB_s"], row["keypoints_loop"], row["keypoints_batch"], row["same_counts"],
              row["same_planes"]), flush=True)
    del frames, buf, buf1, kps, planes
    torch.cuda.empty_cache()
print("(loop is the libm flavour, batch the GS_NO_STDLIB flavour: the flavours differ in angles and descriptors, not in corners)")
with open(OUT, "w") as f:
    json.dump(results, f, indent=1)
    f.write("\n")
print("wrote", OUT)
