#!/usr/bin/env python3
"""gsh_orb_extract_pyramid_batch (pyramid ORB of the reference's default build, glibc trig on the host, keypoints on the
device) against the loop it replaces -- gsh_orb_extract_pyramid per frame -- with the GS_NO_STDLIB batch entry beside them
for what the host trig costs, and gsbatch's `orb` verb on 64 720p files against another build of the driver.

    python scripts/ubench_orb_pyramid_libm.py [out.json]   # default profiles/orb_pyramid_libm_batch.json; the log is stdout

nkps 2500, threshold 20, 3 levels (nanomagick's values); frames from gsh_synth_batch.  Per shape (1, 32 and 256 x 720p,
64 x 4K), in one process: a warm-up of every form, then ROUNDS rounds with the forms alternating inside every round, each
timed with a host clock round as many back-to-back repetitions as fill WINDOW_MS, ending in a device synchronise; the
median with min and max kept.
  loop     per frame gsh_orb_extract_pyramid: synchronous, four host round trips per frame, keypoints on the host
  batch    gsh_orb_extract_pyramid_batch: the same flavour, one round trip per call, keypoints stay on the device
  nostdlib gsh_orb_extract_pyramid_batch_nostdlib: the other flavour, no round trip at all
The keypoint records of loop and batch are compared.  Then, in rounds of their own under gsh_profile(1), the split of the
batch call (gsh_orb_pyramid_batch_times): device work before the round trip, copy down, host trig, copy up, device work
after.
GSBATCH_OLD=<path to another build's gsbatch>: `gsbatch -v orb` on 64 generated 720p files, ROUNDS alternating runs of that
binary and of this tree's, wall time and the `stages` and `write` figures of -v.  UB_TINY=1: the script's own rehearsal on small frames;
UB_LIB: another build of the library."""
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import grayskull_amd as gs

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "orb_pyramid_libm_batch.json")
ROUNDS = int(os.environ.get("UB_ROUNDS", "5"))
WINDOW_MS = float(os.environ.get("UB_WINDOW_MS", "100"))
NKPS, THR, LEVELS = 2500, 20, 3
SHAPES = ((1, 1280, 720), (32, 1280, 720), (256, 1280, 720), (64, 3840, 2160))  # (frames, w, h)
FILES, FW, FH = 64, 1280, 720
if os.environ.get("UB_TINY"):  # rehearsal of the script itself
    SHAPES, NKPS, FILES, FW, FH = ((3, 203, 171), (1, 160, 128)), 90, 3, 203, 171
g = gs.Grayskull(os.environ["UB_LIB"]) if os.environ.get("UB_LIB") else gs.lib()
g.use_torch_stream()
g.set_async(True)


def timeit(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / reps


results = {"device": torch.cuda.get_device_name(0), "library": g.version(), "rounds": ROUNDS, "nkps": NKPS, "threshold": THR, "levels": LEVELS,
           "forms": {"loop": "gsh_orb_extract_pyramid per frame (libm flavour, synchronous, host keypoints)",
                     "batch": "gsh_orb_extract_pyramid_batch (libm flavour, one round trip per call, device keypoints)",
                     "nostdlib": "gsh_orb_extract_pyramid_batch_nostdlib (GS_NO_STDLIB flavour, no round trip)"},
           "split": ["device_before", "copy_down", "host_trig", "copy_up", "device_after"], "rows": []}
for (n, w, h) in SHAPES:
    frames = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
    g.synth_batch(frames, 40)
    buf1 = torch.zeros(g.orb_pyramid_buffer_bytes(w, h, LEVELS), dtype=torch.uint8, device="cuda")
    buf = torch.zeros(g.orb_pyramid_batch_buffer_bytes(w, h, LEVELS, n), dtype=torch.uint8, device="cuda")
    kps = torch.zeros((n, NKPS, 12), dtype=torch.int32, device="cuda")
    counts = torch.zeros(n, dtype=torch.int32, device="cuda")
    loop_kps = [None] * n

    def loop():
        for f in range(n):
            loop_kps[f] = g.orb_extract_pyramid_dev(frames[f], buf1, NKPS, THR, LEVELS)

    def batch():
        g.orb_extract_pyramid_batch(frames, buf, kps, counts, NKPS, THR, LEVELS)

    def nostdlib():
        g.orb_extract_pyramid_batch_nostdlib(frames, buf, kps, counts, NKPS, THR, LEVELS)

    fns = {"loop": loop, "nostdlib": nostdlib, "batch": batch}  # batch last: its records are the ones compared
    for fn in fns.values():  # warm-up: code objects, scratch growth
        fn()
    torch.cuda.synchronize()
    reps = {k: max(2, min(500, int(WINDOW_MS / max(timeit(fn, 2), 1e-3)) + 1)) for k, fn in fns.items()}
    r = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            r[k].append(timeit(fn, reps[k]))
    bc, bk = counts.cpu().numpy(), kps.cpu().numpy()
    same = all(int(bc[f]) == len(loop_kps[f]) and bk[f, :bc[f]].tobytes() == loop_kps[f].tobytes() for f in range(n))
    g.profile(True)
    split = []
    for _ in range(ROUNDS):
        batch()
        split.append(g.orb_pyramid_batch_times())
    g.profile(False)
    row = {"frames": n, "w": w, "h": h, "reps": reps, "keypoints": int(bc.sum()), "batch_equals_loop": bool(same),
           "split_ms": [statistics.median(s[i] for s in split) for i in range(5)]}
    for k, v in r.items():
        row[k + "_ms"] = statistics.median(v)
        row[k + "_ms_min_max"] = [min(v), max(v)]
    row["batch_over_loop"] = row["batch_ms"] / row["loop_ms"]
    row["batch_minus_nostdlib_ms"] = row["batch_ms"] - row["nostdlib_ms"]
    row["faster_beyond_spread"] = bool(max(r["batch"]) < min(r["loop"]))
    results["rows"].append(row)
    print("%3d x %dx%d  loop %9.4f ms [%.4f, %.4f]  batch %8.4f [%.4f, %.4f]  nostdlib %8.4f [%.4f, %.4f]  batch/loop %.4f  beyond the spread: %s | "
          "split: before %.4f  down %.4f  host %.4f  up %.4f  after %.4f | keypoints %d  batch == loop: %s" % (
              n, w, h, row["loop_ms"], *row["loop_ms_min_max"], row["batch_ms"], *row["batch_ms_min_max"], row["nostdlib_ms"],
              *row["nostdlib_ms_min_max"], row["batch_over_loop"], row["faster_beyond_spread"], *row["split_ms"], row["keypoints"], same), flush=True)
    del frames, buf, buf1, kps
    torch.cuda.empty_cache()

# ---- gsbatch orb on files: another build's driver against this tree's, alternating ------------------------------------------
old = os.environ.get("GSBATCH_OLD")
if old:
    new = os.path.join(ROOT, "grayskull_amd", "gsbatch")
    with tempfile.TemporaryDirectory() as tmp:
        frames = torch.empty((FILES + 1, FH, FW), dtype=torch.uint8, device="cuda")
        g.synth_batch(frames, 77)
        imgs = frames.cpu().numpy()
        imgs[:, 0, 0] = np.maximum(imgs[:, 0, 0], 33)  # no leading whitespace byte (the reference's reader)
        paths = []
        for i, a in enumerate(imgs):
            paths.append(os.path.join(tmp, "f%02d.pgm" % i))
            with open(paths[-1], "wb") as f:
                f.write(b"P5\n%d %d\n255\n" % (FW, FH) + a.tobytes())
        template, files = paths[0], paths[1:]
        runs = {"old": [], "new": []}
        digests = {}
        for rnd in range(ROUNDS + 1):  # round 0: warm-up of both (file cache, code objects)
            for name, exe in (("old", old), ("new", new)):
                out = os.path.join(tmp, "out_%s_%d" % (name, rnd))
                os.mkdir(out)
                t0 = time.perf_counter()
                p = subprocess.run([exe, "-v", "-o", out, "orb", template, "--", *files], capture_output=True)
                wall = 1e3 * (time.perf_counter() - t0)
                err = p.stderr.decode()
                m = re.search(r"stages ([0-9.]+) ms, download ([0-9.]+) ms, write ([0-9.]+) ms", err)
                stages, write = float(m.group(1)), float(m.group(3))
                listing = sorted(os.listdir(out))
                digests[name] = [(f, open(os.path.join(out, f), "rb").read()) for f in listing]
                if rnd:
                    runs[name].append((wall, stages, write))
        row = {"files": FILES, "w": FW, "h": FH, "old": "the driver and library of the parent commit", "new": "this tree's",
               "note": "the old driver runs the verb file by file inside its `write` phase, the new one per slice inside `stages`",
               "same_output_files": digests["old"] == digests["new"],
               "output_files": len(digests["new"])}
        for name, v in runs.items():
            row[name + "_wall_ms"] = statistics.median(x[0] for x in v)
            row[name + "_wall_ms_min_max"] = [min(x[0] for x in v), max(x[0] for x in v)]
            row[name + "_stages_ms"] = statistics.median(x[1] for x in v)
            row[name + "_stages_ms_min_max"] = [min(x[1] for x in v), max(x[1] for x in v)]
            row[name + "_write_ms"] = statistics.median(x[2] for x in v)
        results["gsbatch_orb"] = row
        print("gsbatch orb, %d x %dx%d files: wall old %.1f ms [%.1f, %.1f]  new %.1f [%.1f, %.1f] | stages old %.2f [%.2f, %.2f]  new %.2f [%.2f, %.2f] | "
              "write old %.1f  new %.1f | %d output files, identical: %s" % (FILES, FW, FH, row["old_wall_ms"], *row["old_wall_ms_min_max"], row["new_wall_ms"],
                                                  *row["new_wall_ms_min_max"], row["old_stages_ms"], *row["old_stages_ms_min_max"],
                                                  row["new_stages_ms"], *row["new_stages_ms_min_max"], row["old_write_ms"], row["new_write_ms"], row["output_files"], row["same_output_files"]))
with open(OUT, "w") as f:
    json.dump(results, f, indent=1)
    f.write("\n")
print("wrote", OUT)
