#!/usr/bin/env python3
"""gsh_locate_template_windows_batch against what a caller had before it, on device-side search rectangles.

    python scripts/ubench_tmatch_windows.py [out.json]   # default profiles/tmatch_windows.json; the log is stdout

Per shape, in one process, on the same seeded inputs: the points of all forms are compared, every form is warmed up, then
ROUNDS rounds with the forms alternating inside every round, each timed with stream events around as many back-to-back
repetitions as fill WINDOW_MS; the median with min and max kept, and the raw rounds.
  (a) loop     download the rectangles, then per window gsh_crop_batch (n = 1) + gsh_locate_template_batch
  (b) patches  gsh_crop_resize_batch(nearest) at the windows' size + gsh_locate_template_batch(ntmpl == n); equal-sized windows only
  (c) windows  gsh_locate_template_windows_batch
  (d) frames   the whole-frame gsh_locate_template_batch (one template): what tracking without windows costs; context only,
               its points are other points
`spread` = the largest (max - min) / median among the rounds of (a), (b) and (c) is the yardstick: (c) has to be faster than
(a) by more than it, and not slower than (b) beyond it.
Multiply-adds per second of (c): positions x taps of every window over its time -- the whole call, launches and the key
pass included, so a lower bound of the kernel's -- against the v_dot4_u32_u8 issue bound of the chip: CUs x 4 SIMDs x 32
lanes a cycle x 4 products x 2.4 GHz.  The kernel issues two v_dot4 per four products that count (I.T and I.I), so half the
bound is the most it can reach."""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import grayskull_amd as gs

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "tmatch_windows.json")
ROUNDS = int(os.environ.get("UB_ROUNDS", "5"))
WINDOW_MS = float(os.environ.get("UB_WINDOW_MS", "150"))
# (frames, iw, ih, windows per frame, window side, template side, a template per window)
SHAPES = ((256, 1280, 720, 1, 96, 32, False), (32, 1280, 720, 64, 64, 16, True), (64, 3840, 2160, 16, 192, 64, False), (1, 1280, 720, 1, 96, 32, False))
if os.environ.get("UB_TINY"):  # rehearsal of the script itself
    SHAPES = ((3, 320, 200, 2, 48, 16, True), (1, 320, 200, 1, 64, 16, False))
g = gs.Grayskull(os.environ["UB_LIB"]) if os.environ.get("UB_LIB") else gs.lib()
g.use_torch_stream()
g.set_async(True)


def commit():
    if os.environ.get("UB_COMMIT"):
        return os.environ["UB_COMMIT"]
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except (OSError, subprocess.CalledProcessError):
        return "unknown"


def timeit(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


props = torch.cuda.get_device_properties(0)
DOT4_BOUND = props.multi_processor_count * 4 * 32 * 4 * 2.4e9
results = {"device": torch.cuda.get_device_name(0), "library": g.version(), "commit": commit(), "rounds": ROUNDS,
           "dot4_issue_bound_mac_per_s": DOT4_BOUND,
           "forms": {"loop": "download the rectangles; per window gsh_crop_batch (n = 1) + gsh_locate_template_batch",
                     "patches": "gsh_crop_resize_batch(nearest) + gsh_locate_template_batch(ntmpl == n)",
                     "windows": "gsh_locate_template_windows_batch", "frames": "whole-frame gsh_locate_template_batch, one template (context)"},
           "rows": []}
for (n, iw, ih, per, ws, t, per_window) in SHAPES:
    nwin = n * per
    img = torch.empty((n, ih, iw), dtype=torch.uint8, device="cuda")
    g.synth_batch(img, 700 + n)
    rng = np.random.default_rng(nwin)
    windows_h = np.stack([rng.integers(0, iw - ws + 1, nwin), rng.integers(0, ih - ws + 1, nwin), np.full(nwin, ws), np.full(nwin, ws)], 1).astype(np.int32)
    frame_of_h = np.repeat(np.arange(n, dtype=np.int32), per)
    windows, frame_of = torch.from_numpy(windows_h).cuda(), torch.from_numpy(frame_of_h).cuda()
    ntmpl = nwin if per_window else 1
    tmpl = torch.empty((ntmpl, t, t), dtype=torch.uint8, device="cuda")
    for p in range(ntmpl):  # cut from inside window p of its frame, then disturbed: no window holds it exactly
        x, y, f = int(windows_h[p, 0]) + (ws - t) // 3, int(windows_h[p, 1]) + (ws - t) // 2, int(frame_of_h[p])
        tmpl[p] = img[f, y:y + t, x:x + t]
    tmpl[:, ::3, ::5] ^= 0x55
    tm = tmpl if per_window else tmpl[0].contiguous()
    patch = torch.empty((1, ws, ws), dtype=torch.uint8, device="cuda")
    patches = torch.empty((nwin, ws, ws), dtype=torch.uint8, device="cuda")
    best = {k: torch.zeros((nwin, 2), dtype=torch.int32, device="cuda") for k in ("loop", "patches", "windows")}
    score = {k: torch.zeros(nwin, dtype=torch.uint8, device="cuda") for k in best}
    best_d, score_d = torch.zeros((n, 2), dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")

    def loop():
        wh = windows.cpu().numpy()  # the round trip
        fh = frame_of.cpu().numpy()
        for p in range(nwin):
            x, y, w, h = (int(v) for v in wh[p])
            f = int(fh[p])
            g.crop_batch(patch, img[f:f + 1], x, y, w, h)
            g.locate_template_batch(patch, tm[p] if per_window else tm, best["loop"][p:p + 1], score["loop"][p:p + 1])

    def by_patches():
        g.crop_resize_batch(patches, img, windows, frame_of, nearest=True)
        g.locate_template_batch(patches, tmpl if per_window else tm, best["patches"], score["patches"])

    def by_windows():
        g.locate_template_windows_batch(img, tm, windows, (ws, ws), best["windows"], score["windows"], frame_of)

    def whole_frames():
        g.locate_template_batch(img, tmpl[0].contiguous(), best_d, score_d)

    fns = {"loop": loop, "patches": by_patches, "windows": by_windows, "frames": whole_frames}
    for fn in fns.values():  # warm-up: code objects, scratch growth
        fn()
    torch.cuda.synchronize()
    origin = windows[:, :2]
    same = bool(torch.equal(best["loop"] + origin, best["windows"]) and torch.equal(best["patches"] + origin, best["windows"]) and
                torch.equal(score["loop"], score["windows"]) and torch.equal(score["patches"], score["windows"]))
    # every timed window lasts about WINDOW_MS: a shorter one measures the clock and the scheduler
    reps = {k: max(2, min(2000, int(WINDOW_MS / max(timeit(fn, 2), 1e-3)) + 1)) for k, fn in fns.items()}
    r = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            r[k].append(timeit(fn, reps[k]))
    macs = float(nwin) * (ws - t + 1) ** 2 * t * t
    row = {"frames": n, "iw": iw, "ih": ih, "windows": nwin, "ww": ws, "wh": ws, "tw": t, "th": t, "ntmpl": ntmpl, "same_points": same, "reps": reps,
           "multiply_adds": macs}
    for k, v in r.items():
        row[k + "_ms"] = statistics.median(v)
        row[k + "_ms_min_max"] = [min(v), max(v)]
        row[k + "_ms_rounds"] = v
    row["spread"] = max((max(r[k]) - min(r[k])) / row[k + "_ms"] for k in ("loop", "patches", "windows"))
    row["windows_over_loop"] = row["windows_ms"] / row["loop_ms"]
    row["windows_over_patches"] = row["windows_ms"] / row["patches_ms"]
    row["windows_over_frames"] = row["windows_ms"] / row["frames_ms"]
    row["windows_mac_per_s"] = macs / (row["windows_ms"] * 1e-3)
    row["windows_of_dot4_bound"] = row["windows_mac_per_s"] / DOT4_BOUND
    row["faster_than_loop"] = bool(max(r["windows"]) < min(r["loop"]) and row["windows_over_loop"] < 1 - row["spread"])
    row["not_slower_than_patches"] = bool(row["windows_over_patches"] <= 1 + row["spread"])
    results["rows"].append(row)
    print("%3d x %dx%d, %4d windows %dx%d, %dx%d (%d templates)  loop %9.3f ms [%.3f, %.3f]  patches %8.4f [%.4f, %.4f]  windows %8.4f [%.4f, %.4f]  "
          "frames %8.4f [%.4f, %.4f]  windows/loop %.4f  windows/patches %.3f  spread %.3f  %.2f TMAC/s = %.3f of the dot4 bound  same points: %s" % (
              n, iw, ih, nwin, ws, ws, t, t, ntmpl, row["loop_ms"], *row["loop_ms_min_max"], row["patches_ms"], *row["patches_ms_min_max"],
              row["windows_ms"], *row["windows_ms_min_max"], row["frames_ms"], *row["frames_ms_min_max"], row["windows_over_loop"],
              row["windows_over_patches"], row["spread"], row["windows_mac_per_s"] / 1e12, row["windows_of_dot4_bound"], same), flush=True)
    del img, patches
    torch.cuda.empty_cache()
with open(OUT, "w") as f:
    json.dump(results, f, indent=1)
    f.write("\n")
print("wrote", OUT)
