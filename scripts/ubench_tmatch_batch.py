#!/usr/bin/env python3
"""gsh_match_template_batch + gsh_find_best_match_batch and gsh_locate_template_batch against the loop a caller had to
write before them: per frame gs_match_template on device pointers and gs_find_best_match, whose partial maxima come back
through a blocking copy.

    python scripts/ubench_tmatch_batch.py [out.json]   # default profiles/tmatch_batch.json; the log is stdout

Per shape (32 and 256 frames of 1280 x 720, 64 frames of 3840 x 2160; templates 16 x 16, 64 x 64, 128 x 128), in one
process: a warm-up of every form, then ROUNDS rounds with the three forms alternating inside every round, each timed with
stream events around as many back-to-back repetitions as fill WINDOW_MS; the median with min and max kept.
  (a) loop    for f: gs_match_template(img[f], tmpl, map); gs_find_best_match(map)
  (b) batch   gsh_match_template_batch + gsh_find_best_match_batch
  (c) locate  gsh_locate_template_batch
The best points of the three forms are compared; `spread_a` = (max - min) / median of (a)'s rounds is the yardstick for
"not slower": (b) and (c) should not exceed (a) by more than it, and (c) should not exceed (b).

With UB_PARENT=<the grayskull_amd directory of a checkout of the parent commit, built> the one-frame gs_match_template is timed
too, at the shapes of scripts/ubench_tmatch.py: parent, this library, parent again in every round, all in this process; the
two parent series against each other give the parent's own spread ("single_frame" in the JSON)."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import grayskull_amd as gs

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "tmatch_batch.json")
ROUNDS = int(os.environ.get("UB_ROUNDS", "5"))
WINDOW_MS = float(os.environ.get("UB_WINDOW_MS", "150"))
SHAPES = ((32, 1280, 720), (256, 1280, 720), (64, 3840, 2160))
TEMPLATES = (16, 64, 128)
if os.environ.get("UB_TINY"):  # rehearsal of the script itself
    SHAPES, TEMPLATES = ((3, 320, 200),), (16, 64)
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


results = {"device": torch.cuda.get_device_name(0), "library": g.version(), "rounds": ROUNDS,
           "forms": {"loop": "per frame gs_match_template + gs_find_best_match (device pointers, async on; the argmax syncs)",
                     "batch": "gsh_match_template_batch + gsh_find_best_match_batch", "locate": "gsh_locate_template_batch"},
           "rows": []}
for (n, iw, ih) in SHAPES:
    img = torch.empty((n, ih, iw), dtype=torch.uint8, device="cuda")
    g.synth_batch(img, 900 + n)
    for t in TEMPLATES:
        rw, rh = iw - t + 1, ih - t + 1
        tmpl = img[n // 2, ih // 3:ih // 3 + t, iw // 2:iw // 2 + t].contiguous()
        tmpl[::3, ::5] ^= 0x55  # no frame holds it exactly
        maps = torch.empty((n, rh, rw), dtype=torch.uint8, device="cuda")
        one = torch.empty((rh, rw), dtype=torch.uint8, device="cuda")
        best_b, best_c = (torch.zeros((n, 2), dtype=torch.int32, device="cuda") for _ in range(2))
        score_b, score_c = (torch.zeros(n, dtype=torch.uint8, device="cuda") for _ in range(2))
        best_a = np.zeros((n, 2), np.int32)

        def loop():
            for f in range(n):
                g.match_template(img[f], tmpl, one)
                best_a[f] = g.find_best_match(one)

        def batch():
            g.match_template_batch(maps, img, tmpl)
            g.find_best_match_batch(maps, best_b, score_b)

        def locate():
            g.locate_template_batch(img, tmpl, best_c, score_c)

        fns = {"loop": loop, "batch": batch, "locate": locate}
        for fn in fns.values():  # warm-up: code objects, scratch growth
            fn()
        torch.cuda.synchronize()
        # every timed window lasts about WINDOW_MS: a shorter one measures the clock and the scheduler
        reps = {k: max(2, min(200, int(WINDOW_MS / max(timeit(fn, 2), 1e-3)) + 1)) for k, fn in fns.items()}
        r = {k: [] for k in fns}
        for _ in range(ROUNDS):
            for k, fn in fns.items():
                r[k].append(timeit(fn, reps[k]))
        same = bool(np.array_equal(best_a, best_b.cpu().numpy()) and torch.equal(best_b, best_c) and torch.equal(score_b, score_c))
        row = {"frames": n, "iw": iw, "ih": ih, "tw": t, "th": t, "same_points": same, "reps": reps}
        for k, v in r.items():
            row[k + "_ms"] = statistics.median(v)
            row[k + "_ms_min_max"] = [min(v), max(v)]
        row["spread_a"] = (max(r["loop"]) - min(r["loop"])) / row["loop_ms"]
        row["batch_over_loop"] = row["batch_ms"] / row["loop_ms"]
        row["locate_over_loop"] = row["locate_ms"] / row["loop_ms"]
        row["locate_over_batch"] = row["locate_ms"] / row["batch_ms"]
        results["rows"].append(row)
        print("%3d x %dx%d, %3dx%-3d  loop %8.3f ms [%.3f, %.3f]  batch %8.3f [%.3f, %.3f]  locate %8.3f [%.3f, %.3f]  batch/loop %.3f  locate/loop %.3f  "
              "locate/batch %.3f  same points: %s" % (n, iw, ih, t, t, row["loop_ms"], *row["loop_ms_min_max"], row["batch_ms"], *row["batch_ms_min_max"],
                                                       row["locate_ms"], *row["locate_ms_min_max"], row["batch_over_loop"], row["locate_over_loop"],
                                                       row["locate_over_batch"], same), flush=True)
        del maps, one
    del img
    torch.cuda.empty_cache()


def parent_library(pkg_dir):
    """the parent commit's package (a checkout built beside this one), imported under another name, bound to ITS library"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("grayskull_parent", os.path.join(pkg_dir, "__init__.py"), submodule_search_locations=[pkg_dir])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["grayskull_parent"] = mod
    spec.loader.exec_module(mod)
    p = mod.Grayskull(os.path.join(pkg_dir, "libgrayskull_hip.so"))
    p.use_torch_stream()
    p.set_async(True)
    return p


# ---- the single-frame call against the parent commit: the shapes of scripts/ubench_tmatch.py, one frame, gs_match_template on
# device pointers.  Per round: parent, this library, parent again -- the two parent series against each other are the parent's
# own run-to-run spread, the yardstick for "the drop-in call did not get slower".
if os.environ.get("UB_PARENT"):
    par = parent_library(os.environ["UB_PARENT"])
    results["single_frame"] = {"parent_library": par.version(), "what": "gs_match_template, one frame, device pointers; ms, median [min, max] over the rounds",
                               "rows": []}
    for (iw, ih) in ((1280, 720), (3840, 2160)) if not os.environ.get("UB_TINY") else ((320, 200),):
        img = torch.empty((1, ih, iw), dtype=torch.uint8, device="cuda")
        g.synth_batch(img, 4)
        for (tw, th) in ((16, 16), (32, 32), (64, 64), (128, 128), (181, 181), (256, 64)):
            if 50 + tw > iw or 100 + th > ih:  # the rehearsal's small frame
                continue
            tmpl = img[0, 100:100 + th, 50:50 + tw].contiguous()
            tmpl[::3, ::5] ^= 0x55
            out = {k: torch.zeros((ih - th + 1, iw - tw + 1), dtype=torch.uint8, device="cuda") for k in ("parent_a", "new", "parent_b")}
            fns = {"parent_a": lambda: par.match_template(img[0], tmpl, out["parent_a"]), "new": lambda: g.match_template(img[0], tmpl, out["new"]),
                   "parent_b": lambda: par.match_template(img[0], tmpl, out["parent_b"])}
            for fn in fns.values():
                fn()
            torch.cuda.synchronize()
            reps = max(5, min(2000, int(WINDOW_MS / max(timeit(fns["new"], 5), 1e-3)) + 1))
            r = {k: [] for k in fns}
            for _ in range(ROUNDS):
                for k, fn in fns.items():
                    r[k].append(timeit(fn, reps))
            row = {"iw": iw, "ih": ih, "tw": tw, "th": th, "reps": reps, "same_bytes": bool(torch.equal(out["new"], out["parent_a"]))}
            for k, v in r.items():
                row[k + "_ms"] = statistics.median(v)
                row[k + "_ms_min_max"] = [min(v), max(v)]
            pa = r["parent_a"] + r["parent_b"]
            row["parent_spread"] = (max(pa) - min(pa)) / statistics.median(pa)
            row["new_over_parent"] = row["new_ms"] / statistics.median(pa)
            results["single_frame"]["rows"].append(row)
            print("1 x %dx%d, %3dx%-3d  parent %.4f [%.4f, %.4f] / %.4f [%.4f, %.4f]  new %.4f [%.4f, %.4f]  new/parent %.3f  parent spread %.3f  same bytes: %s" % (
                iw, ih, tw, th, row["parent_a_ms"], *row["parent_a_ms_min_max"], row["parent_b_ms"], *row["parent_b_ms_min_max"], row["new_ms"],
                *row["new_ms_min_max"], row["new_over_parent"], row["parent_spread"], row["same_bytes"]), flush=True)
with open(OUT, "w") as f:
    json.dump(results, f, indent=1)
    f.write("\n")
print("wrote", OUT)
