#!/usr/bin/env python3
"""gsh_trace_contours_batch on 64 x 3840x2160 frames in three input families: one frame-filling disc per frame (one
long contour), x3-upscaled noise through blobs_batch(cap 1000) -> blob_contour_starts_batch -> trace_contours_batch,
and 64 small discs per frame.  Per family: moves and tile reloads per frame (counted on the host from the walk's
path), microseconds per frame in the batch (device events round the call, median of the repetitions, `visited` cleared
outside the timed region), nanoseconds per move, one frame alone through the drop-in gs_trace_contour on device
pointers (wall clock), and the reference on one CPU thread for the same calls (oracle/_ref/libgs_ref.so; only walks
the restatement has shown to end -- the reference does not return from the others).  The distinct frames of every
timed batch are compared with the reference's results.  Writes one JSON file (--out) and prints it.
CONTOURS_FRAMES / CONTOURS_REPS override the batch size / timed repetitions."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import grayskull_amd as gs  # noqa: E402
import contour_cases as cc  # noqa: E402
from grayskull_amd import CONTOUR_DTYPE  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contours_bench.json"))
args = ap.parse_args()

g = gs.lib()
g.use_torch_stream()
n, h, w = int(os.environ.get("CONTOURS_FRAMES", 64)), 2160, 3840
reps = int(os.environ.get("CONTOURS_REPS", 21))
DISTINCT = 2  # distinct frames per family; the batch repeats them
rng = np.random.default_rng(77)
ref = cc.Ref()


def median_us(fn, clear):
    ts = []
    for i in range(reps + 2):
        clear()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if i >= 2:
            ts.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(ts))


def host_side(img, starts):
    """reference results of one frame (ended walks by the compiled reference, endless by the restatement), moves, tile
    reloads and the reference's CPU time for the ended walks"""
    want, want_vis, endless = cc.expected_sequence(img, starts, ref=ref)
    moves = reloads = 0
    origin = None
    ended = [s for s, r in zip(starts, want) if r[2] == cc.ENDED]
    for s in ended:  # moves and tile reloads of the walks that end
        r, m, origin = cc.tile_reloads(img, s, origin=origin)
        moves, reloads = moves + m, reloads + r
    if endless:  # the timed batch walks these too: their moves up to the first repeated state (the kernel makes up to ~4x that)
        tr, scratch = cc.Tracer(img), np.zeros(img.shape, np.uint8)
        moves += sum(tr.trace(scratch, s)[3] for s, r in zip(starts, want) if r[2] != cc.ENDED)
    vis = np.zeros(img.shape, np.uint8)
    t0 = time.perf_counter()
    for s in ended:
        ref.trace(img, vis, s, status=cc.ENDED)
    cpu_us = (time.perf_counter() - t0) * 1e6
    return want, want_vis, endless, moves, reloads, cpu_us


def run_family(name, frames, starts=None, cap=None):
    """frames: DISTINCT numpy frames.  starts given: traced as they are; else through the blob chain with `cap`"""
    batch = torch.from_numpy(np.stack([frames[f % DISTINCT] for f in range(n)])).cuda()
    vis = torch.zeros_like(batch)
    if starts is None:
        lab = torch.zeros(batch.shape, dtype=torch.int16, device="cuda")
        blobs = torch.zeros((n, cap, 8), dtype=torch.int32, device="cuda")
        counts = torch.zeros(n, dtype=torch.int32, device="cuda")
        g.blobs_batch(batch, lab, blobs, counts, cap)
        cont = torch.zeros((n, cap, 7), dtype=torch.int32, device="cuda")
        us_starts = median_us(lambda: g.blob_contour_starts_batch(lab, blobs, counts, cont), lambda: None)
        torch.cuda.synchronize()
        recs = cont.cpu().numpy().view(CONTOUR_DTYPE).reshape(n, cap)
        cnt = counts.cpu().numpy()
        starts = [[(int(r["sx"]), int(r["sy"])) for r in recs[f, :cnt[f]]] for f in range(DISTINCT)]
    else:
        us_starts = None
        per = max(len(s) for s in starts)
        recs = np.zeros((n, per), CONTOUR_DTYPE)
        for f in range(n):
            for k, s in enumerate(starts[f % DISTINCT]):
                recs[f, k]["sx"], recs[f, k]["sy"] = s
        cont = torch.from_numpy(recs.view(np.int32).reshape(n, per, 7)).cuda()
        counts = torch.tensor([len(starts[f % DISTINCT]) for f in range(n)], dtype=torch.int32, device="cuda")
    st = torch.zeros((n, cont.shape[1]), dtype=torch.uint8, device="cuda")
    us = median_us(lambda: g.trace_contours_batch(batch, vis, cont, counts, st), lambda: vis.zero_())
    got = cont.cpu().numpy().view(CONTOUR_DTYPE).reshape(n, -1)
    gvis, gst = vis.cpu().numpy(), st.cpu().numpy()
    moves = reloads = endless = 0
    cpu_us = 0.0
    for f in range(DISTINCT):
        want, want_vis, e, m, r, c = host_side(frames[f], starts[f])
        for ff in range(f, n, DISTINCT):  # every timed frame: the distinct ones against the reference, the repeats alike
            cc.assert_sequence_equal([cc.rec_tuple(x) for x in got[ff, :len(want)]], gvis[ff], want, want_vis,
                                     "%s frame %d" % (name, ff), got_status=gst[ff])
        moves, reloads, endless, cpu_us = moves + m, reloads + r, endless + e, cpu_us + c
    # one frame alone through the drop-in on device pointers (wall clock, synchronised)
    one, ovis = batch[0].contiguous(), torch.zeros_like(batch[0])
    walls = []
    for i in range(7):
        ovis.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for s in starts[0]:
            g.trace_contour(one, ovis, s)
        walls.append((time.perf_counter() - t0) * 1e6)
    return {"family": name, "frames": n, "contours_per_frame": sum(len(s) for s in starts) / DISTINCT,
            "endless_per_frame": endless / DISTINCT, "moves_per_frame": moves / DISTINCT, "tile_reloads_per_frame": reloads / DISTINCT,
            "batch_us_per_frame": us / n, "batch_ns_per_move": us * 1e3 / (n * moves / DISTINCT) if moves else None,
            "batch_us_total": us, "starts_us_per_frame": None if us_starts is None else us_starts / n,
            "single_frame_dropin_us": float(np.median(walls)), "reference_cpu_us_per_frame": cpu_us / DISTINCT}


rows = []
big = [cc.discs(h, w, [(w // 2 + 3 * f, h // 2 - 2 * f, 1000 + 10 * f)]) for f in range(DISTINCT)]
rows.append(run_family("one_disc_r1000", big, starts=[cc.start_pixels(b)[:1] for b in big]))
noise = [cc.upscaled_noise(rng, h, w, 3) for _ in range(DISTINCT)]
rows.append(run_family("noise_x3_chain_cap1000", noise, cap=1000))
small = [cc.disc_grid(h, w, 8, 8, 20 + 4 * f) for f in range(DISTINCT)]
# the raster-first pixel of the disc (cx, cy, r) is the one pixel of its top row: (cx, cy - r)
tops = [[(cx, cy - (20 + 4 * f)) for cx, cy in cc.disc_grid_centres(h, w, 8, 8)] for f in range(DISTINCT)]
assert all(small[f][y, x] and not small[f][y - 1, x] and not small[f][y, x - 1] for f in range(DISTINCT) for x, y in tops[f])
rows.append(run_family("64_discs", small, starts=tops))
out = {"device": torch.cuda.get_device_name(0), "library": g.version(), "reps": reps, "rows": rows}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(out))
