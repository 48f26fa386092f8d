#!/usr/bin/env python3
"""gsh_match_templates_batch / gsh_locate_templates_batch against the loop a caller wrote before them: per template
gsh_match_template_batch / gsh_locate_template_batch with ntmpl = 1, in the same process (their code is the parent's).

    python scripts/ubench_tmatch_bank.py [out.json]   # default profiles/tmatch_bank.json; the log is stdout

Per shape, in one process: a warm-up of every form, then ROUNDS rounds with the forms alternating inside every round, each
timed with stream events around as many back-to-back repetitions as fill WINDOW_MS; the median with min and max kept.
  loop_maps    for t: gsh_match_template_batch(img, tmpl[t]) -> maps[t]           (m, n, rh, rw)
  bank_maps    gsh_match_templates_batch under key 27 = 2 (k_match_bank_mfma)     (n, m, rh, rw)
  entry_maps   gsh_match_templates_batch under key 27 = 1 (the entry's own loop: window sums computed once)
  loop_locate / bank_locate / entry_locate   the same three with gsh_locate_template(s)_batch
Every timed result is compared with the loop's bytes.  `spread` = (max - min) / median of the loop's rounds is the yardstick:
the rule sends a shape to the bank kernel only where bank < loop (1 - spread).
`useful_tops` = 2 n rw rh m tw th / time of the bank kernel's form; `issued_tops` counts what the matrix cores are given (rows
padded to 16 taps, an even number of slots a band, templates to groups of 32 or 64) -- to hold against the issue rate that
scripts/ubench_src/ubench_mfma_i8.cpp measures on the same box (UB_MFMA_TOPS, recorded in the JSON)."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import grayskull_amd as gs

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "tmatch_bank.json")
ROUNDS = int(os.environ.get("UB_ROUNDS", "5"))
WINDOW_MS = float(os.environ.get("UB_WINDOW_MS", "100"))
# (frames, iw, ih, m, t)
SHAPES = [(32, 1280, 720, m, 16) for m in (16, 64, 256)] + [(32, 1280, 720, m, 32) for m in (16, 64)] + [
    (32, 1280, 720, 32, 64), (8, 3840, 2160, 64, 32), (1, 1280, 720, 64, 16)] + [(32, 1280, 720, m, t) for t in (16, 32) for m in (1, 2, 4, 8)]
if os.environ.get("UB_TINY"):  # rehearsal of the script itself
    SHAPES = [(2, 160, 100, 5, 16), (1, 160, 100, 2, 32)]
if os.environ.get("UB_ONLY"):  # "a:b": a slice of the list, for a run split over several calls
    lo, hi = (int(x) if x else None for x in os.environ["UB_ONLY"].split(":"))
    SHAPES = SHAPES[lo:hi]
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


def issued_taps(t, m):
    spr = (t + 15) // 16
    band = max(1, 32 // spr)
    band = min(band & ~1 if band >= 2 else band, t)
    full, rest = divmod(t, band)
    slots = full * ((band * spr + 1) & ~1) + (((rest * spr + 1) & ~1) if rest else 0)
    group = 64 if m > 32 else 32
    return 16 * slots * ((m + group - 1) // group) * group


results = {"device": torch.cuda.get_device_name(0), "library": g.version(), "rounds": ROUNDS,
           "mfma_i8_issue_tops": float(os.environ.get("UB_MFMA_TOPS", "0")) or None, "rows": []}
if os.path.exists(OUT) and os.environ.get("UB_ONLY"):  # a later slice of the same run
    results["rows"] = json.load(open(OUT))["rows"]
for (n, iw, ih, m, t) in SHAPES:
    rw, rh = iw - t + 1, ih - t + 1
    img = torch.empty((n, ih, iw), dtype=torch.uint8, device="cuda")
    g.synth_batch(img, 900 + n)
    ys = np.random.default_rng(m).integers(0, rh, m)
    xs = np.random.default_rng(m + 1).integers(0, rw, m)
    bank = torch.stack([img[k % n, y:y + t, x:x + t] for k, (x, y) in enumerate(zip(xs, ys))]).contiguous()
    bank[:, ::3, ::5] ^= 0x55  # no frame holds them exactly
    maps_l = torch.empty((m, n, rh, rw), dtype=torch.uint8, device="cuda")
    maps_b = torch.empty((n, m, rh, rw), dtype=torch.uint8, device="cuda")
    best_l, score_l = torch.zeros((m, n, 2), dtype=torch.int32, device="cuda"), torch.zeros((m, n), dtype=torch.uint8, device="cuda")
    best_b, score_b = torch.zeros((n, m, 2), dtype=torch.int32, device="cuda"), torch.zeros((n, m), dtype=torch.uint8, device="cuda")
    winner = torch.zeros(n, dtype=torch.int32, device="cuda")

    def loop_maps():
        for k in range(m):
            g.match_template_batch(maps_l[k], img, bank[k])

    def loop_locate():
        for k in range(m):
            g.locate_template_batch(img, bank[k], best_l[k], score_l[k])

    def keyed(key27, fn):
        def f():
            g.tune(27, key27)
            fn()
            g.tune(27, 0)
        return f

    def entry_maps():
        g.match_templates_batch(maps_b, img, bank)

    def entry_locate():
        g.locate_templates_batch(img, bank, best_b, score_b, winner)

    def same_maps():
        return all(torch.equal(maps_b[:, k], maps_l[k]) for k in range(m))

    def same_points():
        return bool(torch.equal(best_b, best_l.permute(1, 0, 2)) and torch.equal(score_b, score_l.permute(1, 0)))

    fns = {"loop_maps": loop_maps, "bank_maps": keyed(2, entry_maps), "entry_maps": keyed(1, entry_maps),
           "loop_locate": loop_locate, "bank_locate": keyed(2, entry_locate), "entry_locate": keyed(1, entry_locate)}
    same = {}
    for k, fn in fns.items():  # warm-up (code objects, scratch growth) and the comparison with the loop's bytes
        maps_b.fill_(0x5A), best_b.fill_(0x5A5A5A5A), score_b.fill_(0x5A)
        fn()
        torch.cuda.synchronize()
        if k.endswith("maps") and k != "loop_maps":
            same[k] = same_maps()
        if k.endswith("locate") and k != "loop_locate":
            same[k] = same_points()
    reps = {k: max(2, min(200, int(WINDOW_MS / max(timeit(fn, 2), 1e-3)) + 1)) for k, fn in fns.items()}
    r = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            r[k].append(timeit(fn, reps[k]))
    row = {"frames": n, "iw": iw, "ih": ih, "m": m, "tw": t, "th": t, "same_bytes": same, "reps": reps}
    for k, v in r.items():
        row[k + "_ms"] = statistics.median(v)
        row[k + "_ms_min_max"] = [min(v), max(v)]
    for what in ("maps", "locate"):
        lo = r["loop_" + what]
        row["spread_loop_" + what] = (max(lo) - min(lo)) / row["loop_%s_ms" % what]
        row["bank_over_loop_" + what] = row["bank_%s_ms" % what] / row["loop_%s_ms" % what]
        row["entry_over_loop_" + what] = row["entry_%s_ms" % what] / row["loop_%s_ms" % what]
        row["bank_pays_" + what] = bool(row["bank_over_loop_" + what] < 1 - row["spread_loop_" + what])
        row["useful_tops_" + what] = 2.0 * n * rw * rh * m * t * t / (row["bank_%s_ms" % what] * 1e-3) / 1e12
        row["issued_tops_" + what] = 2.0 * n * (-(-rw // 64) * 64) * (-(-rh // 8) * 8) * issued_taps(t, m) / (row["bank_%s_ms" % what] * 1e-3) / 1e12
    results["rows"].append(row)
    print("%2d x %dx%d, %3d of %dx%d  maps: loop %9.3f ms [%.3f, %.3f] bank %9.3f (x%.3f) entry-loop %9.3f (x%.3f)  locate: loop %9.3f [%.3f, %.3f] bank %9.3f (x%.3f) "
          "entry-loop %9.3f (x%.3f)  useful %.0f / %.0f TOPS, issued %.0f / %.0f  same: %s" % (
              n, iw, ih, m, t, t, row["loop_maps_ms"], *row["loop_maps_ms_min_max"], row["bank_maps_ms"], row["bank_over_loop_maps"], row["entry_maps_ms"],
              row["entry_over_loop_maps"], row["loop_locate_ms"], *row["loop_locate_ms_min_max"], row["bank_locate_ms"], row["bank_over_loop_locate"],
              row["entry_locate_ms"], row["entry_over_loop_locate"], row["useful_tops_maps"], row["useful_tops_locate"], row["issued_tops_maps"],
              row["issued_tops_locate"], all(same.values())), flush=True)
    del maps_l, maps_b, img
    torch.cuda.empty_cache()
    with open(OUT, "w") as f:  # after every shape: a run cut short keeps what it measured
        json.dump(results, f, indent=1)
        f.write("\n")
print("wrote", OUT)
