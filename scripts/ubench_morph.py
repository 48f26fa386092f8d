#!/usr/bin/env python3
"""gsh_morph_batch (ceil(n / 4) passes of radius <= 4) against n repeated gsh_dilate_batch / gsh_erode_batch launches (what
the `morph` verb of gsbatch ran before) and one such launch as the unit, on 64 x 3840x2160, 64 x 3838x2160 (ragged) and
8 x 1920x1080; then the band height of each single-pass radius (gsh_tune key 0) on the two 4K shapes.
Events around back-to-back launches after a warm-up, three rounds with the two forms alternating (median; min and max
kept).  The three planes lie 320 KiB past a multiple of 2 MiB apart (docs/design/next_and_not_kept.md section 4).
    python scripts/ubench_morph.py [out.json]        (default profiles/morph_fused_bench.json; the log is stdout)"""
import json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import grayskull_amd as gs
g = gs.Grayskull(os.environ["UB_LIB"]) if os.environ.get("UB_LIB") else gs.lib(); g.use_torch_stream()
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "morph_fused_bench.json")
SHAPES = ((64, 2160, 3840), (64, 2160, 3838), (8, 1080, 1920))
ITERS = (2, 3, 4, 8, 9, 19)
BANDS = (0, 8, 12, 16, 24, 32, 48, 64, 128)
def timeit(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn(); fn(); torch.cuda.synchronize(); e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps
def rounds(fns, reps, n=3):
    """{name: [ms per round]}, the forms alternating inside every round"""
    out = {k: [] for k in fns}
    for _ in range(n):
        for k, fn in fns.items(): out[k].append(timeit(fn, reps))
    return out
def med(v): return statistics.median(v)
results = {"device": torch.cuda.get_device_name(0), "library": g.version(), "rows": [], "band_rows": []}
for (F, H, W) in SHAPES:
    nb = F * H * W
    pitch = ((nb + (2 << 20) - 1) & ~((2 << 20) - 1)) + (320 << 10)
    flat = torch.empty(3 * pitch, dtype=torch.uint8, device="cuda")
    src, a, b = (flat[k * pitch:k * pitch + nb].view(F, H, W) for k in range(3))
    g.synth_batch(src, 1000)
    for dilate in (1, 0):
        one = g.dilate_batch if dilate else g.erode_batch
        def repeated(n, last=a, other=b):
            """n launches, the planes swapped after each like the driver's loop; the result lands in `last`"""
            cur, dsts = src, ([last, other] * n)[:n][::-1]
            for d in dsts: one(d, cur); cur = d
        reps = 20 if F * H * W > (1 << 27) else 100
        unit = med(rounds({"u": lambda: one(a, src)}, reps)["u"])
        for it in ITERS:
            r = rounds({"fused": lambda: g.morph_batch(a, src, it, dilate, tmp=b), "repeated": lambda: repeated(it)}, max(4, reps // it))
            g.morph_batch(a, src, it, dilate, tmp=b); keep = a.clone(); repeated(it)
            same = bool(torch.equal(a, keep))
            row = {"frames": F, "w": W, "h": H, "op": "dilate" if dilate else "erode", "iterations": it, "passes": (it + 3) // 4,
                   "unit_ms": unit, "fused_ms": med(r["fused"]), "fused_ms_min_max": [min(r["fused"]), max(r["fused"])],
                   "repeated_ms": med(r["repeated"]), "repeated_ms_min_max": [min(r["repeated"]), max(r["repeated"])], "same_bytes": same}
            results["rows"].append(row)
            print("%d x %dx%d %-6s n=%-2d  unit %.4f ms   fused %.4f ms (%d passes, %.2f units)   repeated %.4f ms (%.2f units)   "
                  "fused/repeated %.3f   same bytes: %s" % (F, W, H, row["op"], it, unit, row["fused_ms"], row["passes"], row["fused_ms"] / unit,
                                                            row["repeated_ms"], row["repeated_ms"] / unit, row["fused_ms"] / row["repeated_ms"], same), flush=True)
        if F * H * W > (1 << 27):
            for it in (2, 3, 4):
                line = []
                for T in BANDS:
                    g.tune(0, T)
                    ms = med(rounds({"f": lambda: g.morph_batch(a, src, it, dilate)}, 20)["f"])
                    g.tune(0, 0)
                    results["band_rows"].append({"frames": F, "w": W, "h": H, "op": "dilate" if dilate else "erode", "radius": it, "band_rows": T, "ms": ms})
                    line.append("T=%d %.4f" % (T, ms))
                print("%d x %dx%d %-6s radius %d by band rows (0 = the launcher's own): %s" % (F, W, H, "dilate" if dilate else "erode", it, "  ".join(line)), flush=True)
    del flat, src, a, b
with open(OUT, "w") as f:
    json.dump(results, f, indent=1); f.write("\n")
print("wrote", OUT)
