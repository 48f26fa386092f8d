#!/usr/bin/env python3
"""gsh_match_orb_batch against the loop a caller had to write before it: download the n counts of the extraction
(a host sync), then per pair gsh_match_orb_dev -- three dependent launches each.

    python scripts/ubench_match_batch.py [out.json]   # default profiles/match_batch.json; the log is stdout

Per shape (32 and 256 pairs of 500 x 500, 64 pairs of 2500 x 2500, one set of 2500 against 256 sets of 2500, one pair of
500 x 500 and of 2500 x 2500), in one process: a warm-up of both forms, then ROUNDS rounds with the two alternating
inside every round, each timed with stream events around as many back-to-back repetitions as fill WINDOW_MS; the median
with min and max kept.
  loop     counts -> host (blocking copy), then for p: gsh_match_orb_dev(k1[p], n1[p], k2[p], n2[p])
  batch    gsh_match_orb_batch
Gpairs/s = descriptor pairs compared per second; the issue bound is bench.py's: 8 v_xor_b32 at the full VALU rate + 8
v_bcnt_u32_b32 at the VOP3 rate per pair and lane.  The matches of the batch are compared with the loop's.
(profiles/match_batch_forms.json / .log: the same script on a build that still had the kernel's two candidate forms -- LDS
broadcast and scalar loads -- behind a tuning key, columns `lds` and `sgpr`.)"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import grayskull_amd as gs

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "match_batch.json")
ROUNDS = int(os.environ.get("UB_ROUNDS", "5"))
WINDOW_MS = float(os.environ.get("UB_WINDOW_MS", "100"))
VALU_RATE_GINST = {"full": 1000.0, "half": 578.0}  # bench.py
BOUND = 64.0 / (8.0 / (VALU_RATE_GINST["full"] * 1e9) + 8.0 / (VALU_RATE_GINST["half"] * 1e9)) / 1e9  # Gpairs/s
# (pairs, query sets, records per query set, train sets, records per train set)
SHAPES = ((32, 32, 500, 32, 500), (256, 256, 500, 256, 500), (64, 64, 2500, 64, 2500), (256, 1, 2500, 256, 2500),
          (1, 1, 500, 1, 500), (1, 1, 2500, 1, 2500))
if os.environ.get("UB_TINY"):  # rehearsal of the script itself
    SHAPES = ((3, 3, 70, 3, 90), (3, 1, 70, 3, 90))
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


def descriptors(rng, nset, cap):
    """nset x cap records with random descriptors"""
    k = np.zeros((nset, cap, 12), np.uint32)
    k[:, :, 4:] = rng.integers(0, 2 ** 32, (nset, cap, 8), dtype=np.uint64)
    return k


def with_partners(rng, k, base):
    """every third record of every set becomes a base record with one bit flipped per dword (distance 8): partners across
    the sets, so that the ratio test accepts a realistic share"""
    third = k[:, ::3, 4:]
    flip = (1 << rng.integers(0, 32, third.shape, dtype=np.uint64)).astype(np.uint32)
    k[:, ::3, 4:] = base[:k.shape[1]:3, 4:][None] ^ flip


results = {"device": torch.cuda.get_device_name(0), "library": g.version(), "rounds": ROUNDS, "issue_bound_Gpairs_s": round(BOUND, 1),
           "forms": {"loop": "counts to the host (blocking), then gsh_match_orb_dev per pair",
                     "batch": "gsh_match_orb_batch"},
           "rows": []}
rng = np.random.default_rng(7)
for (n, nset1, cap1, nset2, cap2) in SHAPES:
    base = descriptors(rng, 1, max(cap1, cap2))[0]
    h1, h2 = descriptors(rng, nset1, cap1), descriptors(rng, nset2, cap2)
    with_partners(rng, h1, base), with_partners(rng, h2, base)
    k1, k2 = torch.from_numpy(h1.view(np.int32)).cuda(), torch.from_numpy(h2.view(np.int32)).cuda()
    n1 = torch.full((nset1,), cap1, dtype=torch.int32, device="cuda")
    n2 = torch.full((nset2,), cap2, dtype=torch.int32, device="cuda")
    out = {f: (torch.zeros((n, cap1, 3), dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda"))
           for f in ("loop", "batch")}

    def loop():
        m, c = out["loop"]
        c1, c2 = n1.cpu().numpy(), n2.cpu().numpy()  # the sync a caller of the per-pair entry needs
        for p in range(n):
            a, b = (p if nset1 > 1 else 0), (p if nset2 > 1 else 0)
            g.match_orb_dev(k1[a], int(c1[a]), k2[b], int(c2[b]), m[p], c[p:p + 1], cap1, 60.0)

    def batch():
        g.match_orb_batch(k1 if nset1 > 1 else k1[0], n1, k2 if nset2 > 1 else k2[0], n2, *out["batch"], 60.0)

    fns = {"loop": loop, "batch": batch}
    for fn in fns.values():  # warm-up: code objects, scratch growth
        fn()
    torch.cuda.synchronize()
    reps = {k: max(2, min(500, int(WINDOW_MS / max(timeit(fn, 2), 1e-3)) + 1)) for k, fn in fns.items()}
    r = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            r[k].append(timeit(fn, reps[k]))
    cl = out["loop"][1].cpu().numpy()
    same = torch.equal(out["batch"][1], out["loop"][1]) and all(torch.equal(out["batch"][0][p, :cl[p]], out["loop"][0][p, :cl[p]]) for p in range(n))
    pairs = n * cap1 * cap2
    row = {"pairs": n, "query_sets": nset1, "queries": cap1, "train_sets": nset2, "train": cap2, "matches": int(cl.sum()), "same_matches": bool(same),
           "reps": reps}
    for k, v in r.items():
        row[k + "_ms"] = statistics.median(v)
        row[k + "_ms_min_max"] = [min(v), max(v)]
        row[k + "_Gpairs_s"] = pairs / statistics.median(v) / 1e6
    row["spread_loop"] = (max(r["loop"]) - min(r["loop"])) / row["loop_ms"]
    row["batch_over_loop"] = row["batch_ms"] / row["loop_ms"]
    row["batch_frac_of_issue_bound"] = row["batch_Gpairs_s"] / BOUND
    results["rows"].append(row)
    print("%3d pairs, %3d x %4d against %3d x %4d  loop %9.4f ms [%.4f, %.4f]  batch %8.4f [%.4f, %.4f]  batch/loop %.4f  "
          "%.1f Gpairs/s = %.3f of the bound  matches %d  same: %s" % (
              n, nset1, cap1, nset2, cap2, row["loop_ms"], *row["loop_ms_min_max"], row["batch_ms"], *row["batch_ms_min_max"],
              row["batch_over_loop"], row["batch_Gpairs_s"], row["batch_frac_of_issue_bound"], row["matches"], same), flush=True)
    del k1, k2, out
    torch.cuda.empty_cache()
with open(OUT, "w") as f:
    json.dump(results, f, indent=1)
    f.write("\n")
print("wrote", OUT)
