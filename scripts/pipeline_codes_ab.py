#!/usr/bin/env python3
"""A/B of gsh_edge_pipeline_batch's coded chunks (gsh_tune key 28) in ONE process on one GPU: the benchmark's batch
(512 x 3840x2160, radius 2, tmp = NULL) timed under each listed value of the key, the values taken in turn round after round
so that clock drift hits all of them alike.

    python scripts/pipeline_codes_ab.py [--values 0,-1,256] [--rounds 5] [--steps 10] [--frames 512] [--out FILE]

  0    the rule (codes around the guess from the chunk before)      -1   never: every chunk on the byte path
  -2   the rule with the guess from two chunks back                 -3   ... from one chunk back
  256  every guess forced to 255: the window is [240, 254], every frame of the batch misses and is redone by the repair
       launch -- the stated cost of a batch whose frames have nothing to do with each other

Prints one JSON line: per value the median and the range of ms per step over the rounds, and whether dst and thr were the
same bytes under every value."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--values", default="0,-1,256")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import grayskull_amd as gs
    g = gs.Grayskull(os.environ["GS_BENCH_LIB"]) if os.environ.get("GS_BENCH_LIB") else gs.lib()
    g.set_device(0)
    g.use_torch_stream()
    values = [int(v) for v in a.values.split(",")]
    src = torch.empty((a.frames, a.height, a.width), dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    hist = torch.zeros((a.frames, 256), dtype=torch.int32, device="cuda")
    thr = torch.zeros(a.frames, dtype=torch.uint8, device="cuda")
    g.synth_batch(src, 1000)
    torch.cuda.synchronize()

    def step():
        g.edge_pipeline_batch(dst, None, src, 2, hist, thr)

    ms = {v: [] for v in values}
    sums = {}
    try:
        for v in values:  # warm-up and the bytes each value leaves
            g.tune(28, v)
            dst.fill_(9)
            step(), step()
            torch.cuda.synchronize()
            sums[v] = (int(dst.view(torch.int64).sum().item()), thr.cpu().numpy().tolist())
        for _ in range(a.rounds):
            for v in values:
                g.tune(28, v)
                step()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    step()
                torch.cuda.synchronize()
                ms[v].append((time.perf_counter() - t0) / a.steps * 1e3)
    finally:
        g.tune(28, 0)
    first = sums[values[0]]
    out = {"workload": "%d x %dx%d, radius 2, tmp = NULL" % (a.frames, a.width, a.height), "rounds": a.rounds, "steps_per_round": a.steps,
           "same_bytes_under_every_value": all(s == first for s in sums.values()),
           "thr_min_max": [min(first[1]), max(first[1])],
           "ms_per_step": {str(v): {"median": round(statistics.median(x), 4), "min": round(min(x), 4), "max": round(max(x), 4),
                                    "all": [round(y, 4) for y in x]} for v, x in ms.items()}}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
