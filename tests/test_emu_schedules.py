"""The kernels under permuted block and wave orders (CPU, kernel-logic emulator).

The emulator used to know one order: the workgroups of a launch ascending, the threads of a workgroup ascending in every
scheduling round.  That is the kindest order for every inter-block and inter-wave protocol of the library ("the chunks
before me have finished", "the last block to arrive has the highest index").  tests/emu/hip_emu.h now has a switch
(emu_set_schedule / GS_EMU_SCHEDULE): the blocks of a launch and the threads of a round each ascending (0), descending
(1), outside-in (2) or in a permutation drawn from a seed (3).  This module

  * runs tests/emu/test_sched.cpp, which logs the order emu::launch really takes (a switch that did nothing would make
    everything else here pass), and
  * repeats the existing comparisons against the CPU oracle (the case modules; nothing is restated) under the schedules
    (blocks, threads) = (1, 0), (0, 1), (1, 1), (2, 2) and (3, 3) with two seeds, for every kernel that has LDS, a wave
    or quad exchange, an atomic, or reads what another block of its launch wrote: k_fast.h, k_fast_nms.h, k_orb.h,
    k_lbp.h, k_lbp_tile.h, k_compact.h, k_pointwise.h (histogram, Otsu, checksum), k_blobs.h, k_contour.h, k_box.h,
    k_strip.h / k_stencil.h / k_morphk.h / k_fused.h, k_integral.h and k_tmatch.h.  docs/design/oracle_and_parity.md
    (section 6) names the test that runs each of them.

Left out: the pure per-pixel kernels (resize, crop, perspective, threshold, synth).  A thread of theirs reads its input
and writes its own output pixel; there is nothing between threads or blocks that an order could change.

Every test takes every schedule.  The whole matrix of cases under every schedule would take several times as long as
tests/test_emu_logic.py, which is the time this module may take, so inside a test the cases are DEALT over the
schedules (`deal`): in a fixed shuffled order, schedule k takes every share-th case from the k-th on.  Every case
runs under at least one permuted schedule, every schedule meets every family of cases, every tune key value meets
several schedules.  Dealt, every case under two of the six schedules: the kernels whose only protocol is between the
waves of one block (strip, box, morph, fused, integral), the FAST matrix and the key 20 routes of the template match.
Everything else -- FAST batches, ORB selection, matching, histogram / Otsu / checksum, the blob, paint and contour hand
cases, the random blob frames, the contour batches -- runs under all six.  The LBP early exit, the one protocol BETWEEN
blocks whose outcome an order can change, has its cases assigned by hand (LBP_PLAN).

What no schedule of this emulator can show is listed in hip_emu.h: two workgroups resident at once, preemption between
two memory operations, streams.
"""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import blob_cases as bc
import blob_paint_cases as bpc
import contour_cases as cc
import morph_cases as mc
import parity_cases as pc
import sequence_cases as sc
from grayskull_amd import BLOB_DTYPE
from oracle.pyoracle import Oracle
from test_property_shapes import _body_histogram_batch, _img
from util import assert_same, random_cascade

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
MEM = pc.Mem("host")

# (blocks, threads, seed)
SCHEDULES = ((1, 0, 0), (0, 1, 0), (1, 1, 0), (2, 2, 0), (3, 3, 1), (3, 3, 2))


def set_schedule(emu, blocks, threads, seed=0):
    emu.c.emu_set_schedule.argtypes = [C.c_int, C.c_int, C.c_ulonglong]
    emu.c.emu_set_schedule.restype = None
    emu.c.emu_set_schedule(blocks, threads, seed)


def get_schedule(emu):
    b, t, s = C.c_int(-1), C.c_int(-1), C.c_ulonglong(0)
    emu.c.emu_get_schedule(C.byref(b), C.byref(t), C.byref(s))
    return b.value, t.value, s.value


class Sched:
    def __init__(self, emu, index):
        self.emu, self.index = emu, index
        self.blocks, self.threads, self.seed = SCHEDULES[index]

    def on(self):
        self.before = get_schedule(self.emu)  # kind 0, or what GS_EMU_SCHEDULE put the whole run under
        set_schedule(self.emu, self.blocks, self.threads, self.seed)

    def off(self):
        set_schedule(self.emu, *self.before)

    def deal(self, cases, share):
        """this schedule's part of `cases`: a fixed shuffle, then every share-th case from index % share on -- with six
        schedules and share <= 6 every case is run, under 6 / share schedules"""
        cases = list(cases)
        random.Random(len(cases)).shuffle(cases)
        assert 6 % share == 0
        return cases[self.index % share::share]


@pytest.fixture(params=range(len(SCHEDULES)), ids=["b%dt%ds%d" % s for s in SCHEDULES])
def sched(request, emu):
    s = Sched(emu, request.param)
    s.on()
    try:
        assert get_schedule(emu) == SCHEDULES[request.param]
        yield s
    finally:
        s.off()


# ---- the scheduler itself ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sched_program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("sched") / "test_sched"
    subprocess.check_call(["g++", "-DGS_EMU", "-std=c++17", "-O1", "-g", "-Wall", "-I", EMU_DIR,
                           os.path.join(EMU_DIR, "test_sched.cpp"), os.path.join(EMU_DIR, "hip_emu.cpp"), "-o", str(exe)])
    return str(exe)


def test_scheduler_runs_every_block_and_thread_in_the_promised_order(sched_program):
    """tests/emu/test_sched.cpp: grids of 1, 2, 7 and 64 x 3 x 2 blocks, blocks of 1, 64, 65, 256 and 1024 threads, every
    kind of either order"""
    env = {k: v for k, v in os.environ.items() if k != "GS_EMU_SCHEDULE"}
    r = subprocess.run([sched_program], capture_output=True, env=env)
    assert r.returncode == 0 and b"all passed" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def test_schedule_from_the_environment(sched_program):
    """GS_EMU_SCHEDULE=blocks,threads[,seed] is read by the emulator itself: 5 blocks outside-in, 3 threads descending"""
    def run(value):
        env = dict(os.environ)
        env.pop("GS_EMU_SCHEDULE", None)
        if value is not None:
            env["GS_EMU_SCHEDULE"] = value
        return subprocess.run([sched_program, "env"], capture_output=True, env=env)
    asc = ["%d.%d" % (b, t) for b in range(5) for t in range(3)]
    r = run(None)
    assert r.returncode == 0 and r.stdout.decode().split() == ["schedule", "0", "0", "0", "order"] + asc
    r = run("2,1,5")
    want = ["%d.%d" % (b, t) for b in (0, 4, 1, 3, 2) for t in (2, 1, 0)]
    assert r.returncode == 0 and r.stdout.decode().split() == ["schedule", "2", "1", "5", "order"] + want
    r = run("3,0")
    got = r.stdout.decode().split()
    assert r.returncode == 0 and got[:4] == ["schedule", "3", "0", "0"] and sorted(got[5:]) == sorted(asc)
    assert run("4,0").returncode != 0 and run("nonsense").returncode != 0  # a typo must not mean "ascending"


def test_schedule_switch_of_the_loaded_library(emu):
    """the same switch through the emulator library's exported function; what was in force before (kind 0, or the
    schedule GS_EMU_SCHEDULE put the whole run under) is restored in a finally"""
    before = get_schedule(emu)
    try:
        set_schedule(emu, 2, 3, 99)
        assert get_schedule(emu) == (2, 3, 99)
    finally:
        set_schedule(emu, *before)
    assert get_schedule(emu) == before


# ---- LBP: the max_rects early exit ------------------------------------------------------------------------------------
K_CHUNK, K_GROUP_SHIFT, K_SUPER_SHIFT = 2048, 5, 10  # k_compact.h kChunkItems, k_lbp.h kLbpGroupShift / kLbpSuperShift


class LbpInput:
    """one integral image + cascade + scan parameters, the oracle's uncapped hits per chunk, and a model of which chunks
    a block order lets k_lbp_cascade skip"""

    def __init__(self, emu, oracle, casc, img, sf, mn, mx, step):
        self.casc, self.params = casc, (sf, mn, mx, step)
        self.ii = oracle.integral(img)
        h, w = img.shape
        self.total = emu.lbp_window_count(casc, w, h, sf, mn, mx, step)
        # the scale loop of the launcher (gs_detect.cpp build_scales = ref :819-821), float32
        self.scales, base, s = [], 0, np.float32(mn)
        while s <= np.float32(mx):
            ww, wh = int(np.float32(casc.window_w) * s), int(np.float32(casc.window_h) * s)
            if ww > w or wh > h:
                break
            nx, ny = (w - ww) // step + 1, (h - wh) // step + 1
            nch = (nx * ny + K_CHUNK - 1) // K_CHUNK
            self.scales.append(dict(w=ww, h=wh, nx=nx, ny=ny, nchunks=nch, base=base))
            base += nch
            s = np.float32(s * np.float32(sf))
        assert sum(q["nx"] * q["ny"] for q in self.scales) == self.total, "the scale loop restated here is not the launcher's"
        self.nchunks = base
        self.all = oracle.lbp_detect(casc, self.ii, self.total, sf, mn, mx, step)  # a cap no scan reaches
        self.hits = np.zeros(base, np.int64)
        by_size = {(q["w"], q["h"]): q for q in self.scales}
        assert len(by_size) == len(self.scales)
        for r in self.all:
            q = by_size[(int(r["w"]), int(r["h"]))]
            self.hits[q["base"] + ((int(r["y"]) // step) * q["nx"] + int(r["x"]) // step) // K_CHUNK] += 1
        self._oracle, self._rects, self._asc = oracle, {}, {}

    def expected(self, cap):
        if cap not in self._rects:
            self._rects[cap] = self._oracle.lbp_detect(self.casc, self.ii, cap, *self.params)
        return self._rects[cap]

    def model(self, order, cap, swizzle):
        """windows k_lbp_cascade evaluates when ALL scales share one launch (key 14 = 1) and its blocks run in `order`
        (a function position -> linear block): k_lbp.h:308-344 and :498-505, block by block.  The emulator runs a block
        to completion before the next starts, so a block sees exactly what the blocks before it IN THIS ORDER published."""
        gx = max(q["nchunks"] for q in self.scales)
        if swizzle:
            gx = (gx + 7) & ~7
        n = gx * len(self.scales)
        group = np.zeros((self.nchunks >> K_GROUP_SHIFT) + 1, np.int64)
        sup = np.zeros((self.nchunks >> K_SUPER_SHIFT) + 1, np.int64)
        total_hits = evaluated = 0
        booked = cap < min(self.total, 0xffffffff)
        for i in range(n):
            b = order(n, i)
            bx, q = b % gx, self.scales[b // gx]
            cx = bx
            if swizzle:
                per, j = (q["nchunks"] + 7) >> 3, bx >> 3
                if j >= per:
                    continue
                cx = (bx & 7) * per + j
            if cx >= q["nchunks"]:
                continue
            lin = q["base"] + cx
            g1, g2 = lin >> K_GROUP_SHIFT, lin >> K_SUPER_SHIFT
            before = 0
            if booked and total_hits >= cap:
                before = int(sup[:g2].sum() + group[g2 << (K_SUPER_SHIFT - K_GROUP_SHIFT):g1].sum())
            if before >= cap:
                continue
            evaluated += min(K_CHUNK, q["nx"] * q["ny"] - cx * K_CHUNK)
            c = int(self.hits[lin])
            if c and booked:
                group[g1] += c
                sup[g2] += c
                total_hits += c
        return evaluated

    def ideal(self, cap):
        """every chunk knows all that precedes it (chunks in scan order): the most any order may skip.  A block that
        sees less -- counters of chunks that have not run yet are 0, and a partial sum only skips less -- evaluates
        more, so this is a lower bound for EVERY order, chunk mapping and kernel choice with chunk-sized work items."""
        return self.model(lambda n, i: i, cap, False)


ORDERS = {0: lambda n, i: i, 1: lambda n, i: n - 1 - i, 2: lambda n, i: n - 1 - i // 2 if i & 1 else i // 2}

_LBP = {}


def lbp_input(name, emu, oracle, cascade):
    if name not in _LBP:
        off = get_schedule(emu)
        set_schedule(emu, 0, 0, 0)  # lbp_window_count and the oracle launch nothing; be sure anyway
        try:
            if name == "E":  # the edge map and call of test_lbp_chunk_granular_early_exit: 43 chunks in the first scale
                _LBP[name] = LbpInput(emu, oracle, cascade, oracle.sobel(oracle.blur(Oracle.synth(352, 288, 1000), 2)), 1.1, 1.0, 4.0, 1)
            else:  # the permissive random cascade: thousands of hits per scale
                _LBP[name] = LbpInput(emu, oracle, random_cascade(2), Oracle.synth(300, 260, 5), 1.3, 1.0, 3.0, 1)
        finally:
            set_schedule(emu, *off)
    return _LBP[name]


def lbp_run(emu, inp, cap):
    cnt = np.zeros(4, np.uint64)
    emu.lbp_count_evaluated(cnt)
    try:
        r = emu.lbp_detect(inp.casc, inp.ii.copy(), cap, *inp.params)
    finally:
        emu.lbp_count_evaluated(None)
    return r, int(cnt[0])


def lbp_ascending(emu, inp, key14, cap):
    """windows evaluated with blocks in ascending order and chunks / tiles in dispatch order (key 13 = 1), per
    (input, key 14, cap); measured once.  For the tile kernel, too, that order gives every block the complete sums of
    what precedes it (tiles to the left and above have finished), so no order may evaluate fewer."""
    k = (key14, cap)
    if k not in inp._asc:
        was = get_schedule(emu)
        set_schedule(emu, 0, 0, 0)
        try:
            emu.tune(14, key14), emu.tune(13, 1)
            r, ev = lbp_run(emu, inp, cap)
            assert_same(r, inp.expected(cap), "ascending, key 14 = %d cap %d" % (key14, cap))
            inp._asc[k] = ev
        finally:
            emu.tune(14, 0), emu.tune(13, 0)
            set_schedule(emu, *was)
    return inp._asc[k]


# schedule index -> (input, key 14, key 13, cap).  Inputs: E = 352 x 288 edge map (caps 1, 20, 60, 4096), R = random
# cascade on 300 x 260 (caps 1, 100, 3000); key 14: 0 rule, 1 k_lbp_cascade everywhere, 2 k_lbp_tile; key 13: 0 rule,
# 1 dispatch order, 2 XCD-aware mapping.  A full scan of E costs the emulator 8-13 s, so the cases that evaluate (nearly)
# everything are spread: each schedule has one or two of them.
LBP_PLAN = {
    0: (("E", 1, 0, 1), ("E", 1, 0, 20), ("E", 0, 0, 1), ("E", 2, 1, 20), ("R", 1, 0, 100), ("R", 1, 0, 3000), ("R", 0, 0, 1),
        ("R", 2, 2, 3000)),
    1: (("E", 1, 0, 1), ("E", 1, 0, 20), ("E", 1, 1, 1), ("E", 2, 0, 1), ("R", 1, 0, 1), ("R", 1, 1, 3000), ("R", 2, 0, 100)),
    2: (("E", 0, 0, 20), ("E", 1, 2, 1), ("E", 2, 2, 1), ("R", 1, 2, 3000), ("R", 0, 1, 100), ("R", 1, 0, 1)),
    3: (("E", 1, 0, 1), ("E", 1, 0, 20), ("E", 1, 2, 1), ("E", 0, 1, 1), ("R", 1, 0, 3000), ("R", 2, 2, 1), ("R", 1, 2, 100)),
    4: (("E", 1, 0, 1), ("E", 1, 2, 20), ("E", 0, 2, 1), ("E", 2, 0, 20), ("R", 1, 0, 100), ("R", 0, 0, 3000), ("R", 1, 2, 1)),
    5: (("E", 2, 0, 4096), ("E", 0, 0, 60), ("E", 1, 1, 1), ("R", 1, 1, 1), ("R", 2, 0, 100), ("R", 0, 2, 3000)),
}


def test_lbp_early_exit_is_exact_and_skips_only_what_the_order_allows(emu, oracle, cascade, sched):
    """rectangles: the oracle's first max_rects hits under every order.  Windows evaluated (gsh_lbp_count_evaluated):

    * never more than there are, and all of them when the scan has fewer hits than the cap;
    * never fewer than with every chunk knowing all that precedes it (LbpInput.ideal / lbp_ascending);
    * key 14 = 1 puts all scales into ONE launch of k_lbp_cascade (gs_detect.cpp: consecutive scales with the same choice
      share a launch), so for the fixed block orders the count is worked out block by block (LbpInput.model) and must
      be met exactly.  Descending without the XCD mapping: nothing that precedes a block in scan order has run when it
      starts, so every window is evaluated -- strictly more than ascending at cap 1.  (With the XCD mapping block x is
      chunk (x % 8) * per + x / 8: a block with a higher x may hold an earlier chunk, and descending order may skip;
      the model follows the mapping.)
    * with the rule or the tile kernel (key 14 = 0 / 2) scales are split over several launches by LDS need, and a launch
      sees everything earlier launches published whatever its own order: only the bounds are asserted there."""
    for name, key14, key13, cap in LBP_PLAN[sched.index]:
        inp = lbp_input(name, emu, oracle, cascade)
        what = "%s key14=%d key13=%d cap %d" % (name, key14, key13, cap)
        if len(inp.all) < cap:
            low = inp.total  # the cap is never reached: no counter ever lets a block skip
        else:
            low = inp.ideal(cap) if key14 == 1 else lbp_ascending(emu, inp, key14, cap)
        try:
            emu.tune(14, key14), emu.tune(13, key13)
            r, ev = lbp_run(emu, inp, cap)
        finally:
            emu.tune(14, 0), emu.tune(13, 0)
        print("%s schedule %s: %d of %d windows evaluated, lower bound %d" % (what, SCHEDULES[sched.index], ev, inp.total, low))
        assert_same(r, inp.expected(cap), what)
        assert low <= ev <= inp.total, (what, low, ev, inp.total)
        if len(inp.all) < cap:
            assert ev == inp.total, "%s: nothing to skip when the cap is never reached" % what
        if key14 == 1 and sched.blocks in ORDERS:
            assert ev == inp.model(ORDERS[sched.blocks], cap, key13 == 2), what
            if sched.blocks == 1 and key13 != 2:
                assert ev == inp.total, "%s: descending order has nothing before any block" % what
                if cap == 1:
                    assert ev > inp.ideal(cap), what


# ---- FAST / NMS / compaction / ORB / matching ---------------------------------------------------------------------------
def _fast_images(w, h):
    rs = np.random.RandomState(w + h)
    flat = np.full((h, w), 100, np.uint8)
    flat[::3, ::3] = 140  # a lattice of equal corners: ties everywhere
    dark = rs.randint(0, 256, (h, w)).astype(np.uint8)
    dark[h // 4:h // 2, w // 3:2 * w // 3] = rs.randint(0, 12, (h // 2 - h // 4, 2 * w // 3 - w // 3))  # p < t: the unsigned-wrap class
    return {"random": rs.randint(0, 256, (h, w)).astype(np.uint8), "flat": flat, "dark": dark}


FAST_SIZES = ((131, 64), (70, 71), (260, 17))
FAST_CASES = [(size, kind, k7, k19, k18) for size in FAST_SIZES for kind in ("random", "flat", "dark")
              for k7 in (0, 2) for k19 in (0, 1) for k18 in (0, 1, 2)]


def test_fast_score_nms_and_compaction(emu, oracle, sched):
    """gs_fast (k_fast_score_q4 / _px, k_fast_nms_sparse / k_fast_nms, k_compact.h): caps 1, 9 and 30000"""
    for (w, h), kind, k7, k19, k18 in sched.deal(FAST_CASES, 3):
        try:
            emu.tune(7, k7), emu.tune(19, k19), emu.tune(18, k18)
            pc.fast(emu, oracle, _fast_images(w, h)[kind], MEM, threshold=12, caps=(1, 9, 30000))
        finally:
            emu.tune(7, 0), emu.tune(19, 0), emu.tune(18, 0)


def test_fast_batch_split_over_launches(emu, oracle, sched):
    """3 frames, two per launch (key 8 = 2): the tiles are numbered over the whole batch"""
    w, h, n = 131, 64, 3
    frames = np.stack([_fast_images(w, h)[k] for k in ("random", "flat", "dark")])
    for cap in (1, 9, 30000):
        sm, kps, counts = np.zeros_like(frames), np.zeros((n, cap, 12), np.uint32), np.zeros(n, np.uint32)
        try:
            emu.tune(8, 2)
            emu.fast_batch(frames, sm, kps, counts, cap, 12)
        finally:
            emu.tune(8, 0)
        for f in range(n):
            ko, smo = oracle.fast(frames[f], cap, 12)
            assert counts[f] == len(ko), (cap, f)
            assert_same(kps[f, :len(ko)].reshape(-1).view(ko.dtype), ko, "cap %d frame %d" % (cap, f))
            assert_same(sm[f], smo, "cap %d scoremap %d" % (cap, f))


def test_orb_selection_among_equal_responses(emu, oracle, sched):
    """gsh_orb_extract_batch_nostdlib on binary frames (many equal responses), nkps 1, 3 and 40: the cap cuts inside a
    group of equal responses, so the stable order of k_orb.h's selection (cnt[] / mask) decides who is kept; and
    gs_orb_extract + the host-side batch on a synthetic frame"""
    rs = np.random.RandomState(17)
    frames = np.stack([_img(rs, 70, 71, 2) for _ in range(2)])
    for nkps in (1, 3, 40):
        pc.orb_nostdlib(emu, sc.port_nostdlib(), frames, nkps=nkps, threshold=20)
    pc.orb_batch(emu, oracle, np.stack([Oracle.synth(96, 80, 31), _img(rs, 96, 80, 2)]), MEM, nkps=9)
    pc.orb(emu, oracle, Oracle.synth(67, 45, 7), MEM, nkps=30)


@pytest.mark.parametrize("n1,n2", [(5, 63), (3, 65), (70, 513)])
def test_match_orb(emu, oracle, sched, n1, n2):
    pc.match_random(emu, oracle, n1, n2)


# ---- blobs, corners, largest, paint, contours ----------------------------------------------------------------------------
def test_blob_and_contour_hand_cases(emu, sched):
    from test_blobs import check_hand_cases as blob_hand_cases
    from test_contours import HostArrays, check_hand_cases as contour_hand_cases
    blob_hand_cases(emu)
    contour_hand_cases(emu, HostArrays)
    bpc.check_hand_cases(emu, bpc.Host)


@pytest.mark.parametrize("w", [63, 65, 130])
def test_blobs_corners_largest_and_paint_on_random_frames(emu, sched, w):
    """k_blobs.h (run labelling, atomic-min union, ordered record compaction), corners, largest, paint: random binary
    frames with nblobs below, at and above the number of start pixels; then batches of 3, two frames per launch"""
    rng = np.random.default_rng(w)
    h = 21
    frames = np.stack([bc.random_mask(rng, h, w, d) for d in (0.5, 0.62, 0.8)])
    starts = bc.start_count(frames[0])
    for cap in (max(starts - 1, 1), starts, starts + 1):
        got = emu.blobs(frames[0], cap)
        bc.assert_blobs_equal(got, bc.spec_blobs(frames[0], cap), "w %d cap %d (%d start pixels)" % (w, cap, starts))
    recs, labels = got
    for r in recs[:: max(1, len(recs) // 5)]:
        assert emu.blob_corners(frames[0], labels, r) == bc.spec_corners(frames[0], labels, r)
    cap = 40
    want = [bc.spec_blobs(f, cap) for f in frames]
    lab, out, cnt = np.zeros(frames.shape, np.int16), np.zeros((3, cap, 8), np.int32), np.zeros(3, np.int32)
    try:
        emu.tune(8, 2)
        emu.blobs_batch(frames, lab, out, cnt, cap)
        got = out.view(BLOB_DTYPE).reshape(3, cap)
        for f in range(3):
            bc.assert_blobs_equal((got[f, :int(cnt[f])], lab[f].view(np.uint16)), want[f], "batch frame %d" % f)
        bpc.check_against_spec(emu, bpc.Host, frames, [wf[0] for wf in want], "paint, w %d" % w, nblobs=cap)
        blobs, counts = bpc.pack([wf[0] for wf in want], cap)
        best, idx = bpc.run_largest(emu, bpc.Host, blobs, counts)
        for f in range(3):
            k = bpc.largest(want[f][0], min(len(want[f][0]), cap))
            assert idx[f] == k and np.array_equal(best[f], blobs[f, k]), f
    finally:
        emu.tune(8, 0)


def test_contour_batches(emu, sched):
    """k_contour.h: the batch that decides endless walks, split over launches (key 8 = 3 on 7 frames)"""
    from test_contours import HostArrays, check_split
    check_split(emu, HostArrays)


# ---- histogram / Otsu / checksum -------------------------------------------------------------------------------------
@pytest.mark.parametrize("bpf,piece", [(2, 0), (5, 0), (2, 999), (5, 999)])
def test_histogram_otsu_batch(emu, oracle, sched, bpf, piece):
    """the body of test_histogram_batch_any_shape at (n, w, h) = (3, 300, 40): blocks per frame (key 11) 2 and 5, whole
    frames and pieces of 999 bytes (key 12): partial histograms of several blocks folded by another kernel"""
    for kind in (0, 1, 2):
        _body_histogram_batch(emu, oracle, 3, 300, 40, 40 + kind, kind, piece, bpf)


def test_checksum_and_otsu_probes(emu, oracle, sched):
    b = sc.Backend(emu, oracle, MEM)
    sc.probe_checksum(b, None)
    sc.probe_otsu(b, None)


# ---- integral, template matching ---------------------------------------------------------------------------------------
INTEGRAL_SHAPES = ((37, 9), (612, 13), (1029, 17), (2049, 21), (4097, 33))


def test_integral_batch(emu, oracle, sched):
    """k_integral.h: row scans whose carries cross waves (widths past 1024, 2048, 4096), n = 2"""
    for (w, h) in sched.deal(INTEGRAL_SHAPES + ((4097, 9),), 3):
        rs = np.random.RandomState(w)
        src = np.stack([rs.randint(0, 256, (h, w)).astype(np.uint8), np.full((h, w), 255, np.uint8)])
        ii = np.zeros((2, h, w), np.uint32)
        emu.integral_batch(src, ii)
        for f in range(2):
            assert_same(ii[f], oracle.integral(src[f]), "gsh_integral_batch %dx%d frame %d" % (w, h, f))


def test_match_template_with_the_table_of_squares(emu, oracle, sched):
    """the smallest case of test_match_template_on_the_matrix_cores; key 20 = 5 takes sum I'^2 from the integral table of
    squares, 2 from the sliding sums, 1 is the dot-product kernel"""
    iw, ih, tw, th = 100, 80, 16, 4
    rs = np.random.RandomState(iw + tw)
    img = rs.randint(0, 256, (ih, iw)).astype(np.uint8)
    tmpls = [rs.randint(0, 256, (th, tw)).astype(np.uint8), img[ih - th:, iw - tw:].copy()]
    try:
        for key20 in sorted(set(sched.deal([5, 2, 1], 3) + [5])):
            for t in tmpls:
                emu.tune(20, key20)
                r = np.zeros((ih - th + 1, iw - tw + 1), np.uint8)
                emu.match_template(img, t, r)
                assert_same(r, oracle.match_template(img, t), "gs_match_template key 20 = %d" % key20)
    finally:
        emu.tune(20, 0)


# ---- strip, box, morph, fused: protocols between the waves of one block ----------------------------------------------------
STRIP_CASES = [(w, h, T) for (w, h) in ((1040, 11), (2064, 17), (4112, 23)) for T in (0, 1, 5)]


def test_strip_kernels(emu, oracle, sched):
    """k_strip.h / k_stencil.h: blur radii 1-3, sobel, erode, dilate on rows that two and four waves share, band heights
    (key 0) by rule, 1 and 5"""
    for (w, h, T) in sched.deal(STRIP_CASES, 3):
        try:
            emu.tune(0, T)
            pc.stencils(emu, oracle, Oracle.synth(w, h, w + h + T), MEM, radii=(1, 2, 3))
        finally:
            emu.tune(0, 0)


BOX_CASES = [(w, h, r, T) for (w, h) in ((1040, 13), (2064, 11), (4112, 23), (1038, 19), (2049, 15))
             for r in (4, 9, 16, 20) for T in (0, 1, 5)]


def test_box_kernels(emu, oracle, sched):
    """k_box.h: the register-ring kernel where the frame has 2 r + 1 rows (r = 4 and 9 at these heights), k_box16 for the
    rest (r = 9 on the lower frames, r = 16 and 20), the edge kernel of ragged widths; both modes (blur, adaptive
    threshold); band heights (key 0) by rule, 1 and 5 for either kernel"""
    rng = np.random.RandomState(9)
    for (w, h, r, T) in sched.deal(BOX_CASES, 3):
        img = rng.randint(0, 256, (h, w)).astype(np.uint8)
        img[:, : w // 2] |= 0xF0
        try:
            emu.tune(0, T)
            d = np.zeros_like(img)
            emu.blur(d, img.copy(), r)
            assert_same(d, oracle.blur(img, r), "gs_blur r=%d T=%d %dx%d" % (r, T, w, h))
            d = np.zeros_like(img)
            emu.adaptive_threshold(d, img.copy(), r, 5)
            assert_same(d, oracle.adaptive_threshold(img, r, 5), "gs_adaptive_threshold r=%d T=%d %dx%d" % (r, T, w, h))
        finally:
            emu.tune(0, 0)


MORPH_CASES = [(w, h, it, dilate) for (w, h) in ((1040, 11), (2064, 17), (4112, 23), (2049, 9)) for it in range(1, 10)
               for dilate in (True, False)]


def test_morph_batch(emu, sched):
    """k_morphk.h: 1 to 9 iterations (one to three passes, both parities of the plane alternation)"""
    rng = np.random.default_rng(31)
    for (w, h, it, dilate) in sched.deal(MORPH_CASES, 3):
        mc.check(emu, mc.Host, mc.frames(rng, 2, h, w, "random"), it, dilate, "schedules")


def test_fused_edge_pipeline(emu, oracle, sched):
    """k_fused.h: blur -> sobel -> histogram in one kernel, Otsu and threshold behind it; r = 1-3; 5 frames in chunks of 2
    (key 5)"""
    cases = [(w, h, r, T) for (w, h) in ((1040, 11), (2064, 9), (4112, 5), (80, 23)) for r in (1, 2, 3) for T in (0, 1, 5)]
    for (w, h, r, T) in sched.deal(cases, 3) + [(80, 37, 1 + sched.index % 3, 0)]:
        n = 5
        src = np.stack([Oracle.synth(w, h, 300 + w + i) for i in range(n)])
        out, hist, thr = np.full_like(src, 7), np.zeros((n, 256), np.uint32), np.zeros(n, np.uint8)
        try:
            emu.tune(5, 2), emu.tune(0, T)
            emu.edge_pipeline_batch(out, None, src, r, hist, thr)
        finally:
            emu.tune(5, 0), emu.tune(0, 0)
        for i in range(n):
            s = oracle.sobel(oracle.blur(src[i], r))
            t = oracle.otsu_threshold(s)
            assert np.array_equal(hist[i], oracle.histogram(s)), "histogram of frame %d, %dx%d r=%d T=%d" % (i, w, h, r, T)
            assert thr[i] == t
            assert np.array_equal(out[i], oracle.threshold(s, t)), "frame %d, %dx%d r=%d T=%d" % (i, w, h, r, T)
