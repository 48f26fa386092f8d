"""Shared cases of tests/test_cap_sweep.py (emulator) and tests/test_gpu_cap_sweep.py (MI355X): every ordered, capped output
of the library -- gs_fast keypoints, gs_lbp_detect rectangles, gs_match_orb matches, the nkps of gs_orb_extract and of the
batched pyramid ORB, gs_blobs' nblobs, and their batch forms -- run at EVERY cap (or at caps_for(): every mask-word, half-word,
QUAD-group and chunk seam) instead of the handful of caps the other files pin.

`g` is a bound library, `o` the oracle, `mem` a parity_cases.Mem ("host": numpy, which the emulator also takes for device
memory; "device": torch CUDA tensors).  For FAST, LBP and matching the reference stops at `n >= cap` inside its scan loop
(ref grayskull.h :530, :824-831, :685), so the expected list is the PREFIX of one uncapped oracle run; that property is the
reference's, so it is checked on the oracle itself at a sample of the caps before any library call.  For ORB the FAST cap
min(4 * nkps, 5000) changes the candidate set (ref :656): no prefix, the oracle is called at every nkps.  For blobs the cap
changes the labels of the whole plane: the reference is called at every nblobs.

Every condition on an INPUT (seams with hits on both sides, a keypoint in a chunk >= 1024, caps on both sides of the first
scale, the pyramid's quota states, accepted queries in three chunks, a non-prefix ORB list) is an assert on oracle results,
made when the case is built -- before the first library call of any test that uses it."""
import numpy as np

import blob_cases as bc
import lbp_cascade_cases as lc
import orb_pyramid_batch_cases as oc
import orb_pyramid_libm_cases as ol
import parity_cases as pc
from grayskull_amd import BLOB_DTYPE
from oracle.pyoracle import Oracle
from shape_frontier_cases import contrast_windows
from util import assert_same

_MEMO = {}


def memo(key, make):
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def frozen(a):
    a.setflags(write=False)
    return a


# ---- the cap set ---------------------------------------------------------------------------------------------------------
UNITS = (32, 64, 2048)  # items of a half word, of a mask word, of a chunk


def caps_for(T, marks=(), randoms=200, units=UNITS):
    """the caps of a sweep that is too long to run in full: 1..130 (two 64-bit mask words, two half-word seams), every
    k * 32 +- 1, k * 64 +- 1 and k * 2048 +- 1 up to T, m - 1 .. m + 1 for every mark (scale boundaries, chunk and per-frame
    totals), T - 1 .. T + 2, and `randoms` caps drawn by RandomState(T) from 1 .. T + 2; sorted, all >= 1.  (randoms, units: what the
    emulator's thinner sweeps keep of the last and of the k * unit series)"""
    s = set(range(1, 131))
    for unit in units:
        for k in range(1, T // unit + 1):
            s.update((k * unit - 1, k * unit + 1))
    for m in tuple(marks) + (T,):
        s.update((m - 1, m, m + 1))
    s.add(T + 2)
    if randoms:
        s.update(int(c) for c in np.random.RandomState(T).randint(1, T + 3, randoms))
    return sorted(c for c in s if c >= 1)


def all_caps(T, lowest=1):
    return list(range(lowest, T + 3))


def host(mem, t, dtype):
    """a buffer of either kind of memory as a numpy array of `dtype` (Mem.get leaves a host array's type alone)"""
    return np.asarray(mem.get(t)).view(dtype)


def u32(records):
    """records (structured) -> (n, words) uint32"""
    r = np.ascontiguousarray(records)
    return r.view(np.uint32).reshape(len(r), -1)


# ---- 1. gs_fast, gsh_fast_batch --------------------------------------------------------------------------------------------
RING = tuple(zip((0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1), (-3, -3, -2, -1, 0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3)))
SEAMS = (32, 64, 256, 2048)  # half word | mask word (lane of k_emit) | QUAD group of k_fast_nms | chunk
PLANTED_W, PLANTED_H = 306, 16


def planted_corners():
    """306 x 16, all 5, with the ring of parity_cases.fast_unsigned_wrap_quirk (sixteen 20s round a 5: response 15 at
    threshold 20) planted so that the items s - 1 and s of every seam s are keypoints in BOTH numberings: (y-3) * (w-6) + (x-3)
    of k_fast_nms (300 per row) and (y-3) * tx * 64 + (x-3) of the sparse pass (tx = 5: 320 per row).  Items s - 1 and s are
    neighbouring pixels, so the corners come in pairs: their rings overlap, neither ring covers the other's centre, and the
    equal responses both pass the `>` of the maximum test.  Pairs lie at least 8 px apart.  Row 0 of the interior is the same
    in both numberings (items 31 | 32, 63 | 64, 255 | 256); 2047 | 2048 is row 6, columns 247 | 248 in the first and 127 | 128
    in the second."""
    w, h = PLANTED_W, PLANTED_H
    strides = (w - 6, (w - 6 + 63) // 64 * 64)
    img = np.full((h, w), 5, np.uint8)
    centres = set()
    for stride in strides:
        for s in SEAMS:
            for item in (s - 1, s):
                r, c = divmod(item, stride)
                assert c < w - 6 and r < h - 6
                centres.add((c + 3, r + 3))
    for (x, y) in centres:
        for dx, dy in RING:
            img[y + dy, x + dx] = 20
    for (x, y) in centres:
        assert img[y, x] == 5, "a ring covers a centre"
    return img, strides


def _fast_frames():
    return {"synth96x80": (Oracle.synth(96, 80, 5), 20),
            "random131x70": (np.random.RandomState(3).randint(0, 256, (70, 131)).astype(np.uint8), 12),
            "random300x40": (np.random.RandomState(3).randint(0, 256, (40, 300)).astype(np.uint8), 12),
            "planted306x16": (planted_corners()[0], 20)}


FAST_SMALL = ("synth96x80", "random131x70", "random300x40", "planted306x16")
# name: (w, h, the value of gsh_tune key 19 the frame is for): more than kEmitSelfScan = 1024 chunks, so k_chunk_scan runs and
# its 1024-wide loop makes a second pass.  Sparse pass: one word per 64-px tile row, ceil(1 * 39994 / 32) = 1250 chunks;
# item kernel: ceil(10 * 209994 / 2048) = 1026 chunks
FAST_TALL = {"tall16x40000": (16, 40000, 0), "tall16x210000": (16, 210000, 1)}
TALL_THRESHOLD = 30


class FastCase:
    pass


def fast_case(o, name):
    """frame, threshold, the caller's score map, the oracle's uncapped list and score map; for the small frames the prefix
    property checked on the oracle at caps_for(T)[::7], for the tall ones at 5 caps, and the input conditions"""
    def make():
        c = FastCase()
        c.name = name
        if name in FAST_TALL:
            w, h, c.key19 = FAST_TALL[name]
            c.img = contrast_windows(np.random.RandomState(h).randint(0, 256, (h, w)).astype(np.uint8))
            c.thr = TALL_THRESHOLD
        else:
            c.img, c.thr = _fast_frames()[name]
            h, w = c.img.shape
        c.sm0 = np.random.RandomState(1).randint(0, 256, (h, w)).astype(np.uint8)  # the NMS reads the caller's 3-px frame
        if name.startswith("planted"):
            c.sm0 &= 15  # items 31 .. 256 lie in the first interior row, next to the caller's bytes: none may exceed the response 15
        frozen(c.sm0)
        limit = min((w - 6) * (h - 6), 100000)
        c.full, c.smo = o.fast(c.img, limit, c.thr, c.sm0)
        c.T = len(c.full)
        assert c.T < limit or limit == (w - 6) * (h - 6)
        frozen(c.full), frozen(c.smo), frozen(c.img)
        if name in FAST_TALL:
            assert 10 < c.T < 3000, "%s: %d keypoints" % (name, c.T)
            x, y = c.full["x"].astype(np.int64), c.full["y"].astype(np.int64)
            stride = (w - 6 + 63) // 64 * 64 if c.key19 == 0 else w - 6
            chunk = ((y - 3) * stride + (x - 3)) // 2048
            nchunks = -(-((h - 6) * stride) // 2048)
            assert nchunks > 1024, "%s: %d chunks: k_emit would scan for itself" % (name, nchunks)
            assert (chunk == 0).any() and (chunk >= 1024).any(), "%s: chunks %d .. %d" % (name, chunk.min(), chunk.max())
            c.sampled = sorted({1, c.T // 4, c.T // 2, c.T - 1, c.T + 1})
        else:
            assert c.T > 8
            c.sampled = caps_for(c.T)[::7]
        if name.startswith("planted"):
            x, y = c.full["x"].astype(np.int64), c.full["y"].astype(np.int64)
            for stride in planted_corners()[1]:
                items = set(((y - 3) * stride + (x - 3)).tolist())
                for s in SEAMS:
                    assert s - 1 in items and s in items, "no keypoint on both sides of item %d at %d items per row" % (s, stride)
            assert (c.full["response"] == 15).all() and c.T == 10
        for cap in c.sampled:  # the prefix property is the reference's: checked here, on the CPU
            ko, smo = o.fast(c.img, cap, c.thr, c.sm0)
            assert_same(ko, c.full[:cap], "%s: the oracle at cap %d is not the prefix of its uncapped list" % (name, cap))
            assert_same(smo, c.smo, "%s: the oracle's score map at cap %d" % (name, cap))
        return c
    return memo(("fast", name), make)


def check_fast(g, o, mem, name, key19, caps=None):
    """gs_fast at every cap (default: 1 .. T + 2) under gsh_tune key 19 = 0 (sparse NMS, k_emit's half-word loop) or 1
    (k_fast_nms, the QUAD loop): the keypoints are the prefix of the oracle's uncapped list; the score map at the sampled caps"""
    c = fast_case(o, name)
    caps = all_caps(c.T) if caps is None else caps
    sampled = set(c.sampled)
    s = mem.put(c.img)
    g.tune(19, key19)
    try:
        for cap in sorted(set(caps) | sampled):
            sm = mem.put(c.sm0)
            k = g.fast(s, sm, cap, c.thr)
            assert_same(k, c.full[:cap], "gs_fast %s, key 19 = %d, %s memory, cap %d of %d" % (name, key19, mem.kind, cap, c.T))
            if cap in sampled:
                assert_same(mem.get(sm), c.smo, "gs_fast score map %s, key 19 = %d, cap %d" % (name, key19, cap))
    finally:
        g.tune(19, 0)


def fast_batch_case(o):
    def make():
        c = FastCase()
        c.thr = 12
        c.frames = frozen(np.stack([np.random.RandomState(seed).randint(0, 256, (70, 131)).astype(np.uint8) for seed in (3, 4, 5)]))
        c.sm0 = frozen(np.random.RandomState(1).randint(0, 256, c.frames.shape).astype(np.uint8))
        c.full = [o.fast(f, 64 * 125, c.thr, s) for f, s in zip(c.frames, c.sm0)]
        c.T = [len(k) for k, _ in c.full]
        assert len(set(c.T)) == 3 and min(c.T) > 130, c.T
        return c
    return memo("fast batch", make)


def check_fast_batch(g, o, mem, key19, caps=None):
    """gsh_fast_batch on three 131 x 70 frames, one call per cap: counts[f] == min(T_f, cap), the prefix, and the records
    from counts[f] to cap keep their random prefill"""
    c = fast_batch_case(o)
    n = len(c.frames)
    caps = all_caps(max(c.T)) if caps is None else caps
    s = mem.put(c.frames)
    g.tune(19, key19)
    try:
        for cap in caps:
            pre = np.random.RandomState(cap).randint(0, 2 ** 32, (n, cap, 12), dtype=np.uint64).astype(np.uint32)
            kps, counts, sm = mem.put(pre), mem.put(np.full(n, 0x5A5A5A5A, np.uint32)), mem.put(c.sm0)
            g.fast_batch(s, sm, kps, counts, cap, c.thr)
            g.sync()
            k, cnt = host(mem, kps, np.uint32), host(mem, counts, np.uint32)
            what = "gsh_fast_batch key 19 = %d, cap %d" % (key19, cap)
            for f in range(n):
                m = min(c.T[f], cap)
                assert int(cnt[f]) == m, "%s frame %d: count %d, expected %d" % (what, f, cnt[f], m)
                assert_same(k[f, :m], u32(c.full[f][0][:m]), "%s frame %d" % (what, f))
                assert_same(k[f, m:], pre[f, m:], "%s frame %d: records beyond the count" % (what, f))
            if cap in (1, max(c.T) + 2):
                for f in range(n):
                    assert_same(mem.get(sm)[f], c.full[f][1], "%s frame %d score map" % (what, f))
    finally:
        g.tune(19, 0)


# ---- 2. gs_lbp_detect, gsh_lbp_detect_batch --------------------------------------------------------------------------------
LBP_NAMES = ("every_branch", "two_stages", "truth_tables")
LBP_SCAN = (1.2, 1.0, 3.0, 1)
LBP_ORDER = ("edges", "flat", "synth")


class LbpCase:
    pass


def scale_marks(full):
    """the cumulative detection counts after every scale of an uncapped list (window widths grow with the scale)"""
    widths = full["w"].astype(np.int64)
    assert (np.diff(widths) >= 0).all()
    return [int((widths <= w).sum()) for w in np.unique(widths)]


def lbp_case(o, name, randoms=200, units=UNITS):
    def make():
        s = LbpCase()
        s.c = c = lc.case(name, o)
        s.full = {f: lc.expected(c, o, f, (lc.UNCAPPED,) + LBP_SCAN) for f in lc.ALL_FRAMES}
        s.T = len(s.full["synth"])
        marks = sorted({m for f in lc.ALL_FRAMES for m in scale_marks(s.full[f])})
        s.n0 = int((s.full["synth"]["w"] == c.casc.window_w).sum())  # as lbp_cascade_cases.case() counts the first scale
        assert s.n0 == scale_marks(s.full["synth"])[0] and len(scale_marks(s.full["synth"])) >= 2
        s.caps = caps_for(s.T, marks, randoms, units)
        below, above = sum(1 for k in s.caps if k < s.n0), sum(1 for k in s.caps if s.n0 < k <= s.T)
        assert below >= 20 and above >= 20, "%s: %d caps below and %d above the first scale's %d detections" % (name, below, above, s.n0)
        for cap in s.caps[::11]:  # the prefix property, on the oracle
            assert_same(o.lbp_detect(c.casc, c.ii["synth"], cap, *LBP_SCAN), s.full["synth"][:cap],
                        "%s: the oracle at max_rects %d is not the prefix of its uncapped list" % (name, cap))
        return s
    return memo(("lbp", name, randoms, units), make)


def check_lbp(g, o, mems, name, key14, randoms=200, units=UNITS):
    """gs_lbp_detect on the synth frame under gsh_tune key 14 = 0 (the rule) / 1 (k_lbp_cascade everywhere), host and device
    tables: every cap of the set gives the prefix"""
    s = lbp_case(o, name, randoms, units)
    tables = [(m, m.put(s.c.ii["synth"])) for m in mems]
    g.tune(14, key14)
    try:
        for cap in s.caps:
            for m, t in tables:
                assert_same(g.lbp_detect(s.c.casc, t, cap, *LBP_SCAN), s.full["synth"][:cap],
                            "gs_lbp_detect %s, key 14 = %d, %s table, max_rects %d of %d (first scale %d)" % (name, key14, m.kind, cap, s.T, s.n0))
    finally:
        g.tune(14, 0)


def check_lbp_batch(g, o, mem, name, randoms=200, units=UNITS, part=(0, 1)):
    """gsh_lbp_detect_batch on the case's three frames, one call per cap: per frame min(T_f, cap) rectangles, its own prefix,
    and the prefill beyond.  part = (i, k): the caps i, i + k, i + 2 k, .. of the set alone"""
    s = lbp_case(o, name, randoms, units)
    ii = mem.put(np.stack([s.c.ii[f] for f in LBP_ORDER]))
    want = [np.stack([r["x"], r["y"], r["w"], r["h"]], 1).astype(np.uint32).reshape(-1, 4) for r in (s.full[f] for f in LBP_ORDER)]
    dc = g.cascade_create(s.c.casc)
    try:
        for cap in s.caps[part[0]::part[1]]:
            rects, counts = mem.zeros((3, cap, 4), np.uint32, 0x5A5A5A5A), mem.zeros(3, np.uint32, 0x5A5A5A5A)
            g.lbp_detect_batch(dc, ii, rects, counts, cap, *LBP_SCAN)
            g.sync()
            r, n = host(mem, rects, np.uint32), host(mem, counts, np.uint32)
            for k, f in enumerate(LBP_ORDER):
                m = min(len(want[k]), cap)
                what = "gsh_lbp_detect_batch %s, %s frame, max_rects %d of %d" % (name, f, cap, len(want[k]))
                assert int(n[k]) == m, "%s: %d rectangles, expected %d" % (what, n[k], m)
                assert_same(r[k, :m], want[k][:m], what)
                assert (r[k, m:] == 0x5A5A5A5A).all(), what + ": records beyond the count"
    finally:
        dc.close()


# ---- 3. gs_match_orb, gsh_match_orb_dev, gsh_match_orb_batch -----------------------------------------------------------------
MATCH_DISTANCE = 60.0


class MatchCase:
    pass


def match_case(o, n1, n2, cuts):
    """random_descriptors(n1, n2); cuts: the query counts of the batch's pairs (the first is n1).  The oracle's list at
    max_matches = n1 per cut, and the prefix property on the oracle at caps[::13]"""
    def make():
        c = MatchCase()
        c.k1, c.k2 = pc.random_descriptors(n1, n2)
        c.cuts = cuts
        c.full = [frozen(o.match_orb(c.k1[:q], c.k2, q, MATCH_DISTANCE)) for q in cuts]
        c.A = len(c.full[0])
        assert len({len(f) for f in c.full}) == len(cuts), "the pairs of the batch accept the same number of queries"
        idx = c.full[0]["idx1"].astype(np.int64)
        words = set((idx // 64).tolist())
        assert len(words) >= 3, "the accepted queries span fewer than three mask words"
        if n1 > 2048:
            chunks = idx // 2048
            if n2 == 64:
                # random_descriptors(4200, 64) keeps a partner in the train set for the last queries only: chunk 0 accepts
                # nothing (its wave of k_emit returns on a zero count), the two later chunks emit
                assert set(chunks.tolist()) == {1, 2}, "accepted queries in chunks %r" % set(chunks.tolist())
            else:
                assert set(chunks.tolist()) >= {0, 1, 2}, "no accepted query in one of the three chunks"
            first = int(idx[chunks == 1][0])
            assert (idx < first).sum() < first, "no rejected query before the first accepted one of the second chunk (%d)" % first
        c.caps = all_caps(c.A) if n1 <= 2048 else caps_for(c.A, [len(f) for f in c.full])
        for cap in c.caps[::13]:
            for q, f in zip(cuts, c.full):
                assert_same(o.match_orb(c.k1[:q], c.k2, cap, MATCH_DISTANCE), f[:cap], "%d x %d: the oracle at max_matches %d is not the prefix" % (q, n2, cap))
        return c
    return memo(("match", n1, n2, cuts), make)


def check_match_dropin(g, o, n1, n2, cuts, caps=None):
    c = match_case(o, n1, n2, cuts)
    for cap in caps or c.caps:
        assert_same(g.match_orb(c.k1, c.k2, cap, MATCH_DISTANCE), c.full[0][:cap], "gs_match_orb %d x %d, max_matches %d of %d" % (n1, n2, cap, c.A))


def check_match_dev(g, o, mem, n1, n2, cuts, caps=None):
    c = match_case(o, n1, n2, cuts)
    d1, d2 = mem.put(u32(c.k1)), mem.put(u32(c.k2))
    want = u32(c.full[0])
    for cap in caps or c.caps:
        matches, count = mem.zeros((cap, 3), np.uint32, 0x5A5A5A5A), mem.zeros(1, np.uint32, 0x5A5A5A5A)
        g.match_orb_dev(d1, n1, d2, n2, matches, count, cap, MATCH_DISTANCE)
        g.sync()
        m, n = host(mem, matches, np.uint32), int(host(mem, count, np.uint32)[0])
        what = "gsh_match_orb_dev %d x %d, max_matches %d of %d" % (n1, n2, cap, c.A)
        assert n == min(c.A, cap), "%s: count %d" % (what, n)
        assert_same(m[:n], want[:n], what)
        assert (m[n:] == 0x5A5A5A5A).all(), what + ": records beyond the count"


def check_match_batch(g, o, mem, n1, n2, cuts, caps=None):
    """one pair per cut in one call per cap: the query sets are copies of one set cut by the device-side n1, the train set is shared"""
    c = match_case(o, n1, n2, cuts)
    n = len(cuts)
    d1 = mem.put(np.stack([u32(c.k1)] * n))
    dn1, d2 = mem.put(np.asarray(cuts, np.uint32)), mem.put(u32(c.k2))
    want = [u32(f) for f in c.full]
    for cap in caps or c.caps:
        matches, counts = mem.zeros((n, cap, 3), np.uint32, 0x5A5A5A5A), mem.zeros(n, np.uint32, 0x5A5A5A5A)
        g.match_orb_batch(d1, dn1, d2, None, matches, counts, MATCH_DISTANCE)
        g.sync()
        m, cnt = host(mem, matches, np.uint32), host(mem, counts, np.uint32)
        for p in range(n):
            k = min(len(want[p]), cap)
            what = "gsh_match_orb_batch pair %d (%d x %d), max_matches %d of %d" % (p, cuts[p], n2, cap, len(want[p]))
            assert int(cnt[p]) == k, "%s: count %d" % (what, cnt[p])
            assert_same(m[p, :k], want[p][:k], what)
            assert (m[p, k:] == 0x5A5A5A5A).all(), what + ": records beyond the count"


# ---- 4. nkps of ORB ----------------------------------------------------------------------------------------------------------
ORB_SHAPES = ((96, 80), (131, 97))
ORB_THR = 20


def nostdlib_oracle():
    """the reference header compiled with -DGS_NO_STDLIB where oracle/_ref was built (what tests/test_property_shapes.py
    uses), else the restatement switched to the same polynomials"""
    from oracle import pyoracle
    return memo("ns oracle", lambda: Oracle("reference_nostdlib") if pyoracle.have_reference_nostdlib() else oc.ns())


class OrbCase:
    pass


def orb_case(o, w, h, flavour):
    """two synth frames of one shape, a random score map; the oracle's list at EVERY nkps from 1 to K + 2 (K: the larger
    frame count at nkps = 1250), and the assert that some list is no prefix of the largest one"""
    def make():
        c = OrbCase()
        c.frames = frozen(np.stack([Oracle.synth(w, h, 5), Oracle.synth(w, h, 6)]))
        c.sm0 = frozen(np.random.RandomState(7).randint(0, 256, c.frames.shape).astype(np.uint8))
        sm = c.sm0 if flavour == "libm" else np.zeros_like(c.sm0)  # parity_cases.orb_nostdlib passes a zeroed score map
        top = [o.orb_extract(f, 1250, ORB_THR, s) for f, s in zip(c.frames, sm)]
        c.K = max(len(k) for k in top)
        assert c.K > 8
        c.want = {nkps: [frozen(o.orb_extract(f, nkps, ORB_THR, s)) for f, s in zip(c.frames, sm)] for nkps in all_caps(c.K)}
        c.not_prefix = [nkps for nkps in all_caps(c.K) if any(k.tobytes() != t[:len(k)].tobytes() for k, t in zip(c.want[nkps], top))]
        assert c.not_prefix, "every swept list is a prefix of the largest: the sweep could not tell min(4 * nkps, 5000) from one cap"
        return c
    return memo(("orb", w, h, flavour), make)


def check_orb_dropin(g, o, mem, w, h, sweep=None):
    """gs_orb_extract (libm flavour) at every nkps on both frames"""
    c = orb_case(o, w, h, "libm")
    for f, img in enumerate(c.frames):
        s = mem.put(img)
        for nkps in sweep or all_caps(c.K):
            k = g.orb_extract(s, nkps, ORB_THR, mem.put(c.sm0[f]))
            assert_same(k, c.want[nkps][f], "gs_orb_extract %dx%d frame %d, %s memory, nkps %d of %d" % (w, h, f, mem.kind, nkps, c.K))


def check_orb_batch(g, o, mem, w, h, sweep=None):
    """gsh_orb_extract_batch (libm flavour) on the two frames in one call per nkps"""
    c = orb_case(o, w, h, "libm")
    s = mem.put(c.frames)
    for nkps in sweep or all_caps(c.K):
        got = g.orb_extract_batch_dev(s, mem.put(c.sm0), nkps, ORB_THR)
        for f in range(len(c.frames)):
            assert_same(got[f], c.want[nkps][f], "gsh_orb_extract_batch %dx%d frame %d, nkps %d of %d" % (w, h, f, nkps, c.K))


def check_orb_batch_nostdlib(g, w, h, sweep=None):
    """gsh_orb_extract_batch_nostdlib at every nkps through parity_cases.orb_nostdlib"""
    o = nostdlib_oracle()
    c = orb_case(o, w, h, "nostdlib")
    for nkps in sweep or all_caps(c.K):
        pc.orb_nostdlib(g, o, c.frames, nkps=nkps, threshold=ORB_THR)


# (w, h, levels, the nkps swept): the third case is there for `per == 0` alone: with two and three levels per is zero for
# nkps 1 and for nkps 1, 2 only -- three swept values; four levels add nkps 1, 2, 3
PYRAMID_SWEEPS = ((131, 97, 2, range(1, 101)), (203, 171, 3, range(1, 101)), (300, 270, 4, range(1, 9)))
PYRAMID_SEED = 120


def pyramid_sweep(flavour, w, h, levels, sweep):
    """the expected values of every nkps of one sweep, from orb_expected of the flavour's case file (computed on the prefill
    that run_orb gives the buffer), and per nkps which quota states it is in: "per0" (nkps / L == 0: every level but the last
    is skipped), "per" (it is not), "own_cap" (the last-level quotas differ inside the batch, and for one frame the selection
    from its own min(4 * quota, 5000) candidates differs from the one a uniform min(4 * nkps, 5000) gives:
    orb_pyramid_batch_cases.check_cap_per_frame)"""
    def make():
        cases = oc if flavour == "nostdlib" else ol
        frames = oc.batch_abcd(w, h)
        n = len(frames)
        nb1 = sum(oc.plane_sizes(w, h, levels))
        L = len(oc.dims(w, h, levels))
        pre = np.random.RandomState(PYRAMID_SEED).randint(0, 256, n * nb1).astype(np.uint8)  # run_orb's first draw
        states = {}
        for nkps in sweep:
            key = "sweep %s %dx%d nkps %d" % (flavour, w, h, nkps)
            kw = {} if flavour == "nostdlib" else {"differs": False}
            want = cases.orb_expected(key, frames, nkps, levels, pre, **kw)
            pl = [p for _, _, p in want]
            st = {"per0"} if nkps // L == 0 else {"per"}
            assert all((p[0][0] == 0) == (nkps // L == 0) for p in pl)
            if len({p[-1][0] for p in pl}) > 1:
                for f, p in enumerate(pl):
                    quota = p[-1][0]
                    lev = oc.levels_of(frames[f], levels)[-1]
                    lh, lw = lev.shape
                    own = oc.select(oc.port().fast(lev, min(4 * quota, 5000), oc.THR)[0], quota, lw, lh)
                    uniform = oc.select(oc.port().fast(lev, min(4 * nkps, 5000), oc.THR)[0], quota, lw, lh)
                    if own != uniform:
                        st.add("own_cap")
            states[nkps] = st
        return frames, states
    return memo(("pyramid", flavour, w, h, levels, tuple(sweep)), make)


def pyramid_states(flavour):
    """over all sweeps: how many swept (case, nkps) are in each quota state; each must occur at least 5 times"""
    count = {"per0": 0, "per": 0, "own_cap": 0}
    for (w, h, levels, sweep) in PYRAMID_SWEEPS:
        for st in pyramid_sweep(flavour, w, h, levels, sweep)[1].values():
            for k in st:
                count[k] += 1
    assert min(count.values()) >= 5, "the pyramid sweeps do not cross every quota boundary 5 times: %r" % count
    return count


def check_pyramid(g, gd, flavour, w, h, levels, sweep):
    """gsh_orb_extract_pyramid_batch_nostdlib / gsh_orb_extract_pyramid_batch at every nkps of the sweep through the case
    file's run_orb: counts, level_counts, records and buffer between guards.  4 guard checks per nkps"""
    pyramid_states(flavour)
    cases = oc if flavour == "nostdlib" else ol
    frames, _ = pyramid_sweep(flavour, w, h, levels, sweep)
    for nkps in sweep:
        cases.run_orb(g, gd, "sweep %s %dx%d nkps %d" % (flavour, w, h, nkps), PYRAMID_SEED, frames, nkps, levels)


# ---- 5. gs_blobs, gsh_blobs_batch --------------------------------------------------------------------------------------------
def blob_reference():
    """the compiled reference where oracle/_ref was built, else the plain-Python restatement: as tests/test_gpu_blobs.py decides"""
    from oracle import pyoracle
    return memo("blob ref", lambda: bc.Ref().blobs if pyoracle.have_reference() else bc.spec_blobs)


def blob_expected(name, img, cap):
    return memo(("blobs", name, cap), lambda: blob_reference()(img, cap))


def blob_frames(shapes=None):
    """blob_cases.emu_frames(), or its random frames of the given (w, h) shapes"""
    frames = memo("blob frames", bc.emu_frames)
    if shapes is None:
        return frames
    return [(name, img) for name, img in frames if name.startswith("random") and (img.shape[1], img.shape[0]) in shapes]


def check_blobs(g, mem, name, img, caps=None):
    """gs_blobs at every nblobs from 1 to starts + 2 (or `caps`): records, count and the whole label plane; device memory:
    image and labels on the device"""
    starts = bc.start_count(img)
    d = mem.put(img)
    for cap in (all_caps(starts) if caps is None else caps):
        want = blob_expected(name, img, cap)
        if mem.kind == "host":
            got = g.blobs(d, cap)
        else:
            recs, lab = g.blobs(d, cap, labels=mem.put(np.zeros(img.shape, np.int16)))
            got = (recs, host(mem, lab, np.uint16))
        bc.assert_blobs_equal(got, want, "gs_blobs %s, %s memory, nblobs %d (%d start pixels)" % (name, mem.kind, cap, starts))


def check_blobs_batch(g, mem, shape, caps=None):
    """gsh_blobs_batch: the four densities of one shape as one 4-frame batch per cap"""
    frames = blob_frames((shape,))
    assert len(frames) == 4
    batch = np.stack([img for _, img in frames])
    starts = [bc.start_count(img) for img in batch]
    d = mem.put(batch)
    for cap in (all_caps(max(starts)) if caps is None else caps):
        lab, recs = mem.put(np.zeros(batch.shape, np.int16)), mem.zeros((4, cap, 8), np.uint32, 0x5A5A5A5A)
        counts = mem.zeros(4, np.uint32, 0x5A5A5A5A)
        g.blobs_batch(d, lab, recs, counts, cap)
        g.sync()
        r, l, n = host(mem, recs, np.uint32), host(mem, lab, np.uint16), host(mem, counts, np.uint32)
        for f, (name, img) in enumerate(frames):
            m = int(n[f])
            assert m <= cap
            got = (np.ascontiguousarray(r[f, :m]).reshape(-1).view(BLOB_DTYPE), l[f])
            bc.assert_blobs_equal(got, blob_expected(name, img, cap), "gsh_blobs_batch %s, nblobs %d (%d start pixels)" % (name, cap, starts[f]))
