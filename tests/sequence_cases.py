"""Backend-agnostic checks of what ONE call at ONE shape cannot see (tests/test_sequences.py on the emulator,
tests/test_gpu_sequences.py on the MI355X):

  A  direct parity of gsh_fast_score_batch, gsh_orb_extract, gsh_match_orb_dev and gsh_threshold_batch_dev
  B  chains of batch calls with no host sync or copy until the end, against the same chain with gsh_sync() after every
     call and against the oracle step by step; consecutive calls share a scratch slot that has to grow in mid-chain
  C  history independence: a small sparse call right after gsh_shutdown() and after "dirtying" calls of the same and of
     every other entry point that shares one of its scratch slots; the LBP geometry cache, the drop-in cascade cache and
     the jump table of gsh_synth_batch
  D  (GPU only, in test_gpu_sequences.py) switching streams with work still queued on the one left

`g` : grayskull_amd.Grayskull, `o` : oracle.pyoracle.Oracle, `mem` : parity_cases.Mem("host") for the emulator (its
"device" memory is host memory) or Mem("device") for torch CUDA tensors.  Every comparison is bit-exact."""
import copy

import numpy as np

import blob_cases as bc
import contour_cases as cc
import parity_cases as pc
from grayskull_amd import BLOB_DTYPE, CONTOUR_DTYPE, KEYPOINT_DTYPE
from oracle.pyoracle import Oracle
from util import assert_same, random_cascade

_SIGNED = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}
_CACHE = {}


class Backend:
    """a library, the oracle and one kind of "device" memory"""

    def __init__(self, g, o, mem):
        self.g, self.o, self.mem = g, o, mem
        self.dev = mem.kind == "device"

    def put(self, a):
        a = np.ascontiguousarray(a)
        if not self.dev:
            return a.copy()
        import torch
        if a.dtype in _SIGNED:  # torch has no arithmetic on these; carry the bits
            a = a.view(_SIGNED[a.dtype])
        return torch.from_numpy(a.copy()).cuda()

    def get(self, t, dtype=None):
        a = t.cpu().numpy() if self.dev else np.array(t)
        return a.view(dtype) if dtype is not None else a

    def sync(self):
        """everything the library and torch have enqueued is done"""
        self.g.sync()
        if self.dev:
            import torch
            torch.cuda.synchronize()

    def prefix(self, t, n, h, w):
        """the first n*h*w bytes of a uint8 buffer as (n, h, w) frames, without a copy"""
        flat = t.view(-1) if self.dev else t.reshape(-1)
        v = flat[:n * h * w]
        return v.view(n, h, w) if self.dev else v.reshape(n, h, w)

    def bytes2d(self, t, rows):
        """an int32 buffer as `rows` rows of bytes, without a copy"""
        if self.dev:
            import torch
            return t.view(torch.uint8).view(rows, -1)
        return t.view(np.uint8).reshape(rows, -1)


def synth_frames(w, h, n, seed):
    return np.stack([Oracle.synth(w, h, seed + i) for i in range(n)])


def port_nostdlib():
    if "ns" not in _CACHE:
        _CACHE["ns"] = Oracle("port_nostdlib")
    return _CACHE["ns"]


def rects_u32(r):
    return np.stack([r["x"], r["y"], r["w"], r["h"]], 1).astype(np.uint32) if len(r) else np.zeros((0, 4), np.uint32)


# ======================================================================================================================
# A. direct parity
# ======================================================================================================================
FAST_SCORE_SHAPES = ((7, 7), (8, 8), (67, 45), (260, 17), (131, 64), (1283, 517))


def fast_score(b, w, h, thresholds=(5, 20, 200, 300), ns=(1, 3), kinds=("synth", "noise", "low")):
    """gsh_fast_score_batch == the score map of the oracle's gs_fast.  The reference writes EVERY score in its first
    pass (ref grayskull.h:489-515, gs_set at :513) before the second pass (:517-532) selects keypoints, and the second
    pass only reads the map, so the keypoint cap has no bearing on it.  The destination starts as a random plane: the
    3-px frame keeps it.  With odd w*h frames 1 and 2 of a batch start at odd addresses; at threshold 300 `p - threshold`
    wraps for every pixel (the "darker" class of ref :498)."""
    g, o = b.g, b.o
    rs = np.random.RandomState(w * 977 + h)
    try:
        for n in ns:
            for kind in kinds:
                if kind == "synth":
                    img = synth_frames(w, h, n, 11)
                else:
                    img = rs.randint(0, 256 if kind == "noise" else 40, (n, h, w)).astype(np.uint8)
                d0 = rs.randint(0, 256, (n, h, w)).astype(np.uint8)
                s = b.put(img)
                for thr in thresholds:
                    exp = np.stack([o.fast(img[f], 1, thr, d0[f])[1] for f in range(n)])
                    for key7 in (0, 2):
                        g.tune(7, key7)
                        d = b.put(d0)
                        g.fast_score_batch(d, s, thr)
                        b.sync()
                        assert_same(b.get(d), exp, "fast score %dx%d n=%d %s thr=%d key7=%d" % (w, h, n, kind, thr, key7))
    finally:
        g.tune(7, 0)


ORB_DEV_SHAPES = ((96, 80), (67, 45), (640, 480), (31, 31))


def orb_extract_dev(b, w, h, threshold=20):
    """gsh_orb_extract (one device frame, keypoints to the host) == gs_orb_extract with the caller's non-zero score
    map, == frame 0 of gsh_orb_extract_batch; the score map it leaves is gs_fast's.  At 31 x 31 the 15-px border leaves
    the single position (15, 15)."""
    g, o = b.g, b.o
    rs = np.random.RandomState(w * 31 + h)
    frames = [Oracle.synth(w, h, 4), rs.randint(0, 256, (h, w)).astype(np.uint8), np.zeros((h, w), np.uint8)]
    sm0 = rs.randint(1, 256, (h, w)).astype(np.uint8)
    found = 0
    for i, img in enumerate(frames):
        for nkps in (1, 50, 500):
            what = "gsh_orb_extract %dx%d frame %d nkps=%d" % (w, h, i, nkps)
            sm = b.put(sm0)
            k = g.orb_extract_dev(b.put(img), sm, nkps, threshold)
            ko = o.orb_extract(img, nkps, threshold, sm0)
            assert len(k) == len(ko), "%s: %d keypoints, expected %d" % (what, len(k), len(ko))
            assert_same(k, ko, what)
            assert_same(k["angle"].view(np.uint32), ko["angle"].view(np.uint32), what + " angle bits")
            assert_same(b.get(sm), o.fast(img, min(nkps * 4, 5000), threshold, sm0)[1], what + " score map")
            kb = g.orb_extract_batch_dev(b.put(img[None]), b.put(sm0[None]), nkps, threshold)[0]
            assert_same(k, kb, what + " vs frame 0 of the batch")
            found += len(k)
    assert found > 0 or (w, h) == (31, 31)


MATCH_DEV_SIZES = ((1, 1), (5, 63), (3, 65), (4, 257), (70, 513), (300, 1030))
MATCH_SENTINEL = 0xA5A5A5A5


def _match_dev_once(b, k1, n1, k2, n2, mm, md, what):
    g, o = b.g, b.o
    exp = o.match_orb(k1[:n1], k2[:n2], mm, md)
    cap = mm + 5
    dm = b.put(np.full((cap, 3), MATCH_SENTINEL, np.uint32))
    dc = b.put(np.full(1, 0xFFFFFFFF, np.uint32))
    raw1 = k1.view(np.uint32).reshape(-1, 12) if len(k1) else np.zeros((1, 12), np.uint32)
    g.match_orb_dev(b.put(raw1), n1, b.put(k2.view(np.uint32).reshape(-1, 12)), n2, dm, dc, mm, md)
    b.sync()
    cnt = int(b.get(dc, np.uint32)[0])
    out = b.get(dm, np.uint32)
    assert cnt == len(exp), "%s: count %d, expected %d" % (what, cnt, len(exp))
    assert_same(out[:cnt].reshape(-1), exp.view(np.uint32).reshape(-1) if cnt else out[:0].reshape(-1), what)
    assert (out[cnt:] == MATCH_SENTINEL).all(), "%s: records at and beyond count were written" % what
    return cnt


def match_orb_dev(b, n1, n2):
    """gsh_match_orb_dev (keypoints, matches and count on the device) == gs_match_orb on pc.random_descriptors; records
    at and beyond `count` keep the sentinel; n1 == 0 and max_matches == 0 give count 0 and touch nothing; a cap below
    the number of hits keeps the first ones"""
    k1, k2 = pc.random_descriptors(n1, n2)
    what = "gsh_match_orb_dev %d x %d" % (n1, n2)
    for mm, md in ((n1 + 3, 60.0), (max(1, n1 // 2), 256.0), (n1, 2.0)):
        _match_dev_once(b, k1, n1, k2, n2, mm, md, "%s max=%d dist=%g" % (what, mm, md))
    hits = _match_dev_once(b, k1, n1, k2, n2, n1, 256.0, what + " all hits")
    if hits > 1:
        assert _match_dev_once(b, k1, n1, k2, n2, hits - 1, 256.0, what + " one fewer than the hits") == hits - 1
        assert _match_dev_once(b, k1, n1, k2, n2, 1, 256.0, what + " cap 1") == 1
    assert _match_dev_once(b, k1, 0, k2, n2, 7, 256.0, what + " n1 = 0") == 0
    assert _match_dev_once(b, k1, n1, k2, n2, 0, 256.0, what + " max_matches = 0") == 0


THRESHOLD_DEV_SHAPES = ((1, 1), (5, 1), (67, 45), (1031, 3), (2064, 5))
THRESHOLD_DEV_THR = (0, 1, 128, 254, 255)


def threshold_batch_dev(g, o, bufs, w, h, off):
    """gsh_threshold_batch_dev with one threshold per frame, inside sentinel-guarded buffers at byte offset `off`"""
    n = len(THRESHOLD_DEV_THR)
    rs = np.random.RandomState(w * 13 + h + off)
    img = rs.randint(0, 256, (n, h, w)).astype(np.uint8)
    img.reshape(n, -1)[:, :min(4, w * h)] = np.array([0, 1, 254, 255], np.uint8)[:min(4, w * h)]
    buf, v = bufs.make(n, h, w, off, img)
    tbuf, tv = bufs.make(1, 1, n, off, np.array(THRESHOLD_DEV_THR, np.uint8).reshape(1, 1, n))
    g.threshold_batch(v, tv)
    g.sync()
    got = bufs.host(v)
    for f, t in enumerate(THRESHOLD_DEV_THR):
        assert_same(got[f], o.threshold(img[f], t), "threshold_batch_dev %dx%d base+%d frame %d thr %d" % (w, h, off, f, t))
    assert bufs.guards_ok(buf, off, n * h * w), "threshold_batch_dev %dx%d base+%d wrote outside the frames" % (w, h, off)
    assert bufs.guards_ok(tbuf, off, n) and np.array_equal(bufs.host(tv).reshape(-1), THRESHOLD_DEV_THR)


# ======================================================================================================================
# B. unsynced chains
# ======================================================================================================================
def _run(b, steps, sync_each):
    """every input is uploaded; then the calls alone, with gsh_sync() after each one or with none until the end"""
    b.sync()
    for step in steps:
        step()
        if sync_each:
            b.g.sync()
    b.sync()


def _checksum(a):
    a = np.ascontiguousarray(a).reshape(-1)
    return np.sum(np.arange(1, a.size + 1, dtype=np.uint64) * (a.astype(np.uint64) + np.uint64(1)), dtype=np.uint64)


def chain1(b, sync_each, check=False):
    """SL_HISTP: histogram_batch (2 x 67x45) -> otsu_batch (9 x 612x96) -> edge_pipeline_batch(tmp = NULL) on
    40 x 1024x64 in chunks of 8 (five chunks: the side stream works) -> histogram_batch and checksum_batch of its output"""
    g, o = b.g, b.o
    A, B, Cf = synth_frames(67, 45, 2, 100), synth_frames(612, 96, 9, 200), synth_frames(1024, 64, 40, 300)
    dA, dB, dC = b.put(A), b.put(B), b.put(Cf)
    hist1, hist2, thr2 = b.put(np.zeros((2, 256), np.uint32)), b.put(np.zeros((9, 256), np.uint32)), b.put(np.zeros(9, np.uint8))
    dst, hist3, thr3 = b.put(np.full(Cf.shape, 7, np.uint8)), b.put(np.zeros((40, 256), np.uint32)), b.put(np.zeros(40, np.uint8))
    hist4, sums = b.put(np.zeros((40, 256), np.uint32)), b.put(np.zeros(40, np.uint64))

    def pipeline():
        g.tune(5, 8)
        g.edge_pipeline_batch(dst, None, dC, 2, hist3, thr3)

    try:
        _run(b, [lambda: g.histogram_batch(dA, hist1), lambda: g.otsu_batch(dB, hist2, thr2), pipeline,
                 lambda: g.histogram_batch(dst, hist4), lambda: g.checksum_batch(dst, sums)], sync_each)
    finally:
        g.tune(5, 0)
    out = dict(hist1=b.get(hist1, np.uint32), hist2=b.get(hist2, np.uint32), thr2=b.get(thr2), dst=b.get(dst),
               hist3=b.get(hist3, np.uint32), thr3=b.get(thr3), hist4=b.get(hist4, np.uint32), sums=b.get(sums, np.uint64))
    if check:
        for f in range(2):
            assert_same(out["hist1"][f], o.histogram(A[f]), "chain 1 step 1 frame %d" % f)
        for f in range(9):
            assert int(out["thr2"][f]) == o.otsu_threshold(B[f]), "chain 1 step 2 frame %d" % f
            assert_same(out["hist2"][f], o.histogram(B[f]), "chain 1 step 2 histogram %d" % f)
        for f in range(40):
            s = o.sobel(o.blur(Cf[f], 2))
            t = o.otsu_threshold(s)
            assert int(out["thr3"][f]) == t, "chain 1 step 3 frame %d" % f
            assert_same(out["hist3"][f], o.histogram(s), "chain 1 step 3 histogram %d" % f)
            e = o.threshold(s, t)
            assert_same(out["dst"][f], e, "chain 1 step 3 frame %d" % f)
            assert_same(out["hist4"][f], o.histogram(e), "chain 1 step 4 frame %d" % f)
            assert int(out["sums"][f]) == int(_checksum(e)), "chain 1 step 5 frame %d" % f
    return out


C2_ADAPT = (3, 70, 1366)  # ragged width; 3 x 70 x 1366 bytes are a prefix of the 6 x 96 x 612 of the step before


def chain2_inputs():
    return synth_frames(100, 33, 3, 400), synth_frames(612, 96, 6, 500)


def chain2(b, sync_each, check=False):
    """SL_AUX / SL_II: blur_sobel_batch r = 4 (unfused, 3 x 100x33) -> edge_pipeline_batch(tmp = NULL, r = 5) on
    6 x 612x96 -> blur_batch r = 9 by the integral route (key 6 = 3) -> adaptive_threshold_batch r = 13 on the same bytes
    read as 3 x 1366x70 with k_box_edge on the side stream (key 6 = 7) -> integral_batch"""
    g, o = b.g, b.o
    S1, S2 = chain2_inputs()
    d1, d2, d3 = b.put(np.full(S1.shape, 9, np.uint8)), b.put(np.full(S2.shape, 9, np.uint8)), b.put(np.full(S2.shape, 9, np.uint8))
    s1, s2 = b.put(S1), b.put(S2)
    hist2, thr2 = b.put(np.zeros((6, 256), np.uint32)), b.put(np.zeros(6, np.uint8))
    v3 = b.prefix(d3, *C2_ADAPT)
    d4, ii = b.put(np.full(C2_ADAPT, 9, np.uint8)), b.put(np.zeros(C2_ADAPT, np.uint32))

    def blur9():
        g.tune(6, 3)
        g.blur_batch(d3, d2, 9)

    def adaptive():
        g.tune(6, 7)
        g.adaptive_threshold_batch(d4, v3, 13, 5)

    try:
        _run(b, [lambda: g.blur_sobel_batch(d1, s1, 4), lambda: g.edge_pipeline_batch(d2, None, s2, 5, hist2, thr2), blur9,
                 adaptive, lambda: g.integral_batch(d4, ii)], sync_each)
    finally:
        g.tune(6, 0)
    out = dict(d1=b.get(d1), d2=b.get(d2), hist2=b.get(hist2, np.uint32), thr2=b.get(thr2), d3=b.get(d3), d4=b.get(d4),
               ii=b.get(ii, np.uint32))
    if check:
        for f in range(3):
            assert_same(out["d1"][f], o.sobel(o.blur(S1[f], 4)), "chain 2 step 1 frame %d" % f)
        e3 = np.zeros(S2.shape, np.uint8)
        for f in range(6):
            s = o.sobel(o.blur(S2[f], 5))
            t = o.otsu_threshold(s)
            assert int(out["thr2"][f]) == t, "chain 2 step 2 frame %d" % f
            assert_same(out["hist2"][f], o.histogram(s), "chain 2 step 2 histogram %d" % f)
            e2 = o.threshold(s, t)
            assert_same(out["d2"][f], e2, "chain 2 step 2 frame %d" % f)
            e3[f] = o.blur(e2, 9)
            assert_same(out["d3"][f], e3[f], "chain 2 step 3 frame %d" % f)
        n, h, w = C2_ADAPT
        for f, fr in enumerate(e3.reshape(-1)[:n * h * w].reshape(n, h, w)):
            e4 = o.adaptive_threshold(fr, 13, 5)
            assert_same(out["d4"][f], e4, "chain 2 step 4 frame %d" % f)
            assert_same(out["ii"][f], o.integral(e4), "chain 2 step 5 frame %d" % f)
    return out


def chain2_dropin(b, sync_each):
    """the drop-in gs_* calls of chain 2 on device pointers, frame by frame: gs_blur(4) -> gs_sobel -> gs_blur(9, integral
    route) -> gs_adaptive_threshold(13, k_box_edge on the side stream) -> gs_integral.  (gs_histogram and
    gs_otsu_threshold hand their result to the host, so they end an unsynced stretch by definition and stay out.)
    The caller switches gsh_set_async on for the unsynced run."""
    g = b.g
    _, S2 = chain2_inputs()
    S2 = S2[:3]
    s = b.put(S2)
    t1, t2, t3, t4 = (b.put(np.zeros(S2.shape, np.uint8)) for _ in range(4))
    ii = b.put(np.zeros(S2.shape, np.uint32))
    steps = []
    for f in range(len(S2)):
        steps += [lambda f=f: g.blur(t1[f], s[f], 4), lambda f=f: g.sobel(t2[f], t1[f]),
                  lambda f=f: (g.tune(6, 3), g.blur(t3[f], t2[f], 9)),
                  lambda f=f: (g.tune(6, 7), g.adaptive_threshold(t4[f], t3[f], 13, 5)), lambda f=f: g.integral(t4[f], ii[f])]
    try:
        _run(b, steps, sync_each)
    finally:
        g.tune(6, 0)
    return dict(t1=b.get(t1), t2=b.get(t2), t3=b.get(t3), t4=b.get(t4), ii=b.get(ii, np.uint32)), S2


def check_chain2_dropin(o, out, S2):
    for f, img in enumerate(S2):
        e1 = o.blur(img, 4)
        e2 = o.sobel(e1)
        e3 = o.blur(e2, 9)
        e4 = o.adaptive_threshold(e3, 13, 5)
        for name, e in (("t1", e1), ("t2", e2), ("t3", e3), ("t4", e4), ("ii", o.integral(e4))):
            assert_same(out[name][f], e, "drop-in chain frame %d %s" % (f, name))


C3_LBP = ((4096, 1.2, 1.0, 3.0, 2), (300, 1.1, 1.0, 2.0, 1), (4096, 1.2, 1.0, 3.0, 1))
C3_NKPS = 60


def chain3(b, sync_each, casc, check=False):
    """SL_MASK / SL_CNT / SL_PAD: integral_batch -> lbp_detect_batch (frontal face on 3 x 320x200, a random cascade on
    2 x 96x80, frontal face again at another step) -> fast_batch on 5 x 260x17, then on 3 x 640x480 ->
    orb_extract_batch_nostdlib -> match_orb_dev on the keypoint records of its frames 0 and 1"""
    g, o = b.g, b.o
    F1, F2 = synth_frames(320, 200, 3, 600), synth_frames(96, 80, 2, 700)
    G1 = np.random.RandomState(17).randint(0, 256, (5, 17, 260)).astype(np.uint8)
    G2 = synth_frames(640, 480, 3, 800)
    rc = random_cascade(1)
    dcs = [g.cascade_create(casc), g.cascade_create(rc)]
    f1, f2, g1, g2 = b.put(F1), b.put(F2), b.put(G1), b.put(G2)
    ii1, ii2 = b.put(np.zeros(F1.shape, np.uint32)), b.put(np.zeros(F2.shape, np.uint32))
    plan = ((dcs[0], ii1, 3), (dcs[1], ii2, 2), (dcs[0], ii1, 3))
    rects = [b.put(np.zeros((n, p[0], 4), np.uint32)) for (_, _, n), p in zip(plan, C3_LBP)]
    rcnt = [b.put(np.zeros(n, np.uint32)) for (_, _, n) in plan]
    sm1, k1, c1 = b.put(np.zeros(G1.shape, np.uint8)), b.put(np.zeros((5, 200, 12), np.uint32)), b.put(np.zeros(5, np.uint32))
    sm2, k2, c2 = b.put(np.zeros(G2.shape, np.uint8)), b.put(np.zeros((3, 800, 12), np.uint32)), b.put(np.zeros(3, np.uint32))
    sm3, k3, c3 = b.put(np.zeros(G2.shape, np.uint8)), b.put(np.zeros((3, C3_NKPS, 12), np.uint32)), b.put(np.zeros(3, np.uint32))
    mt, mc = b.put(np.full((C3_NKPS + 4, 3), MATCH_SENTINEL, np.uint32)), b.put(np.full(1, 0xFFFFFFFF, np.uint32))
    steps = [lambda: g.integral_batch(f1, ii1), lambda: g.integral_batch(f2, ii2)]
    for i, ((dc, ii, n), p) in enumerate(zip(plan, C3_LBP)):
        steps.append(lambda i=i, dc=dc, ii=ii, p=p: g.lbp_detect_batch(dc, ii, rects[i], rcnt[i], *p))
    steps += [lambda: g.fast_batch(g1, sm1, k1, c1, 200, 20), lambda: g.fast_batch(g2, sm2, k2, c2, 800, 20),
              lambda: g.orb_extract_batch_nostdlib(g2, sm3, k3, c3, C3_NKPS, 20),
              # n1 = n2 = the cap: the counts are still on the device; records beyond a frame's count are the zeros they were
              lambda: g.match_orb_dev(k3[0], C3_NKPS, k3[1], C3_NKPS, mt, mc, C3_NKPS, 80.0)]
    try:
        _run(b, steps, sync_each)
        out = dict(ii1=b.get(ii1, np.uint32), ii2=b.get(ii2, np.uint32), sm1=b.get(sm1), k1=b.get(k1, np.uint32),
                   c1=b.get(c1, np.uint32), sm2=b.get(sm2), k2=b.get(k2, np.uint32), c2=b.get(c2, np.uint32), sm3=b.get(sm3),
                   k3=b.get(k3, np.uint32), c3=b.get(c3, np.uint32), mt=b.get(mt, np.uint32), mc=b.get(mc, np.uint32))
        for i in range(3):
            out["rects%d" % i], out["rcnt%d" % i] = b.get(rects[i], np.uint32), b.get(rcnt[i], np.uint32)
    finally:
        for dc in dcs:
            dc.close()
    if check:
        for f in range(3):
            assert_same(out["ii1"][f], o.integral(F1[f]), "chain 3 integral %d" % f)
        for i, (frames, c) in enumerate(((F1, casc), (F2, rc), (F1, casc))):
            for f, img in enumerate(frames):
                ro = o.lbp_detect(c, o.integral(img), *C3_LBP[i])
                assert int(out["rcnt%d" % i][f]) == len(ro), "chain 3 lbp call %d frame %d: count" % (i, f)
                assert_same(out["rects%d" % i][f, :len(ro)], rects_u32(ro), "chain 3 lbp call %d frame %d" % (i, f))
        for frames, sm, k, c, cap, tag in ((G1, "sm1", "k1", "c1", 200, "260x17"), (G2, "sm2", "k2", "c2", 800, "640x480")):
            for f, img in enumerate(frames):
                ko, smo = o.fast(img, cap, 20)
                assert int(out[c][f]) == len(ko), "chain 3 fast %s frame %d: count" % (tag, f)
                assert_same(out[k][f, :len(ko)].reshape(-1), ko.view(np.uint32).reshape(-1), "chain 3 fast %s frame %d" % (tag, f))
                assert_same(out[sm][f], smo, "chain 3 fast %s score map %d" % (tag, f))
        ns = port_nostdlib()
        padded = np.zeros((3, C3_NKPS), KEYPOINT_DTYPE)
        for f, img in enumerate(G2):
            ko = ns.orb_extract(img, C3_NKPS, 20)
            assert int(out["c3"][f]) == len(ko), "chain 3 orb frame %d: count" % f
            padded[f, :len(ko)] = ko
            assert_same(out["k3"][f].reshape(-1), padded[f].view(np.uint32).reshape(-1), "chain 3 orb frame %d" % f)
        mo = o.match_orb(padded[0], padded[1], C3_NKPS, 80.0)
        assert int(out["mc"][0]) == len(mo) and len(mo) > 0, "chain 3 match count"
        assert_same(out["mt"][:len(mo)].reshape(-1), mo.view(np.uint32).reshape(-1), "chain 3 matches")
        assert (out["mt"][len(mo):] == MATCH_SENTINEL).all()
    return out


C4_CAP, C4_DW, C4_DH = 300, 40, 30


def chain4_frames():
    rng = np.random.default_rng(44)
    passes = []
    for n, h, w in ((7, 97, 203), (3, 250, 517)):
        masks = []
        for f in range(n):
            kind = f % 4
            masks.append(cc.upscaled_noise(rng, h, w, 3) if kind == 0 else cc.random_discs(rng, h, w, 12, 3, 14) if kind == 1
                         else bc.random_mask(rng, h, w, 0.5) if kind == 2 else cc.random_rects(rng, h, w, 10))
        noise = rng.integers(0, 50, (n, h, w))
        gray = (np.where(np.stack(masks) > 0, 200, 20) + noise).astype(np.uint8)  # 20..69 or 200..249
        thr = np.array([70 + 18 * f for f in range(n)], np.uint8)                 # all of them cut between the two
        passes.append((gray, thr))
    return passes


def _blobs_ref(img, cap):
    from oracle import pyoracle
    return bc.Ref().blobs(img, cap) if pyoracle.have_reference() else bc.spec_blobs(img, cap)


def chain4(b, sync_each, check=False):
    """components: threshold_batch_dev -> blobs_batch(cap 300) -> blob_contour_starts_batch -> trace_contours_batch ->
    blob_corners_batch (of each frame's first blob, gathered on the stream by gs_crop over the records' bytes) ->
    perspective_correct_batch, on 7 x 203x97 and then on 3 x 517x250 with no sync in between"""
    g, o = b.g, b.o
    passes = chain4_frames()
    steps, bufs = [], []
    for gray, thr in passes:
        n, h, w = gray.shape
        d = dict(src=b.put(gray), orig=b.put(gray), thr=b.put(thr), lab=b.put(np.zeros(gray.shape, np.int16)),
                 blobs=b.put(np.zeros((n, C4_CAP, 8), np.int32)), counts=b.put(np.zeros(n, np.int32)),
                 cont=b.put(np.zeros((n, C4_CAP, 7), np.int32)), vis=b.put(np.zeros(gray.shape, np.uint8)),
                 st=b.put(np.full((n, C4_CAP), 77, np.uint8)), first=b.put(np.zeros((n, 8), np.int32)),
                 corners=b.put(np.zeros((n, 4, 2), np.int32)), out=b.put(np.zeros((n, C4_DH, C4_DW), np.uint8)))
        bufs.append(d)
        steps += [lambda d=d: g.threshold_batch(d["src"], d["thr"]),
                  lambda d=d: g.blobs_batch(d["src"], d["lab"], d["blobs"], d["counts"], C4_CAP),
                  lambda d=d: g.blob_contour_starts_batch(d["lab"], d["blobs"], d["counts"], d["cont"]),
                  lambda d=d: g.trace_contours_batch(d["src"], d["vis"], d["cont"], d["counts"], d["st"]),
                  lambda d=d, n=n: g.crop(b.bytes2d(d["first"], n), b.bytes2d(d["blobs"], n), 0, 0, 32, n),
                  lambda d=d: g.blob_corners_batch(d["src"], d["lab"], d["first"], d["corners"]),
                  lambda d=d: g.perspective_correct_batch(d["out"], d["orig"], d["corners"])]
    g.set_async(True)  # gs_crop on device pointers must not end in a stream sync of its own
    try:
        _run(b, steps, sync_each)
    finally:
        g.set_async(False)
    out = {}
    for p, d in enumerate(bufs):
        for k, v in d.items():
            out["%s%d" % (k, p)] = b.get(v)
    if check:
        for p, (gray, thr) in enumerate(passes):
            n = len(gray)
            recs_all = np.ascontiguousarray(out["blobs%d" % p]).view(BLOB_DTYPE).reshape(n, C4_CAP)
            cont_all = np.ascontiguousarray(out["cont%d" % p]).view(CONTOUR_DTYPE).reshape(n, C4_CAP)
            for f in range(n):
                what = "chain 4 pass %d frame %d" % (p, f)
                binary = o.threshold(gray[f], int(thr[f]))
                assert_same(out["src%d" % p][f], binary, what + " threshold")
                recs, labels = _blobs_ref(binary, C4_CAP)
                m = int(out["counts%d" % p][f])
                bc.assert_blobs_equal((recs_all[f, :m], out["lab%d" % p][f].view(np.uint16)), (recs, labels), what)
                starts = [(int(np.nonzero(labels[int(r["y"])] == r["label"])[0][0]), int(r["y"])) for r in recs]
                assert [(int(r["sx"]), int(r["sy"])) for r in cont_all[f, :m]] == starts, what + " starts"
                want, want_vis, _ = cc.expected_sequence(binary, starts)  # endless walks: the restatement's limit values
                cc.assert_sequence_equal([cc.rec_tuple(r) for r in cont_all[f, :m]], out["vis%d" % p][f], want, want_vis, what,
                                         got_status=out["st%d" % p][f])
                assert (out["st%d" % p][f, m:] == 77).all()
                assert m > 0, what
                corners = bc.spec_corners(binary, labels, recs[0])
                assert [tuple(c) for c in out["corners%d" % p][f].tolist()] == corners, what + " corners"
                assert_same(out["out%d" % p][f], bc.spec_perspective(C4_DW, C4_DH, gray[f], corners), what + " perspective")
    return out


def assert_runs_equal(a, c, what):
    assert a.keys() == c.keys()
    for k in a:
        assert a[k].tobytes() == c[k].tobytes(), "%s: buffer %s of the unsynced run differs from the synced run" % (what, k)


def chain_pair(b, chain, what, **kw):
    """`chain` with gsh_sync() after every call, checked against the oracle step by step; then with no sync until the end:
    every buffer byte-identical"""
    ref = chain(b, True, check=True, **kw)
    assert_runs_equal(chain(b, False, **kw), ref, what)
    return ref


# ======================================================================================================================
# C. history independence
# ======================================================================================================================
def _lbp_batch(b, dc, ii, cap, sf, mn, mx, step):
    n = ii.shape[0]
    rects, counts = b.put(np.zeros((n, cap, 4), np.uint32)), b.put(np.zeros(n, np.uint32))
    b.g.lbp_detect_batch(dc, b.put(ii), rects, counts, cap, sf, mn, mx, step)
    b.sync()
    return b.get(rects, np.uint32), b.get(counts, np.uint32)


def _check_lbp_batch(b, casc, dc, frames, params, what):
    ii = np.stack([b.o.integral(f) for f in frames])
    r, c = _lbp_batch(b, dc, ii, *params)
    for f in range(len(frames)):
        ro = b.o.lbp_detect(casc, ii[f], *params)
        assert int(c[f]) == len(ro), "%s frame %d: %d rects, expected %d" % (what, f, int(c[f]), len(ro))
        assert_same(r[f, :len(ro)], rects_u32(ro), "%s frame %d" % (what, f))
    return int(c.sum())


def _sparse_frames():
    """a few bright rectangles on grey under a little noise (a score is the SMALLEST ring difference, 0 without it): a
    handful of corners per frame"""
    rng = np.random.default_rng(90)
    return np.stack([(cc.random_rects(rng, 80, 96, 4, 8, 25) // 2 + rng.integers(60, 69, (80, 96))).astype(np.uint8) for f in range(2)])


def probe_fast_batch(b, casc):
    img = _sparse_frames()
    sm, k, c = b.put(np.zeros(img.shape, np.uint8)), b.put(np.zeros((2, 64, 12), np.uint32)), b.put(np.zeros(2, np.uint32))
    b.g.fast_batch(b.put(img), sm, k, c, 64, 20)
    b.sync()
    total = 0
    for f in range(2):
        ko, smo = b.o.fast(img[f], 64, 20)
        assert int(b.get(c, np.uint32)[f]) == len(ko), "probe fast_batch frame %d: count" % f
        assert_same(b.get(k, np.uint32)[f, :len(ko)].reshape(-1), ko.view(np.uint32).reshape(-1), "probe fast_batch frame %d" % f)
        assert_same(b.get(sm)[f], smo, "probe fast_batch score map %d" % f)
        total += len(ko)
    assert 0 < total < 100


def probe_lbp_batch(b, casc):
    rc = random_cascade(5, permissive=False)
    for c, frames, params in ((rc, synth_frames(96, 80, 2, 9), (200, 1.2, 1.0, 2.5, 2)),
                              (casc, synth_frames(160, 120, 1, 4), (64, 1.2, 1.0, 3.0, 1))):
        dc = b.g.cascade_create(c)
        try:
            _check_lbp_batch(b, c, dc, frames, params, "probe lbp_detect_batch")
        finally:
            dc.close()


def probe_lbp_dropin(b, casc):
    rc = random_cascade(5, permissive=False)
    for c, img, params in ((rc, Oracle.synth(96, 80, 9), (200, 1.2, 1.0, 2.5, 2)), (casc, Oracle.synth(160, 120, 4), (64, 1.2, 1.0, 3.0, 1))):
        ii = b.o.integral(img)
        assert_same(b.g.lbp_detect(c, b.put(ii), *params), b.o.lbp_detect(c, ii, *params), "probe gs_lbp_detect")


def probe_orb_batch(b, casc):
    img = _sparse_frames()
    got = b.g.orb_extract_batch_dev(b.put(img), b.put(np.zeros(img.shape, np.uint8)), 20, 20)
    total = 0
    for f in range(2):
        ko = b.o.orb_extract(img[f], 20, 20)
        assert_same(got[f], ko, "probe orb_extract_batch frame %d" % f)
        total += len(ko)
    assert total > 0


def probe_match(b, casc):
    k1, k2 = pc.random_descriptors(5, 63)
    assert_same(b.g.match_orb(k1, k2, 8, 60.0), b.o.match_orb(k1, k2, 8, 60.0), "probe gs_match_orb")
    assert _match_dev_once(b, k1, 5, k2, 63, 8, 60.0, "probe gsh_match_orb_dev") > 0


def probe_otsu(b, casc):
    img = synth_frames(67, 45, 2, 21)
    hist, thr = b.put(np.zeros((2, 256), np.uint32)), b.put(np.zeros(2, np.uint8))
    b.g.otsu_batch(b.put(img), hist, thr)
    b.sync()
    for f in range(2):
        assert int(b.get(thr)[f]) == b.o.otsu_threshold(img[f]), "probe otsu_batch frame %d" % f
        assert_same(b.get(hist, np.uint32)[f], b.o.histogram(img[f]), "probe otsu_batch histogram %d" % f)


def probe_checksum(b, casc):
    img = synth_frames(67, 45, 2, 22)
    sums = b.put(np.zeros(2, np.uint64))
    b.g.checksum_batch(b.put(img), sums)
    b.sync()
    for f in range(2):
        assert int(b.get(sums, np.uint64)[f]) == int(_checksum(img[f])), "probe checksum_batch frame %d" % f


def _probe_masks():
    return np.stack([cc.random_discs(np.random.default_rng(5 + f), 40, 60, 4, 2, 6) for f in range(2)])


def probe_blobs(b, casc):
    img = _probe_masks()
    lab, recs, cnt = b.put(np.zeros(img.shape, np.int16)), b.put(np.zeros((2, 20, 8), np.int32)), b.put(np.zeros(2, np.int32))
    b.g.blobs_batch(b.put(img), lab, recs, cnt, 20)
    b.sync()
    got = np.ascontiguousarray(b.get(recs)).view(BLOB_DTYPE).reshape(2, 20)
    for f in range(2):
        m = int(b.get(cnt)[f])
        assert m > 0
        bc.assert_blobs_equal((got[f, :m], b.get(lab)[f].view(np.uint16)), bc.spec_blobs(img[f], 20), "probe blobs_batch frame %d" % f)


def _trace(b, imgs, starts):
    n, per = len(imgs), max(1, max(len(s) for s in starts))
    recs = np.zeros((n, per), CONTOUR_DTYPE)
    for f, ss in enumerate(starts):
        for k, s in enumerate(ss):
            recs[f, k]["sx"], recs[f, k]["sy"] = s
    d_rec, d_vis = b.put(recs.view(np.int32).reshape(n, per, 7)), b.put(np.zeros(imgs.shape, np.uint8))
    d_st = b.put(np.full((n, per), 77, np.uint8))
    b.g.trace_contours_batch(b.put(imgs), d_vis, d_rec, b.put(np.array([len(s) for s in starts], np.int32)), d_st)
    b.sync()
    return np.ascontiguousarray(b.get(d_rec)).view(CONTOUR_DTYPE).reshape(n, per), b.get(d_vis), b.get(d_st)


def probe_trace(b, casc):
    img = _probe_masks()
    starts = [cc.start_pixels(f) for f in img]
    got, vis, st = _trace(b, img, starts)
    for f in range(2):
        want, want_vis, _ = cc.expected_sequence(img[f], starts[f])
        cc.assert_sequence_equal([cc.rec_tuple(r) for r in got[f, :len(starts[f])]], vis[f], want, want_vis,
                                 "probe trace_contours_batch frame %d" % f, got_status=st[f])


def probe_synth(b, casc):
    d = b.put(np.zeros((2, 45, 67), np.uint8))
    b.g.synth_batch(d, 5)
    b.sync()
    assert_same(b.get(d), synth_frames(67, 45, 2, 5), "probe synth_batch")


# ---- the dirtying calls: larger, denser inputs that set as many mask, count and partial words as they can ----------
def _noise(shape, seed=1):
    return np.random.RandomState(seed).randint(0, 256, shape).astype(np.uint8)


def dirty_fast(b, casc):
    img = _noise((4, 120, 200))
    b.g.fast_batch(b.put(img), b.put(np.zeros(img.shape, np.uint8)), b.put(np.zeros((4, 5000, 12), np.uint32)),
                   b.put(np.zeros(4, np.uint32)), 5000, 5)
    b.sync()


def _edge_integrals(b, n, w, h):
    return np.stack([b.o.integral(b.o.sobel(Oracle.synth(w, h, 30 + f))) for f in range(n)])


def dirty_lbp(b, casc):
    dc = b.g.cascade_create(random_cascade(1))
    try:
        _, c = _lbp_batch(b, dc, _edge_integrals(b, 2, 200, 150), 100000, 1.1, 1.0, 4.0, 1)
        assert int(c.sum()) > 5000  # it really was dense
    finally:
        dc.close()


def dirty_lbp_dropin(b, casc):
    assert len(b.g.lbp_detect(random_cascade(1), b.put(_edge_integrals(b, 1, 200, 150)[0]), 100000, 1.1, 1.0, 4.0, 1)) > 2500


def dirty_orb(b, casc):
    img = _noise((2, 120, 200), 2)
    b.g.orb_extract_batch_dev(b.put(img), b.put(np.zeros(img.shape, np.uint8)), 1000, 5)


def dirty_match(b, casc):
    """all-equal descriptors (every best distance 0, every ratio test a tie), then a train set that is a copy of the query
    set (every query matches: every mask bit set), through both entry points"""
    n = 700
    k1 = np.zeros(n, KEYPOINT_DTYPE)
    k1.view(np.uint32).reshape(n, 12)[:, 4:] = 0x5A5A5A5A
    b.g.match_orb(k1, k1, n, 256.0)
    k2, _ = pc.random_descriptors(n, 2)
    assert len(b.g.match_orb(k2, k2, n, 256.0)) == n
    _match_dev_once(b, k2, n, k2, n, n, 256.0, "dirtying gsh_match_orb_dev")


def dirty_otsu(b, casc):
    img = _noise((6, 96, 612), 3)
    b.g.otsu_batch(b.put(img), b.put(np.zeros((6, 256), np.uint32)), b.put(np.zeros(6, np.uint8)))
    b.sync()


def dirty_hist(b, casc):
    b.g.histogram_batch(b.put(_noise((6, 96, 612), 4)), b.put(np.zeros((6, 256), np.uint32)))
    b.sync()


def dirty_pipeline(b, casc):
    img = _noise((6, 64, 256), 5)
    for tmp in (None, b.put(np.zeros(img.shape, np.uint8))):
        b.g.edge_pipeline_batch(b.put(np.zeros(img.shape, np.uint8)), tmp, b.put(img), 2, b.put(np.zeros((6, 256), np.uint32)),
                                b.put(np.zeros(6, np.uint8)))
        b.sync()


def dirty_checksum(b, casc):
    b.g.checksum_batch(b.put(_noise((5, 64, 1024), 6)), b.put(np.zeros(5, np.uint64)))
    b.sync()


def dirty_tmatch(b, casc):
    img = _noise((96, 128), 7)
    b.g.match_template(b.put(img), b.put(_noise((16, 16), 8)), b.put(np.zeros((81, 113), np.uint8)))
    b.sync()


def dirty_integral_host(b, casc):
    b.g.integral(_noise((96, 128), 9))


def dirty_blobs(b, casc):
    img = np.stack([bc.checkerboard(64, 128)] * 3)
    b.g.blobs_batch(b.put(img), b.put(np.zeros(img.shape, np.int16)), b.put(np.zeros((3, 5000, 8), np.int32)),
                    b.put(np.zeros(3, np.int32)), 5000)
    b.sync()


def dirty_trace(b, casc):
    img = np.stack([cc.random_mask(np.random.default_rng(70 + f), 100, 120, 0.6) for f in range(2)])
    _trace(b, img, [cc.start_pixels(f) for f in img])


def dirty_synth(b, casc):
    b.g.synth_batch(b.put(np.zeros((4, 100, 300), np.uint8)), 99)
    b.sync()


_COMPACTORS = (dirty_fast, dirty_lbp, dirty_lbp_dropin, dirty_orb, dirty_match)
# probe -> (the dirtying call of the same entry point, those of the other entry points that share one of its slots)
HISTORY = {
    "fast_batch": (probe_fast_batch, (dirty_fast, dirty_lbp, dirty_lbp_dropin, dirty_orb, dirty_match, dirty_checksum, dirty_tmatch)),
    "lbp_detect_batch": (probe_lbp_batch, (dirty_lbp, dirty_lbp_dropin, dirty_fast, dirty_orb, dirty_match, dirty_tmatch,
                                          dirty_integral_host)),
    "gs_lbp_detect": (probe_lbp_dropin, (dirty_lbp_dropin, dirty_lbp, dirty_fast, dirty_orb, dirty_match, dirty_tmatch,
                                        dirty_integral_host)),
    "orb_extract_batch": (probe_orb_batch, (dirty_orb, dirty_fast, dirty_lbp, dirty_lbp_dropin, dirty_match, dirty_checksum)),
    "match_orb": (probe_match, (dirty_match, dirty_fast, dirty_lbp, dirty_lbp_dropin, dirty_orb, dirty_tmatch, dirty_checksum)),
    "otsu_batch": (probe_otsu, (dirty_otsu, dirty_hist, dirty_pipeline)),
    "checksum_batch": (probe_checksum, (dirty_checksum, dirty_tmatch) + _COMPACTORS),
    "blobs_batch": (probe_blobs, (dirty_blobs,)),
    "trace_contours_batch": (probe_trace, (dirty_trace, dirty_blobs)),
    "synth_batch": (probe_synth, (dirty_synth,)),
}


def history_independence(b, casc, name):
    """the probe call right after gsh_shutdown(), then after each dirtying call: always the oracle's result"""
    probe, dirtiers = HISTORY[name]
    b.sync()
    b.g.shutdown()
    probe(b, casc)
    for dirty in dirtiers:
        dirty(b, casc)
        try:
            probe(b, casc)
        except AssertionError as e:
            raise AssertionError("after %s: %s" % (dirty.__name__, e)) from e
    b.g.shutdown()  # ... and the probe once more on fresh scratch after all of it (jump table, caches rebuilt)
    probe(b, casc)


LBP_KEY_STEPS = (("base", (96, 80, 1.2, 1.0, 3.0, 2)), ("iw", (104, 80, 1.2, 1.0, 3.0, 2)), ("ih", (104, 72, 1.2, 1.0, 3.0, 2)),
                 ("sf", (104, 72, 1.3, 1.0, 3.0, 2)), ("mn", (104, 72, 1.3, 1.5, 3.0, 2)), ("mx", (104, 72, 1.3, 1.5, 2.5, 2)),
                 ("step", (104, 72, 1.3, 1.5, 2.5, 1)), ("step", (104, 72, 1.3, 1.5, 2.5, 3)))


def lbp_geometry_cache_key(b):
    """one handle, consecutive calls that differ in ONE field of the geometry cache's key (iw, ih, sf, mn, mx, step)"""
    rc = random_cascade(1)
    dc = b.g.cascade_create(rc)
    try:
        seen = []
        for field, (iw, ih, sf, mn, mx, step) in LBP_KEY_STEPS:
            frames = synth_frames(iw, ih, 2, 12)
            total = _check_lbp_batch(b, rc, dc, frames, (4096, sf, mn, mx, step), "geometry cache after changing %s" % field)
            assert total > 0
            seen.append(total)
        assert len(set(seen)) > len(seen) // 2  # the fields do matter on this input
    finally:
        dc.close()


def dropin_cascade_edited_in_place(b):
    """gs_lbp_detect re-reads the caller's tables on every call (ref :790-835): an edit of stage_threshold[0] IN PLACE, same
    struct and same array addresses, must show in the next call"""
    rc = copy.deepcopy(random_cascade(1))
    rc._struct = None
    ii = b.o.integral(Oracle.synth(96, 80, 12))
    params = (4096, 1.2, 1.0, 3.0, 1)
    first = b.g.lbp_detect(rc, b.put(ii), *params)
    assert_same(first, b.o.lbp_detect(rc, ii, *params), "gs_lbp_detect before the edit")
    addr = rc.stage_threshold.ctypes.data
    rc.stage_threshold[0] = 0.4
    assert rc.stage_threshold.ctypes.data == addr
    second = b.g.lbp_detect(rc, b.put(ii), *params)
    exp = b.o.lbp_detect(rc, ii, *params)
    assert len(exp) != len(first), "the edit does not change the oracle's result: the case checks nothing"
    assert_same(second, exp, "gs_lbp_detect after stage_threshold[0] was edited in place")


# ======================================================================================================================
# D. switching streams (GPU only)
# ======================================================================================================================
def stream_switch(b):
    """Work queued on stream A (otsu_batch on 64 x 1920x1080, lbp_detect_batch on 8 integral tables), then with no host sync
    the same entry points on stream B (2 x 67x45, one 96x80 table, the SAME cascade handle, so the geometry tables, the
    partial histograms and the compaction words are all shared), then histogram_batch on the library's own stream.
    Scratch belongs to the thread, so gsh_set_stream has to order B behind A and the own stream behind B: every output
    equals the oracle's.  A race test: a pass does not prove the order, a failure disproves it."""
    import torch
    g, o = b.g, b.o
    rc = random_cascade(1)
    big = torch.empty((64, 1080, 1920), dtype=torch.uint8, device="cuda")
    g.synth_batch(big, 1000)
    FA, FB, FC = synth_frames(640, 480, 8, 40), synth_frames(96, 80, 1, 60), synth_frames(67, 45, 2, 70)
    SB = synth_frames(67, 45, 2, 80)
    iiA, iiB = np.stack([o.integral(f) for f in FA]), np.stack([o.integral(f) for f in FB])
    d_iiA, d_iiB, d_sb, d_fc = b.put(iiA), b.put(iiB), b.put(SB), b.put(FC)
    histA, thrA = b.put(np.zeros((64, 256), np.uint32)), b.put(np.zeros(64, np.uint8))
    histB, thrB = b.put(np.zeros((2, 256), np.uint32)), b.put(np.zeros(2, np.uint8))
    rA, cA = b.put(np.zeros((8, 4096, 4), np.uint32)), b.put(np.zeros(8, np.uint32))
    rB, cB = b.put(np.zeros((1, 4096, 4), np.uint32)), b.put(np.zeros(1, np.uint32))
    histC = b.put(np.zeros((2, 256), np.uint32))
    pA, pB = (4096, 1.1, 1.0, 4.0, 1), (4096, 1.2, 1.0, 2.0, 2)
    dc = g.cascade_create(rc)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    b.sync()
    big_host = big.cpu().numpy()
    try:
        g.set_stream(sa.cuda_stream)
        g.otsu_batch(big, histA, thrA)
        g.lbp_detect_batch(dc, d_iiA, rA, cA, *pA)
        g.set_stream(sb.cuda_stream)
        g.otsu_batch(d_sb, histB, thrB)
        g.lbp_detect_batch(dc, d_iiB, rB, cB, *pB)
        g.set_stream(None)
        g.histogram_batch(d_fc, histC)
        sa.synchronize(), sb.synchronize()
        b.sync()
    finally:
        g.set_stream(None)
        torch.cuda.synchronize()
        dc.close()
    bad = []
    tA, hA = b.get(thrA), b.get(histA, np.uint32)
    for f in range(64):
        if int(tA[f]) != o.otsu_threshold(big_host[f]) or not np.array_equal(hA[f], o.histogram(big_host[f])):
            bad.append("A otsu frame %d" % f)
    for tag, frames, ii, r, c, p in (("A", FA, iiA, rA, cA, pA), ("B", FB, iiB, rB, cB, pB)):
        rr, cc_ = b.get(r, np.uint32), b.get(c, np.uint32)
        for f in range(len(frames)):
            ro = o.lbp_detect(rc, ii[f], *p)
            assert len(ro) > 0
            if int(cc_[f]) != len(ro) or not np.array_equal(rr[f, :len(ro)], rects_u32(ro)):
                bad.append("%s lbp table %d (%d rects, expected %d)" % (tag, f, int(cc_[f]), len(ro)))
    for f in range(2):
        if int(b.get(thrB)[f]) != o.otsu_threshold(SB[f]) or not np.array_equal(b.get(histB, np.uint32)[f], o.histogram(SB[f])):
            bad.append("B otsu frame %d" % f)
        if not np.array_equal(b.get(histC, np.uint32)[f], o.histogram(FC[f])):
            bad.append("own-stream histogram frame %d" % f)
    assert not bad, "%d outputs differ from the oracle after the stream switches: %s" % (len(bad), ", ".join(bad[:12]))
