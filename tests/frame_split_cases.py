"""Shared cases of tests/test_frame_split.py (emulator) and tests/test_gpu_frame_split.py (MI355X): every gsh_*_batch entry
with more than one launch per call, every frame of every output against the oracle's single-frame function on that frame.

Every batch entry cuts its n frames into launches through `for_frames` (gs_internal.h); each launch after the first takes
its pointers at `f0` frames into the caller's arrays (thr + f0, hist + f0 * 256, counts + f0, rects + f0 * max_rects * 4,
a scratch plane, seed0 + f0) and its geometry from `nn`, the frames of this launch.  gsh_tune key 8 caps the frames of a
launch: a case runs its call under key 8 = 0 (one launch), 1 (7 launches of one frame), 2 (2 + 2 + 2 + 1) and 3 (3 + 3 + 1).

`b` is a guard_cases.Backend: a bound library, the oracle, guarded device memory (numpy for the emulator) and guarded host
memory.  Every output starts as SENTINEL bytes between guards (guard_cases.Guarded.make; in-place entries start as their
input), every input lies between guards too and is compared with its copy afterwards.  `_check` first names the frames of
an output that still hold their prefill although the oracle changes them -- a launch that never ran, or ran somewhere else
-- and then compares the whole output and both guards with the expectation (util.first_diff's message through
Guarded.check).  The expectation of a frame never comes from the library.

What a case asserts about its own inputs, with the oracle alone (`_distinct`, `_records`): the expected outputs of any two
frames differ (a result written one frame off cannot match), every frame of a record output has a record, and under a
cap that is part of the case one frame is capped and one is not.

A case is (id, run); run(b, splits) makes the call once per value of key 8 in `splits`.  The id names the route the shape
takes by the launcher's rule (gs_stencil.cpp, gs_detect.cpp): w = 20 the per-pixel fallbacks (strip_ok wants 32 columns),
64 whole 16-pixel strips, 68 ragged rows at dword-aligned addresses, 67 rows at any byte phase."""
import contextlib
import functools

import numpy as np

import guard_cases as gd
import tmatch_batch_cases as tb
from grayskull_amd import KEYPOINT_DTYPE, RECT_DTYPE
from oracle import pyoracle
from oracle.pyoracle import Oracle
from parity_cases import Mem
from util import random_cascade

N, H = 7, 24
SPLITS = (0, 1, 2, 3)
SENTINEL = 0x5A
WIDTHS = ((20, "px"), (64, "strips"), (68, "ragged_dword_rows"), (67, "any_byte_phase"))


def launches(n, split):
    """the frames of each launch of a call with n frames under key 8 = split"""
    step = split if split > 0 else 32768
    return [min(step, n - f0) for f0 in range(0, n, step)]


assert [launches(N, s) for s in SPLITS] == [[7], [1] * 7, [2, 2, 2, 1], [3, 3, 1]]


@functools.lru_cache(maxsize=None)
def frames(seed, n, h, w):
    """n different frames like geom_batch_cases.frames -- noise over a row, column and frame ramp -- with a noise amplitude
    that grows with the frame, so that histograms and Otsu thresholds differ from frame to frame as well"""
    rng = np.random.default_rng(seed)
    amp = (40 + (np.arange(n) * 211 // max(n - 1, 1)))[:, None, None]
    a = (rng.integers(0, 256, (n, h, w)) * amp // 256 + np.arange(n)[:, None, None] * 3).astype(np.uint8)
    a[:, ::3, ::2] = (np.arange(n)[:, None, None] * 37 + np.arange(h)[None, ::3, None] * 5 + np.arange(w)[None, None, ::2]).astype(np.uint8)
    a.setflags(write=False)
    return a


@contextlib.contextmanager
def tuned(g, keys):
    """gsh_tune keys for the length of a call; every one back to 0 whatever happens inside"""
    try:
        for k, v in keys.items():
            g.tune(k, v)
        yield
    finally:
        for k in keys:
            g.tune(k, 0)


_NOSTDLIB = []


def nostdlib():
    """the oracle with the GS_NO_STDLIB trig: the compiled reference where oracle/_ref has it, else the restatement"""
    if not _NOSTDLIB:
        _NOSTDLIB.append(Oracle("reference_nostdlib") if pyoracle.have_reference_nostdlib() else Oracle("port_nostdlib"))
    return _NOSTDLIB[0]


_EXPECTED = {}


def expected(key, make):
    """a case's expectation: computed once with the oracle, shared by every split, back end and stream, never written"""
    if key not in _EXPECTED:
        v = make()
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _EXPECTED[key] = v
    return _EXPECTED[key]


def _distinct(exp, what):
    """the expected outputs of any two frames differ"""
    flat = [np.ascontiguousarray(e).view(np.uint8).reshape(-1) for e in exp]
    for i in range(len(flat)):
        for j in range(i + 1, len(flat)):
            assert not np.array_equal(flat[i], flat[j]), "broken case %s: frames %d and %d expect the same output" % (what, i, j)


def sentinel(shape, dtype=np.uint8):
    return np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, SENTINEL, np.uint8).view(dtype).reshape(shape)


class Out:
    """one output of a call: its expectation (frame-major unless by_frame is False), the memory it lives in and its
    prefill (None: SENTINEL bytes)"""

    def __init__(self, name, exp, prefill=None, host=False, stride=None, by_frame=True, distinct=True, off=0):
        self.name, self.exp, self.host, self.by_frame, self.distinct, self.off = name, np.ascontiguousarray(exp), host, by_frame, distinct, off
        self.prefill = sentinel(self.exp.shape, self.exp.dtype) if prefill is None else np.ascontiguousarray(prefill)
        self.stride = stride


def _check(m, buf, out, what):
    raw = buf.store.cpu().numpy() if m.kind == "device" else np.asarray(buf.store)
    got, pre = raw[buf.lo:buf.lo + buf.nbytes], buf.pre
    want = out.exp.view(np.uint8).reshape(-1)
    n = len(out.exp) if out.by_frame else 1
    per = buf.nbytes // n
    idle = [f for f in range(n) if np.array_equal(got[f * per:(f + 1) * per], pre[f * per:(f + 1) * per])
            and not np.array_equal(want[f * per:(f + 1) * per], pre[f * per:(f + 1) * per])]
    assert not idle, "%s: frames %s of %d still hold their prefill: the launch that owns them never ran, or wrote elsewhere" % (what, idle, n)
    m.check(buf, out.exp, what)


def run_call(b, what, ins, outs, call, splits, keys=None):
    """call(output views, input views) once per split on fresh guarded buffers; ins: numpy arrays; outs: Out"""
    for o in outs:
        if o.by_frame and o.distinct:
            _distinct(o.exp, "%s %s" % (what, o.name))
    for split in splits:
        tag = "%s, key 8 = %d (launches of %s)" % (what, split, "+".join(str(k) for k in launches(len(ins[0]) if ins else len(outs[0].exp), split)))
        ib = [b.dev.make(a.shape, a.dtype, 0, prefill=a, stride=a.shape[-1] * a.dtype.itemsize) for a in ins]
        ob = [(b.host if o.host else b.dev).make(o.exp.shape, o.exp.dtype, o.off, prefill=o.prefill, stride=o.stride) for o in outs]
        with tuned(b.g, {**(keys or {}), 8: split}):
            call([v for _, v in ob], [v for _, v in ib])
            b.sync()
        for o, (buf, _) in zip(outs, ob):
            _check(b.host if o.host else b.dev, buf, o, "%s: %s" % (tag, o.name))
        for k, (buf, _) in enumerate(ib):
            b.dev.check(buf, None, "%s: input %d was written" % (tag, k))


def per_frame(fn, src):
    return np.stack([fn(f) for f in src])


CASES = []


def image_case(name, what, w, h, call, oracle_fn, keys=None, seed=None, out_shape=None):
    """an entry that reads n frames and writes n frames: dst = oracle_fn(o, frame, sentinel-filled dst frame)"""
    def run(b, splits):
        src = frames(seed if seed is not None else w * 31 + h, N, h, w)
        exp = expected(name, lambda: np.stack([oracle_fn(b.o, f, sentinel(out_shape or f.shape)) for f in src]))
        run_call(b, "%s %d x %dx%d" % (what, N, w, h), [src], [Out("dst", exp, stride=exp.shape[-1])], lambda o, i: call(b.g, o[0], i[0]), splits, keys)
    CASES.append((name, run))


# ---- sobel, erode, dilate: the four widths -------------------------------------------------------------------------------------
for _w, _route in WIDTHS:
    image_case("sobel_batch-w%d-%s" % (_w, _route), "gsh_sobel_batch", _w, H, lambda g, d, s: g.sobel_batch(d, s), lambda o, f, d: o.sobel(f, d))
    image_case("erode_batch-w%d-%s" % (_w, _route), "gsh_erode_batch", _w, H, lambda g, d, s: g.erode_batch(d, s), lambda o, f, d: o.erode(f))
    image_case("dilate_batch-w%d-%s" % (_w, _route), "gsh_dilate_batch", _w, H, lambda g, d, s: g.dilate_batch(d, s), lambda o, f, d: o.dilate(f))

# ---- blur and adaptive threshold: the five routes of launch_blur / launch_box_generic ---------------------------------------
# (w, r, route, keys): k_blur16<R> for r <= 3 (gs_blur only; gs_adaptive_threshold has no such kernel and starts at the ring);
# the register ring k_box16r for r <= 16 and h >= 2 r + 1, with k_box_edge for the last columns of ragged rows; k_box16
# beyond; the integral route k_box_px where strip_ok fails (w = 20: the table by rows + columns) and under key 6 = 3
# (w = 64: the banded table)
BOX_ROUTES = [(64, 5, "ring", {}), (64, 11, "ring", {}), (68, 5, "ring+box_edge", {}), (67, 5, "ring+box_edge", {}), (67, 11, "ring+box_edge", {}),
              (68, 11, "ring+box_edge", {}), (64, 20, "box16", {}), (67, 20, "box16", {}),
              (20, 5, "integral_rows_cols+box_px", {}), (64, 5, "key6_3-integral_banded+box_px", {6: 3})]
for _w, _r in ((64, 1), (67, 1), (64, 3), (68, 3), (67, 3)):
    image_case("blur_batch-w%d-r%d-blur16" % (_w, _r), "gsh_blur_batch r = %d" % _r, _w, H, lambda g, d, s, r=_r: g.blur_batch(d, s, r),
               lambda o, f, d, r=_r: o.blur(f, r))
for _w, _r, _route, _keys in BOX_ROUTES:
    assert (_route.startswith("ring")) == (_r <= 16 and H >= 2 * _r + 1 and _w >= 32 and not _keys)
    image_case("blur_batch-w%d-r%d-%s" % (_w, _r, _route), "gsh_blur_batch r = %d" % _r, _w, H, lambda g, d, s, r=_r: g.blur_batch(d, s, r),
               lambda o, f, d, r=_r: o.blur(f, r), keys=_keys)
for _w, _r, _c, _route, _keys in ([(64, 2, 5, "ring", {}), (67, 2, 5, "ring+box_edge", {}), (67, 5, -7, "ring+box_edge", {})]
                                  + [(w, r, 5, route, keys) for w, r, route, keys in BOX_ROUTES if r != 11]):
    image_case("adaptive_threshold_batch-w%d-r%d-c%d-%s" % (_w, _r, _c, _route), "gsh_adaptive_threshold_batch r = %d, c = %d" % (_r, _c), _w, H,
               lambda g, d, s, r=_r, c=_c: g.adaptive_threshold_batch(d, s, r, c), lambda o, f, d, r=_r, c=_c: o.adaptive_threshold(f, r, c), keys=_keys)

# ---- filter: k_filter16 for 3 x 3 kernels with sum |k| <= 128 and norm <= 256 on frames that pass strip_ok, else k_filter_px ----
GAUSS = np.array([[1, 2, 1], [2, 4, 2], [1, 2, 1]], np.int8)
WIDE53 = np.array([[1, 0, -1, 2, 1], [0, 3, 1, 0, -2], [1, -1, 2, 0, 1]], np.int8)
ABS129 = np.array([[16, -16, 16], [-16, 1, 16], [16, -16, 16]], np.int8)
for _w, _route in WIDTHS:
    image_case("filter_batch-w%d-gauss16-%s" % (_w, "filter_px" if _w < 32 else "filter16-" + _route), "gsh_filter_batch 3x3 / 16", _w, H,
               lambda g, d, s: g.filter_batch(d, s, GAUSS, 16), lambda o, f, d: o.filter(f, GAUSS, 16))
image_case("filter_batch-w64-5x3-filter_px", "gsh_filter_batch 5x3 / 2", 64, H, lambda g, d, s: g.filter_batch(d, s, WIDE53, 2), lambda o, f, d: o.filter(f, WIDE53, 2))
image_case("filter_batch-w67-abs129-filter_px", "gsh_filter_batch abs129 / 7", 67, H, lambda g, d, s: g.filter_batch(d, s, ABS129, 7), lambda o, f, d: o.filter(f, ABS129, 7))

# ---- downsample: k_downsample8 from 16 source columns on, else k_downsample_px -----------------------------------------------
for _w, _route in ((64, "downsample8"), (67, "downsample8"), (14, "downsample_px")):
    image_case("downsample_batch-sw%d-%s" % (_w, _route), "gsh_downsample_batch", _w, H, lambda g, d, s: g.downsample_batch(d, s),
               lambda o, f, d: o.downsample(f), out_shape=(H // 2, _w // 2))


# ---- pyramid: level-major planes, n frames each ------------------------------------------------------------------------------
def pyramid_case(w, h, n_levels, L):
    name = "pyramid_batch-%dx%d-%d_levels_asked-%d_built" % (w, h, n_levels, L)

    def run(b, splits):
        import orb_pyramid_batch_cases as pb
        src = frames(w + h, N, h, w)
        d = pb.dims(w, h, n_levels)
        assert len(d) == L
        nbytes = N * sum(x * y for x, y in d[1:])

        def make():
            per = [pb.levels_of(f, n_levels) for f in src]
            for l in range(1, L):
                _distinct([p[l] for p in per], "%s level %d" % (name, l))
            exp, used = pb.pyramid_expected(src, n_levels, sentinel(nbytes))
            assert used == nbytes
            return exp
        exp = expected(name, make)
        run_call(b, "gsh_pyramid_batch %d x %dx%d, %d levels" % (N, w, h, n_levels), [src], [Out("levels", exp, stride=w, by_frame=False)],
                 lambda o, i: b.g.pyramid_batch(o[0], i[0], n_levels), splits)
    CASES.append((name, run))


pyramid_case(131, 129, 3, 3)  # three levels need 128 rows: a level lower than 32 rows is not built
pyramid_case(67, 70, 4, 2)  # level 2 would be 16 x 17: the level rule stops before it


# ---- histogram, Otsu: hist[f], thr[f] ------------------------------------------------------------------------------------------
def hist_case(w, route, keys=None):
    tag = "-key12_500_pieces" if keys else ""

    def run_hist(b, splits):
        src = frames(1, N, H, w)
        hists = expected(("hist", w), lambda: per_frame(b.o.histogram, src))
        run_call(b, "gsh_histogram_batch %d x %dx%d" % (N, w, H), [src], [Out("hist", hists, stride=1024, off=4)],
                 lambda o, i: b.g.histogram_batch(i[0], o[0]), splits, keys)

    def run_otsu(b, splits):
        src = frames(1, N, H, w)
        hists = expected(("hist", w), lambda: per_frame(b.o.histogram, src))
        thr = expected(("otsu", w), lambda: np.array([b.o.otsu_threshold(f) for f in src], np.uint8))
        run_call(b, "gsh_otsu_batch %d x %dx%d" % (N, w, H), [src], [Out("hist_scratch", hists, stride=1024), Out("thr", thr, off=1)],
                 lambda o, i: b.g.otsu_batch(i[0], o[0], o[1]), splits, keys)
    CASES.append(("histogram_batch-w%d-%s%s" % (w, route, tag), run_hist))
    CASES.append(("otsu_batch-w%d-%s%s" % (w, route, tag), run_otsu))


for _w, _route in WIDTHS:
    hist_case(_w, "hist_partial")
hist_case(67, "frame_by_frame", {12: 500})  # 67 x 24 = 1608 bytes: three pieces of 500 and a rest of 108 per frame

# ---- threshold in place: scalar, thr[f], thr[f] + offset ----------------------------------------------------------------------
THR = np.arange(40, 40 + 20 * N, 20, dtype=np.uint8)


def threshold_case(w, kind, offset=0):
    name = "threshold_batch%s-w%d%s" % ({"scalar": "", "dev": "_dev-thr_per_frame", "dev_offset": "_dev_offset"}[kind], w, "%+d" % offset if offset else "")

    def run(b, splits):
        src = frames(w + 9, N, H, w)
        at = [100] * N if kind == "scalar" else [(int(t) + offset) & 255 for t in THR]
        exp = expected(name, lambda: np.stack([b.o.threshold(f, t) for f, t in zip(src, at)]))
        if kind != "scalar":  # a threshold read one frame off must show: the neighbour's threshold gives another picture
            for f in range(N):
                for g in (f - 1, f + 1):
                    assert not (0 <= g < N) or not np.array_equal(exp[f], b.o.threshold(src[f], at[g])), "broken case %s" % name

        def call(o, i):
            if kind == "scalar":
                b.g.threshold_batch(o[0], 100)
            elif kind == "dev":
                b.g.threshold_batch(o[0], i[0])
            else:
                b.g.threshold_batch_dev_offset(o[0], i[0], offset)
        run_call(b, "gsh_%s %d x %dx%d" % (name, N, w, H), [THR] if kind != "scalar" else [], [Out("img", exp, prefill=src, stride=w)], call, splits)
    CASES.append((name, run))


for _w in (64, 67):
    threshold_case(_w, "scalar")
    threshold_case(_w, "dev")
    threshold_case(_w, "dev_offset", 10)
    threshold_case(_w, "dev_offset", -3)

# ---- blur + sobel: fused for r <= 3, else launch_blur into the library's scratch of fb * n bytes, then launch_sobel -----------
for _w, _r, _route in ((64, 2, "fused"), (67, 2, "fused"), (64, 4, "unfused-scratch_plane"), (67, 4, "unfused-scratch_plane")):
    image_case("blur_sobel_batch-w%d-r%d-%s" % (_w, _r, _route), "gsh_blur_sobel_batch r = %d" % _r, _w, H, lambda g, d, s, r=_r: g.blur_sobel_batch(d, s, r),
               lambda o, f, d, r=_r: o.sobel(o.blur(f, r)))


# ---- the edge pipeline: dst, hist[f], thr[f] (and tmp) -------------------------------------------------------------------------
def pipeline_expected(o, src, r):
    blurred = per_frame(lambda f: o.blur(f, r), src)
    edges = per_frame(o.sobel, blurred)
    thr = np.array([o.otsu_threshold(e) for e in edges], np.uint8)
    return blurred, per_frame(o.histogram, edges), thr, np.stack([o.threshold(e, int(t)) for e, t in zip(edges, thr)])


def pipeline_outs(b, w, r, with_tmp):
    src = frames(1, N, H, w)
    blurred, hists, thr, final = expected(("pipeline", w, r), lambda: pipeline_expected(b.o, src, r))
    outs = [Out("dst", final, stride=w), Out("hist_scratch", hists, stride=1024), Out("thr", thr)]
    return src, outs + ([Out("tmp", blurred, stride=w)] if with_tmp else [])


def pipeline_case(w, r, with_tmp, route):
    name = "edge_pipeline_batch-w%d-r%d-%s-%s" % (w, r, "tmp" if with_tmp else "no_tmp", route)

    def run(b, splits):
        src, outs = pipeline_outs(b, w, r, with_tmp)

        def call(o, i):
            if route.startswith("fused_with_histogram"):  # strip_ok16: whole strips, dst and src 16-byte aligned
                assert w % 16 == 0 and gd._ptr(o[0]) % 16 == 0 and gd._ptr(i[0]) % 16 == 0
            b.g.edge_pipeline_batch(o[0], o[3] if with_tmp else None, i[0], r, o[1], o[2])
        run_call(b, "gsh_edge_pipeline_batch (%s) %d x %dx%d r = %d" % (route, N, w, H, r), [src], outs, call, splits)
    CASES.append((name, run))


pipeline_case(64, 2, False, "fused_with_histogram")
pipeline_case(67, 2, False, "fused_blur_sobel+otsu")
pipeline_case(64, 2, True, "blur+sobel+otsu")
pipeline_case(64, 4, False, "scratch_plane-blur+sobel+otsu")

# ---- integral: rows + columns below 32 columns, else bands; ragged rows; column chunks beyond 4096 ----------------------------
for _w, _h, _route in ((20, H, "rows+cols"), (64, H, "banded"), (67, H, "banded_ragged"), (4112, 8, "banded_wide_column_chunks")):
    def _run(b, splits, w=_w, h=_h, name="integral_batch-%dx%d-%s" % (_w, _h, _route)):
        src = frames(w + 17, N, h, w)
        exp = expected(name, lambda: per_frame(b.o.integral, src))
        run_call(b, "gsh_integral_batch %d x %dx%d" % (N, w, h), [src], [Out("ii", exp, stride=4 * w)], lambda o, i: b.g.integral_batch(i[0], o[0]), splits)
    CASES.append(("integral_batch-%dx%d-%s" % (_w, _h, _route), _run))


# ---- ORB: kps[f], counts[f], score maps ----------------------------------------------------------------------------------------
ORB_W, ORB_H, ORB_THR = 90, 60, 20


ORB_SIDES = (3, 5, 7, 9, 11, 13, 15)


@functools.lru_cache(maxsize=None)
def orb_frames(n=N, seed=1):
    """n frames of 90 x 60 whose keypoint counts all differ (1, 4, 6, 14, 17, 26, 29 with the oracle): a square of noise
    in the middle (a keypoint keeps 15 pixels from every edge) whose side grows with the frame, over a gentle row, column
    and frame ramp that has no corner of its own"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:ORB_H, 0:ORB_W]
    out = np.empty((n, ORB_H, ORB_W), np.uint8)
    for f in range(n):
        a = (90 + x // 4 + y // 3 + f).astype(np.uint8)
        s = ORB_SIDES[f % len(ORB_SIDES)]
        x0, y0 = ORB_W // 2 - s // 2 + (f % 3) - 1, ORB_H // 2 - s // 2 + (f % 2)
        win = (x >= x0) & (x < x0 + s) & (y >= y0) & (y < y0 + s)
        a[win] = rng.integers(0, 256, int(win.sum()), dtype=np.uint8)
        out[f] = a
    out.setflags(write=False)
    return out


def _records(lists, cap, what, capped_and_not):
    """every frame has a record, no two frames the same list; under a cap that is part of the case one frame reaches it and
    one does not.  lists: the oracle's uncapped lists"""
    assert all(len(r) >= 1 for r in lists), "broken case %s: a frame without a record: %s" % (what, [len(r) for r in lists])
    cut = [r[:cap] for r in lists]
    for i in range(len(cut)):
        for j in range(i + 1, len(cut)):
            assert not (len(cut[i]) == len(cut[j]) and cut[i].tobytes() == cut[j].tobytes()), "broken case %s: frames %d and %d have equal record lists" % (what, i, j)
    if capped_and_not:
        assert any(len(r) > cap for r in lists) and any(len(r) <= cap for r in lists), "broken case %s: cap %d against %s" % (what, cap, [len(r) for r in lists])


def orb_expected(o, fast_o, src, nkps):
    """(kps laid over the sentinel, counts, score maps with the sentinel in their 3-px frame)"""
    n = len(src)
    ek, ec = sentinel((n, nkps), KEYPOINT_DTYPE), np.zeros(n, np.uint32)
    es = sentinel(src.shape).copy()
    for f in range(n):
        ko = o.orb_extract(src[f], nkps, ORB_THR, es[f])
        es[f] = fast_o.fast(src[f], min(nkps * 4, 5000), ORB_THR, es[f])[1]
        ek[f, :len(ko)] = ko
        ec[f] = len(ko)
    return ek, ec, es


def orb_case(kind, nkps):
    name = "orb_extract_batch_%s-90x60-nkps%d%s" % (kind, nkps, "-capped" if nkps == 3 else "")

    def run(b, splits):
        src = orb_frames()
        o = nostdlib() if kind == "nostdlib" else b.o

        def make():
            _records([o.orb_extract(f, 100000, ORB_THR) for f in src], nkps, name, nkps == 3)
            return orb_expected(o, b.o, src, nkps)
        ek, ec, es = expected(name, make)
        host = kind == "dev"
        outs = [Out("kps", ek, host=host, off=4), Out("counts", ec, host=host, distinct=nkps != 3, off=4), Out("score maps", es, stride=ORB_W, off=1)]

        def call(ov, iv):
            if kind == "nostdlib":
                b.g.orb_extract_batch_nostdlib(iv[0], ov[2], ov[0], ov[1], nkps, ORB_THR)
            else:
                b.g.c.gsh_orb_extract_batch(gd._ptr(iv[0]), ORB_W, ORB_H, len(src), gd._ptr(ov[2]), gd._ptr(ov[0]), gd._ptr(ov[1]), nkps, ORB_THR)
        run_call(b, "gsh_%s" % name, [src], outs, call, splits)
    CASES.append((name, run))


orb_case("nostdlib", 30)
orb_case("nostdlib", 3)
orb_case("dev", 30)


# ---- template matching: result maps, best[f], score[f] (tmatch_batch_cases.run: guarded 0x5a buffers, the oracle per frame) ----
def template_case(per_frame_tmpl):
    name = "match_locate_find_best_template_batch-8x8_on_64x40-%s-dot4" % ("template_per_frame" if per_frame_tmpl else "one_template")

    def run(b, splits):
        seed = 1 if per_frame_tmpl else 3  # chosen with the oracle: the seven best points and the seven scores all differ
        img = frames(seed, N, 40, 64)
        tmpl = tb.frames(seed + 1000, N if per_frame_tmpl else 1, 8, 8)
        tmpl = tmpl if per_frame_tmpl else tmpl[0]
        assert tb.plan(64, 40, 8, 8, N) == "dot4" == tb.plan(64, 40, 8, 8, 1)
        maps, best, score = tb.expected([b.o], name, img, tmpl)
        _distinct(maps, name + " maps"), _distinct(best, name + " best"), _distinct(score, name + " score")
        for split in splits:
            with tuned(b.g, {8: split}):
                tb.run(b.g, Mem("device" if b.gpu else "host"), [b.o], name, img, tmpl, "%s, key 8 = %d" % (name, split))
    CASES.append((name, run))


template_case(False)
template_case(True)


# ---- synth and checksum: seed0 + f, sums[f] ------------------------------------------------------------------------------------
for _w in (64, 67):
    def _run_synth(b, splits, w=_w):
        exp = expected(("synth", w), lambda: np.stack([Oracle.synth(w, H, 700 + f) for f in range(N)]))
        run_call(b, "gsh_synth_batch %d x %dx%d" % (N, w, H), [], [Out("dst", exp, stride=w)], lambda o, i: b.g.synth_batch(o[0], 700), splits)

    def _run_checksum(b, splits, w=_w):
        src = frames(w + 21, N, H, w)
        exp = expected(("checksum", w), lambda: np.array([gd._checksum(f) for f in src], np.uint64))
        assert int(exp[0]) == sum((i + 1) * (int(v) + 1) for i, v in enumerate(src[0].reshape(-1))) % 2 ** 64
        run_call(b, "gsh_checksum_batch %d x %dx%d" % (N, w, H), [src], [Out("sums", exp)], lambda o, i: b.g.checksum_batch(i[0], o[0]), splits)
    CASES.append(("synth_batch-w%d-seed0_plus_f" % _w, _run_synth))
    CASES.append(("checksum_batch-w%d" % _w, _run_checksum))


# ======================================================================================================================
# the groups key 8 does not govern
# ======================================================================================================================
LBP_W, LBP_H, LBP_PARAMS = 48, 40, (1.2, 1.0, 1.6, 2)
LBP_GROUP = 8


@functools.lru_cache(maxsize=None)
def lbp_inputs(n):
    src = frames(77, n, LBP_H, LBP_W)
    ii = np.stack([Oracle("port").integral(f) for f in src])
    ii.setflags(write=False)
    return src, ii


def check_lbp_group(b, n, cap, armed=False):
    """gsh_lbp_detect_batch cuts n frames into launches of kLbpGroup = 8 whatever key 8 says: n = 9 is 8 + 1, n = 17 is
    8 + 8 + 1.  Every frame's rects and count against gs_lbp_detect on that frame's table; cap 12 caps every frame, cap 64
    none (asserted).  armed: with gsh_lbp_count_evaluated's counting kernels, as lbp_cascade_cases.check_batch does"""
    assert n > LBP_GROUP and n % LBP_GROUP == 1
    casc = random_cascade(2, permissive=True)
    src, ii = lbp_inputs(n)
    name = "gsh_lbp_detect_batch %d x %dx%d cap %d" % (n, LBP_W, LBP_H, cap)

    def make():
        full = [b.o.lbp_detect(casc, t, 100000, *LBP_PARAMS) for t in ii]
        _records(full, cap, name, False)
        assert all(len(r) > 12 for r in full) and all(len(r) <= 64 for r in full), [len(r) for r in full]
        er, ec = sentinel((n, cap), RECT_DTYPE), np.zeros(n, np.uint32)
        for f in range(n):
            ro = b.o.lbp_detect(casc, ii[f], cap, *LBP_PARAMS)
            assert len(ro) == min(len(full[f]), cap) and ro.tobytes() == full[f][:cap].tobytes()
            er[f, :len(ro)] = ro
            ec[f] = len(ro)
        return er, ec
    er, ec = expected((name,), make)
    dc = b.g.cascade_create(casc)
    ev = b.dev.put(np.zeros(4, np.int64)) if armed else None
    try:
        def call(o, i):
            b.g.lbp_count_evaluated(ev)
            try:
                b.g.lbp_detect_batch(dc, i[0], o[0], o[1], cap, *LBP_PARAMS)
                b.sync()
            finally:
                b.g.lbp_count_evaluated(None)
        run_call(b, name + (" (counting kernels)" if armed else ""), [ii], [Out("rects", er, off=4), Out("counts", ec, distinct=False, off=4)], call, (0,))
        if armed:
            e = np.asarray(ev.cpu().numpy() if b.gpu else ev)
            total = b.g.lbp_window_count(casc, LBP_W, LBP_H, *LBP_PARAMS)
            assert 0 < int(e[0]) <= n * total and int(e[1]) >= int(e[0]), (e, total)
    finally:
        dc.close()


LBP_GROUP_CASES = [(9, 12, False), (9, 64, False), (17, 12, False), (17, 64, False), (17, 12, True)]


def lbp_group_id(c):
    return "lbp_detect_batch-kLbpGroup-n%d_launches_%s-cap%d%s" % (c[0], "+".join(str(k) for k in launches(c[0], LBP_GROUP)), c[1], "-counting" if c[2] else "")


# ---- kOrbGroup = 4096 frames per pass of gsh_orb_extract_batch (GPU only: the emulator would take minutes) -------------------
ORB_GROUP, ORB_PERIOD = 4096, 5


def check_orb_group(b, nkps=30):
    """4097 frames of 90 x 60, frame f = base[f % 5] with five different base frames: the passes are 4096 + 1, five oracle
    calls give every frame's list and score map, and a list placed one pass off cannot match since 4096 = 1 mod 5"""
    n = ORB_GROUP + 1
    assert ORB_GROUP % ORB_PERIOD == 1
    base = orb_frames()[2:2 + ORB_PERIOD]
    name = "gsh_orb_extract_batch %d x %dx%d nkps %d" % (n, ORB_W, ORB_H, nkps)

    def make():
        _records([b.o.orb_extract(f, 100000, ORB_THR) for f in base], nkps, name, False)
        ek, ec, es = orb_expected(b.o, b.o, base, nkps)
        _distinct(ek, name + " kps"), _distinct(ec, name + " counts"), _distinct(es, name + " score maps")
        which = np.arange(n) % ORB_PERIOD
        return ek[which], ec[which], es[which], np.ascontiguousarray(base[which])
    ek, ec, es, src = expected(name, make)
    outs = [Out("kps", ek, host=True, distinct=False, off=4), Out("counts", ec, host=True, distinct=False, off=4),
            Out("score maps", es, stride=ORB_W, distinct=False)]
    run_call(b, name, [src], outs, lambda ov, iv: b.g.c.gsh_orb_extract_batch(gd._ptr(iv[0]), ORB_W, ORB_H, n, gd._ptr(ov[2]), gd._ptr(ov[0]),
                                                                               gd._ptr(ov[1]), nkps, ORB_THR), (0,))


# ---- the scratch group of the integral box route: (256 MiB) / (4 w h) + 1 frames (GPU only) ------------------------------------
BOX_GROUP_W, BOX_GROUP_N, BOX_GROUP_PERIOD = 1024, 66, 7


def check_box_scratch_group(b, mode):
    """gsh_blur_batch r = 4 (mode "blur") / gsh_adaptive_threshold_batch r = 4, c = 5 (mode "adaptive") under key 6 = 3 on 66
    frames of 1024 x 1024: the scratch table holds 65 frames, the launches are 65 + 1.  Frames periodic with period 7 (65 = 2
    mod 7: frame 65 is not frame 0, and a result one group off cannot match); seven oracle calls give every frame"""
    w, n = BOX_GROUP_W, BOX_GROUP_N
    group = (256 << 20) // (4 * w * w) + 1
    assert group == 65 and n == group + 1 and group % BOX_GROUP_PERIOD not in (0,)
    base = frames(5, BOX_GROUP_PERIOD, w, w)
    name = "box scratch group, %s r = 4: %d x %dx%d under key 6 = 3" % (mode, n, w, w)
    fn = (lambda f: b.o.blur(f, 4)) if mode == "blur" else (lambda f: b.o.adaptive_threshold(f, 4, 5))

    def make():
        e = per_frame(fn, base)
        _distinct(e, name)
        which = np.arange(n) % BOX_GROUP_PERIOD
        return e[which], np.ascontiguousarray(base[which])
    exp, src = expected(name, make)
    call = (lambda o, i: b.g.blur_batch(o[0], i[0], 4)) if mode == "blur" else (lambda o, i: b.g.adaptive_threshold_batch(o[0], i[0], 4, 5))
    run_call(b, name, [src], [Out("dst", exp, stride=w, distinct=False)], call, (0,), {6: 3})


# ---- GPU-only combinations ------------------------------------------------------------------------------------------------------
def check_pipeline_chunks(b, chunk, split):
    """gsh_edge_pipeline_batch r = 2, tmp = NULL on 7 x 64x24 in chunks of `chunk` frames (key 5) whose inner
    for_frames(f0, nn, kMaxZ, ...) takes launches of `split` frames (key 8): on the GPU every chunk but the last runs its
    Otsu, threshold and frame zeroing on the side stream.  Then the same call twice in a row with no host sync between the
    two, on the frames in reverse order the second time: the second call reuses the partial-histogram scratch"""
    src, outs = pipeline_outs(b, 64, 2, False)
    what = "gsh_edge_pipeline_batch (fused, chunks of %d) %d x 64x%d" % (chunk, N, H)
    run_call(b, what, [src], outs, lambda o, i: b.g.edge_pipeline_batch(o[0], None, i[0], 2, o[1], o[2]), (split,), {5: chunk})
    rev = [Out(o.name + " of the second call", o.exp[::-1], stride=o.stride) for o in outs]
    both = outs + rev

    def twice(o, i):
        b.g.edge_pipeline_batch(o[0], None, i[0], 2, o[1], o[2])
        b.g.edge_pipeline_batch(o[3], None, i[1], 2, o[4], o[5])
    run_call(b, what + ", twice without a sync", [src, np.ascontiguousarray(src[::-1])], both, twice, (split,), {5: chunk})


def check_side_stream_box_edge(b, mode, split):
    """gsh_blur_batch r = 13 / gsh_adaptive_threshold_batch r = 13, c = 5 on 7 x 67x40 under key 6 = 7: k_box_edge of every
    launch goes to the side stream, and every launch records and waits on the same pair of events.  gsh_integral_batch on
    the result follows with no sync in between, as tests/sequence_cases.py does for the unsplit form"""
    w, h, r = 67, 40, 13
    assert r <= 16 and h >= 2 * r + 1 and w % 16  # the ring kernel, ragged rows
    src = frames(9, N, h, w)
    fn = (lambda f: b.o.blur(f, r)) if mode == "blur" else (lambda f: b.o.adaptive_threshold(f, r, 5))
    name = "side-stream k_box_edge, %s r = %d, %d x %dx%d" % (mode, r, N, w, h)

    def make():
        e = per_frame(fn, src)
        return e, per_frame(b.o.integral, e)
    exp, ii = expected(name, make)

    def call(o, i):
        (b.g.blur_batch(o[0], i[0], r) if mode == "blur" else b.g.adaptive_threshold_batch(o[0], i[0], r, 5))
        b.g.integral_batch(o[0], o[1])
    run_call(b, name, [src], [Out("dst", exp, stride=w), Out("integral of dst", ii, stride=4 * w)], call, (split,), {6: 7})
