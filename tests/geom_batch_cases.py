"""Shared cases of tests/test_geom_batch.py (emulator) and tests/test_gpu_geom_batch.py (MI355X): gsh_crop_batch,
gsh_resize_batch, gsh_resize_nn_batch and gsh_crop_resize_batch against the oracle's gs_crop / gs_resize / gs_resize_nn,
frame by frame and byte for byte.

`g` is a bound library, `mem` a parity_cases.Mem ("host": the emulator takes host memory for device memory; "device":
torch CUDA tensors), `oracles` the CPU oracles that must all give the expected bytes (the C restatement, and the compiled
reference wherever oracle/_ref was built).

Every run: all frames of a batch differ, dst is pre-filled with 0x5a and sits inside a larger buffer whose other bytes
must come back untouched, src is compared with its copy afterwards.

The launcher's rule (gs_stencil.cpp, resize_plan) is restated in `plan` so that every shape can say which branch it takes:
with more than four source pixels per result pixel (sw sh > 4 dw dh) the launch gets no LDS and every block gathers its
taps from global memory.  Else a block of k_resize_tile covers 256 output columns and `band` output rows and stages at
most E(256, sw, dw) x E(band, sh, dh) source bytes, E(c, s, d) = min(s, ceil(c s / d) + 3); the largest band of 16, 8, 4
rows that needs at most 16 KiB is taken, else 4 rows if they need at most 48 KiB, else again no LDS.  Whatever the form,
at most 65535 bands: a taller result takes bands of ceil(dh / 65535) rows, rounded up to a multiple of 4, with the LDS
size of the band it had (a block whose rectangle no longer fits gathers)."""
import functools

import numpy as np

FILL, GUARD = 0x5A, 0xA5
PRE, POST = 64, 64
LDS_SMALL, LDS_MAX = 16 * 1024, 48 * 1024
MAX_BANDS = 65535


def extent(c, s, d):
    return min(s, (c * s + d - 1) // d + 3)


def plan(dw, dh, sw, sh, any_density=False):
    """(output rows per block, bytes of LDS) of gsh_resize_batch / gs_resize; 0 bytes = the gather form.  any_density:
    under gsh_tune(25, 2), which stages whatever the scale"""
    band, lds = _plan_lds(dw, dh, sw, sh, any_density)
    if (dh + band - 1) // band > MAX_BANDS:
        band = ((dh + MAX_BANDS - 1) // MAX_BANDS + 3) & ~3
    return band, lds


def _plan_lds(dw, dh, sw, sh, any_density):
    if sw * sh > 4 * dw * dh and not any_density:
        return 16, 0
    pitch = (extent(min(dw, 256), sw, dw) + 3) & ~3
    for band in (16, 8, 4):
        need = pitch * extent(min(band, dh), sh, dh)
        if need <= (LDS_SMALL if band > 4 else LDS_MAX):
            return band, need
    return 16, 0


def sync(mem):
    if mem.kind != "host":
        import torch
        torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def frames(seed, n, h, w):
    """n different frames: noise over a ramp, so that a wrong frame, row or column shows"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (n, h, w), dtype=np.uint8)
    a[:, ::3, ::2] = (np.arange(n)[:, None, None] * 37 + np.arange(h)[None, ::3, None] * 5 + np.arange(w)[None, None, ::2]).astype(np.uint8)
    a.setflags(write=False)
    return a


class Guarded:
    """`nbytes` payload bytes `off` bytes past an aligned address inside a larger buffer of GUARD bytes"""

    def __init__(self, mem, payload, off=0):
        payload = np.ascontiguousarray(payload, np.uint8).reshape(-1)
        self.mem, self.lo, self.n = mem, PRE + off, payload.size
        host = np.full(self.lo + self.n + POST, GUARD, np.uint8)
        host[self.lo:self.lo + self.n] = payload
        self.buf = mem.put(host)

    def view(self, shape):
        return self.buf[self.lo:self.lo + self.n].reshape(shape)

    def payload(self, what):
        sync(self.mem)
        a = np.asarray(self.mem.get(self.buf))
        assert (a[:self.lo] == GUARD).all() and (a[self.lo + self.n:] == GUARD).all(), "%s: bytes around the buffer were written" % what
        return a[self.lo:self.lo + self.n].copy()


def _run(g, mem, src, dshape, call, what, off=0, soff=0):
    """call(dst view, src view) on guarded buffers -> the dst bytes; src must come back unchanged"""
    s = Guarded(mem, src, soff)
    d = Guarded(mem, np.full(int(np.prod(dshape)), FILL, np.uint8), off)
    call(d.view(dshape), s.view(src.shape))
    out = d.payload(what).reshape(dshape)
    assert np.array_equal(s.payload(what).reshape(src.shape), src), "%s: src was written" % what
    return out


def _same(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%s: %d bytes differ, first at (f, y, x) = %s: got %d, expected %d" % (
        what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


_EXPECTED = {}


def expected_resize(oracles, key, src, dw, dh, nearest):
    """computed once per case and shared by every back end and schedule; every oracle has to agree"""
    k = ("resize", key, dw, dh, nearest)
    if k not in _EXPECTED:
        want = [np.stack([o.resize(f, dw, dh, nearest) for f in src]) for o in oracles]
        for w in want[1:]:
            assert np.array_equal(w, want[0]), "the oracles disagree on %s" % (k,)
        want[0].setflags(write=False)
        _EXPECTED[k] = want[0]
    return _EXPECTED[k]


def expected_crop(oracles, key, src, roi):
    k = ("crop", key, roi)
    if k not in _EXPECTED:
        want = [np.stack([o.crop(f, *roi) for f in src]) for o in oracles]
        for w in want[1:]:
            assert np.array_equal(w, want[0]), "the oracles disagree on %s" % (k,)
        _EXPECTED[k] = want[0]
    return _EXPECTED[k]


def check_resize(g, mem, oracles, n, sw, sh, dw, dh, nearest, off=0, soff=0, seed=5):
    src = frames(seed, n, sh, sw)
    what = "gsh_resize%s_batch %d x %dx%d -> %dx%d (+%d, src +%d)" % ("_nn" if nearest else "", n, sw, sh, dw, dh, off, soff)
    got = _run(g, mem, src, (n, dh, dw), lambda d, s: g.resize_batch(d, s, nearest), what, off, soff)
    _same(got, expected_resize(oracles, (seed, n, sw, sh), src, dw, dh, nearest), what)
    return got


def check_crop(g, mem, oracles, n, sw, sh, roi, off=0, soff=0, seed=6):
    src = frames(seed, n, sh, sw)
    what = "gsh_crop_batch %d x %dx%d roi %s (+%d, src +%d)" % (n, sw, sh, roi, off, soff)
    got = _run(g, mem, src, (n, roi[3], roi[2]), lambda d, s: g.crop_batch(d, s, *roi), what, off, soff)
    _same(got, expected_crop(oracles, (seed, n, sw, sh), src, roi), what)
    return got


# ---- tile and store edges: (n, sw, sh, dw, dh); every one bilinear and nearest -----------------------------------------
# widths around the dword of a lane (1, 3, 4, 5), the wave (63 x 4 = 252 is inside 255, 256, 257: the 256-column tile) and
# two tiles (257, 300); heights around the four waves of a block.  By the rule only the results of at least 97 x 53 / 4
# pixels are staged (255, 256, 257 x 7, 300 x 5 and 7), the smaller ones gathered; every case therefore runs a
# second time under gsh_tune(25, 2), where all of them are staged at band 16.
TILE_EDGE_CASES = [(3, 97, 53, dw, dh) for dw in (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 300) for dh in (1, 2, 3, 4, 5, 7)]
# dw * dh odd with n = 3 (5x3 and 63x1 are in the list above): frames 1 and 2 of dst start off 4-byte alignment; the 7x9
# source does the same on the source side
ODD_SOURCE_CASES = [(3, 7, 9, 5, 3), (3, 7, 9, 63, 1), (3, 7, 9, 16, 12), (3, 7, 9, 7, 9)]

# ---- scale classes: (n, sw, sh, dw, dh, branch) with branch = plan(dw, dh, sw, sh), asserted ---------------------------
SCALE_CASES = [
    (2, 64, 16, 64, 16, (16, 1024)),        # identity
    (2, 64, 16, 128, 32, (16, 704)),        # exact x2
    (2, 64, 16, 32, 8, (16, 1024)),         # exact /2
    (2, 37, 23, 100, 61, (16, 400)),        # non-integer upscale; 61 = 3 x 16 + 13 rows
    (2, 1, 1, 70, 9, (16, 4)),              # extreme upscale: sw - 1 = 0 clamps everything
    (2, 3, 2, 200, 50, (16, 8)),
    (2, 41, 1, 90, 5, (16, 44)),            # single-row source
    (2, 1, 41, 5, 90, (16, 44)),            # single-column source
    (2, 41, 29, 1, 17, (16, 0)),            # single-column result (gathered: 70 source pixels per result pixel)
    (2, 41, 29, 17, 1, (16, 0)),            # single-row result
    (2, 300, 200, 128, 77, (16, 0)),        # non-integer downscale, 6.1 source pixels per result pixel: the gather form
    (2, 300, 200, 160, 110, (16, 9900)),   # non-integer downscale below 2 x 2, staged at band 16
    (2, 600, 40, 300, 20, (8, 9804)),       # exact /2 of a wide frame, band 8: 16 rows would need 516 x 35 bytes
    (2, 4096, 8, 256, 32, (4, 16384)),      # / 16 in x, x 4 in y: band 4 in the large budget (8 rows: 4096 x 5)
    (2, 16384, 4, 256, 64, (16, 0)),        # / 64 in x, x 16 in y: 4 rows still span 16384 x 4 bytes > 48 KiB: the gather form
    (2, 2000, 60, 8, 4, (16, 0)),           # strong downscale, 3750 source pixels per result pixel: the gather form
    (2, 2000, 60, 300, 9, (16, 0)),         # the same with two tiles
    (2, 300, 200, 147, 99, (16, 0)),        # just past four source pixels per result pixel (4.12): the gather form
    (2, 300, 200, 150, 100, (16, 10500)),   # exactly four: staged
    (2, 64, 40, 50, 33, (16, 1472)),        # band boundary: 33 = 2 x 16 + 1 rows
    (2, 600, 34, 300, 17, (8, 9804)),       # band boundary at band 8: 17 = 2 x 8 + 1
    (2, 4096, 8, 256, 33, (4, 16384)),      # band boundary at band 4: 33 = 8 x 4 + 1
]


def check_tile_edge_case(g, mem, oracles, case):
    n, sw, sh, dw, dh = case
    band, lds = plan(dw, dh, sw, sh, any_density=True)
    assert band == 16 and lds > 0 and (plan(dw, dh, sw, sh) == (16, lds if sw * sh <= 4 * dw * dh else 0))
    for nearest in (False, True):
        check_resize(g, mem, oracles, n, sw, sh, dw, dh, nearest)
    try:
        g.tune(25, 2)
        for nearest in (False, True):
            check_resize(g, mem, oracles, n, sw, sh, dw, dh, nearest)
    finally:
        g.tune(25, 0)


def check_scale_case(g, mem, oracles, case):
    n, sw, sh, dw, dh, branch = case
    assert plan(dw, dh, sw, sh) == branch, (case, plan(dw, dh, sw, sh))
    for nearest in (False, True):
        check_resize(g, mem, oracles, n, sw, sh, dw, dh, nearest)


def check_tile_and_store_edges(g, mem, oracles):
    for case in TILE_EDGE_CASES + ODD_SOURCE_CASES:
        check_tile_edge_case(g, mem, oracles, case)
    for off in (1, 2, 3):  # the whole batch off alignment, both sides
        check_resize(g, mem, oracles, 3, 97, 53, 65, 5, False, off=off, soff=(off + 1) & 3)
        check_resize(g, mem, oracles, 3, 97, 53, 65, 5, True, off=off, soff=(off + 1) & 3)


def check_scale_classes(g, mem, oracles):
    for case in SCALE_CASES:
        check_scale_case(g, mem, oracles, case)


def check_forced_gather_and_split(g, mem, oracles):
    """GSH_TUNE_GEOM_FORM (key 25) = 1: the staged shapes through the gather form, 2: staging whatever the scale; key 8:
    two frames per launch"""
    try:
        g.tune(25, 1)
        for case in SCALE_CASES[3:12:2] + [(3, 97, 53, 257, 7, None)]:
            for nearest in (False, True):
                check_resize(g, mem, oracles, *case[:5], nearest)
        g.tune(25, 2)  # ... and the sparse shapes through the staged form (2000 x 60 fits 48 KiB at no band: still gathered)
        for case in ((2, 300, 200, 128, 77), (2, 300, 200, 147, 99), (2, 2000, 60, 300, 9), (2, 400, 80, 20, 17)):
            for nearest in (False, True):
                check_resize(g, mem, oracles, *case, nearest)
    finally:
        g.tune(25, 0)
    try:
        g.tune(8, 2)
        for nearest in (False, True):
            check_resize(g, mem, oracles, 3, 97, 53, 65, 5, nearest)
        check_crop(g, mem, oracles, 3, 131, 9, (3, 2, 65, 5))
    finally:
        g.tune(8, 0)


def check_nearest_wrap(g, mem, oracles):
    """1 x 70001 -> 1 x 66000: x * sw passes 2^32 from x = 61356 on, and the reference's 32-bit product wraps; sx is not
    monotone there, so these blocks gather"""
    assert 61356 * 70001 >= 2 ** 32 > 61355 * 70001
    got = check_resize(g, mem, oracles, 1, 70001, 1, 66000, 1, True, seed=9)
    src = frames(9, 1, 1, 70001)
    x = np.arange(66000, dtype=np.uint64)
    assert np.array_equal(got[0, 0], src[0, 0, ((x * 70001) % 2 ** 32) // 66000])
    check_resize(g, mem, oracles, 1, 70001, 1, 66000, 1, False, seed=9)


CROP_ROIS = [(x, y, w, 5) for x in (0, 1, 2, 3, 5) for w in (1, 3, 4, 15, 16, 17, 64, 65) for y in ((x + w) % 4,)]


def check_crop_cases(g, mem, oracles):
    for roi in CROP_ROIS:
        check_crop(g, mem, oracles, 3, 131, 9, roi)
    check_crop(g, mem, oracles, 3, 131, 9, (0, 0, 131, 9))        # the whole frame: gs_copy
    check_crop(g, mem, oracles, 3, 131, 9, (131 - 17, 9 - 4, 17, 4))  # touching the right and bottom edges
    check_crop(g, mem, oracles, 3, 131, 9, (130, 8, 1, 1))
    check_crop(g, mem, oracles, 2, 1100, 6, (3, 1, 1093, 5))      # two blocks of 64 lanes x 16 bytes in x
    for off in (1, 2, 3):
        check_crop(g, mem, oracles, 3, 131, 9, (5, 1, 65, 7), off=off, soff=(off + 2) & 3)


# ---- gsh_crop_resize_batch ---------------------------------------------------------------------------------------------
PATCH_W, PATCH_H = 16, 12
# on frames of 120 x 80: the whole frame, one pixel, touching left + top, touching right + bottom, an inner window; then the
# four that must give zeros: x + w wraps 2^32, empty, reaching outside the frame, (valid rectangle, frame index = n)
ROIS = np.array([(0, 0, 120, 80), (5, 7, 1, 1), (0, 0, 30, 20), (90, 60, 30, 20), (33, 21, 50, 31),
                 (0xFFFFFFF0, 3, 0x20, 10), (10, 10, 0, 5), (100, 10, 30, 20), (8, 8, 40, 40)], np.uint32)
FRAME_OF = np.array([1, 0, 1, 1, 0, 0, 1, 0, 2], np.uint32)  # unsorted, with repeats; the last one = n


def _patch(oracles, frames_, f, roi, nearest):
    x, y, w, h = (int(v) for v in roi)
    n, sh, sw = frames_.shape
    if w == 0 or h == 0 or x >= sw or w > sw - x or y >= sh or h > sh - y or f >= n:
        return np.zeros((PATCH_H, PATCH_W), np.uint8)
    want = [o.resize(o.crop(frames_[f], x, y, w, h), PATCH_W, PATCH_H, nearest) for o in oracles]
    for w_ in want[1:]:
        assert np.array_equal(w_, want[0])
    return want[0]


def check_crop_resize(g, mem, oracles):
    for n, frame_of in ((2, FRAME_OF), (2, None), (9, None)):
        src = frames(7, n, 80, 120)
        for nearest in (False, True):
            what = "gsh_crop_resize_batch n = %d, frame_of %s, %s" % (n, "given" if frame_of is not None else "NULL", "nearest" if nearest else "bilinear")
            rois_d = mem.put(ROIS)
            fo_d = mem.put(frame_of) if frame_of is not None else None
            got = _run(g, mem, src, (len(ROIS), PATCH_H, PATCH_W),
                       lambda d, s: g.crop_resize_batch(d, s, rois_d, fo_d, nearest), what, off=1 if nearest else 0)
            fo = frame_of if frame_of is not None else np.arange(len(ROIS))
            want = np.stack([_patch(oracles, src, int(fo[p]), ROIS[p], nearest) for p in range(len(ROIS))])
            _same(got, want, what)
            zero = [p for p in range(len(ROIS)) if p in (5, 6, 7) or int(fo[p]) >= n]
            assert all((got[p] == 0).all() for p in zero) and len(zero) >= (4 if n == 2 else 3), what
            assert np.array_equal(np.asarray(mem.get(rois_d)).view(np.uint32).reshape(ROIS.shape), ROIS), "rois were written"
    # windows larger than the block's LDS (16 KiB): these blocks gather
    src = frames(8, 2, 150, 700)
    rois = np.array([(0, 0, 700, 150), (1, 1, 698, 148), (10, 20, 64, 48)], np.uint32)
    fo = np.array([1, 0, 1], np.uint32)
    for nearest in (False, True):
        rois_d, fo_d = mem.put(rois), mem.put(fo)
        got = _run(g, mem, src, (3, PATCH_H, PATCH_W), lambda d, s: g.crop_resize_batch(d, s, rois_d, fo_d, nearest), "large windows")
        want = np.stack([_patch(oracles, src, int(fo[p]), rois[p], nearest) for p in range(3)])
        _same(got, want, "gsh_crop_resize_batch, windows beyond the LDS")


def check_dropin_equality(g, mem, oracles):
    """gs_resize / gs_resize_nn / gs_crop / gs_copy frame by frame give the bytes of the batch call"""
    for (n, sw, sh, dw, dh) in ((3, 97, 53, 257, 7), (3, 7, 9, 5, 3), (2, 37, 23, 100, 61), (2, 300, 200, 128, 77),
                                (2, 2000, 60, 8, 4), (2, 1200, 40, 20, 9)):
        src = frames(5, n, sh, sw)
        for nearest in (False, True):
            batch = check_resize(g, mem, oracles, n, sw, sh, dw, dh, nearest)
            for f in range(n):
                d = mem.zeros((dh, dw), fill=FILL)
                g.resize(d, mem.put(src[f]), nearest)
                sync(mem)
                assert np.array_equal(np.asarray(mem.get(d)), batch[f]), ("gs_resize", sw, sh, dw, dh, nearest, f)
    src = frames(6, 3, 9, 131)
    for roi in ((0, 0, 131, 9), (5, 1, 65, 7), (3, 2, 17, 5)):
        batch = check_crop(g, mem, oracles, 3, 131, 9, roi)
        for f in range(3):
            d = mem.zeros((roi[3], roi[2]), fill=FILL)
            if roi == (0, 0, 131, 9):
                g.copy(d, mem.put(src[f]))
            else:
                g.crop(d, mem.put(src[f]), *roi)
            sync(mem)
            assert np.array_equal(np.asarray(mem.get(d)), batch[f]), ("gs_crop", roi, f)


ALL_CHECKS = (check_tile_and_store_edges, check_scale_classes, check_forced_gather_and_split, check_nearest_wrap,
              check_crop_cases, check_crop_resize, check_dropin_equality)
