"""Shared cases of tests/test_gpu_shape_frontier.py (MI355X) and tests/test_shape_frontier.py (emulator, plan): frames
taller than any other test's (a row-derived grid.y past 65535), wider (hundreds of strip column blocks) and of 2^31 bytes
and more (32-bit offset edges).  Everything is compared bit for bit; every dst starts as SENT bytes, and an output that is
still SENT everywhere is reported as a launch that never ran.

`g` is a bound library, `mem` a parity_cases.Mem, `o` the reference fixture (the compiled reference, or the restatement
checked against its recorded digests).  Inputs are seeded noise over a row and column ramp (`frame`).

A. Tall frames.  For every case: the launcher, its grid.y as a function of the frame, `past` = the smallest height of
the case whose grid.y exceeds 65535 and `last` = the largest height that keeps it at or below 65535.

  grid2d family, blocks of 64 x 4 threads: grid.y = ceil(rows / 4), past 65535 for rows > 262140.
    case                launcher (kernel)                                 rows          past -> grid.y    last
    sobel               launch_sobel (k_sobel_px, w < 32)                 h             262200 -> 65550   262140
    erode, dilate       launch_morph (k_morph_px)                         h             262200 -> 65550   262140
    morph2/5 e, d       launch_morph_iter (k_morphr_px)                   h             262200 -> 65550   262140
    blur1/2/7           launch_box_generic (k_box_px; integral: below)    h             262200 -> 65550   262140
    adaptive2           launch_box_generic<1> (k_box_px)                  h             262200 -> 65550   262140
    filter3x3, 5x3      gsh_filter_batch (k_filter_px)                    h             262200 -> 65550   262140
    fast_px             launch_fast_score (k_fast_score_px, key 7 = 2)    h - 6         262200 -> 65549   262146
    fast (both)         launch_fast (k_fast_clip, smaller score map)      h             262200 -> 65550   262140
    crop, crop_batch    launch_crop (k_crop_rows)                         roi.h         262200 -> 65550   262140
    crop_wrapped        gs_crop (k_crop_wrapped)                          roi.h         262200 -> 65550   262140
    perspective         launch_perspective (k_perspective)                dh            262200 -> 65550   262140
    tmatch4x4           tm_launch (k_match_template4, iw % 4 == 0)        ih - th + 1   262200 -> 65550   262143
    tmatch40x5          tm_launch (k_match_template4, 44 % 4 == 0)        ih - th + 1   262200 -> 65549   262144
    tmatch5x4_w17       tm_launch (k_match_template, iw % 4 != 0)         ih - th + 1   262200 -> 65550   262143
    lbp                 launch_integral_pad (k_integral_pad)              ih + 1        262200 -> 65551   262139
    downsample20        gsh_downsample_batch (k_downsample8, sw >= 16)    sh / 2        524400 -> 65550   524281
    downsample14        gsh_downsample_batch (k_downsample_px)            sh / 2        524400 -> 65550   524281
  (the k_box_px cases also run launch_integral's rows + columns form, w < 32: k_integral_rows with grid.x = h.)

  strip kernels at w = 32: two strips, a block of 64 x 4 threads takes four bands of T rows: grid.y = ceil(ceil(rows / T) / 4)
  with T = max(short_T, 2 halo_rows) from strip_cfg and its callers.
    erode, dilate       launch_morph (k_morph16): T = 4, rows = h                       1048600 -> 65538   1048560
    blur1               launch_blur (k_blur16<1>): T = max(4, 2) = 4, rows = h          1048600 -> 65538   1048560
    sobel               launch_sobel (k_sobel16): T = 6, rows = h - 2                   1572900 -> 65538   1572842
    blur2               launch_blur (k_blur16<2>): T = max(6, 4) = 6, rows = h          1572900 -> 65538   1572840
    filter3x3           gsh_filter_batch (k_filter16): T = 8, rows = h                  2097200 -> 65538   2097120
    integral            launch_integral (k_integral_colsum): grid.y = nb = ceil(h / 32) 2097200 -> 65538   2097120
    blur3               launch_blur (k_blur16<3>): T = max(12, 6) = 12, rows = h        3145800 -> 65538   3145680
    morph2              launch_morphk<2> (k_morphk16): T = max(16, 8) = 16, rows = h    4194400 -> 65538   4194240
  (the last two, 100 and 134 MB, against the same call on chunks of 2^20 rows and three bands of the reference: _chunked.)

  matrix-core template route: 32 x 16 template on 64 x ih, ib = 64 ih >= 4 MiB: k_tm_s2_corners has grid.y = rh = ih - 15.
    tmatch_mfma         tm_launch (k_tm_s2_corners)                                     65600 -> 65585     65550

  gs_resize / gs_resize_nn 8 x 1000 -> 8 x dh: resize_plan takes bands of 16 rows, grid.y = ceil(dh / 16); past 65535 it
  raises the band to ceil(dh / 65535) rounded up to a multiple of 4:
    resize              launch_resize (k_resize_tile)      1048700: band 20, grid.y 52435;   1048560: band 16, grid.y 65535

B. Wide frames 262200 x 9 and 1048600 x 4 (FAST, which needs 7 rows: 1048600 x 8): 65 / 257 column blocks of the strip
kernels (17 / 65 at four waves a block), k_integral_wave's column chunks, k_box_px behind the integral route (w > 4096).

C. One frame of 65536 x 32800 = 2 149 580 800 bytes (tests/test_gpu_shape_frontier.py has the references)."""
import functools

import numpy as np

from parity_cases import SENTINEL as SENT
from util import assert_same

GRID_MAX = 65535
K3 = np.array([[1, 2, 1], [2, 4, 2], [1, 2, 1]], np.int8)
K53 = np.array([[1, 0, -1, 2, 1], [0, 3, 0, -2, 1], [1, -1, 2, 0, 1]], np.int8)  # 5 wide, 3 high


@functools.lru_cache(maxsize=4)
def frame(seed, h, w):
    """noise over a ramp, so that a wrong row or column shows"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (h, w), dtype=np.uint8)
    a[::3, ::2] = (np.arange(h)[::3, None] * 5 + np.arange(w)[None, ::2]).astype(np.uint8)
    a.setflags(write=False)
    return a


def ceil_div(a, b):
    return (a + b - 1) // b


def sync(mem):
    if mem.kind != "host":
        import torch
        torch.cuda.synchronize()


def check(got, want, what):
    got = np.asarray(got)
    assert not (got.view(np.uint8) == SENT).all(), "%s: the output still holds its prefill everywhere (the launch never ran)" % what
    assert_same(got, want, what)


# ---- operations: op(g, mems, o, img, what); the drop-in ones take host or device pointers, BATCH_OPS device pointers only ----
def _unary(call, expect):
    def op(g, mems, o, img, what):
        want = expect(o, img)
        for mem in mems:
            d = mem.zeros(img.shape, fill=SENT)
            call(g, d, mem.put(img))
            sync(mem)
            check(mem.get(d), want, "%s, %s pointers" % (what, mem.kind))
    return op


def _rows_equal(mem, a, b):
    if mem.kind == "host":
        return np.array_equal(a, b)
    import torch
    return torch.equal(a, b)


CHUNK, LAP, BAND = 1 << 20, 64, 128


def _chunked(call, expect, rows_per_block):
    """For the two frames on which the reference takes 10 to 20 s: the whole frame against the same call on chunks of 2^20
    rows cut with 64 rows of overlap (grid.y a third of the limit: what the other cases pin), byte for byte, and three bands
    of 128 rows against the reference: the top, the rows around the first block past grid.y = 65535, the bottom."""
    def op(g, mems, o, img, what):
        h = img.shape[0]
        bands = []
        for r0 in (0, min(h - BAND, rows_per_block * GRID_MAX - BAND // 2), h - BAND):
            lo, hi = max(0, r0 - 8), min(h, r0 + BAND + 8)
            bands.append((r0, expect(o, img[lo:hi])[r0 - lo:r0 - lo + BAND]))
        for mem in mems:
            s, d = mem.put(img), mem.zeros(img.shape, fill=SENT)
            call(g, d, s)
            sync(mem)
            for r0, want in bands:
                check(np.asarray(mem.get(d[r0:r0 + BAND])), want, "%s, %s pointers, rows %d.." % (what, mem.kind, r0))
            for r0 in range(0, h, CHUNK):
                lo, hi = max(0, r0 - LAP), min(h, r0 + CHUNK + LAP)
                part = mem.zeros((hi - lo, img.shape[1]), fill=SENT)
                call(g, part, s[lo:hi])
                sync(mem)
                n = min(CHUNK, h - r0)
                assert _rows_equal(mem, d[r0:r0 + n], part[r0 - lo:r0 - lo + n]), "%s, %s pointers: rows %d.. differ from the chunk's" % (what, mem.kind, r0)
    return op


def _iterate(f, n):
    def run(o, img):
        for _ in range(n):
            img = getattr(o, f)(img)
        return img
    return run


def _morph_batch(it, dilate):
    return _unary(lambda g, d, s: g.morph_batch(d[None], s[None], it, dilate), _iterate("dilate" if dilate else "erode", it))


def op_integral(g, mems, o, img, what):
    want = o.integral(img)
    exp = (np.cumsum(np.cumsum(img, 0, dtype=np.uint64), 1, dtype=np.uint64) % (1 << 32)).astype(np.uint32)
    assert np.array_equal(want, exp), what + ": the oracle differs from numpy's 64-bit cumulative sums mod 2^32"
    for mem in mems:
        ii = mem.put(np.full(img.shape, SENT * 0x01010101, np.uint32))
        g.integral(mem.put(img), ii)
        sync(mem)
        check(mem.get(ii, np.uint32), want, "%s, %s pointers" % (what, mem.kind))


def _op(prepare, run):
    """prepare(o, img) -> the expectation, computed once; run(g, mem, img, want, what) for host and device pointers"""
    def op(g, mems, o, img, what):
        want = prepare(o, img)
        for mem in mems:
            run(g, mem, img, want, "%s, %s pointers" % (what, mem.kind))
    return op


FAST_CAP, FAST_THRESHOLD = 3000, 30


def contrast_windows(img):
    """gs_fast stops at its cap, and on noise that is within the first rows.  So the FAST cases keep the frame's low four bits
    around 100 (no corner at threshold 30, rows and columns still differ) and its full contrast in three windows of 40 rows
    (columns, for wide frames): the first, the ones around row 4 x 65535, the last.  A hundred keypoints, from all three."""
    h, w = img.shape
    out = (100 + (img & 15)).astype(np.uint8)
    length = max(h, w)
    for p in (0, min(length // 2, 4 * GRID_MAX) - 20, length - 40):
        if h >= w:
            out[p:p + 40] = img[p:p + 40]
        else:
            out[:, p:p + 40] = img[:, p:p + 40]
    return out


def _fast(key7, clip):
    def score_map(img):
        h, w = img.shape
        # clip: a smaller score map, for k_fast_clip.  Its prefill is 1, not SENT: the NMS pass reads the caller's 3-px frame,
        # and 0xAB there would suppress every corner of an 8-row image; a pass that never ran leaves 1 where 0 or a score belongs
        return np.full((h - 5 if h > 100 else h, w - 3) if clip else (h, w), 1, np.uint8)

    def prepare(o, img):
        h, w = img.shape
        img = contrast_windows(img)
        ko, smo = o.fast(img, FAST_CAP, FAST_THRESHOLD, scoremap=score_map(img))
        along = ko["y"] if h >= w else ko["x"]
        assert 10 < len(ko) < FAST_CAP and along.min() < 40 and along.max() >= max(h, w) - 46, "keypoints expected from the first to the last window"
        return ko, smo

    def run(g, mem, img, want, what):
        img = contrast_windows(img)
        sm = mem.put(score_map(img))
        try:
            g.tune(7, key7)
            k = g.fast(mem.put(img), sm, FAST_CAP, FAST_THRESHOLD)
        finally:
            g.tune(7, 0)
        assert_same(k, want[0], what + " keypoints")
        assert_same(np.asarray(mem.get(sm)), want[1], what + " score map")
    return _op(prepare, run)


def _crop(batch=False, wrapped=False):
    def roi(img):
        h, w = img.shape
        return (0xFFFFFFFF, 0, 3, h) if wrapped else (1, 0, w - 2, h)  # wrapped: ref :155 accepts it, column 0 reads 0

    def run(g, mem, img, want, what):
        d = mem.zeros(want.shape, fill=SENT)
        if batch:
            g.crop_batch(d[None], mem.put(img)[None], *roi(img))
        else:
            g.crop(d, mem.put(img), *roi(img))
        sync(mem)
        check(mem.get(d), want, what)
    return _op(lambda o, img: o.crop(img, *roi(img)), run)


def spec_perspective(dw, dh, src, c):
    """blob_cases.spec_perspective (ref :423-444 in float32, operation for operation) on whole arrays"""
    f = np.float32
    sh, sw = src.shape
    with np.errstate(invalid="ignore", divide="ignore"):
        u = (np.arange(dw, dtype=f) / (f(dw) - f(1)))[None, :]
        v = (np.arange(dh, dtype=f) / (f(dh) - f(1)))[:, None]
        top_x = f(c[0][0]) * (f(1) - u) + f(c[1][0]) * u
        top_y = f(c[0][1]) * (f(1) - u) + f(c[1][1]) * u
        bot_x = f(c[3][0]) * (f(1) - u) + f(c[2][0]) * u
        bot_y = f(c[3][1]) * (f(1) - u) + f(c[2][1]) * u
        sx_f = top_x * (f(1) - v) + bot_x * v
        sy_f = top_y * (f(1) - v) + bot_y * v
        mx, my = f(sw) - f(1), f(sh) - f(1)
        sx_f = np.where(sx_f < mx, sx_f, mx)
        sx_f = np.where(f(0) > sx_f, f(0), sx_f)
        sy_f = np.where(sy_f < my, sy_f, my)
        sy_f = np.where(f(0) > sy_f, f(0), sy_f)
        sx, sy = sx_f.astype(np.int64), sy_f.astype(np.int64)
        sx1, sy1 = np.minimum(sx + 1, sw - 1), np.minimum(sy + 1, sh - 1)
        dx, dy = sx_f - sx.astype(f), sy_f - sy.astype(f)
        s = src.astype(f)
        p = (s[sy, sx] * (f(1) - dx) * (f(1) - dy)) + (s[sy, sx1] * dx * (f(1) - dy)) + (s[sy1, sx] * (f(1) - dx) * dy) + (s[sy1, sx1] * dx * dy)
    assert p.dtype == f
    return p.astype(np.int64).astype(np.uint8)


PERSPECTIVE_CORNERS = ((3, 2), (44, 5), (47, 61), (1, 57))  # tl, tr, br, bl inside the 50 x 64 source


def _perspective():
    """img only gives the destination's shape; the source is frame(3, 64, 50)"""
    def run(g, mem, img, want, what):
        d = mem.zeros(img.shape, fill=SENT)
        g.perspective_correct(d, mem.put(frame(3, 64, 50)), PERSPECTIVE_CORNERS)
        sync(mem)
        check(mem.get(d), want, what)
    return _op(lambda o, img: spec_perspective(img.shape[1], img.shape[0], frame(3, 64, 50), PERSPECTIVE_CORNERS), run)


def _tmatch(tw, th):
    def tmpl(img):
        h = img.shape[0]
        return img[h - 7 - th:h - 7, 1:1 + tw].copy()  # cut near the bottom: the zero-distance match lies in the last blocks

    def run(g, mem, img, want, what):
        r = mem.zeros(want.shape, fill=SENT)
        g.match_template(mem.put(img), mem.put(tmpl(img)), r)
        sync(mem)
        got = np.asarray(mem.get(r))
        check(got, want, what)
        assert got[img.shape[0] - 7 - th, 1] == 255, what
    return _op(lambda o, img: o.match_template(img, tmpl(img)), run)


MFMA_TW, MFMA_TH, MFMA_BAND = 32, 16, 200


def _tmatch_mfma():
    """32 x 16 template: three bands of 200 result rows (top, around result row 65535, bottom) against the oracle"""
    def tmpl(img):
        h = img.shape[0]
        return img[h - 40:h - 40 + MFMA_TH, 5:5 + MFMA_TW].copy()

    def bands(img):
        rh = img.shape[0] - MFMA_TH + 1
        return (0, min(GRID_MAX, rh - MFMA_BAND) - MFMA_BAND // 2, rh - MFMA_BAND)

    def prepare(o, img):
        return [o.match_template(img[r0:r0 + MFMA_BAND + MFMA_TH - 1], tmpl(img)) for r0 in bands(img)]

    def run(g, mem, img, want, what):
        h, w = img.shape
        r = mem.zeros((h - MFMA_TH + 1, w - MFMA_TW + 1), fill=SENT)
        g.match_template(mem.put(img), mem.put(tmpl(img)), r)
        sync(mem)
        got = np.asarray(mem.get(r))
        assert not (got == SENT).all(), "%s: the output still holds its prefill everywhere (the launch never ran)" % what
        for r0, band in zip(bands(img), want):
            assert_same(got[r0:r0 + MFMA_BAND], band, "%s, result rows %d.." % (what, r0))
        assert got[h - 40, 5] == 255, what
    return _op(prepare, run)


def _lbp():
    """a permissive cascade at step 2: a quarter of a million detections, down to the last window row, so that the rows of the
    padded table the last blocks write are all read (a cascade that rejects nearly everything reads them and says no)"""
    from util import random_cascade
    params = (2000000, 1.2, 1.0, 1.2, 2)

    def prepare(o, img):
        ii = o.integral(img)
        want = o.lbp_detect(random_cascade(3), ii, *params)
        assert 100000 < len(want) < params[0] and want["y"].max() >= img.shape[0] - 26 and (want["y"] >= img.shape[0] - 32).sum() >= 4, len(want)
        return ii, want

    def run(g, mem, img, want, what):
        assert_same(g.lbp_detect(random_cascade(3), mem.put(want[0]), *params), want[1], what)
    return _op(prepare, run)


def _downsample():
    def run(g, mem, img, want, what):
        d = mem.zeros(want.shape, fill=SENT)
        g.downsample(d, mem.put(img))
        sync(mem)
        check(mem.get(d), want, what)
    return _op(lambda o, img: o.downsample(img), run)


def _resize(nearest):
    """img only gives the destination's shape; the source is frame(4, 1000, 8)"""
    def run(g, mem, img, want, what):
        d = mem.zeros(img.shape, fill=SENT)
        g.resize(d, mem.put(frame(4, 1000, 8)), nearest)
        sync(mem)
        check(mem.get(d), want, what)
    return _op(lambda o, img: o.resize(frame(4, 1000, 8), img.shape[1], img.shape[0], nearest), run)


OPS = {
    "sobel": _unary(lambda g, d, s: g.sobel(d, s), lambda o, a: o.sobel(a, np.full_like(a, SENT))),
    "erode": _unary(lambda g, d, s: g.erode(d, s), lambda o, a: o.erode(a)),
    "dilate": _unary(lambda g, d, s: g.dilate(d, s), lambda o, a: o.dilate(a)),
    "morph2e": _morph_batch(2, False), "morph2d": _morph_batch(2, True), "morph5e": _morph_batch(5, False), "morph5d": _morph_batch(5, True),
    "blur1": _unary(lambda g, d, s: g.blur(d, s, 1), lambda o, a: o.blur(a, 1)),
    "blur2": _unary(lambda g, d, s: g.blur(d, s, 2), lambda o, a: o.blur(a, 2)),
    "blur3": _unary(lambda g, d, s: g.blur(d, s, 3), lambda o, a: o.blur(a, 3)),
    "blur7": _unary(lambda g, d, s: g.blur(d, s, 7), lambda o, a: o.blur(a, 7)),
    "adaptive2": _unary(lambda g, d, s: g.adaptive_threshold(d, s, 2, 3), lambda o, a: o.adaptive_threshold(a, 2, 3)),
    "filter3x3": _unary(lambda g, d, s: g.filter(d, s, K3, 16), lambda o, a: o.filter(a, K3, 16)),
    "filter5x3": _unary(lambda g, d, s: g.filter(d, s, K53, 4), lambda o, a: o.filter(a, K53, 4)),
    "blur3_chunked": _chunked(lambda g, d, s: g.blur(d, s, 3), lambda o, a: o.blur(a, 3), 4 * 12),
    "morph2e_chunked": _chunked(lambda g, d, s: g.morph_batch(d[None], s[None], 2, False), _iterate("erode", 2), 4 * 16),
    "integral": op_integral,
    "fast": _fast(0, True), "fast_px": _fast(2, True), "fast_whole_map": _fast(0, False),
    "crop": _crop(), "crop_batch": _crop(batch=True), "crop_wrapped": _crop(wrapped=True),
    "perspective": _perspective(),
    "tmatch4x4": _tmatch(4, 4), "tmatch40x5": _tmatch(40, 5), "tmatch5x4": _tmatch(5, 4), "tmatch_mfma": _tmatch_mfma(),
    "lbp": _lbp(), "downsample": _downsample(),
    "resize": _resize(False), "resize_nn": _resize(True),
}
BATCH_OPS = ("morph2e", "morph2d", "morph5e", "morph5d", "morph2e_chunked", "crop_batch")  # gsh_* entries: device pointers only


def grid2d_y(rows):
    return ceil_div(rows, 4)


def strip_y(T, trim=0):
    return lambda h: ceil_div(ceil_div(h - trim, T), 4)


# (id, op, w, grid.y as a function of the frame height, past, last), smallest frames first
TALL_GRID2D = [(name, name, 16, grid2d_y, 262200, 262140) for name in (
    "sobel", "erode", "dilate", "morph2e", "morph2d", "morph5e", "morph5d", "blur1", "blur2", "blur7", "adaptive2", "filter3x3",
    "filter5x3", "crop", "crop_batch", "crop_wrapped", "perspective")] + [
    ("fast", "fast", 16, grid2d_y, 262200, 262140),
    ("fast_px", "fast_px", 16, lambda h: grid2d_y(h - 6), 262200, 262146),
    ("tmatch4x4", "tmatch4x4", 16, lambda h: grid2d_y(h - 3), 262200, 262143),
    ("tmatch5x4_w17", "tmatch5x4", 17, lambda h: grid2d_y(h - 3), 262200, 262143),
    ("tmatch40x5", "tmatch40x5", 44, lambda h: grid2d_y(h - 4), 262200, 262144),
    ("lbp", "lbp", 30, lambda h: (h + 4) // 4, 262200, 262139),
    ("downsample20", "downsample", 20, lambda h: grid2d_y(h // 2), 524400, 524281),
    ("downsample14", "downsample", 14, lambda h: grid2d_y(h // 2), 524400, 524281),
]
TALL_STRIP = [
    ("strip_erode", "erode", 32, strip_y(4), 1048600, 1048560),
    ("strip_dilate", "dilate", 32, strip_y(4), 1048600, 1048560),
    ("strip_blur1", "blur1", 32, strip_y(4), 1048600, 1048560),
    ("strip_sobel", "sobel", 32, strip_y(6, 2), 1572900, 1572842),
    ("strip_blur2", "blur2", 32, strip_y(6), 1572900, 1572840),
    ("strip_filter3x3", "filter3x3", 32, strip_y(8), 2097200, 2097120),
    ("strip_integral", "integral", 32, lambda h: ceil_div(h, 32), 2097200, 2097120),
    ("strip_blur3", "blur3_chunked", 32, strip_y(12), 3145800, 3145680),
    ("strip_morph2e", "morph2e_chunked", 32, strip_y(16), 4194400, 4194240),
]
TALL_MFMA = [("tmatch_mfma", "tmatch_mfma", 64, lambda h: h - 15, 65600, 65550)]
TALL_RESIZE = [("resize", "resize", 8, lambda h: ceil_div(h, 20 if ceil_div(h, 16) > GRID_MAX else 16), 1048700, 1048560),
               ("resize_nn", "resize_nn", 8, lambda h: ceil_div(h, 20 if ceil_div(h, 16) > GRID_MAX else 16), 1048700, 1048560)]
TALL = TALL_GRID2D + TALL_MFMA + TALL_RESIZE + TALL_STRIP
TALL_CASES = [(c, side) for c in TALL for side in ("past", "last")]


def check_frontier(case):
    """the heights are what the docstring says: `past` is the first grid.y beyond 65535 only in the sense that `last` is the
    largest height at or below it and past > last"""
    name, op, w, grid_y, past, last = case
    if op.startswith("resize"):  # capped by resize_plan: 1048560 is the last height with bands of 16 rows
        assert ceil_div(past, 16) > GRID_MAX >= grid_y(past) and ceil_div(last, 16) == GRID_MAX == grid_y(last) and ceil_div(last + 1, 16) > GRID_MAX
        return
    assert grid_y(past) > GRID_MAX >= grid_y(last) and grid_y(last + 1) > GRID_MAX, (name, grid_y(past), grid_y(last))


def _mems(op, mems):
    return [m for m in mems if m.kind != "host" or op not in BATCH_OPS] if len(mems) > 1 else mems


def run_tall(g, mems, o, case, side):
    """mems: [Mem("device"), Mem("host")] on the GPU, [Mem("host")] on the emulator (which takes host memory for both)"""
    name, op, w, grid_y, past, last = case
    h = past if side == "past" else last
    seed = 1 + sum(map(ord, name)) + (1000 if side == "last" else 0)  # the two frames of a case share no rows
    OPS[op](g, _mems(op, mems), o, frame(seed, h, w), "%s %d x %d (%s, grid.y %d)" % (name, w, h, side, grid_y(h)))


WIDE_SHAPES = ((262200, 9), (1048600, 4))
WIDE_OPS = ("sobel", "erode", "dilate", "blur1", "blur2", "blur7", "adaptive2", "filter3x3", "filter5x3", "integral", "downsample")
WIDE_CASES = [(op, w, h) for (w, h) in WIDE_SHAPES for op in WIDE_OPS] + [("fast_whole_map", 262200, 9), ("fast", 1048600, 8), ("fast_px", 1048600, 8)]


def run_wide(g, mems, o, case):
    op, w, h = case
    OPS[op](g, _mems(op, mems), o, frame(7 + h, h, w), "%s %d x %d" % (op, w, h))
