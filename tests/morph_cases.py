"""Shared pieces of tests/test_morph_fused.py (emulator) and tests/test_gpu_morph_fused.py (MI355X): the specification of
gsh_morph_batch and the cases both back ends run.

The specification: `iterations` applications of gs_erode / gs_dilate (ref grayskull.h:286-304) are ONE min / max over the
(2 n + 1)^2 window clipped to the image -- min with 255 fill, max with 0 fill.  check_spec_equals_iterated_reference ties
this numpy restatement to the reference's own loop applied n times; everything else compares the library with it."""
import numpy as np

from blob_paint_cases import Device, Host  # noqa: F401  (the two back ends: host memory for the emulator, torch on the GPU)

# whole strips, the tail lane anchored at w - 16, a wave seam, the ragged / realigning lane shifts (t % 64 == 1 and 63),
# the helper lane; 16, 17 and 31 fail strip_ok like the two of NARROW (per-pixel kernels)
WIDTHS = (16, 17, 31, 32, 33, 48, 1023, 1024, 1025, 1040, 1041, 1056, 2049)
NARROW = (1, 20)
HEIGHTS = (1, 2, 3, 4, 7, 8, 9, 17, 33)
ITERATIONS = (1, 2, 3, 4, 5, 7, 8, 9, 13)  # every remainder, one to four passes, both parities of the plane alternation
BAND_ROWS = (1, 2, 3, 5, 16, 0)  # gsh_tune key 0; 0 = the launcher's own
SENTINEL = 0xA5


def spec(a, n, dilate):
    """a (..., h, w) uint8 -> the clipped (2 n + 1)^2 max (dilate) / min of every frame"""
    a = np.asarray(a, np.uint8)
    h, w = a.shape[-2:]
    op = np.maximum if dilate else np.minimum
    p = np.full(a.shape[:-2] + (h + 2 * n, w + 2 * n), 0 if dilate else 255, np.uint8)
    p[..., n:n + h, n:n + w] = a
    r = p[..., :, 0:w].copy()
    for d in range(1, 2 * n + 1):
        r = op(r, p[..., :, d:d + w])
    o = r[..., 0:h, :].copy()
    for d in range(1, 2 * n + 1):
        o = op(o, r[..., d:d + h, :])
    return o


def frames(rng, n, h, w, kind):
    if kind == "random":
        return rng.integers(0, 256, (n, h, w), dtype=np.uint8)
    if kind == "binary":
        return (rng.integers(0, 100, (n, h, w)) < 8).astype(np.uint8) * 255
    if kind == "binary_dense":
        return (rng.integers(0, 100, (n, h, w)) < 92).astype(np.uint8) * 255
    return np.full((n, h, w), {"zeros": 0, "ones": 255}[kind], np.uint8)


def check_spec_equals_iterated_reference(oracles):
    """the anchor: the reference's 3x3 loop applied n times against the clipped window, on the CPU"""
    rng = np.random.default_rng(11)
    for (h, w) in ((1, 1), (1, 7), (7, 1), (5, 5), (4, 9), (13, 21), (24, 40)):
        imgs = [frames(rng, 1, h, w, k)[0] for k in ("random", "binary", "binary_dense")]
        for (y, x) in {(0, 0), (h - 1, w - 1), (h // 2, w // 2), (0, w - 1)}:
            one = np.zeros((h, w), np.uint8)
            one[y, x] = 255
            imgs += [one, 255 - one]
        for o in oracles:
            for img in imgs:
                for dilate in (True, False):
                    cur, step = img, (o.dilate if dilate else o.erode)
                    for n in range(1, 10):
                        cur = np.asarray(step(np.ascontiguousarray(cur)))
                        if n <= 6 or n == 9:
                            assert np.array_equal(cur, spec(img, n, dilate)), (o.kind, h, w, n, dilate)


def _planes(X, count, fb, offset, fill=SENTINEL):
    """`count` frames of fb bytes between two guard frames, the first frame `offset` bytes past the allocation's
    (at least 16-byte aligned) start -> (the whole device buffer, its (count + 2) * fb payload view)"""
    buf = X.put(np.full((count + 2) * fb + 16, fill, np.uint8))
    return buf, buf[offset:offset + (count + 2) * fb]


def run(g, X, src, iterations, dilate, tmp="own", offset=0, tmp_offset=None):
    """gsh_morph_batch on src (n, h, w) -> (n, h, w); asserts the guard frames around dst and tmp untouched and src
    unchanged.  tmp: "own" = a caller's plane, None = the library's scratch.  offset: dst and src start that many
    bytes past an aligned address (tmp: tmp_offset, default the same)."""
    src = np.ascontiguousarray(src)
    n, h, w = src.shape
    fb = h * w
    _, dflat = _planes(X, n, fb, offset)
    _, sflat = _planes(X, n, fb, offset)
    s = sflat[fb:fb + n * fb].reshape(n, h, w)
    if X is Host:
        s[...] = src
    else:
        s.copy_(X.put(src))
    d = dflat[fb:fb + n * fb].reshape(n, h, w)
    t, tflat = None, None
    if tmp == "own":
        _, tflat = _planes(X, n, fb, offset if tmp_offset is None else tmp_offset)
        t = tflat[fb:fb + n * fb].reshape(n, h, w)
    g.morph_batch(d, s, iterations, dilate, tmp=t)
    out, sall = X.get(dflat), X.get(sflat)
    assert (out[:fb] == SENTINEL).all() and (out[fb + n * fb:] == SENTINEL).all(), "written outside dst"
    assert np.array_equal(sall[fb:fb + n * fb].reshape(n, h, w), src), "src was written"
    assert (sall[:fb] == SENTINEL).all() and (sall[fb + n * fb:] == SENTINEL).all(), "written around src"
    if tflat is not None:
        tall = X.get(tflat)
        assert (tall[:fb] == SENTINEL).all() and (tall[fb + n * fb:] == SENTINEL).all(), "written outside tmp"
    return out[fb:fb + n * fb].reshape(n, h, w).copy()


def check(g, X, src, iterations, dilate, what, **kw):
    got = run(g, X, src, iterations, dilate, **kw)
    want = spec(src, iterations, dilate)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%s, %s %d on %s: %d bytes differ, first at (f, y, x) = %s: got %d, expected %d" % (
        what, "dilate" if dilate else "erode", iterations, src.shape, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])
    return got


def check_widths(g, X):
    """every width at the heights around the ring depth, every single-pass radius and two multi-pass counts"""
    rng = np.random.default_rng(21)
    for w in WIDTHS + NARROW:
        for h in (3, 9):
            for it in (1, 2, 3, 4, 7, 9):
                for dilate in (True, False):
                    check(g, X, frames(rng, 1, h, w, "random"), it, dilate, "widths")
        check(g, X, frames(rng, 1, 9, w, "binary"), 4, True, "widths binary")
        check(g, X, frames(rng, 1, 9, w, "binary_dense"), 4, False, "widths binary")


def check_heights_and_iterations(g, X):
    """every height x every iteration count, both ops, batches of 1 and 3, on a ragged, a whole-strip and a narrow width"""
    rng = np.random.default_rng(22)
    for w in (33, 48, 20):
        for h in HEIGHTS:
            for it in ITERATIONS:
                for dilate in (True, False):
                    check(g, X, frames(rng, 1 if (h + it) % 2 else 3, h, w, "random"), it, dilate, "heights")
    for w in (1041, 2049):  # two and three wave columns
        for h, it in ((1, 13), (2, 5), (17, 8), (33, 13), (8, 3)):
            for dilate in (True, False):
                check(g, X, frames(rng, 3 if h < 17 else 1, h, w, "random"), it, dilate, "heights, wide")


def check_content(g, X):
    rng = np.random.default_rng(23)
    for (h, w) in ((17, 48), (9, 1041), (7, 20)):
        for it in (1, 3, 4, 9):
            for kind in ("zeros", "ones", "binary", "binary_dense"):
                for dilate in (True, False):
                    check(g, X, frames(rng, 2, h, w, kind), it, dilate, kind)


def check_single_pixels(g, X):
    """one 255 in black under dilate / one 0 in white under erode becomes the exact clipped square: at every corner, on
    every edge, on both sides of the wave seam x = 1023 | 1024, and on both sides of a forced band seam"""
    h, w, T = 21, 1056, 5
    spots = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, 500), (h - 1, 500), (10, 0), (10, w - 1),
             (10, 1023), (10, 1024), (3, 1020), (12, 1027), (T - 1, 700), (T, 700), (2 * T - 1, 1023), (2 * T, 1024)]
    for band in (T, 0):
        g.tune(0, band)
        try:
            for it in (2, 3, 4, 9):
                for dilate in (True, False):
                    src = np.full((len(spots), h, w), 0 if dilate else 255, np.uint8)
                    for f, (y, x) in enumerate(spots):
                        src[f, y, x] = 255 if dilate else 0
                    got = check(g, X, src, it, dilate, "single pixel, band rows %d" % band)
                    for f, (y, x) in enumerate(spots):
                        sq = np.zeros((h, w), bool)
                        sq[max(0, y - it):y + it + 1, max(0, x - it):x + it + 1] = True
                        assert np.array_equal(got[f] == (255 if dilate else 0), sq), (band, it, dilate, y, x)
        finally:
            g.tune(0, 0)


def check_band_rows_and_block_shapes(g, X):
    """gsh_tune key 0 forces the band height, key 1 the block shape, key 8 the frames per launch"""
    rng = np.random.default_rng(24)
    for band in BAND_ROWS:
        g.tune(0, band)
        try:
            for (h, w) in ((17, 48), (33, 33), (9, 1041)):
                for it in (2, 3, 4, 9, 13) if w < 1000 else (4, 7):
                    for dilate in (True, False):
                        check(g, X, frames(rng, 2, h, w, "random"), it, dilate, "band rows %d" % band)
        finally:
            g.tune(0, 0)
    for shape in (1, 2, 3):
        g.tune(1, shape)
        try:
            for (h, w) in ((9, 48), (9, 1041), (5, 2049), (17, 1025)):
                for it in (2, 3, 4, 9):
                    for dilate in (True, False):
                        for band in (0, 3):
                            g.tune(0, band)
                            check(g, X, frames(rng, 2, h, w, "random"), it, dilate, "block shape %d band rows %d" % (shape, band))
        finally:
            g.tune(1, 0), g.tune(0, 0)
    for fpl in (1, 2):
        g.tune(8, fpl)
        try:
            for (h, w) in ((9, 33), (4, 1025), (7, 20)):
                for it in (1, 4, 6, 9):
                    for dilate in (True, False):
                        check(g, X, frames(rng, 3, h, w, "random"), it, dilate, "frames per launch %d" % fpl)
        finally:
            g.tune(8, 0)


def check_byte_offsets(g, X):
    """frames 1, 2 and 3 bytes past an aligned address: the realigning strip flavour on aligned widths too; the
    library's own (aligned) scratch and a caller's plane at another phase between the passes"""
    rng = np.random.default_rng(25)
    for off in (1, 2, 3):
        for w in (32, 33, 48, 1024, 1025, 1040, 1056, 20):
            for it in (2, 3, 4, 9):
                for dilate in (True, False):
                    src = frames(rng, 2, 9, w, "random")
                    check(g, X, src, it, dilate, "offset %d" % off, offset=off)
                    if it > 4:
                        check(g, X, src, it, dilate, "offset %d, own scratch" % off, offset=off, tmp=None)
                        check(g, X, src, it, dilate, "offset %d, tmp at %d" % (off, (off + 1) & 3), offset=off, tmp_offset=(off + 1) & 3)


def check_tmp_forms(g, X):
    """tmp=None (the library's grow-only scratch, growing between calls) and a caller's plane give the same bytes"""
    rng = np.random.default_rng(26)
    for (n, h, w) in ((1, 9, 48), (3, 17, 1041), (2, 33, 33), (5, 40, 130)):  # growing batches: the scratch grows
        for it in (5, 8, 9, 13):
            for dilate in (True, False):
                src = frames(rng, n, h, w, "random")
                a = check(g, X, src, it, dilate, "tmp=None", tmp=None)
                b = check(g, X, src, it, dilate, "tmp supplied", tmp="own")
                assert np.array_equal(a, b)


def check_one_iteration_is_the_3x3_entry(g, X):
    rng = np.random.default_rng(27)
    for (h, w) in ((9, 48), (17, 1041), (7, 20), (1, 33)):
        src = frames(rng, 2, h, w, "random")
        for dilate in (True, False):
            d = X.put(np.zeros_like(src))
            (g.dilate_batch if dilate else g.erode_batch)(d, X.put(src))
            assert np.array_equal(X.get(d), run(g, X, src, 1, dilate, tmp=None)), (h, w, dilate)


ALL_CHECKS = (check_widths, check_heights_and_iterations, check_content, check_single_pixels, check_band_rows_and_block_shapes,
              check_byte_offsets, check_tmp_forms, check_one_iteration_is_the_3x3_entry)
