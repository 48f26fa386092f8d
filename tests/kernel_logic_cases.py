"""Shared cases of tests/test_emu_logic.py (emulator) and tests/test_gpu_kernel_logic.py (MI355X): the kernel-logic cases
that used to run on the emulator only -- every ring radius, every clamp of the adaptive compare, every FAST threshold where
p + t wraps, every histogram alignment -- as functions of (g, o, mem), or (g, reference, mem) where the expectation is the
compiled reference's.

`g`   : grayskull_amd.Grayskull bound to the emulator library or to the product library
`o`   : oracle.pyoracle.Oracle (the C restatement); `reference`: the fixture of that name
`mem` : parity_cases.Mem("host") or Mem("device").  The drop-in gs_* calls take either kind of pointer on the GPU; the
        gsh_*_batch calls take device pointers there, so their cases run with Mem("device") on the GPU and Mem("host") on
        the emulator (whose 'device' memory is host memory).

Every output starts as SENTINEL bytes, never as zeros.  Every gsh_tune call sits in try / finally (`tuned`) and is put back
to 0.  An expectation never comes from the library: it is the oracle's (or the reference's) result for the same input,
computed once per case and shared by the band heights, routes and memory kinds that must all give it.
"""
import numpy as np

from frame_split_cases import nostdlib, tuned
from oracle.pyoracle import Oracle
from parity_cases import SENTINEL, fast, stencils
from util import assert_same


def _float_bits(v):
    return np.float32(v).tobytes()


# ---------------------------------------------------------------------------------------------------- orientation
ORIENT_RADII = (15, 36, 37, 60, 90)  # 36 = kOrientExactR (k_orb.h): the last radius of the integer sums; beyond: k_orient_moments_seq


def orientation_images(r):
    """the two inputs per radius: a generated frame and a 251-fill, side 2 r + 31, upper half divided by 3 (a strong
    vertical gradient: large |m01|)"""
    side = 2 * r + 31
    out = []
    for seed, img in ((1, Oracle.synth(side, side, r)), (2, np.full((side, side), 251, np.uint8))):
        img = img.copy()
        img[: side // 2] //= 3
        out.append((seed, img))
    return side, out


def orientation(g, reference, mems, r):
    """gs_compute_orientation == the reference, as the 32 bits of the float: beyond r = 36 the moment sums pass 2^24 and the
    reference's float32 accumulation order matters"""
    side, imgs = orientation_images(r)
    for seed, img in imgs:
        exp = reference.orientation(img, side // 2, side // 2, r)
        for mem in mems:
            got = g.compute_orientation(mem.put(img), side // 2, side // 2, r)
            assert _float_bits(got) == _float_bits(exp), (r, seed, mem.kind, got, exp)


def orientation_nostdlib(g, mems, r):
    """gs_compute_orientation_nostdlib == the GS_NO_STDLIB flavour of the reference (the same moments through the float32
    atan2 polynomial)"""
    o_ns = nostdlib()
    side, imgs = orientation_images(r)
    for seed, img in imgs:
        exp = o_ns.orientation(img, side // 2, side // 2, r)
        for mem in mems:
            got = g.compute_orientation_nostdlib(mem.put(img), side // 2, side // 2, r)
            assert _float_bits(got) == _float_bits(exp), (r, seed, mem.kind, got, exp)


# ---------------------------------------------------------------------------------------------------- ring box kernels
RING_SHAPES = [(32, 17), (48, 40), (272, 33), (96, 17), (1040, 19), (64, 70),
               (33, 17), (47, 40), (270, 33), (63, 35), (1038, 19), (65, 70), (81, 33)]
# one shape per wider block size (a thread owns 16 px: 128 threads above 1024 px, 256 above 2048), whole and ragged strips
RING_SHAPES_WIDE = [(2064, 35), (2071, 35), (4096, 33), (3838, 34)]
RING_RADII = tuple(range(1, 17))
# both sides of every clamp of the product form of the compare (k_box.h), and the constants that leave it
RING_C = (5, -7, 300, -300, 255, -255, 256, 0, (1 << 30) - 1, -(1 << 30) + 1, 1 << 30, -(1 << 31))
RING_C_WIDE = (5, -300, 256)


def ring_radii(shape):
    """the radii whose ring kernel a frame of that shape takes: shorter frames take k_box16 (the any-radius cases)"""
    return [r for r in RING_RADII if shape[1] >= 2 * r + 1]


def is_ring_case(w, h, r, c, key6):
    """the preconditions of the register-ring route, restated from launch_box_generic (gs_stencil.cpp): the default route
    (key 6 = 0), a strip-kernel frame of at least two threads, the whole window inside the frame's height, a radius that has a
    ring kernel, and for the adaptive compare a constant inside the product form.  c = None is gs_blur, whose radii 1 .. 3
    are k_blur16's on such frames (launch_blur)"""
    if key6 != 0 or not (32 <= w <= 4096 and 1 <= r <= 16 and h >= 2 * r + 1):
        return False
    return r >= 4 if c is None else -(1 << 30) < c < (1 << 30)


def ring_images(shape, wide=False):
    w, h = shape
    rng = np.random.RandomState(w + h)
    imgs = [rng.randint(0, 256, (h, w)).astype(np.uint8), np.full((h, w), 255, np.uint8)]
    if not wide:
        imgs.append(Oracle.synth(w, h, 7))
        imgs[2][:, : w // 2] |= 0xF0
    return imgs


def box_ring(g, o, mems, shape, r, wide=False):
    """k_box16r<MODE, r> (the window's raw rows in a register ring, constant tap counts, multiply-high quotient from a table
    for clipped rows too) against the oracle, and the same inputs through k_box16 (gsh_tune key 6 = 4) and through the integral
    table + k_box_px (key 6 = 3): three routes, one answer.  Bright images (largest sums), bands of 1, 5, 2 r + 1 and 2 r + 2
    rows (key 0), compare constants on both sides of every clamp of the product form and four outside it.  Ragged widths: the
    ring kernel over the whole strips with the last one a feeder + k_box_edge for the last 16 + w % 16 columns.  (gs_blur with
    r <= 3 is k_blur16 on these widths; the adaptive form is the ring kernel at every radius.)

    Returns how many calls met is_ring_case, blur and adaptive."""
    w, h = shape
    assert h >= 2 * r + 1, "a shorter frame takes k_box16: not a case of this function"
    imgs = ring_images(shape, wide)
    cs = RING_C_WIDE if wide else RING_C
    exp_blur = [o.blur(img, r) for img in imgs]
    exp_adapt = [{c: o.adaptive_threshold(img, r, c) for c in cs} for img in imgs]
    ring = [0, 0]

    def blur(mem, s, k, what):
        d = mem.zeros((h, w), fill=SENTINEL)
        g.blur(d, s, r)
        assert_same(mem.get(d), exp_blur[k], "gs_blur r=%d %s img %d %dx%d (%s)" % (r, what, k, w, h, mem.kind))

    def adapt(mem, s, k, c, what):
        d = mem.zeros((h, w), fill=SENTINEL)
        g.adaptive_threshold(d, s, r, c)
        assert_same(mem.get(d), exp_adapt[k][c], "gs_adaptive_threshold r=%d c=%d %s img %d %dx%d (%s)" % (r, c, what, k, w, h, mem.kind))

    for mem in mems:
        src = [mem.put(img) for img in imgs]
        with tuned(g, {0: 0}):
            for k in range(len(imgs)):
                for T in ((0,) if k else (0, 1, 5, 2 * r + 1, 2 * r + 2)):
                    g.tune(0, T)
                    blur(mem, src[k], k, "T=%d" % T)
                    ring[0] += is_ring_case(w, h, r, None, 0)
                    for c in (cs if T == 0 else (5,)):
                        adapt(mem, src[k], k, c, "T=%d" % T)
                        ring[1] += is_ring_case(w, h, r, c, 0)
        for key6, what in ((4, "k_box16"), (3, "integral route")):  # the other two routes on the same input
            with tuned(g, {6: key6}):
                assert not is_ring_case(w, h, r, 5, key6)
                blur(mem, src[0], 0, what)
                adapt(mem, src[0], 0, 5, what)
    return ring


# ---------------------------------------------------------------------------------------------------- any-radius box
ANY_RADII = (30, 31, 32, 33, 56, 57, 100, 127)
ANY_SHAPES = ((96, 80), (272, 90))


def box_any_radius(g, o, mems, r, shapes=ANY_SHAPES):
    """k_box16: the quotient of unclipped rows is one multiply up to r = 31 and the float estimate + fix-up beyond; the sliding
    route serves radii up to 127 (u16 column sums, 128-entry LDS halo).  gs_blur and gs_adaptive_threshold on images with a
    bright half (large sums)"""
    rng = np.random.RandomState(3)
    for (w, h) in shapes:
        img = rng.randint(0, 256, (h, w)).astype(np.uint8)
        img[:, :w // 2] |= 0xF0
        eb, ea = o.blur(img, r), o.adaptive_threshold(img, r, -3)
        for mem in mems:
            s = mem.put(img)
            d = mem.zeros(img.shape, fill=SENTINEL)
            g.blur(d, s, r)
            assert_same(mem.get(d), eb, "gs_blur r=%d %dx%d (%s)" % (r, w, h, mem.kind))
            d = mem.zeros(img.shape, fill=SENTINEL)
            g.adaptive_threshold(d, s, r, -3)
            assert_same(mem.get(d), ea, "gs_adaptive_threshold r=%d %dx%d (%s)" % (r, w, h, mem.kind))


BAND_HEIGHTS = (1, 2, 3, 8, 17, 50, 200)


def box_band_heights(g, o, mem, heights=BAND_HEIGHTS):
    """k_box16 / k_box16r with bands of 1 .. 200 rows (gsh_tune key 0; the launcher itself picks 8 .. h) on a batch of three
    50 x 64 frames, r = 4, 9 and 20"""
    rng = np.random.RandomState(11)
    img = rng.randint(0, 256, (3, 50, 64)).astype(np.uint8)
    exp = {r: [o.blur(img[f], r) for f in range(3)] for r in (4, 9, 20)}
    s = mem.put(img)
    with tuned(g, {0: 0}):
        for T in heights:
            g.tune(0, T)
            for r in (4, 9, 20):
                d = mem.zeros(img.shape, fill=SENTINEL)
                g.blur_batch(d, s, r)
                g.sync()
                got = mem.get(d)
                for f in range(3):
                    assert_same(got[f], exp[r][f], "band height %d, r=%d, frame %d" % (T, r, f))


FULL_WIDTH_SHAPES = ((4096, 4), (4080, 3))
FULL_WIDTH_RADII = (4, 31, 32, 127)


def box_full_width(g, o, mems, shape, radii=FULL_WIDTH_RADII):
    """rows as wide as the box kernels go (4096 = 256 threads x 16 px) with radii on both sides of every switch"""
    w, h = shape
    wide = np.random.RandomState(11 + w).randint(0, 256, (h, w)).astype(np.uint8)
    for r in radii:
        eb, ea = o.blur(wide, r), o.adaptive_threshold(wide, r, 3)
        for mem in mems:
            s = mem.put(wide)
            d = mem.zeros(wide.shape, fill=SENTINEL)
            g.blur(d, s, r)
            assert_same(mem.get(d), eb, "gs_blur r=%d %dx%d (%s)" % (r, w, h, mem.kind))
            d = mem.zeros(wide.shape, fill=SENTINEL)
            g.adaptive_threshold(d, s, r, 3)
            assert_same(mem.get(d), ea, "gs_adaptive_threshold r=%d %dx%d (%s)" % (r, w, h, mem.kind))


# ---------------------------------------------------------------------------------------------------- strip launch tuning
# geom: block shape 64 x 4, 256 x 1, 128 x 2 (gsh_tune key 1 = 1, 3, 2); frame: one of three frame shapes
STRIP_GEOM_KEY = (1, 3, 2)
STRIP_FRAMES = {1: (2064, 11), 2: (64, 23), 3: (4112, 4)}
STRIP_BAND_ROWS = (0, 1, 5)


def strip_launch_tuning(g, o, mems, geom, frame):
    """gsh_tune: block shape x rows-per-band, incl. bands of 1 row, a 256 x 1 block on a 64-px frame and a 64 x 4 block on a
    4112-px frame: blur r = 1, 2, 3, sobel, erode and dilate are the oracle's under every one"""
    w, h = STRIP_FRAMES[frame]
    with tuned(g, {0: 0, 1: 0}):
        for T in STRIP_BAND_ROWS:
            g.tune(0, T), g.tune(1, STRIP_GEOM_KEY[geom])
            for mem in mems:
                stencils(g, o, Oracle.synth(w, h, w + h + T), mem, radii=(1, 2, 3))


# ---------------------------------------------------------------------------------------------------- FAST
FAST_THRESHOLDS = (0, 1, 255, 256, 300, 0x7fffffff, 0x80000000, 0xffffff00, 0xffffff01, 0xfffffff0, 0xffffffff)


def fast_shape(g, o, mem, shape):
    """gs_fast under both score kernels (gsh_tune key 7: 0 LDS tile, 4 px per thread + candidate queue (default), 2 one global
    byte load per ring pixel): a generated frame, noise at a low threshold with caps 5000 and 1, p < t everywhere, and noise
    under every threshold of FAST_THRESHOLDS, incl. those where p + t wraps"""
    w, h = shape
    for strip in (0, 2):
        with tuned(g, {7: strip}):
            fast(g, o, Oracle.synth(w, h, 5), mem)
            rs = np.random.RandomState(1)
            fast(g, o, rs.randint(0, 256, (h, w)).astype(np.uint8), mem, threshold=5, caps=(5000, 1))
            fast(g, o, rs.randint(0, 40, (h, w)).astype(np.uint8), mem, threshold=30)  # p < t everywhere
            img = rs.randint(0, 256, (h, w)).astype(np.uint8)
            for t in FAST_THRESHOLDS:
                fast(g, o, img, mem, threshold=t, caps=(5000,))


FAST_RAGGED_TILE_SHAPES = ((70, 23), (131, 77), (64, 38), (200, 135))


def fast_tiles_that_stick_out(g, o, mem):
    """k_fast_score_q4<48>: a thread filters 4 pixels of three tile rows, the candidate queue and the in-place path for dense
    tiles span the 48-row tile; frame heights that leave ragged last tiles"""
    rs = np.random.RandomState(31)
    for (w, h) in FAST_RAGGED_TILE_SHAPES:
        fast(g, o, Oracle.synth(w, h, 5), mem)
        fast(g, o, rs.randint(0, 256, (h, w)).astype(np.uint8), mem, threshold=5, caps=(5000,))   # dense: scored in place
        fast(g, o, (rs.randint(0, 256, (h, w)) * (rs.rand(h, w) < 0.2)).astype(np.uint8), mem, threshold=40)


def fast_batch_in_xcd_order(g, o, mem, order):
    """k_fast_score_q4 numbers its 64 x 16 tiles over the whole batch and hands XCD k the k-th eighth of them (gsh_tune
    key 18 = 1: launch order): 5 frames of 4 x 3 tiles = 60 tiles, so the 1-D grid has four blocks without a tile"""
    n, h, w = 5, 40, 200
    frames = np.stack([Oracle.synth(w, h, 30 + f) for f in range(n)])
    frames[3, 5:30, 20:150] = np.random.RandomState(3).randint(0, 256, (25, 130))
    sm = mem.zeros(frames.shape)
    kps = mem.zeros((n, 300, 12), np.uint32, fill=0xABABABAB)
    counts = mem.zeros(n, np.uint32, fill=0xABABABAB)
    with tuned(g, {18: order}):
        g.fast_batch(mem.put(frames), sm, kps, counts, 300, 20)
        g.sync()
    sm, kps, counts = mem.get(sm), mem.get(kps, np.uint32), mem.get(counts, np.uint32)
    for f in range(n):
        ko, smo = o.fast(frames[f], 300, 20)
        assert counts[f] == len(ko), f
        assert_same(kps[f, :len(ko)].reshape(-1).view(ko.dtype), ko, "frame %d" % f)
        assert_same(sm[f], smo, "scoremap %d" % f)


SCORE_MAP_SIZES = ((96, 72), (91, 70), (50, 72), (96, 30), (101, 80), (40, 33), (4, 4))


def fast_score_map_of_another_size(g, reference, mems):
    """the reference writes the score map through gs_set and reads it through gs_get (ref :512, :518-524): a map smaller or
    larger than the image is legal, positions outside it read 0 and are never written"""
    img = Oracle.synth(96, 72, 31)
    rs = np.random.RandomState(5)
    for (sw, sh) in SCORE_MAP_SIZES:
        sm0 = rs.randint(0, 3, (sh, sw)).astype(np.uint8)  # a caller's map is not necessarily zeroed
        exp, sm_exp = reference.fast(img, 500, 20, scoremap=sm0)
        for mem in mems:
            sm = mem.put(sm0)
            got = g.fast(mem.put(img), sm, 500, 20)
            assert_same(got, exp, "keypoints with a %dx%d map (%s)" % (sw, sh, mem.kind))
            assert_same(mem.get(sm), sm_exp, "score map %dx%d after the call (%s)" % (sw, sh, mem.kind))


# ---------------------------------------------------------------------------------------------------- histogram
HIST_ALIGNMENT_SHAPES = [(1, 1), (3, 1), (5, 3), (1, 16), (17, 1), (31, 1), (11, 3), (1, 33), (7, 9), (70, 1), (4099, 1), (37, 111),
                         (256 * 16 * 3 + 5, 1)]


def _hist_prefill(mem, n):
    """a histogram output that holds 0xAB bytes: gsh_histogram_batch writes every bin, it adds to nothing"""
    return mem.zeros((n, 256), np.uint32, fill=0xABABABAB)


def histogram_every_alignment(g, o, mem):
    """k_hist_partial counts whole 16-byte chunks from a queue of loads in flight and the bytes before the first / after the
    last whole chunk one by one: frames of 1 .. 70 bytes and 4 KB +- a few at every base alignment (frame f of a batch starts
    at f * w * h bytes; the last load of the last frame straddles the end of the buffer)"""
    rng = np.random.RandomState(11)
    for w, h in HIST_ALIGNMENT_SHAPES:
        n = 17 if w * h < 5000 else 3
        a = rng.randint(0, 256, (n, h, w)).astype(np.uint8)
        hist = _hist_prefill(mem, n)
        g.histogram_batch(mem.put(a), hist)
        g.sync()
        hist = mem.get(hist, np.uint32)
        for f in range(n):
            assert np.array_equal(hist[f], o.histogram(a[f])), (w, h, f)


HIST_PIECES = [(4096, (1, 37, 300)), (1000, (2, 70, 1000)), (333, (3, 9, 111)), (999, (1, 1, 999)), (999, (1, 2, 999)), (5000, (1, 1, 4999))]


def histogram_in_pieces(g, o, mem):
    """images above 1 GB are counted in pieces (k_hist_partial addresses a frame with 32-bit offsets); gsh_tune key 12 lowers
    the piece size so that 1000 .. 70000-byte images take that path: whole pieces + a remainder, odd piece sizes (every piece
    starts at another alignment), batches"""
    rng = np.random.RandomState(5)
    with tuned(g, {12: 0}):
        for piece, (n, h, w) in HIST_PIECES:
            g.tune(12, piece)
            a = rng.randint(0, 256, (n, h, w)).astype(np.uint8)
            src = mem.put(a)
            hist = _hist_prefill(mem, n)
            g.histogram_batch(src, hist)
            g.sync()
            got = mem.get(hist, np.uint32)
            for f in range(n):
                assert np.array_equal(got[f], o.histogram(a[f])), (piece, n, h, w, f)
            thr = mem.zeros(n, np.uint8, fill=SENTINEL)
            g.otsu_batch(src, hist, thr)
            g.sync()
            assert [int(t) for t in mem.get(thr)] == [o.otsu_threshold(a[f]) for f in range(n)]


# ---------------------------------------------------------------------------------------------------- fused pipeline
FUSED_SHAPES = [(64, 23), (2064, 9), (4112, 5), (32, 3), (48, 4)]


def fused_edge_pipeline(g, o, mem, radius, shape):
    """gsh_edge_pipeline_batch(tmp=NULL): fused blur->sobel->histogram kernel vs the oracle chain, bands of the launcher's
    choice, of 1 and of 3 rows"""
    w, h = shape
    n = 2
    src = np.stack([Oracle.synth(w, h, 300 + w + i) for i in range(n)])
    exp = []
    for i in range(n):
        s = o.sobel(o.blur(src[i], radius))
        t = o.otsu_threshold(s)
        exp.append((o.histogram(s), t, o.threshold(s, t)))
    s_m = mem.put(src)
    with tuned(g, {0: 0}):
        for T in (0, 1, 3):
            g.tune(0, T)
            out = mem.zeros(src.shape, fill=7)
            hist = _hist_prefill(mem, n)
            thr = mem.zeros(n, np.uint8, fill=SENTINEL)
            g.edge_pipeline_batch(out, None, s_m, radius, hist, thr)
            g.sync()
            got_out, got_hist, got_thr = mem.get(out), mem.get(hist, np.uint32), mem.get(thr)
            for i in range(n):
                assert np.array_equal(got_hist[i], exp[i][0]), "histogram of the sobel image (T=%d, frame %d)" % (T, i)
                assert got_thr[i] == exp[i][1], (T, i)
                assert_same(got_out[i], exp[i][2], "thresholded edges (T=%d, frame %d)" % (T, i))


def blur_sobel_batch(g, o, mem, radius, nhw=(2, 21, 64)):
    """gsh_blur_sobel_batch == gs_blur then gs_sobel into a zeroed image (fused for radius 1..3)"""
    n, h, w = nhw
    src = np.stack([Oracle.synth(w, h, 40 + i) for i in range(n)])
    dst = mem.zeros(src.shape, fill=9)
    g.blur_sobel_batch(dst, mem.put(src), radius)
    g.sync()
    got = mem.get(dst)
    for i in range(n):
        assert_same(got[i], o.sobel(o.blur(src[i], radius)), "blur_sobel r=%d frame %d" % (radius, i))


def template_wider_than_the_lds_tile(g, o, mems):
    """templates wider than 16381 px take the per-tap kernel; 16380 is the widest dot4 / LDS-row case"""
    rs = np.random.RandomState(2)
    for (iw, ih, tw, th) in ((16420, 3, 16400, 2), (16400, 2, 16380, 2)):
        img = rs.randint(0, 256, (ih, iw)).astype(np.uint8)
        t = rs.randint(0, 256, (th, tw)).astype(np.uint8)
        exp = o.match_template(img, t)
        for mem in mems:
            r = mem.zeros((ih - th + 1, iw - tw + 1), fill=SENTINEL)
            g.match_template(mem.put(img), mem.put(t), r)
            assert_same(mem.get(r), exp, "gs_match_template %dx%d (%s)" % (tw, th, mem.kind))
