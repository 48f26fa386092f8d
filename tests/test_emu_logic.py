"""Kernel LOGIC parity on CPU: the same kernel sources (grayskull_amd/csrc/k_*.h + gs_*.cpp)
compiled for the host-fiber SIMT emulator (tests/emu) and compared with the oracle on tiny
inputs.  This is a development/CI aid for a container without a GPU -- the real parity tests are
the `-m gpu` ones, which run the HIP build on the MI355X: test_gpu_parity.py, and test_gpu_kernel_logic.py
for the cases whose bodies live in kernel_logic_cases.py and run here and there."""
import ctypes as C
import os

import numpy as np
import pytest

import kernel_logic_cases as kl
import parity_cases as pc
from oracle.pyoracle import Oracle
from util import assert_same, lena, random_cascade

MEM = pc.Mem("host")

# widths: ragged (px kernels), multiples of 16 (strip kernels), >1024 (wave seams), tiny
SHAPES = [(67, 45), (64, 40), (16, 16), (1040, 7), (2064, 5), (33, 3), (1, 1), (2, 2), (3, 3), (16, 1), (7, 64)]


@pytest.mark.parametrize("shape", SHAPES)
def test_stencils(emu, oracle, shape):
    w, h = shape
    pc.stencils(emu, oracle, Oracle.synth(w, h, w * 7 + h), MEM)
    rs = np.random.RandomState(w + h)
    pc.stencils(emu, oracle, rs.randint(0, 256, (h, w)).astype(np.uint8), MEM, radii=(1, 2, 3, 9))


def test_stencils_extremes(emu, oracle):
    for v in (0, 255):
        pc.stencils(emu, oracle, np.full((9, 48), v, np.uint8), MEM)
    chk = ((np.indices((10, 32)).sum(0) % 2) * 255).astype(np.uint8)
    pc.stencils(emu, oracle, chk, MEM)
    pc.stencils(emu, oracle, Oracle.synth(20, 9, 3), MEM, radii=(0, 20, 1000))  # radius >= image


@pytest.mark.parametrize("shape", [(67, 45), (64, 40), (1, 1), (5, 1), (1031, 3), (48, 33), (2064, 4), (4096, 3), (272, 70)])
def test_pointwise_and_integral(emu, oracle, shape):
    w, h = shape
    img = Oracle.synth(w, h, 11 + w)
    pc.pointwise(emu, oracle, img, MEM)
    pc.integral(emu, oracle, img, MEM)
    pc.integral(emu, oracle, np.full((h, w), 255, np.uint8), MEM)


def test_otsu_scan_float_order(emu, oracle):
    """histograms whose float32 sums exceed 2^24 (rounding order matters)"""
    rs = np.random.RandomState(5)
    for _ in range(3):
        img = rs.choice(256, size=(96, 256), p=rs.dirichlet(np.ones(256) * 0.3)).astype(np.uint8)
        assert emu.otsu_threshold(img) == oracle.otsu_threshold(img)


@pytest.mark.parametrize("shape", [(67, 45), (40, 24), (64, 40), (48, 9), (32, 3), (1040, 5), (32, 1), (272, 150)])
def test_next_rows(emu, oracle, shape):
    w, h = shape
    pc.next_rows(emu, oracle, Oracle.synth(w, h, 21), MEM)
    pc.next_rows(emu, oracle, np.random.RandomState(w + h).randint(0, 256, (h, w)).astype(np.uint8), MEM)


@pytest.mark.parametrize("shape", [(67, 45), (96, 80), (7, 7), (6, 30), (40, 8), (300, 12), (260, 17), (8, 8), (516, 9),
                                   (64, 40), (48, 7), (32, 16), (1040, 9), (2064, 8)])
def test_fast(emu, oracle, shape):
    kl.fast_shape(emu, oracle, MEM, shape)


def test_fast_score_tiles_that_stick_out_of_the_frame(emu, oracle):
    """k_fast_score_q4<48>: a thread filters 4 pixels of three tile rows, the candidate queue and the in-place path for dense
    tiles span the 48-row tile; frame heights that leave ragged last tiles"""
    kl.fast_tiles_that_stick_out(emu, oracle, MEM)


def test_fast_tile_kernel_equals_per_pixel_kernel(emu, oracle):
    """k_fast_score_q4 (the default) against k_fast_score_px (gsh_tune key 7 = 2: one global byte load per ring pixel) and the
    oracle: block corners, noise and a p < t region, two waves wide"""
    rs = np.random.RandomState(11)
    img = Oracle.synth(264, 40, 9)
    img[8:20, 100:140] = rs.randint(0, 12, (12, 40))       # p < threshold: the unsigned-wrap class
    img[25:33, 250:264] = rs.randint(0, 256, (8, 14))      # texture up to the right border
    for t in (20, 3, 200):
        pc.fast(emu, oracle, img, MEM, threshold=t, caps=(5000,))
        for mode in (2,):
            emu.tune(7, mode)
            try:
                pc.fast(emu, oracle, img, MEM, threshold=t, caps=(5000,))
            finally:
                emu.tune(7, 0)
        emu.tune(18, 1)  # default score kernel with its tiles in launch order instead of the XCD-aware order
        try:
            pc.fast(emu, oracle, img, MEM, threshold=t, caps=(5000,))
        finally:
            emu.tune(18, 0)


@pytest.mark.parametrize("shape", [(96, 80), (64, 40), (1040, 9), (32, 7), (272, 33)])
def test_fast_sparse_nms_kernel_equals_item_kernel(emu, oracle, shape):
    """pass 2 of gs_fast: k_fast_nms_sparse (default: only the pixels of the score kernel's bitmap) and k_fast_nms (item by
    item, gsh_tune key 19 = 1) give the oracle's keypoints in the oracle's order -- plateaus (ties survive), peaks next to the
    never-written 3-px frame of a caller's non-zero score map, caps that cut the list inside a row"""
    w, h = shape
    rs = np.random.RandomState(w + h)
    flat = np.full((h, w), 100, np.uint8)
    flat[::3, ::3] = 140                      # a lattice of equal corners: plateaus / ties everywhere
    imgs = [Oracle.synth(w, h, 8), rs.randint(0, 256, (h, w)).astype(np.uint8), flat]
    for key19 in (0, 1):
        try:
            emu.tune(19, key19)
            for img in imgs:
                pc.fast(emu, oracle, img, MEM, threshold=12, caps=(5000, 9, 1))
        finally:
            emu.tune(19, 0)


def test_fast_quirk(emu, oracle):
    pc.fast_unsigned_wrap_quirk(emu, oracle, MEM)


@pytest.mark.parametrize("shape", [(96, 80), (67, 45)])
def test_orb_and_match(emu, oracle, shape):
    w, h = shape
    pc.orb(emu, oracle, Oracle.synth(w, h, 7), MEM)


@pytest.mark.parametrize("n1,n2", [(1, 1), (5, 63), (7, 64), (3, 65), (9, 255), (4, 257), (6, 300), (70, 513), (2, 1030)])
def test_match_orb_on_random_descriptors_around_the_trip_sizes(emu, oracle, n1, n2):
    """k_match reads four train descriptors per lane and trip (64 lanes x 4 = 256 per trip, index clamped past the end): train
    sets of 1, 63 .. 65, 255 .. 257, 300, 513, 1030 descriptors, with duplicated train descriptors (the FIRST index of the
    minimum wins, ref :690), exact partners, near partners and the 0.8 ratio test on both sides"""
    pc.match_random(emu, oracle, n1, n2)


@pytest.mark.parametrize("shape,levels,nkps", [((130, 70), 4, 50), ((96, 80), 3, 31), ((64, 64), 3, 10)])
def test_orb_pyramid(emu, oracle, shape, levels, nkps):
    w, h = shape
    pc.orb_pyramid(emu, oracle, Oracle.synth(w, h, 21), MEM, nkps=nkps, levels=levels)


@pytest.mark.parametrize("shape", [(67, 45), (40, 8), (5, 3), (130, 33)])
def test_geometry_and_template_matching(emu, oracle, shape):
    w, h = shape
    pc.geometry(emu, oracle, Oracle.synth(w, h, 3 * w + h), MEM)
    pc.geometry(emu, oracle, np.random.RandomState(w).randint(0, 256, (h, w)).astype(np.uint8), MEM, seed=9)


@pytest.mark.parametrize("case", [(100, 80, 16, 4), (131, 70, 17, 5), (200, 150, 31, 8), (97, 90, 32, 32), (260, 140, 64, 64),
                                  (300, 200, 128, 128), (290, 66, 160, 3 + 1), (64, 64, 64, 64), (129, 65, 33, 33), (400, 40, 256, 8)])
def test_match_template_on_the_matrix_cores(emu, oracle, case):
    """k_match_template_mfma (templates of 16 x 4 .. 32768 taps): the cross term as Toeplitz matrix products in the i8 MFMA
    accumulator, sum I'^2 from the two sliding-sum kernels (key 20 = 5: from four corners of the integral table of squares, the route of frames of 4 Mpx and more) -- against the oracle and against the dot-product kernels
    (gsh_tune key 20 = 1): result sizes below, at and above the 128 x 64 block tile, widths that leave 1 .. 31 columns in
    the last K step, a template as large as the image, all-0 / all-255 images against all-255 / all-0 templates (the
    largest sums), and an exact sub-image (score 255 at its place)"""
    iw, ih, tw, th = case
    rs = np.random.RandomState(iw + tw)
    img = rs.randint(0, 256, (ih, iw)).astype(np.uint8)
    tmpls = [rs.randint(0, 256, (th, tw)).astype(np.uint8), img[ih - th:, iw - tw:].copy(), np.full((th, tw), 255, np.uint8)]
    imgs = [img, img, np.zeros_like(img)]
    if tw * th <= 4096:
        tmpls.append(np.zeros((th, tw), np.uint8)); imgs.append(np.full_like(img, 255))
    try:
        for im, t in zip(imgs, tmpls):
            ro = oracle.match_template(im, t)
            for tiles in (2, 3, 8, 5):  # 8: 64 x 128 tiles with the template taken a band of 32 rows at a time; 64 x 128 tiles / 32 x 64 tiles with the template rows split over the block's waves / 5: sum I'^2 from the integral table of squares
                emu.tune(20, tiles)
                r = np.zeros((ih - th + 1, iw - tw + 1), np.uint8)
                emu.match_template(im, t, r)
                assert_same(r, ro, "gs_match_template (mfma, key 20 = %d) %dx%d on %dx%d" % (tiles, tw, th, iw, ih))
    finally:
        emu.tune(20, 0)
    try:
        emu.tune(20, 1)
        r = np.zeros((ih - th + 1, iw - tw + 1), np.uint8)
        emu.match_template(img, tmpls[0], r)
        assert_same(r, oracle.match_template(img, tmpls[0]), "gs_match_template (dot4) %dx%d" % (tw, th))
    finally:
        emu.tune(20, 0)


def test_template_wider_than_the_lds_tile(emu, oracle):
    """templates wider than 16381 px take the per-tap kernel; 16380 is the widest dot4 / LDS-row case"""
    kl.template_wider_than_the_lds_tile(emu, oracle, (MEM,))


def test_orb_batch(emu, oracle):
    frames = np.stack([Oracle.synth(96, 80, 31), np.zeros((80, 96), np.uint8), Oracle.synth(96, 80, 32),
                       np.random.RandomState(3).randint(0, 256, (80, 96)).astype(np.uint8)])
    pc.orb_batch(emu, oracle, frames, MEM, nkps=40)
    pc.orb_batch(emu, oracle, frames[:1], MEM, nkps=3)
    pc.orb_batch(emu, oracle, np.stack([Oracle.synth(40, 6, 1)]), MEM)  # below FAST's minimum size


def test_orb_batch_with_the_host_thread_pool(emu, oracle):
    """gsh_orb_extract_batch with more than 4096 kept keypoints: the libm half (atan2f / sinf per keypoint) is spread over
    the library's parked host threads (HostPool); twice, so that the second call runs on workers that already exist"""
    rs = np.random.RandomState(21)
    frames = rs.randint(0, 256, (12, 96, 176)).astype(np.uint8)  # noise: hundreds of corners per frame
    for _ in range(2):
        pc.orb_batch(emu, oracle, frames, MEM, nkps=400)
    got = emu.orb_extract_batch_dev(MEM.put(frames), MEM.put(np.zeros_like(frames)), 400, 20)
    assert sum(len(k) for k in got) >= 4096, "the case must reach the pool's threshold"


def test_orb_batch_host_pool_survives_fork(emu, oracle):
    """a fork()ed child (Python multiprocessing's default start method) inherits the pool object but none of its parked
    threads: it must build its own workers instead of waiting for the parent's (which hung gsh_orb_extract_batch), and its
    exit must not join threads that do not exist.  Emulator only: a forked HIP runtime is not supported by ROCm itself."""
    import signal
    rs = np.random.RandomState(22)
    frames = rs.randint(0, 256, (12, 96, 176)).astype(np.uint8)
    want = emu.orb_extract_batch_dev(MEM.put(frames), MEM.put(np.zeros_like(frames)), 400, 20)  # parent: workers exist now
    assert sum(len(k) for k in want) >= 4096
    pid = os.fork()
    if pid == 0:
        code = 3
        try:
            signal.alarm(60)  # a hang ends the child, not the test session
            got = emu.orb_extract_batch_dev(MEM.put(frames), MEM.put(np.zeros_like(frames)), 400, 20)
            code = 0 if all(a.tobytes() == b.tobytes() for a, b in zip(got, want)) and len(got) == len(want) else 4
        finally:
            os._exit(code)
    _, status = os.waitpid(pid, 0)
    assert os.WIFEXITED(status) and os.WEXITSTATUS(status) == 0, "child: status %#x" % status
    again = emu.orb_extract_batch_dev(MEM.put(frames), MEM.put(np.zeros_like(frames)), 400, 20)  # the parent's pool is intact
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, want))


def test_lbp(emu, oracle, cascade):
    img = Oracle.synth(96, 80, 7)
    pc.lbp(emu, oracle, img, MEM, cascade, params=((4096, 1.1, 1.0, 4.0, 1), (10, 1.3, 1.0, 2.0, 3)),
           windows=((0, 0, 1.0), (5, 3, 1.2), (72, 56, 1.0), (73, 56, 1.0), (0, 0, 3.4)))
    # a permissive random cascade: hundreds of hits -> exercises (scale, y, x) order and the cap
    rc = random_cascade(1)
    pc.lbp(emu, oracle, Oracle.synth(64, 48, 9), MEM, rc,
           params=((4096, 1.25, 1.0, 2.0, 2), (37, 1.25, 1.0, 2.0, 1), (1, 1.5, 1.0, 1.6, 1)),
           windows=((0, 0, 1.0), (1, 0, 1.0), (0, 1, 1.5), (40, 24, 1.0)))


def test_lena_pipeline(emu, oracle, kat):
    """config 1 on the reference's own fixture, against the reference-generated hashes"""
    from util import fnv
    img = lena()
    a, b = np.zeros_like(img), np.zeros_like(img)
    emu.blur(a, img, 2)
    emu.sobel(b, a)
    assert fnv(a) == kat["lena"]["blur"]["2"] and fnv(b) == kat["lena"]["blur_sobel"]
    t = emu.otsu_threshold(img)
    assert t == kat["lena"]["otsu_src"]
    c = img.copy()
    emu.threshold(c, t)
    assert fnv(c) == kat["lena"]["thr_src"]
    # BASELINE configs[0] proper: lena resized to 512x512 (gs_resize, float32 bilinear), blur 2, sobel into a
    # zeroed image -- SURVEY 8(c) hash of the reference's output
    big = np.zeros((512, 512), np.uint8)
    emu.resize(big, img)
    a5, b5 = np.zeros_like(big), np.zeros_like(big)
    emu.blur(a5, big, 2)
    emu.sobel(b5, a5)
    assert fnv(b5) == kat["lena"]["resize512_blur2_sobel"]


@pytest.mark.parametrize("radius", [1, 2, 3, 5])
def test_blur_sobel_batch(emu, oracle, radius):
    """gsh_blur_sobel_batch == gs_blur then gs_sobel into a zeroed image (fused for radius 1..3)"""
    kl.blur_sobel_batch(emu, oracle, MEM, radius)


def test_batch_entry_points(emu, oracle):
    """gsh_* batch calls (emulator: 'device' memory is host memory)"""
    n, h, w = 3, 20, 48
    src = np.stack([Oracle.synth(w, h, 100 + i) for i in range(n)])
    dst = np.zeros_like(src)
    emu.blur_batch(dst, src, 2)
    for i in range(n):
        assert np.array_equal(dst[i], oracle.blur(src[i], 2))
    tmp, out = np.zeros_like(src), np.full_like(src, 7)
    hist = np.zeros((n, 256), np.uint32)
    thr = np.zeros(n, np.uint8)
    emu.edge_pipeline_batch(out, tmp, src, 2, hist, thr)
    for i in range(n):
        s = oracle.sobel(oracle.blur(src[i], 2))
        t = oracle.otsu_threshold(s)
        assert thr[i] == t and np.array_equal(hist[i], oracle.histogram(s))
        assert np.array_equal(out[i], oracle.threshold(s, t))
    gen = np.zeros((2, 45, 67), np.uint8)
    emu.synth_batch(gen, 5)
    assert np.array_equal(gen[0], Oracle.synth(67, 45, 5)) and np.array_equal(gen[1], Oracle.synth(67, 45, 6))
    sums = np.zeros(2, np.uint64)
    emu.checksum_batch(gen, sums)
    idx = np.arange(1, 67 * 45 + 1, dtype=np.uint64)
    for i in range(2):
        assert sums[i] == np.sum(idx * (gen[i].reshape(-1).astype(np.uint64) + 1), dtype=np.uint64)


@pytest.mark.parametrize("geom", [0, 1, 2])
@pytest.mark.parametrize("frame", [1, 2, 3])
def test_strip_launch_tuning_never_changes_results(emu, oracle, geom, frame):
    """gsh_tune: block shape x rows-per-band, incl. bands of 1 row"""
    kl.strip_launch_tuning(emu, oracle, (MEM,), geom, frame)


@pytest.mark.parametrize("radius", [1, 2, 3])
@pytest.mark.parametrize("shape", [(64, 23), (2064, 9), (4112, 5), (32, 3), (48, 4)])
def test_fused_edge_pipeline_equals_separate_calls(emu, oracle, radius, shape):
    """gsh_edge_pipeline_batch(tmp=NULL): fused blur->sobel->histogram kernel vs the oracle chain"""
    kl.fused_edge_pipeline(emu, oracle, MEM, radius, shape)


@pytest.mark.parametrize("chunk,n", [(3, 7), (2, 6), (4, 5), (1, 3), (8, 5)])
def test_fused_edge_pipeline_in_chunks(emu, oracle, chunk, n):
    """gsh_edge_pipeline_batch cut into chunks (key 5 = frames per chunk): whole chunks, a shorter last chunk, one frame per
    chunk, one chunk; two band heights.  (On the GPU every chunk's Otsu + threshold pass runs on a side stream under the next
    chunk's kernel; the emulator runs the launches in order.)"""
    w, h = 80, 37
    src = np.stack([Oracle.synth(w, h, 900 + i) for i in range(n)])
    try:
        emu.tune(5, chunk)
        for T in (0, 5):
            emu.tune(0, T)
            out = np.full_like(src, 9)
            hist = np.zeros((n, 256), np.uint32)
            thr = np.zeros(n, np.uint8)
            emu.edge_pipeline_batch(out, None, src, 2, hist, thr)
            for i in range(n):
                s = oracle.sobel(oracle.blur(src[i], 2))
                t = oracle.otsu_threshold(s)
                assert np.array_equal(hist[i], oracle.histogram(s)), "histogram of frame %d" % i
                assert thr[i] == t, "threshold of frame %d" % i
                assert np.array_equal(out[i], oracle.threshold(s, t)), "frame %d" % i
    finally:
        emu.tune(5, 0), emu.tune(0, 0)


@pytest.mark.parametrize("preset", [0, 1, 2, 3])
def test_lbp_survivor_repacking_never_changes_results(emu, oracle, cascade, preset):
    """gsh_tune 4: dense single phase vs block-local survivor re-packing at various stage splits"""
    try:
        emu.tune(4, preset)
        pc.lbp(emu, oracle, Oracle.synth(96, 80, 7), MEM, cascade, params=((4096, 1.1, 1.0, 4.0, 1),))
        pc.lbp(emu, oracle, Oracle.synth(64, 48, 9), MEM, random_cascade(1),
               params=((4096, 1.25, 1.0, 2.0, 2), (37, 1.25, 1.0, 2.0, 1)))
        pc.lbp(emu, oracle, Oracle.synth(80, 60, 11), MEM, random_cascade(4, nstages=6, weaks_per_stage=2),
               params=((500, 1.2, 1.0, 2.5, 1),))
    finally:
        emu.tune(4, 0)


@pytest.mark.parametrize("knob", [3 + 16 * 10, 6 + 16 * 0, 15 + 16 * 0, 4 + 16 * 5, 1000 + 3 + 32 * 5])
def test_lbp_adaptive_first_repack_never_changes_results(emu, oracle, cascade, knob):
    """default preset: the first re-packing point is chosen per block from the survivor count (k_lbp.h
    LbpPhases::adaptive_max); key 9 = max stages + 16 * tenths forces early, late and never-early choices,
    key 4 >= 1000 a custom fixed split -- rectangles are the oracle's for all of them"""
    edges = oracle.sobel(oracle.blur(Oracle.synth(128, 96, 1000), 2))
    try:
        if knob >= 1000: emu.tune(4, knob)
        else: emu.tune(9, knob)
        pc.lbp(emu, oracle, edges, MEM, cascade, params=((4096, 1.1, 1.0, 4.0, 1),))
        pc.lbp(emu, oracle, Oracle.synth(96, 80, 7), MEM, cascade, params=((4096, 1.1, 1.0, 4.0, 1),))
        pc.lbp(emu, oracle, Oracle.synth(64, 48, 9), MEM, random_cascade(1), params=((4096, 1.25, 1.0, 2.0, 2),))
        pc.lbp(emu, oracle, Oracle.synth(80, 60, 11), MEM, random_cascade(4, nstages=3, weaks_per_stage=2),
               params=((500, 1.2, 1.0, 2.5, 1),))
    finally:
        emu.tune(4, 0); emu.tune(9, 0)


def test_lbp_odd_sizes_cascades_and_tables(emu, oracle, cascade):
    """sizes that are not multiples of 64, images barely larger than the window, short / long / strict cascades, caps
    that cut a scale, and tables that are NOT integral images (arbitrary u32 words, what the reference would happily
    index; sums that wrap mod 2^32): the oracle's rectangles every time.  (Round 3 ran these through the optional stage
    prefilter k_lbp_dense as well; that kernel lost on speed and was removed in round 4.)"""
    edges = oracle.sobel(oracle.blur(Oracle.synth(200, 150, 1000), 2))
    if True:
        pc.lbp(emu, oracle, edges, MEM, cascade, params=((4096, 1.1, 1.0, 4.0, 1), (7, 1.1, 1.0, 4.0, 1), (60, 1.3, 1.0, 3.0, 1)))
        pc.lbp(emu, oracle, Oracle.synth(96, 80, 7), MEM, cascade, params=((4096, 1.1, 1.0, 4.0, 1),))
        pc.lbp(emu, oracle, Oracle.synth(40, 30, 3), MEM, cascade, params=((4096, 1.1, 1.0, 4.0, 1),))
        pc.lbp(emu, oracle, Oracle.synth(130, 70, 9), MEM, random_cascade(1), params=((4096, 1.25, 1.0, 2.0, 1), (37, 1.25, 1.0, 2.0, 1)))
        pc.lbp(emu, oracle, Oracle.synth(80, 60, 11), MEM, random_cascade(4, nstages=6, weaks_per_stage=2), params=((500, 1.2, 1.0, 2.5, 1),))
        pc.lbp(emu, oracle, Oracle.synth(80, 60, 12), MEM, random_cascade(5, nstages=3, weaks_per_stage=5), params=((500, 1.2, 1.0, 2.5, 1),))
        pc.lbp(emu, oracle, Oracle.synth(80, 60, 13), MEM, random_cascade(6, nstages=2, weaks_per_stage=7), params=((500, 1.2, 1.0, 2.5, 1),))
        pc.lbp(emu, oracle, Oracle.synth(80, 60, 13), MEM, random_cascade(7, nstages=3, weaks_per_stage=3, permissive=False), params=((500, 1.2, 1.0, 2.5, 1),))
        # a table that is NOT an integral image (arbitrary u32 words, what the reference would happily index):
        rnd = np.random.RandomState(5).randint(0, 2 ** 32, (90, 130), dtype=np.uint64).astype(np.uint32)
        for casc in (cascade, random_cascade(1)):
            assert_same(emu.lbp_detect(casc, rnd.copy(), 4096, 1.2, 1.0, 3.0, 1), oracle.lbp_detect(casc, rnd, 4096, 1.2, 1.0, 3.0, 1),
                        "non-integral table")
        wrap = oracle.integral(np.full((70, 100), 255, np.uint8)) + np.uint32(0xfffffff0)  # wraps mod 2^32 inside the table
        assert_same(emu.lbp_detect(cascade, wrap.copy(), 4096, 1.2, 1.0, 3.0, 1), oracle.lbp_detect(cascade, wrap, 4096, 1.2, 1.0, 3.0, 1),
                    "table offset by a constant: not an integral image at its first row / column")



def test_lbp_cap_reached_in_early_scales(emu, oracle, cascade):
    """config-5 style input (sobel edge map): many hits, max_rects reached before the last scale --
    later scales are skipped on the GPU exactly because they cannot contribute (ref :819-823)"""
    edges = oracle.sobel(oracle.blur(Oracle.synth(160, 120, 1000), 2))
    pc.lbp(emu, oracle, edges, MEM, cascade, params=((4096, 1.1, 1.0, 4.0, 1), (5, 1.1, 1.0, 4.0, 1), (60, 1.2, 1.0, 3.0, 2)))
    pc.lbp(emu, oracle, Oracle.synth(64, 48, 9), MEM, random_cascade(1), params=((3, 1.25, 1.0, 2.0, 1), (200, 1.1, 1.0, 2.0, 1)))


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_lbp_tile_shapes_never_change_results(emu, oracle, cascade, mode):
    """key 14: 1 = k_lbp_cascade for every scale, 2 + i = tile shape i of k_lbp_tile (k_lbp_tile.h: corners from an LDS tile,
    per-wave dense phase, survivors one lane per (window, classifier) pair) wherever its tile fits -- partial tiles at the
    right / bottom edge, steps 1..3, caps inside and across scales, stages longer than 32 classifiers (window-parallel
    fallback of the pair phase), a cascade that ends inside the dense phase"""
    edges = oracle.sobel(oracle.blur(Oracle.synth(200, 150, 1000), 2))
    try:
        emu.tune(14, mode)
        pc.lbp(emu, oracle, edges, MEM, cascade, params=((4096, 1.1, 1.0, 4.0, 1), (7, 1.1, 1.0, 4.0, 1), (60, 1.3, 1.0, 3.0, 2)))
        pc.lbp(emu, oracle, Oracle.synth(96, 80, 7), MEM, cascade, params=((4096, 1.1, 1.0, 4.0, 1), (10, 1.3, 1.0, 2.0, 3)))
        pc.lbp(emu, oracle, Oracle.synth(130, 70, 9), MEM, random_cascade(1), params=((4096, 1.25, 1.0, 2.0, 1), (37, 1.25, 1.0, 2.0, 1), (1, 1.5, 1.0, 1.6, 1)))
        pc.lbp(emu, oracle, Oracle.synth(80, 60, 11), MEM, random_cascade(4, nstages=6, weaks_per_stage=2), params=((500, 1.2, 1.0, 2.5, 1),))
        pc.lbp(emu, oracle, Oracle.synth(80, 60, 12), MEM, random_cascade(5, nstages=4, weaks_per_stage=40), params=((500, 1.2, 1.0, 2.5, 1),))
        pc.lbp(emu, oracle, Oracle.synth(80, 60, 13), MEM, random_cascade(6, nstages=2, weaks_per_stage=7), params=((500, 1.2, 1.0, 2.5, 1),))
        pc.lbp(emu, oracle, Oracle.synth(80, 60, 13), MEM, random_cascade(7, nstages=3, weaks_per_stage=3, permissive=False), params=((500, 1.2, 1.0, 2.5, 1),))
        # tables that are no integral images (mod 2^32 arithmetic must hold in the tile as in the table)
        rnd = np.random.RandomState(5).randint(0, 2 ** 32, (60, 80), dtype=np.uint64).astype(np.uint32)
        rc = random_cascade(2)
        assert_same(emu.lbp_detect(rc, rnd.copy(), 4096, 1.2, 1.0, 3.0, 1), oracle.lbp_detect(rc, rnd, 4096, 1.2, 1.0, 3.0, 1), "random table")
    finally:
        emu.tune(14, 0)


@pytest.mark.parametrize("knob", [1 + 16 * 2, 2 + 16 * 8, 3 + 16 * 0, 1 + 16 * 10, 0 + 16 * 7])
def test_lbp_tile_dense_to_pair_switch_never_changes_results(emu, oracle, cascade, knob):
    """key 15 = first + 16 * tenths: how long a wave of k_lbp_tile stays dense (stages [0, first), then while more than
    tenths/10 of its windows live) before it goes to one lane per (window, classifier) pair -- early, late, never-early;
    first = 0 (key 112) is taken as 1 (it used to read stage[-1])"""
    edges = oracle.sobel(oracle.blur(Oracle.synth(200, 150, 1000), 2))
    try:
        emu.tune(15, knob)
        pc.lbp(emu, oracle, edges, MEM, cascade, params=((4096, 1.1, 1.0, 4.0, 1), (7, 1.1, 1.0, 4.0, 1)))
        pc.lbp(emu, oracle, Oracle.synth(130, 70, 9), MEM, random_cascade(1), params=((4096, 1.25, 1.0, 2.0, 1), (37, 1.25, 1.0, 2.0, 1)))
        pc.lbp(emu, oracle, Oracle.synth(80, 60, 12), MEM, random_cascade(5, nstages=4, weaks_per_stage=14), params=((500, 1.2, 1.0, 2.5, 1),))
    finally:
        emu.tune(15, 0)


def test_lbp_chunk_granular_early_exit(emu, oracle, cascade):
    """max_rects early exit at chunk-group granularity (ref :819-831): a chunk is skipped once the
    detections published by the groups that wholly precede it reach the cap.  The result must be the
    reference's first max_rects hits for every cap; on frames with enough chunks (> 32 per scale)
    small caps must really skip work (counter of evaluated windows)."""
    edges = oracle.sobel(oracle.blur(Oracle.synth(352, 288, 1000), 2))
    ii = oracle.integral(edges)
    total = emu.lbp_window_count(cascade, 352, 288, 1.1, 1.0, 4.0, 1)
    evaluated = {}
    for cap in (1, 20, 60, 4096):
        cnt = np.zeros(4, np.uint64)
        emu.lbp_count_evaluated(cnt)
        try:
            r = emu.lbp_detect(cascade, ii.copy(), cap, 1.1, 1.0, 4.0, 1)
        finally:
            emu.lbp_count_evaluated(None)
        assert_same(r, oracle.lbp_detect(cascade, ii, cap, 1.1, 1.0, 4.0, 1), "cap %d" % cap)
        evaluated[cap] = int(cnt[0])
    assert evaluated[4096] == total, "nothing to skip when the cap is never reached"
    assert evaluated[1] < evaluated[20] < total and evaluated[20] <= evaluated[60] <= total, evaluated
    # a permissive random cascade: thousands of hits per scale, caps inside the first scale / across scales
    rc = random_cascade(2)
    img = Oracle.synth(300, 260, 5)
    ii = oracle.integral(img)
    for cap in (1, 100, 3000, 40000):
        assert_same(emu.lbp_detect(rc, ii.copy(), cap, 1.3, 1.0, 3.0, 1), oracle.lbp_detect(rc, ii, cap, 1.3, 1.0, 3.0, 1),
                    "random cascade cap %d" % cap)


# ---- hardening items of the round-1 review (ADVICE.md / VERDICT.md "What's weak" 7-9) -------------------
def test_cascade_edited_in_place_takes_effect(emu, oracle):
    """the reference re-reads the caller's tables on every call; the flattened copy is cached by a
    hash of the table CONTENTS, so an in-place edit (same pointers, same shapes) must change the result"""
    rc = random_cascade(2)
    ii = oracle.integral(Oracle.synth(96, 80, 7))
    before = emu.lbp_detect(rc, ii.copy(), 4096, 1.2, 1.0, 2.0, 1)
    assert_same(before, oracle.lbp_detect(rc, ii, 4096, 1.2, 1.0, 2.0, 1), "before the edit")
    assert len(before) > 0
    rc.stage_threshold[:] = 1e9       # nothing can pass any more; same arrays, same addresses
    rc.weak_left_val[:] = -1.0
    after = emu.lbp_detect(rc, ii.copy(), 4096, 1.2, 1.0, 2.0, 1)
    assert_same(after, oracle.lbp_detect(rc, ii, 4096, 1.2, 1.0, 2.0, 1), "after the edit")
    assert len(after) == 0
    assert emu.lbp_window(rc, ii.copy(), 0, 0, 1.0) == oracle.lbp_window(rc, ii, 0, 0, 1.0) == 0


def test_synth_after_shutdown_regenerates_its_jump_table(emu):
    a = np.zeros((2, 40, 72), np.uint8)
    emu.synth_batch(a, 11)
    emu.shutdown()  # frees the scratch slot that holds the generator's jump table
    b = np.zeros_like(a)
    emu.synth_batch(b, 11)
    assert_same(a, b, "frames after gsh_shutdown")
    assert_same(a[1], Oracle.synth(72, 40, 12), "generator vs the CPU one")


def test_pyramid_with_zero_levels_or_zero_keypoints_returns_nothing(emu):
    img = Oracle.synth(96, 80, 3)
    buf = np.zeros(Oracle.orb_pyramid_buffer_bytes(96, 80, 3) + 64, np.uint8)
    assert len(emu.orb_extract_pyramid_dev(img, buf, 50, 20, 0)) == 0  # nanomagick.c:262: empty level loop
    assert len(emu.orb_extract_pyramid_dev(img, buf, 0, 20, 3)) == 0


@pytest.mark.parametrize("r", [15, 36, 37, 60, 90])
def test_orientation_any_radius_matches_the_reference_float_order(emu, reference, r):
    """beyond r = 36 the moment sums pass 2^24 and the reference's float32 accumulation order matters"""
    kl.orientation(emu, reference, (MEM,), r)


@pytest.mark.parametrize("r", [37, 60])
def test_orientation_nostdlib_beyond_the_exact_radius(emu, r):
    """the same moments through the GS_NO_STDLIB atan2 polynomial"""
    kl.orientation_nostdlib(emu, (MEM,), r)


def fast_many_frames(g, oracle, n):
    """n tiny frames in one gsh_fast_batch / gsh_orb_extract_batch (SURVEY 8c quirk image: 9x9, all 5, ring of (4,4) = 20)"""
    one = np.full((9, 9), 5, np.uint8)
    for dx, dy in ((0, -3), (1, -3), (2, -2), (3, -1), (3, 0), (3, 1), (2, 2), (1, 3), (0, 3), (-1, 3), (-2, 2), (-3, 1),
                   (-3, 0), (-3, -1), (-2, -2), (-1, -3)):
        one[4 + dy, 4 + dx] = 20
    ko, smo = oracle.fast(one, 4, 20)
    assert len(ko) == 1 and smo[4, 4] == 15
    return one, ko, smo


def test_fast_batch_split_over_several_launches(emu, oracle):
    """the frame index rides in grid.y / grid.z (documented limit 65535; the ROCm 7.0 runtime takes more, as
    tests/test_gpu_shape_frontier.py observes for row-derived grids): every launcher splits big batches; gsh_tune
    key 8 lowers the split size so that 40 frames already take three launches (the GPU suite runs 70,000)"""
    n = 40
    one, ko, smo = fast_many_frames(emu, oracle, n)
    frames = np.repeat(one[None], n, 0)
    frames[n - 1] = 5  # the last frame is flat
    sm = np.zeros_like(frames)
    kps = np.zeros((n, 4, 12), np.uint32)
    counts = np.zeros(n, np.uint32)
    try:
        emu.tune(8, 16)
        emu.fast_batch(frames, sm, kps, counts, 4, 20)
    finally:
        emu.tune(8, 0)
    for f in range(n - 1):
        assert counts[f] == 1, f
        assert_same(kps[f, :1].reshape(-1).view(ko.dtype), ko, "frame %d" % f)
        assert_same(sm[f], smo, "scoremap %d" % f)
    assert counts[n - 1] == 0


@pytest.mark.parametrize("order", [0, 1])
def test_fast_batch_tiles_of_several_frames_in_xcd_order(emu, oracle, order):
    """k_fast_score_q4 numbers its 64 x 16 tiles over the whole batch and hands XCD k the k-th eighth of them (gsh_tune
    key 18 = 1: launch order): 5 frames of 4 x 3 tiles = 60 tiles, so the 1-D grid has four blocks without a tile"""
    kl.fast_batch_in_xcd_order(emu, oracle, MEM, order)


def test_device_resident_orb_with_the_reference_nostdlib_trig(emu, reference):
    """gsh_orb_extract_batch_nostdlib: selection (stable sort by response + border filter + cap), orientation and
    BRIEF on the device with the GS_NO_STDLIB polynomials (ref :70-88) == the reference header built with
    -DGS_NO_STDLIB; the restatement switched to the polynomials agrees with that build too"""
    from oracle import pyoracle
    if not pyoracle.have_reference_nostdlib():
        pytest.skip("oracle/_ref/libgs_ref_nostdlib.so not present")
    ref_ns, port_ns = Oracle("reference_nostdlib"), Oracle("port_nostdlib")
    frames = np.stack([Oracle.synth(128, 96, 70 + i) for i in range(3)])
    frames[2] = np.random.RandomState(2).randint(0, 256, (96, 128)).astype(np.uint8)
    for nkps in (60, 7, 2000):  # cap = min(4 nkps, 5000): 240 / 28 / 5000 candidates
        pc.orb_nostdlib(emu, ref_ns, frames, nkps=nkps)
    for f in range(3):
        assert_same(port_ns.orb_extract(frames[f], 60, 20), ref_ns.orb_extract(frames[f], 60, 20), "restatement, polynomial trig")
    flat = np.full((1, 40, 40), 9, np.uint8)  # no candidates at all; and a frame smaller than 7 px
    pc.orb_nostdlib(emu, ref_ns, flat, nkps=10)
    for y in (-3.5, -1.0, 0.0, 2.0):  # the polynomials themselves, including the x == 0 branch
        for x in (-2.0, 0.0, 1.0, 7.25):
            assert np.float32(port_ns.lib.orc_atan2_poly(C.c_float(y), C.c_float(x))).tobytes() == \
                np.float32(ref_ns.atan2(y, x)).tobytes()


def test_fast_with_a_score_map_of_another_size(emu, reference):
    """the reference writes the score map through gs_set and reads it through gs_get (ref :512, :518-524): a map
    smaller or larger than the image is legal, positions outside it read 0 and are never written"""
    kl.fast_score_map_of_another_size(emu, reference, (MEM,))


def test_histogram_ragged_frames_every_alignment(emu, oracle):
    """k_hist_partial counts whole 16-byte chunks from a queue of loads in flight and the bytes before the
    first / after the last whole chunk one by one: frames of 1 .. 70 bytes and 4 KB +- a few at every base
    alignment (frame f of a batch starts at f * w * h bytes)"""
    kl.histogram_every_alignment(emu, oracle, MEM)


def test_histogram_of_an_image_larger_than_one_launch_frame(emu, oracle):
    """images above 1 GB are counted in pieces (k_hist_partial addresses a frame with 32-bit offsets); gsh_tune key 12
    lowers the piece size so that 1000 .. 70000-byte images take that path: whole pieces + a remainder, odd piece sizes
    (every piece starts at another alignment), batches"""
    kl.histogram_in_pieces(emu, oracle, MEM)


@pytest.mark.parametrize("mode", [1, 2])
def test_lbp_chunk_to_xcd_mapping_never_changes_results(emu, oracle, cascade, mode):
    """gsh_tune key 13: 1 = chunks in dispatch order, 2 = XCD-aware mapping (chunk = (block % 8) * ceil(nchunks / 8) + block / 8,
    grid padded to a multiple of 8) -- forced on small images: scales with 1, 7, 9 and a few dozen chunks, caps reached early"""
    edges = oracle.sobel(oracle.blur(Oracle.synth(200, 150, 1000), 2))
    try:
        emu.tune(13, mode)
        pc.lbp(emu, oracle, edges, MEM, cascade, params=((4096, 1.1, 1.0, 4.0, 1), (7, 1.1, 1.0, 4.0, 1), (300, 1.3, 1.0, 3.0, 2)))
        pc.lbp(emu, oracle, Oracle.synth(96, 80, 7), MEM, cascade, params=((4096, 1.1, 1.0, 4.0, 1),))
        pc.lbp(emu, oracle, Oracle.synth(64, 48, 9), MEM, random_cascade(1), params=((4096, 1.25, 1.0, 2.0, 2), (3, 1.25, 1.0, 2.0, 1)))
    finally:
        emu.tune(13, 0)


def test_box_radii_around_the_quotient_switch_and_up_to_127(emu, oracle):
    """k_box16: the quotient of unclipped rows is one multiply up to r = 31 and the float estimate + fix-up beyond; the
    sliding route serves radii up to 127 (u16 column sums, 128-entry LDS halo).  gs_blur and gs_adaptive_threshold on
    images with a bright half (large sums)"""
    for r in kl.ANY_RADII:
        kl.box_any_radius(emu, oracle, (MEM,), r)


@pytest.mark.parametrize("shape", [(32, 17), (48, 40), (272, 33), (96, 17), (1040, 19), (64, 70),
                                   (33, 17), (47, 40), (270, 33), (63, 35), (1038, 19), (65, 70), (81, 33)])
def test_box_register_ring_kernel_every_radius(emu, oracle, shape):
    """k_box16r<MODE, r> for r = 1 .. 16 (the window's raw rows in a register ring, constant tap counts, multiply-high
    quotient from a table for clipped rows too) against the oracle and against k_box16 (gsh_tune key 6 = 4): widths of 2
    threads up to 65, heights down to 2 r + 1, bright images (largest sums), bands of 1 .. h rows, and compare constants
    on both sides of every clamp of the product form.  Ragged widths (w % 16 = 1, 15, 14, ...; round 5): the ring kernel
    over the whole strips with the last one a feeder + k_box_edge (one wave per band) for the last 16 + w % 16 columns."""
    for r in kl.ring_radii(shape):  # shorter frames take k_box16 (covered by the any-radius tests)
        kl.box_ring(emu, oracle, (MEM,), shape, r)


def test_box_kernel_any_band_height_and_full_width(emu, oracle):
    """k_box16 with bands of 1 .. 200 rows (gsh_tune key 0; the launcher itself picks 8 .. h) on a batch, and on rows as
    wide as the kernel goes (4096 = 256 threads x 16 px) with radii on both sides of every switch"""
    kl.box_band_heights(emu, oracle, MEM)
    for shape in kl.FULL_WIDTH_SHAPES:
        kl.box_full_width(emu, oracle, (MEM,), shape)
