"""gs_trace_contour (ref grayskull.h:446-480) on the kernel-logic emulator: the reference's own test vector, hand
cases against a plain-Python restatement, ending walks against the compiled reference (oracle/_ref/libgs_ref.so),
endless walks -- on which the reference does not return -- against the restatement's limit values, the batch, the
blob-record glue and a strict C99 caller.  tests/test_gpu_contours.py runs the same checks on an MI355X."""
import os
import subprocess
import sys

import numpy as np
import pytest

import blob_cases as bc
import contour_cases as cc
from grayskull_amd import BLOB_DTYPE, CONTOUR_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
W = 255
U32 = cc.U32


class HostArrays:
    """the emulator's "device" memory is host memory: numpy arrays go to the batch calls as they are"""

    @staticmethod
    def dev(a):
        return np.ascontiguousarray(a)

    @staticmethod
    def host(a):
        return a

    @staticmethod
    def sync():
        pass


def batch_trace(g, xp, imgs, starts, counts=None, status=True, visited=None, per_frame=None):
    """gsh_trace_contours_batch on frames `imgs` (n, h, w) with starts[f] = [(x, y)] -> per frame ([(length, box)],
    [status] or None), and the visited planes"""
    n = len(imgs)
    per_frame = per_frame or max(1, max(len(s) for s in starts))
    if counts is None and any(len(s) != per_frame for s in starts):
        counts = [len(s) for s in starts]  # counts == NULL traces all per_frame records of every frame
    recs = np.zeros((n, per_frame), CONTOUR_DTYPE)
    recs["x"], recs["length"] = 0xDEAD, 0xBEEF  # never read; overwritten for the traced ones
    for f, ss in enumerate(starts):
        for k, s in enumerate(ss):
            recs[f, k]["sx"], recs[f, k]["sy"] = int(s[0]) & U32, int(s[1]) & U32
    before = recs.copy()
    d_img = xp.dev(np.stack(imgs))
    d_vis = xp.dev(np.zeros(np.stack(imgs).shape, np.uint8) if visited is None else np.stack(visited))
    d_rec = xp.dev(recs.view(np.int32).reshape(n, per_frame, 7))
    d_cnt = None if counts is None else xp.dev(np.asarray(counts, np.int32))
    d_st = xp.dev(np.full((n, per_frame), 77, np.uint8)) if status else None
    g.trace_contours_batch(d_img, d_vis, d_rec, d_cnt, d_st)
    xp.sync()
    out = np.ascontiguousarray(xp.host(d_rec)).view(CONTOUR_DTYPE).reshape(n, per_frame)
    st = xp.host(d_st) if status else None
    res = []
    for f in range(n):
        m = min(len(starts[f]) if counts is None else int(counts[f]), per_frame)
        # records beyond the traced ones, and every start, are left as they were
        assert out[f, m:].tobytes() == before[f, m:].tobytes()
        assert np.array_equal(out[f]["sx"], before[f]["sx"]) and np.array_equal(out[f]["sy"], before[f]["sy"])
        if status:
            assert (st[f, m:] == 77).all()
        res.append(([cc.rec_tuple(r) for r in out[f, :m]], None if st is None else [int(v) for v in st[f, :m]]))
    return res, xp.host(d_vis)


def check_one(g, img, start, visited=None, what=""):
    """one drop-in call against the restatement -> (length, box, status, moves) of the restatement"""
    img = np.ascontiguousarray(img)
    vis0 = np.zeros(img.shape, np.uint8) if visited is None else visited
    length, box, vis, status, moves = cc.spec_trace(img, vis0, start)
    got_vis = vis0.copy()
    got = cc.rec_tuple(g.trace_contour(img, got_vis, start))
    assert got == (length, box), "%s start %s: %s, expected %s" % (what, start, got, (length, box))
    assert np.array_equal(got_vis, vis), "%s start %s: visited" % (what, start)
    return length, box, status, moves


def check_hand_cases(g, xp):
    """every hand-derived case on the library `g` (emulator or GPU)"""
    # 1. the reference's own vector (ref test.c:261-287): recorded results
    vis = np.zeros((5, 5), np.uint8)
    r = g.trace_contour(cc.TEST_C_IMAGE, vis, cc.TEST_C_START)
    assert cc.rec_tuple(r) == (cc.TEST_C_LENGTH, cc.TEST_C_BOX) == (10, (1, 0, 4, 5))
    assert (int(r["sx"]), int(r["sy"])) == cc.TEST_C_START
    assert np.array_equal(vis, cc.TEST_C_VISITED)
    assert cc.spec_trace(cc.TEST_C_IMAGE, np.zeros((5, 5), np.uint8), cc.TEST_C_START)[:2] == (10, (1, 0, 4, 5))

    # isolated pixel: no neighbour, the start is still counted and marked
    img = np.zeros((9, 11), np.uint8)
    img[4, 6] = W
    assert check_one(g, img, (6, 4))[:3] == (1, (6, 4, 1, 1), 0)
    # a start that is background, next to a blob: it is counted and marked, then the walk runs on the blob
    img = np.zeros((12, 14), np.uint8)
    img[3:8, 4:9] = W
    length, box, status, _ = check_one(g, img, (3, 5))
    # by hand: E to (4, 5), NE to the inner pixel (5, 4), NE to (6, 3) on the top edge, then clockwise round the outline
    # for ever: the start, one inner pixel, the 16 pixels of the outline; box from x = 3 (the start) to 8, y = 3 to 7
    assert (length, box) == (1 + 1 + 16, (3, 3, 6, 5))
    assert status == cc.ENDLESS  # it never comes back to a start that is not foreground
    # start already visited: the length excludes it
    vis = np.zeros(img.shape, np.uint8)
    vis[3, 4] = 255
    vis[3, 5] = 1  # any non-zero byte counts as visited, and becomes 255
    assert check_one(g, img, (4, 3), visited=vis)[0] == 16 - 2
    # starts outside the image: (w, y), (x, h), (0xFFFFFFFF, 0) -- the last one has column 0 as its eastern neighbour
    img = np.zeros((6, 7), np.uint8)
    img[0:3, 0:2] = W
    img[2:5, 6] = W
    img[5, 2:5] = W
    for s in ((7, 3), (3, 6), (U32, 0), (U32, 1), (U32, U32), (7, 6), (2 ** 31, 2), (2 ** 31 - 1, 2), (0, 2 ** 31)):
        check_one(g, img, s, what="outside")
    assert check_one(g, img, (U32, 0))[0] > 1 and check_one(g, img, (7, 3))[0] > 1
    # box.x drops after box.w was set: box.w stays below the width of the bounding box
    img = np.zeros((8, 12), np.uint8)
    img[1, 5:10] = W
    img[2, 4] = W
    img[3, 3] = W
    img[4, 1:3] = W
    length, box, status, _ = check_one(g, img, (5, 1))
    ys, xs = np.nonzero(cc.spec_trace(img, np.zeros(img.shape, np.uint8), (5, 1))[2])
    assert box[0] == xs.min() and box[2] < xs.max() - xs.min() + 1, "the case must have box.w < bounding width"
    # a pixel of value exactly 128 is background here (it is foreground for gs_blobs)
    img = np.zeros((5, 9), np.uint8)
    img[2, 2:5] = W
    img[2, 5] = 128
    img[2, 6] = 129
    assert check_one(g, img, (2, 2))[:2] == (3, (2, 2, 3, 1))
    assert check_one(g, img, (6, 2))[:2] == (1, (6, 2, 1, 1))
    # the smallest endless example: the limit values
    length, box, status, _ = check_one(g, cc.ENDLESS_EXAMPLE, (0, 0))
    assert status == cc.ENDLESS and (length, box) == (7, (0, 0, 2, 5))
    (res, vis) = batch_trace(g, xp, [cc.ENDLESS_EXAMPLE], [[(0, 0)]])
    assert res[0] == ([(7, (0, 0, 2, 5))], [1])
    # 1 x N and N x 1 images, widths round the tile size
    rng = np.random.default_rng(3)
    for shape in ((1, 1), (1, 200), (150, 1), (1, 64), (64, 1), (1, 33), (2, 130), (130, 2)):
        img = cc.random_mask(rng, shape[0], shape[1], 0.7)
        ss = cc.start_pixels(img) + [(0, 0), (shape[1] - 1, shape[0] - 1)]
        want, want_vis, _ = cc.expected_sequence(img, ss)
        got, got_vis = cc.lib_sequence_dropin(g, img, ss)
        cc.assert_sequence_equal(got, got_vis, want, want_vis, "shape %s" % (shape,))
    # a contour that crosses tile borders diagonally (tiles are 64 x 64, re-centred on the walker) ...
    img = np.zeros((300, 310), np.uint8)
    for i in range(290):
        img[5 + i, 3 + i:3 + i + 3] = W
    length, box, status, moves = check_one(g, img, (3, 5), what="diagonal")
    assert status == 0 and moves > 500
    # ... and one that runs along a tile border for more than 200 px: the tile loaded for start (40, 40) ends at row
    # 71, where the band's lower edge lies
    img = np.zeros((120, 400), np.uint8)
    img[40:72, 40:380] = W
    length, box, status, moves = check_one(g, img, (40, 40), what="along")
    assert status == 0 and (length, box) == (2 * (340 + 32) - 4, (40, 40, 340, 32))
    img[72, 40:380] = W
    assert check_one(g, img, (40, 40), what="along + 1")[2] == 0
    # two contours of one frame that share pixels, in both orders: the later one's length skips the shared pixels
    img = np.zeros((40, 60), np.uint8)
    img[5:20, 5:30] = W
    img[10:15, 30:50] = W
    a, b = (5, 5), (30, 10)  # b: another pixel of the same outline
    for order in ((a, b), (b, a)):
        want, want_vis, _ = cc.expected_sequence(img, order)
        got, got_vis = cc.lib_sequence_dropin(g, img, order)
        cc.assert_sequence_equal(got, got_vis, want, want_vis, "shared %s" % (order,))
        (res, vis) = batch_trace(g, xp, [img], [list(order)])
        cc.assert_sequence_equal(res[0][0], vis[0], want, want_vis, "shared batch %s" % (order,), got_status=res[0][1])
    ab = cc.expected_sequence(img, (a, b))[0]
    ba = cc.expected_sequence(img, (b, a))[0]
    assert ab[0][0] != ba[1][0] and ab[1][0] != ba[0][0], "lengths must depend on the order"


def check_family_frames(g, xp, ref, frames, what, budget=300000, dropin_device=None):
    """the start pixels of every frame (all of one size), in raster order, on one visited plane per frame: the batch,
    the drop-in sequence on host pointers and, with `dropin_device` (GPU), on device pointers, against the compiled
    reference (endless walks: the restatement).  Every start pixel where the frame's walks fit `budget` moves, else a
    sample spread over the whole frame with a floor on its size (cc.sampled_starts); the sizes are printed.  At most a
    tenth of the cases may be endless.  -> (cases, endless)"""
    sampled = [cc.sampled_starts(img, budget) for img in frames]
    starts = [s for s, _ in sampled]
    for f, (ss, total) in enumerate(sampled):
        print("%s frame %d: %d of %d start pixels" % (what, f, len(ss), total))
        assert len(ss) >= min(12, total), (what, f)
    wants = [cc.expected_sequence(img, ss, ref=ref) for img, ss in zip(frames, starts)]
    res, vis = batch_trace(g, xp, frames, starts)
    for f, (img, ss) in enumerate(zip(frames, starts)):
        want, want_vis, _ = wants[f]
        cc.assert_sequence_equal(res[f][0], vis[f], want, want_vis, "%s frame %d batch" % (what, f), got_status=res[f][1])
        got, got_vis = cc.lib_sequence_dropin(g, img, ss)
        cc.assert_sequence_equal(got, got_vis, want, want_vis, "%s frame %d drop-in, host pointers" % (what, f))
        if dropin_device is not None:
            got, got_vis = dropin_device(g, img, ss)
            cc.assert_sequence_equal(got, got_vis, want, want_vis, "%s frame %d drop-in, device pointers" % (what, f))
    cases, endless = sum(len(s) for s in starts), sum(w_[2] for w_ in wants)
    assert cases > 0 and endless * 10 <= cases, "%s: %d of %d cases endless: too many left out of the reference comparison" % (
        what, endless, cases)
    return cases, endless


def family_frames(rng, h, w):
    return [cc.upscaled_noise(rng, h, w, 2), cc.upscaled_noise(rng, h, w, 3), cc.random_discs(rng, h, w, max(3, w // 25), 3, 20),
            cc.random_rects(rng, h, w, max(3, w // 25)), bc.spiral(h, w, gap=3)]


def check_endless(g, xp, frames, what, dropin_stride=1, budget=None):
    """every start pixel (`budget`: a sample, see cc.sampled_starts), on one visited plane per frame (batch: status, limit length,
    box, visited) and each alone on a fresh plane (drop-in), against the restatement; at least a quarter of the cases
    must be endless"""
    starts = [cc.start_pixels(img) if budget is None else cc.sampled_starts(img, budget)[0] for img in frames]
    res, vis = batch_trace(g, xp, frames, starts)
    cases = endless = 0
    for f, (img, ss) in enumerate(zip(frames, starts)):
        want, want_vis, e = cc.expected_sequence(img, ss)
        cc.assert_sequence_equal(res[f][0], vis[f], want, want_vis, "%s frame %d batch" % (what, f), got_status=res[f][1])
        cases, endless = cases + len(ss), endless + e
        for s in ss[::dropin_stride]:
            status = check_one(g, img, s, what=what)[2]
            cases, endless = cases + 1, endless + (status == cc.ENDLESS)
    assert endless * 4 >= cases, "%s: only %d of %d cases endless" % (what, endless, cases)
    return cases, endless


def chain_expected(ref, img, cap):
    """the reference's gs_blobs, a host search for each blob's raster-first labelled pixel, gs_trace_contour per blob
    in label order on one visited plane (endless ones by the restatement)"""
    recs, labels = bc.Ref().blobs(img, cap)
    starts = []
    for r in recs:
        y = int(r["y"])
        xs = np.nonzero(labels[y] == r["label"])[0]
        assert len(xs) and xs[0] >= r["x"]
        starts.append((int(xs[0]), y))
    want, want_vis, endless = cc.expected_sequence(img, starts, ref=ref)
    return recs, labels, starts, want, want_vis, endless


def check_starts_glue(g, xp, rng):
    """gsh_blob_contour_starts_batch against a host search, with labels / records from the restatement of gs_blobs"""
    frames = [cc.upscaled_noise(rng, 50, 150, 2), cc.random_discs(rng, 50, 150, 12, 2, 9), bc.random_mask(rng, 50, 150, 0.5)]
    nb = 40
    labs, blobs, counts, wants = [], np.zeros((len(frames), nb), BLOB_DTYPE), [], []
    for f, img in enumerate(frames):
        recs, labels = bc.spec_blobs(img, nb)
        m = len(recs) if f != 1 else min(len(recs), 5)  # frame 1: fewer than there are
        blobs[f, :len(recs)] = recs
        labs.append(labels)
        counts.append(m)
        wants.append([(int(np.nonzero(labels[int(r["y"])] == r["label"])[0][0]), int(r["y"])) for r in recs[:m]])
    out = np.zeros((len(frames), nb), CONTOUR_DTYPE)
    out["x"] = 0xABCD
    before = out.copy()
    d_out = xp.dev(out.view(np.int32).reshape(len(frames), nb, 7))
    g.blob_contour_starts_batch(xp.dev(np.stack(labs).view(np.int16)), xp.dev(blobs.view(np.int32).reshape(len(frames), nb, 8)),
                                xp.dev(np.asarray(counts, np.int32)), d_out)
    xp.sync()
    got = np.ascontiguousarray(xp.host(d_out)).view(CONTOUR_DTYPE).reshape(len(frames), nb)
    for f in range(len(frames)):
        m = counts[f]
        assert [(int(r["sx"]), int(r["sy"])) for r in got[f, :m]] == wants[f], f
        assert got[f, m:].tobytes() == before[f, m:].tobytes()
        for fld in ("x", "y", "w", "h", "length"):
            assert np.array_equal(got[f][fld], before[f][fld])


def check_split(g, xp):
    """gsh_tune key 8 (frames per launch) = 3 on a 7-frame batch changes nothing"""
    rng = np.random.default_rng(8)
    frames = [cc.upscaled_noise(rng, 70, 90, 2) if f % 2 else cc.random_mask(rng, 70, 90, 0.6) for f in range(7)]
    starts = [cc.start_pixels(img)[:30] for img in frames]
    counts = [len(s) - (f % 3) for f, s in enumerate(starts)]
    outs = []
    for fpl in (0, 3):
        g.tune(8, fpl)
        try:
            outs.append(batch_trace(g, xp, frames, starts, counts=counts))
        finally:
            g.tune(8, 0)
    assert outs[0][0] == outs[1][0] and np.array_equal(outs[0][1], outs[1][1])
    for f, img in enumerate(frames):
        want, want_vis, _ = cc.expected_sequence(img, starts[f][:counts[f]])
        cc.assert_sequence_equal(outs[1][0][f][0], outs[1][1][f], want, want_vis, "split frame %d" % f, got_status=outs[1][0][f][1])


def build_c_program(tmp_path, libdir, libname):
    exe = tmp_path / "contour_dropin"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INC,
                           os.path.join(ROOT, "tests", "c", "test_contour_dropin.c"), "-o", str(exe),
                           "-L", libdir, "-l:" + libname, "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib",
                           "-Wl,-rpath-link,/opt/rocm/lib"])
    return subprocess.check_output([str(exe)]).decode()


def _ref():
    from oracle import pyoracle
    if not pyoracle.have_reference():
        pytest.skip("oracle/_ref/libgs_ref.so not built")
    return cc.Ref()


# ---- the tests --------------------------------------------------------------------------------------------------------
def test_restatement_matches_reference_on_its_own_vector_and_decides_endlessness():
    ref = _ref()
    vis = np.zeros((5, 5), np.uint8)
    assert ref.trace(cc.TEST_C_IMAGE, vis, cc.TEST_C_START) == (10, (1, 0, 4, 5)) and np.array_equal(vis, cc.TEST_C_VISITED)
    with pytest.raises(AssertionError, match="does not return"):
        ref.trace(cc.ENDLESS_EXAMPLE, np.zeros((5, 2), np.uint8), (0, 0))
    # the cycle of the example: (1,3) -> (1,4) -> (0,4), entered after 5 moves
    assert cc.spec_trace(cc.ENDLESS_EXAMPLE, np.zeros((5, 2), np.uint8), (0, 0))[3:] == (cc.ENDLESS, 8)


def test_hand_derived_cases_emulated(emu):
    check_hand_cases(emu, HostArrays)


@pytest.mark.parametrize("w", [63, 65, 200, 1000, 4097])
def test_ending_walks_match_reference_emulated(emu, w):
    ref = _ref()
    rng = np.random.default_rng(w)
    check_family_frames(emu, HostArrays, ref, family_frames(rng, 70 + w % 7, w), "w %d" % w)


def test_families_at_96x128_end_as_recorded():
    """the families of the reference comparison hardly ever produce an endless walk (0 of several hundred starts),
    thresholded blurred noise does: the first is what makes them usable, the second what keeps the rule honest"""
    rng = np.random.default_rng(1)
    for fam in family_frames(rng, 128, 96):
        starts = cc.start_pixels(fam)
        assert cc.expected_sequence(fam, starts)[2] * 10 <= len(starts)
    img = bc.blurred_noise(rng, 128, 96, passes=1)
    img = np.where(img > np.median(img), 255, 0).astype(np.uint8)
    starts = cc.start_pixels(img)
    assert cc.expected_sequence(img, starts)[2] * 4 >= len(starts)


def test_endless_walks_match_restatement_emulated(emu):
    rng = np.random.default_rng(6)
    frames = [cc.random_mask(rng, 128, 96, 0.6)]
    img = bc.blurred_noise(rng, 128, 96, passes=1)
    frames.append(np.where(img > np.median(img), 255, 0).astype(np.uint8))
    check_endless(emu, HostArrays, frames, "96 x 128")


def test_counts_and_null_status_emulated(emu):
    rng = np.random.default_rng(12)
    frames = [cc.upscaled_noise(rng, 40, 80, 2) for _ in range(3)]
    starts = [cc.start_pixels(img)[:12] for img in frames]
    counts = [len(starts[0]), 0, 1000]  # one frame traces nothing, one count above per_frame is clamped
    res, vis = batch_trace(emu, HostArrays, frames, starts, counts=counts, status=False, per_frame=12)
    for f, img in enumerate(frames):
        m = min(counts[f], 12)
        want, want_vis, _ = cc.expected_sequence(img, starts[f][:m])
        cc.assert_sequence_equal(res[f][0][:len(want)], vis[f], want, want_vis, "frame %d" % f)
    assert not vis[1].any()


def test_blob_contour_starts_emulated(emu):
    check_starts_glue(emu, HostArrays, np.random.default_rng(21))


def test_chain_blobs_starts_trace_emulated(emu):
    """gs_blobs -> starts -> trace on the emulator, small frames, against the reference's functions"""
    ref = _ref()
    rng = np.random.default_rng(31)
    frames = [cc.upscaled_noise(rng, 60, 130, 3), cc.random_discs(rng, 60, 130, 10, 3, 12)]
    cap = 100
    n = len(frames)
    img = np.stack(frames)
    lab = np.zeros(img.shape, np.int16)
    blobs = np.zeros((n, cap, 8), np.int32)
    counts = np.zeros(n, np.int32)
    emu.blobs_batch(img, lab, blobs, counts, cap)
    cont = np.zeros((n, cap, 7), np.int32)
    emu.blob_contour_starts_batch(lab, blobs, counts, cont)
    vis = np.zeros(img.shape, np.uint8)
    st = np.zeros((n, cap), np.uint8)
    emu.trace_contours_batch(img, vis, cont, counts, st)
    got = cont.view(CONTOUR_DTYPE).reshape(n, cap)
    for f in range(n):
        recs, labels, starts, want, want_vis, _ = chain_expected(ref, frames[f], cap)
        assert int(counts[f]) == len(recs)
        assert [(int(r["sx"]), int(r["sy"])) for r in got[f, :len(recs)]] == starts
        cc.assert_sequence_equal([cc.rec_tuple(r) for r in got[f, :len(recs)]], vis[f], want, want_vis, "frame %d" % f,
                                 got_status=st[f])


def test_frames_per_launch_split_emulated(emu):
    check_split(emu, HostArrays)


def test_c99_contour_program_against_emulated_kernels(tmp_path, emu):
    assert "all passed" in build_c_program(tmp_path, os.path.join(ROOT, "tests", "emu"), "libgs_kernel_emu.so")


def test_contour_struct_in_python_abi():
    from grayskull_amd import _abi
    import ctypes as C
    assert C.sizeof(_abi.GsContour) == 28 == CONTOUR_DTYPE.itemsize
    assert [_abi.GsContour.box.offset, _abi.GsContour.start.offset, _abi.GsContour.length.offset] == [0, 16, 24]
    assert [CONTOUR_DTYPE.fields[f][1] for f in ("x", "sx", "length")] == [0, 16, 24]


def test_trace_contour_precondition_aborts_with_the_reference_text(emu, tmp_path):
    prog = tmp_path / "bad_contour.py"
    prog.write_text('''
import sys, numpy as np
sys.path.insert(0, %r)
import grayskull_amd as G
g = G.Grayskull(%r)
g.trace_contour(np.zeros((4, 4), np.uint8), np.zeros((5, 4), np.uint8), (0, 0))
''' % (ROOT, os.path.join(ROOT, "tests", "emu", "libgs_kernel_emu.so")))
    r = subprocess.run([sys.executable, str(prog)], capture_output=True)
    assert r.returncode == -6, r
    assert b"Assertion failed: gs_valid(img) && gs_valid(visited) && img.w == visited.w && img.h == visited.h" in r.stderr
