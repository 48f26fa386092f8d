"""The guard net: every caller-owned output buffer of the public surface inside guards (tests/test_guards.py on the
emulator, tests/test_gpu_guards.py on the MI355X).

Each case puts every output of one entry point into a buffer made by `Guarded.make`: the view the library gets lies
between two guards of a fixed byte pattern (at least 4096 bytes and two rows / records each) and starts as seeded random
bytes.  After the call `Guarded.check` asserts
  (a) the part the call owns equals the oracle bit for bit,
  (b) both guards are intact (the first damaged offset is named),
  (c) every byte of the view the call does not own still holds its prefill.
(a) and (c) are one comparison with `expected`: the prefill with the oracle's result laid over the owned part.

Two paths per case.  "dev": device pointers -- torch CUDA memory on the GPU; on the emulator numpy memory, with the
emulator's switch emu_device_pointers(1) (gs_internal.h, emulator builds only) for the drop-in gs_* calls, so that their kernels run
straight on the guarded buffer.  "host": host pointers (guarded numpy arrays) through the drop-in gs_* calls: the staged
path, whose copy-back size is computed on the host.

Who owns what (asserted by the cases; see docs/design/oracle_and_parity.md):
  images (resize, crop, template result, perspective, synth, pipeline dst / tmp)   every byte of the image
  score maps (gsh_fast_score_batch, gsh_fast_batch, gs_fast, ORB)                 the interior; the 3-px frame is kept
  record lists (FAST, ORB, LBP, match, blobs)        whole records below counts[f]; records at and beyond it are kept
  counts / count / thr / hist / sums / index / largest / corners                  every element
  gs_blob records                                    all 32 bytes of a record, the 2 padding bytes behind `label` as 0
  contours (gsh_trace_contours_batch)                box and length of records below counts[f]; start and the rest kept
  contours (gsh_blob_contour_starts_batch)           start of records below counts[f]; everything else kept
  status                                             entries below counts[f]
  visited, in-place threshold                        the bytes the reference changes

Guard check per public function that writes caller memory (include/grayskull.h, include/grayskull_hip.h):
  gs_blur gs_sobel gs_erode gs_dilate gs_adaptive_threshold gs_filter gs_downsample     dropin_strip
  gs_histogram gs_threshold gs_integral gs_brief_descriptor(_nostdlib)                  dropin_strip
  gs_crop gs_copy gs_resize gs_resize_nn                                                geometry
  gs_match_template                                                                     template_*
  gs_fast                                                                               fast (drop-in paths)
  gs_orb_extract gs_orb_extract_nostdlib                                                orb (drop-in paths)
  gs_match_orb                                                                          match (drop-in paths)
  gs_lbp_detect                                                                         lbp (drop-in paths)
  gs_blobs gs_blob_corners gs_perspective_correct                                       blobs / perspective (drop-in paths)
  gs_trace_contour                                                                      contours (drop-in paths)
  gsh_blur_batch gsh_sobel_batch gsh_erode_batch gsh_dilate_batch gsh_filter_batch      tests/test_ragged.py
  gsh_adaptive_threshold_batch gsh_blur_sobel_batch gsh_integral_batch                  tests/test_ragged.py
  gsh_downsample_batch                                                                  tests/test_ragged.py
  gsh_morph_batch                                                                       tests/morph_cases.py
  gsh_blob_paint_batch                                                                  tests/blob_paint_cases.py
  gsh_histogram_batch gsh_otsu_batch gsh_edge_pipeline_batch                            pointwise
  gsh_threshold_batch gsh_threshold_batch_dev gsh_threshold_batch_dev_offset            threshold
  gsh_checksum_batch gsh_synth_batch                                                    synth_checksum
  gsh_fast_score_batch gsh_fast_batch                                                   fast
  gsh_orb_extract gsh_orb_extract_batch gsh_orb_extract_batch_nostdlib                  orb
  gsh_orb_extract_pyramid                                                               orb_pyramid
  gsh_match_orb_dev                                                                     match
  gsh_lbp_detect_batch                                                                  lbp
  gsh_blobs_batch gsh_blob_corners_batch gsh_blob_largest_batch                         blobs
  gsh_perspective_correct_batch                                                         perspective
  gsh_trace_contours_batch gsh_blob_contour_starts_batch                                contours
(gsh_upload / gsh_download / gsh_memset, gsh_profile_read, gsh_lbp_count_evaluated and the gsh_comm_* collectives move
bytes whose count the caller names; they have no kernel-side bounds of their own and stay with their own tests.)

Every case returns nothing and counts its guard checks in `Backend.checked`; the test files assert that count against
the one the parametrisation implies (`expect`), so that a branch that silently runs nothing cannot pass."""
import contextlib
import ctypes as C

import numpy as np

import blob_cases as bc
import contour_cases as cc
import parity_cases as pc
from grayskull_amd import _ptr, BLOB_DTYPE, CONTOUR_DTYPE, KEYPOINT_DTYPE, MATCH_DTYPE, POINT_DTYPE, RECT_DTYPE
from grayskull_amd._abi import GsImage
from oracle.pyoracle import Oracle
from util import random_cascade

GUARD_MIN = 4096
RECORD_OFFS = (0, 4)   # record lists 16-byte aligned (the kernels' 16-byte store paths, what hipMalloc gives) and not
ALIGN = 64


def _pattern(a, b):
    """the guards' bytes at store indices [a, b): fixed, and no constant"""
    i = np.arange(a, b, dtype=np.int64)
    return ((i * 151 + 89) & 0xFF).astype(np.uint8)


class Buf:
    """one guarded allocation: `store` (all bytes), the view at [lo, lo + nbytes), its prefill"""

    def __init__(self, store, lo, shape, dtype, pre):
        self.store, self.lo, self.shape, self.dtype, self.pre = store, lo, tuple(shape), np.dtype(dtype), pre
        self.nbytes = pre.size

    def expected(self):
        """a copy of the prefill in the view's type and shape: lay the oracle's result over the part the call owns"""
        return self.pre.copy().view(self.dtype).reshape(self.shape)


class Guarded:
    """guarded buffers of one kind of memory: "host" numpy arrays, "device" torch CUDA tensors"""

    def __init__(self, kind, seed=1):
        assert kind in ("host", "device")
        self.kind, self.rs, self.checked = kind, np.random.RandomState(seed), 0
        self.keep = []  # every buffer lives as long as this object: cases pass raw addresses of temporaries to the C ABI
        if kind == "device":
            import torch
            self.torch = torch

    def make(self, shape, dtype=np.uint8, off=0, prefill=None, stride=None):
        """-> (buf, view): view has `shape` / `dtype` and starts GUARD + off bytes into buf's bytes (off: a multiple of
        the C type's alignment; the base is 64-byte aligned).  prefill: the view's initial contents (default: seeded random
        bytes).  stride: bytes of one row / record of this output (default: the last axis); each guard holds two."""
        dtype = np.dtype(dtype)
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        align = dtype.alignment if dtype.names is None else 4
        assert off % align == 0, "offset %d breaks the alignment of %s" % (off, dtype)
        nbytes = int(np.prod(shape)) * dtype.itemsize
        if stride is None:
            stride = shape[-1] * dtype.itemsize
        guard = -(-max(GUARD_MIN, 2 * stride) // ALIGN) * ALIGN
        lo, total = guard + off, guard + off + nbytes + guard
        if prefill is None:
            pre = self.rs.randint(0, 256, nbytes).astype(np.uint8)
        else:
            pre = np.ascontiguousarray(prefill).view(np.uint8).reshape(-1).copy()
            assert pre.size == nbytes
        init = np.concatenate([_pattern(0, lo), pre, _pattern(lo + nbytes, total)])
        if self.kind == "host":
            raw = np.empty(total + ALIGN, np.uint8)
            a0 = (-raw.ctypes.data) % ALIGN
            store = raw[a0:a0 + total]
            store[:] = init
            view = store[lo:lo + nbytes].view(dtype).reshape(shape)
            assert view.ctypes.data % ALIGN == off % ALIGN
        else:
            t = self.torch
            store = t.from_numpy(init).cuda()
            v = store[lo:lo + nbytes]
            if dtype.names is not None:
                view = v.view(t.int32).view(shape + (dtype.itemsize // 4,))
            else:
                td = {1: t.uint8, 2: t.int16, 4: t.int32, 8: t.int64}[dtype.itemsize]
                view = v.view(td).view(shape) if dtype.itemsize > 1 else v.view(shape)
            assert view.data_ptr() % ALIGN == off % ALIGN
        self.keep.append(store)
        return Buf(store, lo, shape, dtype, pre), view

    def put(self, a, off=0):
        """an input: `a`'s bytes at the same kind of address (its guards are not checked)"""
        a = np.ascontiguousarray(a)
        return self.make(a.shape, a.dtype, off, prefill=a)[1]

    def check(self, buf, exp=None, what="", owned=None):
        """(b) both guards intact, then (a) + (c): the view equals `exp` (None: the prefill, i.e. nothing was written)
        byte for byte.  owned: optional bool array, one per byte of the view, True where the call owns the byte; without
        it a byte counts as not owned where `exp` equals the prefill (which one owned byte in 256 does by chance: the
        message says so).  -> the view's contents as a numpy array"""
        self.checked += 1
        a = buf.store.cpu().numpy() if self.kind == "device" else np.array(buf.store)
        lo, hi = buf.lo, buf.lo + buf.nbytes
        bad = np.flatnonzero(a[:lo] != _pattern(0, lo))
        assert bad.size == 0, "%s: front guard damaged: %d bytes, the first %d bytes before the output (now 0x%02x)" % (
            what, bad.size, lo - int(bad[-1]), int(a[bad[-1]]))
        bad = np.flatnonzero(a[hi:] != _pattern(hi, a.size))
        assert bad.size == 0, "%s: rear guard damaged: %d bytes, the first %d bytes past the output's end (now 0x%02x)" % (
            what, bad.size, int(bad[0]), int(a[hi + bad[0]]))
        got = a[lo:hi]
        want = buf.pre if exp is None else np.ascontiguousarray(exp).view(np.uint8).reshape(-1)
        assert want.size == got.size, "%s: expected %d bytes, the view has %d" % (what, want.size, got.size)
        bad = np.flatnonzero(got != want)
        if bad.size:
            i = int(bad[0])
            keep = (want == buf.pre) if owned is None else ~np.ascontiguousarray(owned).reshape(-1)
            unowned = np.flatnonzero((got != want) & keep)
            if unowned.size:
                j = int(unowned[0])
                raise AssertionError("%s: %d bytes that had to keep their prefill%s were changed, the first at byte %d of the output "
                                     "(element %d): prefill 0x%02x, now 0x%02x; %d bytes differ in all"
                                     % (what, unowned.size, " (bytes the call does not own, or owned bytes whose expected value equals "
                                        "the random prefill)" if owned is None else " (the call does not own them)", j,
                                        j // buf.dtype.itemsize, int(buf.pre[j]), int(got[j]), bad.size))
            raise AssertionError("%s: %d bytes differ from the oracle, the first at byte %d (element %d): got 0x%02x, expected 0x%02x"
                                 % (what, bad.size, i, i // buf.dtype.itemsize, int(got[i]), int(want[i])))
        return got.copy().view(buf.dtype).reshape(buf.shape)


class Backend:
    """a library, the oracle, guarded device memory (numpy for the emulator) and guarded host memory"""

    def __init__(self, g, o, gpu):
        self.g, self.o, self.gpu = g, o, gpu
        self.dev = Guarded("device" if gpu else "host", seed=2)
        self.host = Guarded("host", seed=3)
        self.ns = None
        self.roff = 4  # byte offset of every record list of a case (RECORD_OFFS); set by the test

    @property
    def checked(self):
        return self.dev.checked + self.host.checked

    def mem(self, path):
        return self.dev if path == "dev" else self.host

    def sync(self):
        self.g.sync()
        if self.gpu:
            self.dev.torch.cuda.synchronize()

    @contextlib.contextmanager
    def dropin(self, path):
        """drop-in gs_* calls on `path` pointers: the emulator is told to take them for device pointers"""
        if self.gpu or path == "host":
            yield
            return
        self.g.c.emu_device_pointers(1)
        try:
            yield
        finally:
            self.g.c.emu_device_pointers(0)

    def nostdlib(self):
        """the oracle with the GS_NO_STDLIB trig (compiled reference where built)"""
        if self.ns is None:
            from oracle import pyoracle
            self.ns = Oracle("reference_nostdlib") if (pyoracle.have_reference_nostdlib() and not self.o.port) else Oracle("port_nostdlib")
        return self.ns


def _img(a):
    return GsImage(int(a.shape[1]), int(a.shape[0]), _ptr(a))


def _noise(shape, seed):
    return np.random.RandomState(seed).randint(0, 256, shape).astype(np.uint8)


# ======================================================================================================================
# strip-class drop-ins (their batch forms are guarded by tests/test_ragged.py)
# ======================================================================================================================
K3 = np.array([[1, -2, 1], [2, 4, -2], [1, 2, 1]], np.int8)
DROPIN_STRIP_SHAPES = ((37, 9, 1), (64, 23, 3), (131, 6, 0))
DROPIN_STRIP_CHECKS = len(DROPIN_STRIP_SHAPES) * 13


def dropin_strip(b, path):
    """gs_blur (k_strip, r = 2; sliding box, r = 5), gs_sobel (the 1-px frame keeps the prefill), gs_erode, gs_dilate,
    gs_adaptive_threshold, gs_filter, gs_downsample, gs_histogram, gs_threshold (in place), gs_integral and
    gs_brief_descriptor(_nostdlib) (only the 32 descriptor bytes of the record are written) through the drop-in calls"""
    g, o, m = b.g, b.o, b.mem(path)
    with b.dropin(path):
        for w, h, off in DROPIN_STRIP_SHAPES:
            img = _noise((h, w), w * h)
            s = m.put(img, off)
            what = "%dx%d at +%d (%s)" % (w, h, off, path)
            for name, run, ref in (("gs_blur r=2", lambda d: g.blur(d, s, 2), lambda e: o.blur(img, 2)),
                                   ("gs_blur r=5", lambda d: g.blur(d, s, 5), lambda e: o.blur(img, 5)),
                                   ("gs_sobel", lambda d: g.sobel(d, s), lambda e: o.sobel(img, e)),
                                   ("gs_erode", lambda d: g.erode(d, s), lambda e: o.erode(img)),
                                   ("gs_dilate", lambda d: g.dilate(d, s), lambda e: o.dilate(img)),
                                   ("gs_adaptive_threshold", lambda d: g.adaptive_threshold(d, s, 4, 3), lambda e: o.adaptive_threshold(img, 4, 3)),
                                   ("gs_filter", lambda d: g.filter(d, s, K3, 8), lambda e: o.filter(img, K3, 8))):
                db, d = m.make((h, w), np.uint8, off)
                run(d)
                b.sync()
                m.check(db, ref(db.expected()), name + " " + what)
            db, d = m.make((h // 2, w // 2), np.uint8, off)
            g.downsample(d, s)
            b.sync()
            m.check(db, o.downsample(img), "gs_downsample " + what)
            hb, hv = m.make(256, np.uint32, 4 * (off % 2))
            g.c.gs_histogram(_img(s), _ptr(hv))
            b.sync()
            m.check(hb, o.histogram(img), "gs_histogram " + what)
            tb, tv = m.make((h, w), np.uint8, off, prefill=img)
            g.threshold(tv, 100)
            b.sync()
            m.check(tb, o.threshold(img, 100), "gs_threshold " + what)
            ib, iv = m.make((h, w), np.uint32, 4 * (off % 2), stride=4 * w)
            g.c.gs_integral(_img(s), _ptr(iv))
            b.sync()
            m.check(ib, o.integral(img), "gs_integral " + what)
            # the middle one of three keypoint records: x, y, angle are read, its descriptor is written, response stays
            for name, orc in (("gs_brief_descriptor", o), ("gs_brief_descriptor_nostdlib", b.nostdlib())):
                exp = m.rs.randint(0, 256, 3 * 48).astype(np.uint8).view(KEYPOINT_DTYPE)
                exp[1]["x"], exp[1]["y"], exp[1]["angle"] = w // 2, h // 2, 0.7
                kb, kv = m.make(3, KEYPOINT_DTYPE, 4 * (off % 2), prefill=exp)
                getattr(g.c, name)(_img(s), _ptr(kv[1:2]))
                b.sync()
                exp[1]["desc"] = orc.brief(img, w // 2, h // 2, 0.7)
                m.check(kb, exp, name + " " + what)


# ======================================================================================================================
# geometry
# ======================================================================================================================
GEOM_SRC = ((67, 45), (5, 3))
GEOM_DST = ((13, 7), (64, 5), (65, 6), (129, 2), (63, 4), (1, 1))   # dh % 4 = 3, 1, 2, 2, 0; dw % 64 = 13, 0, 1, 1, 63
GEOM_CROPS = ((60, 40, 7, 5), (3, 44, 64, 1), (0, 0, 67, 45), (66, 0, 1, 45), (2, 38, 65, 6), (0xFFFFFFFF, 3, 2, 41))
GEOM_CHECKS = len(GEOM_SRC) * len(GEOM_DST) * 2 + len(GEOM_CROPS) + 2


def geometry(b, path):
    """gs_resize (k_resize) and gs_resize_nn (k_resize_nn): blocks are 64 x 4, so destination heights dh % 4 in
    {0, 1, 2, 3} and widths dw % 64 in {0, 1, 13, 63} leave idle rows and columns in the last blocks; gs_crop (k_crop) with
    rectangles that reach the source's right and bottom edge, and one that sticks out of it on the left by way of the
    reference's own wrapping test (roi.x = 2^32 - 1, roi.w = 2: ref :155 accepts it, column 0 reads 0); gs_copy.
    A rectangle that fails the reference's assertion aborts in the library as in the reference and is not run.
    Every byte of the destination is the call's."""
    g, o, m = b.g, b.o, b.mem(path)
    with b.dropin(path):
        k = 0
        for sw, sh in GEOM_SRC:
            img = _noise((sh, sw), sw)
            s = m.put(img, k % 3)
            for dw, dh in GEOM_DST:
                for nn in (False, True):
                    off = (k, k + 1)[nn] % 4
                    db, d = m.make((dh, dw), np.uint8, off)
                    g.resize(d, s, nn)
                    b.sync()
                    m.check(db, o.resize(img, dw, dh, nn), "gs_resize%s %dx%d -> %dx%d at +%d (%s)" % ("_nn" if nn else "", sw, sh, dw, dh, off, path))
                    k += 1
        img = _noise((45, 67), 5)
        s = m.put(img, 1)
        for i, (rx, ry, rw, rh) in enumerate(GEOM_CROPS):
            db, d = m.make((rh, rw), np.uint8, i % 4)
            g.crop(d, s, rx, ry, rw, rh)
            b.sync()
            m.check(db, o.crop(img, rx, ry, rw, rh), "gs_crop %s (%s)" % ((rx, ry, rw, rh), path))
        for (w, h) in ((67, 45), (5, 3)):
            img = _noise((h, w), 6)
            db, d = m.make((h, w), np.uint8, 3)
            g.copy(d, m.put(img, 2))
            b.sync()
            m.check(db, img, "gs_copy %dx%d (%s)" % (w, h, path))


# ======================================================================================================================
# template matching
# ======================================================================================================================
# (iw, ih, tw, th, image offset, key 20)
TEMPLATE_DOT4 = tuple((iw, 9, tw, 3, 0, 0) for iw in (28, 32, 36, 264) for tw in (4, 5, 6, 7, 8)) + ((12, 7, 12, 7, 0, 0),)
TEMPLATE_BYTE = ((29, 9, 4, 3, 0, 0), (30, 8, 5, 3, 0, 0), (28, 9, 4, 3, 1, 0), (7, 5, 7, 5, 1, 0))
TEMPLATE_PX = ((16420, 3, 16400, 2, 0, 0),)
# >= 512 taps and >= 16 wide: 16 x 32; results rw in {63, 64, 65, 127, 129}, rh in {31, 33, 65} around the 32 x 64 / 64 x 128 tiles
TEMPLATE_MFMA = ((78, 62, 16, 32, 0, 3), (79, 64, 16, 32, 0, 3), (80, 62, 16, 32, 0, 0), (142, 64, 16, 32, 0, 2), (144, 96, 16, 32, 0, 2),
                 (144, 64, 16, 32, 0, 8), (80, 96, 16, 36, 0, 8), (32, 16, 32, 16, 0, 0))
TEMPLATE_OFFS = (0, 1, 2, 3)


def template(b, path, cases):
    """gs_match_template, one route per list of cases (the launcher's conditions, gs_stencil.cpp):
    TEMPLATE_DOT4  k_match_template4: image w % 4 == 0 on a 4-byte-aligned base; result widths rw % 4 in {0, 1, 2, 3} and
                   rw = 257 .. 261 (just above 256 = one block of 64 lanes x 4); tw % 4 in {0, 1, 2, 3} (rw % 4 == 3 needs tw % 4 == 2); the result at
                   offsets 0 .. 3, so that the last thread of a row ends on the dword store and on the byte loop
    TEMPLATE_BYTE  k_match_template: image w % 4 != 0, or the image base at offset 1
    TEMPLATE_PX    k_match_template_px: a template wider than kTmplTile - 3
    TEMPLATE_MFMA  k_match_template_mfma<4, 2> (key 20 = 3 or by rule), <1, 2> (key 20 = 2) and the banded form (key 20 =
                   8, th > 32 for a second band): results around the 32 x 64 and 64 x 128 tile edges
    each list ends with a 1 x 1 result, the template as large as the image.  Every byte of the result is the call's.
    The route per list holds on the dev path.  On the host path the image is staged into 16-byte-aligned scratch, so the
    offset-1 cases of TEMPLATE_BYTE with w % 4 == 0 run k_match_template4 there; the result is staged too, and what the
    host path checks is the copy-back."""
    g, o, m = b.g, b.o, b.mem(path)
    with b.dropin(path):
        try:
            for iw, ih, tw, th, ioff, key in cases:
                rs = np.random.RandomState(iw * 7 + tw)
                img, t = rs.randint(0, 256, (ih, iw)).astype(np.uint8), rs.randint(0, 256, (th, tw)).astype(np.uint8)
                if (iw, ih) == (tw, th):
                    t = img.copy()
                ro = o.match_template(img, t)
                s, ts = m.put(img, ioff), m.put(t, 0)
                g.tune(20, key)
                for off in TEMPLATE_OFFS if iw < 1000 and key == 0 else (1,):
                    rb, r = m.make(ro.shape, np.uint8, off)
                    g.match_template(s, ts, r)
                    b.sync()
                    m.check(rb, ro, "gs_match_template %dx%d on %dx%d, image at +%d, result at +%d, key 20 = %d (%s)" % (tw, th, iw, ih, ioff, off, key, path))
        finally:
            g.tune(20, 0)


def template_checks(cases):
    return sum(len(TEMPLATE_OFFS) if iw < 1000 and key == 0 else 1 for iw, ih, tw, th, ioff, key in cases)


# ======================================================================================================================
# histogram / Otsu / pipeline / threshold / checksum / synth
# ======================================================================================================================
POINTWISE_N = (1, 3, 5)
POINTWISE_SHAPES = ((33, 3), (64, 23))


def pipeline_routes(n, w, h):
    return ("ragged", "tmp") + ((("fused",) + (("fused, chunks of 2",) if n == 5 else ())) if w % 16 == 0 else ())


POINTWISE_CHECKS = sum(1 + 2 + sum(4 if r == "tmp" else 3 for r in pipeline_routes(n, w, h)) for n in POINTWISE_N for (w, h) in POINTWISE_SHAPES)


def pointwise(b):
    """gsh_histogram_batch (n x 256 u32: all written), gsh_otsu_batch (hist_scratch: the n histograms; thr: n bytes) and
    gsh_edge_pipeline_batch, by the launcher's conditions (gs_stencil.cpp):
      "fused"   tmp == NULL, w % 16 == 0, w >= 32, h > 2 r, src and dst 16-byte aligned (offset 0): the hot path --
                launch_blur_sobel_hist writes dst and the per-block partial histograms, k_otsu (its `partial` branch) folds
                them into hist_scratch and writes thr, then k_threshold and k_zero_frame on dst.  64 x 23 only; with n = 5
                once more in chunks of 2 frames (key 5 = 2: the side stream on the GPU)
      "ragged"  tmp == NULL, w % 16 != 0 or src / dst at odd addresses (offsets 1 and 3): gsh_blur_sobel_batch (the fused
                kernel without its histogram half), then k_hist + k_otsu, k_threshold
      "tmp"     tmp given: launch_blur into tmp, launch_sobel, k_zero_frame, k_hist + k_otsu, k_threshold
    dst, tmp, hist_scratch and thr all guarded.  n in {1, 3, 5}: thr's n bytes end off a dword boundary, and thr also
    starts off one (offsets 1 and 3)."""
    g, o, m = b.g, b.o, b.dev
    for n in POINTWISE_N:
        for w, h in POINTWISE_SHAPES:
            img = _noise((n, h, w), n * w)
            s = m.put(img, 1)
            what = "%d x %dx%d" % (n, w, h)
            hists = np.stack([o.histogram(f) for f in img])
            hb, hv = m.make((n, 256), np.uint32, 4)
            g.histogram_batch(s, hv)
            b.sync()
            m.check(hb, hists, "gsh_histogram_batch " + what)
            hb, hv = m.make((n, 256), np.uint32, 0)
            tb, tv = m.make(n, np.uint8, 1)
            g.otsu_batch(s, hv, tv)
            b.sync()
            m.check(hb, hists, "gsh_otsu_batch hist_scratch " + what)
            m.check(tb, np.array([o.otsu_threshold(f) for f in img], np.uint8), "gsh_otsu_batch thr " + what)
            r = 2 if h > 4 else 1
            blurred = np.stack([o.blur(f, r) for f in img])
            edges = np.stack([o.sobel(f) for f in blurred])
            thr = np.array([o.otsu_threshold(f) for f in edges], np.uint8)
            final = np.stack([o.threshold(f, int(t)) for f, t in zip(edges, thr)])
            for route in pipeline_routes(n, w, h):
                with_tmp, aligned = route == "tmp", route.startswith("fused")
                tag = "gsh_edge_pipeline_batch (%s) %s" % (route, what)
                db, d = m.make((n, h, w), np.uint8, 0 if aligned else 3, stride=w)
                hb, hv = m.make((n, 256), np.uint32, 4)
                tb, tv = m.make(n, np.uint8, 3)
                pb, pv = m.make((n, h, w), np.uint8, 2, stride=w) if with_tmp else (None, None)
                if aligned:
                    assert w % 16 == 0 and w >= 32 and h > 2 * r and _ptr(d) % 16 == 0
                try:
                    g.tune(5, 2 if route == "fused, chunks of 2" else 0)
                    g.edge_pipeline_batch(d, pv, m.put(img, 0) if aligned else s, r, hv, tv)
                    b.sync()
                finally:
                    g.tune(5, 0)
                m.check(db, final, tag + " dst")
                m.check(hb, np.stack([o.histogram(f) for f in edges]), tag + " hist_scratch")
                m.check(tb, thr, tag + " thr")
                if with_tmp:
                    m.check(pb, blurred, tag + " tmp")


THRESHOLD_OFFS = tuple(range(1, 16))
THRESHOLD_SHAPES = ((33, 3), (5, 1), (257, 2))
THRESHOLD_CHECKS = len(THRESHOLD_OFFS) * 3 * 2


def threshold(b):
    """gsh_threshold_batch, gsh_threshold_batch_dev and gsh_threshold_batch_dev_offset in place on 3 frames at byte
    offsets 1 .. 15 (k_threshold packs 16-byte accesses where it can): the guards are the neighbours; thr is read only"""
    g, o, m = b.g, b.o, b.dev
    for i, off in enumerate(THRESHOLD_OFFS):
        w, h = THRESHOLD_SHAPES[i % len(THRESHOLD_SHAPES)]
        img = _noise((3, h, w), off)
        thr = np.array([0, 128, 250], np.uint8)
        for kind in ("const", "dev", "dev_offset"):
            ib, iv = m.make((3, h, w), np.uint8, off, prefill=img, stride=w)
            tb, tv = m.make(3, np.uint8, off % 4, prefill=thr)
            if kind == "const":
                g.threshold_batch(iv, 77)
                exp = np.stack([o.threshold(f, 77) for f in img])
            elif kind == "dev":
                g.threshold_batch(iv, tv)
                exp = np.stack([o.threshold(f, int(t)) for f, t in zip(img, thr)])
            else:
                g.threshold_batch_dev_offset(iv, tv, 10)
                exp = np.stack([o.threshold(f, (int(t) + 10) & 255) for f, t in zip(img, thr)])
            b.sync()
            m.check(ib, exp, "gsh_threshold_batch %s 3 x %dx%d at +%d" % (kind, w, h, off))
            m.check(tb, None, "gsh_threshold_batch %s thr (read only)" % kind)


SYNTH_SHAPES = ((8, 8), (13, 5), (33, 2), (5, 3), (67, 45), (16, 17))   # w*h % 4 = 0, 1, 2, 3, 3, 0; four below 256 pixels
SYNTH_CHECKS = len(SYNTH_SHAPES) * 2 * 2


def _checksum(a):
    a = np.ascontiguousarray(a).reshape(-1)
    return np.sum(np.arange(1, a.size + 1, dtype=np.uint64) * (a.astype(np.uint64) + np.uint64(1)), dtype=np.uint64)


def synth_checksum(b):
    """gsh_synth_batch (k_synth_pixels packs dword stores when aligned: frames of w*h % 4 in {0, 1, 2, 3} at offsets 0 and
    1, frames smaller than one 256-pixel run) and gsh_checksum_batch (n u64 sums, n = 3)"""
    g, m = b.g, b.dev
    for w, h in SYNTH_SHAPES:
        exp = np.stack([Oracle.synth(w, h, 40 + f) for f in range(3)])
        for off in (0, 1):
            db, d = m.make((3, h, w), np.uint8, off, stride=w)
            g.synth_batch(d, 40)
            b.sync()
            m.check(db, exp, "gsh_synth_batch 3 x %dx%d at +%d" % (w, h, off))
            sb, sv = m.make(3, np.uint64, 8 * off)
            g.checksum_batch(m.put(exp, off), sv)
            b.sync()
            m.check(sb, np.array([_checksum(f) for f in exp], np.uint64), "gsh_checksum_batch 3 x %dx%d at +%d" % (w, h, off))


# ======================================================================================================================
# capped record lists: FAST, ORB, match, LBP
# ======================================================================================================================
def _caps(H):
    """caps around the oracle's uncapped count H: 1 and H - 1 cut the list (H > cap), H and H + 1 do not"""
    assert H >= 3, "the input yields %d records: too few for caps of 1, H - 1, H, H + 1" % H
    caps = (1, H - 1, H, H + 1)
    assert H > caps[0] and H > caps[1]
    return caps


def _busy_flat(busy, n=3):
    """busy, flat, busy[, flat, busy]: a flat (all 100) frame has no corners / hits, and a busy frame comes last"""
    flat = np.full_like(busy[0], 100)
    return np.stack([busy[i // 2] if i % 2 == 0 else flat for i in range(n)])


def _lay(exp, f, recs):
    """oracle records over the first len(recs) slots of frame f of an expected record list"""
    if len(recs):
        exp[f, :len(recs)] = recs


FAST_SHAPES = ((7, 7), (40, 8), (260, 17), (1283, 5), (1283, 9))
FAST_KEYS = (0, 2)


def _fast_frames(w, h):
    rs = np.random.RandomState(w + h)
    busy = [(rs.randint(0, 256, (h, w)) * (rs.rand(h, w) < 0.7)).astype(np.uint8) for _ in range(2)]
    if (w, h) == (7, 7):  # one interior pixel: a dark centre in a bright ring is its only corner
        for f in busy:
            f[...] = 200
            f[3, 3] = 10
    return _busy_flat(busy)


def fast_checks(w, h):
    if h < 7:
        return len(FAST_KEYS) * (2 * 3 + 2 * 2)
    return len(FAST_KEYS) * (1 + (4 if (w, h) != (7, 7) else 1) * 3 + 2 * 2)


def fast(b, w, h, thr=20):
    """gsh_fast_score_batch (k_fast_score_q4; key 7 = 2: k_fast_score_px), gsh_fast_batch and gs_fast (score pass,
    k_fast_nms_sparse, k_emit) at sizes whose tiles stick out of the frame.  Score maps: the interior is written, the
    3-px frame keeps the prefill.  kps: whole 48-byte records below counts[f] (angle and descriptor as 0, like the
    reference's compound literal, ref :530); records at and beyond counts[f] keep the prefill; counts: all n.
    Batches are busy, flat, busy: the flat frame's slots stay the prefill.  Caps 1, H - 1, H, H + 1 around the uncapped
    count H of the busiest frame (7 x 7 has one candidate pixel: cap 1 only).  At 1283 x 5 the reference's loops are empty
    (ref :489) and gsh_fast_score_batch's precondition h >= 7 excludes it: gsh_fast_batch and gs_fast write the zero counts
    and nothing else, neither the lists nor the score maps; 1283 x 9 is the same width with an interior."""
    g, o, m = b.g, b.o, b.dev
    frames = _fast_frames(w, h)
    n = len(frames)
    try:
        for key in FAST_KEYS:
            g.tune(7, key)
            tag = "%dx%d key 7 = %d" % (w, h, key)
            s = m.put(frames, 1)
            H = max(len(o.fast(f, 100000, thr)[0]) for f in frames)
            if h >= 7:
                sb, sv = m.make((n, h, w), np.uint8, 3, stride=w)
                g.fast_score_batch(sv, s, thr)
                b.sync()
                m.check(sb, np.stack([o.fast(frames[f], 1, thr, sb.expected()[f])[1] for f in range(n)]), "gsh_fast_score_batch " + tag)
                assert H >= 1 and len(o.fast(frames[1], 100000, thr)[0]) == 0
            else:
                assert H == 0
            for cap in ((1, 5) if h < 7 else _caps(H) if (w, h) != (7, 7) else (1,)):
                sb, sv = m.make((n, h, w), np.uint8, 1, stride=w)
                kb, kv = m.make((n, cap), KEYPOINT_DTYPE, b.roff)
                cb, cv = m.make(n, np.uint32, 4)
                g.fast_batch(s, sv, kv, cv, cap, thr)
                b.sync()
                ek, es, ec = kb.expected(), sb.expected(), np.zeros(n, np.uint32)
                for f in range(n):
                    ko, es[f] = o.fast(frames[f], cap, thr, es[f])
                    _lay(ek, f, ko)
                    ec[f] = len(ko)
                m.check(kb, ek, "gsh_fast_batch kps cap %d of %d, %s" % (cap, H, tag))
                m.check(cb, ec, "gsh_fast_batch counts cap %d, %s" % (cap, tag))
                m.check(sb, es, "gsh_fast_batch score map cap %d, %s" % (cap, tag))
            for path in ("dev", "host"):
                mm = b.mem(path)
                H0 = len(o.fast(frames[0], 100000, thr)[0])   # gs_fast runs on frame 0: one below what IT yields
                cap = max(1, H0 - 1)
                assert H0 > cap or H0 <= 1, "gs_fast would not be capped"
                with b.dropin(path):
                    sb, sv = mm.make((h, w), np.uint8, 2)
                    kb, kv = mm.make(cap, KEYPOINT_DTYPE, b.roff)
                    got = g.c.gs_fast(_img(mm.put(frames[0], 1)), _img(sv), _ptr(kv), cap, thr)
                    b.sync()
                ko, es = o.fast(frames[0], cap, thr, sb.expected())
                assert got == len(ko)
                ek = kb.expected()
                ek[:len(ko)] = ko
                mm.check(kb, ek, "gs_fast kps cap %d (%s) %s" % (cap, path, tag))
                mm.check(sb, es, "gs_fast score map (%s) %s" % (path, tag))
    finally:
        g.tune(7, 0)


ORB_SHAPES = ((96, 80), (130, 70))


def _orb_frames(w, h):
    busy = [Oracle.synth(w, h, 31 + w), _noise((h, w), 3 + w)]
    return _busy_flat(busy)


def orb_checks():
    return 4 * (3 + 3 + 1 + 1) + 3 * 2 + 2


def orb(b, w, h, thr=20):
    """gsh_orb_extract_batch and gsh_orb_extract (host lists: the records are set field by field on the host),
    gsh_orb_extract_batch_nostdlib (device lists: k_orb_select writes x, y, response of the first counts[f] records,
    k_orb_describe their angle and descriptor), gs_orb_extract and gs_orb_extract_nostdlib, with nkps 1, H - 1, H, H + 1
    around the number H of keypoints the busiest frame yields uncapped.  Records at and beyond counts[f] keep the prefill;
    the score map's 3-px frame too."""
    g, o, m, hm = b.g, b.o, b.dev, b.host
    ns = b.nostdlib()
    frames = _orb_frames(w, h)
    n = len(frames)
    H = max(len(o.orb_extract(f, 100000, thr)) for f in frames)
    assert len(o.orb_extract(frames[1], 100000, thr)) == 0
    s = m.put(frames, 1)
    for cap in _caps(H):
        tag = "%dx%d nkps %d of %d" % (w, h, cap, H)
        # host lists
        sb, sv = m.make((n, h, w), np.uint8, 3, stride=w)
        kb, kv = hm.make((n, cap), KEYPOINT_DTYPE, b.roff)
        cb, cv = hm.make(n, np.uint32, 4)
        g.c.gsh_orb_extract_batch(_ptr(s), w, h, n, _ptr(sv), _ptr(kv), _ptr(cv), cap, thr)
        b.sync()
        ek, es, ec = kb.expected(), sb.expected(), np.zeros(n, np.uint32)
        for f in range(n):
            ko = o.orb_extract(frames[f], cap, thr, es[f])
            es[f] = o.fast(frames[f], min(cap * 4, 5000), thr, es[f])[1]
            _lay(ek, f, ko)
            ec[f] = len(ko)
        hm.check(kb, ek, "gsh_orb_extract_batch kps " + tag)
        hm.check(cb, ec, "gsh_orb_extract_batch counts " + tag)
        m.check(sb, es, "gsh_orb_extract_batch score maps " + tag)
        # device lists, GS_NO_STDLIB trig
        sb, sv = m.make((n, h, w), np.uint8, 1, stride=w)
        kb, kv = m.make((n, cap), KEYPOINT_DTYPE, b.roff)
        cb, cv = m.make(n, np.uint32, 4)
        g.orb_extract_batch_nostdlib(s, sv, kv, cv, cap, thr)
        b.sync()
        ek, es, ec = kb.expected(), sb.expected(), np.zeros(n, np.uint32)
        for f in range(n):
            ko = ns.orb_extract(frames[f], cap, thr, es[f])
            es[f] = o.fast(frames[f], min(cap * 4, 5000), thr, es[f])[1]
            _lay(ek, f, ko)
            ec[f] = len(ko)
        m.check(kb, ek, "gsh_orb_extract_batch_nostdlib kps " + tag)
        m.check(cb, ec, "gsh_orb_extract_batch_nostdlib counts " + tag)
        m.check(sb, es, "gsh_orb_extract_batch_nostdlib score maps " + tag)
        # one device frame, host list
        kb, kv = hm.make(cap, KEYPOINT_DTYPE, b.roff)
        got = g.c.gsh_orb_extract(_ptr(s[2]), w, h, _ptr(m.put(frames[2])), _ptr(kv), cap, thr)
        ko = o.orb_extract(frames[2], cap, thr)
        assert got == len(ko)
        ek = kb.expected()
        ek[:len(ko)] = ko
        hm.check(kb, ek, "gsh_orb_extract kps " + tag)
        # gs_orb_extract with host pointers (this cap), device pointers below
        sb, sv = hm.make((h, w), np.uint8, 1)
        kb, kv = hm.make(cap, KEYPOINT_DTYPE, b.roff)
        got = g.c.gs_orb_extract(_img(hm.put(frames[0], 3)), _ptr(kv), cap, thr, _ptr(sv))
        ko = o.orb_extract(frames[0], cap, thr, sb.expected())
        assert got == len(ko)
        ek = kb.expected()
        ek[:len(ko)] = ko
        hm.check(kb, ek, "gs_orb_extract kps (host) " + tag)
    cap = len(o.orb_extract(frames[0], 100000, thr)) - 1   # one below what frame 0 yields: H > cap
    assert cap >= 2
    for path in ("dev", "host"):
        mm = b.mem(path)
        for flavour, orc in (("", o), ("_nostdlib", ns)):
            if flavour == "" and path == "host":
                continue  # done above for every cap
            with b.dropin(path):
                sb, sv = mm.make((h, w), np.uint8, 1)
                kb, kv = mm.make(cap, KEYPOINT_DTYPE, b.roff)
                fn = getattr(g.c, "gs_orb_extract" + flavour)
                got = fn(_img(mm.put(frames[0], 3)), _ptr(kv), cap, thr, _ptr(sv))
                b.sync()
            ko = orc.orb_extract(frames[0], cap, thr, sb.expected())
            assert got == len(ko) == cap
            ek = kb.expected()
            ek[:len(ko)] = ko
            mm.check(kb, ek, "gs_orb_extract%s kps (%s) %dx%d nkps %d" % (flavour, path, w, h, cap))
            mm.check(sb, o.fast(frames[0], min(cap * 4, 5000), thr, sb.expected())[1], "gs_orb_extract%s score map (%s)" % (flavour, path))
    # nkps above the candidates through the staged path: the copy-back takes the count, not the cap
    sb, sv = hm.make((h, w), np.uint8, 1)
    kb, kv = hm.make(H + 1, KEYPOINT_DTYPE, b.roff)
    got = g.c.gs_orb_extract_nostdlib(_img(hm.put(frames[2], 3)), _ptr(kv), H + 1, thr, _ptr(sv))
    ko = ns.orb_extract(frames[2], H + 1, thr, sb.expected())
    assert got == len(ko)
    ek = kb.expected()
    ek[:len(ko)] = ko
    hm.check(kb, ek, "gs_orb_extract_nostdlib kps (host) nkps above the candidates")
    hm.check(sb, o.fast(frames[2], min((H + 1) * 4, 5000), thr, sb.expected())[1], "gs_orb_extract_nostdlib score map (host)")


ORB_PYRAMID_CASES = ((96, 80, 3), (130, 70, 4), (160, 130, 3))
ORB_PYRAMID_CHECKS = 4 * 2


def orb_pyramid(b, w, h, levels, thr=20):
    """gsh_orb_extract_pyramid: buffer_dev of exactly gsh_orb_pyramid_buffer_bytes inside guards (levels 1.. back to back,
    then one score map per level; the maps' 3-px frames keep the caller's bytes), the host kps list inside guards;
    nkps 1, H - 1, H, H + 1 around the keypoints H all levels yield together, none of them divisible by the number of
    levels where that can be had.  Records at and beyond the returned count keep the prefill."""
    g, o, m, hm = b.g, b.o, b.dev, b.host
    img = Oracle.synth(w, h, 21)
    nb = g.orb_pyramid_buffer_bytes(w, h, levels)
    assert nb == o.orb_pyramid_buffer_bytes(w, h, levels)
    H = len(o.orb_extract_pyramid(img, 100000, thr, levels)[0])
    s = m.put(img, 1)
    for cap in _caps(H):
        bb, bv = m.make(nb, np.uint8, 1, stride=w)
        kb, kv = hm.make(cap, KEYPOINT_DTYPE, b.roff)
        got = g.c.gsh_orb_extract_pyramid(_ptr(s), w, h, _ptr(bv), _ptr(kv), cap, thr, levels)
        ko, bo = o.orb_extract_pyramid(img, cap, thr, levels, bb.expected())
        assert got == len(ko), "pyramid count %d, expected %d" % (got, len(ko))
        ek = kb.expected()
        ek[:len(ko)] = ko
        hm.check(kb, ek, "gsh_orb_extract_pyramid kps %dx%d %d levels nkps %d of %d" % (w, h, levels, cap, H))
        m.check(bb, bo[:nb], "gsh_orb_extract_pyramid buffer %dx%d %d levels nkps %d" % (w, h, levels, cap))


MATCH_SIZES = ((5, 63), (70, 513), (9, 255))
MATCH_CHECKS = 4 * 2 + 2 * 2


def match(b, n1, n2):
    """gsh_match_orb_dev and gs_match_orb (k_match, k_emit<MatchEmit>) on random_descriptors: max_matches 1, H - 1, H,
    H + 1 around the H matches accepted at distance 256.  matches: whole 12-byte records below count, the rest keeps
    the prefill; count: one u32."""
    g, o, m = b.g, b.o, b.dev
    k1, k2 = pc.random_descriptors(n1, n2)
    H = len(o.match_orb(k1, k2, n1 + 5, 256.0))
    d1, d2 = m.put(k1, 4), m.put(k2, 8)
    for cap in _caps(H):
        exp = o.match_orb(k1, k2, cap, 256.0)
        mb, mv = m.make(cap, MATCH_DTYPE, b.roff)
        cb, cv = m.make(1, np.uint32, 4)
        g.match_orb_dev(d1, n1, d2, n2, mv, cv, cap, 256.0)
        b.sync()
        em = mb.expected()
        em[:len(exp)] = exp
        m.check(mb, em, "gsh_match_orb_dev matches %d x %d max %d of %d" % (n1, n2, cap, H))
        m.check(cb, np.array([len(exp)], np.uint32), "gsh_match_orb_dev count %d x %d max %d" % (n1, n2, cap))
    for path in ("dev", "host"):
        mm = b.mem(path)
        for cap in (H - 1, H + 1):
            exp = o.match_orb(k1, k2, cap, 256.0)
            with b.dropin(path):
                mb, mv = mm.make(cap, MATCH_DTYPE, b.roff)
                got = g.c.gs_match_orb(_ptr(mm.put(k1, 4)), n1, _ptr(mm.put(k2, 4)), n2, _ptr(mv), cap, 256.0)
                b.sync()
            assert got == len(exp)
            em = mb.expected()
            em[:len(exp)] = exp
            mm.check(mb, em, "gs_match_orb (%s) %d x %d max %d of %d" % (path, n1, n2, cap, H))


LBP_CASES = ((64, 48, 1, 0), (64, 48, 2, 1), (96, 80, 2, 0), (96, 80, 1, 1))   # (w, h, step, key 14)
LBP_CHECKS = 4 * 2 + 2


def lbp(b, w, h, step, key14):
    """gsh_lbp_detect_batch and gs_lbp_detect with random_cascade(seed, permissive=True): thousands of hits; key 14 = 0
    the rule's choice (k_lbp_tile where the tile fits), 1 k_lbp_cascade for every scale.  max_rects 1, H - 1, H, H + 1
    around the busiest frame's uncapped count H; frames busy, flat, busy (a flat frame passes no window of this
    cascade: asserted).  rects: whole 16-byte records below counts[f], the rest keeps the prefill; counts: all n."""
    g, o, m = b.g, b.o, b.dev
    rc = random_cascade(1, permissive=True)
    params = (1.2, 1.0, 2.5, step)
    busy = [Oracle.synth(w, h, 9), Oracle.synth(w, h, 12)]
    flat = np.zeros((h, w), np.uint8)
    frames = np.stack([busy[0], flat, busy[1]])
    ii = np.stack([o.integral(f) for f in frames])
    full = [o.lbp_detect(rc, t, 1000000, *params) for t in ii]
    H = max(len(r) for r in full)
    assert len(full[1]) == 0 and len(full[0]) >= 3, "the flat frame must pass no window, the busy ones many"
    dc = g.cascade_create(rc)
    try:
        g.tune(14, key14)
        dii = m.put(ii, 4)
        for cap in _caps(H):
            rb, rv = m.make((3, cap), RECT_DTYPE, b.roff)
            cb, cv = m.make(3, np.uint32, 4)
            g.lbp_detect_batch(dc, dii, rv, cv, cap, *params)
            b.sync()
            er, ec = rb.expected(), np.zeros(3, np.uint32)
            for f in range(3):
                _lay(er, f, full[f][:cap])
                ec[f] = min(len(full[f]), cap)
            m.check(rb, er, "gsh_lbp_detect_batch rects %dx%d step %d key 14 = %d max %d of %d" % (w, h, step, key14, cap, H))
            m.check(cb, ec, "gsh_lbp_detect_batch counts max %d" % cap)
        for path in ("dev", "host"):
            mm = b.mem(path)
            cap = len(full[0]) - 1
            with b.dropin(path):
                rb, rv = mm.make(cap, RECT_DTYPE, b.roff)
                got = g.c.gs_lbp_detect(C.addressof(rc.as_struct()), _ptr(mm.put(ii[0], 4)), w, h, _ptr(rv), cap, *params)
                b.sync()
            assert got == cap
            mm.check(rb, full[0][:cap], "gs_lbp_detect (%s) %dx%d step %d max %d" % (path, w, h, step, cap))
    finally:
        g.tune(14, 0)
        dc.close()
    return [len(r) for r in full]


# ======================================================================================================================
# blobs, corners, largest, perspective, contours
# ======================================================================================================================
BLOB_WIDTHS = (63, 64, 65, 130)
BLOB_CHECKS = 4 * 3 + 3 + 1 + 2 * 3


def _blobs_ref(img, cap):
    from oracle import pyoracle
    return bc.Ref().blobs(img, cap) if pyoracle.have_reference() else bc.spec_blobs(img, cap)


def _corners_ref(img, labels, blob):
    """gs_blob_corners of the compiled reference where oracle/_ref is built, else the restatement of blob_cases"""
    from oracle import pyoracle
    return bc.Ref().corners(img, labels, blob) if pyoracle.have_reference() else bc.spec_corners(img, labels, blob)


def _perspective_ref(dw, dh, src, corners):
    """gs_perspective_correct of the compiled reference where oracle/_ref is built, else the restatement"""
    from oracle import pyoracle
    return bc.Ref().perspective(dw, dh, src, corners) if pyoracle.have_reference() else bc.spec_perspective(dw, dh, src, corners)


def _blob_frames(w, h=12):
    rng = np.random.default_rng(w)
    busy = [cc.random_rects(rng, h, w, 14, 1, 6), bc.random_mask(rng, h, w, 0.35)]
    return np.stack([busy[0], np.zeros((h, w), np.uint8), busy[1]])


def blobs(b, w):
    """gsh_blobs_batch (k_blob_label stores 8 labels per 16 bytes: w in {63, 64, 65, 130} with the labels at 2-byte
    offsets meets a ragged row end), nblobs 1, H - 1, H, H + 1: labels all written; records below counts[f] whole (the
    two padding bytes as 0), the rest untouched (the header's promise); counts all n.  gsh_blob_largest_batch with and
    without index, gsh_blob_corners_batch; gs_blobs and gs_blob_corners on both paths."""
    g, m = b.g, b.dev
    frames = _blob_frames(w)
    n, h = frames.shape[0], frames.shape[1]
    H = max(len(_blobs_ref(f, 60000)[0]) for f in frames)
    s = m.put(frames, 1)
    last = None
    for cap in _caps(H):
        lb, lv = m.make((n, h, w), np.uint16, 2, stride=2 * w)
        rb, rv = m.make((n, cap), BLOB_DTYPE, b.roff)
        cb, cv = m.make(n, np.uint32, 4)
        g.blobs_batch(s, lv, rv, cv, cap)
        b.sync()
        el, er, ec = lb.expected(), rb.expected(), np.zeros(n, np.uint32)
        for f in range(n):
            recs, el[f] = _blobs_ref(frames[f], cap)
            recs = recs.copy()
            recs["pad"] = 0
            _lay(er, f, recs)
            ec[f] = len(recs)
        tag = "%d x %dx%d nblobs %d of %d" % (n, w, h, cap, H)
        m.check(lb, el, "gsh_blobs_batch labels " + tag)
        m.check(rb, er, "gsh_blobs_batch records " + tag)
        m.check(cb, ec, "gsh_blobs_batch counts " + tag)
        if cap == H:
            last = (el, er, ec)
    el, er, ec = last
    d_lab, d_rec, d_cnt = m.put(el, 2), m.put(er, 4), m.put(ec, 4)
    for with_index in (True, False):
        gb, gv = m.make(n, BLOB_DTYPE, b.roff)
        ib, iv = m.make(n, np.uint32, 4)
        g.blob_largest_batch(d_rec, d_cnt, gv, iv if with_index else None)
        b.sync()
        eg, ei = np.zeros(n, BLOB_DTYPE), np.full(n, 0xFFFFFFFF, np.uint32)
        for f in range(n):
            if ec[f]:
                best = 0
                for i in range(1, int(ec[f])):
                    if er[f, i]["area"] > er[f, best]["area"]:
                        best = i
                eg[f], ei[f] = er[f, best], best
        m.check(gb, eg, "gsh_blob_largest_batch largest (index %s) %dx%d" % ("given" if with_index else "NULL", w, h))
        if with_index:
            m.check(ib, ei, "gsh_blob_largest_batch index %dx%d" % (w, h))
    # corners of each frame's first record (the flat frame: a record of zeros, centroid (0, 0))
    first = np.zeros(n, BLOB_DTYPE)
    for f in range(n):
        if ec[f]:
            first[f] = er[f, 0]
    kb, kv = m.make((n, 4), POINT_DTYPE, b.roff)
    fr = m.put(first, 4)
    g.blob_corners_batch(s, d_lab, fr, kv)
    b.sync()
    ek = np.zeros((n, 4), POINT_DTYPE)
    for f in range(n):
        for i, (x, y) in enumerate(_corners_ref(frames[f], el[f], first[f])):
            ek[f, i] = (x, y)
    m.check(kb, ek, "gsh_blob_corners_batch %dx%d" % (w, h))
    for path in ("dev", "host"):
        mm = b.mem(path)
        cap = H - 1
        with b.dropin(path):
            lb, lv = mm.make((h, w), np.uint16, 2, stride=2 * w)
            rb, rv = mm.make(cap, BLOB_DTYPE, b.roff)
            got = g.c.gs_blobs(_img(mm.put(frames[2], 1)), _ptr(lv), _ptr(rv), cap)
            b.sync()
            recs, labels = _blobs_ref(frames[2], cap)
            recs = recs.copy()
            recs["pad"] = 0
            assert got == len(recs)
            e = rb.expected()
            e[:len(recs)] = recs
            mm.check(lb, labels, "gs_blobs labels (%s) %dx%d nblobs %d" % (path, w, h, cap))
            mm.check(rb, e, "gs_blobs records (%s) %dx%d nblobs %d" % (path, w, h, cap))
            kb, kv = mm.make(4, POINT_DTYPE, b.roff)
            g.c.gs_blob_corners(_img(mm.put(frames[2], 1)), _ptr(mm.put(labels, 2)), _ptr(mm.put(recs[:1], 4)), _ptr(kv))
            b.sync()
            e = np.zeros(4, POINT_DTYPE)
            for i, (x, y) in enumerate(_corners_ref(frames[2], labels, recs[0])):
                e[i] = (x, y)
            mm.check(kb, e, "gs_blob_corners (%s) %dx%d" % (path, w, h))


PERSPECTIVE_DST = ((13, 7), (64, 5), (65, 6), (129, 2), (1, 9), (63, 4))
PERSPECTIVE_CHECKS = len(PERSPECTIVE_DST) * 3


def perspective(b):
    """gsh_perspective_correct_batch (k_perspective, blocks of 64 x 4: dw % 64 and dh % 4 as for resize, a 1-wide
    destination) on 3 frames, and gs_perspective_correct on both paths.  Every byte of the destination is the call's."""
    g, m = b.g, b.dev
    src = np.stack([Oracle.synth(40, 30, 5 + f) for f in range(3)])
    corners = np.array([[[3, 2], [35, 4], [38, 27], [1, 25]], [[0, 0], [39, 0], [39, 29], [0, 29]], [[10, 5], [20, 3], [30, 28], [5, 20]]], np.uint32)
    s, c = m.put(src, 1), m.put(corners, 4)
    for i, (dw, dh) in enumerate(PERSPECTIVE_DST):
        exp = np.stack([_perspective_ref(dw, dh, src[f], [tuple(p) for p in corners[f].tolist()]) for f in range(3)])
        db, d = m.make((3, dh, dw), np.uint8, i % 4, stride=dw)
        g.perspective_correct_batch(d, s, c)
        b.sync()
        m.check(db, exp, "gsh_perspective_correct_batch 3 x -> %dx%d at +%d" % (dw, dh, i % 4))
        for path in ("dev", "host"):
            mm = b.mem(path)
            with b.dropin(path):
                db, d = mm.make((dh, dw), np.uint8, (i + 1) % 4)
                g.c.gs_perspective_correct(_img(d), _img(mm.put(src[0], 1)), _ptr(mm.put(corners[0], 4)))
                b.sync()
            mm.check(db, exp[0], "gs_perspective_correct (%s) -> %dx%d" % (path, dw, dh))


CONTOUR_SHAPES = ((33, 21, 3), (64, 17, 3), (47, 9, 5))   # (w, h, n): n * per_frame odd where per_frame is
CONTOUR_CHECKS = 2 * 3 + 1 + 2


def contours(b, w, h, n):
    """gsh_blob_contour_starts_batch (only `start` of the records below counts[f] is written) and
    gsh_trace_contours_batch (of each record below counts[f] box and length are written, start is read; status entries
    below counts[f]; visited: the pixels the reference marks) on frames busy, flat, busy[, flat, busy], with counts from
    gsh_blobs_batch and with counts == NULL over a list of exactly per_frame records, n * per_frame odd; gs_trace_contour
    on both paths (visited guarded; the record is the host's)."""
    g, m = b.g, b.dev
    rng = np.random.default_rng(w * h)
    busy = [cc.random_discs(rng, h, w, 5, 2, 5) for _ in range(3)]
    frames = np.stack([busy[i // 2] if i % 2 == 0 else np.zeros((h, w), np.uint8) for i in range(n)])
    refs = [_blobs_ref(f, 60000) for f in frames]
    per = max(len(r[0]) for r in refs) | 1
    assert (n * per) % 2 == 1
    labels = np.stack([r[1] for r in refs])
    recs = np.zeros((n, per), BLOB_DTYPE)
    counts = np.zeros(n, np.uint32)
    for f, (r, _) in enumerate(refs):
        recs[f, :len(r)], counts[f] = r, len(r)
        # behind the count a stale record any pixel of row 0 without a label answers to: reading it would write a start
        recs[f, len(r):]["area"], recs[f, len(r):]["w"], recs[f, len(r):]["h"] = 1, w, h
    s = m.put(frames, 1)
    d_lab, d_rec, d_cnt = m.put(labels, 2), m.put(recs, 4), m.put(counts, 4)
    cb, cv = m.make((n, per), CONTOUR_DTYPE, b.roff)
    g.blob_contour_starts_batch(d_lab, d_rec, d_cnt, cv)
    b.sync()
    ec = cb.expected()
    starts = []
    for f in range(n):
        st = [(int(np.nonzero(labels[f][int(r["y"])] == r["label"])[0][0]), int(r["y"])) for r in refs[f][0]]
        starts.append(st)
        for k, (x, y) in enumerate(st):
            ec[f, k]["sx"], ec[f, k]["sy"] = x, y
    after_starts = m.check(cb, ec, "gsh_blob_contour_starts_batch %d x %dx%d, %d records per frame" % (n, w, h, per))
    for with_counts in (True, False):
        tag = "gsh_trace_contours_batch %d x %dx%d (counts %s)" % (n, w, h, "given" if with_counts else "NULL")
        # counts == NULL traces all per_frame records: the ones behind the blobs start at pixel (0, 0)
        rec_in = after_starts.copy()
        if not with_counts:
            for f in range(n):
                rec_in[f, int(counts[f]):] = np.zeros(1, CONTOUR_DTYPE)
        vis0 = np.where(_noise((n, h, w), 7) < 40, 255, 0).astype(np.uint8)
        rb, rv = m.make((n, per), CONTOUR_DTYPE, b.roff, prefill=rec_in)
        vb, vv = m.make((n, h, w), np.uint8, 3, prefill=vis0, stride=w)
        sb, sv = m.make((n, per), np.uint8, 1)
        g.trace_contours_batch(s, vv, rv, d_cnt if with_counts else None, sv)
        b.sync()
        er, ev, es = rb.expected(), vis0.copy(), sb.expected()
        for f in range(n):
            k_n = int(counts[f]) if with_counts else per
            st = [(int(rec_in[f, k]["sx"]), int(rec_in[f, k]["sy"])) for k in range(k_n)]
            want, ev[f], _ = cc.expected_sequence(frames[f], st, visited=vis0[f])
            for k, (length, box, status) in enumerate(want):
                er[f, k]["x"], er[f, k]["y"], er[f, k]["w"], er[f, k]["h"] = box
                er[f, k]["length"] = length
                es[f, k] = status
        m.check(rb, er, tag + " contours")
        m.check(vb, ev, tag + " visited")
        m.check(sb, es, tag + " status")
    for path in ("dev", "host"):
        mm = b.mem(path)
        st = starts[0][0]
        with b.dropin(path):
            vb, vv = mm.make((h, w), np.uint8, 1, prefill=np.zeros((h, w), np.uint8))
            got = g.trace_contour(mm.put(frames[0], 3), vv, st)
            b.sync()
        length, box, ev, _, _ = cc.spec_trace(frames[0], np.zeros((h, w), np.uint8), st)
        assert cc.rec_tuple(got) == (length, box)
        mm.check(vb, ev, "gs_trace_contour visited (%s) %dx%d" % (path, w, h))
