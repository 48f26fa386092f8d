"""Shared pieces of tests/test_blobs.py (emulator) and tests/test_gpu_blobs.py (MI355X): a plain-Python
restatement of gs_blobs / gs_blob_corners / gs_perspective_correct (ref grayskull.h:330-444, statement for
statement) for the hand-derived cases, the reference's compiled functions over ctypes, input generators and
the field-by-field comparison."""
import ctypes as C

import numpy as np

from grayskull_amd import BLOB_DTYPE, POINT_DTYPE
from grayskull_amd._abi import GsImage

FIELDS = ("label", "area", "x", "y", "w", "h", "cx", "cy")
U32 = 0xFFFFFFFF


def spec_blobs(img, nblobs):
    """ref :330-402 with Python ints: the labels array and the m compacted records"""
    h, w = img.shape
    fg = img >= 128
    labels = np.zeros((h, w), np.int64)
    parents = list(range(nblobs + 1))
    recs = {}

    def root(x):
        while parents[x] != x:
            parents[x] = parents[parents[x]]
            x = parents[x]
        return x

    nxt = 1
    for y in range(h):
        for x in range(w):
            if not fg[y, x]:
                continue
            left = labels[y, x - 1] if x > 0 else 0
            top = labels[y - 1, x] if y > 0 else 0
            n = min(left, top) if left and top else (left or top)
            if not n:
                if nxt > nblobs:
                    continue
                recs[nxt] = [1, x, y, x, y, x, y]
                labels[y, x] = nxt
                nxt += 1
            else:
                labels[y, x] = n
                r = recs[n]
                r[0] += 1
                r[1], r[2], r[3], r[4] = min(x, r[1]), min(y, r[2]), max(x, r[3]), max(y, r[4])
                r[5], r[6] = (r[5] + x) & U32, (r[6] + y) & U32
                if left and top and left != top:
                    a, b = root(left), root(top)
                    if a != b:
                        parents[max(a, b)] = min(a, b)
    for i in range(1, nxt):
        rt = root(i)
        if rt != i:
            a, b = recs[rt], recs[i]
            a[0] += b[0]
            a[1], a[2], a[3], a[4] = min(a[1], b[1]), min(a[2], b[2]), max(a[3], b[3]), max(a[4], b[4])
            a[5], a[6] = (a[5] + b[5]) & U32, (a[6] + b[6]) & U32
            b[0] = 0
    for y in range(h):
        for x in range(w):
            if labels[y, x]:
                labels[y, x] = root(labels[y, x])
    out = [(i, r[0], r[1], r[2], r[3] - r[1] + 1, r[4] - r[2] + 1, r[5] // r[0], r[6] // r[0])
           for i, r in sorted(recs.items()) if r[0]]
    recs_np = np.zeros(len(out), BLOB_DTYPE)
    for k, t in enumerate(out):
        for f, v in zip(FIELDS, t):
            recs_np[k][f] = v
    return recs_np, labels.astype(np.uint16)


def spec_corners(img, labels, b):
    """ref :404-421"""
    h, w = img.shape
    c = (int(b["cx"]), int(b["cy"]))
    tl = tr = br = bl = c
    mn_s, mx_s, mn_d, mx_d = 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, -2 ** 31
    y, ey, ex = int(b["y"]), (int(b["y"]) + int(b["h"])) & U32, (int(b["x"]) + int(b["w"])) & U32
    while y < ey:
        x = int(b["x"])
        while x < ex:
            if x < w and y < h and img[y, x] >= 128 and labels[y, x] == b["label"]:
                s, d = x + y, x - y
                if s < mn_s:
                    mn_s, tl = s, (x, y)
                if s > mx_s:
                    mx_s, br = s, (x, y)
                if d < mn_d:
                    mn_d, bl = d, (x, y)
                if d > mx_d:
                    mx_d, tr = d, (x, y)
            x += 1
        y += 1
    return [tl, tr, br, bl]


def spec_perspective(dw, dh, src, c):
    """ref :423-444 in float32, operation for operation (numpy float32 arithmetic does not contract)"""
    f = np.float32
    sh, sw = src.shape
    out = np.zeros((dh, dw), np.uint8)
    with np.errstate(invalid="ignore", divide="ignore"):
        wf, hf = f(dw) - f(1), f(dh) - f(1)
        for y in range(dh):
            for x in range(dw):
                u, v = f(x) / wf, f(y) / hf
                top_x = f(c[0][0]) * (f(1) - u) + f(c[1][0]) * u
                top_y = f(c[0][1]) * (f(1) - u) + f(c[1][1]) * u
                bot_x = f(c[3][0]) * (f(1) - u) + f(c[2][0]) * u
                bot_y = f(c[3][1]) * (f(1) - u) + f(c[2][1]) * u
                sx_f = top_x * (f(1) - v) + bot_x * v
                sy_f = top_y * (f(1) - v) + bot_y * v
                mx, my = f(sw) - f(1), f(sh) - f(1)
                sx_f = sx_f if sx_f < mx else mx
                sx_f = f(0) if f(0) > sx_f else sx_f
                sy_f = sy_f if sy_f < my else my
                sy_f = f(0) if f(0) > sy_f else sy_f
                sx, sy = int(sx_f), int(sy_f)
                sx1, sy1 = min(sx + 1, sw - 1), min(sy + 1, sh - 1)
                dx, dy = sx_f - f(sx), sy_f - f(sy)
                g = lambda xx, yy: f(src[yy, xx]) if xx < sw and yy < sh else f(0)  # noqa: E731
                p = (g(sx, sy) * (f(1) - dx) * (f(1) - dy)) + (g(sx1, sy) * dx * (f(1) - dy)) + \
                    (g(sx, sy1) * (f(1) - dx) * dy) + (g(sx1, sy1) * dx * dy)
                out[y, x] = int(p)
    return out


class Ref:
    """the compiled, unmodified reference header (oracle/_ref/libgs_ref.so) for the three functions and the scan
    chain's first stages"""

    def __init__(self):
        from oracle.pyoracle import REF_SO
        L = self.L = C.CDLL(REF_SO)
        L.gs_blobs.restype = C.c_uint
        L.gs_blobs.argtypes = [GsImage, C.c_void_p, C.c_void_p, C.c_uint]
        L.gs_blob_corners.argtypes = [GsImage, C.c_void_p, C.c_void_p, C.c_void_p]
        L.gs_perspective_correct.argtypes = [GsImage, GsImage, C.c_void_p]
        L.gs_blur.argtypes = [GsImage, GsImage, C.c_uint]
        L.gs_otsu_threshold.restype = C.c_uint8
        L.gs_otsu_threshold.argtypes = [GsImage]
        L.gs_threshold.argtypes = [GsImage, C.c_uint8]

    @staticmethod
    def _img(a):
        return GsImage(a.shape[1], a.shape[0], a.ctypes.data)

    def blobs(self, img, nblobs):
        img = np.ascontiguousarray(img)
        # with nblobs >= 65535 and more than 65535 start pixels the reference wraps its u16 label counter to 0 and
        # writes blobs[-1] (undefined behaviour: a heap corruption that aborts the process); never go there
        assert nblobs < 65535 or start_count(img) <= 65535, "the reference is undefined for this input"
        labels = np.zeros(img.shape, np.uint16)
        recs = np.zeros(nblobs, BLOB_DTYPE)
        m = self.L.gs_blobs(self._img(img), labels.ctypes.data, recs.ctypes.data, nblobs)
        return recs[:m].copy(), labels

    def corners(self, img, labels, blob):
        b = np.ascontiguousarray(np.asarray(blob, BLOB_DTYPE).reshape(1))
        c = np.zeros(4, POINT_DTYPE)
        self.L.gs_blob_corners(self._img(np.ascontiguousarray(img)), np.ascontiguousarray(labels).ctypes.data,
                               b.ctypes.data, c.ctypes.data)
        return [(int(p["x"]), int(p["y"])) for p in c]

    def perspective(self, dw, dh, src, corners):
        out = np.zeros((dh, dw), np.uint8)
        c = np.ascontiguousarray(np.asarray(corners, np.uint32).reshape(4, 2))
        self.L.gs_perspective_correct(self._img(out), self._img(np.ascontiguousarray(src)), c.ctypes.data)
        return out

    def scan(self, img, nblobs=1000, dw=800, dh=1000):
        """nanomagick's `scan` verb (ref examples/nanomagick/nanomagick.c:187-210), step by step"""
        tmp = np.zeros_like(img)
        self.L.gs_blur(self._img(tmp), self._img(img), 1)
        t = (int(self.L.gs_otsu_threshold(self._img(tmp))) + 10) & 255
        self.L.gs_threshold(self._img(tmp), t)
        recs, labels = self.blobs(tmp, nblobs)
        largest = 0
        for i in range(1, len(recs)):
            if recs[i]["area"] > recs[largest]["area"]:
                largest = i
        corners = self.corners(tmp, labels, recs[largest])
        return tmp, recs, labels, largest, corners, self.perspective(dw, dh, img, corners)


def assert_blobs_equal(got, want, what=""):
    (gr, gl), (wr, wl) = got, want
    assert len(gr) == len(wr), "%s: %d blobs, expected %d" % (what, len(gr), len(wr))
    for f in FIELDS:
        assert np.array_equal(np.asarray(gr[f], np.int64), np.asarray(wr[f], np.int64)), "%s: field %s differs" % (what, f)
    gl, wl = np.asarray(gl), np.asarray(wl)
    assert gl.shape == wl.shape and np.array_equal(gl, wl), \
        "%s: labels differ at %d pixels" % (what, int(np.count_nonzero(gl != wl)) if gl.shape == wl.shape else -1)


def start_count(img):
    fg = img >= 128
    left = np.zeros_like(fg)
    left[:, 1:] = fg[:, :-1]
    top = np.zeros_like(fg)
    top[1:] = fg[:-1]
    return int(np.count_nonzero(fg & ~left & ~top))


# ---- input families -----------------------------------------------------------------------------------------------
def random_mask(rng, h, w, density):
    return np.where(rng.random((h, w)) < density, 255, 0).astype(np.uint8)


def checkerboard(h, w):
    return ((np.indices((h, w)).sum(0) % 2) * 255).astype(np.uint8)


def spiral(h, w, gap=2):
    """one 1-px-wide square spiral: a single component that crosses every row and column band many times"""
    img = np.zeros((h, w), np.uint8)
    top, left, bottom, right = 0, 0, h - 1, w - 1
    while top <= bottom and left <= right:
        img[top, left:right + 1] = 255
        img[top:bottom + 1, right] = 255
        if bottom - top >= gap:
            img[bottom, left:right + 1] = 255
        if right - left >= gap and bottom - top > gap:
            img[top + gap:bottom + 1, left] = 255
        top, left, bottom, right = top + gap, left + gap, bottom - gap, right - gap
    return img


def maze(rng, h, w):
    """walls on a 2-px lattice with random openings: long, winding, many-branched components"""
    img = np.zeros((h, w), np.uint8)
    img[::2, :] = 255
    img[:, ::2] = 255
    holes = rng.random((h, w)) < 0.35
    img[holes & ((np.indices((h, w)).sum(0) % 2) == 1)] = 0
    return img


def dots(h, w, period=16, size=5):
    img = np.zeros((h, w), np.uint8)
    for dy in range(size):
        for dx in range(size):
            img[dy::period, dx::period] = 255
    return img


def blurred_noise(rng, h, w, passes=2):
    """smoothed noise (box filter over uint16) -> the caller thresholds it"""
    a = rng.integers(0, 256, (h, w)).astype(np.float32)
    for _ in range(passes):
        a = (a + np.roll(a, 1, 0) + np.roll(a, -1, 0) + np.roll(a, 1, 1) + np.roll(a, -1, 1)) / 5
    return np.clip(a, 0, 255).astype(np.uint8)


def emu_frames():
    """small frames that still span several 64-px words and many rows; widths off the word size"""
    rng = np.random.default_rng(2024)
    out = []
    for (h, w) in ((23, 70), (40, 131), (17, 200), (64, 64), (9, 257)):
        for d in (0.5, 0.59, 0.65, 0.8):
            out.append(("random %dx%d d=%.2f" % (w, h, d), random_mask(rng, h, w, d)))
    out.append(("checkerboard", checkerboard(21, 133)))
    out.append(("spiral", spiral(41, 150)))
    out.append(("maze", maze(rng, 37, 139)))
    out.append(("dots", dots(48, 130, period=6, size=3)))
    return out
