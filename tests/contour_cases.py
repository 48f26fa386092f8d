"""Shared pieces of tests/test_contours.py (emulator) and tests/test_gpu_contours.py (MI355X): a plain-Python
restatement of gs_trace_contour (ref grayskull.h:446-480, statement for statement) that also DECIDES whether the
reference's walk ends, the reference's compiled function over ctypes, input families and comparison helpers.

The reference's walk does not end on many ordinary inputs (a state (p, dir, seenstart) repeats and the stop test is
never passed again).  So the compiled reference is only ever called on a case the restatement has shown to end:
Ref.trace asserts that first.  Everything else would hang the test run."""
import ctypes as C

import numpy as np

from grayskull_amd import CONTOUR_DTYPE
from grayskull_amd._abi import GsImage

U32 = 0xFFFFFFFF
DX = (1, 1, 0, -1, -1, -1, 0, 1)
DY = (0, 1, 1, 1, 0, -1, -1, -1)
W = 255
ENDED, ENDLESS, CAPPED = 0, 1, 2

# ref test.c:261-287: the reference's own unit test: image, start, and the results it asserts
TEST_C_IMAGE = np.array([[0, W, W, W, 0],
                         [0, W, W, W, 0],
                         [0, W, 0, W, W],
                         [0, W, W, W, 0],
                         [0, 0, W, 0, W]], np.uint8)
TEST_C_VISITED = np.array([[0, W, W, W, 0],
                           [0, W, 0, W, 0],
                           [0, W, 0, 0, W],
                           [0, W, 0, W, 0],
                           [0, 0, W, 0, 0]], np.uint8)
TEST_C_START, TEST_C_LENGTH, TEST_C_BOX = (1, 0), 10, (1, 0, 4, 5)
# the smallest input found on which the reference never returns: start (0, 0), the walk circles (1,3) (1,4) (0,4)
ENDLESS_EXAMPLE = np.array([[W, W], [W, 0], [W, 0], [0, W], [W, W]], np.uint8)  # start (0, 0) never ends


def _s32(v):
    """unsigned -> int, as the reference's `int nx = p.x + dx[d]` converts"""
    v &= U32
    return v - (1 << 32) if v & 0x80000000 else v


class Tracer:
    """ref :446-480 on Python ints for one image, deciding exactly whether the walk ends.  The walk is a deterministic
    map on the states (p, dir, seenstart); a bitmap of 16 bits per pixel remembers every state met, so the first
    repeat is found exactly.  From there the reference goes round the same cycle for ever: length and visited are
    final (every pixel of the cycle has been marked), box.x / box.y are final, and one more trip round the cycle --
    until the repeated state comes up again -- gives box.w / box.h the values they keep."""

    def __init__(self, img):
        self.h, self.w = img.shape
        self.px = np.ascontiguousarray(img).tobytes()
        self.seen_states = bytearray(2 * self.w * self.h)

    def trace(self, vis, start):
        """the walk from `start`, marking the (h, w) uint8 array `vis` IN PLACE -> (length, box, status, moves, marked):
        `moves` up to the stop or the first repeat, `marked` the flat indices of the pixels set to 255"""
        w, h, img, states = self.w, self.h, self.px, self.seen_states
        v = memoryview(vis).cast("B")
        sx, sy = int(start[0]) & U32, int(start[1]) & U32
        length = moves = 0
        bx, by, bw, bh = sx, sy, 1, 1
        px, py, dr, seen = sx, sy, 7, 0
        status, repeat = ENDED, None
        touched, marked = [], []
        while True:
            inside = px < w and py < h
            if inside:
                key = (py * w + px) * 16 + dr * 2 + seen
                if repeat is None:
                    if states[key >> 3] >> (key & 7) & 1:
                        status, repeat = ENDLESS, key
                    else:
                        states[key >> 3] |= 1 << (key & 7)
                        touched.append(key >> 3)
                elif key == repeat:
                    break
                if v[py * w + px] == 0:
                    length += 1
                v[py * w + px] = 255
                marked.append(py * w + px)
            else:
                length += 1  # gs_get outside the image: 0; gs_set: nothing
            for i in range(8):
                d = (dr + 1 + i) & 7
                nx, ny = _s32(px + DX[d]), _s32(py + DY[d])
                if 0 <= nx < w and 0 <= ny < h and img[ny * w + nx] > 128:
                    break
            else:
                break
            px, py, dr = nx, ny, (d + 6) & 7
            if repeat is None:
                moves += 1
            bx, by = min(bx, px), min(by, py)
            bw, bh = max(bw, (px - bx + 1) & U32), max(bh, (py - by + 1) & U32)
            if repeat is None and px == sx and py == sy:
                if seen:
                    break
                seen = 1
        for k in touched:
            states[k] = 0
        return length & U32, (bx, by, bw, bh), status, moves, marked


def spec_trace(img, visited, start):
    """-> (length, (x, y, w, h), visited', status, moves); `visited` is not modified (see Tracer)"""
    vis = np.array(visited, np.uint8, copy=True)
    length, box, status, moves, _ = Tracer(img).trace(vis, start)
    return length, box, vis, status, moves


def tile_reloads(img, start, tile=64, origin=None):
    """(re)loads of the kernel's `tile` x `tile` window on the walk from `start` (ended walks only) -> (reloads, moves,
    origin): the window is centred on p whenever p reaches its outermost rows / columns, and outlives a contour
    (`origin`: where the previous contour of the frame left it)"""
    h, w = img.shape
    flat = np.ascontiguousarray(img).tobytes()
    px, py, dr, seen = int(start[0]), int(start[1]), 7, 0
    reloads = moves = 0
    while True:
        if origin is None or not (1 <= px - origin[0] <= tile - 2 and 1 <= py - origin[1] <= tile - 2):
            origin, reloads = (px - tile // 2, py - tile // 2), reloads + 1
        for i in range(8):
            d = (dr + 1 + i) % 8
            nx, ny = px + DX[d], py + DY[d]
            if 0 <= nx < w and 0 <= ny < h and flat[ny * w + nx] > 128:
                break
        else:
            return reloads, moves, origin
        px, py, dr, moves = nx, ny, (d + 6) % 8, moves + 1
        if (px, py) == (int(start[0]), int(start[1])):
            if seen:
                return reloads, moves, origin
            seen = 1


class Ref:
    """the compiled, unmodified reference header (oracle/_ref/libgs_ref.so)"""

    def __init__(self):
        from oracle.pyoracle import REF_SO
        L = self.L = C.CDLL(REF_SO)
        L.gs_trace_contour.restype = None
        L.gs_trace_contour.argtypes = [GsImage, GsImage, C.c_void_p]
        L.gs_blobs.restype = C.c_uint
        L.gs_blobs.argtypes = [GsImage, C.c_void_p, C.c_void_p, C.c_uint]

    def trace(self, img, visited, start, status=None):
        """gs_trace_contour on `visited` IN PLACE -> (length, box).  Only for walks that end: `status` is what the
        restatement found for this very call (None: it is run here first, on a copy) -- the reference itself would
        never come back from an endless walk."""
        assert img.dtype == np.uint8 and visited.dtype == np.uint8 and img.flags.c_contiguous and visited.flags.c_contiguous
        if status is None:
            status = spec_trace(img, visited, start)[3]
        assert status == ENDED, "the reference does not return from this walk (start %s)" % (start,)
        c = np.zeros(1, CONTOUR_DTYPE)
        c["sx"], c["sy"] = int(start[0]) & U32, int(start[1]) & U32
        self.L.gs_trace_contour(GsImage(img.shape[1], img.shape[0], img.ctypes.data),
                                GsImage(visited.shape[1], visited.shape[0], visited.ctypes.data), c.ctypes.data)
        return rec_tuple(c[0])


def rec_tuple(r):
    """CONTOUR_DTYPE record -> (length, box)"""
    return int(r["length"]), (int(r["x"]), int(r["y"]), int(r["w"]), int(r["h"]))


# ---- start pixels and expected results of a whole frame ---------------------------------------------------------------
def start_pixels(img):
    """foreground (> 128) pixels whose left and top neighbours are not foreground, in raster order, as (x, y)"""
    fg = img > 128
    left = np.zeros_like(fg)
    left[:, 1:] = fg[:, :-1]
    top = np.zeros_like(fg)
    top[1:] = fg[:-1]
    ys, xs = np.nonzero(fg & ~left & ~top)
    return [(int(x), int(y)) for x, y in zip(xs, ys)]


def sampled_starts(img, budget, floor=12, probes=16):
    """start pixels of `img` in raster order for one shared visited plane: all of them where their walks fit `budget`
    moves, else every k-th, spread over the whole frame -> (starts, number of start pixels in the frame).
    Above the percolation threshold (x2 / x3 noise at density 0.55 is, for 8-connected walks) one cluster spans the
    frame and every start pixel on its rim walks that whole rim -- about 70 000 moves each at 3840 x 2160, against some
    10^5 start pixels: 10^9 moves and more per frame, hours for the restatement that must decide every walk before
    the reference may be called.  k comes from the mean walk of `probes` start pixels spread over the frame, each
    traced alone.  At least min(floor, all) start pixels are kept whatever the budget says."""
    every = start_pixels(img)
    if len(every) <= floor:
        return every, len(every)
    tracer = Tracer(img)
    probe = every[::max(1, len(every) // probes)][:probes]
    mean = max(1.0, sum(tracer.trace(np.zeros(img.shape, np.uint8), s)[3] for s in probe) / len(probe))
    want = max(floor, int(budget / mean))
    k = max(1, -(-len(every) // want))
    out = every[::k]
    assert len(out) >= min(floor, len(every))
    return out, len(every)


def expected_sequence(img, starts, ref=None, visited=None):
    """the contours from `starts`, traced one after the other on one visited plane -> ([(length, box, status)], visited,
    number of endless ones).  With `ref`, every walk the restatement finds to end is also run through the compiled
    reference, on a plane of its own that takes the restatement's marks for the endless ones, and must agree."""
    img = np.ascontiguousarray(img)
    vis = np.zeros(img.shape, np.uint8) if visited is None else np.array(visited, np.uint8, copy=True)
    rvis = vis.copy() if ref is not None else None
    tracer = Tracer(img)
    out, endless = [], 0
    for s in starts:
        length, box, status, _, marked = tracer.trace(vis, s)
        if ref is not None:
            if status == ENDED:
                assert ref.trace(img, rvis, s, status=status) == (length, box), "restatement and reference differ at %s" % (s,)
            else:
                rvis.reshape(-1)[marked] = 255
        endless += status != ENDED
        out.append((length, box, status))
    if ref is not None:
        assert np.array_equal(vis, rvis), "restatement and reference differ in visited"
    return out, vis, endless


# ---- input families -----------------------------------------------------------------------------------------------
def upscaled_noise(rng, h, w, k, density=0.55):
    """a random mask of density `density`, every pixel blown up to k x k (np.kron), cropped to (h, w)"""
    small = (rng.random(((h + k - 1) // k, (w + k - 1) // k)) < density).astype(np.uint8)
    return (np.kron(small, np.ones((k, k), np.uint8))[:h, :w] * 255).astype(np.uint8)


def discs(h, w, centres_radii):
    img = np.zeros((h, w), np.uint8)
    for cx, cy, r in centres_radii:
        xa, xb, ya, yb = max(cx - r, 0), min(cx + r + 1, w), max(cy - r, 0), min(cy + r + 1, h)
        if xa < xb and ya < yb:
            yy, xx = np.mgrid[ya:yb, xa:xb]
            img[ya:yb, xa:xb][(xx - cx) ** 2 + (yy - cy) ** 2 <= r * r] = 255
    return img


def random_discs(rng, h, w, n, rmin=3, rmax=20):
    return discs(h, w, [(int(rng.integers(0, w)), int(rng.integers(0, h)), int(rng.integers(rmin, rmax + 1))) for _ in range(n)])


def disc_grid_centres(h, w, nx, ny):
    return [(int((i + 0.5) * w / nx), int((j + 0.5) * h / ny)) for j in range(ny) for i in range(nx)]


def disc_grid(h, w, nx, ny, r):
    """nx x ny separate filled discs of radius r on a regular grid"""
    return discs(h, w, [(cx, cy, r) for cx, cy in disc_grid_centres(h, w, nx, ny)])


def random_rects(rng, h, w, n, smin=2, smax=30):
    img = np.zeros((h, w), np.uint8)
    for _ in range(n):
        x, y = int(rng.integers(0, w)), int(rng.integers(0, h))
        img[y:y + int(rng.integers(smin, smax + 1)), x:x + int(rng.integers(smin, smax + 1))] = 255
    return img


def random_mask(rng, h, w, density):
    return np.where(rng.random((h, w)) < density, 255, 0).astype(np.uint8)


# ---- the library side -------------------------------------------------------------------------------------------------
def lib_sequence_dropin(g, img, starts, visited=None):
    """the same sequence of drop-in calls on the library `g` with host pointers -> ([(length, box)], visited)"""
    vis = np.zeros(img.shape, np.uint8) if visited is None else visited.copy()
    return [rec_tuple(g.trace_contour(img, vis, s)) for s in starts], vis


def assert_sequence_equal(got, got_vis, want, want_vis, what="", got_status=None):
    assert len(got) == len(want), what
    for k, (g_, w_) in enumerate(zip(got, want)):
        assert g_[0] == w_[0], "%s: contour %d: length %d, expected %d" % (what, k, g_[0], w_[0])
        assert tuple(g_[1]) == tuple(w_[1]), "%s: contour %d: box %s, expected %s" % (what, k, g_[1], w_[1])
        if got_status is not None:
            assert int(got_status[k]) == w_[2], "%s: contour %d: status %d, expected %d" % (what, k, int(got_status[k]), w_[2])
    assert np.array_equal(got_vis, want_vis), "%s: visited differs at %d pixels" % (what, int(np.count_nonzero(got_vis != want_vis)))
