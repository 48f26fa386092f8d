"""Shared pieces of tests/test_blob_paint.py (emulator), tests/test_gpu_blob_paint.py (MI355X) and
tests/test_gsbatch_blobs.py: a numpy restatement of the picture nanomagick's `blobs` verb draws, written from the rule
in include/grayskull_hip.h (gsh_blob_paint_batch), the largest-blob rule of its `scan` verb, and the cases both
back ends run.

The rule: the picture starts as zeros; record i < count marks, for y1 <= y <= y2 and x1 <= x <= x2 (both INCLUSIVE,
x1 = max(0, (int)x - 2), y1 = max(0, (int)y - 2), x2 = min(w, x + w_box + 2), y2 = min(h, y + h_box + 2) in wrapping
u32), the byte at linear index y * w + x with 128 -- so x == w lands on column 0 of the next row, and indices at or
past w * h are DROPPED (the reference writes outside its buffer there); then every pixel with img > 128 becomes 255."""
import numpy as np

import blob_cases as bc
from grayskull_amd import BLOB_DTYPE

U32 = 1 << 32


def spec_paint(img, recs, count):
    """-> (picture (h, w) uint8, sorted array of the dropped linear indices >= w * h)"""
    h, w = img.shape
    npx = h * w
    r = np.asarray(recs[:count])
    x, y = r["x"].astype(np.int64), r["y"].astype(np.int64)
    as_int = lambda v: np.where(v >= 1 << 31, v - U32, v)  # noqa: E731  the reference's (int) cast
    x1, y1 = np.maximum(0, as_int(x) - 2), np.maximum(0, as_int(y) - 2)
    x2 = np.minimum(w, (x + r["w"].astype(np.int64) + 2) % U32)
    y2 = np.minimum(h, (y + r["h"].astype(np.int64) + 2) % U32)
    keep = (x1 <= x2) & (y1 <= y2)
    x1, y1, x2, y2 = x1[keep], y1[keep], x2[keep], y2[keep]
    rows = y2 - y1 + 1
    # one span [y w + x1, y w + x2] per (record, row); a difference array over every index a span can reach
    which = np.repeat(np.arange(len(rows)), rows)
    ys = np.arange(int(rows.sum())) - np.repeat(np.cumsum(rows) - rows, rows) + y1[which]
    diff = np.zeros((h + 1) * w + w + 2, np.int64)
    np.add.at(diff, ys * w + x1[which], 1)
    np.add.at(diff, ys * w + x2[which] + 1, -1)
    covered = np.cumsum(diff) > 0
    out = np.where(covered[:npx], 128, 0).astype(np.uint8)
    out[img.reshape(-1) > 128] = 255
    return out.reshape(h, w), np.flatnonzero(covered[npx:]) + npx


def largest(recs, count):
    """ref nanomagick.c:196-199: index of the FIRST record of maximum area among the first `count` (count >= 1)"""
    best = 0
    for i in range(1, count):
        if recs[i]["area"] > recs[best]["area"]:
            best = i
    return best


def assert_label_order(recs, what=""):
    """records as gs_blobs leaves them: box.y never decreases (the paint kernel's early exit rests on it)"""
    y = np.asarray(recs["y"], np.int64)
    assert (np.diff(y) >= 0).all(), "%s: box.y decreases" % what


class Host:
    """emulator: "device" memory is host memory"""

    @staticmethod
    def put(a):
        return np.ascontiguousarray(a)

    @staticmethod
    def get(a):
        return np.asarray(a)

    @staticmethod
    def sync():
        pass


class Device:
    @staticmethod
    def put(a):
        import torch
        a = np.ascontiguousarray(a)
        if a.dtype == np.uint32:
            a = a.view(np.int32)
        if a.dtype == np.uint16:
            a = a.view(np.int16)
        return torch.from_numpy(a).cuda()

    @staticmethod
    def get(t):
        import torch
        torch.cuda.synchronize()
        a = t.cpu().numpy()
        return a.view(np.uint32) if a.dtype == np.int32 else a

    @staticmethod
    def sync():
        import torch
        torch.cuda.synchronize()


def pack(rec_lists, nblobs):
    """per-frame record arrays -> ((n, nblobs, 8) uint32 with garbage behind each frame's count, counts)"""
    n = len(rec_lists)
    blobs = np.full((n, nblobs, 8), 0xdeadbeef, np.uint32)  # records past the count must never be read as boxes
    counts = np.zeros(n, np.uint32)
    for f, r in enumerate(rec_lists):
        m = min(len(r), nblobs)
        blobs[f, :m] = np.asarray(r[:m]).view(np.uint32).reshape(m, 8)
        counts[f] = len(r)
    return blobs, counts


def paint(g, X, imgs, rec_lists, nblobs=None, fill=77):
    """gsh_blob_paint_batch on the frames `imgs` (n, h, w) with the given per-frame records -> (n, h, w) pictures; also
    asserts that nothing outside dst was written (guard frames before and after)"""
    imgs = np.ascontiguousarray(imgs)
    n, h, w = imgs.shape
    nblobs = nblobs or max(1, max(len(r) for r in rec_lists))
    blobs, counts = pack(rec_lists, nblobs)
    guard = np.full((n + 2, h, w), fill, np.uint8)
    d = X.put(guard)
    g.blob_paint_batch(d[1:n + 1], X.put(imgs), X.put(blobs), X.put(counts))
    out = X.get(d)
    assert (out[0] == fill).all() and (out[n + 1] == fill).all(), "written outside dst"
    return out[1:n + 1]


def check_against_spec(g, X, imgs, rec_lists, what, nblobs=None):
    imgs = np.ascontiguousarray(imgs)
    got = paint(g, X, imgs, rec_lists, nblobs)
    dropped = []
    for f in range(imgs.shape[0]):
        cnt = min(len(rec_lists[f]), nblobs or len(rec_lists[f]))
        assert_label_order(rec_lists[f][:cnt], what)
        want, drop = spec_paint(imgs[f], rec_lists[f], cnt)
        bad = np.flatnonzero(got[f].reshape(-1) != want.reshape(-1))
        assert bad.size == 0, "%s frame %d: %d bytes differ, first at %d: got %d, expected %d" % (
            what, f, bad.size, bad[0], got[f].reshape(-1)[bad[0]], want.reshape(-1)[bad[0]])
        dropped.append(drop)
    return got, dropped


def _blobs(g, img, cap):
    recs, _ = g.blobs(np.ascontiguousarray(img), cap)
    return recs


def mixed_mask(rng, h, w, density=0.25):
    """fg / bg with the values around both tests: gs_blobs takes >= 128, the picture > 128"""
    v = rng.choice(np.array([0, 90, 127, 128, 129, 255], np.uint8), size=(h, w), p=[(1 - density) / 3] * 3 + [density / 3] * 3)
    return v.astype(np.uint8)


SHAPES = ((1, 1), (5, 1), (1, 200), (7, 63), (9, 64), (33, 65), (40, 130), (70, 1000))
WIDE = (2, 66000)  # wider than the 65521 pixels whose coverage bits a block holds: the two-pass fallback


def check_hand_cases(g, X):
    W = 255
    # the clamp at 0: a blob in the top-left corner, box (0, 0, 2, 2) -> rows 0..4, columns 0..4
    img = np.zeros((12, 20), np.uint8)
    img[0:2, 0:2] = W
    got, drop = check_against_spec(g, X, img[None], [_blobs(g, img, 10)], "top-left")
    assert (got[0][:5, :5][img[:5, :5] == 0] == 128).all() and got[0][5, 0] == 0 and got[0][0, 5] == 0 and drop[0].size == 0

    # touching the right edge: x2 = w, so x == w marks column 0 of the row below, for every row of the box
    img = np.zeros((12, 20), np.uint8)
    img[3:5, 18:20] = W
    got, drop = check_against_spec(g, X, img[None], [_blobs(g, img, 10)], "right edge")
    assert (got[0][2:9, 0] == 128).all() and got[0][1, 0] == 0 and got[0][9, 0] == 0 and got[0][4, 1] == 0 and drop[0].size == 0

    # the bottom rows: y2 = h, row h is dropped whole
    img = np.zeros((12, 20), np.uint8)
    img[10:12, 5:8] = W
    got, drop = check_against_spec(g, X, img[None], [_blobs(g, img, 10)], "bottom")
    assert drop[0].tolist() == list(range(12 * 20 + 3, 12 * 20 + 11)) and (got[0][8:, 3:11][img[8:, 3:11] == 0] == 128).all()

    # the bottom-right corner: wrap and drop at once -- (h - 1, w) is index w h, the first one dropped; followed by a
    # black frame that must stay black (nothing leaks into frame f + 1)
    img = np.zeros((12, 20), np.uint8)
    img[10:12, 18:20] = W
    both = np.stack([img, np.zeros_like(img)])
    got, drop = check_against_spec(g, X, both, [_blobs(g, img, 10), _blobs(g, both[1], 10)], "bottom-right")
    assert drop[0][0] == 12 * 20 and not got[1].any() and got[0][11, 0] == 128 and got[0][9, 0] == 128

    # overlapping padded boxes
    img = np.zeros((16, 40), np.uint8)
    img[2:6, 3:9] = W
    img[7:12, 10:14] = W
    img[4:5, 11:30] = W
    check_against_spec(g, X, img[None], [_blobs(g, img, 10)], "overlap")

    # a foreground pixel of exactly 128: fg for gs_blobs, not for the picture -- 128 inside its box, never 255
    img = np.zeros((9, 30), np.uint8)
    img[4, 10:13] = 128
    img[4, 13] = 129
    got, _ = check_against_spec(g, X, img[None], [_blobs(g, img, 10)], "value 128")
    assert got[0][4, 10:14].tolist() == [128, 128, 128, 255]

    # a capped frame: start pixels beyond nblobs get no record, their pixels lie outside every box and are still 255;
    # the 128-valued pixel out there stays 0
    img = np.zeros((30, 50), np.uint8)
    img[1:3, 1:3] = W
    img[20:22, 40:42] = W
    img[25, 10] = 128
    recs = _blobs(g, img, 1)
    assert len(recs) == 1
    got, _ = check_against_spec(g, X, img[None], [recs], "capped")
    assert (got[0][20:22, 40:42] == 255).all() and got[0][19, 40] == 0 and got[0][25, 10] == 0

    # a frame-filling blob and a ring around the frame: one record whose box is the whole frame (a wave shares its spans)
    full = np.full((37, 150), 200, np.uint8)
    full[::5, ::7] = 128
    ring = np.zeros((37, 150), np.uint8)
    ring[0], ring[-1], ring[:, 0], ring[:, -1] = W, W, W, W
    ring[10:12, 40:44] = W
    for rows in (0, 1, 5):
        g.tune(0, rows)
        try:
            for name, img in (("full", full), ("ring", ring)):
                recs = _blobs(g, img, 10)
                got, drop = check_against_spec(g, X, img[None], [recs], "%s, band rows %d" % (name, rows))
                assert int(recs[0]["w"]) == 150 and int(recs[0]["h"]) == 37 and drop[0].size == 151 and not (got[0] == 0).any()
        finally:
            g.tune(0, 0)

    # count 0: only the > 128 overlay
    img = np.full((9, 33), 128, np.uint8)
    img[2, 3] = 200
    got = paint(g, X, img[None], [np.zeros(0, BLOB_DTYPE)], nblobs=4)
    assert got[0][2, 3] == 255 and np.count_nonzero(got[0]) == 1


def check_shapes(g, X, shapes=SHAPES + (WIDE,), band_rows=(0, 1, 3)):
    """random frames of every shape, records from the library's own gs_blobs (pinned to the reference by
    tests/test_blobs.py / test_gpu_blobs.py), whole and capped; gsh_tune key 0 forces bands of 1 and 3 rows so that the
    small shapes, too, are cut into several blocks"""
    rng = np.random.default_rng(77)
    for (h, w) in shapes:
        img = mixed_mask(rng, h, w, 0.3 if w * h < 20000 else 0.02)
        if h * w > 1:
            img[h - 1, w - 1] = 255  # a box that reaches the bottom-right corner: the wrap and the drop
        for cap in (3, 150):
            recs = _blobs(g, img, cap)
            for rows in band_rows:
                g.tune(0, rows)
                try:
                    check_against_spec(g, X, img[None], [recs], "%dx%d cap %d band rows %d" % (w, h, cap, rows), nblobs=cap)
                finally:
                    g.tune(0, 0)


def check_batches(g, X):
    """n = 3 with different counts (one of them 0); frames per launch 1 splits the batch; frame f never touches f + 1"""
    rng = np.random.default_rng(5)
    h, w = 21, 75
    imgs = np.stack([mixed_mask(rng, h, w, 0.06), np.zeros((h, w), np.uint8), mixed_mask(rng, h, w, 0.02)])
    imgs[0, h - 2:, w - 3:] = 255  # frame 0 drops indices; frame 1 (black, count 0) must stay black
    recs = [_blobs(g, imgs[f], 150) for f in range(3)]
    assert len({len(r) for r in recs}) == 3 and len(recs[1]) == 0
    outs = []
    for fpl in (0, 1):
        g.tune(8, fpl)
        try:
            got, drop = check_against_spec(g, X, imgs, recs, "batch, frames per launch %d" % fpl, nblobs=150)
        finally:
            g.tune(8, 0)
        assert drop[0].size > 0 and not got[1].any()
        outs.append(got)
    assert np.array_equal(outs[0], outs[1])


def run_largest(g, X, blobs, counts, with_index=True):
    n = blobs.shape[0]
    out = X.put(np.full((n, 8), 0x55555555, np.uint32))
    idx = X.put(np.full(n, 0x55555555, np.uint32)) if with_index else None
    g.blob_largest_batch(X.put(blobs), X.put(counts), out, idx)
    return X.get(out), (X.get(idx) if with_index else None)


def check_largest(g, X):
    rng = np.random.default_rng(1)
    for nblobs in (1, 7, 64, 300, 5000):  # one wave per frame up to 4096 records, a block of four beyond
        n = 6
        blobs = rng.integers(0, 1 << 32, (n, nblobs, 8), dtype=np.uint64).astype(np.uint32)
        blobs[:, :, 1] = rng.integers(0, 50, (n, nblobs))  # few distinct areas: ties everywhere
        if nblobs > 4:
            blobs[2, :, 1] = 9  # all tie: the first wins
            blobs[3, nblobs - 1, 1] = 0xffffffff  # the maximum in the last record, area beyond 2^31
        counts = np.array([0, 1, nblobs, nblobs, nblobs + 17, max(1, nblobs // 2)], np.uint32)
        got, idx = run_largest(g, X, blobs, counts)
        g.tune(8, 2)  # frames per launch: three launches
        try:
            split, split_idx = run_largest(g, X, blobs, counts)
        finally:
            g.tune(8, 0)
        assert np.array_equal(got, split) and np.array_equal(idx, split_idx)
        recs = blobs.view(BLOB_DTYPE).reshape(n, nblobs)
        for f in range(n):
            c = min(int(counts[f]), nblobs)
            if c == 0:
                assert not got[f].any() and idx[f] == 0xffffffff
            else:
                k = largest(recs[f], c)
                assert idx[f] == k and np.array_equal(got[f], blobs[f, k]), (nblobs, f, int(idx[f]), k)
        got2, _ = run_largest(g, X, blobs, counts, with_index=False)
        assert np.array_equal(got, got2)


def check_threshold_offset(g, X):
    rng = np.random.default_rng(2)
    imgs = rng.integers(0, 256, (5, 13, 37), dtype=np.uint8)
    thr = np.array([0, 100, 250, 253, 3], np.uint8)
    a, b = X.put(imgs.copy()), X.put(imgs.copy())
    g.threshold_batch(a, X.put(thr))
    g.threshold_batch_dev_offset(b, X.put(thr), 0)
    assert np.array_equal(X.get(a), X.get(b))
    for off in (10, -3, 256, -300):
        d, t = X.put(imgs.copy()), X.put(thr.copy())
        g.threshold_batch_dev_offset(d, t, off)
        want = np.stack([np.where(imgs[f] > ((int(thr[f]) + off) & 255), 255, 0) for f in range(5)]).astype(np.uint8)
        assert np.array_equal(X.get(d), want), off
        assert np.array_equal(X.get(t), thr)  # thr is not modified
    assert (250 + 10) & 255 == 4  # the wrap the issue names: frame 2 at offset 10 thresholds at 4
