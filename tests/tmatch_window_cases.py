"""Shared cases of tests/test_tmatch_windows.py (emulator) and tests/test_gpu_tmatch_windows.py (MI355X):
gsh_match_template_windows_batch, gsh_locate_template_windows_batch and gsh_search_windows_batch against the oracle chain
gs_crop -> gs_match_template -> gs_find_best_match plus the window's origin, map by map and byte for byte.

`g` is a bound library, `mem` a parity_cases.Mem, `oracles` the CPU oracles that must all give the expected bytes (the C
restatement, and the compiled reference wherever oracle/_ref was built), as in tests/tmatch_bank_cases.py.

Every run (`run`): map slots, points and scores are pre-filled with 0x5a and sit inside larger buffers whose other bytes must
come back untouched; of a slot only the window's own map (row pitch rw_p) may change, of an invalid window nothing; img,
tmpl, windows and frame_of are compared with their copies afterwards.

The launcher's plan (gs_stencil.cpp: tm_win_form) is restated in `form`: the template is walked in bands of at most 256
columns and of as many rows as keep (31 + rows) staged image rows and the template's rows within 24 KB of LDS."""
import numpy as np

from geom_batch_cases import FILL, Guarded, sync
from tmatch_bank_cases import tuned
from tmatch_batch_cases import frames

INVALID = 0xFFFFFFFF


def form(tw, th):
    """(band rows, band columns) of k_tmatch_windows for a tw x th template"""
    cols = min(tw, 256)
    tpdw = (cols + 3) // 4
    ipdw = tpdw + 8
    ipdw += (8 - ipdw % 16) % 16
    assert ipdw % 16 == 8
    return min(th, (24 * 1024 // 4 - 31 * ipdw) // (ipdw + tpdw)), cols


def valid(win, f, n, iw, ih, tw, th, mw, mh):
    """the header's rule, in Python's unbounded integers"""
    x, y, w, h = (int(v) for v in win)
    return f < n and tw <= w <= mw and th <= h <= mh and x + w <= iw and y + h <= ih


_EXPECTED = {}


def expected(oracles, key, img, tmpl, windows, frame_of, max_size):
    """per window (map or None, (x, y) in frame coordinates, score) of the oracle chain; computed once per case"""
    if key not in _EXPECTED:
        n, ih, iw = img.shape
        th, tw = tmpl.shape[-2:]
        want = []
        for o in oracles:
            per = []
            for p, win in enumerate(windows):
                f = int(frame_of[p]) if frame_of is not None else p
                if not valid(win, f, n, iw, ih, tw, th, *max_size):
                    per.append((None, (INVALID, INVALID), 0))
                    continue
                x, y, w, h = (int(v) for v in win)
                m = o.match_template(o.crop(img[f], x, y, w, h), tmpl[p] if tmpl.ndim == 3 else tmpl)
                bx, by = o.find_best_match(m)
                per.append((m, (x + bx, y + by), int(m[by, bx])))
            want.append(per)
        for per in want[1:]:
            for a, b in zip(per, want[0]):
                assert a[1:] == b[1:] and (a[0] is None) == (b[0] is None) and (a[0] is None or np.array_equal(a[0], b[0])), \
                    "the oracles disagree on %s" % (key,)
        for m, (bx, by), s in want[0]:  # what the header says about a map of zeros
            assert m is None or (s == m.max() and (s > 0 or not m.any()))
        _EXPECTED[key] = want[0]
    return _EXPECTED[key]


def run_once(g, mem, want, img, tmpl, windows, frame_of, max_size, what):
    """the two entries on guarded buffers against `want` -> (slots (nwin, mrh * mrw), best (nwin, 2) u32, score (nwin))"""
    th, tw = tmpl.shape[-2:]
    nwin = len(windows)
    mrw, mrh = max_size[0] - tw + 1, max_size[1] - th + 1
    si, stp = Guarded(mem, img), Guarded(mem, tmpl, off=1)
    iv, tv = si.view(img.shape), stp.view(tmpl.shape)
    windows = np.ascontiguousarray(windows, np.uint32).reshape(nwin, 4)
    d_win = mem.put(windows)
    d_fo = mem.put(np.ascontiguousarray(frame_of, np.uint32)) if frame_of is not None else None
    res = Guarded(mem, np.full(nwin * mrh * mrw, FILL, np.uint8), off=2)
    g.match_template_windows_batch(res.view((nwin, mrh, mrw)), iv, tv, d_win, max_size, d_fo)
    slots = res.payload(what + ": maps").reshape(nwin, mrh * mrw)
    for p, (m, _, _) in enumerate(want):
        used = 0 if m is None else m.size
        if m is not None:
            got = slots[p, :used].reshape(m.shape)
            bad = np.argwhere(got != m)
            assert bad.size == 0, "%s: map %d %s: %d bytes differ, first at (y, x) = %s: got %d, expected %d" % (
                what, p, tuple(windows[p]), len(bad), tuple(bad[0]), got[tuple(bad[0])], m[tuple(bad[0])])
        assert (slots[p, used:] == FILL).all(), "%s: slot %d was written beyond its map" % (what, p)
    want_best = np.array([b for _, b, _ in want], np.uint32).reshape(nwin, 2)
    want_score = np.array([s for _, _, s in want], np.uint8)
    for with_score in (True, False):
        best, score = Guarded(mem, np.full(nwin * 8, FILL, np.uint8)), Guarded(mem, np.full(nwin, FILL, np.uint8), off=3)
        g.locate_template_windows_batch(iv, tv, d_win, max_size, best.view((nwin, 8)), score.view((nwin,)) if with_score else None, d_fo)
        lb, ls = best.payload(what).view(np.uint32).reshape(nwin, 2), score.payload(what)
        assert np.array_equal(lb, want_best), (what, "gsh_locate_template_windows_batch", lb, want_best)
        assert np.array_equal(ls, want_score if with_score else np.full(nwin, FILL, np.uint8)), (what, "score", ls, want_score)
    assert np.array_equal(si.payload(what).reshape(img.shape), img), what + ": img was written"
    assert np.array_equal(stp.payload(what).reshape(tmpl.shape), tmpl), what + ": tmpl was written"
    sync(mem)
    assert np.array_equal(np.asarray(mem.get(d_win)).view(np.uint32), windows), what + ": windows were written"
    assert d_fo is None or np.array_equal(np.asarray(mem.get(d_fo)).view(np.uint32), np.asarray(frame_of, np.uint32)), what + ": frame_of was written"
    return slots, want_best.copy(), want_score.copy()


def run(g, mem, oracles, key, img, tmpl, windows, frame_of, max_size, what):
    want = expected(oracles, key, img, tmpl, windows, frame_of, max_size)
    return run_once(g, mem, want, img, tmpl, windows, frame_of, max_size, what)


# ---- the cases -----------------------------------------------------------------------------------------------------------
def check_origins_and_phases(g, mem, oracles):
    """1: frames 200 and 199 wide (rows start at one phase / at all four), windows from x = 40, 41, 42, 43, windows on the right
    edge, the bottom edge and both, the whole frame, and a window of the template's size (one position)"""
    for iw in (200, 199):
        ih = 120
        img = frames(61, 2, ih, iw)
        tmpl = np.array(img[1, 30:37, 50:59])  # 9 x 7, inside the windows at x = 40 .. 43 of frame 1
        windows = [(40, 25, 30, 25), (41, 25, 30, 25), (42, 26, 30, 25), (43, 27, 30, 25),
                   (iw - 33, 10, 33, 20), (17, ih - 22, 40, 22), (iw - 31, ih - 19, 31, 19), (0, 0, iw, ih), (50, 60, 9, 7), (50, 30, 9, 7)]
        frame_of = [1, 1, 1, 1, 0, 1, 1, 1, 0, 1]  # the window on both edges lies in the LAST frame: its rows end with the batch
        _, best, score = run(g, mem, oracles, ("phases", iw), img, tmpl, windows, frame_of, (iw, ih), "origins and phases, %d columns" % iw)
        for p in (0, 1, 2, 3, 7, 9):
            assert tuple(best[p]) == (50, 30) and score[p] == 255, (p, best[p], score[p])
        assert tuple(best[8]) == (50, 60)  # one position: wherever the score is, it is the origin


TEMPLATE_SIZES = ((1, 1), (5, 3), (7, 1), (1, 9), (16, 16), (33, 17), (64, 64), (120, 100))


def check_template_sizes(g, mem, oracles):
    """2: every size on 200 x 120 frames, one window round a place the template was cut from and one on the frame's right and
    bottom edge.  120 x 100 forces the walk over template ROWS: its staged row is 40 dwords and its own row 30, so 24 KB hold
    (6144 - 31 * 40) / 70 = 70 template rows of the 100 (form).  260 x 5 on a 300 x 24 frame forces the walk over template
    COLUMNS, which no template that fits a 200-wide frame can: a band takes at most 256 columns."""
    assert form(120, 100) == (70, 120) and form(64, 64) == (64, 64) and form(260, 5) == (5, 256)
    for (iw, ih), sizes in (((200, 120), TEMPLATE_SIZES), ((300, 24), ((260, 5),))):
        img = frames(62, 2, ih, iw)
        for tw, th in sizes:
            x0, y0 = min(27, iw - tw), min(9, ih - th)
            tmpl = np.array(img[1, y0:y0 + th, x0:x0 + tw])
            wx, wy = max(0, x0 - 14), max(0, y0 - 5)
            w, h = min(tw + 40, iw - wx), min(th + 12, ih - wy)
            windows = [(wx, wy, w, h), (iw - w, ih - h, w, h), (wx, wy, w, h)]
            _, best, score = run(g, mem, oracles, ("sizes", iw, tw, th), img, tmpl, windows, [1, 1, 0], (w, h), "template %d x %d" % (tw, th))
            assert score[0] == 255 and (tw * th < 16 or tuple(best[0]) == (x0, y0))


def check_window_sizes(g, mem, oracles):
    """3: windows of 20 x 20 .. 96 x 80 under max 96 x 80 in one call (a 12 x 10 template: the largest map is 85 x 71 = 3 x 3
    tiles, the smallest 9 x 11 = one tile, whose other eight blocks leave), with one template for all and one per window"""
    img = frames(63, 3, 120, 200)
    windows = [(5, 7, 20, 20), (100, 40, 96, 80), (33, 3, 33, 47), (1, 90, 64, 21), (170, 2, 21, 64), (60, 30, 44, 80), (0, 0, 96, 10), (13, 13, 12, 10)]
    frame_of = [0, 1, 2, 0, 1, 2, 0, 1]
    per = np.stack([img[f, y + 3:y + 13, x + 2:x + 14] if w >= 14 and h >= 13 else img[f, y:y + 10, x:x + 12] for (x, y, w, h), f in zip(windows, frame_of)])
    _, best, score = run(g, mem, oracles, "sizes per window", img, per, windows, frame_of, (96, 80), "window sizes, a template per window")
    assert (score == 255).all()
    run(g, mem, oracles, "sizes one template", img, per[1], windows, frame_of, (96, 80), "window sizes, one template")


def check_frame_of(g, mem, oracles):
    """4: frame indices repeated and descending, three overlapping windows of one frame; and the NULL form (window p in frame p)"""
    img = frames(64, 4, 60, 90)
    tmpl = np.array(img[2, 20:28, 30:41])
    windows = [(20, 10, 40, 30), (25, 15, 40, 30), (22, 12, 30, 25), (0, 0, 40, 30), (50, 30, 40, 30), (20, 10, 40, 30)]
    _, best, score = run(g, mem, oracles, "frame_of", img, tmpl, windows, [2, 2, 2, 3, 1, 0], (40, 30), "frame_of")
    assert all(tuple(best[p]) == (30, 20) and score[p] == 255 for p in range(3))
    _, best, score = run(g, mem, oracles, "frame_of NULL", img, tmpl, windows[:4], None, (40, 30), "frame_of = NULL")
    assert score[2] == 255 and score[0] < 255


def check_ties_and_extremes(g, mem, oracles):
    """5: flat on flat (every score 255: the origin, 255), white on black (an all-zero map: the origin, 0 -- not the sentinel),
    and a template pasted at A = origin + (40, 2) and B = origin + (3, 20): A is the first in raster order, B lies in the tile
    column before A's"""
    img = np.array(frames(65, 3, 70, 110))
    img[0], img[1] = 77, 0
    tmpl = np.stack([np.full((8, 8), 77, np.uint8), np.full((8, 8), 255, np.uint8), np.array(frames(66, 1, 8, 8)[0])])
    wx, wy = 21, 9
    for x, y in ((wx + 40, wy + 2), (wx + 3, wy + 20)):
        img[2, y:y + 8, x:x + 8] = tmpl[2]
    windows = [(13, 11, 50, 40), (14, 12, 50, 40), (wx, wy, 60, 45)]
    slots, best, score = run(g, mem, oracles, "ties", img, tmpl, windows, None, (60, 45), "ties and extremes")
    assert [tuple(b) for b in best] == [(13, 11), (14, 12), (wx + 40, wy + 2)] and list(score) == [255, 0, 255]
    assert (slots[0, :43 * 33] == 255).all() and not slots[1, :43 * 33].any() and (slots[2, :53 * 38] == 255).sum() == 2


def check_invalid_windows(g, mem, oracles):
    """6: every kind of invalid window between valid ones: the sentinel, score 0, the slot untouched, the neighbours right"""
    n, ih, iw = 2, 60, 90
    img = frames(67, n, ih, iw)
    tmpl = np.array(img[1, 20:28, 30:38])
    ok = (20, 10, 40, 30)
    windows = [ok, (20, 10, 7, 30), (20, 10, 40, 7), ok, (0xFFFFFFF0, 10, 32, 30), (20, ih - 29, 40, 30), ok, ok, (20, 10, 41, 30),
               (20, 10, 0, 30), ok, (20, 0xFFFFFFF8, 40, 16)]
    frame_of = [1, 1, 1, 0, 1, 1, 1, n, 1, 1, 1, 1]
    want = expected(oracles, "invalid", img, tmpl, windows, frame_of, (40, 30))
    assert [m is not None for m, _, _ in want] == [True, False, False, True, False, False, True, False, False, False, True, False]
    _, best, score = run(g, mem, oracles, "invalid", img, tmpl, windows, frame_of, (40, 30), "invalid windows")
    for p, (m, _, _) in enumerate(want):
        assert (tuple(best[p]) == (INVALID, INVALID) and score[p] == 0) == (m is None)
    assert all(tuple(best[p]) == (30, 20) and score[p] == 255 for p in (0, 6, 10))


def check_window_split(g, mem, oracles):
    """7: five windows under gsh_tune key 8 = 0, 1, 2 and 3 (one launch; five; 2 + 2 + 1; 3 + 2): the same bytes"""
    img = frames(68, 2, 60, 90)
    windows = [(20, 10, 40, 30), (1, 2, 33, 21), (50, 30, 40, 30), (0, 0, 12, 9), (45, 17, 27, 30)]
    frame_of = [1, 0, 1, 0, 1]
    tmpl = np.stack([img[f, y:y + 9, x:x + 12] for (x, y, _, _), f in zip(windows, frame_of)])
    outs = []
    for key8 in (0, 1, 2, 3):
        with tuned(g, key8=key8):
            outs.append(run(g, mem, oracles, "split", img, tmpl, windows, frame_of, (40, 30), "window axis split, key 8 = %d" % key8))
    assert all(all(np.array_equal(a, b) for a, b in zip(outs[0], o)) for o in outs[1:])
    assert (outs[0][2] == 255).all()


def search_windows(at, bw, bh, mx, my, iw, ih):
    """the header's rule restated"""
    out = np.zeros((len(at), 4), np.uint32)
    for p, (x, y) in enumerate((int(a), int(b)) for a, b in at):
        if x >= iw or y >= ih:
            continue
        x0, y0 = max(x - mx, 0), max(y - my, 0)
        x1, y1 = min(x + bw + mx, iw), min(y + bh + my, ih)
        out[p] = (x0, y0, x1 - x0, y1 - y0)
    return out


def check_search_windows(g, mem, oracles):
    """8: interior points, points within the margin of every edge and corner, boxes that stick out of the frame, x = iw, y = ih,
    the sentinel, coordinates near 2^32, and margins of 0"""
    iw, ih = 200, 120
    at = np.array([(100, 60), (3, 60), (100, 2), (195, 60), (100, 117), (0, 0), (199, 119), (2, 118), (197, 1), (190, 110), (iw, 5), (5, ih),
                   (INVALID, INVALID), (0xFFFFFFF0, 4), (4, 0xFFFFFFF0), (6, 6)], np.uint32)
    for bw, bh, mx, my in ((16, 16, 6, 6), (16, 12, 0, 0), (32, 8, 6, 0), (1, 1, 300, 300), (16, 16, 0xFFFFFFFF, 3)):
        d_at = mem.put(at)
        out = Guarded(mem, np.full(len(at) * 16, FILL, np.uint8))
        g.search_windows_batch(d_at, (bw, bh), (mx, my), (iw, ih), out.view((len(at), 16)))
        got = out.payload("search windows").view(np.uint32).reshape(len(at), 4)
        assert np.array_equal(got, search_windows(at, bw, bh, mx, my, iw, ih)), (bw, bh, mx, my, got)
        assert np.array_equal(np.asarray(mem.get(d_at)).view(np.uint32), at)
    assert not got[10:15].any()  # outside the frame: no window
    g.search_windows_batch(d_at[0:0], (16, 16), (6, 6), (iw, ih), None)  # nwin == 0: nothing is checked


def check_against_crop_resize_and_locate(g, mem, oracles):
    """9: equal-sized windows: crop_resize_batch(nearest) at the window's own size (a copy) + locate_template_batch with a
    template per patch, plus the origins, is the new locate"""
    img = frames(69, 3, 120, 200)
    windows = np.array([(5, 7, 48, 40), (150, 80, 48, 40), (33, 3, 48, 40), (152, 0, 48, 40), (77, 41, 48, 40)], np.uint32)
    frame_of = np.array([0, 1, 2, 2, 0], np.uint32)
    tmpl = np.stack([img[(f + 1) % 3, y + 5:y + 21, x + 9:x + 25] for (x, y, _, _), f in zip(windows, frame_of)])  # from ANOTHER frame: scores below 255
    nwin = len(windows)
    d_img, d_t, d_win, d_fo = mem.put(img), mem.put(tmpl), mem.put(windows), mem.put(frame_of)
    patches, old_best, old_score = mem.zeros((nwin, 40, 48), fill=FILL), mem.zeros((nwin, 8), fill=FILL), mem.zeros((nwin,), fill=FILL)
    g.crop_resize_batch(patches, d_img, d_win, d_fo, nearest=True)
    g.locate_template_batch(patches, d_t, old_best, old_score)
    new_best, new_score = mem.zeros((nwin, 8), fill=FILL), mem.zeros((nwin,), fill=FILL)
    g.locate_template_windows_batch(d_img, d_t, d_win, (48, 40), new_best, new_score, d_fo)
    sync(mem)
    ob = np.asarray(mem.get(old_best)).view(np.uint32).reshape(nwin, 2) + windows[:, :2]
    nb = np.asarray(mem.get(new_best)).view(np.uint32).reshape(nwin, 2)
    assert np.array_equal(ob, nb), (ob, nb)
    assert np.array_equal(np.asarray(mem.get(old_score)), np.asarray(mem.get(new_score)))
    want = expected(oracles, "older path", img, tmpl, windows, frame_of, (48, 40))
    assert [b for _, b, _ in want] == [tuple(int(v) for v in b) for b in nb]


def check_nothing_to_do(g, mem, oracles):
    """nwin == 0 launches nothing and checks nothing (the NULL and zero-sized arguments would abort)"""
    b = mem.zeros((2, 8), fill=FILL)
    g.c.gsh_locate_template_windows_batch(None, 0, 0, 0, None, 0, 0, 7, None, None, 0, 0, 0, None, None)
    g.c.gsh_match_template_windows_batch(None, 0, 0, 0, None, 0, 0, 7, None, None, 0, 0, 0, None)
    g.c.gsh_search_windows_batch(None, 0, 0, 0, 0, 0, 0, 0, None)
    sync(mem)
    assert (np.asarray(mem.get(b)) == FILL).all()


ALL_CHECKS = (check_origins_and_phases, check_template_sizes, check_window_sizes, check_frame_of, check_ties_and_extremes,
              check_invalid_windows, check_window_split, check_search_windows, check_against_crop_resize_and_locate, check_nothing_to_do)
