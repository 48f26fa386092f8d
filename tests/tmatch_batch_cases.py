"""Shared cases of tests/test_tmatch_batch.py (emulator) and tests/test_gpu_tmatch_batch.py (MI355X):
gsh_match_template_batch, gsh_find_best_match_batch and gsh_locate_template_batch against the oracle's gs_match_template /
gs_find_best_match, frame by frame and byte for byte.

`g` is a bound library, `mem` a parity_cases.Mem ("host": the emulator takes host memory for device memory; "device":
torch CUDA tensors), `oracles` the CPU oracles that must all give the expected bytes (the C restatement, and the compiled
reference wherever oracle/_ref was built).

Every run (`run`): the frames of a batch all differ; result, best and score are pre-filled with 0x5a and sit inside larger
buffers whose other bytes must come back untouched; img and tmpl are compared with their copies afterwards.  One run
makes the three calls -- maps, best of the maps, locate -- and compares all of them with the oracle, so every case also
shows that locate equals match-then-find on its route; `without_score` repeats the last two with score = NULL.

The launcher's rule (gs_stencil.cpp: tm_route, tm_form, tm_chunk_frames) is restated in `plan`, so that every case can say
which kernel and which tile form it takes:
  route   of ONE frame's geometry: the matrix cores for templates 16 .. 257 wide, at least 4 high, of 512 .. 32768 taps
          (from any number of taps under key 20 = 2, 3, 8) whose block fits 150 KiB of LDS; else the dot-product kernels
          up to kTmplTile - 3 = 16381 columns -- four results per thread when the frame width is a multiple of 4 --, else
          the per-pixel kernel
  form    of the matrix-core kernel: 32 x 64 "split" tiles while the launch has fewer than 512 blocks of 64 x 128 --
          tiles per frame times the frames of the launch (a chunk) --, else whole 64 x 128 tiles, "banded" for templates
          higher than 32 rows.  key 20 = 2: whole, 3: split, 8: whole and banded where the template is high enough."""
import contextlib
import functools

import numpy as np

from geom_batch_cases import FILL, Guarded, sync

BAND, TMPL_TILE, LDS_MAX, BLOCKS = 32, 16384, 150 * 1024, 512


def form(tw, th, rw, rh, frames, key20=0):
    """(name, bytes of LDS) of k_match_template_mfma for a launch of `frames` frames"""
    nkc = (tw + 62) // 32
    split = key20 == 3 or (key20 not in (2, 8) and ((rw + 127) // 128) * ((rh + 63) // 64) * frames < BLOCKS)
    band = not split and key20 != 2 and th > BAND
    rows = BAND if band else th
    lds = max(((31 if split else 63) + rows) * ((32 if split else 96) + 32 * nkc + 16) + rows * (32 * nkc + 48) + 16, 32768 if split else 0)
    return ("split" if split else "band" if band else "whole"), lds


def plan(iw, ih, tw, th, frames, key20=0):
    """the kernel a launch of `frames` frames of iw x ih takes: "whole" / "split" / "band" (k_match_template_mfma), "dot4"
    (k_match_template4), "dot" (k_match_template), "px" (k_match_template_px)"""
    rw, rh, taps, nkc = iw - tw + 1, ih - th + 1, tw * th, (tw + 62) // 32
    if (key20 != 1 and tw >= 16 and nkc <= 9 and th >= 4 and (taps >= 512 or key20 in (2, 3, 8)) and taps <= 32768
            and form(tw, th, rw, rh, 1, key20)[1] <= LDS_MAX and iw * ih < 0x7fffffff):
        name, lds = form(tw, th, rw, rh, frames, key20)
        return name if lds <= LDS_MAX else form(tw, th, rw, rh, 1, key20)[0]
    if tw > TMPL_TILE - 3:
        return "px"
    return "dot4" if iw % 4 == 0 else "dot"


@functools.lru_cache(maxsize=None)
def frames(seed, n, h, w):
    """n different frames of noise"""
    a = np.random.default_rng(seed).integers(0, 256, (n, h, w), dtype=np.uint8)
    a.setflags(write=False)
    return a


@contextlib.contextmanager
def tuned(g, key20=0, key26=0):
    try:
        g.tune(20, key20), g.tune(26, key26)
        yield
    finally:
        g.tune(20, 0), g.tune(26, 0)


_EXPECTED = {}


def expected(oracles, key, img, tmpl):
    """(maps, best (n, 2), score (n)) of the oracles, computed once per case and shared by every back end, key and schedule"""
    if key not in _EXPECTED:
        per_frame = tmpl.ndim == 3
        want = []
        for o in oracles:
            maps = np.stack([o.match_template(f, tmpl[i] if per_frame else tmpl) for i, f in enumerate(img)])
            best = np.array([o.find_best_match(m) for m in maps], np.uint32).reshape(-1, 2)
            want.append((maps, best))
        for maps, best in want[1:]:
            assert np.array_equal(maps, want[0][0]) and np.array_equal(best, want[0][1]), "the oracles disagree on %s" % (key,)
        maps, best = want[0]
        score = np.array([m[y, x] for m, (x, y) in zip(maps, best)], np.uint8)
        for m, b, s in zip(maps, best, score):  # what the header says about a map of zeros
            assert s == m.max() and (s > 0 or (tuple(b) == (0, 0) and not m.any()))
        for a in (maps, best, score):
            a.setflags(write=False)
        _EXPECTED[key] = (maps, best, score)
    return _EXPECTED[key]


def _same_maps(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%s: %d bytes differ, first at (f, y, x) = %s: got %d, expected %d" % (
        what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def run(g, mem, oracles, key, img, tmpl, what, without_score=False):
    """the three entries on guarded buffers against the oracle -> (maps, best, score) as the library gave them"""
    n, ih, iw = img.shape
    th, tw = tmpl.shape[-2:]
    rh, rw = ih - th + 1, iw - tw + 1
    want_maps, want_best, want_score = expected(oracles, key, img, tmpl)
    si, stp = Guarded(mem, img), Guarded(mem, tmpl, off=1)
    iv, tv = si.view(img.shape), stp.view(tmpl.shape)

    def outputs():
        return (Guarded(mem, np.full(n * 8, FILL, np.uint8)), Guarded(mem, np.full(n, FILL, np.uint8), off=3))

    def points(b):
        return b.payload(what).view(np.uint32).reshape(n, 2)

    res = Guarded(mem, np.full(n * rh * rw, FILL, np.uint8), off=2)
    g.match_template_batch(res.view((n, rh, rw)), iv, tv)
    maps = res.payload(what + ": maps").reshape(n, rh, rw)
    _same_maps(maps, want_maps, what + ": gsh_match_template_batch")
    best, score = outputs()
    g.find_best_match_batch(res.view((n, rh, rw)), best.view((n, 8)), score.view((n,)))
    fb, fs = points(best), score.payload(what)
    assert np.array_equal(fb, want_best) and np.array_equal(fs, want_score), (what, "gsh_find_best_match_batch", fb, want_best, fs, want_score)
    assert np.array_equal(res.payload(what).reshape(n, rh, rw), want_maps), what + ": find_best_match_batch wrote its input"
    best, score = outputs()
    g.locate_template_batch(iv, tv, best.view((n, 8)), score.view((n,)))
    lb, ls = points(best), score.payload(what)
    assert np.array_equal(lb, want_best) and np.array_equal(ls, want_score), (what, "gsh_locate_template_batch", lb, want_best, ls, want_score)
    if without_score:  # score = NULL: the points alone
        best, _ = outputs()
        g.locate_template_batch(iv, tv, best.view((n, 8)))
        assert np.array_equal(points(best), want_best), what + ": locate, score = None"
        best, _ = outputs()
        g.find_best_match_batch(res.view((n, rh, rw)), best.view((n, 8)))
        assert np.array_equal(points(best), want_best), what + ": find, score = None"
    assert np.array_equal(si.payload(what).reshape(img.shape), img), what + ": img was written"
    assert np.array_equal(stp.payload(what).reshape(tmpl.shape), tmpl), what + ": tmpl was written"
    return maps, lb, ls


# ---- the cases -----------------------------------------------------------------------------------------------------------
def small_frames():
    """three frames of 150 x 100 and a 16 x 32 template cut from frame 1 at (70, 37): 512 taps, nkc = 2, result 135 x 69 -- two
    ragged column tiles and two row tiles of a 64 x 128 block, 3 x 3 tiles of 32 x 64"""
    img = frames(11, 3, 100, 150)
    return img, np.ascontiguousarray(img[1, 37:69, 70:86])


def check_whole_tiles(g, mem, oracles):
    """1: key 20 = 2, 64 x 128 tiles"""
    img, tmpl = small_frames()
    assert plan(150, 100, 16, 32, 3, key20=2) == "whole" and plan(150, 100, 16, 32, 3) == "split"
    with tuned(g, key20=2):
        _, best, score = run(g, mem, oracles, "small", img, tmpl, "whole tiles", without_score=True)
    assert tuple(best[1]) == (70, 37) and score[1] == 255


def check_split_and_banded(g, mem, oracles):
    """2: the same frames on 32 x 64 tiles (key 20 = 3); a 20 x 40 template on 160 x 110 taken 32 rows at a time (key 20 = 8)"""
    img, tmpl = small_frames()
    assert plan(150, 100, 16, 32, 3, key20=3) == "split"
    with tuned(g, key20=3):
        run(g, mem, oracles, "small", img, tmpl, "split tiles")
    img = frames(12, 3, 110, 160)
    tmpl = np.ascontiguousarray(img[2, 50:90, 101:121])
    assert plan(160, 110, 20, 40, 3, key20=8) == "band" and plan(160, 110, 20, 40, 3) == "split"
    with tuned(g, key20=8):
        _, best, score = run(g, mem, oracles, "banded", img, tmpl, "banded tiles")
    assert tuple(best[2]) == (101, 50) and score[2] == 255


def check_default_rules_few_blocks(g, mem, oracles):
    """3, the side below 512 blocks: no key set, three frames of 4 whole tiles each take the split form; 8 x 8 templates (64
    taps) take the dot-product kernels whatever the number of frames"""
    img, tmpl = small_frames()
    assert plan(150, 100, 16, 32, 3) == "split" and plan(150, 100, 16, 32, 127) == "split" and plan(150, 100, 16, 32, 128) == "whole"
    run(g, mem, oracles, "small", img, tmpl, "default rule, 12 blocks")
    img = frames(13, 5, 33, 44)
    assert plan(44, 33, 8, 8, 5) == "dot4"
    run(g, mem, oracles, "8x8", img, np.ascontiguousarray(img[3, 20:28, 30:38]), "default rule, 8 x 8")


def check_per_frame_templates(g, mem, oracles):
    """4: template f is cut from frame f at a place of its own, so frame f's best point is that place, with score 255"""
    img, _ = small_frames()
    at = ((5, 60), (130, 2), (66, 33))  # (x, y): the tiles' corners and middle
    tmpl = np.stack([img[f, y:y + 32, x:x + 16] for f, (x, y) in enumerate(at)])
    for key20 in (2, 3):
        with tuned(g, key20=key20):
            _, best, score = run(g, mem, oracles, "per-frame", img, tmpl, "per-frame templates, key 20 = %d" % key20)
        assert [tuple(b) for b in best] == list(at) and (score == 255).all()
    img = frames(14, 3, 21, 40)  # ... and on the dot-product route
    at = ((0, 0), (33, 16), (17, 9))
    tmpl = np.stack([img[f, y:y + 5, x:x + 7] for f, (x, y) in enumerate(at)])
    assert plan(40, 21, 7, 5, 3) == "dot4"
    _, best, score = run(g, mem, oracles, "per-frame dot", img, tmpl, "per-frame templates, dot products")
    assert [tuple(b) for b in best] == list(at) and (score == 255).all()


def check_dot_and_wide_routes(g, mem, oracles):
    """5: 7 x 5 on a width that is a multiple of 4 and on one that is not; a template of 16382 columns"""
    for iw, kernel in ((300, "dot4"), (301, "dot")):
        img = frames(15, 2, 23, iw)
        assert plan(iw, 23, 7, 5, 2) == kernel
        run(g, mem, oracles, kernel, img, np.ascontiguousarray(img[1, 11:16, 290:297]), kernel, without_score=True)
    img = frames(16, 2, 3, 16390)
    assert plan(16390, 3, 16382, 2, 2) == "px" and plan(16390, 3, 16381, 2, 2) == "dot"
    run(g, mem, oracles, "px", img, np.ascontiguousarray(img[0, 1:3, 5:16387]), "wide template")


@functools.lru_cache(maxsize=None)
def twice():
    """frame 0 holds the template at A = (130, 40) and B = (5, 50): different 64 x 128 tiles, A's the later one in block
    order; frame 1 at A = (100, 10) and B = (20, 20): the same tile, A in wave 1 and B in wave 0.  B lies left of and below A
    both times, so A is the first maximum in raster order and the second in tile / wave order."""
    img = np.array(frames(17, 2, 100, 150))
    tmpl = np.array(frames(18, 1, 32, 16)[0])
    places = (((130, 40), (5, 50)), ((100, 10), (20, 20)))
    for f, pair in enumerate(places):
        for x, y in pair:
            img[f, y:y + 32, x:x + 16] = tmpl
    img.setflags(write=False)
    return img, tmpl, places


def check_first_maximum(g, mem, oracles):
    """6"""
    img, tmpl, places = twice()
    for key20 in (2, 3, 1):  # whole tiles, split tiles, dot products
        with tuned(g, key20=key20):
            maps, best, score = run(g, mem, oracles, "twice", img, tmpl, "two maxima, key 20 = %d" % key20)
        for f, (a, b) in enumerate(places):
            assert maps[f][a[1], a[0]] == 255 and maps[f][b[1], b[0]] == 255 and (maps[f] == 255).sum() == 2
            assert tuple(best[f]) == a and score[f] == 255


@functools.lru_cache(maxsize=None)
def with_a_frame_of_zeros():
    img = np.array(frames(19, 3, 100, 150))
    img[1] = 0
    img.setflags(write=False)
    return img, np.full((32, 16), 255, np.uint8)


def check_all_zero_map(g, mem, oracles):
    """7: frame 1 is black and the template white: its map is all zeros, {0, 0} / 0; frames 0 and 2 are not affected"""
    img, tmpl = with_a_frame_of_zeros()
    for key20 in (2, 3, 1):
        with tuned(g, key20=key20):
            maps, best, score = run(g, mem, oracles, "zeros", img, tmpl, "a map of zeros, key 20 = %d" % key20)
        assert not maps[1].any() and tuple(best[1]) == (0, 0) and score[1] == 0
        assert score[0] > 0 and score[2] > 0


def check_chunk_boundary(g, mem, oracles):
    """9: key 26 = 2: three frames are a chunk of two and a chunk of one.  On the matrix cores the capped run gives the
    oracle's bytes like the uncapped run of case 1, so the two are identical; on the dot products both runs are made here and
    compared.  With per-frame templates the second chunk has to start at template 2."""
    img, tmpl = small_frames()
    with tuned(g, key20=2, key26=2):
        run(g, mem, oracles, "small", img, tmpl, "whole tiles in chunks of two frames")
    with tuned(g, key20=1):
        ref = run(g, mem, oracles, "small", img, tmpl, "dot products, one chunk")
    with tuned(g, key20=1, key26=2):
        got = run(g, mem, oracles, "small", img, tmpl, "dot products in chunks of two frames")
    assert all(np.array_equal(a, b) for a, b in zip(ref, got))
    at = ((5, 60), (130, 2), (66, 33))
    tmpl = np.stack([img[f, y:y + 32, x:x + 16] for f, (x, y) in enumerate(at)])
    with tuned(g, key20=3, key26=2):
        _, best, _ = run(g, mem, oracles, "per-frame", img, tmpl, "per-frame templates in chunks")
    assert [tuple(b) for b in best] == list(at)


@contextlib.contextmanager
def dropin_on_device_pointers(g, mem):
    """the emulator's gs_* calls take caller pointers for device memory only on request (gs_internal.h)"""
    if mem.kind != "host":
        yield
        return
    g.c.emu_device_pointers(1)
    try:
        yield
    finally:
        g.c.emu_device_pointers(0)


def check_one_frame_equals_dropin(g, mem, oracles):
    """10: n = 1 gives what gs_match_template / gs_find_best_match give for the same frame on device pointers, on every route"""
    for img, tmpl, key in ((small_frames()[0][1:2], small_frames()[1], "one small"), (frames(15, 2, 23, 300)[1:2], np.ascontiguousarray(frames(15, 2, 23, 300)[1, 11:16, 290:297]), "one dot4"),
                           (twice()[0][0:1], twice()[1], "one twice")):
        maps, best, _ = run(g, mem, oracles, key, img, tmpl, "n = 1: " + key)
        d = mem.zeros(maps.shape[1:], fill=FILL)
        with dropin_on_device_pointers(g, mem):
            g.match_template(mem.put(img[0]), mem.put(tmpl), d)
            sync(mem)
            assert np.array_equal(np.asarray(mem.get(d)), maps[0]), key
            assert tuple(g.find_best_match(d)) == tuple(best[0]), key


def check_nothing_for_no_frames(g, mem, oracles):
    """11, the part that returns: n = 0 launches nothing and checks nothing (the NULL and zero-sized arguments would abort)"""
    a = mem.zeros((2, 9, 20), fill=3)
    b = mem.zeros((2, 8), fill=FILL)
    g.match_template_batch(a[0:0], a[0:0], a[0])
    g.find_best_match_batch(a[0:0], b[0:0], None)
    g.locate_template_batch(a[0:0], a[0], b[0:0], None)
    g.c.gsh_match_template_batch(None, 0, 0, 0, None, 50, 50, 7, None)
    g.c.gsh_find_best_match_batch(None, 0, 0, 0, None, None)
    g.c.gsh_locate_template_batch(None, 0, 0, 0, None, 50, 50, 7, None, None)
    sync(mem)
    assert (np.asarray(mem.get(a)) == 3).all() and (np.asarray(mem.get(b)) == FILL).all()


ALL_CHECKS = (check_whole_tiles, check_split_and_banded, check_default_rules_few_blocks, check_per_frame_templates,
              check_dot_and_wide_routes, check_first_maximum, check_all_zero_map, check_chunk_boundary,
              check_one_frame_equals_dropin, check_nothing_for_no_frames)
