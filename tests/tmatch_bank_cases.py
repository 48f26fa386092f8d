"""Shared cases of tests/test_tmatch_bank.py (emulator) and tests/test_gpu_tmatch_bank.py (MI355X):
gsh_match_templates_batch and gsh_locate_templates_batch -- n frames against a bank of m templates of one size -- against the
oracle's gs_match_template / gs_find_best_match, map by map and byte for byte.

`g` is a bound library, `mem` a parity_cases.Mem, `oracles` the CPU oracles that must all give the expected bytes (the C
restatement, and the compiled reference wherever oracle/_ref was built), as in tests/tmatch_batch_cases.py.

Every run (`run`): maps, points, scores and winners are pre-filled with 0x5a and sit inside larger buffers whose other bytes
must come back untouched; img and tmpl are compared with their copies afterwards; `winner` is checked against numpy's
argmax (the first maximum) of the expected scores.  Every case takes `key27` and runs under gsh_tune key 27 = 2 (the bank kernel,
k_match_bank_mfma) or key 27 = 1 (the loop of single-template launches); the test files run each case under both.

The launcher's rule (gs_stencil.cpp: tm_bank_form) is restated in `takes`: the bank kernel is valid for templates up to 512
wide (32 slots of 16 bytes a row) with at most 32768 taps.  Its tiles: a block is 8 result rows x 64 columns, its four waves
4 rows x 32 columns each (wave = 2 (row / 4 % 2) + column / 32 % 2); templates go in groups of 32 (m <= 32) or 64."""
import contextlib
import functools

import numpy as np

from geom_batch_cases import FILL, Guarded, sync
from tmatch_batch_cases import frames

BOTH = (2, 1)


def takes(tw, th):
    """True where key 27 = 2 runs k_match_bank_mfma (else the loop runs whatever the key)"""
    return (tw + 15) // 16 <= 32 and tw * th <= 32768


@contextlib.contextmanager
def tuned(g, key27=0, key26=0, key8=0):
    try:
        g.tune(27, key27), g.tune(26, key26), g.tune(8, key8)
        yield
    finally:
        g.tune(27, 0), g.tune(26, 0), g.tune(8, 0)


_EXPECTED = {}


def expected(oracles, key, img, bank):
    """(maps (n, m, rh, rw), best (n, m, 2), score (n, m), winner (n)) of the oracles, map by map; computed once per case"""
    if key not in _EXPECTED:
        want = []
        for o in oracles:
            maps = np.stack([np.stack([o.match_template(f, t) for t in bank]) for f in img])
            best = np.array([[o.find_best_match(m) for m in per] for per in maps], np.uint32).reshape(len(img), len(bank), 2)
            want.append((maps, best))
        for maps, best in want[1:]:
            assert np.array_equal(maps, want[0][0]) and np.array_equal(best, want[0][1]), "the oracles disagree on %s" % (key,)
        maps, best = want[0]
        score = np.array([[m[y, x] for m, (x, y) in zip(per, b)] for per, b in zip(maps, best)], np.uint8)
        for per, bb, ss in zip(maps, best, score):  # what the header says about a map of zeros
            for m, b, s in zip(per, bb, ss):
                assert s == m.max() and (s > 0 or (tuple(b) == (0, 0) and not m.any()))
        winner = np.argmax(score, axis=1).astype(np.uint32)  # numpy: the first of several maxima
        for a in (maps, best, score, winner):
            a.setflags(write=False)
        _EXPECTED[key] = (maps, best, score, winner)
    return _EXPECTED[key]


def _same_maps(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%s: %d bytes differ, first at (f, t, y, x) = %s: got %d, expected %d" % (
        what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def run_once(g, mem, want, img, bank, what, optional=True):
    """the two entries on guarded buffers against `want` -> (maps, best, score, winner) as the library gave them"""
    n, ih, iw = img.shape
    m, th, tw = bank.shape
    rh, rw = ih - th + 1, iw - tw + 1
    want_maps, want_best, want_score, want_winner = want
    si, stp = Guarded(mem, img), Guarded(mem, bank, off=1)
    iv, tv = si.view(img.shape), stp.view(bank.shape)
    res = Guarded(mem, np.full(n * m * rh * rw, FILL, np.uint8), off=2)
    g.match_templates_batch(res.view((n, m, rh, rw)), iv, tv)
    maps = res.payload(what + ": maps").reshape(n, m, rh, rw)
    _same_maps(maps, want_maps, what + ": gsh_match_templates_batch")

    def outputs():
        return (Guarded(mem, np.full(n * m * 8, FILL, np.uint8)), Guarded(mem, np.full(n * m, FILL, np.uint8), off=3),
                Guarded(mem, np.full(n * 4, FILL, np.uint8), off=4))

    def points(b):
        return b.payload(what).view(np.uint32).reshape(n, m, 2)

    best, score, winner = outputs()
    g.locate_templates_batch(iv, tv, best.view((n, m, 8)), score.view((n, m)), winner.view((n, 4)))
    lb, ls, lw = points(best), score.payload(what).reshape(n, m), winner.payload(what).view(np.uint32)
    assert np.array_equal(lb, want_best) and np.array_equal(ls, want_score), (what, "gsh_locate_templates_batch", lb, want_best, ls, want_score)
    assert np.array_equal(lw, want_winner), (what, "winner", lw, want_winner)
    if optional:  # score = NULL and winner = NULL, one at a time
        best, score, _ = outputs()
        g.locate_templates_batch(iv, tv, best.view((n, m, 8)), score.view((n, m)))
        assert np.array_equal(points(best), want_best) and np.array_equal(score.payload(what).reshape(n, m), want_score), what + ": winner = None"
        best, _, winner = outputs()
        g.locate_templates_batch(iv, tv, best.view((n, m, 8)), None, winner.view((n, 4)))
        assert np.array_equal(points(best), want_best) and np.array_equal(winner.payload(what).view(np.uint32), want_winner), what + ": score = None"
    assert np.array_equal(si.payload(what).reshape(img.shape), img), what + ": img was written"
    assert np.array_equal(stp.payload(what).reshape(bank.shape), bank), what + ": tmpl was written"
    return maps, lb, ls, lw


def run(g, mem, oracles, key, img, bank, what, key27, optional=False, **tune):
    """run_once under key 27 = key27 against the oracle"""
    want = expected(oracles, key, img, bank)
    with tuned(g, key27=key27, **tune):
        return run_once(g, mem, want, img, bank, "%s, key 27 = %d" % (what, key27), optional)


# ---- the cases -----------------------------------------------------------------------------------------------------------
def check_basics(g, mem, oracles, key27):
    """1: three frames of 150 x 100, five 16 x 32 templates (result 135 x 69: three ragged block columns, nine block rows);
    template t is cut from frame t % 3 at a place of its own -- the frame's corner, the corner of block (1, 1), the last
    block, and two places inside waves 3 and 1.  m = 5: 27 of the group's 32 templates are zero rows."""
    img = frames(31, 3, 100, 150)
    at = ((0, 0), (64, 8), (130, 60), (33, 37), (97, 21))  # (x, y)
    bank = np.stack([img[t % 3, y:y + 32, x:x + 16] for t, (x, y) in enumerate(at)])
    assert takes(16, 32)
    maps, best, score, winner = run(g, mem, oracles, "basics", img, bank, "basics", key27)
    for t, (x, y) in enumerate(at):
        assert maps[t % 3, t, y, x] == 255 and tuple(best[t % 3, t]) == (x, y) and score[t % 3, t] == 255
    assert list(winner) == [0, 1, 2]  # templates 0 and 3 both score 255 on frame 0: the lower index


def check_group_boundary(g, mem, oracles, key27):
    """2: two frames of 44 x 33, 8 x 8 templates: m = 31, 32 (one group of 32), 33 (a group of 64, 31 zero rows) and 70 (two
    groups of 64, the second with 6 templates); nothing beyond map m - 1 is written (the guards)"""
    img = frames(32, 2, 33, 44)
    rng = np.random.default_rng(33)
    all70 = np.stack([img[t % 2, y:y + 8, x:x + 8] for t, (x, y) in enumerate(zip(rng.integers(0, 37, 70), rng.integers(0, 26, 70)))])
    assert takes(8, 8)
    for m in (31, 32, 33, 70):
        _, _, score, _ = run(g, mem, oracles, ("groups", m), img, all70[:m], "%d templates" % m, key27)
        assert all(score[t % 2, t] == 255 for t in range(m))


def check_widths_off_the_slots(g, mem, oracles, key27):
    """3: 7 x 5 and 17 x 3 (one and two slots a row, an odd number of slots in all: the zero slot), 33 x 9, and 16 x 1 (one row:
    one slot and the zero slot), each as a bank of three, on a frame width that is a multiple of 4 and on one that is not"""
    for iw in (300, 301):
        img = frames(34, 2, 23, iw)
        for tw, th in ((7, 5), (17, 3), (33, 9), (16, 1)):
            at = ((iw - tw, 23 - th), (0, 0), (131, 7))
            bank = np.stack([img[t % 2, y:y + th, x:x + tw] for t, (x, y) in enumerate(at)])
            assert takes(tw, th)
            _, best, score, _ = run(g, mem, oracles, ("widths", iw, tw, th), img, bank, "%d x %d on %d columns" % (tw, th, iw), key27)
            assert all(score[t % 2, t] == 255 and tuple(best[t % 2, t]) == at[t] for t in range(3))


def check_maps_of_zeros(g, mem, oracles, key27):
    """4: a black frame against white 64 x 64 templates and the reverse: maps of zeros, {0, 0} / 0, winner 0, the frames around
    it unaffected"""
    for tone in (0, 255):
        img = np.array(frames(35, 3, 70, 90))
        img[1] = tone
        bank = np.full((2, 64, 64), 255 - tone, np.uint8)
        maps, best, score, winner = run(g, mem, oracles, ("extremes", tone), img, bank, "a frame of %d" % tone, key27)
        assert not maps[1].any() and not best[1].any() and not score[1].any() and winner[1] == 0
        assert score[0].all() and score[2].all()


def check_accumulator_bound(g, mem, oracles, key27):
    """4: 256 x 128 checkerboards of 0 / 255 (32768 taps, 16 slots a row: the bank kernel takes them under key 27 = 2, two rows
    a band) against 300 x 130 frames of the inverse pattern and of the pattern itself: every window is either the template
    (255) or its inverse (0, the largest sum of squares there is)"""
    yy, xx = np.mgrid[0:130, 0:300]
    board = (((yy + xx) & 1) * 255).astype(np.uint8)
    img = np.stack([255 - board, board])
    bank = np.stack([board[:128, :256], 255 - board[:128, :256]])
    assert takes(256, 128)
    maps, best, score, winner = run(g, mem, oracles, "checkerboards", img, bank, "checkerboards", key27)
    assert set(np.unique(maps)) == {0, 255} and maps[0, 0, 0, 0] == 0 and maps[0, 0, 0, 1] == 255 and maps[0, 1, 0, 0] == 255
    assert [tuple(b) for b in best.reshape(-1, 2)] == [(1, 0), (0, 0), (0, 0), (1, 0)] and list(winner) == [0, 0]


@functools.lru_cache(maxsize=None)
def twice():
    """The template lies at A and at B of each frame; A is the first in raster order and the later one in the bank kernel's
    block and wave order.  Frame 0: A = (130, 40) in block column 2, B = (5, 44) in block column 0 of the same block row (rows
    40 .. 47).  Frame 1: A = (100, 8) and B = (70, 10), both in block (1, 1): A in wave 1, B in wave 0.  The bank holds the
    template at indices 1 and 4."""
    img = np.array(frames(36, 2, 100, 150))
    bank = np.array(frames(37, 5, 32, 16))
    bank[4] = bank[1]
    places = (((130, 40), (5, 44)), ((100, 8), (70, 10)))
    for f, pair in enumerate(places):
        for x, y in pair:
            img[f, y:y + 32, x:x + 16] = bank[1]
    img.setflags(write=False), bank.setflags(write=False)
    return img, bank, places


def check_first_maximum(g, mem, oracles, key27):
    """5"""
    img, bank, places = twice()
    maps, best, score, winner = run(g, mem, oracles, "twice", img, bank, "two maxima", key27)
    for f, (a, b) in enumerate(places):
        for t in (1, 4):
            assert maps[f, t][a[1], a[0]] == 255 and maps[f, t][b[1], b[0]] == 255 and (maps[f, t] == 255).sum() == 2
            assert tuple(best[f, t]) == a and score[f, t] == 255
        assert np.array_equal(maps[f, 1], maps[f, 4]) and winner[f] == 1


def check_chunks(g, mem, oracles, key27):
    """6: three frames of 90 x 40 and three 16 x 32 templates (result 75 x 9: 2 x 2 blocks a frame), template t from frame t:
    the uncapped run, key 26 = 2 -- a chunk of two frames and a chunk of one -- and key 8 = 1 -- a frame a launch -- give the
    same bytes, the oracle's"""
    img = frames(40, 3, 40, 90)
    at = ((70, 8), (0, 3), (33, 0))
    bank = np.stack([img[t, y:y + 32, x:x + 16] for t, (x, y) in enumerate(at)])
    ref = run(g, mem, oracles, "chunks", img, bank, "one chunk", key27)
    for what, tune in (("chunks of two frames", dict(key26=2)), ("a frame a launch", dict(key8=1))):
        got = run(g, mem, oracles, "chunks", img, bank, what, key27, **tune)
        assert all(np.array_equal(a, b) for a, b in zip(ref, got))
    assert [tuple(ref[1][t, t]) for t in range(3)] == list(at) and list(ref[3]) == [0, 1, 2]


def check_agreement_with_the_single_template_entries(g, mem, oracles, key27):
    """7, same library: m = 1 equals gsh_match_template_batch(ntmpl = 1); a bank equals the loop over its templates, maps and
    locate, on the matrix-core route of the loop (16 x 32) and on its dot products (8 x 8)"""
    for key, img, bank in (("agree 16x32", frames(41, 2, 40, 90), frames(38, 3, 32, 16)), ("agree 8x8", frames(32, 2, 33, 44), frames(39, 3, 8, 8))):
        n, ih, iw = img.shape
        m, th, tw = bank.shape
        rh, rw = ih - th + 1, iw - tw + 1
        d_img, d_bank = mem.put(img), mem.put(bank)
        loop_maps, loop_best, loop_score = mem.zeros((m, n, rh, rw), fill=FILL), mem.zeros((m, n, 8), fill=FILL), mem.zeros((m, n), fill=FILL)
        for t in range(m):
            g.match_template_batch(loop_maps[t], d_img, d_bank[t])
            g.locate_template_batch(d_img, d_bank[t], loop_best[t], loop_score[t])
        sync(mem)
        lm = np.asarray(mem.get(loop_maps)).transpose(1, 0, 2, 3)
        lb = np.asarray(mem.get(loop_best)).view(np.uint32).reshape(m, n, 2).transpose(1, 0, 2)
        ls = np.asarray(mem.get(loop_score)).transpose(1, 0)
        want = (lm, lb, ls, np.argmax(ls, axis=1).astype(np.uint32))
        with tuned(g, key27=key27):
            run_once(g, mem, want, img, bank, "%s against the loop, key 27 = %d" % (key, key27), optional=True)
            run_once(g, mem, tuple(a[:, :1] for a in want[:3]) + (np.zeros(n, np.uint32),), img, bank[:1], "%s: m = 1, key 27 = %d" % (key, key27))
        assert all(np.array_equal(a, b) for a, b in zip(want, expected(oracles, key, img, bank)))  # and the loop is the oracle's


def check_nothing_to_do(g, mem, oracles, key27):
    """8: n = 0 or m = 0 launches nothing and checks nothing (the NULL and zero-sized arguments would abort)"""
    a = mem.zeros((2, 9, 20), fill=3)
    b = mem.zeros((2, 8), fill=FILL)
    g.match_templates_batch(a[0:0], a[0:0], a)
    g.match_templates_batch(a[0:0], a, a[0:0])
    g.locate_templates_batch(a[0:0], a, b[0:0], None, None)
    g.locate_templates_batch(a, a[0:0], b[0:0], None, None)
    for n, m in ((0, 7), (7, 0), (0, 0)):
        g.c.gsh_match_templates_batch(None, 0, 0, n, None, 50, 50, m, None)
        g.c.gsh_locate_templates_batch(None, 0, 0, n, None, 50, 50, m, None, None, None)
    sync(mem)
    assert (np.asarray(mem.get(a)) == 3).all() and (np.asarray(mem.get(b)) == FILL).all()


def check_default_rule(g, mem, oracles):
    """no key set (gs_stencil.cpp: tm_bank): 8 x 8 templates, whose single-template route is the dot products, take the loop at
    m = 3 and the bank kernel at m = 4; 16 x 32 templates, whose route is the matrix cores, the loop at m = 15 and the bank
    kernel at m = 16 -- the oracle's bytes on both sides of both limits"""
    img = frames(32, 2, 33, 44)
    bank = frames(42, 4, 8, 8)
    for m in (3, 4):
        run(g, mem, oracles, ("default 8x8", m), img, bank[:m], "default rule, %d of 8 x 8" % m, 0)
    img = frames(41, 2, 40, 90)
    bank = frames(43, 16, 32, 16)
    for m in (15, 16):
        run(g, mem, oracles, ("default 16x32", m), img, bank[:m], "default rule, %d of 16 x 32" % m, 0)


ALL_CHECKS = (check_basics, check_group_boundary, check_widths_off_the_slots, check_maps_of_zeros, check_accumulator_bound,
              check_first_maximum, check_chunks, check_agreement_with_the_single_template_entries, check_nothing_to_do)
