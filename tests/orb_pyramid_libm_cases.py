"""Shared cases of tests/test_orb_pyramid_libm_batch.py (emulator) and tests/test_gpu_orb_pyramid_libm_batch.py (MI355X):
gsh_orb_extract_pyramid_batch -- the pyramid ORB of the reference's default build, glibc trig on the host -- and
gsh_orb_pyramid_buffer_fill_batch, frame by frame and byte for byte.

The frames, the layout helpers and the buffer conventions are those of tests/orb_pyramid_batch_cases.py (imported, not
edited); what differs is the oracle: Oracle("port").orb_extract_pyramid per frame, whose atan2f / sinf are the glibc of the
machine the test runs on, like the library's host half -- so every comparison is bit-exact.  Every main case first asserts
FROM THE ORACLES that its expectation differs from Oracle("port_nostdlib")'s in at least one descriptor: passing by calling
the other flavour's entry is impossible.  Outputs lie between guards and start as seeded random bytes; every case states its
number of guard checks (`checks`)."""
import numpy as np

import orb_pyramid_batch_cases as oc
from grayskull_amd import KEYPOINT_DTYPE
from oracle.pyoracle import Oracle
from orb_pyramid_batch_cases import THR, batch_abcd, dims, frame_a, frame_b, frame_c, frame_d, gather, plane_sizes, scatter, sync

_EXPECTED = {}


def per_level(frame, nkps, n_levels, buf_f, thr=THR):
    """oc.per_level with the libm oracle: the driver's loop on Oracle("port").orb_extract -> [(quota, keypoints)] per level"""
    lev = oc.levels_of(frame, n_levels)
    L = len(lev)
    sizes = [p.size for p in lev[1:]] + [p.size for p in lev]
    out, total = [], 0
    for l in range(L):
        quota = nkps // L if l < L - 1 else nkps - total
        if quota == 0:
            out.append((0, np.zeros(0, KEYPOINT_DTYPE)))
            continue
        so = sum(sizes[:L - 1 + l])
        k = oc.port().orb_extract(lev[l], quota, thr, buf_f[so:so + lev[l].size].reshape(lev[l].shape))
        out.append((quota, k))
        total += len(k)
    return out


def orb_expected(key, frames, nkps, n_levels, pre_buf, thr=THR, differs=True):
    """per frame the libm oracle's (keypoints, single-frame buffer, [(quota, kept)] per level), computed once per key.
    differs: assert that some descriptor of the batch is not what the GS_NO_STDLIB oracle gives"""
    if key not in _EXPECTED:
        n, h, w = frames.shape
        sizes = plane_sizes(w, h, n_levels)
        out, other = [], False
        for f in range(n):
            buf_f = gather(pre_buf, f, sizes, n)
            ko, bo = oc.port().orb_extract_pyramid(frames[f], nkps, thr, n_levels, buf_f)
            pl = per_level(frames[f], nkps, n_levels, buf_f, thr)
            cat = []
            for l, (_, k) in enumerate(pl):
                k = k.copy()
                k["x"] <<= l
                k["y"] <<= l
                cat.append(k)
            cat = np.concatenate(cat) if cat else np.zeros(0, KEYPOINT_DTYPE)
            assert cat.tobytes() == ko.tobytes(), "the restated level loop and the oracle's pyramid disagree on frame %d of %s" % (f, key)
            kn, bn = oc.ns().orb_extract_pyramid(frames[f], nkps, thr, n_levels, buf_f)
            # the selection needs no trig: the same keypoints and score maps in both flavours, other angles and descriptors
            assert len(kn) == len(ko) and np.array_equal(kn["x"], ko["x"]) and np.array_equal(bn[:sum(sizes)], bo[:sum(sizes)])
            other = other or bool((kn["desc"] != ko["desc"]).any())
            out.append((ko, bo[:sum(sizes)], [(q, len(k)) for q, k in pl]))
        assert other or not differs, "%s: no descriptor tells the libm flavour from the GS_NO_STDLIB one" % key
        _EXPECTED[key] = out
    return _EXPECTED[key]


class Pending:
    """one enqueued call: its guarded buffers and what they have to hold"""


def start_orb(g, gd, key, seed, frames, nkps, n_levels, with_lc=True, thr=THR):
    """the call on guarded, randomly prefilled buffers; nothing is read back"""
    n, h, w = frames.shape
    p = Pending()
    p.key, p.frames, p.nkps, p.n_levels, p.thr, p.with_lc = key, frames, nkps, n_levels, thr, with_lc
    p.sizes = plane_sizes(w, h, n_levels)
    nb1 = sum(p.sizes)
    assert nb1 == Oracle.orb_pyramid_buffer_bytes(w, h, n_levels) == g.orb_pyramid_buffer_bytes(w, h, n_levels)
    rs = np.random.RandomState(seed)
    p.bb, bv = gd.make(n * nb1, np.uint8, 1, prefill=rs.randint(0, 256, n * nb1).astype(np.uint8), stride=w)
    p.kb, kv = gd.make((n, nkps), KEYPOINT_DTYPE, 4, prefill=rs.randint(0, 256, n * nkps * 48).astype(np.uint8))
    p.cb, cv = gd.make(n, np.uint32, 4)
    p.lb, lv = gd.make((n, 4), np.uint32, 4) if with_lc else (None, None)
    g.orb_extract_pyramid_batch(gd.put(frames, 1), bv, kv, cv, nkps, thr, n_levels, lv)
    return p


def finish_orb(gd, p):
    """the guard checks of a call (3, 4 with level_counts) -> [[(quota, kept)] per level] per frame"""
    n, h, w = p.frames.shape
    want = orb_expected(p.key, p.frames, p.nkps, p.n_levels, p.bb.expected().reshape(-1), p.thr)
    eb, ek, ec, el = p.bb.expected().reshape(-1), p.kb.expected(), np.zeros(n, np.uint32), np.zeros((n, 4), np.uint32)
    for f, (ko, bo, pl) in enumerate(want):
        scatter(eb, f, p.sizes, n, bo)
        if len(ko):
            ek[f, :len(ko)] = ko
        ec[f] = len(ko)
        el[f, :len(pl)] = [kept for _, kept in pl]
    what = "%s: %d x %dx%d, %d levels, nkps %d" % (p.key, n, w, h, p.n_levels, p.nkps)
    gd.check(p.cb, ec, "counts, " + what)
    if p.with_lc:
        gd.check(p.lb, el, "level_counts, " + what)
    gd.check(p.kb, ek, "kps, " + what)
    gd.check(p.bb, eb, "buffer, " + what)
    return [pl for _, _, pl in want]


def run_orb(g, gd, key, seed, frames, nkps, n_levels, with_lc=True, thr=THR):
    p = start_orb(g, gd, key, seed, frames, nkps, n_levels, with_lc, thr)
    sync(g, gd)
    return finish_orb(gd, p)


def totals(pl):
    return [sum(k for _, k in p) for p in pl]


def check_quotas_differ_in_one_batch(g, gd):
    """203 x 171, 3 levels, nkps 90: last-level quotas 30 / 90 / 30 / 41 inside one batch, totals 68 / 0 / 76 / 59"""
    pl = run_orb(g, gd, "libm quotas", 101, batch_abcd(203, 171), 90, 3)
    assert [p[-1][0] for p in pl] == [30, 90, 30, 41] and totals(pl) == [68, 0, 76, 59], pl


def check_remainder_is_not_per(g, gd):
    """203 x 171, 3 levels, nkps 31: quotas 10, 10, then 21 / 31 / 11 / 11; totals 18 / 0 / 31 / 30"""
    pl = run_orb(g, gd, "libm remainder", 102, batch_abcd(203, 171), 31, 3)
    assert [p[2][0] for p in pl] == [21, 31, 11, 11] and totals(pl) == [18, 0, 31, 30], pl


def check_cap_per_frame(g, gd):
    """131 x 97, 2 levels, nkps 9: frame C's last level has a quota of 5, so its own FAST cap is 20, not 36"""
    pl = run_orb(g, gd, "libm cap", 103, batch_abcd(131, 97), 9, 2)
    assert pl[2][-1][0] == 5, pl


def check_per_is_zero(g, gd):
    """203 x 171, 3 levels, nkps 2: per == 0, levels 0 and 1 are skipped and their score maps keep their prefill"""
    pl = run_orb(g, gd, "libm per0", 104, batch_abcd(203, 171), 2, 3)
    assert all(p[0] == (0, 0) and p[1] == (0, 0) and p[2][0] == 2 for p in pl) and any(p[2][1] > 0 for p in pl), pl


def check_four_levels(g, gd):
    """300 x 270, 4 levels, nkps 50: the last level is 37 x 33"""
    assert dims(300, 270, 4)[-1] == (37, 33)
    pl = run_orb(g, gd, "libm four", 105, batch_abcd(300, 270), 50, 4)
    assert all(len(p) == 4 for p in pl) and sum(totals(pl)) > 50
    assert any(p[3][1] > 0 for p in pl), "no keypoint comes from the fourth level"


def check_levels_stop_early(g, gd):
    """96 x 80, 3 levels, nkps 40: the third level would be 24 x 20, so L = 2"""
    assert len(dims(96, 80, 3)) == 2
    pl = run_orb(g, gd, "libm stop", 106, batch_abcd(96, 80), 40, 3)
    assert all(len(p) == 2 and p[0][0] == 20 for p in pl)


def check_single_frame_layout(g, gd):
    """n = 1 of 203 x 171: the buffer equals the oracle's single-frame buffer byte for byte"""
    sizes = plane_sizes(203, 171, 3)
    b = np.arange(sum(sizes), dtype=np.uint32).astype(np.uint8)
    assert np.array_equal(gather(b, 0, sizes, 1), b)
    run_orb(g, gd, "libm single", 107, batch_abcd(203, 171)[:1], 90, 3)


def check_without_level_counts(g, gd):
    """level_counts = NULL"""
    run_orb(g, gd, "libm quotas", 101, batch_abcd(203, 171), 90, 3, with_lc=False)


def check_launch_split(g, gd):
    """gsh_tune key 8 = 2 and = 3 with four frames of 131 x 97 (launches of 2 + 2 and of 3 + 1): the same results"""
    for per_launch in (2, 3):
        g.tune(8, per_launch)
        try:
            run_orb(g, gd, "libm cap", 103, batch_abcd(131, 97), 9, 2)
            run_orb(g, gd, "libm cap", 103, batch_abcd(131, 97), 9, 2, with_lc=False)
        finally:
            g.tune(8, 0)


def other_frames(w, h):
    """frames C, D, B, A with other seeds: another batch of the quota case's shape"""
    return np.stack([frame_c(w, h, 9), frame_d(w, h, 13), frame_b(w, h), frame_a(w, h, 41)])


def check_two_calls_then_one_sync(g, gd):
    """the quota case on two different batches, the second call right behind the first, both results checked only after the
    second: the second call's host half writes the pinned trig staging the first call's upload was read from"""
    a = start_orb(g, gd, "libm quotas", 101, batch_abcd(203, 171), 90, 3)
    b = start_orb(g, gd, "libm quotas 2", 111, other_frames(203, 171), 90, 3)
    sync(g, gd)
    assert totals(finish_orb(gd, a)) == [68, 0, 76, 59]
    pl = finish_orb(gd, b)
    assert sum(1 for t in totals(pl) if t > 20) >= 3, pl


def check_degenerate(g, gd):
    """n_levels = 0, nkps = 0 and 6 x 40 frames: counts and level_counts are zeroed and nothing else is touched; n = 0 returns
    before any check"""
    for w, h, nkps, n_levels in ((203, 171, 5, 0), (203, 171, 0, 3), (6, 40, 5, 3), (40, 6, 5, 1)):
        frames = np.stack([Oracle.synth(w, h, 5 + f) for f in range(3)])
        n = len(frames)
        bb, bv = gd.make(n * max(1, sum(plane_sizes(w, h, n_levels or 3))), np.uint8, 1)
        kb, kv = gd.make((n, max(nkps, 1)), KEYPOINT_DTYPE, 4)
        what = "%dx%d nkps %d, %d levels" % (w, h, nkps, n_levels)
        for with_lc in (True, False):
            cb, cv = gd.make(n, np.uint32, 4)
            lb, lv = gd.make((n, 4), np.uint32, 4)
            g.orb_extract_pyramid_batch(gd.put(frames, 1), bv, kv, cv, nkps, THR, n_levels, lv if with_lc else None)
            sync(g, gd)
            gd.check(cb, np.zeros(n, np.uint32), "counts, " + what)
            gd.check(lb, np.zeros((n, 4), np.uint32) if with_lc else None, "level_counts, " + what)
        gd.check(kb, None, "kps, " + what)
        gd.check(bb, None, "buffer, " + what)
    g.c.gsh_orb_extract_pyramid_batch(None, 0, 0, 0, None, None, None, None, 5, THR, 3)


for _c, _k in ((check_quotas_differ_in_one_batch, 4), (check_remainder_is_not_per, 4), (check_cap_per_frame, 4), (check_per_is_zero, 4),
               (check_four_levels, 4), (check_levels_stop_early, 4), (check_single_frame_layout, 4), (check_without_level_counts, 3),
               (check_launch_split, 14), (check_two_calls_then_one_sync, 8), (check_degenerate, 4 * 6)):
    _c.checks = _k

ORB_CHECKS = (check_quotas_differ_in_one_batch, check_remainder_is_not_per, check_cap_per_frame, check_per_is_zero, check_four_levels,
              check_levels_stop_early, check_single_frame_layout, check_without_level_counts, check_launch_split,
              check_two_calls_then_one_sync, check_degenerate)


# ---- gsh_orb_pyramid_buffer_fill_batch -----------------------------------------------------------------------------------
# (w, h, n_levels, L, n)
FILL_CASES = ((203, 171, 3, 3, 3), (203, 171, 3, 3, 1), (263, 261, 4, 4, 3), (263, 261, 4, 4, 1), (203, 171, 1, 1, 3), (96, 80, 3, 2, 2))


def check_fill(g, gd, w, h, n_levels, L, n):
    """a random single-frame buffer at an odd address -> the batch buffer (at another odd phase) equals the scatter of the
    single buffer into every frame, its guards intact"""
    sizes = plane_sizes(w, h, n_levels)
    assert len(sizes) == 2 * L - 1
    nb1 = sum(sizes)
    single = np.random.RandomState(w + n).randint(0, 256, nb1).astype(np.uint8)
    bb, bv = gd.make(n * nb1, np.uint8, 3, stride=w)
    g.orb_pyramid_buffer_fill_batch(bv, gd.put(single, 1), w, h, n_levels, n)
    sync(g, gd)
    exp = bb.expected().reshape(-1)
    for f in range(n):
        scatter(exp, f, sizes, n, single)
    assert n > 1 or np.array_equal(exp, single)
    gd.check(bb, exp, "gsh_orb_pyramid_buffer_fill_batch %d x %dx%d, %d levels" % (n, w, h, n_levels), owned=np.ones(exp.size, bool))


check_fill.checks = 1


def check_fill_writes_nothing(g, gd):
    """n == 0 and n_levels == 0 write nothing and check nothing; a frame split (gsh_tune key 8 = 2 on three frames) fills
    every frame"""
    w, h = 203, 171
    nb1 = sum(plane_sizes(w, h, 3))
    single = gd.put(np.random.RandomState(3).randint(0, 256, nb1).astype(np.uint8), 1)
    bb, bv = gd.make(3 * nb1, np.uint8, 1, stride=w)
    g.orb_pyramid_buffer_fill_batch(bv, single, w, h, 3, 0)
    g.orb_pyramid_buffer_fill_batch(bv, single, w, h, 0, 3)
    g.c.gsh_orb_pyramid_buffer_fill_batch(None, None, 0, 0, 3, 0)
    sync(g, gd)
    gd.check(bb, None, "gsh_orb_pyramid_buffer_fill_batch n = 0 / n_levels = 0")
    g.tune(8, 2)
    try:
        check_fill(g, gd, w, h, 3, 3, 3)
    finally:
        g.tune(8, 0)


check_fill_writes_nothing.checks = 2
