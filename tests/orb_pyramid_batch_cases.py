"""Shared cases of tests/test_orb_pyramid_batch.py (emulator) and tests/test_gpu_orb_pyramid_batch.py (MI355X):
gsh_pyramid_batch and gsh_orb_extract_pyramid_batch_nostdlib against the oracle, frame by frame and byte for byte.

`g` is a bound library, `gd` a guard_cases.Guarded ("host": the emulator takes host memory for device memory; "device":
torch CUDA tensors).  Expected values come from the oracle only: Oracle("port_nostdlib").orb_extract_pyramid per frame --
called with the frame's planes of the batch buffer's prefill gathered into the single-frame layout -- and Oracle.downsample.
Every output (level planes, buffer, kps, counts, level_counts) lies between guards and starts as seeded random bytes, so the
caller-owned 3-px frames of the score maps are kept AND read, and the records at and beyond counts[f] must keep their
prefill.  Every case states how many guard checks it makes (`checks`); the tests assert that count.

The level counts have no oracle call of their own: `per_level` restates the driver's loop (nanomagick.c:272-288) with
Oracle.orb_extract on the Oracle.downsample'd levels, and every case asserts that its concatenation IS the oracle's
orb_extract_pyramid result before it is used."""
import numpy as np

from grayskull_amd import KEYPOINT_DTYPE
from oracle.pyoracle import Oracle

THR = 20
_NS, _PORT, _EXPECTED = [], [], {}


def ns():
    if not _NS:
        _NS.append(Oracle("port_nostdlib"))
    return _NS[0]


def port():
    if not _PORT:
        _PORT.append(Oracle("port"))
    return _PORT[0]


def sync(g, gd):
    g.sync()
    if gd.kind == "device":
        gd.torch.cuda.synchronize()


def dims(w, h, n_levels):
    """the driver's levels (nanomagick.c:247-260): [(w, h), (w/2, h/2), ...]"""
    out = [(w, h)]
    for _ in range(1, min(n_levels, 4)):
        nw, nh = out[-1][0] // 2, out[-1][1] // 2
        if nw < 32 or nh < 32:
            break
        out.append((nw, nh))
    return out if n_levels else []


def plane_sizes(w, h, n_levels):
    """bytes of one frame's planes in buffer order: levels 1 .. L-1, then score maps 0 .. L-1"""
    d = dims(w, h, n_levels)
    return [a * b for a, b in d[1:]] + [a * b for a, b in d]


def gather(batch, f, sizes, n):
    """frame f's planes of a level-major batch buffer as one single-frame buffer"""
    out, off = [], 0
    for s in sizes:
        out.append(batch[off + f * s:off + (f + 1) * s])
        off += n * s
    return np.concatenate(out) if out else np.zeros(0, np.uint8)


def scatter(batch, f, sizes, n, single):
    off, so = 0, 0
    for s in sizes:
        batch[off + f * s:off + (f + 1) * s] = single[so:so + s]
        off, so = off + n * s, so + s


def levels_of(frame, n_levels):
    out = [np.ascontiguousarray(frame)]
    for _ in dims(frame.shape[1], frame.shape[0], n_levels)[1:]:
        out.append(port().downsample(out[-1]))
    return out


# ---- gsh_pyramid_batch -----------------------------------------------------------------------------------------------------
# (w, h, n_levels, L)
PYRAMID_CASES = ((64, 64, 2, 2), (65, 67, 2, 2), (128, 64, 3, 2), (263, 261, 4, 4), (300, 270, 4, 4), (1030, 70, 2, 2), (70, 1030, 2, 2))


def pyramid_frames(w, h):
    return np.stack([Oracle.synth(w, h, 11 + 5 * f) for f in range(3)])


def pyramid_expected(frames, n_levels, pre):
    """the level planes (n frames each, level-major) laid over a copy of the prefill"""
    n, h, w = frames.shape
    exp, off = pre.copy(), 0
    per_frame = [levels_of(f, n_levels) for f in frames]
    for l in range(1, len(per_frame[0])):
        for f in range(n):
            p = per_frame[f][l].reshape(-1)
            exp[off:off + p.size] = p
            off += p.size
    return exp, off


def check_pyramid(g, gd, w, h, n_levels, L):
    """n = 3 synth frames at an odd address; the level planes inside guards, exactly as large as the levels"""
    frames = pyramid_frames(w, h)
    n = len(frames)
    d = dims(w, h, n_levels)
    assert len(d) == L
    nbytes = n * sum(a * b for a, b in d[1:])
    bb, bv = gd.make(nbytes, np.uint8, 1, stride=w)
    g.pyramid_batch(bv, gd.put(frames, 1 if (w * h) % 2 == 0 else 0), n_levels)
    sync(g, gd)
    exp, used = pyramid_expected(frames, n_levels, bb.expected())
    assert used == nbytes
    gd.check(bb, exp, "gsh_pyramid_batch %dx%d, %d levels" % (w, h, n_levels))


check_pyramid.checks = 1


def check_pyramid_level_rules(g, gd):
    """n_levels = 1 writes nothing (the guarded prefill stays); n_levels = 9 equals n_levels = 4; n = 0 touches nothing"""
    w, h = 263, 261
    frames = pyramid_frames(w, h)
    s = gd.put(frames, 1)
    nbytes = len(frames) * sum(a * b for a, b in dims(w, h, 4)[1:])
    bb, bv = gd.make(nbytes, np.uint8, 1, stride=w)
    g.pyramid_batch(bv, s, 1)
    g.pyramid_batch(bv, s, 0)
    g.pyramid_batch(bv, s[0:0], 4)
    g.c.gsh_pyramid_batch(None, None, 0, 0, 0, 4)
    sync(g, gd)
    gd.check(bb, None, "gsh_pyramid_batch n_levels = 1 / 0, n = 0")
    exp, _ = pyramid_expected(frames, 4, bb.expected())
    g.pyramid_batch(bv, s, 9)
    sync(g, gd)
    gd.check(bb, exp, "gsh_pyramid_batch n_levels = 9")


check_pyramid_level_rules.checks = 2


# ---- gsh_orb_extract_pyramid_batch_nostdlib ----------------------------------------------------------------------------------
def frame_a(w, h, seed=21):
    return Oracle.synth(w, h, seed)


def frame_b(w, h, seed=0):
    return np.full((h, w), 90, np.uint8)


def frame_c(w, h, seed=3):
    s = min(80, h - 40, w - 40)
    f = np.full((h, w), 40, np.uint8)
    y0, x0 = h // 2 - s // 2, w // 2 - s // 2
    f[y0:y0 + s, x0:x0 + s] = Oracle.synth(s, s, seed)
    return f


def frame_d(w, h, seed=7):
    f = Oracle.synth(w, h, seed).copy()
    f[:, :w // 2] = 17
    return f


def batch_abcd(w, h):
    return np.stack([frame_a(w, h), frame_b(w, h), frame_c(w, h), frame_d(w, h)])


def per_level(frame, nkps, n_levels, buf_f, thr=THR):
    """the driver's loop restated on the oracle's single-level calls -> [(quota, keypoints of the level, unscaled)] per
    level; buf_f: the frame's single-frame buffer (its score maps' frames are read)"""
    lev = levels_of(frame, n_levels)
    L = len(lev)
    sizes = [p.size for p in lev[1:]] + [p.size for p in lev]
    out, total = [], 0
    for l in range(L):
        quota = nkps // L if l < L - 1 else nkps - total
        if quota == 0:
            out.append((0, np.zeros(0, KEYPOINT_DTYPE)))
            continue
        so = sum(sizes[:L - 1 + l])
        k = ns().orb_extract(lev[l], quota, thr, buf_f[so:so + lev[l].size].reshape(lev[l].shape))
        out.append((quota, k))
        total += len(k)
    return out


def orb_expected(key, frames, nkps, n_levels, pre_buf, thr=THR):
    """per frame the oracle's (keypoints, single-frame buffer, [(quota, kept)] per level), computed once per case"""
    if key not in _EXPECTED:
        n, h, w = frames.shape
        sizes = plane_sizes(w, h, n_levels)
        out = []
        for f in range(n):
            buf_f = gather(pre_buf, f, sizes, n)
            ko, bo = ns().orb_extract_pyramid(frames[f], nkps, thr, n_levels, buf_f)
            pl = per_level(frames[f], nkps, n_levels, buf_f, thr)
            cat = []
            for l, (_, k) in enumerate(pl):
                k = k.copy()
                k["x"] <<= l
                k["y"] <<= l
                cat.append(k)
            cat = np.concatenate(cat) if cat else np.zeros(0, KEYPOINT_DTYPE)
            assert cat.tobytes() == ko.tobytes(), "the restated level loop and the oracle's pyramid disagree on frame %d of %s" % (f, key)
            out.append((ko, bo[:sum(sizes)], [(q, len(k)) for q, k in pl]))
        _EXPECTED[key] = out
    return _EXPECTED[key]


def run_orb(g, gd, key, seed, frames, nkps, n_levels, with_lc=True, thr=THR):
    """one call on guarded buffers against the oracle -> [[(quota, kept)] per level] per frame.  3 guard checks, 4 with
    level_counts"""
    n, h, w = frames.shape
    sizes = plane_sizes(w, h, n_levels)
    nb1 = sum(sizes)
    assert nb1 == Oracle.orb_pyramid_buffer_bytes(w, h, n_levels) == g.orb_pyramid_buffer_bytes(w, h, n_levels)
    assert g.orb_pyramid_batch_buffer_bytes(w, h, n_levels, n) == n * nb1
    rs = np.random.RandomState(seed)
    bb, bv = gd.make(n * nb1, np.uint8, 1, prefill=rs.randint(0, 256, n * nb1).astype(np.uint8), stride=w)
    kb, kv = gd.make((n, nkps), KEYPOINT_DTYPE, 4, prefill=rs.randint(0, 256, n * nkps * 48).astype(np.uint8))
    cb, cv = gd.make(n, np.uint32, 4)
    lb, lv = gd.make((n, 4), np.uint32, 4) if with_lc else (None, None)
    g.orb_extract_pyramid_batch_nostdlib(gd.put(frames, 1), bv, kv, cv, nkps, thr, n_levels, lv)
    sync(g, gd)
    want = orb_expected(key, frames, nkps, n_levels, bb.expected().reshape(-1), thr)
    eb, ek, ec, el = bb.expected().reshape(-1), kb.expected(), np.zeros(n, np.uint32), np.zeros((n, 4), np.uint32)
    for f, (ko, bo, pl) in enumerate(want):
        scatter(eb, f, sizes, n, bo)
        if len(ko):
            ek[f, :len(ko)] = ko
        ec[f] = len(ko)
        el[f, :len(pl)] = [kept for _, kept in pl]
    what = "%s: %d x %dx%d, %d levels, nkps %d" % (key, n, w, h, n_levels, nkps)
    gd.check(cb, ec, "counts, " + what)
    if with_lc:
        gd.check(lb, el, "level_counts, " + what)
    gd.check(kb, ek, "kps, " + what)
    gd.check(bb, eb, "buffer, " + what)
    return [pl for _, _, pl in want]


def check_quotas_differ_in_one_batch(g, gd):
    """203 x 171, 3 levels, nkps 90: the frames' last-level quotas differ inside one batch (30 / 90 / 30 / 41), totals
    68 / 0 / 76 / 59"""
    pl = run_orb(g, gd, "quotas", 101, batch_abcd(203, 171), 90, 3)
    last = [p[-1][0] for p in pl]
    assert len(set(last)) >= 3, last
    assert last == [30, 90, 30, 41] and [sum(k for _, k in p) for p in pl] == [68, 0, 76, 59], pl


def check_remainder_is_not_per(g, gd):
    """203 x 171, 3 levels, nkps 31: quotas 10, 10, then 21 / 31 / 11 / 11; frame A's level 0 keeps none of its corners, because
    its first 40 in scan order all lie in the 15-px border: the FAST cap shows in the result"""
    frames = batch_abcd(203, 171)
    pl = run_orb(g, gd, "remainder", 102, frames, 31, 3)
    assert [p[0][0] for p in pl] == [10] * 4 and [p[1][0] for p in pl] == [10] * 4
    assert [p[2][0] for p in pl] == [21, 31, 11, 11], pl
    assert pl[0][0] == (10, 0) and len(port().fast(frames[0], 5000, THR)[0]) > 40


def select(cands, quota, w, h):
    """ref :657-667 on a candidate list: stable descending sort by response, 15-px border filter, the first `quota`"""
    order = np.argsort(-cands["response"].astype(np.int64), kind="stable")
    c = cands[order]
    ok = (c["x"] >= 15) & (c["y"] >= 15) & (c["x"] < w - 15) & (c["y"] < h - 15)
    return [(int(x), int(y)) for x, y in zip(c["x"][ok][:quota], c["y"][ok][:quota])]


def check_cap_per_frame(g, gd):
    """131 x 97, 2 levels, nkps 9: frame C's last level has 39 corners and a quota of 5, so its cap is 20; selecting from the
    first min(4 * 9, 5000) = 36 candidates gives another keypoint list -- the case a uniform cap gets wrong.  Both
    selections are computed from oracle.fast + stable sort + border filter and must differ for a frame of the batch."""
    frames = batch_abcd(131, 97)
    pl = run_orb(g, gd, "cap", 103, frames, 9, 2)
    differ = []
    for f, p in enumerate(pl):
        quota = p[-1][0]
        lev = levels_of(frames[f], 2)[1]
        h, w = lev.shape
        own = select(port().fast(lev, min(4 * quota, 5000), THR)[0], quota, w, h)
        uniform = select(port().fast(lev, min(4 * 9, 5000), THR)[0], quota, w, h)
        differ.append(own != uniform)
    assert any(differ), "no frame of the batch tells the frame's own cap from the uniform one"
    assert pl[2][-1][0] == 5 and differ[2], (pl, differ)


def check_per_is_zero(g, gd):
    """203 x 171, 3 levels, nkps 2: per == 0, levels 0 and 1 are skipped and their score-map planes keep their prefill
    (run_orb compares the whole buffer); level counts 0, 0, k"""
    pl = run_orb(g, gd, "per0", 104, batch_abcd(203, 171), 2, 3)
    assert all(p[0] == (0, 0) and p[1] == (0, 0) and p[2][0] == 2 for p in pl), pl
    assert any(p[2][1] > 0 for p in pl)


def check_four_levels(g, gd):
    """300 x 270, 4 levels, nkps 50: the last level is 37 x 33"""
    assert dims(300, 270, 4)[-1] == (37, 33)
    pl = run_orb(g, gd, "four", 105, batch_abcd(300, 270), 50, 4)
    assert all(len(p) == 4 for p in pl) and sum(k for p in pl for _, k in p) > 50


def check_levels_stop_early(g, gd):
    """96 x 80, 3 levels, nkps 40: the third level would be 24 x 20, so L = 2"""
    assert len(dims(96, 80, 3)) == 2
    pl = run_orb(g, gd, "stop", 106, batch_abcd(96, 80), 40, 3)
    assert all(len(p) == 2 and p[0][0] == 20 for p in pl)


def check_single_frame_layout(g, gd):
    """n = 1 of 203 x 171: the buffer equals the oracle's single-frame buffer byte for byte (gather / scatter are the
    identity for n = 1: asserted)"""
    frames = batch_abcd(203, 171)[:1]
    sizes = plane_sizes(203, 171, 3)
    b = np.arange(sum(sizes), dtype=np.uint32).astype(np.uint8)
    assert np.array_equal(gather(b, 0, sizes, 1), b)
    run_orb(g, gd, "single", 107, frames, 90, 3)


def check_without_level_counts(g, gd):
    """level_counts = NULL"""
    run_orb(g, gd, "quotas", 101, batch_abcd(203, 171), 90, 3, with_lc=False)


def check_launch_split(g, gd):
    """GSH_TUNE_FRAMES_PER_LAUNCH = 2 with four frames of 131 x 97 and gsh_tune key 8 = 3 (launches of 3 and 1): the same
    results, every plane at its level-major place"""
    for per_launch in (2, 3):
        g.tune(8, per_launch)
        try:
            run_orb(g, gd, "cap", 103, batch_abcd(131, 97), 9, 2)
        finally:
            g.tune(8, 0)


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
            g.orb_extract_pyramid_batch_nostdlib(gd.put(frames, 1), bv, kv, cv, nkps, THR, n_levels, lv if with_lc else None)
            sync(g, gd)
            gd.check(cb, np.zeros(n, np.uint32), "counts, " + what)
            gd.check(lb, np.zeros((n, 4), np.uint32) if with_lc else None, "level_counts, " + what)
        gd.check(kb, None, "kps, " + what)
        gd.check(bb, None, "buffer, " + what)
    g.c.gsh_orb_extract_pyramid_batch_nostdlib(None, 0, 0, 0, None, None, None, None, 5, THR, 3)


for _c, _k in ((check_quotas_differ_in_one_batch, 4), (check_remainder_is_not_per, 4), (check_cap_per_frame, 4), (check_per_is_zero, 4),
               (check_four_levels, 4), (check_levels_stop_early, 4), (check_single_frame_layout, 4), (check_without_level_counts, 3),
               (check_launch_split, 8), (check_degenerate, 4 * 6)):
    _c.checks = _k

ORB_CHECKS = (check_quotas_differ_in_one_batch, check_remainder_is_not_per, check_cap_per_frame, check_per_is_zero, check_four_levels,
              check_levels_stop_early, check_single_frame_layout, check_without_level_counts, check_launch_split, check_degenerate)
