"""Shared pieces of tests/test_lbp_cascades.py (emulator) and tests/test_gpu_lbp_cascades.py (MI355X): LBP cascades whose
STRUCTURE selects the code gs_lbp_detect runs -- stages decided by a truth table (1..12 classifiers), by the sequential
float32 sum with one lane per (window, classifier) pair (13..32, two windows per wave at 32), by a window per lane (above
32), first, in the middle and last; 1 to 8 subset words per classifier; stages stored out of order, sharing classifiers,
with classifiers no stage reaches; windows that are neither 24 x 24 nor square; scans that start at scale 0.5.

structured_cascade() builds such a cascade AROUND A FRAME: the lookup bit of every (window, classifier) of the frame's
scale-1 scan is restated in numpy (ref grayskull.h:769-808), and a stage's threshold is the exact sequential float32 sum
of one window that reaches the stage, at about the 30 % quantile of 201 such windows (for a stage above 12 classifiers: the
sampled window of rank 50..70 nearest to rank 60 whose sum is smaller when added in reverse order or in float64).  So sum == threshold happens on the frame
(and passes: the reference rejects on sum < threshold), and every stage passes some windows and rejects others.  Leaf values
mix three magnitudes (4096, 1, 3e-4: half an ulp of the first is 2.4e-4), so a float32 sum depends on the order of its adds.

Two conditions on these INPUTS are asserted whenever a case is built (case(); CPU oracle and numpy only):
  check_stage_coverage      every stage is entered by >= 256 windows of the frame's scale-1 scan, passes one, rejects one
  check_order_sensitivity   for every stage of more than 12 classifiers, among the windows that reach it, the verdict of the
                            sequential float32 sum differs from the reversed-order float32 sum's for at least one window and
                            from a float64 sum's for at least one: a kernel that added in another order or precision would
                            return other rectangles
The one stage with a NaN threshold is the exception the arithmetic forces: !(sum < NaN) holds for every sum, so it can reject
nothing; it has 2 classifiers and is asserted to pass every window it sees.

No feature rectangle leaves its window at any scale a case scans (assert_features_inside restates the test of build_scales,
gs_detect.cpp): the reference reads outside its table there, so no value is right, and the library's clamped form is not
part of these cases."""
import numpy as np

from grayskull_amd.cascade import Cascade
from oracle.pyoracle import Oracle
from util import assert_same

F32 = np.float32
UNCAPPED = 200000  # more than any scan of a <= 200 x 150 frame has windows: the cap can never be reached
MAGNITUDES = (4096.0, 1.0, 3e-4)


# ---- the reference's geometry, restated ------------------------------------------------------------------------------------
def scan_scales(window_w, window_h, iw, ih, scale_factor, min_scale, max_scale):
    """the float32 scale progression of ref :819-821 -> [(scale, win_w, win_h)]"""
    out, scale, sf = [], F32(min_scale), F32(scale_factor)
    while scale <= F32(max_scale):
        win_w, win_h = int(F32(window_w) * scale), int(F32(window_h) * scale)
        if win_w > iw or win_h > ih:
            break
        out.append((scale, win_w, win_h))
        scale = F32(scale * sf)
    return out


def scaled_feature(feat, scale):
    """ref :799-804: (fx, fy, fw, fh) of one feature at a float32 scale"""
    fx, fy, fw, fh = (int(F32(int(v)) * F32(scale)) for v in feat)
    return fx, fy, max(fw, 1), max(fh, 1)


def feature_inside(feat, window_w, window_h, scale):
    """the test of build_scales (gs_detect.cpp): the 3 x 3 cells of the scaled feature lie inside the scaled window"""
    fx, fy, fw, fh = scaled_feature(feat, scale)
    win_w, win_h = int(F32(window_w) * F32(scale)), int(F32(window_h) * F32(scale))
    return fx >= 0 and fy >= 0 and fx + 3 * fw <= win_w and fy + 3 * fh <= win_h


def assert_features_inside(casc, scales):
    feats = casc.features.reshape(-1, 4)
    for scale in scales:
        for wi in range(casc.nweaks):  # build_scales tests every stored classifier, reached or not
            f = feats[casc.weak_feature_idx[wi]]
            assert feature_inside(f, casc.window_w, casc.window_h, scale), "classifier %d leaves the window at scale %r" % (wi, scale)


def lookup_bits(casc, img, scale=1.0):
    """ref :769-808 for every window of one scale (step 1) and every stored classifier -> bool (nweaks, ny, nx).
    uint32 arithmetic wraps like the reference's unsigned sums."""
    ih, iw = img.shape
    P = np.zeros((ih + 1, iw + 1), np.uint32)
    P[1:, 1:] = np.cumsum(np.cumsum(img.astype(np.uint64), 0), 1).astype(np.uint32)
    win_w, win_h = int(F32(casc.window_w) * F32(scale)), int(F32(casc.window_h) * F32(scale))
    ny, nx = ih - win_h + 1, iw - win_w + 1
    feats = casc.features.reshape(-1, 4)
    bits = np.zeros((casc.nweaks, ny, nx), bool)
    with np.errstate(over="ignore"):
        for wi in range(casc.nweaks):
            fx, fy, fw, fh = scaled_feature(feats[casc.weak_feature_idx[wi]], scale)
            G = [[P[fy + j * fh:fy + j * fh + ny, fx + i * fw:fx + i * fw + nx] for i in range(4)] for j in range(4)]
            c = [[G[j + 1][i + 1] - G[j][i + 1] - G[j + 1][i] + G[j][i] for i in range(3)] for j in range(3)]
            ctr = c[1][1]
            code = np.zeros((ny, nx), np.uint32)
            for cell in (c[0][0], c[0][1], c[0][2], c[1][2], c[2][2], c[2][1], c[2][0], c[1][0]):  # tl tc tr r br bc bl l
                code = (code << np.uint32(1)) | (cell >= ctr)
            idx, bit = (code >> np.uint32(5)).astype(np.int64), code & np.uint32(31)
            n, off = int(casc.weak_num_subsets[wi]), int(casc.weak_subset_offset[wi])
            words = casc.subsets.view(np.uint32)[off + np.minimum(idx, n - 1)]
            bits[wi] = (idx < n) & (((words >> bit) & np.uint32(1)) != 0)
    return bits


def stage_sums(casc, s, bits, order=1, dtype=F32):
    """the sum of ref :796-809 for stage s over windows with lookup bits `bits` (nweaks, ...): sequential adds in `dtype`,
    in weak order (order = 1) or reversed (-1)"""
    first, n = int(casc.stage_weak_start[s]), int(casc.stage_nweaks[s])
    total = np.zeros(bits.shape[1:], dtype)
    with np.errstate(invalid="ignore"):
        for wi in list(range(first, first + n))[::order]:
            total = total + np.where(bits[wi], casc.weak_left_val[wi], casc.weak_right_val[wi]).astype(dtype)
    return total


def passes(sums, threshold):
    with np.errstate(invalid="ignore"):
        return ~(sums < sums.dtype.type(threshold))  # ref :810 rejects on sum < threshold: NaN on either side passes


# ---- the generator ---------------------------------------------------------------------------------------------------------
def structured_cascade(seed, stage_sizes, window_w, window_h, frame, fit_scales=(1.0,), shuffle=True, share_stages=None,
                       unreachable=(), share_subsets=False, specials=False):
    """stage_sizes: classifiers per stage in EVALUATION order.  frame: the uint8 image the thresholds are drawn from.
    fit_scales: every scale at which no feature may leave the window.  shuffle: the stages' classifier ranges are stored in
    a shuffled order.  share_stages = (i, j): stage j's range is the tail of stage i's (the whole of it at equal sizes).
    unreachable: sizes of runs of classifiers, stored between the stages' ranges, that no stage reaches (their leaves are
    NaN: a kernel that read one would pass everything).  share_subsets: two classifiers of the largest stage share a subset
    range.  specials: a -0.0 and a +inf leaf in the first stage above 12 classifiers, and a NaN threshold on the (one)
    stage of exactly 2 classifiers."""
    rs = np.random.RandomState(seed)
    ns = len(stage_sizes)
    # storage: one block of classifiers per stage that owns its range, the unreachable runs between them
    owners = [s for s in range(ns) if not (share_stages and s == share_stages[1])]
    blocks = [("stage", s, stage_sizes[s]) for s in owners] + [("dead", -1, n) for n in unreachable]
    if shuffle and len(blocks) > 1:
        perm = rs.permutation(len(blocks))
        if (perm == np.arange(len(blocks))).all():
            perm = np.roll(perm, 1)
        blocks = [blocks[i] for i in perm]
    start, dead, nw = np.zeros(ns, np.uint16), [], 0
    for kind, s, n in blocks:
        if kind == "stage":
            start[s] = nw
        else:
            dead += range(nw, nw + n)
        nw += n
    if share_stages:
        i, j = share_stages
        assert stage_sizes[j] <= stage_sizes[i]
        start[j] = start[i] + stage_sizes[i] - stage_sizes[j]
    assert nw <= 400, "at most 400 classifiers: the tables stay far inside the block's LDS"
    # features: rejection-sampled until the 3 x 3 cells stay inside the window at every scale of the case
    nf = nw + 3
    feats = np.zeros((nf, 4), np.int8)
    for i in range(nf):
        while True:
            fw, fh = rs.randint(1, max(2, min(window_w // 3, 7))), rs.randint(1, max(2, min(window_h // 3, 7)))
            f = (rs.randint(0, window_w - 3 * fw + 1), rs.randint(0, window_h - 3 * fh + 1), fw, fh)
            if all(feature_inside(f, window_w, window_h, sc) for sc in fit_scales):
                feats[i] = f
                break
    mag = lambda: (np.asarray(MAGNITUDES)[rs.choice(3, nw, p=(0.2, 0.3, 0.5))] * rs.uniform(0.5, 1.5, nw) * rs.choice((-1.0, 1.0), nw)).astype(F32)
    left, right = mag(), mag()
    left[dead], right[dead] = np.nan, np.nan
    nsub = rs.randint(1, 9, nw).astype(np.uint16)
    off = (np.cumsum(nsub) - nsub).astype(np.uint16)
    subsets = rs.randint(-2 ** 31, 2 ** 31 - 1, int(nsub.sum())).astype(np.int32)
    if share_subsets:  # the second classifier of the largest stage looks its code up in the first one's words
        a = int(start[int(np.argmax(stage_sizes))])
        nsub[a + 1] = min(nsub[a + 1], nsub[a])
        off[a + 1] = off[a]
    nan_stage = None
    if specials:
        fl = next(s for s in range(ns) if stage_sizes[s] > 12)
        left[int(start[fl])] = -0.0
        right[int(start[fl]) + 3] = np.inf
        nan_stage = stage_sizes.index(2)
    casc = Cascade(window_w, window_h, features=feats.reshape(-1), weak_feature_idx=rs.randint(0, nf, nw).astype(np.uint16),
                   weak_left_val=left, weak_right_val=right, weak_subset_offset=off, weak_num_subsets=nsub, subsets=subsets,
                   stage_weak_start=start, stage_nweaks=np.asarray(stage_sizes, np.uint16), stage_threshold=np.zeros(ns, F32))
    # thresholds: stage by stage over the windows of the frame's scale-1 scan that are still alive
    bits = lookup_bits(casc, frame).reshape(nw, -1)
    alive = np.arange(bits.shape[1])
    for s in range(ns):
        assert len(alive) >= 201, "stage %d: too few windows left to draw a threshold from" % s
        sums = stage_sums(casc, s, bits[:, alive])
        sample = rs.choice(len(alive), 201, replace=False)
        ranked = sample[np.argsort(sums[sample], kind="stable")]
        pick = ranked[60]
        if stage_sizes[s] > 12:
            # among the sampled windows of rank 50..70, the one nearest rank 60 whose sum comes out SMALLER when it is added
            # in reverse order and when it is added in float64: that window passes (sum == threshold) only with the
            # reference's own adds
            b = bits[:, alive[ranked]]
            rev, f64 = stage_sums(casc, s, b, order=-1), stage_sums(casc, s, b, dtype=np.float64)
            for r in sorted(range(50, 71), key=lambda r: abs(r - 60)):
                if rev[r] < sums[ranked[r]] and f64[r] < np.float64(sums[ranked[r]]):
                    pick = ranked[r]
                    break
        casc.stage_threshold[s] = np.nan if s == nan_stage else sums[pick]
        alive = alive[passes(sums, casc.stage_threshold[s])]
    return casc


# ---- the named cases -------------------------------------------------------------------------------------------------------
def _params(cap_later):
    """(max_rects, scale_factor, min_scale, max_scale, step); cap_later is set per case from the oracle's uncapped scan"""
    return [(UNCAPPED, 1.2, 1.0, 3.0, 1), (7, 1.2, 1.0, 3.0, 1), (cap_later, 1.2, 1.0, 3.0, 1), (UNCAPPED, 1.3, 0.5, 2.0, 1),
            (UNCAPPED, 1.25, 1.0, 2.5, 2), (7, 1.3, 0.5, 2.0, 2)]


SCANS = ((1.2, 1.0, 3.0), (1.3, 0.5, 2.0), (1.25, 1.0, 2.5))  # the (scale_factor, min_scale, max_scale) of _params
WINDOW_SCALES = (1.0, 0.5, 2.3)                               # the scales check_windows asks gs_lbp_window for

# name: (seed, stage sizes in evaluation order, window, frame (w, h), generator options)
SPECS = {
    # every way of deciding a stage in one cascade, the window-per-lane form last; stored out of order
    "every_branch": (1, [3, 12, 13, 31, 32, 33, 40], (24, 24), (150, 110), {}),
    # the dense phase starts on the float sum; classifiers that no stage reaches; a tall window
    "float_sum_first": (1, [13, 5, 70], (20, 28), (163, 117), {"unreachable": (9, 4)}),
    # one stage: k_lbp_cascade by rule (no adaptive re-packing below three stages); a wide window
    "single_stage": (1, [40], (31, 17), (181, 131), {}),
    # two stages, the last one by truth table; the smallest window
    "two_stages": (1, [33, 2], (12, 12), (150, 110), {}),
    # one-word and many-word truth tables next to a stage that has none; two classifiers share their subset words
    "truth_tables": (2, [1, 1, 11, 12, 65], (31, 17), (200, 150), {"share_subsets": True}),
    # two windows per wave, three times over, the last stage publishing; stages 0 and 2 are the SAME classifiers
    "two_windows_per_wave": (1, [32, 32, 32], (20, 28), (150, 110), {"share_stages": (0, 2)}),
    # 64 classifiers in the dense phase, a 31-classifier float sum last; stage 2's classifiers are the tail of stage 0's
    "wide_first": (1, [64, 6, 31], (12, 12), (163, 117), {"share_stages": (0, 2), "unreachable": (5,)}),
    # NaN threshold (passes everything), +inf and -0.0 leaves
    "specials": (2, [12, 14, 2, 33], (24, 24), (181, 131), {"specials": True}),
}
NAMES = tuple(SPECS)


class Case:
    pass


_CASES = {}


def frames_of(o, w, h, seed):
    """the three frames of a case: a synth frame, a sobel edge map (no Otsu) and a flat one"""
    synth = Oracle.synth(w, h, seed)
    return {"synth": synth, "edges": o.sobel(o.blur(Oracle.synth(w, h, seed + 100), 1)), "flat": np.full((h, w), 90, np.uint8)}


def case(name, o):
    """the named case, built once: cascade, frames, integral images, parameter sets; the two input conditions asserted"""
    if name in _CASES:
        return _CASES[name]
    seed, sizes, (ww, wh), (w, h), opts = SPECS[name]
    c = Case()
    c.name, c.sizes, c.w, c.h = name, sizes, w, h
    c.frames = frames_of(o, w, h, 10 + len(name))
    scales = sorted({float(s[0]) for scan in SCANS for s in scan_scales(ww, wh, w, h, *scan)} | set(WINDOW_SCALES))
    c.casc = structured_cascade(seed, sizes, ww, wh, c.frames["synth"], fit_scales=scales, **opts)
    assert_features_inside(c.casc, scales)
    assert 0.5 in scales and max(scales) > 2.0
    c.ii = {k: o.integral(f) for k, f in c.frames.items()}
    c.entering = check_stage_coverage(c, o)
    check_order_sensitivity(c)
    full = o.lbp_detect(c.casc, c.ii["synth"], UNCAPPED, 1.2, 1.0, 3.0, 1)
    n0 = int((full["w"] == ww).sum())  # detections of the first scale (every later window is larger)
    assert n0 > 7 and len(full) - n0 >= 2, "%s: the caps must cut inside the first and inside a later scale (%d, %d)" % (name, n0, len(full))
    c.params = _params(n0 + (len(full) - n0 + 1) // 2)
    c.expected = {}
    _CASES[name] = c
    return c


def truncated(casc, ns):
    """the cascade cut to its first ns stages (same classifier tables)"""
    t = Cascade(casc.window_w, casc.window_h, **{k: getattr(casc, k) for k in (
        "features", "weak_feature_idx", "weak_left_val", "weak_right_val", "weak_subset_offset", "weak_num_subsets", "subsets")},
        stage_weak_start=casc.stage_weak_start[:ns], stage_nweaks=casc.stage_nweaks[:ns], stage_threshold=casc.stage_threshold[:ns])
    return t


def check_stage_coverage(c, o):
    """condition 1, by the oracle on truncated cascades -> windows of the scale-1 scan that enter each stage (+ that pass the last)"""
    casc, ii = c.casc, c.ii["synth"]
    total = (c.w - casc.window_w + 1) * (c.h - casc.window_h + 1)
    n = [total] + [len(o.lbp_detect(truncated(casc, s), ii, UNCAPPED, 1.2, 1.0, 1.0, 1)) for s in range(1, casc.nstages + 1)]
    for s in range(casc.nstages):
        assert n[s] >= 256, "%s: only %d windows enter stage %d" % (c.name, n[s], s)
        assert n[s + 1] >= 1, "%s: stage %d passes nothing" % (c.name, s)
        if np.isnan(casc.stage_threshold[s]):
            assert casc.stage_nweaks[s] == 2 and n[s + 1] == n[s], "%s: a NaN threshold rejects nothing" % c.name
        else:
            assert n[s + 1] < n[s], "%s: stage %d rejects nothing" % (c.name, s)
    return n


def check_order_sensitivity(c):
    """condition 2, in numpy: over the windows of the scale-1 scan that reach a stage of more than 12 classifiers"""
    casc = c.casc
    bits = lookup_bits(casc, c.frames["synth"]).reshape(casc.nweaks, -1)
    alive = np.arange(bits.shape[1])
    for s in range(casc.nstages):
        b, thr = bits[:, alive], casc.stage_threshold[s]
        verdict = passes(stage_sums(casc, s, b), thr)
        assert len(alive) == c.entering[s] and int(verdict.sum()) == c.entering[s + 1], "the numpy restatement and the oracle disagree"
        if casc.stage_nweaks[s] > 12:
            rev = passes(stage_sums(casc, s, b, order=-1), thr)
            f64 = passes(stage_sums(casc, s, b, dtype=np.float64), thr)
            assert (rev != verdict).any(), "%s stage %d: adding in reverse order changes no verdict" % (c.name, s)
            assert (f64 != verdict).any(), "%s stage %d: adding in float64 changes no verdict" % (c.name, s)
        alive = alive[verdict]


def expected(c, o, frame, params):
    """the oracle's rectangles, computed once per (case, frame, parameters)"""
    key = (frame, params)
    if key not in c.expected:
        c.expected[key] = o.lbp_detect(c.casc, c.ii[frame], *params)
        c.expected[key].setflags(write=False)
    return c.expected[key]


# ---- what both back ends run -----------------------------------------------------------------------------------------------
# (tune key, value): key 14 = 0 the rule, 1 k_lbp_cascade everywhere, 2..4 each tile shape wherever it fits; key 4 = 1 one dense
# phase, no re-packing (k_lbp_cascade); key 15 = first + 16 * tenths moves k_lbp_tile's dense-to-pair switch: 241 = one dense
# stage, then pairs whatever is alive (every stage from the second on is decided in the pair phase); 7 = dense to the last
# stage (every stage of these cascades is decided in the dense phase, the dense phase publishes)
KEYS = ((14, 0), (14, 1), (14, 2), (14, 3), (14, 4), (4, 1), (15, 241), (15, 7))
KEY_IDS = tuple("key%d_%d" % kv for kv in KEYS)


ALL_FRAMES = ("synth", "edges", "flat")
ALL_PARAMS = tuple(range(6))


def check_detect(g, o, mems, name, key, val, plan=None):
    """gs_lbp_detect through the drop-in under one kernel choice, host and device tables.  plan: {frame: indices into the
    case's parameter sets}; None = every parameter set on every frame"""
    c = case(name, o)
    plan = plan or {f: ALL_PARAMS for f in ALL_FRAMES}
    tables = {(f, m.kind): m.put(c.ii[f]) for f in plan for m in mems}
    try:
        g.tune(key, val)
        for f, which in plan.items():
            for p in (c.params[i] for i in which):
                for m in mems:
                    assert_same(g.lbp_detect(c.casc, tables[f, m.kind], *p), expected(c, o, f, p),
                                "%s, %s frame, %s table, key %d = %d, gs_lbp_detect max=%d sf=%g [%g,%g] step=%d" % ((name, f, m.kind, key, val) + p))
    finally:
        g.tune(key, 0)


def check_batch(g, o, mem, name, which=(0, 2, 3, 5)):
    """gsh_lbp_detect_batch on the three frames in one call, then once more with the counting kernels armed; `which`: indices
    into the case's parameter sets"""
    c = case(name, o)
    order = ("edges", "flat", "synth")
    ii = mem.put(np.stack([c.ii[f] for f in order]))
    dc = g.cascade_create(c.casc)
    try:
        for p in (c.params[i] for i in which):
            want = [expected(c, o, f, p) for f in order]
            total = g.lbp_window_count(c.casc, c.w, c.h, *p[1:])
            cap = max(len(r) for r in want) + 2 if p[0] == UNCAPPED else p[0]
            got = []
            for armed in (False, True):
                rects, counts = mem.zeros((3, cap, 4), np.uint32), mem.zeros(3, np.uint32)
                ev = mem.zeros(4, np.int64)
                g.lbp_count_evaluated(ev if armed else None)
                try:
                    g.lbp_detect_batch(dc, ii, rects, counts, cap, *p[1:])
                    g.sync()
                finally:
                    g.lbp_count_evaluated(None)
                r, n, e = np.asarray(mem.get(rects)).view(np.uint32).reshape(3, cap, 4), np.asarray(mem.get(counts)).view(np.uint32), np.asarray(mem.get(ev))
                for k, f in enumerate(order):
                    assert int(n[k]) == min(len(want[k]), cap), "%s batch %s frame %r armed=%s: %d rectangles, expected %d" % (name, f, p, armed, n[k], len(want[k]))
                    w = want[k][:cap]
                    assert_same(r[k, :len(w)], np.stack([w["x"], w["y"], w["w"], w["h"]], 1).astype(np.uint32).reshape(-1, 4),
                                "%s batch %s frame %r armed=%s" % (name, f, p, armed))
                got.append((r.copy(), n.copy()))
                if armed:  # gsh_lbp_window_count counts one frame's scan
                    assert 0 < int(e[0]) <= 3 * total, (name, p, e, total)
                    if p[0] == UNCAPPED:
                        assert int(e[0]) == 3 * total, "nothing to skip when the cap cannot be reached: %r of %d" % (e, 3 * total)
                    assert int(e[1]) >= int(e[0]), "every evaluated window evaluates a classifier"
            assert np.array_equal(got[0][1], got[1][1]) and np.array_equal(got[0][0], got[1][0]), "the counting kernels return other rectangles"
    finally:
        dc.close()


def window_spots(c, o):
    """(x, y, scale) for gs_lbp_window: the origin, the last window that fits and one past it in x and in y, at scale 1, 0.5
    and 2.3, and the first and the last detection of the uncapped scale-1 scan (so both verdicts occur)"""
    ww, wh = c.casc.window_w, c.casc.window_h
    first = expected(c, o, "synth", c.params[0])
    first = first[first["w"] == ww]
    return [(0, 0, 1.0), (c.w - ww, c.h - wh, 1.0), (c.w - ww + 1, c.h - wh, 1.0), (c.w - ww, c.h - wh + 1, 1.0),
            (0, 0, 0.5), (c.w - ww // 2, c.h - wh // 2, 0.5), (c.w - ww // 2 + 1, 0, 0.5), (17, 9, 0.5),
            (0, 0, 2.3), (3, 5, 2.3), (c.w - int(F32(ww) * F32(2.3)), c.h - int(F32(wh) * F32(2.3)), 2.3), (c.w - ww, 0, 2.3),
            (int(first[0]["x"]), int(first[0]["y"]), 1.0), (int(first[-1]["x"]), int(first[-1]["y"]), 1.0)]


def check_windows(g, o, mems, name):
    """gs_lbp_window at window_spots(), on every frame, host and device tables"""
    c = case(name, o)
    spots = window_spots(c, o)
    for f in ALL_FRAMES:
        verdicts = set()
        for m in mems:
            t = m.put(c.ii[f])
            for (x, y, s) in spots:
                want = o.lbp_window(c.casc, c.ii[f], x, y, s)
                assert g.lbp_window(c.casc, t, x, y, s) == want, "%s, %s frame, %s table: gs_lbp_window(%d, %d, %g)" % (name, f, m.kind, x, y, s)
                verdicts.add(want)
        if f == "synth":
            assert verdicts == {0, 1}
