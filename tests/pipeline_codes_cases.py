"""The coded chunks of gsh_edge_pipeline_batch (gs_stencil.cpp; key 28 = GSH_TUNE_PIPELINE_CODES), shared by
tests/test_emu_pipeline_codes.py (emulator, host memory) and tests/test_gpu_pipeline_codes.py (product library, device memory).

A call that is cut into chunks (key 5) runs its chunks after the first through the fused kernel's coded mode: 4-bit codes of
the edge values around a guess of each frame's Otsu threshold, expanded by k_expand_codes where the threshold fell into the
15-level window [b, b + 14], b = clamp(guess, 8, 248) - 8 (a hit), redone by the repair launch where it did not (a miss).
Every check compares dst, thr and hist with the oracle chain and with the unsplit call (key 5 = -1), which never takes the
coded path.  The references are computed once per input set and shared."""
import numpy as np

from oracle.pyoracle import Oracle

KEY_CHUNK, KEY_BAND, KEY_CODES = 5, 0, 28
LAG = 2  # kCodeGuessLag (gs_internal.h): the rule takes frame j's guess from frame j two chunks back (chunk 1: one back)


class Host:
    """the emulator: every buffer is host memory"""
    def __init__(self, g):
        self.g = g

    def put(self, a):
        return np.ascontiguousarray(a).copy()

    def get(self, x):
        return x

    def sync(self):
        pass


class Dev:
    """the product library: device tensors"""
    def __init__(self, g):
        self.g = g

    def put(self, a):
        import torch
        return torch.from_numpy(np.array(a)).cuda()  # a copy: the shared references are read-only

    def get(self, x):
        return x.cpu().numpy()

    def sync(self):
        self.g.sync()


_REF = {}


def reference(oracle, key, make):
    """(src, final frames, thresholds, histograms) of the oracle chain blur(2) -> sobel -> Otsu -> threshold; cached"""
    if key not in _REF:
        src = make()
        edges = [oracle.sobel(oracle.blur(f, 2)) for f in src]
        thr = np.array([oracle.otsu_threshold(e) for e in edges], np.uint8)
        final = np.stack([oracle.threshold(e, int(t)) for e, t in zip(edges, thr)])
        hist = np.stack([oracle.histogram(e) for e in edges]).astype(np.uint32)
        for a in (src, final, thr, hist):
            a.setflags(write=False)
        _REF[key] = (src, final, thr, hist)
    return _REF[key]


def synth_frames(w, h, n, seed, shift_odd=0):
    return np.stack([Oracle.synth(w, h, seed + f) >> (shift_odd if f & 1 else 0) for f in range(n)])


def window_base(guess):
    return min(max(int(guess), 8), 248) - 8


def is_hit(t, guess):
    b = window_base(guess)
    return b <= int(t) <= b + 14


def call(b, src_np, keys, fill=7, dsrc=None):
    """one gsh_edge_pipeline_batch(tmp = NULL, radius 2) under the tune keys `keys` -> (dst, thr, hist) as numpy"""
    n = src_np.shape[0]
    dsrc = b.put(src_np) if dsrc is None else dsrc
    dst, thr, hist = b.put(np.full_like(src_np, fill)), b.put(np.zeros(n, np.uint8)), b.put(np.zeros((n, 256), np.int32))
    try:
        for k, v in keys.items():
            b.g.tune(k, v)
        b.g.edge_pipeline_batch(dst, None, dsrc, 2, hist, thr)
        b.sync()
    finally:
        for k in keys:
            b.g.tune(k, 0)
    return b.get(dst), b.get(thr), b.get(hist).view(np.uint32)


def check(b, ref, keys, what, dsrc=None):
    src, final, thr, hist = ref
    d, t, hs = call(b, src, keys, dsrc=dsrc)
    assert np.array_equal(t, thr), "%s: thr %s, oracle %s" % (what, t.tolist(), thr.tolist())
    assert np.array_equal(hs, hist), "%s: hist" % what
    bad = [f for f in range(len(src)) if not np.array_equal(d[f], final[f])]
    assert not bad, "%s: frames %s differ from the oracle (thr %s)" % (what, bad, thr.tolist())
    return d, t, hs


def check_unsplit(b, ref, what):
    """the unsplit call: today's byte path whatever key 28 says"""
    return check(b, ref, {KEY_CHUNK: -1}, what + ", unsplit")


# ---- shapes -----------------------------------------------------------------------------------------------------------------------
SHAPE_WIDTHS = (32, 48, 256, 1040)  # one strip pair, three strips, several lanes, a second wave (halo lanes)
SHAPE_HEIGHTS = (5, 6, 9, 12)
N_SHAPE = 7


def shapes(b, oracle, w):
    """bands of 3 and 4 rows over 3, 4, 7 and 10 output rows: odd and even row counts, a one-row last band (h = 6, T = 4;
    h = 9, T = 3; h = 12, T = 3), half-filled last pairs; 7 frames in chunks of 2 and of 3 (a one-frame tail chunk).  Under
    the rule and with every guess forced to frame 3's threshold, so that frame 3 (in a coded chunk for both chunk sizes) hits"""
    for h in SHAPE_HEIGHTS:
        ref = reference(oracle, ("shape", w, h), lambda: synth_frames(w, h, N_SHAPE, 300 + w + h))
        thr = ref[2]
        assert is_hit(thr[3], thr[3])
        check_unsplit(b, ref, "%dx%d" % (w, h))
        for T in (3, 4):
            for chunk in (2, 3):
                for codes in (0, int(thr[3]) + 1):
                    check(b, ref, {KEY_CHUNK: chunk, KEY_BAND: T, KEY_CODES: codes},
                          "%dx%d, bands of %d rows, chunks of %d, key 28 = %d" % (w, h, T, chunk, codes))


# ---- forced guesses ---------------------------------------------------------------------------------------------------------------
def window_edges(b, oracle):
    """4 x 128x33 in chunks of one frame (frames 1..3 coded): for each coded frame's threshold t, the window base b forced to
    t + 1 (miss), t (first hit), t - 14 (last hit), t - 15 (miss)"""
    ref = reference(oracle, ("edges", 128, 33), lambda: synth_frames(128, 33, 4, 4242))
    thr = ref[2]
    check_unsplit(b, ref, "128x33")
    done = set()
    for f in (1, 2, 3):
        t = int(thr[f])
        assert 15 <= t <= 239, "the test needs thresholds whose whole window range is reachable: %d" % t
        for base, hit in ((t + 1, False), (t, True), (t - 14, True), (t - 15, False)):
            guess = base + 8
            assert window_base(guess) == base and is_hit(t, guess) == hit
            if guess in done:
                continue
            done.add(guess)
            check(b, ref, {KEY_CHUNK: 1, KEY_CODES: guess + 1}, "128x33, chunks of 1, window base %d (frame %d: t = %d)" % (base, f, t))


def clamp_and_low_thresholds(b, oracle):
    """6 x 64x9 (thresholds of 2 - 12 by the oracle, some below 8) in chunks of one and of four frames: guesses 0 and 255 (the
    clamp: windows [0, 14] and [240, 254]), the rule, and a guess below 8 next to a threshold below 8"""
    ref = reference(oracle, ("low", 64, 9), lambda: synth_frames(64, 9, 6, 4242))
    thr = ref[2]
    assert thr[1:].min() < 8 and thr.max() <= 14, thr.tolist()
    assert all(is_hit(t, 0) for t in thr[1:]) and not any(is_hit(t, 255) for t in thr[1:])
    check_unsplit(b, ref, "64x9")
    for chunk in (1, 4):
        for codes in (1, 256, 0, 4):  # guess 0, guess 255, the rule, guess 3
            check(b, ref, {KEY_CHUNK: chunk, KEY_CODES: codes}, "64x9, chunks of %d, key 28 = %d" % (chunk, codes))


# ---- the rule, with real misses ---------------------------------------------------------------------------------------------------
def rule_outcomes(thr, chunk, lag=LAG):
    """hit / miss of every frame behind chunk 0 with the guess from `lag` chunks back, from the thresholds alone"""
    return [is_hit(thr[f], thr[f - chunk * min(lag, f // chunk)]) for f in range(chunk, len(thr))]


def rule_with_misses(b, oracle):
    """6 x 256x96 in chunks of one frame.  With every odd frame darkened (>> 2) neighbouring thresholds are 45 - 57 and 11 - 14:
    with the guess from the chunk before (key 28 = -3) every frame after the first misses, under the rule (two chunks back)
    frame 1 misses and later ones hit.  Without the darkening they are 54, 57, 47, 45, 51, 53: hits and misses either way"""
    dark = reference(oracle, ("dark", 256, 96), lambda: synth_frames(256, 96, 6, 4242, shift_odd=2))
    plain = reference(oracle, ("plain", 256, 96), lambda: synth_frames(256, 96, 6, 4242))
    assert not any(rule_outcomes(dark[2], 1, lag=1)), dark[2].tolist()
    for thr in (dark[2], plain[2]):
        for lag in ((1, 2) if thr is plain[2] else (2,)):
            mixed = rule_outcomes(thr, 1, lag)
            assert any(mixed) and not all(mixed), (lag, thr.tolist())
    for ref, name in ((dark, "odd frames darkened"), (plain, "plain")):
        check_unsplit(b, ref, "256x96 " + name)
        for codes in (0, -2, -3):  # the rule; the guess from two chunks / one chunk back
            check(b, ref, {KEY_CHUNK: 1, KEY_CODES: codes}, "256x96 %s, chunks of 1, key 28 = %d" % (name, codes))


# ---- key 28 = -1, repeated calls ----------------------------------------------------------------------------------------------------
def never_equals_byte_path(b, oracle):
    """key 28 = -1: every chunk on the byte path, as before the coded path existed"""
    ref = reference(oracle, ("plain", 256, 96), lambda: synth_frames(256, 96, 6, 4242))
    for chunk in (1, 4):
        check(b, ref, {KEY_CHUNK: chunk, KEY_CODES: -1}, "256x96, chunks of %d, key 28 = -1" % chunk)


def repeated_calls(b, oracle, reps=3):
    """the same buffers again and again without anything in between but the checks: the guesses, the code ring and the events
    of one call are reused by the next"""
    ref = reference(oracle, ("plain", 256, 96), lambda: synth_frames(256, 96, 6, 4242))
    dsrc = b.put(ref[0])
    for rep in range(reps):
        for chunk in (1, 2, 4):
            check(b, ref, {KEY_CHUNK: chunk}, "256x96, chunks of %d, call %d" % (chunk, rep), dsrc=dsrc)
