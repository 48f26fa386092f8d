"""gs_blobs / gs_blob_corners / gs_perspective_correct (ref grayskull.h:330-444) on the kernel-logic emulator:
hand-derived cases that need no reference build, then random and structured frames against the compiled
reference (oracle/_ref/libgs_ref.so).  tests/test_gpu_blobs.py runs the same on an MI355X."""
import os
import subprocess
import sys

import numpy as np
import pytest

import blob_cases as bc
from grayskull_amd import BLOB_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")

W = 255
# ref test.c:231-258: the reference's own unit test image and its expected records
TEST_C_IMAGE = np.array([[W, W, 0, 0, W, 0],
                         [W, 0, 0, W, W, 0],
                         [0, 0, W, W, 0, 0],
                         [W, W, W, 0, 0, W],
                         [0, W, 0, 0, 0, W]], np.uint8)


def check_hand_cases(g):
    """every hand-derived case on the library `g` (emulator or GPU)"""
    # ref test.c: labels 1, 2, 6 -- not consecutive; the labels array worked out by hand
    recs, labels = g.blobs(TEST_C_IMAGE, 10)
    assert [tuple(int(r[f]) for f in bc.FIELDS) for r in recs] == \
        [(1, 3, 0, 0, 2, 2, 0, 0), (2, 9, 0, 0, 5, 5, 2, 2), (6, 2, 5, 3, 1, 2, 5, 3)]
    assert labels.tolist() == [[1, 1, 0, 0, 2, 0], [1, 0, 0, 2, 2, 0], [0, 0, 2, 2, 0, 0], [2, 2, 2, 0, 0, 6],
                               [0, 2, 0, 0, 0, 6]]

    # a comb: 40 teeth, each a start pixel, merged by the bar below into ONE blob labelled 1; an isolated pixel
    # after it is start pixel number 41, so its label is 41, not 2
    comb = np.zeros((6, 80), np.uint8)
    comb[0:4, 0:80:2] = W
    comb[4, :] = W
    comb[5, 79] = 0
    comb[5, 2] = 0
    comb = np.vstack([comb, np.zeros((1, 80), np.uint8)])
    comb[6, 50] = W
    recs, labels = g.blobs(comb, 100)
    assert [int(r["label"]) for r in recs] == [1, 41]
    assert int(recs[0]["area"]) == 40 * 4 + 80 and int(recs[1]["area"]) == 1
    bc.assert_blobs_equal((recs, labels), bc.spec_blobs(comb, 100), "comb")

    # the cap is hit mid-row: start pixel 3 (P) at x = 4 of row 0 gets no label, neither do the pixels right of it
    # that are reached only from the left; row 1 picks them up through the top of label 2's pixels
    img = np.array([[W, 0, W, 0, W, W, W, 0, W],
                    [0, 0, W, W, W, W, W, W, W],
                    [W, 0, 0, 0, 0, 0, 0, 0, W]], np.uint8)
    recs, labels = g.blobs(img, 2)
    assert labels.tolist() == [[1, 0, 2, 0, 0, 0, 0, 0, 0],
                               [0, 0, 2, 2, 2, 2, 2, 2, 2],
                               [0, 0, 0, 0, 0, 0, 0, 0, 2]]
    bc.assert_blobs_equal((recs, labels), bc.spec_blobs(img, 2), "cap mid-row")
    bc.assert_blobs_equal(g.blobs(img, 1), bc.spec_blobs(img, 1), "cap 1")

    # all foreground, all background
    full = np.full((37, 150), 200, np.uint8)
    recs, labels = g.blobs(full, 5)
    assert len(recs) == 1 and int(recs[0]["area"]) == 37 * 150 and (labels == 1).all()
    assert (int(recs[0]["w"]), int(recs[0]["h"]), int(recs[0]["cx"]), int(recs[0]["cy"])) == (150, 37, 74, 18)
    recs, labels = g.blobs(np.full((9, 70), 127, np.uint8), 5)
    assert len(recs) == 0 and not labels.any()

    # frames of width 1 and of height 1
    rng = np.random.default_rng(7)
    for shape in ((1, 1), (1, 200), (57, 1), (1, 64), (64, 1)):
        img = bc.random_mask(rng, shape[0], shape[1], 0.6)
        for cap in (1, 3, 1000):
            bc.assert_blobs_equal(g.blobs(img, cap), bc.spec_blobs(img, cap), "shape %s cap %d" % (shape, cap))

    # the centroid's x sum wraps at 2^32 like the reference's unsigned cx: 2 x 70000 pixels sum to 4.9e9
    wide = np.full((2, 70000), W, np.uint8)
    recs, labels = g.blobs(wide, 4)
    sx = 2 * (70000 * 69999 // 2)
    assert sx >= 2 ** 32 and int(recs[0]["cx"]) == (sx % 2 ** 32) // (2 * 70000) and (labels == 1).all()

    # the reference's u16 label counter: 65535 isolated pixels (a 1 x 131070 row, every other pixel set) get labels
    # 1 .. 65535; with nblobs >= 65535 its counter wraps to 0 after the last one and it returns m = 0 (its merge and
    # compact loops run to next - 1 = -1) -- so does the library; with nblobs = 65534 the last pixel is P: 65534 blobs
    row = np.zeros((1, 131070), np.uint8)
    row[0, ::2] = W
    ranks = np.arange(1, 65536)
    for nb in (65535, 70000):
        recs, labels = g.blobs(row, nb)
        assert len(recs) == 0 and np.array_equal(labels[0, ::2], ranks) and not labels[0, 1::2].any(), nb
    recs, labels = g.blobs(row, 65534)
    assert len(recs) == 65534 and np.array_equal(recs["label"], ranks[:-1]) and np.array_equal(recs["x"], 2 * ranks[:-1] - 2)
    assert np.array_equal(labels[0, :-2:2], ranks[:-1]) and labels[0, -2] == 0
    # one more start pixel: the reference is undefined there (it writes blobs[-1]); the library keeps the same rule,
    # m = 0, with the labels of nblobs = 65535 (start pixel 65536 is P)
    row = np.zeros((1, 131072), np.uint8)
    row[0, ::2] = W
    recs, labels = g.blobs(row, 65535)
    assert len(recs) == 0 and np.array_equal(labels[0, :-2:2], ranks) and labels[0, -2] == 0

    # corners: several pixels share the extreme x + y / x - y -- the first in (y, x) order wins (strict < / >)
    diamond = np.zeros((9, 9), np.uint8)
    for y in range(9):
        for x in range(9):
            if abs(x - 4) + abs(y - 4) <= 4 and (x + y) % 3 != 1:
                diamond[y, x] = W
    diamond[0:2, 0:2] = W
    diamond[1, 2] = W
    recs, labels = g.blobs(diamond, 50)
    for r in recs:
        assert g.blob_corners(diamond, labels, r) == bc.spec_corners(diamond, labels, r)
    # the triangle x + y >= 5: its six pixels on x + y = 5 tie for tl, the first in raster order is (5, 0)
    anti = np.where(np.indices((6, 6)).sum(0) >= 5, W, 0).astype(np.uint8)
    recs, labels = g.blobs(anti, 10)
    assert g.blob_corners(anti, labels, recs[0]) == bc.spec_corners(anti, labels, recs[0]) == [(5, 0), (5, 0), (5, 5), (0, 5)]
    # a record taken literally: a box that wraps scans nothing, a label that is absent -> centroid four times
    fake = np.zeros(1, BLOB_DTYPE)[0]
    fake["label"], fake["x"], fake["y"], fake["w"], fake["h"], fake["cx"], fake["cy"] = 2, 3, 1, 2 ** 32 - 2, 4, 7, 8
    assert g.blob_corners(diamond, labels, fake) == [(7, 8)] * 4
    fake["w"], fake["label"] = 100, 77
    assert g.blob_corners(diamond, labels, fake) == [(7, 8)] * 4

    # perspective: a 1-wide destination divides 0 by 0 -- the NaN clamps to src.w - 1 through the ternaries
    src = (np.arange(24 * 31) * 7 % 251).astype(np.uint8).reshape(24, 31)
    for dw, dh, c in ((1, 9, [(2, 3), (20, 1), (28, 22), (1, 17)]), (9, 1, [(2, 3), (20, 1), (28, 22), (1, 17)]),
                      (13, 11, [(0, 0), (30, 0), (30, 23), (0, 23)]), (16, 12, [(5, 4), (25, 2), (29, 20), (3, 21)]),
                      (7, 5, [(40, 3), (50, 60), (2, 90), (1, 1)])):
        out = np.zeros((dh, dw), np.uint8)
        g.perspective_correct(out, src, c)
        assert np.array_equal(out, bc.spec_perspective(dw, dh, src, c)), (dw, dh, c)


def test_hand_derived_cases_emulated(emu):
    check_hand_cases(emu)


def test_blob_struct_layout_strict_c99(tmp_path):
    src = tmp_path / "blob_abi.c"
    src.write_text(r'''
#include <stddef.h>
#include <stdio.h>
#include "grayskull_hip.h"
int main(void) {
  gs_label l = 65535;
  printf("%zu %zu %zu %zu %zu %zu %u\n", sizeof(struct gs_blob), offsetof(struct gs_blob, label),
         offsetof(struct gs_blob, area), offsetof(struct gs_blob, box), offsetof(struct gs_blob, centroid),
         sizeof(gs_label), (unsigned)l);
  return 0;
}''')
    exe = tmp_path / "blob_abi"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INC, str(src), "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).decode().split() == ["32", "0", "4", "8", "24", "2", "65535"]


def test_blobs_precondition_aborts_like_gs_assert(emu, tmp_path):
    prog = tmp_path / "bad_blobs.py"
    prog.write_text('''
import sys, numpy as np
sys.path.insert(0, %r)
import grayskull_amd as G
g = G.Grayskull(%r)
g.blobs(np.zeros((4, 4), np.uint8), 0)
''' % (ROOT, os.path.join(ROOT, "tests", "emu", "libgs_kernel_emu.so")))
    r = subprocess.run([sys.executable, str(prog)], capture_output=True)
    assert r.returncode == -6, r
    assert b"Assertion failed:" in r.stderr and b"nblobs > 0" in r.stderr


# ---- against the compiled reference ---------------------------------------------------------------------------------
def _ref():
    from oracle import pyoracle
    if not pyoracle.have_reference():
        pytest.skip("oracle/_ref/libgs_ref.so not built")
    return bc.Ref()


emu_frames = bc.emu_frames  # the generator lives in blob_cases.py: tests/cap_sweep_cases.py sweeps the same frames


def test_blobs_match_reference_emulated(emu):
    ref = _ref()
    for name, img in emu_frames():
        starts = bc.start_count(img)
        for cap in sorted({1, 2, 150, 1000, 65534, max(starts - 1, 1), starts, starts + 1}):
            got, want = emu.blobs(img, cap), ref.blobs(img, cap)
            bc.assert_blobs_equal(got, want, "%s cap %d (%d start pixels)" % (name, cap, starts))


def test_label_counter_wrap_matches_reference_emulated(emu):
    """exactly 65535 start pixels, nblobs around 65535: the reference is defined there and returns m = 0 once its u16
    counter has wrapped"""
    ref = _ref()
    for w, step in ((131070, 2), (131100, 2)):
        row = np.zeros((1, w), np.uint8)
        row[0, :131070:step] = W
        row[0, 131068:] = W  # for w = 131100 the 65535th start pixel opens a run to the end of the row
        for nb in (65534, 65535, 65536, 70000):
            bc.assert_blobs_equal(emu.blobs(row, nb), ref.blobs(row, nb), "w %d nblobs %d" % (w, nb))


def test_corners_and_perspective_match_reference_emulated(emu):
    ref = _ref()
    rng = np.random.default_rng(5)
    for name, img in emu_frames()[::3]:
        recs, labels = ref.blobs(img, 1000)
        for r in recs[:: max(1, len(recs) // 6)]:
            assert emu.blob_corners(img, labels, r) == ref.corners(img, labels, r), name
        src = bc.blurred_noise(rng, 30, 45)
        c = ref.corners(img, labels, recs[int(np.argmax(recs["area"]))])
        for dw, dh in ((17, 23), (1, 5), (5, 1)):
            out = np.zeros((dh, dw), np.uint8)
            emu.perspective_correct(out, src, c)
            assert np.array_equal(out, ref.perspective(dw, dh, src, c)), (name, dw, dh)
