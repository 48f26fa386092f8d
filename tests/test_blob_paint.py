"""gsh_blob_paint_batch, gsh_blob_largest_batch and gsh_threshold_batch_dev_offset on the kernel-logic emulator: the
hand cases and shapes of tests/blob_paint_cases.py against its numpy restatement of the painting rule, then records
from the compiled reference's gs_blobs.  tests/test_gpu_blob_paint.py runs the same on an MI355X."""
import os
import subprocess
import sys

import numpy as np
import pytest

import blob_cases as bc
import blob_paint_cases as pc
from test_blobs import emu_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_on_a_case_worked_by_hand():
    """3 x 4 frame, one record (x 1, y 0, w 3, h 1): x1 = 0, x2 = min(4, 6) = 4, y1 = 0, y2 = min(3, 3) = 3 -> rows 0..3,
    columns 0..4: every pixel is covered, (y, 4) is (y + 1, 0), row 3 and (2, 4) are dropped"""
    img = np.array([[0, 255, 129, 128], [0, 0, 0, 0], [0, 0, 0, 200]], np.uint8)
    recs = np.zeros(1, pc.BLOB_DTYPE)
    recs[0]["x"], recs[0]["y"], recs[0]["w"], recs[0]["h"], recs[0]["area"] = 1, 0, 3, 1, 3
    pic, drop = pc.spec_paint(img, recs, 1)
    assert pic.tolist() == [[128, 255, 255, 128], [128, 128, 128, 128], [128, 128, 128, 255]]
    assert drop.tolist() == [12, 13, 14, 15, 16]
    pic, drop = pc.spec_paint(img, recs, 0)
    assert pic.tolist() == [[0, 255, 255, 0], [0, 0, 0, 0], [0, 0, 0, 255]] and drop.size == 0
    assert pc.largest(np.array([(0, 5), (0, 9), (0, 9), (0, 1)], [("label", "u4"), ("area", "u4")]), 4) == 1


def test_hand_cases_emulated(emu):
    pc.check_hand_cases(emu, pc.Host)


def test_shapes_and_band_heights_emulated(emu):
    pc.check_shapes(emu, pc.Host)


def test_batches_emulated(emu):
    pc.check_batches(emu, pc.Host)


def test_largest_emulated(emu):
    pc.check_largest(emu, pc.Host)


def test_threshold_offset_emulated(emu):
    pc.check_threshold_offset(emu, pc.Host)


def test_paint_preconditions_abort_like_gs_assert(emu, tmp_path):
    prog = tmp_path / "bad_paint.py"
    prog.write_text('''
import sys, numpy as np
sys.path.insert(0, %r)
import grayskull_amd as G
g = G.Grayskull(%r)
img = np.zeros((2, 4, 4), np.uint8)
g.blob_paint_batch(img[1:], img[:1], np.zeros((1, 2, 8), np.uint32), np.zeros(1, np.uint32))  # fine: no overlap
g.blob_paint_batch(img[:1], img[:1], np.zeros((1, 2, 8), np.uint32), np.zeros(1, np.uint32))
''' % (ROOT, os.path.join(ROOT, "tests", "emu", "libgs_kernel_emu.so")))
    r = subprocess.run([sys.executable, str(prog)], capture_output=True)
    assert r.returncode == -6, r
    assert b"Assertion failed:" in r.stderr and b"<= img" in r.stderr


def test_paint_of_reference_records_emulated(emu):
    """records from the compiled reference's gs_blobs on the frames of tests/test_blobs.py, whole and capped"""
    from oracle import pyoracle
    if not pyoracle.have_reference():
        pytest.skip("oracle/_ref/libgs_ref.so not built")
    ref = bc.Ref()
    for name, img in emu_frames():
        for cap in (2, 150, 1000):
            recs, _ = ref.blobs(img, cap)
            pc.check_against_spec(emu, pc.Host, img[None], [recs], "%s cap %d" % (name, cap), nblobs=cap)
