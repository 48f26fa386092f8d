"""gsh_match_template_batch, gsh_find_best_match_batch and gsh_locate_template_batch on the kernel-logic emulator: the cases
of tests/tmatch_batch_cases.py against the oracle (and the compiled reference wherever oracle/_ref was built), the locate
epilogue's atomic maximum under permuted block and thread orders, and the precondition aborts.
tests/test_gpu_tmatch_batch.py runs the same cases on an MI355X."""
import os
import subprocess
import sys

import pytest

import tmatch_batch_cases as tc
from parity_cases import Mem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_SO = os.path.join(ROOT, "tests", "emu", "libgs_kernel_emu.so")
MEM = Mem("host")


@pytest.fixture(scope="module")
def oracles(oracle):
    from oracle import pyoracle
    return [oracle] + ([pyoracle.Oracle("reference")] if pyoracle.have_reference() else [])


def test_the_rule_restated_for_the_tests():
    """plan() on shapes worked by hand.  1280 x 720 with a 64 x 64 template: result 1217 x 657, 10 x 11 = 110 whole tiles a
    frame: alone (and up to four frames, 440 blocks) split, from five frames (550) whole, banded since 64 > 32 rows.  A 4K
    frame with a 128 x 128 template has 30 x 32 = 960 tiles of its own.  16 x 16 has 256 taps: dot products, four results per thread at width 1280.
    A 16 x 2048 template keeps 2079 rows of 112 bytes resident in the split form (more than 150 KiB), so one small frame takes
    the dot products, and so does every batch of such frames: the route is a frame's, only the form is the launch's."""
    assert tc.plan(1280, 720, 64, 64, 1) == "split" and tc.plan(1280, 720, 64, 64, 4) == "split"
    assert tc.plan(1280, 720, 64, 64, 5) == "band" and tc.plan(1280, 720, 16, 32, 5) == "whole"
    assert tc.plan(3840, 2160, 128, 128, 1) == "band"
    assert tc.plan(1280, 720, 16, 16, 32) == "dot4" and tc.plan(1281, 720, 16, 16, 32) == "dot"
    assert tc.form(16, 2048, 100, 100, 1)[1] > tc.LDS_MAX and tc.plan(115, 2147, 16, 2048, 1) == "dot" == tc.plan(115, 2147, 16, 2048, 600)
    assert tc.plan(4111, 3071, 16, 2048, 1) == "band"  # 32 x 16 = 512 whole tiles: banded, 20 KiB
    assert tc.plan(640, 360, 64, 64, 32) == "band" and 5 * 5 * 32 == 800  # the filling launch of the GPU file


@pytest.mark.parametrize("case", tc.ALL_CHECKS, ids=lambda f: f.__name__[6:])
def test_tmatch_batch_emulated(emu, oracles, case):
    case(emu, MEM, oracles)


# ---- schedules: the key word of a frame receives the waves' maxima in any order ---------------------------------------------
@pytest.mark.parametrize("index", range(6), ids=lambda i: "schedule%d" % i)
def test_locate_under_permuted_block_and_thread_orders(emu, oracles, index):
    """cases 1, 6 and 7 dealt over the six schedules of tests/test_emu_schedules.py (each case under two of them): the maps,
    the batched argmax and the locate epilogue give the same bytes whatever order blocks, waves and lanes run in"""
    from test_emu_schedules import SCHEDULES, set_schedule
    case = (tc.check_whole_tiles, tc.check_first_maximum, tc.check_all_zero_map)[index % 3]
    try:
        set_schedule(emu, *SCHEDULES[index])
        case(emu, MEM, oracles)
    finally:
        set_schedule(emu, 0, 0, 0)


# ---- preconditions ---------------------------------------------------------------------------------------------------------
PROLOGUE = '''
import sys, numpy as np
sys.path.insert(0, %r)
import grayskull_amd as G
g = G.Grayskull(%r)
img = np.zeros((3, 12, 20), np.uint8)
res = np.full((3, 9, 14), 0x5a, np.uint8)
best = np.full((3, 2), 0x5a5a5a5a, np.uint32)
score = np.full(3, 0x5a, np.uint8)
g.match_template_batch(res, img, np.zeros((4, 7), np.uint8))       # fine: one template
g.match_template_batch(res, img, np.zeros((3, 4, 7), np.uint8))    # fine: one per frame
g.locate_template_batch(img, np.zeros((12, 20), np.uint8), best, score)  # fine: a template as large as the frame
assert not best.any() and (score == 255).all()
''' % (ROOT, EMU_SO)


@pytest.mark.parametrize("call, cond", [
    ("g.match_template_batch(res, img, np.zeros((2, 4, 7), np.uint8))", b"ntmpl == 1 || ntmpl == n"),
    ("g.locate_template_batch(img, np.zeros((2, 4, 7), np.uint8), best, score)", b"ntmpl == 1 || ntmpl == n"),
    ("g.match_template_batch(res, img, np.zeros((4, 21), np.uint8))", b"iw >= tw && ih >= th"),
    ("g.locate_template_batch(img, np.zeros((13, 7), np.uint8), best)", b"iw >= tw && ih >= th"),
    ("g.c.gsh_match_template_batch(img.ctypes.data, 20, 12, 3, None, 7, 4, 1, res.ctypes.data)", b"tmpl"),
    ("g.c.gsh_find_best_match_batch(res.ctypes.data, 14, 9, 3, None, None)", b"best"),
], ids=["two_templates_three_frames", "locate_two_templates", "template_wider_than_frame", "template_higher_than_frame",
        "no_template", "no_best"])
def test_preconditions_abort_like_gs_assert(emu, tmp_path, call, cond):
    prog = tmp_path / "bad_tmatch.py"
    prog.write_text(PROLOGUE + call + "\n")
    r = subprocess.run([sys.executable, str(prog)], capture_output=True)
    assert r.returncode == -6, r
    assert b"Assertion failed:" in r.stderr and cond in r.stderr, r.stderr


def test_prologue_alone_passes(emu, tmp_path):
    prog = tmp_path / "good_tmatch.py"
    prog.write_text(PROLOGUE)
    r = subprocess.run([sys.executable, str(prog)], capture_output=True)
    assert r.returncode == 0, r
