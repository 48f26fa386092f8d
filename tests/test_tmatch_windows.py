"""gsh_match_template_windows_batch, gsh_locate_template_windows_batch and gsh_search_windows_batch on the kernel-logic
emulator: the cases of tests/tmatch_window_cases.py against the oracle chain crop -> match_template -> find_best_match (and
the compiled reference wherever oracle/_ref was built), the staging, the band walk and the locate epilogue's atomic maximum
under permuted block and thread orders, and the precondition aborts.  tests/test_gpu_tmatch_windows.py runs the same cases
on an MI355X."""
import os
import subprocess
import sys

import pytest

import tmatch_window_cases as tw
from parity_cases import Mem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_SO = os.path.join(ROOT, "tests", "emu", "libgs_kernel_emu.so")
MEM = Mem("host")


@pytest.fixture(scope="module")
def oracles(oracle):
    from oracle import pyoracle
    return [oracle] + ([pyoracle.Oracle("reference")] if pyoracle.have_reference() else [])


def test_the_plan_restated_for_the_tests():
    """form() on sizes worked by hand: 64 x 64 stages 24-dword rows beside 16-dword template rows, (6144 - 31 * 24) / 40 = 135
    rows fit; 120 x 100 takes 70 rows of 100; 256 columns are one band, 257 are two (72-dword rows beside 64: 28 rows)"""
    assert tw.form(64, 64) == (64, 64) and tw.form(120, 100) == (70, 120) and tw.form(1, 1) == (1, 1)
    assert tw.form(256, 100) == (28, 256) and tw.form(257, 28) == (28, 256) and tw.form(4000, 29) == (28, 256)


@pytest.mark.parametrize("case", tw.ALL_CHECKS, ids=lambda f: f.__name__[6:])
def test_tmatch_windows_emulated(emu, oracles, case):
    case(emu, MEM, oracles)


@pytest.mark.parametrize("index", range(6), ids=lambda i: "schedule%d" % i)
def test_windows_under_permuted_block_and_thread_orders(emu, oracles, index):
    """cases 3, 5 and 6 dealt over the six schedules of tests/test_emu_schedules.py (each case under two of them): maps and
    keys are the same bytes whatever order blocks, waves and lanes run in"""
    from test_emu_schedules import SCHEDULES, set_schedule
    case = (tw.check_window_sizes, tw.check_ties_and_extremes, tw.check_invalid_windows)[index % 3]
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
tmpl = np.zeros((4, 7), np.uint8)
win = np.array([(1, 2, 10, 8), (0, 0, 16, 9), (4, 3, 16, 9)], np.uint32)
fo = np.array([2, 0, 1, 1], np.uint32)
res = np.full((3, 6, 10), 0x5a, np.uint8)
best = np.full((4, 2), 0x5a5a5a5a, np.uint32)
score = np.full(4, 0x5a, np.uint8)
g.match_template_windows_batch(res, img, tmpl, win, (16, 9))   # fine
g.locate_template_windows_batch(img, tmpl, win, (16, 9), best, score, fo)  # fine
assert [tuple(b) for b in best[:3]] == [(1, 2), (0, 0), (4, 3)] and (score[:3] == 255).all() and score[3] == 0x5a
g.locate_template_windows_batch(img, tmpl, np.zeros((4, 4), np.uint32), (20, 12), best, None, fo)  # fine: nwin > n with frame_of
assert (best == 0xffffffff).all()
I, T, W, F, R, B = (a.ctypes.data for a in (img, tmpl, win, fo, res, best))
''' % (ROOT, EMU_SO)


@pytest.mark.parametrize("call, cond", [
    ("g.match_template_windows_batch(res, img, tmpl, win, (6, 9))", b"tw <= max_ww && th <= max_wh"),
    ("g.match_template_windows_batch(res, img, tmpl, win, (21, 9))", b"max_ww <= iw && max_wh <= ih"),
    ("g.c.gsh_locate_template_windows_batch(I, 20, 12, 3, T, 7, 4, 2, W, F, 3, 16, 9, B, None)", b"ntmpl == 1 || ntmpl == nwin"),
    ("g.c.gsh_locate_template_windows_batch(I, 20, 12, 3, T, 7, 4, 1, None, F, 3, 16, 9, B, None)", b"windows_dev"),
    ("g.c.gsh_locate_template_windows_batch(I, 20, 12, 3, T, 7, 4, 1, W, F, 3, 16, 9, None, None)", b"best"),
    ("g.c.gsh_match_template_windows_batch(I, 20, 12, 3, T, 7, 4, 1, W, F, 3, 16, 9, None)", b"result"),
    ("g.c.gsh_locate_template_windows_batch(I, 20, 12, 2, T, 7, 4, 1, W, None, 3, 16, 9, B, None)", b"nwin <= n"),
], ids=["template_larger_than_bound", "bound_larger_than_frame", "templates_neither_1_nor_nwin", "no_windows", "no_best", "no_result",
        "more_windows_than_frames_without_frame_of"])
def test_preconditions_abort_like_gs_assert(emu, tmp_path, call, cond):
    prog = tmp_path / "bad_windows.py"
    prog.write_text(PROLOGUE + call + "\n")
    r = subprocess.run([sys.executable, str(prog)], capture_output=True)
    assert r.returncode == -6, r
    assert b"Assertion failed:" in r.stderr and cond in r.stderr, r.stderr


def test_prologue_alone_passes(emu, tmp_path):
    prog = tmp_path / "good_windows.py"
    prog.write_text(PROLOGUE)
    r = subprocess.run([sys.executable, str(prog)], capture_output=True)
    assert r.returncode == 0, r
