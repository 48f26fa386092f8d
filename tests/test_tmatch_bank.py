"""gsh_match_templates_batch and gsh_locate_templates_batch on the kernel-logic emulator: the cases of
tests/tmatch_bank_cases.py against the oracle (and the compiled reference wherever oracle/_ref was built), the locate
epilogue's block reduction and atomic maximum under permuted block and thread orders, and the precondition aborts.
tests/test_gpu_tmatch_bank.py runs the same cases on an MI355X."""
import os
import subprocess
import sys

import pytest

import tmatch_bank_cases as tb
from parity_cases import Mem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_SO = os.path.join(ROOT, "tests", "emu", "libgs_kernel_emu.so")
MEM = Mem("host")


@pytest.fixture(scope="module")
def oracles(oracle):
    from oracle import pyoracle
    return [oracle] + ([pyoracle.Oracle("reference")] if pyoracle.have_reference() else [])


def test_the_rule_restated_for_the_tests():
    """takes() on sizes worked by hand: 512 columns are 32 slots a row, 513 are 33; 32768 taps is the accumulator's bound"""
    assert tb.takes(512, 64) and not tb.takes(513, 1) and tb.takes(7, 5) and tb.takes(16, 1)
    assert tb.takes(256, 128) and not tb.takes(256, 129)


@pytest.mark.parametrize("key27", tb.BOTH, ids=("bank", "loop"))
@pytest.mark.parametrize("case", tb.ALL_CHECKS, ids=lambda f: f.__name__[6:])
def test_tmatch_bank_emulated(emu, oracles, case, key27):
    case(emu, MEM, oracles, key27)


def test_default_rule_emulated(emu, oracles):
    tb.check_default_rule(emu, MEM, oracles)


@pytest.mark.parametrize("index", range(6), ids=lambda i: "schedule%d" % i)
def test_bank_under_permuted_block_and_thread_orders(emu, oracles, index):
    """cases 5, 6 and 2 on the bank kernel dealt over the six schedules of tests/test_emu_schedules.py (each case under two of
    them): maps and keys are the same bytes whatever order blocks, waves and lanes run in"""
    from test_emu_schedules import SCHEDULES, set_schedule
    case = (tb.check_first_maximum, tb.check_chunks, tb.check_group_boundary)[index % 3]
    try:
        set_schedule(emu, *SCHEDULES[index])
        case(emu, MEM, oracles, 2)
    finally:
        set_schedule(emu, 0, 0, 0)


# ---- preconditions ---------------------------------------------------------------------------------------------------------
PROLOGUE = '''
import sys, numpy as np
sys.path.insert(0, %r)
import grayskull_amd as G
g = G.Grayskull(%r)
img = np.zeros((3, 12, 20), np.uint8)
res = np.full((3, 2, 9, 14), 0x5a, np.uint8)
best = np.full((3, 2, 2), 0x5a5a5a5a, np.uint32)
score = np.full((3, 2), 0x5a, np.uint8)
winner = np.full(3, 0x5a5a5a5a, np.uint32)
g.match_templates_batch(res, img, np.zeros((2, 4, 7), np.uint8))   # fine
g.locate_templates_batch(img, np.zeros((2, 12, 20), np.uint8), best, score, winner)  # fine: templates as large as the frame
assert not best.any() and (score == 255).all() and not winner.any()
''' % (ROOT, EMU_SO)


@pytest.mark.parametrize("call, cond", [
    ("g.match_templates_batch(res, img, np.zeros((2, 4, 21), np.uint8))", b"tw <= iw && th <= ih"),
    ("g.locate_templates_batch(img, np.zeros((2, 13, 7), np.uint8), best)", b"tw <= iw && th <= ih"),
    ("g.c.gsh_match_templates_batch(img.ctypes.data, 20, 12, 3, None, 7, 4, 2, res.ctypes.data)", b"tmpl"),
    ("g.c.gsh_match_templates_batch(img.ctypes.data, 20, 12, 3, img.ctypes.data, 7, 4, 2, None)", b"result"),
    ("g.c.gsh_locate_templates_batch(img.ctypes.data, 20, 12, 3, img.ctypes.data, 7, 4, 2, None, None, None)", b"best"),
    ("g.c.gsh_match_templates_batch(img.ctypes.data, 20, 12, 3, img.ctypes.data, 0, 4, 2, res.ctypes.data)", b"tw > 0"),
], ids=["template_wider_than_frame", "template_higher_than_frame", "no_bank", "no_result", "no_best", "zero_width"])
def test_preconditions_abort_like_gs_assert(emu, tmp_path, call, cond):
    prog = tmp_path / "bad_bank.py"
    prog.write_text(PROLOGUE + call + "\n")
    r = subprocess.run([sys.executable, str(prog)], capture_output=True)
    assert r.returncode == -6, r
    assert b"Assertion failed:" in r.stderr and cond in r.stderr, r.stderr


def test_prologue_alone_passes(emu, tmp_path):
    prog = tmp_path / "good_bank.py"
    prog.write_text(PROLOGUE)
    r = subprocess.run([sys.executable, str(prog)], capture_output=True)
    assert r.returncode == 0, r
