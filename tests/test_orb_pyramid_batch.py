"""gsh_pyramid_batch and gsh_orb_extract_pyramid_batch_nostdlib on the kernel-logic emulator: the cases of
tests/orb_pyramid_batch_cases.py against the oracle, k_pyramid and the level kernels under permuted block and thread
orders, and the precondition aborts.  tests/test_gpu_orb_pyramid_batch.py runs the same cases on an MI355X."""
import os
import subprocess
import sys

import pytest

import orb_pyramid_batch_cases as oc
from guard_cases import Guarded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_SO = os.path.join(ROOT, "tests", "emu", "libgs_kernel_emu.so")


def test_the_layout_restated_for_the_tests():
    """dims() and plane_sizes() on sizes worked by hand: 263 x 261 halves to 131 x 130, 65 x 65, 32 x 32; 128 x 64 stops at
    64 x 32 (32 x 16 is too low); 96 x 80 at 48 x 40; nine levels are four; none is none"""
    assert oc.dims(263, 261, 4) == [(263, 261), (131, 130), (65, 65), (32, 32)] == oc.dims(263, 261, 9)
    assert oc.dims(128, 64, 3) == [(128, 64), (64, 32)] and oc.dims(96, 80, 3) == [(96, 80), (48, 40)]
    assert oc.dims(64, 64, 2) == [(64, 64), (32, 32)] and oc.dims(63, 64, 2) == [(63, 64)] and oc.dims(64, 64, 0) == []
    assert oc.plane_sizes(96, 80, 3) == [48 * 40, 96 * 80, 48 * 40]
    assert sum(oc.plane_sizes(203, 171, 3)) == oc.Oracle.orb_pyramid_buffer_bytes(203, 171, 3)
    assert [c[3] for c in oc.PYRAMID_CASES] == [len(oc.dims(*c[:3])) for c in oc.PYRAMID_CASES]


@pytest.mark.parametrize("w, h, n_levels, L", oc.PYRAMID_CASES, ids=lambda v: str(v))
def test_pyramid_batch_emulated(emu, w, h, n_levels, L):
    gd = Guarded("host", seed=w + h)
    oc.check_pyramid(emu, gd, w, h, n_levels, L)
    assert gd.checked == oc.check_pyramid.checks


def test_pyramid_level_rules_emulated(emu):
    gd = Guarded("host", seed=4)
    oc.check_pyramid_level_rules(emu, gd)
    assert gd.checked == oc.check_pyramid_level_rules.checks


@pytest.mark.parametrize("case", oc.ORB_CHECKS, ids=lambda f: f.__name__[6:])
def test_orb_pyramid_batch_emulated(emu, case):
    gd = Guarded("host", seed=5)
    case(emu, gd)
    assert gd.checked == case.checks


@pytest.mark.parametrize("index", range(6), ids=lambda i: "schedule%d" % i)
def test_under_permuted_block_and_thread_orders(emu, index):
    """the quota, remainder and cap cases and the 263 x 261 pyramid dealt over the six schedules of
    tests/test_emu_schedules.py: the same bytes whatever order blocks, waves and lanes run in"""
    from test_emu_schedules import SCHEDULES, set_schedule
    case = (oc.check_quotas_differ_in_one_batch, oc.check_remainder_is_not_per, oc.check_cap_per_frame)[index % 3]
    gd = Guarded("host", seed=6)
    try:
        set_schedule(emu, *SCHEDULES[index])
        case(emu, gd)
        oc.check_pyramid(emu, gd, 263, 261, 4, 4)
    finally:
        set_schedule(emu, 0, 0, 0)
    assert gd.checked == case.checks + 1


# ---- preconditions ---------------------------------------------------------------------------------------------------------
PROLOGUE = '''
import sys, numpy as np
sys.path.insert(0, %r)
import grayskull_amd as G
g = G.Grayskull(%r)
img = np.zeros((2, 70, 70), np.uint8)
buf = np.zeros(g.orb_pyramid_batch_buffer_bytes(70, 70, 2, 2), np.uint8)
kps = np.zeros((2, 8, 12), np.uint32)
cnt = np.full(2, 0x5a5a5a5a, np.uint32)
g.orb_extract_pyramid_batch_nostdlib(img, buf, kps, cnt, 8, 20, 2)   # fine
assert (cnt == 0).all()
g.pyramid_batch(buf, img, 2)                                         # fine
p = lambda a: a.ctypes.data
''' % (ROOT, EMU_SO)


@pytest.mark.parametrize("call, cond", [
    ("g.c.gsh_orb_extract_pyramid_batch_nostdlib(None, 70, 70, 2, p(buf), p(kps), p(cnt), None, 8, 20, 2)", b"img_dev && buffer_dev && kps_dev && counts_dev"),
    ("g.c.gsh_orb_extract_pyramid_batch_nostdlib(p(img), 70, 70, 2, None, p(kps), p(cnt), None, 8, 20, 2)", b"img_dev && buffer_dev && kps_dev && counts_dev"),
    ("g.c.gsh_orb_extract_pyramid_batch_nostdlib(p(img), 70, 70, 2, p(buf), None, p(cnt), None, 8, 20, 2)", b"img_dev && buffer_dev && kps_dev && counts_dev"),
    ("g.c.gsh_orb_extract_pyramid_batch_nostdlib(p(img), 70, 70, 2, p(buf), p(kps), None, None, 8, 20, 2)", b"img_dev && buffer_dev && kps_dev && counts_dev"),
    ("g.c.gsh_orb_extract_pyramid_batch_nostdlib(p(img), 0, 70, 2, p(buf), p(kps), p(cnt), None, 8, 20, 2)", b"w > 0 && h > 0"),
    ("g.c.gsh_orb_extract_pyramid_batch_nostdlib(p(img), 70, 0, 2, p(buf), p(kps), p(cnt), None, 8, 20, 2)", b"w > 0 && h > 0"),
    ("g.c.gsh_pyramid_batch(None, p(img), 70, 70, 2, 2)", b"levels_dev && img_dev"),
], ids=["no_img", "no_buffer", "no_kps", "no_counts", "w_zero", "h_zero", "pyramid_no_levels"])
def test_preconditions_abort_like_gs_assert(emu, tmp_path, call, cond):
    prog = tmp_path / "bad_pyramid.py"
    prog.write_text(PROLOGUE + call + "\n")
    r = subprocess.run([sys.executable, str(prog)], capture_output=True)
    assert r.returncode == -6, r
    assert b"Assertion failed:" in r.stderr and cond in r.stderr, r.stderr


def test_prologue_alone_passes(emu, tmp_path):
    prog = tmp_path / "good_pyramid.py"
    prog.write_text(PROLOGUE)
    r = subprocess.run([sys.executable, str(prog)], capture_output=True)
    assert r.returncode == 0, r
