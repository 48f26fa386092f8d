"""gsh_orb_extract_pyramid_batch (the pyramid ORB of the reference's default build, glibc trig on the host) and
gsh_orb_pyramid_buffer_fill_batch on the kernel-logic emulator: the cases of tests/orb_pyramid_libm_cases.py against
Oracle("port"), k_orb_moments_levels / k_orb_brief_levels / k_orb_buffer_fill under permuted block and thread orders, and
the precondition aborts.  tests/test_gpu_orb_pyramid_libm_batch.py runs the same cases on an MI355X."""
import os
import subprocess
import sys

import pytest

import orb_pyramid_libm_cases as lc
from guard_cases import Guarded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_SO = os.path.join(ROOT, "tests", "emu", "libgs_kernel_emu.so")


def test_both_entries_are_exported(emu):
    import grayskull_amd
    for name in ("gsh_orb_extract_pyramid_batch", "gsh_orb_pyramid_buffer_fill_batch"):
        assert name in grayskull_amd.EXPORTED_SYMBOLS and hasattr(emu.c, name)
    assert emu.orb_pyramid_batch_times() == [0.0] * 5  # the emulator has no clock to report


@pytest.mark.parametrize("case", lc.ORB_CHECKS, ids=lambda f: f.__name__[6:])
def test_orb_pyramid_libm_batch_emulated(emu, case):
    gd = Guarded("host", seed=5)
    case(emu, gd)
    assert gd.checked == case.checks


@pytest.mark.parametrize("w, h, n_levels, L, n", lc.FILL_CASES, ids=lambda v: str(v))
def test_buffer_fill_emulated(emu, w, h, n_levels, L, n):
    gd = Guarded("host", seed=w + n)
    lc.check_fill(emu, gd, w, h, n_levels, L, n)
    assert gd.checked == lc.check_fill.checks


def test_buffer_fill_writes_nothing_emulated(emu):
    gd = Guarded("host", seed=8)
    lc.check_fill_writes_nothing(emu, gd)
    assert gd.checked == lc.check_fill_writes_nothing.checks


@pytest.mark.parametrize("index", range(6), ids=lambda i: "schedule%d" % i)
def test_under_permuted_block_and_thread_orders(emu, index):
    """the quota, remainder and cap cases and a 263 x 261 fill dealt over the six schedules of tests/test_emu_schedules.py:
    the same bytes whatever order blocks, waves and lanes run in"""
    from test_emu_schedules import SCHEDULES, set_schedule
    case = (lc.check_quotas_differ_in_one_batch, lc.check_remainder_is_not_per, lc.check_cap_per_frame)[index % 3]
    gd = Guarded("host", seed=6)
    try:
        set_schedule(emu, *SCHEDULES[index])
        case(emu, gd)
        lc.check_fill(emu, gd, 263, 261, 4, 4, 2)
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
one = np.zeros(g.orb_pyramid_buffer_bytes(70, 70, 2), np.uint8)
kps = np.zeros((2, 8, 12), np.uint32)
cnt = np.full(2, 0x5a5a5a5a, np.uint32)
g.orb_extract_pyramid_batch(img, buf, kps, cnt, 8, 20, 2)            # fine
assert (cnt == 0).all()
g.orb_pyramid_buffer_fill_batch(buf, one, 70, 70, 2, 2)              # fine
p = lambda a: a.ctypes.data
''' % (ROOT, EMU_SO)


@pytest.mark.parametrize("call, cond", [
    ("g.c.gsh_orb_extract_pyramid_batch(None, 70, 70, 2, p(buf), p(kps), p(cnt), None, 8, 20, 2)", b"img_dev && buffer_dev && kps_dev && counts_dev"),
    ("g.c.gsh_orb_extract_pyramid_batch(p(img), 70, 70, 2, None, p(kps), p(cnt), None, 8, 20, 2)", b"img_dev && buffer_dev && kps_dev && counts_dev"),
    ("g.c.gsh_orb_extract_pyramid_batch(p(img), 70, 70, 2, p(buf), None, p(cnt), None, 8, 20, 2)", b"img_dev && buffer_dev && kps_dev && counts_dev"),
    ("g.c.gsh_orb_extract_pyramid_batch(p(img), 70, 70, 2, p(buf), p(kps), None, None, 8, 20, 2)", b"img_dev && buffer_dev && kps_dev && counts_dev"),
    ("g.c.gsh_orb_extract_pyramid_batch(p(img), 0, 70, 2, p(buf), p(kps), p(cnt), None, 8, 20, 2)", b"w > 0 && h > 0"),
    ("g.c.gsh_orb_extract_pyramid_batch(p(img), 70, 0, 2, p(buf), p(kps), p(cnt), None, 8, 20, 2)", b"w > 0 && h > 0"),
    ("g.c.gsh_orb_pyramid_buffer_fill_batch(None, p(one), 70, 70, 2, 2)", b"buffer_dev && single_dev"),
    ("g.c.gsh_orb_pyramid_buffer_fill_batch(p(buf), None, 70, 70, 2, 2)", b"buffer_dev && single_dev"),
    ("g.c.gsh_orb_pyramid_buffer_fill_batch(p(buf), p(buf) + one.size, 70, 70, 2, 2)", b"single_dev + off <= buffer_dev"),
], ids=["no_img", "no_buffer", "no_kps", "no_counts", "w_zero", "h_zero", "fill_no_buffer", "fill_no_single", "fill_overlap"])
def test_preconditions_abort_like_gs_assert(emu, tmp_path, call, cond):
    prog = tmp_path / "bad_pyramid_libm.py"
    prog.write_text(PROLOGUE + call + "\n")
    r = subprocess.run([sys.executable, str(prog)], capture_output=True)
    assert r.returncode == -6, r
    assert b"Assertion failed:" in r.stderr and cond in r.stderr, r.stderr


def test_prologue_alone_passes(emu, tmp_path):
    prog = tmp_path / "good_pyramid_libm.py"
    prog.write_text(PROLOGUE)
    r = subprocess.run([sys.executable, str(prog)], capture_output=True)
    assert r.returncode == 0, r
