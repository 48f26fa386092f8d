"""gsh_match_orb_batch on the kernel-logic emulator: the cases of tests/match_batch_cases.py against the oracle (and the
compiled reference wherever oracle/_ref was built), the merge of the waves' states under permuted block and thread orders,
and the precondition aborts.  tests/test_gpu_match_batch.py runs the same cases on an
MI355X."""
import os
import subprocess
import sys

import pytest

import match_batch_cases as mc
from parity_cases import Mem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_SO = os.path.join(ROOT, "tests", "emu", "libgs_kernel_emu.so")
MEM = Mem("host")


@pytest.fixture(scope="module")
def oracles(oracle):
    from oracle import pyoracle
    return [oracle] + ([pyoracle.Oracle("reference")] if pyoracle.have_reference() else [])


def test_the_split_restated_for_the_tests():
    """plan() on sizes worked by hand, T = 64 descriptors per tile, S = 16 slices.  500 train descriptors: slices of
    ceil(500 / 16) = 32, the last one 500 - 15 * 32 = 20: 16 waves, half a tile each.  2500: slices of 157 = 64 + 64 + 29,
    three tiles, 16 waves (15 * 157 = 2355 < 2500).  65: slices of 5, 13 waves.  1: one wave, one descriptor.  1025 = S T + 1:
    slices of 65, a full tile and one descriptor more.  1008 = S (T - 1) and 1024 = S T: one tile, one short of full and full."""
    assert (mc.T, mc.S) == (64, 16)
    assert mc.plan(500) == (32, 16, 1) and mc.plan(2500) == (157, 16, 3)
    assert mc.plan(65) == (5, 13, 1) and mc.plan(1) == (1, 1, 1) and mc.plan(0) == (0, 0, 0)
    assert mc.plan(63) == (4, 16, 1) and mc.plan(64) == (4, 16, 1) and mc.plan(129) == (9, 15, 1)
    assert mc.plan(1025) == (65, 16, 2) and mc.plan(1008) == (63, 16, 1) and mc.plan(1024) == (64, 16, 1)
    assert mc.plan(2049) == (129, 16, 3)
    assert set(mc.TRAIN_SIZES) <= {nt for _, nt in mc.CROSSED} | {mc.S * mc.T + 1} and set(mc.QUERY_SIZES) <= {nq for nq, _ in mc.CROSSED} | {2049}


@pytest.mark.parametrize("case", mc.ALL_CHECKS, ids=lambda f: f.__name__[6:])
def test_match_batch_emulated(emu, oracles, case):
    case(emu, MEM, oracles)


# ---- schedules: the waves' states merge to the same result in any order ----------------------------------------------------
@pytest.mark.parametrize("index", range(6), ids=lambda i: "schedule%d" % i)
def test_merge_under_permuted_block_and_thread_orders(emu, oracles, index):
    """cases 1, 3 and 6 dealt over the six schedules of tests/test_emu_schedules.py (each case under two of them): the same
    records whatever order blocks, waves and lanes run in"""
    from test_emu_schedules import SCHEDULES, set_schedule
    case = (mc.check_sizes_in_one_batch, mc.check_set_sharing, mc.check_distance_limits)[index % 3]
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
k = np.zeros((3, 5, 12), np.uint32)
k[:, :, 4:] = np.arange(3 * 5 * 8).reshape(3, 5, 8)
n = np.full(3, 5, np.uint32)
m = np.full((3, 4, 3), 0x5a5a5a5a, np.uint32)
c = np.full(3, 0x5a5a5a5a, np.uint32)
g.match_orb_batch(k, n, k, n, m, c, 60.0)         # fine: three against three, aliased
assert (c == 4).all() and (m[:, :, 0] == m[:, :, 1]).all()
g.match_orb_batch(k[0], None, k, n, m, c, 60.0)   # fine: one query set
g.match_orb_batch(k, n, k[1], None, m, c, 60.0)   # fine: one train set
p = lambda a: a.ctypes.data
''' % (ROOT, EMU_SO)


@pytest.mark.parametrize("call, cond", [
    ("g.match_orb_batch(k[:2], n, k, n, m, c, 60.0)", b"nset1 == 1 || nset1 == n"),
    ("g.match_orb_batch(k, n, k[:2], n, m, c, 60.0)", b"nset2 == 1 || nset2 == n"),
    ("g.c.gsh_match_orb_batch(None, 5, p(n), 3, p(k), 5, p(n), 3, 3, p(m), p(c), 4, 60.0)", b"k1 && k2 && matches && counts"),
    ("g.c.gsh_match_orb_batch(p(k), 5, p(n), 3, p(k), 5, p(n), 3, 3, None, p(c), 4, 60.0)", b"k1 && k2 && matches && counts"),
    ("g.c.gsh_match_orb_batch(p(k), 5, p(n), 3, p(k), 5, p(n), 3, 3, p(m), None, 0, 60.0)", b"k1 && k2 && matches && counts"),
    ("g.c.gsh_match_orb_batch(p(k), 0, p(n), 3, p(k), 5, p(n), 3, 3, p(m), p(c), 4, 60.0)", b"cap1 > 0 && cap2 > 0"),
    ("g.c.gsh_match_orb_batch(p(k), 5, p(n), 3, p(k), 0, None, 1, 3, p(m), p(c), 4, 60.0)", b"cap1 > 0 && cap2 > 0"),
], ids=["two_query_sets_three_pairs", "two_train_sets_three_pairs", "no_k1", "no_matches", "no_counts_even_without_records", "cap1_zero",
        "cap2_zero"])
def test_preconditions_abort_like_gs_assert(emu, tmp_path, call, cond):
    prog = tmp_path / "bad_match.py"
    prog.write_text(PROLOGUE + call + "\n")
    r = subprocess.run([sys.executable, str(prog)], capture_output=True)
    assert r.returncode == -6, r
    assert b"Assertion failed:" in r.stderr and cond in r.stderr, r.stderr


def test_prologue_alone_passes(emu, tmp_path):
    prog = tmp_path / "good_match.py"
    prog.write_text(PROLOGUE)
    r = subprocess.run([sys.executable, str(prog)], capture_output=True)
    assert r.returncode == 0, r
