"""gsh_crop_batch, gsh_resize_batch, gsh_resize_nn_batch and gsh_crop_resize_batch on the kernel-logic emulator: the cases
of tests/geom_batch_cases.py against the oracle (and the compiled reference wherever oracle/_ref was built), the staged
kernel under permuted block and thread orders, the precondition aborts, and the `resize` / `crop` verbs of gsbatch, which
are one batch call per slice.  tests/test_gpu_geom_batch.py runs the same cases on an MI355X."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import geom_batch_cases as gc
from parity_cases import Mem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_SO = os.path.join(ROOT, "tests", "emu", "libgs_kernel_emu.so")
MEM = Mem("host")


@pytest.fixture(scope="module")
def oracles(oracle):
    from oracle import pyoracle
    return [oracle] + ([pyoracle.Oracle("reference")] if pyoracle.have_reference() else [])


def test_the_rule_restated_for_the_tests():
    """plan() on shapes worked by hand: 3840x2160 -> 1920x1080 (four source pixels per result pixel) stages 516 x 19 bytes
    per block of 8 rows (16 rows would need 516 x 35 = 18060 > 16384); 1280x720 -> 1920x1080 176 x 14 at 16 rows;
    3840x2160 -> 640x360 has 36 source pixels per result pixel and 612x816 -> 300x400 4.16: gathered; gsh_tune(25, 2) would
    stage the first at 4 rows, 1540 x 27 bytes"""
    assert gc.plan(1920, 1080, 3840, 2160) == (8, 516 * 19)
    assert gc.plan(1920, 1080, 1280, 720) == (16, 176 * 14)
    assert gc.plan(640, 360, 3840, 2160) == (16, 0) and gc.plan(300, 400, 612, 816) == (16, 0)
    assert gc.plan(640, 360, 3840, 2160, any_density=True) == (4, 1540 * 27)
    assert gc.plan(240, 135, 3840, 2160, any_density=True) == (16, 0)  # 4 rows would need 4100 x 60 bytes
    # at most 65535 bands: 8 x 1000 -> 8 x 1048560 is 65535 bands of 16 rows, 8 x 1048700 would be 65544 and takes bands of
    # ceil(1048700 / 65535) = 17 -> 20 rows with the 8 x 4 bytes of LDS sized for 16; the gather form is capped the same way
    assert gc.plan(8, 1048560, 8, 1000) == (16, 32) and gc.plan(8, 1048561, 8, 1000) == (20, 32)
    assert gc.plan(8, 1048700, 8, 1000) == (20, 32) and (1048700 + 19) // 20 == 52435
    assert gc.plan(8, 1048700, 800, 100000) == (20, 0) and gc.plan(8, 65535 * 20 + 1, 8, 1000) == (24, 32)


@pytest.mark.parametrize("case", gc.ALL_CHECKS, ids=lambda f: f.__name__[6:])
def test_geom_batch_emulated(emu, oracles, case):
    case(emu, MEM, oracles)


# ---- schedules: the staged kernel has LDS and a barrier -----------------------------------------------------------------
@pytest.mark.parametrize("index", range(6), ids=lambda i: "schedule%d" % i)
def test_staged_kernel_under_permuted_block_and_thread_orders(emu, oracles, index):
    """the tile-edge and scale-class cases dealt over the six schedules of tests/test_emu_schedules.py: in a fixed
    shuffled order schedule k takes every third case from k % 3 on, so every case runs under two permuted schedules"""
    from test_emu_schedules import SCHEDULES, set_schedule
    cases = [(gc.check_tile_edge_case, c) for c in gc.TILE_EDGE_CASES + gc.ODD_SOURCE_CASES] + [(gc.check_scale_case, c) for c in gc.SCALE_CASES]
    random.Random(len(cases)).shuffle(cases)
    try:
        set_schedule(emu, *SCHEDULES[index])
        for check, c in cases[index % 3::3]:
            check(emu, MEM, oracles, c)
    finally:
        set_schedule(emu, 0, 0, 0)


# ---- preconditions ---------------------------------------------------------------------------------------------------
PROLOGUE = '''
import sys, numpy as np
sys.path.insert(0, %r)
import grayskull_amd as G
g = G.Grayskull(%r)
a = np.zeros((4, 6, 40), np.uint8)
b = np.zeros((2, 3, 20), np.uint8)
g.resize_batch(b, a[0:2])            # fine
g.crop_batch(b, a[2:4], 20, 3, 20, 3)  # fine: the roi touches the right and bottom edges
''' % (ROOT, EMU_SO)


@pytest.mark.parametrize("call, cond", [
    ("g.resize_batch(a[1:3], a[0:2])", b"apart("),
    ("g.resize_batch(np.zeros((2, 3, 0), np.uint8), a[0:2])", b"dw > 0"),
    ("g.crop_batch(b, a[0:2], 21, 3, 20, 3)", b"roi.w <= sw - roi.x"),
    ("g.crop_batch(b, a[0:2], 0xfffffff0, 0, 0x20, 3)", b"roi.x <= sw"),
    ("g.crop_resize_batch(a[1:3], a[0:2], np.zeros((2, 4), np.uint32))", b"apart("),
], ids=["dst_overlaps_src", "dw_0", "roi_outside", "roi_wraps", "patches_overlap_src"])
def test_preconditions_abort_like_gs_assert(emu, tmp_path, call, cond):
    prog = tmp_path / "bad_geom.py"
    prog.write_text(PROLOGUE + call + "\n")
    r = subprocess.run([sys.executable, str(prog)], capture_output=True)
    assert r.returncode == -6, r
    assert b"Assertion failed:" in r.stderr and cond in r.stderr, r.stderr


def test_prologue_alone_passes(emu, tmp_path):
    prog = tmp_path / "good_geom.py"
    prog.write_text(PROLOGUE)
    r = subprocess.run([sys.executable, str(prog)], capture_output=True)
    assert r.returncode == 0, r


def test_batches_of_nothing_launch_nothing(emu):
    """n == 0 / npatches == 0 return before any check (the overlapping, zero-sized arguments below would abort) or launch"""
    a = np.full((2, 5, 40), 3, np.uint8)
    emu.resize_batch(a[0:0], a[0:0])
    emu.resize_batch(a[0:0], a[0:0], nearest=True)
    emu.crop_batch(a[0:0], a[0:0], 50, 50, 0, 0)
    emu.crop_resize_batch(a[0:0], a, np.zeros((0, 4), np.uint32))
    emu.crop_resize_batch(a, a[0:0], np.zeros((2, 4), np.uint32))
    assert (a == 3).all()


# ---- the driver ------------------------------------------------------------------------------------------------------
def test_gsbatch_resize_and_crop_verbs_emulated(tmp_path, oracle):
    """`resize 200 120 : crop 8 4 96 64 : resize 333 77` over five files of two sizes, two frames per slice so that the
    group of three spans two slices: the oracle's chain per file, and the reference's nanomagick pipe where
    oracle/_ref/nano_ref was built"""
    from tests.test_gsbatch import build_emu, chain_args, nano_chain, oracle_chain, write_pgm
    from tests.util import read_pgm
    exe = build_emu(tmp_path)
    nano = os.path.join(ROOT, "oracle", "_ref", "nano_ref")
    chain = [("resize", ["200", "120"]), ("crop", ["8", "4", "96", "64"]), ("resize", ["333", "77"])]
    rng = np.random.default_rng(4)
    files, imgs = [], []
    for k, (h, w) in enumerate(((96, 160), (101, 131), (96, 160), (101, 131), (96, 160))):
        img = rng.integers(0, 256, (h, w), dtype=np.uint8)
        p = str(tmp_path / ("in%d.pgm" % k))
        write_pgm(p, img)
        files.append(p), imgs.append(img)
    outdir = tmp_path / "out"
    outdir.mkdir()
    env = dict(os.environ, GSBATCH_SLICE_BYTES=str(333 * 77 * 2))
    r = subprocess.run([exe, "-o", str(outdir), *chain_args(chain), "--", *files], capture_output=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr.decode()[-800:]
    for i, (f, img) in enumerate(zip(files, imgs)):
        got = read_pgm(str(outdir / os.path.basename(f)))
        assert np.array_equal(got, oracle_chain(oracle, img, chain)), f
        if os.path.exists(nano):
            exp, err = nano_chain(nano, chain, f, tmp_path, "ref%d" % i)
            assert exp is not None, err
            assert np.array_equal(got, read_pgm(exp)), f
