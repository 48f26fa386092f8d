"""gsh_morph_batch (iterated erode / dilate in ceil(n / 4) passes) on the kernel-logic emulator: the numpy restatement of
tests/morph_cases.py against the reference's own 3x3 loop, then the library against the restatement on every strip
flavour, band height, block shape and plane alternation; the precondition aborts; and the `morph` verb of gsbatch.
tests/test_gpu_morph_fused.py runs the same cases on an MI355X."""
import os
import subprocess
import sys

import numpy as np
import pytest

import morph_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_SO = os.path.join(ROOT, "tests", "emu", "libgs_kernel_emu.so")


def test_restatement_on_cases_worked_by_hand():
    a = np.zeros((5, 7), np.uint8)
    a[0, 6] = 9
    a[3, 2] = 200
    d2 = mc.spec(a, 2, True)
    want = np.zeros((5, 7), np.uint8)
    want[0:3, 4:7] = 9       # the corner pixel: a 3 x 3 square is what the image keeps of the 5 x 5 one
    want[1:5, 0:5] = 200     # rows 1..5 clipped to 1..4, columns 0..4
    assert np.array_equal(d2, want)
    b = np.full((1, 4), 255, np.uint8)
    b[0, 1] = 7
    assert mc.spec(b, 1, False).tolist() == [[7, 7, 7, 255]]  # what lies outside the image never lowers a minimum
    assert mc.spec(b, 3, False).tolist() == [[7, 7, 7, 7]]


def test_spec_equals_iterated_reference(oracle):
    """the C restatement always; the compiled reference's own loop too wherever oracle/_ref was built"""
    from oracle import pyoracle
    oracles = [oracle] + ([pyoracle.Oracle("reference")] if pyoracle.have_reference() else [])
    mc.check_spec_equals_iterated_reference(oracles)


@pytest.mark.parametrize("case", mc.ALL_CHECKS, ids=lambda f: f.__name__[6:])
def test_morph_batch_emulated(emu, case):
    case(emu, mc.Host)


PROLOGUE = '''
import sys, numpy as np
sys.path.insert(0, %r)
import grayskull_amd as G
g = G.Grayskull(%r)
a = np.zeros((4, 6, 40), np.uint8)
g.morph_batch(a[1:2], a[0:1], 9, 1, tmp=a[2:3])  # fine: three planes side by side
g.morph_batch(a[1:2], a[0:1], 4, 0, tmp=a[1:2])  # fine: one pass never touches tmp
''' % (ROOT, EMU_SO)


@pytest.mark.parametrize("call, cond", [
    ("g.morph_batch(a[1:2], a[0:1], 0, 1)", b"iterations >= 1"),
    ("g.morph_batch(a[0:2], a[1:3], 2, 1)", b"<= src"),
    ("g.morph_batch(a[0:2], a[2:4], 5, 0, tmp=a[1:3])", b"<= dst"),
], ids=["iterations_0", "dst_overlaps_src", "tmp_overlaps_dst"])
def test_morph_preconditions_abort_like_gs_assert(emu, tmp_path, call, cond):
    prog = tmp_path / "bad_morph.py"
    prog.write_text(PROLOGUE + call + "\n")
    r = subprocess.run([sys.executable, str(prog)], capture_output=True)
    assert r.returncode == -6, r
    assert b"Assertion failed:" in r.stderr and cond in r.stderr


def test_morph_batch_of_no_frames_launches_nothing(emu):
    a = np.full((1, 5, 40), 3, np.uint8)
    emu.morph_batch(a[0:0], a[0:0], 9, 1)  # n == 0: returns before the overlap checks and any launch
    assert (a == 3).all()


def test_gsbatch_morph_verb_emulated(tmp_path, oracle):
    """`morph dilate 9 : morph erode 10` (two stages of three passes each, the third plane in use) and `morph erode 3` over
    three files of two sizes: the bytes of the reference's nanomagick pipe where oracle/_ref/nano_ref was built, of the
    oracle's 3x3 operators iterated otherwise"""
    from tests.test_gsbatch import build_emu, chain_args, nano_chain, write_pgm
    from tests.util import read_pgm
    exe = build_emu(tmp_path)
    nano = os.path.join(ROOT, "oracle", "_ref", "nano_ref")
    rng = np.random.default_rng(3)
    files = []
    for k, (h, w) in enumerate(((40, 72), (40, 72), (37, 1041))):
        img = ((rng.integers(0, 1000, (h, w)) < 12) * rng.integers(128, 256, (h, w))).astype(np.uint8)
        img[0, 0] = 200  # never all-zero
        p = str(tmp_path / ("in%d.pgm" % k))
        write_pgm(p, img)
        files.append(p)
    for c, chain in enumerate(([("morph", ["dilate", "9"]), ("morph", ["erode", "10"])], [("morph", ["erode", "3"])])):
        outdir = tmp_path / ("out%d" % c)
        outdir.mkdir()
        r = subprocess.run([exe, "-o", str(outdir), *chain_args(chain), "--", *files], capture_output=True, timeout=600)
        assert r.returncode == 0, r.stderr.decode()[-800:]
        for i, f in enumerate(files):
            got = read_pgm(str(outdir / os.path.basename(f)))
            if os.path.exists(nano):
                exp, err = nano_chain(nano, chain, f, tmp_path, "ref%d_%d" % (c, i))
                assert exp is not None, err
                want = read_pgm(exp)
            else:
                want = read_pgm(f)
                for _, (op, n) in chain:
                    for _ in range(int(n)):
                        want = getattr(oracle, op)(np.ascontiguousarray(want))
            assert np.array_equal(got, want), (chain, f)
            assert not np.array_equal(got, read_pgm(f))
