"""gsbatch `orb <template.pgm>` over slices (grayskull_amd/host/gsbatch.c): the template through
gsh_orb_extract_pyramid_batch once per worker, then per slice gsh_orb_pyramid_buffer_fill_batch ->
gsh_orb_extract_pyramid_batch -> gsh_match_orb_batch and one download.  Files and first sidecar lines must be those of the
reference's `nanomagick orb`, one process per file -- in which the scene's pyramid is built in the scratch buffer the
template's extraction left behind -- and `-v` reports the number of batched calls per size group."""
import os
import re
import subprocess

import numpy as np
import pytest

from oracle.pyoracle import Oracle
from tests.test_gsbatch import NANO, ROOT, build_emu, build_ref_nano, write_pgm

ORB_LINE = re.compile(r"gpu 0 group (\d+): orb: template (\d+) keypoint\(s\), (\d+) frame\(s\) in (\d+) batched call\(s\)")


def printable(a):
    """the reference's reader swallows leading pixels that are whitespace bytes (grayskull.h:116)"""
    a = np.ascontiguousarray(a).copy()
    a[0, 0] = max(int(a[0, 0]), 33)
    return a


def compare_with_nanomagick(nano, exe_args, template, files, outdir, tmp_path, env=None):
    """-> (gsbatch's stderr, number of files with a picture); every file: first sidecar line = nanomagick's stdout, picture
    byte-identical, or neither has one"""
    r = subprocess.run([*exe_args, "-v", "-o", str(outdir), "orb", template, "--", *files], capture_output=True, timeout=1800, env=env)
    pictures = 0
    for i, f in enumerate(files):
        out = str(tmp_path / ("nano_%d.pgm" % i))
        rr = subprocess.run([nano, "orb", template, f, out], capture_output=True, timeout=900)
        rec = open(str(outdir / (os.path.basename(f) + ".orb.txt"))).read().splitlines()
        assert rec[0] + "\n" == rr.stdout.decode(), (f, rec[0], rr.stdout)
        mine = str(outdir / os.path.basename(f))
        if rr.returncode != 0:  # no matches: nanomagick writes nothing, neither do we
            assert not os.path.exists(mine) and r.returncode == 1, f
            continue
        pictures += 1
        assert open(mine, "rb").read() == open(out, "rb").read(), "orb picture differs for %s" % f
        assert len(rec) == 1 + int(rec[0].rsplit(" ", 1)[1])
    assert r.returncode == (0 if pictures == len(files) else 1), r.stderr.decode()[-800:]
    return r.stderr.decode(), pictures


@pytest.mark.skipif(not os.path.exists(NANO), reason="reference checkout not present")
def test_gsbatch_orb_over_slices_equals_nanomagick_emulated(tmp_path):
    """a 300 x 270 template, five 203 x 171 windows of it and two 160 x 120 ones; GSBATCH_SLICE_BYTES holds two 203 x 171
    frames, so that group takes three slices, the last of one frame"""
    exe, nano = build_emu(tmp_path), build_ref_nano(tmp_path)
    base = printable(Oracle.synth(300, 270, 5))
    template = str(tmp_path / "template.pgm")
    write_pgm(template, base)
    files = []
    for k in range(5):
        files.append(str(tmp_path / ("scene%d.pgm" % k)))
        write_pgm(files[-1], printable(base[9 * k + 3:9 * k + 3 + 171, 11 * k + 5:11 * k + 5 + 203]))
    for k in range(2):
        files.append(str(tmp_path / ("small%d.pgm" % k)))
        write_pgm(files[-1], printable(base[40 * k + 20:40 * k + 140, 60 * k + 30:60 * k + 190]))
    files = [files[0], files[5], *files[1:5], files[6]]  # the groups interleaved on the command line
    outdir = tmp_path / "out"
    outdir.mkdir()
    err, pictures = compare_with_nanomagick(nano, [exe], template, files, outdir, tmp_path,
                                            env=dict(os.environ, GSBATCH_SLICE_BYTES=str(2 * 203 * 171)))
    assert pictures >= 5, "the scenes are windows of the template: most of them must match"
    lines = {int(m.group(1)): tuple(int(x) for x in m.groups()[1:]) for m in ORB_LINE.finditer(err)}
    assert set(lines) == {0, 1}, err
    nt = len(Oracle("port").orb_extract_pyramid(base, 2500, 20, 3)[0])
    assert lines[0] == (nt, 5, 3) and lines[1] == (nt, 2, 1), (lines, nt)


@pytest.mark.gpu
def test_gsbatch_orb_over_a_slice_on_gpu(tmp_path):
    """nanomagick's own parameters where FAST's cap bites: an 800 x 600 template and three 640 x 480 scenes
    (Oracle.synth seeds 21, 22, 23; seed 21 has 4935 corners against a cap of 3332).  The scene's keypoints then depend on
    the bytes the template's extraction left in the scratch buffer -- asserted from the oracle first -- so equality with the
    reference CLI's own build needs gsh_orb_pyramid_buffer_fill_batch"""
    nano = os.path.join(ROOT, "oracle", "_ref", "nano_ref")
    if not os.path.exists(nano):
        pytest.skip("oracle/_ref/nano_ref was not prebuilt")
    o = Oracle("port")
    tmpl = printable(Oracle.synth(800, 600, 5))
    scenes = [printable(Oracle.synth(640, 480, s)) for s in (21, 22, 23)]
    kt, after_template = o.orb_extract_pyramid(tmpl, 2500, 20, 3, np.zeros(1 << 20, np.uint8))
    over_t, _ = o.orb_extract_pyramid(scenes[0], 2500, 20, 3, after_template)
    over_0, _ = o.orb_extract_pyramid(scenes[0], 2500, 20, 3, np.zeros(1 << 20, np.uint8))
    assert len(over_t) == len(over_0) and over_t.tobytes() != over_0.tobytes(), "the buffer's earlier contents do not show"
    exe = os.path.join(ROOT, "grayskull_amd", "gsbatch")
    assert os.path.exists(exe), "grayskull_amd/gsbatch is built by build() (make tool)"
    template = str(tmp_path / "template.pgm")
    write_pgm(template, tmpl)
    files = []
    for k, s in enumerate(scenes):
        files.append(str(tmp_path / ("scene%d.pgm" % k)))
        write_pgm(files[-1], s)
    outdir = tmp_path / "out"
    outdir.mkdir()
    err, pictures = compare_with_nanomagick(nano, [exe], template, files, outdir, tmp_path)
    assert pictures == 3
    first = open(str(outdir / "scene0.pgm.orb.txt")).readline()
    assert first.startswith("Template: %d keypoints, Scene: %d keypoints" % (len(kt), len(over_t))), first
    m = ORB_LINE.search(err)
    assert m and tuple(int(x) for x in m.groups()) == (0, len(kt), 3, 1), err
