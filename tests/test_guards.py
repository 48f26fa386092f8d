"""The guard net on the kernel-logic emulator (CPU): every caller-owned output of the public surface between two
guards, prefilled with random bytes, compared with the oracle (tests/guard_cases.py).  The drop-in gs_* calls run twice:
on host pointers (the staged path and its copy-back sizes) and, with the emulator told to take caller pointers for device
memory, straight on the guarded buffers.  Each test asserts the number of guard checks its parameters imply.
tests/test_gpu_guards.py runs the same cases on an MI355X."""
import pytest

import guard_cases as gc

PATHS = ("dev", "host")


def _oracle(request):
    from oracle import pyoracle
    return request.getfixturevalue("reference" if pyoracle.have_reference() else "oracle")


@pytest.fixture
def b(emu, request):
    try:
        yield gc.Backend(emu, _oracle(request), gpu=False)
    finally:
        emu.c.emu_device_pointers(0)
        for key in (7, 14, 20):
            emu.tune(key, 0)


@pytest.mark.parametrize("path", PATHS)
def test_dropin_strip_ops(b, path):
    gc.dropin_strip(b, path)
    assert b.checked == gc.DROPIN_STRIP_CHECKS


@pytest.mark.parametrize("path", PATHS)
def test_geometry(b, path):
    gc.geometry(b, path)
    assert b.checked == gc.GEOM_CHECKS


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("route", ["DOT4", "BYTE", "PX", "MFMA"])
def test_match_template(b, route, path):
    cases = getattr(gc, "TEMPLATE_" + route)
    gc.template(b, path, cases)
    assert b.checked == gc.template_checks(cases)


def test_histogram_otsu_pipeline(b):
    gc.pointwise(b)
    assert b.checked == gc.POINTWISE_CHECKS


def test_threshold_in_place(b):
    gc.threshold(b)
    assert b.checked == gc.THRESHOLD_CHECKS


def test_synth_and_checksum(b):
    gc.synth_checksum(b)
    assert b.checked == gc.SYNTH_CHECKS


@pytest.mark.parametrize("roff", gc.RECORD_OFFS)
@pytest.mark.parametrize("shape", gc.FAST_SHAPES)
def test_fast(b, shape, roff):
    b.roff = roff
    gc.fast(b, *shape)
    assert b.checked == gc.fast_checks(*shape)


@pytest.mark.parametrize("roff", gc.RECORD_OFFS)
@pytest.mark.parametrize("shape", gc.ORB_SHAPES)
def test_orb(b, shape, roff):
    b.roff = roff
    gc.orb(b, *shape)
    assert b.checked == gc.orb_checks()


@pytest.mark.parametrize("roff", gc.RECORD_OFFS)
@pytest.mark.parametrize("case", gc.ORB_PYRAMID_CASES)
def test_orb_pyramid(b, case, roff):
    b.roff = roff
    gc.orb_pyramid(b, *case)
    assert b.checked == gc.ORB_PYRAMID_CHECKS


@pytest.mark.parametrize("roff", gc.RECORD_OFFS)
@pytest.mark.parametrize("n1,n2", gc.MATCH_SIZES)
def test_match_orb(b, n1, n2, roff):
    b.roff = roff
    gc.match(b, n1, n2)
    assert b.checked == gc.MATCH_CHECKS


@pytest.mark.parametrize("roff", gc.RECORD_OFFS)
@pytest.mark.parametrize("case", gc.LBP_CASES)
def test_lbp(b, case, roff):
    b.roff = roff
    gc.lbp(b, *case)
    assert b.checked == gc.LBP_CHECKS


@pytest.mark.parametrize("roff", gc.RECORD_OFFS)
@pytest.mark.parametrize("w", gc.BLOB_WIDTHS)
def test_blobs_corners_largest(b, w, roff):
    b.roff = roff
    gc.blobs(b, w)
    assert b.checked == gc.BLOB_CHECKS


def test_perspective(b):
    gc.perspective(b)
    assert b.checked == gc.PERSPECTIVE_CHECKS


@pytest.mark.parametrize("roff", gc.RECORD_OFFS)
@pytest.mark.parametrize("shape", gc.CONTOUR_SHAPES)
def test_contours(b, shape, roff):
    b.roff = roff
    gc.contours(b, *shape)
    assert b.checked == gc.CONTOUR_CHECKS
