"""The cap sweeps of tests/cap_sweep_cases.py on the kernel-logic emulator, thinned to what a CPU can afford: caps_for() --
every mask-word, half-word, QUAD-group and chunk seam, the marks and 200 random caps -- instead of every cap, the small FAST
frames only, blobs on the 70 x 23 and 257 x 9 frames, LBP on `two_stages`.  They check the case code without a GPU and catch
a regression of the host logic; tests/test_gpu_cap_sweep.py runs every cap on an MI355X."""
import pytest

import blob_cases as bc
import cap_sweep_cases as cs
from guard_cases import Guarded
from parity_cases import Mem

HOST = Mem("host")
# two_stages has 41275 detections and the emulator takes 0.1 s per scan: of caps_for() the k * 32 +- 1 and k * 64 +- 1 series
# (2580 caps) and 160 of the random caps stay with the GPU file; 1 .. 130, the chunk seams, the scale marks and T - 1 .. T + 2 run here
LBP_THIN = {"randoms": 40, "units": (2048,)}


def test_caps_for_holds_every_seam():
    caps = cs.caps_for(5000, marks=(777, 4100))
    assert caps == sorted(set(caps)) and caps[0] == 1 and caps[-1] == 5002
    assert set(range(1, 131)) <= set(caps)
    for unit in (32, 64, 2048):
        for k in range(1, 5000 // unit + 1):
            assert k * unit - 1 in caps and k * unit + 1 in caps
    assert {776, 777, 778, 4099, 4100, 4101, 4999, 5000, 5001, 5002} <= set(caps)
    assert cs.caps_for(5000) == cs.caps_for(5000) and len(set(caps) - set(cs.caps_for(5000, (777, 4100), randoms=0))) > 150
    assert cs.caps_for(0) == list(range(1, 131)) and cs.all_caps(3) == [1, 2, 3, 4, 5]


@pytest.mark.parametrize("key19", [0, 1])
@pytest.mark.parametrize("name", cs.FAST_SMALL)
def test_fast_caps_emulated(emu, oracle, name, key19):
    c = cs.fast_case(oracle, name)
    cs.check_fast(emu, oracle, HOST, name, key19, cs.caps_for(c.T))


@pytest.mark.parametrize("key19", [0, 1])
def test_fast_batch_caps_emulated(emu, oracle, key19):
    c = cs.fast_batch_case(oracle)
    cs.check_fast_batch(emu, oracle, HOST, key19, cs.caps_for(max(c.T), c.T))


@pytest.mark.parametrize("key14", [0, 1])
def test_lbp_caps_emulated(emu, oracle, key14):
    cs.check_lbp(emu, oracle, (HOST,), "two_stages", key14, **LBP_THIN)


@pytest.mark.parametrize("part", range(3))
def test_lbp_batch_caps_emulated(emu, oracle, part):
    """three frames per call: the caps are dealt over three tests, so that none outlasts the suite's slowest emulator test"""
    cs.check_lbp_batch(emu, oracle, HOST, "two_stages", part=(part, 3), **LBP_THIN)


MATCH_SMALL = (150, 300, (150, 97, 64))
MATCH_CHUNKS = ((4200, 64, (4200, 4050)), (4200, 1024, (4200, 2049)))


@pytest.mark.parametrize("entry", ["dropin", "dev", "batch"])
def test_match_caps_three_words_emulated(emu, oracle, entry):
    c = cs.match_case(oracle, *MATCH_SMALL)
    caps = cs.caps_for(c.A)
    if entry == "dropin":
        cs.check_match_dropin(emu, oracle, *MATCH_SMALL, caps=caps)
    elif entry == "dev":
        cs.check_match_dev(emu, oracle, HOST, *MATCH_SMALL, caps=caps)
    else:
        cs.check_match_batch(emu, oracle, HOST, *MATCH_SMALL, caps=caps)


@pytest.mark.parametrize("entry", ["dropin", "batch"])
@pytest.mark.parametrize("sizes", MATCH_CHUNKS, ids=lambda s: "%dx%d" % s[:2])
def test_match_caps_three_chunks_emulated(emu, oracle, sizes, entry):
    """4200 queries cost the emulator a second per call: the first and the last cap, the seams of the first two mask words and
    the caps round the total alone; the GPU file runs caps_for(A)"""
    c = cs.match_case(oracle, *sizes)
    caps = sorted({1, 31, 33, 63, 65, c.A - 1, c.A, c.A + 1} & set(c.caps))
    assert len(caps) >= 6
    if entry == "dropin":
        cs.check_match_dropin(emu, oracle, *sizes, caps=caps)
    else:
        cs.check_match_batch(emu, oracle, HOST, *sizes, caps=caps)


def orb_sweep(c):
    """the nkps of the emulator's ORB sweeps: 1 .. 40 (the lists stop being prefixes of the largest one in there: asserted), the
    seams of the first mask word and the counts round K"""
    assert min(c.not_prefix) < 40
    return sorted(set(range(1, 41)) | {63, 64, 65, c.K - 1, c.K, c.K + 1, c.K + 2})


@pytest.mark.parametrize("entry", ["dropin", "batch"])
@pytest.mark.parametrize("w, h", cs.ORB_SHAPES)
def test_orb_nkps_emulated(emu, oracle, w, h, entry):
    sweep = orb_sweep(cs.orb_case(oracle, w, h, "libm"))
    (cs.check_orb_dropin if entry == "dropin" else cs.check_orb_batch)(emu, oracle, HOST, w, h, sweep)


@pytest.mark.parametrize("w, h", cs.ORB_SHAPES)
def test_orb_nkps_nostdlib_emulated(emu, w, h):
    cs.check_orb_batch_nostdlib(emu, w, h, orb_sweep(cs.orb_case(cs.nostdlib_oracle(), w, h, "nostdlib")))


@pytest.mark.parametrize("flavour", ["nostdlib", "libm"])
@pytest.mark.parametrize("w, h, levels, sweep", cs.PYRAMID_SWEEPS, ids=lambda v: str(v) if isinstance(v, int) else "nkps%d" % len(v))
def test_pyramid_nkps_emulated(emu, w, h, levels, sweep, flavour):
    gd = Guarded("host", seed=8)
    cs.check_pyramid(emu, gd, flavour, w, h, levels, sweep)  # caps_for(100) holds every nkps up to 100
    assert gd.checked == 4 * len(sweep)


@pytest.mark.parametrize("shape", [(70, 23), (257, 9)], ids=str)
def test_blob_caps_emulated(emu, shape):
    for name, img in cs.blob_frames((shape,)):
        cs.check_blobs(emu, HOST, name, img, cs.caps_for(bc.start_count(img)))


def test_blob_batch_caps_emulated(emu):
    starts = [bc.start_count(img) for _, img in cs.blob_frames(((70, 23),))]
    cs.check_blobs_batch(emu, HOST, (70, 23), cs.caps_for(max(starts), starts))
