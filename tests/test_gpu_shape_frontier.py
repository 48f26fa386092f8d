"""The shape frontier on the MI355X (tests/shape_frontier_cases.py has the cases and, per case, the launcher and its grid.y):
A. every operation at the smallest height whose row-derived grid.y passes 65535 and at the largest that does not, device and
   host pointers; B. frames of 262200 x 9 and 1048600 x 4; C. one frame of 65536 x 32800 = 2^31 + 2 097 152 bytes, made on
   the device and never copied to the host whole.

C's references: the stencils against the same call on the frame's two halves, cut with 64 rows of overlap (each half is
below 2 GiB and takes the strip route, which the rest of the suite pins; gs_adaptive_threshold's halves, too wide for the
sliding box kernels, take the banded integral table instead), byte for byte away from the cut, and four bands
of 64 rows against the reference on the host; histogram and Otsu against the library's histograms of four quarter frames;
threshold against torch; the integral table against torch.cumsum in 64 bits; ORB against the oracle on the 400-row tail."""
import time

import numpy as np
import pytest

import shape_frontier_cases as sfc
from parity_cases import SENTINEL as SENT, Mem
from util import assert_same

pytestmark = pytest.mark.gpu
MEMS = [Mem("device"), Mem("host")]


@pytest.fixture(autouse=True)
def _wall_time(request):
    t0 = time.time()
    yield
    print("\n[wall] %s %.2f s" % (request.node.name, time.time() - t0))


# ---- A, B ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,side", sfc.TALL_CASES, ids=["%s-%s" % (c[0], side) for c, side in sfc.TALL_CASES])
def test_tall_frames(hip, reference, case, side):
    sfc.check_frontier(case)
    sfc.run_tall(hip, MEMS, reference, case, side)


@pytest.mark.parametrize("case", sfc.WIDE_CASES, ids=["%s-%dx%d" % c for c in sfc.WIDE_CASES])
def test_wide_frames(hip, reference, case):
    sfc.run_wide(hip, MEMS, reference, case)


# ---- C ---------------------------------------------------------------------------------------------------------------
BW, BH = 65536, 32800
CUT, LAP = BH // 2, 64
ROW_2_31 = (1 << 31) // BW  # the row that starts at byte offset 2^31
BANDS = ((0, 64), (CUT - 32, CUT + 32), (ROW_2_31 - 48, ROW_2_31 + 16), (BH - 64, BH))


@pytest.fixture(scope="module")
def big(hip):
    """eight synthetic frames of 65536 x 4100 back to back (the library's generator, equal to the oracle's on the CPU) under
    a row and column ramp: 2 149 580 800 bytes on the device"""
    import torch
    assert BW * BH == 2149580800 and BW * BH == 2 * (1 << 30) + 2097152 and ROW_2_31 == 32768 < BH
    img = torch.empty((BH, BW), dtype=torch.uint8, device="cuda")
    hip.synth_batch(img.view(8, BH // 8, BW), 500)
    hip.sync()
    rows = ((torch.arange(0, BH, 3, device="cuda") * 5) % 256).to(torch.uint8)[:, None]
    cols = (torch.arange(0, BW, 2, device="cuda") % 256).to(torch.uint8)[None, :]
    img[::3, ::2] = rows + cols
    yield img
    del img
    torch.cuda.empty_cache()


@pytest.fixture
def release(hip):
    """the library's scratch (8.6 GiB for gs_blur's table) does not stay allocated on a shared card"""
    import torch
    yield
    torch.cuda.synchronize()
    hip.shutdown()
    torch.cuda.empty_cache()


K3 = sfc.K3
STENCILS = {
    "sobel": (lambda g, d, s: g.sobel(d, s), lambda o, a: o.sobel(a, np.full_like(a, SENT))),
    "erode": (lambda g, d, s: g.erode(d, s), lambda o, a: o.erode(a)),
    "dilate": (lambda g, d, s: g.dilate(d, s), lambda o, a: o.dilate(a)),
    "morph3": (lambda g, d, s: g.morph_batch(d[None], s[None], 3, False), lambda o, a: o.erode(o.erode(o.erode(a)))),
    "filter3x3": (lambda g, d, s: g.filter(d, s, K3, 16), lambda o, a: o.filter(a, K3, 16)),
    "blur2": (lambda g, d, s: g.blur(d, s, 2), lambda o, a: o.blur(a, 2)),
    "adaptive2": (lambda g, d, s: g.adaptive_threshold(d, s, 2, 3), lambda o, a: o.adaptive_threshold(a, 2, 3)),
}


@pytest.mark.parametrize("name", list(STENCILS))
def test_stencils_on_a_frame_of_2_31_bytes(hip, reference, big, release, name):
    import torch
    call, expect = STENCILS[name]
    whole = torch.full_like(big, SENT)
    call(hip, whole, big)  # first: the halves then find the scratch large enough
    torch.cuda.synchronize()
    assert not bool((whole == SENT).all()), "%s: the output still holds its prefill everywhere" % name
    for part, rows, keep in ((big[:CUT + LAP], slice(0, CUT), slice(0, CUT)), (big[CUT - LAP:], slice(CUT, BH), slice(LAP, None))):
        assert part.numel() < 0x7fff0000  # strip_ok: the route of the rest of the suite
        half = torch.full_like(part, SENT)
        call(hip, half, part)
        torch.cuda.synchronize()
        assert torch.equal(whole[rows], half[keep]), "%s: the whole frame differs from its half, rows %s" % (name, rows)
        del half
    for r0, r1 in BANDS:
        lo, hi = max(0, r0 - 8), min(BH, r1 + 8)
        want = expect(reference, big[lo:hi].cpu().numpy())[r0 - lo:r1 - lo]
        assert_same(whole[r0:r1].cpu().numpy(), want, "%s rows %d..%d of the 2^31-byte frame" % (name, r0, r1))


def test_histogram_and_otsu_of_2_31_bytes(hip, oracle, big, release):
    """two whole 1 GiB pieces and a remainder of 2 097 152 bytes (launch_histogram) against four quarter frames"""
    q = BH // 4
    assert q * BW < 1 << 30
    parts = sum(hip.histogram(big[k * q:(k + 1) * q]).astype(np.uint64) for k in range(4))
    assert int(parts.sum()) == BW * BH
    assert_same(hip.histogram(big).astype(np.uint64), parts, "gs_histogram of 2^31 + 2^21 bytes")
    t = hip.otsu_threshold(big)
    assert t == oracle.otsu_from_hist(parts.astype(np.uint32), BW * BH), "gs_otsu_threshold of 2^31 + 2^21 bytes"


def test_threshold_of_2_31_bytes(hip, reference, big, release):
    import torch
    t = 117
    band = big[:16].cpu().numpy()
    assert_same(((band > t) * 255).astype(np.uint8), reference.threshold(band, t), "the torch expression is gs_threshold")
    c = big.clone()
    hip.threshold(c, t)
    torch.cuda.synchronize()
    assert torch.equal(c, (big > t).to(torch.uint8) * 255)


def test_integral_table_of_2_31_bytes(hip, big, release):
    """32768 x 16400: 4 w h >= 2^31 selects k_integral_rows / k_integral_cols; torch.cumsum in 64 bits, masked to 32"""
    import torch
    w, h = 32768, 16400
    assert w * h * 4 >= 1 << 31
    src = big.view(-1)[:w * h].view(h, w)
    ii = torch.full((h, w), SENT * 0x01010101 - (1 << 32), dtype=torch.int32, device="cuda")
    hip.integral(src, ii)
    torch.cuda.synchronize()
    carry = torch.zeros(w, dtype=torch.int64, device="cuda")
    for y in range(0, h, 1025):
        rows = torch.cumsum(src[y:y + 1025].to(torch.int64), 1)
        want = torch.cumsum(rows, 0) + carry
        carry = want[-1].clone()
        got = ii[y:y + 1025].to(torch.int64) & 0xFFFFFFFF
        assert torch.equal(got, want & 0xFFFFFFFF), "gs_integral rows %d.." % y
    assert int(carry[-1]) >= 1 << 32  # the table wrapped


def test_orb_on_a_flat_frame_of_2_31_bytes(hip, oracle, release):
    """PxReader's form for large frames: a flat frame with a dozen patches of noise in its last 200 rows (flat squares have
    no FAST corner that survives the NMS pass: their scores tie); the keypoints are the oracle's on the 400-row tail, y shifted"""
    import torch
    img = torch.full((BH, BW), 100, dtype=torch.uint8, device="cuda")
    rng = np.random.default_rng(12)
    for k in range(12):
        x, y = 300 + k * 5800 + (k % 3) * 7, BH - 180 + (k % 4) * 33
        img[y:y + 14, x:x + 14 + k] = torch.from_numpy(rng.integers(0, 256, (14, 14 + k), dtype=np.uint8)).cuda()
    tail = img[BH - 400:].cpu().numpy()
    want = oracle.orb_extract(tail, 1000, 20)
    assert 100 < len(want) < 1000 and len(set(want["x"] // 5800)) == 12 and want["x"].max() > BW - 2000
    want["y"] += BH - 400
    sm = torch.zeros_like(img)
    got = hip.orb_extract(img, 1000, 20, sm)
    assert_same(got, want, "gs_orb_extract on the 2^31-byte frame")
