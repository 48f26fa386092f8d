"""The kernel-logic cases of tests/test_emu_logic.py on the MI355X: tests/kernel_logic_cases.py holds the bodies, this
module runs them on the product library.  The emulator build compiles the scalar restatement of prims.h (-DGS_EMU), takes
box_blocks_per_cu as a constant and runs every template instantiation through one host compiler; here the buffer
descriptors, the DPP / v_perm / inline-asm primitives, the occupancy-derived band geometry and each of hipcc's 32
k_box16r<MODE, r> kernels compute the answer.

Every case runs with device pointers, and with host pointers where the call is a drop-in gs_* (the gsh_*_batch entries take
device pointers).  Bit-exact against the oracle or the reference; floats as their 32 bits.  What is fixed here, by the
parametrisation: every ring radius 1 .. 16 in both modes on 13 + 4 shapes, the orientation at r = 15, 36, 37, 60, 90, the
eleven FAST thresholds under both score kernels."""
import pytest

import kernel_logic_cases as kl
import parity_cases as pc

pytestmark = pytest.mark.gpu

HOST, DEV = pc.Mem("host"), pc.Mem("device")
BOTH = (DEV, HOST)


def _id(v):
    return "x".join(str(x) for x in v) if isinstance(v, tuple) else None


# ---- orientation
@pytest.mark.parametrize("r", kl.ORIENT_RADII)
def test_orientation_any_radius_matches_the_reference_float_order(hip, reference, r):
    """r = 37, 60, 90: k_orient_moments_seq, one thread in the reference's float32 order, with contraction off"""
    kl.orientation(hip, reference, BOTH, r)


@pytest.mark.parametrize("r", [37, 60])
def test_orientation_nostdlib_beyond_the_exact_radius(hip, r):
    kl.orientation_nostdlib(hip, BOTH, r)


# ---- ring box kernels: every radius, both modes
RING_CASES = [(s, r, False) for s in kl.RING_SHAPES for r in kl.ring_radii(s)] + \
             [(s, r, True) for s in kl.RING_SHAPES_WIDE for r in kl.ring_radii(s)]


def test_ring_cases_cover_every_radius_at_every_block_size():
    """the parametrisation below, not a drawn example: r = 1 .. 16 on a 64-, a 128- and a 256-thread shape, whole and ragged"""
    for shapes in ([s for s in kl.RING_SHAPES if s[0] % 16 == 0], [s for s in kl.RING_SHAPES if s[0] % 16],
                   kl.RING_SHAPES_WIDE[0:1], kl.RING_SHAPES_WIDE[1:2], kl.RING_SHAPES_WIDE[2:3], kl.RING_SHAPES_WIDE[3:4]):
        assert {r for (s, r, _) in RING_CASES if s in shapes} == set(range(1, 17)), shapes


@pytest.mark.parametrize("shape,r,wide", RING_CASES, ids=["%dx%d-r%d" % (s[0], s[1], r) for (s, r, _) in RING_CASES])
def test_box_register_ring_kernel_every_radius(hip, oracle, shape, r, wide):
    """k_box16r<0, r> (r >= 4) and k_box16r<1, r> against the oracle, k_box16 (key 6 = 4) and the integral route (key 6 = 3);
    all-255 frames, bands of 1 / 5 / 2r+1 / 2r+2 rows, twelve compare constants (three on the wide shapes)"""
    blur_ring, adapt_ring = kl.box_ring(hip, oracle, BOTH, shape, r, wide)
    n_img, n_c = (2, len(kl.RING_C_WIDE)) if wide else (3, len(kl.RING_C) - 2)  # 2^30 and -2^31 leave the product form
    assert adapt_ring == len(BOTH) * (n_img * n_c + 4), "every adaptive call inside the product form is a ring case"
    assert blur_ring == (len(BOTH) * (n_img + 4) if r >= 4 else 0)


# ---- any-radius box
@pytest.mark.parametrize("r", kl.ANY_RADII)
def test_box_radii_around_the_quotient_switch_and_up_to_127(hip, oracle, r):
    kl.box_any_radius(hip, oracle, BOTH, r)


def test_box_kernel_any_band_height(hip, oracle):
    kl.box_band_heights(hip, oracle, DEV)


@pytest.mark.parametrize("shape", kl.FULL_WIDTH_SHAPES, ids=_id)
def test_box_kernel_full_width(hip, oracle, shape):
    kl.box_full_width(hip, oracle, BOTH, shape)


# ---- strip launch tuning
@pytest.mark.parametrize("geom", [0, 1, 2])
@pytest.mark.parametrize("frame", [1, 2, 3])
def test_strip_launch_tuning_never_changes_results(hip, oracle, geom, frame):
    kl.strip_launch_tuning(hip, oracle, BOTH, geom, frame)


# ---- FAST
@pytest.mark.parametrize("mem", [HOST, DEV], ids=["host", "device"])
@pytest.mark.parametrize("shape", [(67, 45), (260, 17), (516, 9), (1040, 9), (2064, 8)], ids=_id)
def test_fast_every_wrap_threshold(hip, oracle, shape, mem):
    kl.fast_shape(hip, oracle, mem, shape)


@pytest.mark.parametrize("mem", [HOST, DEV], ids=["host", "device"])
def test_fast_score_tiles_that_stick_out_of_the_frame(hip, oracle, mem):
    kl.fast_tiles_that_stick_out(hip, oracle, mem)


@pytest.mark.parametrize("order", [0, 1])
def test_fast_batch_tiles_of_several_frames_in_xcd_order(hip, oracle, order):
    kl.fast_batch_in_xcd_order(hip, oracle, DEV, order)


def test_fast_with_a_score_map_of_another_size(hip, reference):
    kl.fast_score_map_of_another_size(hip, reference, BOTH)


# ---- histogram
def test_histogram_ragged_frames_every_alignment(hip, oracle):
    kl.histogram_every_alignment(hip, oracle, DEV)


def test_histogram_of_an_image_larger_than_one_launch_frame(hip, oracle):
    kl.histogram_in_pieces(hip, oracle, DEV)


# ---- fused pipeline, blur + sobel, template rows
@pytest.mark.parametrize("radius", [1, 2, 3])
@pytest.mark.parametrize("shape", kl.FUSED_SHAPES, ids=_id)
def test_fused_edge_pipeline_equals_separate_calls(hip, oracle, radius, shape):
    kl.fused_edge_pipeline(hip, oracle, DEV, radius, shape)


@pytest.mark.parametrize("radius", [1, 2, 3, 5])
def test_blur_sobel_batch(hip, oracle, radius):
    kl.blur_sobel_batch(hip, oracle, DEV, radius, nhw=(3, 20, 48))


def test_template_wider_than_the_lds_tile(hip, oracle):
    kl.template_wider_than_the_lds_tile(hip, oracle, BOTH)
