"""The frame split of every gsh_*_batch entry on the MI355X: the cases of tests/frame_split_cases.py on device memory, each
call under gsh_tune key 8 = 0, 1, 2 and 3 and every frame of every output against the oracle's single-frame function; once
more with launches of two frames on a caller's stream; the three fixed groups key 8 does not govern (kLbpGroup, kOrbGroup,
the scratch group of the integral box route); and the two paths that exist on the GPU only, with a frame split inside them:
the side-stream chunks of gsh_edge_pipeline_batch and k_box_edge on the side stream."""
import pytest

import frame_split_cases as fs
import guard_cases as gd

pytestmark = pytest.mark.gpu
IDS = [c[0] for c in fs.CASES]
ENTRY = {"blur": "blur_batch", "adaptive": "adaptive_threshold_batch"}


@pytest.mark.parametrize("name, run", fs.CASES, ids=IDS)
def test_frame_split_gpu(hip, oracle, name, run):
    run(gd.Backend(hip, oracle, gpu=True), fs.SPLITS)


@pytest.mark.parametrize("name, run", fs.CASES, ids=IDS)
def test_frame_split_on_a_caller_stream(hip, oracle, name, run):
    """the matrix once more with launches of 2 + 2 + 2 + 1 frames after use_torch_stream on a stream of the caller's"""
    import torch
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    try:
        with torch.cuda.stream(st):
            hip.use_torch_stream()
            run(gd.Backend(hip, oracle, gpu=True), (2,))
    finally:
        hip.set_stream(None)


@pytest.mark.parametrize("case", fs.LBP_GROUP_CASES, ids=fs.lbp_group_id)
def test_lbp_group_gpu(hip, oracle, case):
    """kLbpGroup = 8 frames per cascade launch: 9 and 17 frames"""
    fs.check_lbp_group(gd.Backend(hip, oracle, gpu=True), *case)


def test_orb_group_4097_frames_passes_of_4096_and_1(hip, oracle):
    """kOrbGroup = 4096 frames per pass of gsh_orb_extract_batch: every list and score map of 4097 frames"""
    fs.check_orb_group(gd.Backend(hip, oracle, gpu=True))


@pytest.mark.parametrize("mode", ["blur", "adaptive"], ids=lambda m: "%s-r4-key6_3-66x1024x1024-launches_65+1" % ENTRY[m])
def test_box_scratch_group_gpu(hip, oracle, mode):
    """the integral box route keeps 256 MiB of table: 65 frames of 1024 x 1024 per launch"""
    fs.check_box_scratch_group(gd.Backend(hip, oracle, gpu=True), mode)


@pytest.mark.parametrize("split", [1, 2, 3], ids=lambda s: "key8_%d" % s)
@pytest.mark.parametrize("chunk", [3, 2], ids=lambda c: "key5_%d" % c)
def test_edge_pipeline_side_stream_chunks_with_a_frame_split_inside(hip, oracle, chunk, split):
    fs.check_pipeline_chunks(gd.Backend(hip, oracle, gpu=True), chunk, split)


@pytest.mark.parametrize("split", [1, 3], ids=lambda s: "key8_%d" % s)
@pytest.mark.parametrize("mode", ["blur", "adaptive"], ids=lambda m: "%s-r13-w67-key6_7" % ENTRY[m])
def test_box_edge_on_the_side_stream_in_every_launch(hip, oracle, mode, split):
    fs.check_side_stream_box_edge(gd.Backend(hip, oracle, gpu=True), mode, split)
