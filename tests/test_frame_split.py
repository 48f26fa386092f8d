"""The frame split of every gsh_*_batch entry on the kernel-logic emulator: the cases of tests/frame_split_cases.py with
host memory, each call under gsh_tune key 8 = 0, 1, 2 and 3 (one launch; 7 launches of one frame; 2 + 2 + 2 + 1; 3 + 3 + 1)
and every frame of every output against the oracle's single-frame function.  tests/test_gpu_frame_split.py runs the same
cases on an MI355X, where the side streams of gsh_edge_pipeline_batch and of k_box_edge exist."""
import pytest

import frame_split_cases as fs
import guard_cases as gd


@pytest.mark.parametrize("name, run", fs.CASES, ids=[c[0] for c in fs.CASES])
def test_frame_split_emulated(emu, oracle, name, run):
    run(gd.Backend(emu, oracle, gpu=False), fs.SPLITS)


@pytest.mark.parametrize("case", fs.LBP_GROUP_CASES, ids=fs.lbp_group_id)
def test_lbp_group_emulated(emu, oracle, case):
    """kLbpGroup = 8 frames per cascade launch, a split key 8 does not govern: 9 and 17 frames"""
    fs.check_lbp_group(gd.Backend(emu, oracle, gpu=False), *case)


@pytest.mark.parametrize("split", [1, 2, 3], ids=lambda s: "key8_%d" % s)
@pytest.mark.parametrize("chunk", [3, 2], ids=lambda c: "key5_%d" % c)
def test_edge_pipeline_chunks_with_a_frame_split_inside_emulated(emu, oracle, chunk, split):
    """key 5 x key 8: the emulator runs the chunks in sequence (no side stream), the nested for_frames is the same"""
    fs.check_pipeline_chunks(gd.Backend(emu, oracle, gpu=False), chunk, split)


@pytest.mark.parametrize("mode", ["blur", "adaptive"])
def test_ragged_ring_box_then_integral_emulated(emu, oracle, mode):
    """r = 13 on 67 x 40 in launches of one frame, then gsh_integral_batch on the result (the side stream of k_box_edge is
    compiled out of the emulator: the edge launch follows the body)"""
    fs.check_side_stream_box_edge(gd.Backend(emu, oracle, gpu=False), mode, 1)


def test_case_ids_are_unique_and_name_a_route():
    ids = [c[0] for c in fs.CASES]
    assert len(set(ids)) == len(ids)
    assert all(i.count("-") >= 1 for i in ids)
