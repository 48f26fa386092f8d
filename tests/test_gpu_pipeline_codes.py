"""The coded chunks of gsh_edge_pipeline_batch on the GPU: coded fused launches on the caller's stream, Otsu, expander and
repair launch on the side stream, ordered by events.  The cases are tests/pipeline_codes_cases.py's, shared with the emulator
test; on top of them a caller-provided stream with a stream-ordered consumer."""
import numpy as np
import pytest

import pipeline_codes_cases as cc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def b(hip):
    return cc.Dev(hip)


@pytest.mark.parametrize("w", cc.SHAPE_WIDTHS)
def test_shapes_bands_and_tail_chunks(b, oracle, w):
    cc.shapes(b, oracle, w)


def test_forced_guesses_at_the_window_edges(b, oracle):
    cc.window_edges(b, oracle)


def test_clamped_guesses_and_thresholds_below_8(b, oracle):
    cc.clamp_and_low_thresholds(b, oracle)


def test_rule_based_guesses_with_real_misses(b, oracle):
    cc.rule_with_misses(b, oracle)


def test_key_28_never_is_the_byte_path(b, oracle):
    cc.never_equals_byte_path(b, oracle)


def test_repeated_calls(b, oracle):
    cc.repeated_calls(b, oracle, reps=3)


def test_caller_provided_stream(b, oracle, hip):
    """the coded chunks on a torch stream, consumed on that stream with no host sync in between; under the rule, with every
    frame forced to miss and with every coded frame's guess forced into the window of frame 2's threshold"""
    import torch
    ref = cc.reference(oracle, ("plain", 256, 96), lambda: cc.synth_frames(256, 96, 6, 4242))
    src, final, tref, href = ref
    dsrc = b.put(src)
    st = torch.cuda.Stream()
    try:
        with torch.cuda.stream(st):
            hip.use_torch_stream()
            for codes in (0, 256, int(tref[2]) + 1):
                hip.tune(cc.KEY_CHUNK, 2), hip.tune(cc.KEY_CODES, codes)
                out, thr = torch.full_like(dsrc, 3), torch.zeros(len(src), dtype=torch.uint8, device="cuda")
                hist = torch.zeros((len(src), 256), dtype=torch.int32, device="cuda")
                hip.edge_pipeline_batch(out, None, dsrc, 2, hist, thr)
                after, tafter = out.clone(), thr.clone()  # stream-ordered consumers
                st.synchronize()
                assert np.array_equal(after.cpu().numpy(), final) and np.array_equal(tafter.cpu().numpy(), tref), "key 28 = %d" % codes
                assert np.array_equal(hist.cpu().numpy().view(np.uint32), href)
    finally:
        hip.tune(cc.KEY_CHUNK, 0), hip.tune(cc.KEY_CODES, 0)
        hip.use_torch_stream()
