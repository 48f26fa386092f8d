"""The coded chunks of gsh_edge_pipeline_batch in the emulator: the fused kernel's coded and repair modes, k_expand_codes and
the chunk logic of gs_stencil.cpp (one stream, chunk after chunk) against the oracle and the unsplit call.  The cases are
tests/pipeline_codes_cases.py's, shared with the GPU test."""
import pytest

import pipeline_codes_cases as cc


@pytest.fixture(scope="module")
def b(emu):
    return cc.Host(emu)


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
    cc.repeated_calls(b, oracle, reps=2)
