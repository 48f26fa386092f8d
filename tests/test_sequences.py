"""Call sequences on the kernel-logic emulator (CPU): direct parity of the four batch entry points no other test
called, chains of batch calls whose scratch slots grow in mid-chain, and history independence of every entry point
that shares per-thread scratch or a cache (tests/sequence_cases.py).  The emulator runs every call to completion, so
"unsynced" is only the call order here; tests/test_gpu_sequences.py runs the same cases on an MI355X, where it is not."""
import pytest

import parity_cases as pc
import sequence_cases as sc
from test_ragged import Bufs


@pytest.fixture
def b(emu, oracle):
    try:
        yield sc.Backend(emu, oracle, pc.Mem("host"))
    finally:
        emu.set_async(False)
        emu.set_stream(None)
        for key in (5, 6, 7):
            emu.tune(key, 0)


# ---- A ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sc.FAST_SCORE_SHAPES)
def test_fast_score_batch(b, shape):
    if shape == (1283, 517):  # a minute on the emulator with every combination; the GPU test runs them all at this size
        sc.fast_score(b, *shape, thresholds=(20, 300), ns=(3,), kinds=("noise",))
    else:
        sc.fast_score(b, *shape)


@pytest.mark.parametrize("shape", sc.ORB_DEV_SHAPES)
def test_orb_extract_single_device_frame(b, shape):
    sc.orb_extract_dev(b, *shape)


@pytest.mark.parametrize("n1,n2", sc.MATCH_DEV_SIZES)
def test_match_orb_dev(b, n1, n2):
    sc.match_orb_dev(b, n1, n2)


@pytest.mark.parametrize("off", [0, 1, 15])
@pytest.mark.parametrize("shape", sc.THRESHOLD_DEV_SHAPES)
def test_threshold_batch_dev(emu, oracle, shape, off):
    sc.threshold_batch_dev(emu, oracle, Bufs("emu"), shape[0], shape[1], off)


# ---- B ----------------------------------------------------------------------------------------------------------------
def test_chain1_histogram_partials(b):
    sc.chain_pair(b, sc.chain1, "chain 1")


def test_chain2_aux_and_integral_scratch(b):
    sc.chain_pair(b, sc.chain2, "chain 2")


def test_chain2_dropin_calls(b):
    ref, frames = sc.chain2_dropin(b, True)
    sc.check_chain2_dropin(b.o, ref, frames)
    b.g.set_async(True)
    sc.assert_runs_equal(sc.chain2_dropin(b, False)[0], ref, "drop-in chain")


def test_chain3_detectors(b, cascade):
    sc.chain_pair(b, sc.chain3, "chain 3", casc=cascade)


def test_chain4_components(b):
    sc.chain_pair(b, sc.chain4, "chain 4")


# ---- C ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sc.HISTORY))
def test_history_independence(b, cascade, name):
    sc.history_independence(b, cascade, name)


def test_lbp_geometry_cache_key_fields(b):
    sc.lbp_geometry_cache_key(b)


def test_dropin_cascade_edited_in_place(b):
    sc.dropin_cascade_edited_in_place(b)
