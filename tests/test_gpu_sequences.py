"""Call sequences on the MI355X (tests/sequence_cases.py): direct parity of the four batch entry points no other test
called; chains of batch calls with no host sync until the end -- on the library's own stream, on a torch.cuda.Stream
and through the drop-in calls under gsh_set_async(1) -- against the same chain synchronised after every call and against
the oracle; history independence of every entry point that shares per-thread scratch or a cache; and the rule of
include/grayskull_hip.h for gsh_set_stream: a switch orders the stream entered behind the stream left."""
import pytest

import parity_cases as pc
import sequence_cases as sc
from test_ragged import Bufs

pytestmark = pytest.mark.gpu


@pytest.fixture
def b(hip, oracle):
    try:
        yield sc.Backend(hip, oracle, pc.Mem("device"))
    finally:
        hip.set_async(False)
        hip.set_stream(None)
        for key in (5, 6, 7):
            hip.tune(key, 0)


def own_and_user_stream(b, chain, what, **kw):
    """synced and checked, unsynced on the library's own stream, unsynced on a torch.cuda.Stream"""
    import torch
    ref = sc.chain_pair(b, chain, what, **kw)
    st = torch.cuda.Stream()
    try:
        b.g.set_stream(st.cuda_stream)
        sc.assert_runs_equal(chain(b, False, **kw), ref, what + " on a torch stream")
    finally:
        b.g.set_stream(None)


# ---- A ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sc.FAST_SCORE_SHAPES)
def test_fast_score_batch(b, shape):
    sc.fast_score(b, *shape)


@pytest.mark.parametrize("shape", sc.ORB_DEV_SHAPES)
def test_orb_extract_single_device_frame(b, shape):
    sc.orb_extract_dev(b, *shape)


@pytest.mark.parametrize("n1,n2", sc.MATCH_DEV_SIZES)
def test_match_orb_dev(b, n1, n2):
    sc.match_orb_dev(b, n1, n2)


@pytest.mark.parametrize("off", [0, 1, 15])
@pytest.mark.parametrize("shape", sc.THRESHOLD_DEV_SHAPES)
def test_threshold_batch_dev(hip, oracle, shape, off):
    sc.threshold_batch_dev(hip, oracle, Bufs("gpu"), shape[0], shape[1], off)


# ---- B ----------------------------------------------------------------------------------------------------------------
def test_chain1_histogram_partials(b):
    own_and_user_stream(b, sc.chain1, "chain 1")


def test_chain2_aux_and_integral_scratch(b):
    own_and_user_stream(b, sc.chain2, "chain 2")


def test_chain2_dropin_calls_async(b):
    """gsh_set_async(1): the drop-in calls on device pointers return without a stream sync"""
    import torch
    ref, frames = sc.chain2_dropin(b, True)
    sc.check_chain2_dropin(b.o, ref, frames)
    b.g.set_async(True)
    sc.assert_runs_equal(sc.chain2_dropin(b, False)[0], ref, "drop-in chain, async")
    st = torch.cuda.Stream()
    b.g.set_stream(st.cuda_stream)
    sc.assert_runs_equal(sc.chain2_dropin(b, False)[0], ref, "drop-in chain, async, on a torch stream")


def test_chain3_detectors(b, cascade):
    own_and_user_stream(b, sc.chain3, "chain 3", casc=cascade)


def test_chain4_components(b):
    own_and_user_stream(b, sc.chain4, "chain 4")


# ---- C ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sc.HISTORY))
def test_history_independence(b, cascade, name):
    sc.history_independence(b, cascade, name)


def test_lbp_geometry_cache_key_fields(b):
    sc.lbp_geometry_cache_key(b)


def test_dropin_cascade_edited_in_place(b):
    sc.dropin_cascade_edited_in_place(b)


# ---- D ----------------------------------------------------------------------------------------------------------------
def test_stream_switch_orders_the_new_stream_behind_the_old(b):
    sc.stream_switch(b)
