"""LBP cascades with large, shared and odd-shaped stages on the kernel-logic emulator: the cases of tests/lbp_cascade_cases.py
against the oracle, the two conditions on the inputs those cases rest on, the structures the named cascades are named for,
and the abort on a cascade whose tables do not fit the block's LDS.  tests/test_gpu_lbp_cascades.py runs the same cases, with
every kernel choice on every frame and parameter set, on an MI355X.

The emulator takes seconds per uncapped scan, so it runs a part of what the GPU runs: under the rule (key 14 = 0) four of the
six parameter sets on the synth frame (uncapped, cap 7, from scale 0.5, step 2) and the capped step-2 scan on the edge map
and the flat frame; under key 14 = 1 and 3 and both values of key 15 the scan whose cap cuts inside a later scale, on the
synth frame; the batch with the capped step-2 scan.  Key 14 = 2 and 4 and key 4 = 1 run on the GPU only."""
import os
import subprocess
import sys

import numpy as np
import pytest

import lbp_cascade_cases as lc
from parity_cases import Mem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_SO = os.path.join(ROOT, "tests", "emu", "libgs_kernel_emu.so")
MEM = Mem("host")
RULE_PLAN = {"synth": (0, 1, 3, 5), "edges": (5,), "flat": (5,)}
OTHER_PLAN = {"synth": (2,)}
EMU_KEYS = ((14, 0), (14, 1), (14, 3), (15, 241), (15, 7))


@pytest.mark.parametrize("name", lc.NAMES)
def test_inputs_cover_every_stage_and_depend_on_the_order_of_adds(oracle, name):
    """case() asserts both conditions while it builds; here, what they rest on is looked at once more from outside"""
    c = lc.case(name, oracle)
    n = c.entering
    assert len(n) == c.casc.nstages + 1 and all(v >= 256 for v in n[:-1]) and n[-1] >= 1
    assert c.casc.nweaks <= 400 and c.w <= 200 and c.h <= 150
    assert c.params[1][0] == 7 and 7 < c.params[2][0] < lc.UNCAPPED
    full, capped = lc.expected(c, oracle, "synth", c.params[0]), lc.expected(c, oracle, "synth", c.params[2])
    ww = c.casc.window_w
    assert len(capped) == c.params[2][0] < len(full) and capped[-1]["w"] > ww, "the second cap cuts inside a later scale"
    assert (lc.expected(c, oracle, "synth", c.params[1])["w"] == ww).all(), "the cap of 7 cuts inside the first scale"
    half = lc.expected(c, oracle, "synth", c.params[3])
    assert half[0]["w"] == ww // 2 and len(half) > 0, "the scan from scale 0.5 detects at scale 0.5"


def test_named_cascades_have_the_structures_they_are_named_for(oracle):
    cs = {name: lc.case(name, oracle).casc for name in lc.NAMES}
    sizes = {int(n) for c in cs.values() for n in c.stage_nweaks}
    assert {1, 11, 12, 13, 31, 32, 33, 40, 64, 65} <= sizes
    assert {c.nstages for c in cs.values()} >= {1, 2}
    assert {(c.window_w, c.window_h) for c in cs.values()} >= {(12, 12), (20, 28), (31, 17), (24, 24)}
    assert any(c.stage_nweaks[0] > 12 for c in cs.values()) and any(c.stage_nweaks[0] > 32 for c in cs.values())
    last = {int(c.stage_nweaks[-1]) for c in cs.values() if c.nstages > 2}
    assert any(n <= 12 for n in {int(cs["two_stages"].stage_nweaks[-1])}) and any(13 <= n < 32 for n in last) and 32 in last and any(n > 32 for n in last)
    for name, c in cs.items():
        assert set(np.unique(c.weak_num_subsets)) <= set(range(1, 9)) and len(np.unique(c.weak_num_subsets)) >= 6, name
        if c.nstages > 2:
            assert (np.diff(c.stage_weak_start.astype(int)) < 0).any(), "%s: stages are stored out of evaluation order" % name
    reached = lambda c: {int(s) + k for s, n in zip(c.stage_weak_start, c.stage_nweaks) for k in range(int(n))}
    for name in ("float_sum_first", "wide_first"):
        dead = sorted(set(range(cs[name].nweaks)) - reached(cs[name]))
        assert dead and np.isnan(cs[name].weak_left_val[dead]).all(), "%s: classifiers no stage reaches" % name
    c = cs["two_windows_per_wave"]
    assert c.stage_weak_start[0] == c.stage_weak_start[2] and c.stage_threshold[0] != c.stage_threshold[2]
    c = cs["wide_first"]
    assert c.stage_weak_start[2] == c.stage_weak_start[0] + 64 - 31
    c = cs["truth_tables"]
    a = int(c.stage_weak_start[4])
    assert c.weak_subset_offset[a] == c.weak_subset_offset[a + 1]
    c = cs["specials"]
    assert np.isnan(c.stage_threshold[2]) and np.isinf(c.weak_right_val).sum() == 1
    assert (c.weak_left_val.view(np.uint32) == 0x80000000).sum() == 1


def test_the_numpy_restatement_agrees_with_the_oracle_at_other_scales(oracle):
    """lookup_bits / stage_sums at scale 0.5 and 1.728 against orc_lbp_window, window by window"""
    c = lc.case("every_branch", oracle)
    for scale in (0.5, float(np.float32(1.2) * np.float32(1.2) * np.float32(1.2))):
        bits = lc.lookup_bits(c.casc, c.frames["synth"], scale)
        ok = np.ones(bits.shape[1:], bool)
        for s in range(c.casc.nstages):
            ok &= lc.passes(lc.stage_sums(c.casc, s, bits), c.casc.stage_threshold[s])
        for (y, x) in [(0, 0), (ok.shape[0] - 1, ok.shape[1] - 1)] + [tuple(p) for p in np.argwhere(ok)[:40]] + [tuple(p) for p in np.argwhere(~ok)[:40]]:
            assert oracle.lbp_window(c.casc, c.ii["synth"], int(x), int(y), scale) == int(ok[y, x]), (scale, x, y)


@pytest.mark.parametrize("kv", EMU_KEYS, ids=lambda kv: "key%d_%d" % kv)
@pytest.mark.parametrize("name", lc.NAMES)
def test_detect(emu, oracle, name, kv):
    lc.check_detect(emu, oracle, [MEM], name, kv[0], kv[1], RULE_PLAN if kv == (14, 0) else OTHER_PLAN)


@pytest.mark.parametrize("name", lc.NAMES)
def test_batch_and_counting_kernels(emu, oracle, name):
    lc.check_batch(emu, oracle, MEM, name, which=(5,))


@pytest.mark.parametrize("name", lc.NAMES)
def test_single_windows(emu, oracle, name):
    lc.check_windows(emu, oracle, [MEM], name)


# ---- tables that do not fit --------------------------------------------------------------------------------------------------
TOO_LARGE = '''
import sys, numpy as np
sys.path.insert(0, %r)
import grayskull_amd as G
from grayskull_amd.cascade import Cascade
g = G.Grayskull(%r)
def cascade(nw):  # one stage of nw classifiers with 8 subset words each: 16 + nw * (16 + 16 + 32) bytes of tables
    return Cascade(24, 24, features=np.tile(np.array([2, 3, 4, 5], np.int8), nw), weak_feature_idx=np.arange(nw, dtype=np.uint16),
                   weak_left_val=np.ones(nw, np.float32), weak_right_val=-np.ones(nw, np.float32),
                   weak_subset_offset=(np.arange(nw) * 8).astype(np.uint16), weak_num_subsets=np.full(nw, 8, np.uint16),
                   subsets=np.full(nw * 8, 0x55555555, np.int32), stage_weak_start=np.zeros(1, np.uint16),
                   stage_nweaks=np.full(1, nw, np.uint16), stage_threshold=np.zeros(1, np.float32))
ii = np.cumsum(np.cumsum(np.full((40, 48), 7, np.uint32), 0), 1).astype(np.uint32)
r = g.lbp_detect(cascade(900), ii, 100, 1.2, 1.0, 1.5, 1)   # fine: 57616 bytes
print("fits", len(r), flush=True)
''' % (ROOT, EMU_SO)


def test_tables_beyond_the_lds_abort_in_the_launcher(emu, tmp_path):
    """961 classifiers with 8 subset words are 61520 bytes of tables: gs_lbp_detect ends in the launcher's assertion, before any
    kernel is asked for more LDS than a block has; 900 (57616 bytes) run"""
    good = tmp_path / "fits.py"
    good.write_text(TOO_LARGE)
    r = subprocess.run([sys.executable, str(good)], capture_output=True)
    assert r.returncode == 0 and b"fits" in r.stdout, r
    bad = tmp_path / "too_large.py"
    bad.write_text(TOO_LARGE + 'g.lbp_detect(cascade(961), ii, 100, 1.2, 1.0, 1.5, 1)\nprint("returned", flush=True)\n')
    r = subprocess.run([sys.executable, str(bad)], capture_output=True)
    assert r.returncode == -6, r
    assert b"Assertion failed:" in r.stderr and b"cascade tables must fit the block's LDS" in r.stderr, r.stderr
    assert b"fits" in r.stdout and b"returned" not in r.stdout
    assert r.stderr.count(b"Assertion failed:") == 1, r.stderr
