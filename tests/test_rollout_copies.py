"""Static guard on the substep loop of the headline kernel so100_rollout_fused<1, 8, 4, 32> (compile only, no GPU): the LDL^T factor
must not be copied round the loop again.  tools/loop_copies.py compiles the one instantiation with the
product's flags and counts ordinary register moves (v_mov*, v_accvgpr_*, v_readlane / v_writelane) per region of the loop."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"

# Reached in section 8f: 36 static copies between the loop's barriers (parent: 89), 11 on wave 0's path (parent: 54), 24 in wave 1's
# RNEA block (parent: 34).  + 4: scheduler noise between rebuilds.
LOOP_COPIES = 36
WAVE0_COPIES = 11
RNEA_COPIES = 24
SLACK = 4


@pytest.fixture(scope="module")
def counts():
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("hipcc not found")
    spec = importlib.util.spec_from_file_location("loop_copies", os.path.join(ROOT, "tools", "loop_copies.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    txt, usage = mod.compile_isa("1, 8, 4, 32", [])
    return mod.summary(txt, usage)


def test_factor_is_not_copied_round_the_substep_loop(counts):
    s = counts
    print({k: s[k]["copy"] for k in ("loop", "wave0_path", "rnea_block", "back_edge_block", "tail")}, s["usage"])
    assert s["loop"]["copy"] <= LOOP_COPIES + SLACK
    assert s["wave0_path"]["copy"] <= WAVE0_COPIES + SLACK
    assert s["rnea_block"]["copy"] <= RNEA_COPIES + SLACK
    assert s["back_edge_block"]["accw"] == 0                     # nothing is parked in AGPRs at the back edge
    assert s["back_edge_block"]["copy"] == 0


def test_headline_kernel_keeps_zero_scratch(counts):
    u = counts["usage"]
    assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0
    # the loop the tool found is the substep loop: two barriers, both legs of about the known size
    assert set(counts["regions"]) == {"b1->b2", "b2->b1"}
    assert 400 < counts["rnea_block"]["total"] < 700 and 550 < counts["wave0_path"]["total"] < 900
