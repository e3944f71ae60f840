"""What tests/test_gpu_kernel_matrix.py rests on, checked without a GPU: the run of tests/matrix_support.py is contact-free and reaches
every kind's branches in the oracle, and the cell list names every flag set that KindOps<KIND>::step / ::rollout dispatch on."""
import os
import re

import pytest

import matrix_support as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("kind", S.KINDS)
def test_matrix_run_is_contact_free_and_reaches_every_branch(kind):
    """All 97 envs, flags C5 and REFP, the oracle alone: the policy mean in float64 on the host plus exp(log_std) policy_noise_ref.  No finger
    pad touches the floor or the cube at the end of any of the 15 steps (the bounds of the GPU module carry no contact-event class), and every
    marked env shows its kind's event: termination by the lost counter (3, 5), last centre re-used (4), reach bonus (2, 6), and the TimeLimit."""
    for name in ("C5", "REFP"):
        runs = S.oracle_alone(kind, S.FLAG_SETS[name])
        assert len(runs) == S.N
        touched = [(r.i, r.pad_contacts) for r in runs if r.pad_contacts]
        assert not touched, (kind, name, touched)
        S.assert_events(kind, runs)
        assert sum(1 for r in runs if 1 in r.codes) == (S.N + S.EVERY - 1)//S.EVERY*(kind in (3, 5))


def test_matrix_lists_every_dispatched_flag_set():
    """A flag set that KindOps<KIND>::step or ::rollout instantiates kernels for must be a row of the matrix, the run-time-flags build (-1)
    must be reached by a row that is NOT instantiated, and the 32-env rollout kernel must exist for exactly the flag sets rollout32 runs."""
    table = S.dispatched_flag_sets(ROOT)
    rows = set(S.FLAG_SETS.values())
    for fn, vals in table.items():
        assert -1 in vals, fn
        assert vals - {-1} <= rows, (fn, sorted(vals - {-1} - rows))
        assert rows - vals, fn                                    # some row falls through to <K, -1>
    assert S.FLAG_SETS["UNINSTANTIATED"] not in table["step"] | table["rollout"]
    src = open(os.path.join(ROOT, "so100_mujoco_rl_amd", "csrc", "so100_kernels.hpp")).read()
    narrow = {S._FLAG_BITS[m] for m in re.findall(r"so100_rollout_fused<KIND,\s*(\w+),\s*4,\s*32>", src)}
    assert narrow == {S.FLAG_SETS[n] for n in S.LAUNCHERS["rollout32"]}
    assert len(S.CELLS) == len(set(S.CELLS)) == 114
    for launcher, names in S.LAUNCHERS.items():                   # every full-width launcher runs every flag set its function dispatches on
        fn = "rollout" if launcher.startswith("rollout") else "step"
        if launcher != "rollout32":
            assert {S.FLAG_SETS[n] for n in names} >= table[fn] - {-1}, launcher
