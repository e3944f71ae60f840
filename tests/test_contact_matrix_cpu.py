"""What tests/test_gpu_contact_matrix.py rests on, checked without a GPU: the run of tests/contact_matrix_support.py really is about
contacts in the oracle, the fp32 host twin follows the oracle through it with no row in the fail class (its event counts are the table
TWIN_EVENTS that the GPU module's caps come from), and the cell list names every contact flag value that KindOps<KIND>::step / ::rollout
dispatch on."""
import os

import numpy as np
import pytest

import contact_matrix_support as S
from oracle import so100_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(kind, name) for kind in S.KINDS for name in S.FLAG_SETS]


@pytest.mark.parametrize("kind,name", PAIRS, ids=[f"{k}-{n}" for k, n in PAIRS])
def test_contact_run_touches_and_the_host_twin_follows_the_oracle(kind, name):
    """The 16 sampled envs, the oracle alone: actions clip(mean64(obs) + sigma policy_noise_ref).
    Coverage (contact_matrix_support.assert_coverage): at least a quarter of the sampled envs that are not parked end 3 or more steps of the
    first launch with a pad or link record, no parked env has one before its reset, under F_PADS_CUBE some env has a pad/cube record, no
    record is dropped over the budget, every observation is finite and the TimeLimit's code 2 falls on step 12, inside the second launch.
    The fp32 host twin (hc_env_step, the SHIPPED settings) on the same actions: equal done codes, every row classified against the oracle's
    (tight < 2e-5, event < 2e-2; rewards / 20, pixel entries / 5, terminal observations included), no fail, and exactly TWIN_EVENTS events."""
    flags = S.FLAG_SETS[name]
    res = S.oracle_alone(kind, flags)
    runs = [run for run, _, _ in res]
    touched, live = S.assert_coverage(kind, flags, runs)
    errs = []
    for run, acts, rows in res:
        assert np.isfinite(run.obs0).all() and np.abs(acts).max() <= 1.0
        obs0, twin, _, _ = S.twin_rows(kind, flags, run.i, acts)
        np.testing.assert_allclose(obs0, run.obs0, rtol=0, atol=1e-6)
        for t, (got, want) in enumerate(zip(twin, rows)):
            assert np.isfinite(want[0]).all() and np.isfinite(want[1]) and (want[3] is None or np.isfinite(want[3]).all()), (run.i, t)
            assert got[2] == want[2], (run.i, t, got[2], want[2])
            errs.append(S.row_error(kind, got[0], want[0], got[1], want[1], got[3], want[3]))
    classes = S.classify(errs)
    print(f"[contact matrix, oracle alone, kind {kind} {name}] {touched} of {live} live sampled envs in contact on >= 3 of {S.T1} steps; pad/cube "
          f"records on {sum(1 for r in runs for c in r.pad_cube if c)} (env, step) rows; host twin vs oracle {classes}, median {np.median(errs):.2e}")
    assert len(errs) == len(S.SAMPLE)*S.T and classes["fail"] == 0 and np.median(errs) < S.TIGHT
    assert classes["event"] == S.TWIN_EVENTS[kind, name], (classes, S.TWIN_EVENTS[kind, name])


@pytest.mark.parametrize("kind,name", PAIRS, ids=[f"{k}-{n}" for k, n in PAIRS])
def test_contact_budget_holds_with_a_manifold_to_spare_in_every_env(kind, name):
    """All 200 envs, the oracle alone and the host twin on its actions: no env ends a step with more than BUDGET_MARGIN = 12 pad / link
    records in the oracle or has more than that many records (the cube's floor records included) in any substep of the twin, 16 being the
    budget, and neither drops one.  The device's contact_stat row may then be held to `nothing dropped` in every env, not the sample alone."""
    flags = S.FLAG_SETS[name]
    worst = 0
    for run, acts, _ in S.oracle_alone(kind, flags, range(S.N)):
        _, _, most, dropped = S.twin_rows(kind, flags, run.i, acts)
        assert run.dropped == 0 and dropped == 0, (run.i, run.dropped, dropped)
        assert max(run.records) <= S.BUDGET_MARGIN and most <= S.BUDGET_MARGIN, (run.i, max(run.records), most)
        worst = max(worst, most, max(run.records))
    assert worst >= 4                                              # a whole manifold somewhere


def test_starts_are_what_the_module_says():
    """the parked quarter, the start families per flag set, and a sample that covers env 0, the last env and the upper half of a 64-env workgroup"""
    assert S.SAMPLE[0] == 0 and S.SAMPLE[-1] == S.N - 1 and len(set(S.SAMPLE)) == 16
    assert any(i % 64 >= 32 and i//64 < S.N//64 for i in S.SAMPLE)
    assert any(S.parked(i) for i in S.SAMPLE) and sum(not S.parked(i) for i in S.SAMPLE) >= 8
    assert [(S.N + epw - 1)//epw for epw in (64, 32, 16)] == [4, 7, 13] and all(S.N % epw == 8 for epw in (64, 32, 16))
    base = S.starts(S.FLAG_SETS["REFP"])[0]
    for name, flags in S.FLAG_SETS.items():
        qpos, qvel = S.starts(flags)
        assert qpos.shape == (S.N, 13) and qvel.shape == (S.N, 12) and qpos.dtype == np.float32
        assert np.isfinite(qpos).all() and np.isfinite(qvel).all()
        assert np.allclose(qpos[::S.PARK_EVERY, :6], S.PARKED_POSE) and not qvel[::S.PARK_EVERY].any()
        moved = np.nonzero(np.abs(qpos - base).max(1) > 0)[0]
        want = set()
        if flags & O.F_PADS_CUBE:
            want |= set(range(S.GRASP_FROM, S.N)) - set(S.FLOOR_NOT_GRASP)
        if flags & O.F_LINKS_FLOOR:
            want |= set(S.WRIST)
        if flags & O.F_LINKS_CUBE:
            want |= set(S.LINK_CUBE)
        assert set(moved) == {i for i in want if not S.parked(i)}, name
    assert {S.SAMPLE.index(i) for i in S.SAMPLE if i in S.WRIST} and {i for i in S.SAMPLE if i in S.LINK_CUBE} and {i for i in S.SAMPLE if i >= S.GRASP_FROM}


def test_contact_matrix_lists_every_dispatched_contact_flag_set():
    """Every compile-time flag value with a pad bit that KindOps<KIND>::step or ::rollout instantiates kernels for is a row of the contact
    matrix; the run-time-flags build (-1) is reached by a row that is not instantiated (C5 | PROXIES for every kind); and the matrix has its
    126 cells: 7 launchers x 6 kinds x 3 flag sets."""
    table = S.dispatched_flag_sets(ROOT)
    rows = set(S.FLAG_SETS.values())
    pad_bits = O.F_PADS_FLOOR | O.F_PADS_CUBE | O.F_LINKS_FLOOR | O.F_LINKS_CUBE
    for fn, vals in table.items():
        assert -1 in vals, fn
        contact = {v for v in vals if v >= 0 and v & pad_bits}
        assert contact and contact <= rows, (fn, sorted(contact - rows))
        assert rows - vals, fn                                    # some row falls through to <K, -1>
    assert S.FLAG_SETS["C5_PROXIES"] not in table["step"] | table["rollout"]
    assert len(S.CELLS) == len(set(S.CELLS)) == 126
    assert set(S.TWIN_EVENTS) == {(kind, name) for kind in S.KINDS for name in S.FLAG_SETS}
