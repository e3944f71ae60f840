"""The arm dynamics of csrc/so100_physics.hpp (arm_trig + arm_bias + arm_mass + arm_factor) on the host, on the states where a term that
is dropped as "identically zero" would show if it were not: the base at rest, one joint moving alone (both signs), v = 0, v = -0.0,
every joint at a limit, and 64 seeded random states inside the joint ranges (tests/_armcheck/armcheck.cpp holds the list; 87 states).
The program is built without FMA contraction, in float and double, pair form (PK = true) and one-vector-at-a-time form.  CPU only.

1. The pair form and the scalar form agree bit for bit, in both types.
2. The results equal, bit for bit (two zeros of opposite sign count as equal), the ones the same program printed when it was built from
   the commit named in tests/golden/arm_zero_terms_parent.json -- the commit before the terms the compiler knows to be zero (the base at
   rest, one-component velocities, the CRBA column seed, zero link offsets: known_zero / zmul / zadd / zsub) were taken out.  This is what
   holds "the results stay what they were": the header may only drop terms that are exactly zero for every finite input, and reorder
   nothing that rounds.  (The program runs BOTH forms with those terms left out; the product's scalar-form kernels keep them.)
   Regenerate (only from a tree whose results are the reference):  python tests/test_arm_zero_terms_cpu.py --write <commit>
3. The double results agree with the fp64 oracle's bias and mass matrix (so100o_forward, as tests/test_hostcheck.py uses it).  Bound: the
   larger of test_hostcheck's (M 1e-15, bias 1e-13) and twice the worst error of the recorded build on these states, which the test
   measures from the recorded words: M 2.8e-17, bias 1.6e-15 -- so the bounds are test_hostcheck's own, 1e-15 and 1e-13."""
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "arm_zero_terms_parent.json")
NSTATES, NWORDS = 87, 48
LABELS = {"random": 64, "rest": 1, "v=0": 4, "one_joint": 12, "limits": 4, "v=-0": 2}
HOSTCHECK_BOUND_M, HOSTCHECK_BOUND_BIAS = 1e-15, 1e-13          # tests/test_hostcheck.py::test_dynamics_and_poses_match_oracle, fp64


def run_armcheck(exe):
    """-> (states [(label, q[6], v[6])], results {(type, pk): [[hex word] * 48] * states})"""
    subprocess.check_call(["make", "-C", os.path.join(HERE, "_armcheck"), "-s", f"OUT={exe}"])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    states, res = [], {}
    for line in out.splitlines():
        w = line.split()
        if w[0] == "S":
            assert int(w[1]) == len(states)
            # (nine digits name a float; the double the program used is that float's value, not the decimal's)
            states.append((w[2], [float(np.float32(x)) for x in w[3:9]], [float(np.float32(x)) for x in w[9:15]]))
        elif w[0] == "R":
            rows = res.setdefault((w[1], int(w[2])), [])
            assert int(w[3]) == len(rows) and len(w) == 4 + NWORDS
            rows.append(w[4:])
    return states, res


@pytest.fixture(scope="module")
def current(tmp_path_factory):
    return run_armcheck(str(tmp_path_factory.mktemp("armcheck") / "armcheck"))


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def same_but_zero_sign(a, b):
    """two hex words equal, or both a zero (all bits clear below the sign bit)"""
    if a == b:
        return True
    top = 1 << (4*len(a) - 1)
    return len(a) == len(b) and (int(a, 16) & ~top) == 0 and (int(b, 16) & ~top) == 0


def as_doubles(words):
    return np.array([struct.unpack("<d", struct.pack("<Q", int(w, 16)))[0] for w in words])


def bias_and_mass(words):
    """bias[6] and the full symmetric M[6, 6] of one fp64 result row"""
    x = as_doubles(words[:27])
    M = np.zeros((6, 6))
    for i in range(6):
        for j in range(i + 1):
            M[i, j] = M[j, i] = x[6 + i*(i + 1)//2 + j]
    return x[:6], M


def oracle_errors(states, rows):
    """worst |M - oracle| and |bias - oracle| of fp64 result rows over the states"""
    import ctypes as C
    from oracle import so100_oracle as O
    from scenes import L, M as MODEL, fresh
    wm = wb = 0.0
    for (label, q, v), words in zip(states, rows):
        d = fresh(np.array(q), np.array(v)); L.so100o_forward(C.byref(MODEL), C.byref(d), 0, 0)
        Mo = O.arr(d.M).reshape(12, 12)[:6, :6]; bo = O.arr(d.qfrc_bias)[:6]
        b, Mh = bias_and_mass(words)
        assert np.isfinite(b).all() and np.isfinite(Mh).all(), label
        wm = max(wm, np.abs(Mh - Mo).max()); wb = max(wb, np.abs(b - bo).max())
    return wm, wb


def test_the_state_list_is_the_stated_one(current, golden):
    states, res = current
    assert len(states) == NSTATES
    assert {k: sum(1 for s in states if s[0] == k) for k in LABELS} == LABELS
    assert set(res) == {("f", 1), ("f", 0), ("d", 1), ("d", 0)} and all(len(r) == NSTATES for r in res.values())
    assert [[s[0], s[1], s[2]] for s in states] == golden["states"]          # the recorded results belong to these states
    rest = states[64]
    assert rest[0] == "rest" and not any(rest[1]) and not any(rest[2])
    assert all(str(x) == "-0.0" for s in states[-2:] for x in s[2])


def test_pair_form_equals_scalar_form_bit_for_bit(current):
    _, res = current
    for t in ("f", "d"):
        bad = [i for i in range(NSTATES) if res[(t, 1)][i] != res[(t, 0)][i]]
        assert not bad, (t, bad)


def test_results_equal_the_recorded_commits(current, golden):
    states, res = current
    for t, key in (("f", "float"), ("d", "double")):
        bad = []
        for i in range(NSTATES):
            want = golden[key][i].split()
            assert len(want) == NWORDS
            for pk in (0, 1):
                for k, (a, b) in enumerate(zip(res[(t, pk)][i], want)):
                    if not same_but_zero_sign(a, b):
                        bad.append((states[i][0], i, pk, k, a, b))
        assert not bad, (key, len(bad), bad[:8])


def test_double_results_agree_with_the_oracle(current, golden):
    states, res = current
    pm, pb = oracle_errors(states, [row.split() for row in golden["double"]])
    bound_m, bound_b = max(HOSTCHECK_BOUND_M, 2*pm), max(HOSTCHECK_BOUND_BIAS, 2*pb)
    print(f"recorded build ({golden['commit']}): worst |M - oracle| {pm:.2e}  |bias - oracle| {pb:.2e}  -> bounds {bound_m:.2e} {bound_b:.2e}")
    for pk in (1, 0):
        wm, wb = oracle_errors(states, res[("d", pk)])
        print(f"this build, PK = {pk}: worst |M - oracle| {wm:.2e}  |bias - oracle| {wb:.2e}")
        assert wm < bound_m and wb < bound_b, (pk, wm, wb)


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--write":
        raise SystemExit(__doc__)
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        st, rs = run_armcheck(os.path.join(d, "armcheck"))
    for t in ("f", "d"):
        assert rs[(t, 1)] == rs[(t, 0)], "pair and scalar form differ: not a tree to record"
    doc = {"commit": sys.argv[2],
           "what": "tests/_armcheck/armcheck.cpp built from that commit's so100_physics.hpp (g++ -O2 -ffp-contract=off): per state the bit "
                   "patterns of bias[6], M[21] (arm_mass) and the LDL^T factor[21]; pair form and scalar form printed the same words",
           "states": [[s[0], s[1], s[2]] for s in st],
           "float": [" ".join(r) for r in rs[("f", 0)]], "double": [" ".join(r) for r in rs[("d", 0)]]}
    with open(GOLDEN, "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")
    print(f"wrote {GOLDEN}: {len(st)} states")
