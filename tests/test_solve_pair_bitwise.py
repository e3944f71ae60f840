"""The pair form of the substep's solve path (so100_physics.hpp: arm_mass_p + ldl6_p, arm_tau_p, ldl6_forward_p / ldl6_back_p, arm_integrate_p)
against the scalar helpers (arm_mass + ldl6, arm_tau, ldl6_solve, arm_integrate) on the host, in float and double, compiled without FMA
contraction: the mass matrix, its factor and D^-1, tau, the forward substitution, the solved acceleration and the integrated q, v, qc, dq must
agree bit for bit on 20 000 random cases of M = arm_mass(q) with
right-hand sides up to the force clamp, and a NaN in one joint's acceleration must leave the other half of its pair untouched.  CPU only."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_solve_pair_form_bitwise_equals_scalar_form(tmp_path):
    exe = str(tmp_path / "solve_pair_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-o", exe,
                           os.path.join(HERE, "_solvepair", "solve_pair_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "float: 20000 trials, 0 mismatches" in r.stdout
    assert "double: 20000 trials, 0 mismatches" in r.stdout
