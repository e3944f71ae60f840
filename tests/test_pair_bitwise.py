"""The pair form of the arm dynamics (so100_physics.hpp: V2, LinkFwdP / LinkBwdP / CrbP) against the one-vector-at-a-time
form on the host, in float and double, compiled without FMA contraction: every bias, mass-matrix and
sin / cos-update entry must agree bit for bit on random joint states.  CPU only."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_pair_form_bitwise_equals_scalar_form(tmp_path):
    exe = str(tmp_path / "pair_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-o", exe,
                           os.path.join(HERE, "_pairbits", "pair_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "float: 20000 trials, 0 mismatches" in r.stdout
    assert "double: 20000 trials, 0 mismatches" in r.stdout
