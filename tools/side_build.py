"""Build a side library with extra preprocessor defines (experiments; the product library is untouched):
    python tools/side_build.py <suffix> -DNAME=VALUE ...     ->  so100_mujoco_rl_amd/libso100sim_<suffix>.so
The recipe is csrc/Makefile's own (OUT / OBJDIR / EXTRA): every object of the product, the same flags plus the given ones; the objects
and resource tables go to a directory of their own, outside csrc.
Use it through SO100_LIB=<path> (so100_mujoco_rl_amd/lib.py)."""
import os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
suffix, defs = sys.argv[1], sys.argv[2:]
csrc = os.path.join(ROOT, "so100_mujoco_rl_amd", "csrc")
odir = os.path.join(ROOT, "gpurun_out", "side_obj_" + suffix); os.makedirs(odir, exist_ok=True)
out = os.path.join(ROOT, "so100_mujoco_rl_amd", f"libso100sim_{suffix}.so")
subprocess.check_call(["make", "-j9", "-C", csrc, "OUT=" + out, "OBJDIR=" + odir, "EXTRA=" + " ".join(defs)])
print("built", out)
