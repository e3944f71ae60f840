"""Side builds (tools/side_build.py, tools/rollout_prof.py build) go through csrc/Makefile's one recipe: OUT / OBJDIR / EXTRA give every
object of the product with the product's flags plus the extra ones, and a library made that way loads through SO100_LIB.  The dry run
checks the recipe for a full side build (which compiles for minutes); the library that is really loaded is linked from the product's
own objects, which is the same link line.  CPU only."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "so100_mujoco_rl_amd", "csrc")
OBJECTS = ["so100_sim.o", "so100_render.o", "so100_learn.o"] + [f"so100_kind{k}.o" for k in range(1, 7)]

pytestmark = pytest.mark.skipif(shutil.which("make") is None or not os.path.exists("/opt/rocm/bin/hipcc"), reason="no build tools here")


def dry_run(*make_vars):
    """the command lines of a full build (-B: whatever is up to date), nothing run: {object name: words} and the link line's words"""
    out = subprocess.run(["make", "-n", "-B", "-C", CSRC] + list(make_vars), capture_output=True, text=True, check=True).stdout
    compiles, link = {}, None
    for line in out.splitlines():
        words = line.split(" 2> ")[0].split()
        if words and words[0].endswith("hipcc"):
            compiles[os.path.basename(words[words.index("-o") + 1])] = words
        elif words and words[0] == "g++":
            assert link is None
            link = words
    return compiles, link


def test_side_build_recipe_is_the_products_with_the_extra_flags(tmp_path):
    product, product_link = dry_run()
    odir, out = str(tmp_path / "obj"), str(tmp_path / "libso100sim_x.so")
    side, side_link = dry_run("OUT=" + out, "OBJDIR=" + odir, "EXTRA=-DX=1 -DY")
    assert sorted(product) == sorted(side) == sorted(OBJECTS)
    for name in OBJECTS:
        p, s = product[name], side[name]
        assert p[p.index("-o") + 1] == name and s[s.index("-o") + 1] == os.path.join(odir, name)
        strip = lambda w: [x for i, x in enumerate(w) if x != "-o" and w[i - 1] != "-o"]
        assert [x for x in strip(s) if x not in ("-DX=1", "-DY")] == strip(p), name       # the product's command line ...
        assert s.index("-DX=1") < s.index("-c") and s.index("-DY") < s.index("-c"), name  # ... and the extra flags, on every object
    objs = lambda w: [x for x in w if x.endswith(".o")]
    assert objs(product_link) == OBJECTS and objs(side_link) == [os.path.join(odir, o) for o in OBJECTS]
    assert side_link[side_link.index("-o") + 1] == out and "-Wl,--no-undefined" in side_link
    assert [x for x in side_link if not x.endswith(".o") and x != out] == [x for x in product_link if not x.endswith(".o") and x != "../libso100sim.so"]


def test_tools_call_the_makefile_and_hold_no_flags_of_their_own(monkeypatch):
    import runpy
    calls = []
    monkeypatch.setattr(subprocess, "check_call", lambda cmd, **kw: calls.append(cmd))
    monkeypatch.setattr(sys, "argv", ["side_build.py", "ab", "-DA=1", "-DB"])
    runpy.run_path(os.path.join(ROOT, "tools", "side_build.py"), run_name="__main__")
    assert len(calls) == 1
    cmd = calls[0]
    assert cmd[0] == "make" and cmd[cmd.index("-C") + 1] == CSRC
    assert "OUT=" + os.path.join(ROOT, "so100_mujoco_rl_amd", "libso100sim_ab.so") in cmd and "EXTRA=-DA=1 -DB" in cmd
    odir = [w[len("OBJDIR="):] for w in cmd if w.startswith("OBJDIR=")][0]
    top = os.path.relpath(odir, ROOT).split(os.sep)[0]
    assert os.path.isdir(odir) and os.path.basename(odir) == "side_obj_ab"
    assert top + "/" in open(os.path.join(ROOT, ".gitignore")).read().split()          # objects land in a directory git ignores
    os.rmdir(odir)
    jobs = [int(m.group(1)) for m in (re.fullmatch(r"-j(\d+)", w) for w in cmd) if m]
    assert len(jobs) == 1 and 1 <= jobs[0] <= 16
    for name in ("side_build.py", "rollout_prof.py"):
        src = open(os.path.join(ROOT, "tools", name)).read()
        assert not re.search(r"hipcc|offload-arch|-O[0-3]\b|-std=|-fPIC|-shared|g\+\+", src), name
    assert "side_build.py" in open(os.path.join(ROOT, "tools", "rollout_prof.py")).read()


def test_a_library_from_the_recipe_loads_through_SO100_LIB(tmp_path):
    """OUT alone: the product's objects (up to date after the build: test_abi.py), linked a second time beside the product"""
    out = str(tmp_path / "libso100sim_side.so")
    subprocess.run(["make", "-j7", "-C", CSRC, "OUT=" + out], capture_output=True, text=True, check=True)
    code = ("from so100_mujoco_rl_amd import lib; L = lib.load(); assert lib.LIB_PATH == %r; "
            "assert all(hasattr(L, s) for s in lib.EXPORTS + lib.LEARN_EXPORTS); print(L.so100_abi_version())" % out)
    env = dict(os.environ, SO100_LIB=out, PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.strip() == "3", res.stderr[-2000:]
