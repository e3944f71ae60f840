"""tests/hostlibs.py declares the signature of every symbol the host twins export: the extern "C" definitions of
tests/_hostcheck/hostcheck.cpp, tests/_rendercheck/rendercheck.cpp, the four sources of tests/_learncheck, tests/_querycheck/querycheck.cpp
and the later queries' twins (tests/_forwardcheck, _trajcheck, _derivcheck, _lqrcheck) are parsed and held against the argtypes / restype of
the loaded libraries.  A symbol added to a .cpp without its line in hostlibs.py fails here, not in whichever test calls it first.  The stand-alone programs of tests/Makefile's selftest target are built and run here too, so
that they stay buildable for a host sanitizer run.  CPU only."""
import ctypes as C
import os
import re
import subprocess

import hostlibs

SCALARS = {"int": C.c_int, "unsigned": C.c_uint, "long": C.c_long, "float": C.c_float, "double": C.c_double, "unsigned long long": C.c_ulonglong}
RETURNS = {"void": None, "void*": C.c_void_p, "int": C.c_int, "long": C.c_long}
PREFIXES = "hc|rc|lc|rn|on|sc|qc|fc|tc|dc|lq"


def expand_macros(src):
    """every function-like #define of `src` (querycheck.cpp stamps its exports out per scalar type) applied to its own-line uses"""
    src = src.replace("\\\n", " ")
    for name, formals, body in re.findall(r"^#define (\w+)\(([^)]*)\)(.*)$", src, flags=re.M):
        def stamp(use):
            text = body
            for formal, actual in zip(formals.split(","), use.group(1).split(",")):
                text = re.sub(r"\b%s\b" % formal.strip(), actual.strip(), text)
            return text.replace("##", "").replace("} ", "}\n")
        src = re.sub(r"^%s\(([^)]*)\)$" % name, stamp, src, flags=re.M)
    return src


def defined_symbols(path):
    """{name: (restype, argtypes)} of the function definitions in a .cpp whose names begin with one of PREFIXES (all of them are extern "C")"""
    src = expand_macros(re.sub(r"//[^\n]*", "", open(path).read()))
    out = {}
    for ret, name, params in re.findall(r'^\s*(?:extern "C" )?(void\*?|int|long)\s+((?:%s)_\w+)\s*\(([^)]*)\)\s*\{' % PREFIXES, src, flags=re.M):
        args = []
        for prm in [x.strip() for x in params.split(",")]:
            if prm in ("", "void"):
                continue
            args.append(C.c_void_p if "*" in prm else SCALARS[" ".join(prm.split()[:-1])])      # (the last word is the parameter's name)
        out[name] = (RETURNS[ret], args)
    return out


def test_every_exported_symbol_has_its_signature_declared():
    learn = ["_learncheck/%s.cpp" % s for s in ("learncheck", "rewnormcheck", "obsnormcheck", "shufflecheck")]
    for load, sources, table in ((hostlibs.hostcheck, ["_hostcheck/hostcheck.cpp"], hostlibs.HOSTCHECK),
                                 (hostlibs.rendercheck, ["_rendercheck/rendercheck.cpp"], hostlibs.RENDERCHECK),
                                 (hostlibs.learncheck, learn, hostlibs.LEARNCHECK),
                                 (hostlibs.querycheck, ["_querycheck/querycheck.cpp"], hostlibs.QUERYCHECK),
                                 (hostlibs.forwardcheck, ["_forwardcheck/forwardcheck.cpp"], hostlibs.FORWARDCHECK),
                                 (hostlibs.trajcheck, ["_trajcheck/trajcheck.cpp"], hostlibs.TRAJCHECK),
                                 (hostlibs.derivcheck, ["_derivcheck/derivcheck.cpp"], hostlibs.DERIVCHECK),
                                 (hostlibs.lqrcheck, ["_lqrcheck/lqrcheck.cpp"], hostlibs.LQRCHECK)):
        want = {}
        for src in sources:
            found = defined_symbols(os.path.join(hostlibs.HERE, src))
            assert found and not set(found) & set(want), src
            want.update(found)
        assert len(want) >= 2 and sorted(want) == sorted(table)
        lib = load()
        for name, (restype, argtypes) in want.items():
            fn = getattr(lib, name)
            assert fn.argtypes is not None and list(fn.argtypes) == argtypes, name
            assert fn.restype is restype, name           # (ctypes' default is c_int: a `long` or pointer result needs its own)
    assert sum(name.startswith("lc_") for name in hostlibs.LEARNCHECK) >= 9
    assert [len(t) for t in (hostlibs.FORWARDCHECK, hostlibs.TRAJCHECK, hostlibs.DERIVCHECK, hostlibs.LQRCHECK)] == [2, 2, 2, 2]     # one entry per precision


def test_selftest_programs_build_and_pass(tmp_path):
    """make selftest without a sanitizer: each *_MAIN program is built into tmp_path, runs, and reports ok"""
    run = subprocess.run(["make", "-C", hostlibs.HERE, "-s", "selftest", f"BUILD={tmp_path}"], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    for line in ("rewnormcheck selftest: ok", "obsnormcheck selftest: ok"):
        assert line in run.stdout, run.stdout
    for precision in ("double", "float"):
        for name in ("querycheck", "forwardcheck", "trajcheck", "derivcheck", "lqrcheck"):
            assert re.search(r"%s selftest \(%s\):.*: ok$" % (name, precision), run.stdout, flags=re.M), run.stdout
