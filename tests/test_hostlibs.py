"""tests/hostlibs.py declares the signature of every symbol the host twins export: the extern "C" definitions of
tests/_hostcheck/hostcheck.cpp, tests/_rendercheck/rendercheck.cpp, the four sources of tests/_learncheck, tests/_querycheck/querycheck.cpp
and the later queries' twins (tests/_forwardcheck, _trajcheck, _derivcheck, _lqrcheck, _closedcheck, _costcheck, _mppicheck, _cemcheck) are parsed and held against the argtypes / restype of
the loaded libraries.  A symbol added to a .cpp without its line in hostlibs.py fails here, not in whichever test calls it first.  The stand-alone programs of tests/Makefile's selftest target are built and run here too, so
that they stay buildable for a host sanitizer run.  CPU only."""
import ctypes as C
import os
import re
import subprocess

import pytest

import hostlibs

SCALARS = {"int": C.c_int, "unsigned": C.c_uint, "long": C.c_long, "float": C.c_float, "double": C.c_double, "unsigned long long": C.c_ulonglong}
RETURNS = {"void": None, "void*": C.c_void_p, "int": C.c_int, "long": C.c_long}
PREFIXES = "hc|rc|lc|rn|on|sc|qc|fc|tc|dc|lq|cc|ck|mp|cm"


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


LEARN = ["_learncheck/%s.cpp" % s for s in ("learncheck", "rewnormcheck", "obsnormcheck", "shufflecheck")]
# name: (loader, sources, table)
LIBRARIES = {"hostcheck": (hostlibs.hostcheck, ["_hostcheck/hostcheck.cpp"], hostlibs.HOSTCHECK),
             "rendercheck": (hostlibs.rendercheck, ["_rendercheck/rendercheck.cpp"], hostlibs.RENDERCHECK),
             "learncheck": (hostlibs.learncheck, LEARN, hostlibs.LEARNCHECK),
             "querycheck": (hostlibs.querycheck, ["_querycheck/querycheck.cpp"], hostlibs.QUERYCHECK),
             "forwardcheck": (hostlibs.forwardcheck, ["_forwardcheck/forwardcheck.cpp"], hostlibs.FORWARDCHECK),
             "trajcheck": (hostlibs.trajcheck, ["_trajcheck/trajcheck.cpp"], hostlibs.TRAJCHECK),
             "derivcheck": (hostlibs.derivcheck, ["_derivcheck/derivcheck.cpp"], hostlibs.DERIVCHECK),
             "lqrcheck": (hostlibs.lqrcheck, ["_lqrcheck/lqrcheck.cpp"], hostlibs.LQRCHECK),
             "closedcheck": (hostlibs.closedcheck, ["_closedcheck/closedcheck.cpp"], hostlibs.CLOSEDCHECK),
             "costcheck": (hostlibs.costcheck, ["_costcheck/costcheck.cpp"], hostlibs.COSTCHECK),
             "mppicheck": (hostlibs.mppicheck, ["_mppicheck/mppicheck.cpp"], hostlibs.MPPICHECK),
             "cemcheck": (hostlibs.cemcheck, ["_cemcheck/cemcheck.cpp"], hostlibs.CEMCHECK)}
# the twins of the four newest queries: each a case of its own in the two parametrised tests below; name: (its symbols, the runs its program reports)
LATER = {"closedcheck": (["cc_closed_loop_d", "cc_closed_loop_f"], ["(double)", "(float)"]),
         "costcheck": (["ck_select_d", "ck_select_f", "ck_terms_d", "ck_terms_f"], ["(double)", "(float)"]),
         "mppicheck": (["mp_blend_d", "mp_blend_f", "mp_sample_d", "mp_sample_f"], ["(double)", "(float)"]),
         "cemcheck": (["cm_key_disagreements", "cm_refit_d", "cm_refit_f", "cm_sample_d", "cm_sample_f"], ["(double)", "(float)", "(keys)"])}


def check_table(load, sources, table):
    """the extern "C" definitions of `sources` are `table`, and the loaded library carries each one's argtypes and restype"""
    want = {}
    for src in sources:
        found = defined_symbols(os.path.join(hostlibs.HERE, src))
        assert found and not set(found) & set(want), src
        want.update(found)
    assert len(want) >= 2 and want == table            # the names, and what the source says of each
    lib = load()
    for name, (restype, argtypes) in want.items():
        fn = getattr(lib, name)
        assert fn.argtypes is not None and list(fn.argtypes) == argtypes, name
        assert fn.restype is restype, name           # (ctypes' default is c_int: a `long` or pointer result needs its own)


def test_every_exported_symbol_has_its_signature_declared():
    for name in LIBRARIES:
        check_table(*LIBRARIES[name])
    assert sum(name.startswith("lc_") for name in hostlibs.LEARNCHECK) >= 9
    assert [len(t) for t in (hostlibs.FORWARDCHECK, hostlibs.TRAJCHECK, hostlibs.DERIVCHECK, hostlibs.LQRCHECK)] == [2, 2, 2, 2]     # one entry per precision


@pytest.mark.parametrize("name", sorted(LATER))
def test_a_later_twins_table_matches_its_source(name):
    """what tests/test_{closed_loop,cost,mppi,cem}_cpu.py each held their own twin to: exactly these symbols, as its source defines them"""
    load, sources, table = LIBRARIES[name]
    check_table(load, sources, table)
    assert sorted(table) == LATER[name][0]


@pytest.fixture(scope="module")
def selftest(tmp_path_factory):
    """make selftest without a sanitizer, once: each *_MAIN program is built into a temporary directory and run"""
    build = tmp_path_factory.mktemp("selftest")
    return subprocess.run(["make", "-C", hostlibs.HERE, "-s", "selftest", f"BUILD={build}"], capture_output=True, text=True)


def test_selftest_programs_build_and_pass(selftest):
    """every program builds, runs and reports ok"""
    run = selftest
    assert run.returncode == 0, run.stdout + run.stderr
    for line in ("rewnormcheck selftest: ok", "obsnormcheck selftest: ok"):
        assert line in run.stdout, run.stdout
    for precision in ("double", "float"):
        for name in ("querycheck", "forwardcheck", "trajcheck", "derivcheck", "lqrcheck", "closedcheck", "costcheck", "mppicheck", "cemcheck"):
            assert re.search(r"%s selftest \(%s\):.*: ok$" % (name, precision), run.stdout, flags=re.M), run.stdout


@pytest.mark.parametrize("name", sorted(LATER))
def test_a_later_twins_stand_alone_program_passes(selftest, name):
    """the program a host sanitizer run uses (make -C tests selftest SAN=...), here without a sanitizer: its lines, in its order, every one ok"""
    assert selftest.returncode == 0, selftest.stdout + selftest.stderr
    runs = LATER[name][1]
    lines = [l for l in selftest.stdout.splitlines() if l.startswith(name + " selftest")]
    assert len(lines) == len(runs) and all(l.endswith(": ok") and r in l for l, r in zip(lines, runs)), selftest.stdout
