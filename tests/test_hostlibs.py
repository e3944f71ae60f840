"""tests/hostlibs.py declares the signature of every symbol the host twins export: the extern "C" definitions of
tests/_hostcheck/hostcheck.cpp, tests/_rendercheck/rendercheck.cpp and tests/_learncheck/learncheck.cpp are parsed and held against the
argtypes / restype of the loaded libraries.  A symbol added to a .cpp without its line in hostlibs.py fails here, not in whichever test
calls it first.  CPU only."""
import ctypes as C
import os
import re

import hostlibs

SCALARS = {"int": C.c_int, "unsigned": C.c_uint, "long": C.c_long, "float": C.c_float, "double": C.c_double, "unsigned long long": C.c_ulonglong}
RETURNS = {"void": None, "void*": C.c_void_p, "int": C.c_int, "long": C.c_long}


def defined_symbols(path):
    """{name: (restype, argtypes)} of the hc_* / rc_* / lc_* function definitions in a .cpp (all of them are extern "C")"""
    src = re.sub(r"//[^\n]*", "", open(path).read())
    out = {}
    for ret, name, params in re.findall(r'^(?:extern "C" )?(void\*?|int|long)\s+((?:hc|rc|lc)_\w+)\s*\(([^)]*)\)\s*\{', src, flags=re.M):
        args = []
        for prm in [x.strip() for x in params.split(",")]:
            if prm in ("", "void"):
                continue
            args.append(C.c_void_p if "*" in prm else SCALARS[" ".join(prm.split()[:-1])])      # (the last word is the parameter's name)
        out[name] = (RETURNS[ret], args)
    return out


def test_every_exported_symbol_has_its_signature_declared():
    for load, src, table in ((hostlibs.hostcheck, "_hostcheck/hostcheck.cpp", hostlibs.HOSTCHECK),
                             (hostlibs.rendercheck, "_rendercheck/rendercheck.cpp", hostlibs.RENDERCHECK),
                             (hostlibs.learncheck, "_learncheck/learncheck.cpp", hostlibs.LEARNCHECK)):
        want = defined_symbols(os.path.join(hostlibs.HERE, src))
        assert len(want) >= 2 and sorted(want) == sorted(table)
        lib = load()
        for name, (restype, argtypes) in want.items():
            fn = getattr(lib, name)
            assert fn.argtypes is not None and list(fn.argtypes) == argtypes, name
            assert fn.restype is restype, name           # (ctypes' default is c_int: a `long` or pointer result needs its own)
