"""The one place that builds and loads the host twins of the device code: tests/_hostcheck/libhostcheck.so (physics, contacts, task
layer, random draws), tests/_rendercheck/librendercheck.so (render), tests/_learncheck/liblearncheck.so (the learner: lc_ its arithmetic,
rn_ reward normalisation, on_ observation normalisation, sc_ the shuffle; four sources, one library), tests/_querycheck/libquerycheck.so
(the four original model queries) and one library each for the later queries: tests/_forwardcheck/libforwardcheck.so (forward dynamics),
tests/_trajcheck/libtrajcheck.so (trajectory), tests/_derivcheck/libderivcheck.so (derivatives), tests/_lqrcheck/liblqrcheck.so (LQR),
tests/_closedcheck/libclosedcheck.so (closed loop), tests/_costcheck/libcostcheck.so (cost terms and selection), tests/_mppicheck/libmppicheck.so
(sampling planner) and tests/_cemcheck/libcemcheck.so (cross-entropy planner; the last three share tests/planner_twin.hpp).
tests/Makefile is the one recipe for all of them.  Each is made once per process and cached; argtypes and restype are declared here for EVERY exported symbol (tests/test_hostlibs.py holds
the tables to the extern "C" definitions), so that no call depends on which test ran first: a `long` result without its restype is
silently cut to 32 bits, a Python float without argtypes raises."""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))

_p, _i, _u, _l, _f, _d, _ull = C.c_void_p, C.c_int, C.c_uint, C.c_long, C.c_float, C.c_double, C.c_ulonglong

# name: (restype, argtypes); every pointer parameter is a c_void_p (numpy arrays through ptr(), C.byref() of a scalar, or None)
HOSTCHECK = {
    "hc_dyn_d": (None, [_p]*4), "hc_dyn_f": (None, [_p]*4),
    "hc_sub_d": (None, [_p]*5 + [_u, _i, _i]), "hc_sub_f": (None, [_p]*5 + [_u, _i, _i]),
    "hc_poses_d": (None, [_p]*2), "hc_poses_f": (None, [_p]*2),
    "hc_cube_d": (None, [_p]*5 + [_u, _i, _i]), "hc_cube_f": (None, [_p]*5 + [_u, _i, _i]),
    "hc_sincos_f": (None, [_f, _p, _p]),
    "hc_dbg_counters": (None, [_p]),
    "hc_capbox_d": (_i, [_p, _p, _d] + [_p]*6), "hc_capbox_f": (_i, [_p, _p, _d] + [_p]*6),
    "hc_csub_d": (None, [_p]*3 + [_u, _i, _i, _i, _p]), "hc_csub_f": (None, [_p]*3 + [_u, _i, _i, _i, _p]),
    "hc_boxbox_d": (_i, [_p]*9), "hc_boxbox_f": (_i, [_p]*9),
    "hc_cdbg_trace": (None, [_i]),
    "hc_cdbg_counters": (None, [_p]),
    "hc_cdbg_passes": (_l, []), "hc_cdbg_signpasses": (_l, []), "hc_cdbg_gradpasses": (_l, []), "hc_cdbg_lastiter": (_l, []),
    "hc_cdbg_hist": (None, [_p, _i]),
    "hc_contact_id_hash": (_i, [_i]),
    "hc_env_new": (_p, [_i]),
    "hc_env_free": (None, [_p]),
    "hc_env_reset": (None, [_p, _i, _ull, _u, _p, _p]),
    "hc_env_step": (None, [_p, _i, _u, _i, _i, _i, _ull, _u] + [_p]*7),
    "hc_env_stats": (None, [_p, _p]),
    "hc_env_qpos": (None, [_p]*3),
    "hc_env_set_state": (None, [_p]*5),
    "hc_philox4x32": (None, [_p]*3),
    "hc_draw8": (None, [_ull, _u, _u, _i, _p]),
    "hc_policy_noise": (None, [_ull, _u, _u, _p]),
    "hc_policy_noise_pairs": (None, [_p, _p, _l, _p, _p]),
}
RENDERCHECK = {
    "rc_record_floats": (_i, []),
    "rc_render": (_i, [_p, _i, _i, _i, _i, _u] + [_p]*5),
}

LEARNCHECK = {
    "lc_num_params": (_i, [_i]),
    "lc_tensor_offset": (_i, [_i, _i]),
    "lc_tensor_size": (_i, [_i, _i]),
    "lc_gae_d": (None, [_i, _p, _p, _p, _l, _p, _d, _d, _d, _p, _p, _l]),
    "lc_gae_f": (None, [_i, _p, _p, _p, _l, _p, _f, _f, _f, _p, _p, _l]),
    "lc_head_d": (None, [_p, _p]), "lc_head_f": (None, [_p, _p]),
    "lc_head_ex_d": (None, [_p, _p]), "lc_head_ex_f": (None, [_p, _p]),
    "lc_adam_d": (None, [_i, _p, _p, _p, _p, _d, _p]),
    "lc_adam_f": (None, [_i, _p, _p, _p, _p, _f, _p]),
    "rn_block": (_i, []),
    "rn_normalize": (None, [_i]*5 + [_p, _d, _d, _d, _p, _p]),
    "on_block": (_i, []), "on_group": (_i, []),
    "on_update": (None, [_l, _i, _i, _p, _p]),
    "on_fold": (None, [_i, _i, _p, _p, _d, _p, _p, _p]),
    "on_normalize": (None, [_l, _i, _p, _p, _p]),
    "sc_shuffle": (None, [_ull, _u, _l, _p]),
    "sc_shuffle_epochs": (None, [_ull, _u, _i, _i, _p]),
}
QUERYCHECK = {
    "qc_kinematics_d": (None, [_l] + [_p]*6), "qc_kinematics_f": (None, [_l] + [_p]*6),
    "qc_jacobian_d": (None, [_l, _p, _i, _p, _p, _p]), "qc_jacobian_f": (None, [_l, _p, _i, _p, _p, _p]),
    "qc_dynamics_d": (None, [_l] + [_p]*6), "qc_dynamics_f": (None, [_l] + [_p]*6),
    "qc_ik_d": (None, [_l, _p, _p, _i, _p, _i, _d, _d, _d] + [_p]*4), "qc_ik_f": (None, [_l, _p, _p, _i, _p, _i, _f, _f, _f] + [_p]*4),
    "qc_joint_range": (None, [_p]),
}
FORWARDCHECK = {
    "fc_forward_d": (None, [_l] + [_p]*3 + [_u, _i, _i] + [_p]*12), "fc_forward_f": (None, [_l] + [_p]*3 + [_u, _i, _i] + [_p]*12),
}
_SIG = (None, [_l] + [_p]*4 + [_i, _i, _i, _u, _i, _i] + [_p]*10)
TRAJCHECK = {"tc_trajectory_d": _SIG, "tc_trajectory_f": _SIG}
DERIVCHECK = {"dc_derivatives_d": (None, [_l] + [_p]*4 + [_i, _i, _u, _i, _i, _d] + [_p]*5),
              "dc_derivatives_f": (None, [_l] + [_p]*4 + [_i, _i, _u, _i, _i, _f] + [_p]*5)}
LQRCHECK = {"lq_lqr_d": (None, [_l, _i, _i] + [_p]*9 + [_d]*4 + [_p]*8),
            "lq_lqr_f": (None, [_l, _i, _i] + [_p]*9 + [_f]*4 + [_p]*8)}
CLOSEDCHECK = {"cc_closed_loop_d": (None, [_l] + [_p]*4 + [_i, _i, _i, _u, _i, _i] + [_p]*4 + [_i, _p, _p, _i, _p, _i, _d, _d] + [_p]*11),
               "cc_closed_loop_f": (None, [_l] + [_p]*4 + [_i, _i, _i, _u, _i, _i] + [_p]*4 + [_i, _p, _p, _i, _p, _i, _f, _f] + [_p]*11)}
COSTCHECK = {"ck_terms_d": (None, [_l, _i, _i, _i, _i] + [_p]*9), "ck_terms_f": (None, [_l, _i, _i, _i, _i] + [_p]*9),
             "ck_select_d": (None, [_l, _i, _i, _i, _i] + [_p]*11), "ck_select_f": (None, [_l, _i, _i, _i, _i] + [_p]*11)}
MPPICHECK = {"mp_sample_d": (None, [_l, _i, _i, _p, _p, _d, _d, _ull, _u, _u] + [_p]*5), "mp_sample_f": (None, [_l, _i, _i, _p, _p, _f, _f, _ull, _u, _u] + [_p]*5),
             "mp_blend_d": (None, [_l, _i, _i, _i, _i] + [_p]*7 + [_d, _i, _i] + [_p]*7), "mp_blend_f": (None, [_l, _i, _i, _i, _i] + [_p]*7 + [_f, _i, _i] + [_p]*7)}
CEMCHECK = {"cm_sample_d": (None, [_l, _i, _i, _p, _p, _d, _d, _ull, _u, _u] + [_p]*5), "cm_sample_f": (None, [_l, _i, _i, _p, _p, _f, _f, _ull, _u, _u] + [_p]*5),
            "cm_refit_d": (None, [_l, _i, _i, _i, _i] + [_p]*7 + [_i, _d] + [_p]*5 + [_i, _i] + [_p]*9),
            "cm_refit_f": (None, [_l, _i, _i, _i, _i] + [_p]*7 + [_i, _f] + [_p]*5 + [_i, _i] + [_p]*9),
            "cm_key_disagreements": (_l, [_l, _p])}

_libs = {}


def _load(target, signatures, make_vars=()):
    """`target` of tests/Makefile (a path under tests/ or an absolute one), made and loaded once"""
    path = os.path.join(HERE, target)
    if path not in _libs:
        subprocess.check_call(["make", "-C", HERE, "-s", target] + list(make_vars))
        lib = C.CDLL(path)
        for name, (restype, argtypes) in signatures.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
        _libs[path] = lib
    return _libs[path]


def hostcheck(out="libhostcheck.so", extra=""):
    """tests/_hostcheck/hostcheck.cpp built into `out` (a name in tests/_hostcheck or an absolute path) with the compiler arguments
    `extra` after the Makefile's own, e.g. -DSO100_MODEL_GEN_HEADER=... for a second generated model"""
    path = os.path.join(HERE, "_hostcheck", out)
    return _load(path, HOSTCHECK, [f"OUT={path}", f"EXTRA={extra}"])


def rendercheck():
    return _load("_rendercheck/librendercheck.so", RENDERCHECK)


def learncheck():
    return _load("_learncheck/liblearncheck.so", LEARNCHECK)


def querycheck():
    return _load("_querycheck/libquerycheck.so", QUERYCHECK)


def forwardcheck():
    return _load("_forwardcheck/libforwardcheck.so", FORWARDCHECK)


def trajcheck():
    return _load("_trajcheck/libtrajcheck.so", TRAJCHECK)


def derivcheck():
    return _load("_derivcheck/libderivcheck.so", DERIVCHECK)


def lqrcheck():
    return _load("_lqrcheck/liblqrcheck.so", LQRCHECK)


def closedcheck():
    return _load("_closedcheck/libclosedcheck.so", CLOSEDCHECK)


def costcheck():
    return _load("_costcheck/libcostcheck.so", COSTCHECK)


def mppicheck():
    return _load("_mppicheck/libmppicheck.so", MPPICHECK)


def cemcheck():
    return _load("_cemcheck/libcemcheck.so", CEMCHECK)


def ptr(a):
    """the data pointer of a numpy array, for a c_void_p parameter; None (a null pointer) passes through"""
    return None if a is None else a.ctypes.data_as(C.c_void_p)
