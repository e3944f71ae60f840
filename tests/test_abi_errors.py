"""Every failure of both C ABIs (include/so100_sim.h, include/so100_learn.h) that is reachable without a GPU, with its exact return
code and the exact bytes so100_last_error() then holds: each argument check of the two create calls in source order, the null-handle
check of every other entry point, the missing-device error, and the thread-local message slot.  The strings were recorded from the
library as it stood before the host layer under the two ABIs was unified; the messages are part of the ABI's behaviour.  CPU only."""
import ctypes as C
import os
import threading

import pytest
import torch

INVALID, NODEVICE = -1, -2


@pytest.fixture(scope="module")
def L():
    from so100_mujoco_rl_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        lib.build()
    return lib.load()


def sim_cfg(**over):
    from so100_mujoco_rl_amd import lib
    kw = dict(env_kind=1, num_envs=16, device=0, flags=lib.F_CUBE_PINNED, solver_iters=2, contact_iters=6, frame_skip=16, max_episode_steps=0,
              seed=0, env_id_offset=0, envs_per_workgroup=0)
    kw.update(over)
    return lib.Config(*[kw[f[0]] for f in lib.Config._fields_])


def learner_cfg(**over):
    from so100_mujoco_rl_amd import lib
    kw = dict(obs_dim=15, device=0, max_minibatch=64, gamma=0.99, gae_lambda=0.95, clip_range=0.2, vf_coef=0.5, max_grad_norm=0.5, lr=3e-4,
              beta1=0.9, beta2=0.999, adam_eps=1e-5)
    kw.update(over)
    return lib.LearnerConfig(*[kw[f[0]] for f in lib.LearnerConfig._fields_])


# so100_create's argument checks in source order: (config overrides, message).  Each row breaks one rule only.
CREATE = [
    (dict(env_kind=0), b"so100_create: env_kind must be 1..6"),
    (dict(env_kind=7), b"so100_create: env_kind must be 1..6"),
    (dict(num_envs=0), b"so100_create: num_envs must be >= 1"),
    (dict(solver_iters=0), b"so100_create: solver_iters must be in 1..64"),
    (dict(solver_iters=65), b"so100_create: solver_iters must be in 1..64"),
    (dict(contact_iters=0), b"so100_create: contact_iters must be in 1..64"),
    (dict(contact_iters=65), b"so100_create: contact_iters must be in 1..64"),
    (dict(frame_skip=0), b"so100_create: frame_skip must be in 1..1024"),
    (dict(frame_skip=1025), b"so100_create: frame_skip must be in 1..1024"),
    (dict(max_episode_steps=-1), b"so100_create: max_episode_steps must be >= 0"),
    (dict(flags=256), b"so100_create: unknown flag bits"),
    (dict(flags=32 | 8), b"so100_create: SO100_F_PADS_CUBE / SO100_F_LINKS_CUBE need a dynamic cube (not SO100_F_CUBE_PINNED)"),
    (dict(flags=128 | 8), b"so100_create: SO100_F_PADS_CUBE / SO100_F_LINKS_CUBE need a dynamic cube (not SO100_F_CUBE_PINNED)"),
    (dict(envs_per_workgroup=8), b"so100_create: envs_per_workgroup must be 0 (automatic), 16, 32 or 64"),
    (dict(envs_per_workgroup=48), b"so100_create: envs_per_workgroup must be 0 (automatic), 16, 32 or 64"),
    (dict(flags=4 | 8), b"so100_create: SO100_F_FLOOR and SO100_F_CUBE_PINNED are mutually exclusive"),
]
# two rules broken at once: the earlier check in the source answers
CREATE_ORDER = [
    (dict(env_kind=0, num_envs=0), b"so100_create: env_kind must be 1..6"),
    (dict(max_episode_steps=-1, flags=256), b"so100_create: max_episode_steps must be >= 0"),
    (dict(flags=4 | 8 | 32), b"so100_create: SO100_F_PADS_CUBE / SO100_F_LINKS_CUBE need a dynamic cube (not SO100_F_CUBE_PINNED)"),
    (dict(flags=4 | 8, envs_per_workgroup=8), b"so100_create: envs_per_workgroup must be 0 (automatic), 16, 32 or 64"),
]

LEARNER_CREATE = [
    (dict(obs_dim=7), b"so100_learner_create: obs_dim must be 15 or 8, got 7"),
    (dict(obs_dim=-3), b"so100_learner_create: obs_dim must be 15 or 8, got -3"),
    (dict(max_minibatch=0), b"so100_learner_create: max_minibatch must be >= 1, got 0"),
    (dict(max_minibatch=-5), b"so100_learner_create: max_minibatch must be >= 1, got -5"),
    (dict(gamma=-0.1), b"so100_learner_create: gamma must be in [0, 1]"),
    (dict(gamma=1.5), b"so100_learner_create: gamma must be in [0, 1]"),
    (dict(gamma=float("nan")), b"so100_learner_create: gamma must be in [0, 1]"),
    (dict(gae_lambda=-0.1), b"so100_learner_create: gae_lambda must be in [0, 1]"),
    (dict(gae_lambda=1.5), b"so100_learner_create: gae_lambda must be in [0, 1]"),
    (dict(clip_range=0.0), b"so100_learner_create: clip_range must be > 0"),
    (dict(vf_coef=-1.0), b"so100_learner_create: vf_coef must be >= 0"),
    (dict(max_grad_norm=0.0), b"so100_learner_create: max_grad_norm must be > 0"),
    (dict(lr=-1.0), b"so100_learner_create: lr must be >= 0"),
    (dict(beta1=1.0), b"so100_learner_create: beta1 and beta2 must be in [0, 1)"),
    (dict(beta2=-0.1), b"so100_learner_create: beta1 and beta2 must be in [0, 1)"),
    (dict(adam_eps=0.0), b"so100_learner_create: adam_eps must be > 0"),
    (dict(obs_dim=7, max_minibatch=0), b"so100_learner_create: obs_dim must be 15 or 8, got 7"),       # source order
    (dict(lr=-1.0, adam_eps=0.0), b"so100_learner_create: lr must be >= 0"),
]


def null_handle_calls(L):
    """(label, call, message): every entry point that takes a handle or a required pointer, given NULL for it.  All return SO100_E_INVALID."""
    from so100_mujoco_rl_amd import lib
    h = C.c_void_p()
    dummy = C.c_void_p(16)              # a non-null pointer that is never dereferenced: the null check of another argument answers first
    return [
        ("create(NULL cfg)", lambda: L.so100_create(None, C.byref(h)), b"so100_create: null argument"),
        ("create(NULL out)", lambda: L.so100_create(C.byref(sim_cfg()), None), b"so100_create: null argument"),
        ("reset", lambda: L.so100_reset(None, None, None, dummy, None), b"so100_reset: null handle"),
        ("step(NULL sim)", lambda: L.so100_step(None, C.byref(lib.StepIO()), None), b"so100_step: null argument"),
        ("policy_forward", lambda: L.so100_policy_forward(None, C.byref(lib.PolicyWeights()), C.byref(lib.PolicyIO()), 0, None),
         b"so100_policy_forward: null argument"),
        ("rollout", lambda: L.so100_rollout(None, C.byref(lib.PolicyWeights()), C.byref(lib.RolloutIO()), 4, 0, None), b"so100_rollout: null argument"),
        ("render", lambda: L.so100_render(None, C.byref(lib.RenderIO()), None), b"so100_render: null argument"),
        ("get_state", lambda: L.so100_get_state(None, dummy, dummy, None), b"so100_get_state: null argument"),
        ("set_state", lambda: L.so100_set_state(None, dummy, dummy, None), b"so100_set_state: null argument"),
        ("get_field", lambda: L.so100_get_field(None, 0, dummy, None), b"so100_get_field: bad argument"),
        ("set_field", lambda: L.so100_set_field(None, 0, dummy, None), b"so100_set_field: bad argument"),
        ("learner_create(NULL cfg)", lambda: L.so100_learner_create(None, C.byref(h)), b"so100_learner_create: null argument"),
        ("learner_create(NULL out)", lambda: L.so100_learner_create(C.byref(learner_cfg()), None), b"so100_learner_create: null argument"),
        ("learner_advantages", lambda: L.so100_learner_advantages(None, C.byref(lib.AdvantagesIO()), 2, 16, None),
         b"so100_learner_advantages: null argument"),
        ("learner_minibatch_step", lambda: L.so100_learner_minibatch_step(None, C.byref(lib.MinibatchIO()), None),
         b"so100_learner_minibatch_step: null argument"),
    ]


def test_create_argument_checks_in_source_order(L):
    for over, msg in CREATE + CREATE_ORDER:
        h = C.c_void_p(1)
        assert L.so100_create(C.byref(sim_cfg(**over)), C.byref(h)) == INVALID, over
        assert L.so100_last_error() == msg, (over, L.so100_last_error())
        assert not h.value, over                # *out is cleared before the first check of the configuration


def test_learner_create_argument_checks_in_source_order(L):
    for over, msg in LEARNER_CREATE:
        h = C.c_void_p(1)
        assert L.so100_learner_create(C.byref(learner_cfg(**over)), C.byref(h)) == INVALID, over
        assert L.so100_last_error() == msg, (over, L.so100_last_error())          # read back through the simulator's so100_last_error
        assert not h.value, over


def test_null_handle_of_every_entry_point(L):
    for label, call, msg in null_handle_calls(L):
        assert call() == INVALID, label
        assert L.so100_last_error() == msg, (label, L.so100_last_error())


def test_calls_that_fail_or_return_without_a_message(L):
    """metadata calls answer with a negative value and leave the message slot alone; destroying nothing is quiet"""
    from so100_mujoco_rl_amd import lib
    assert L.so100_create(C.byref(sim_cfg(num_envs=0)), C.byref(C.c_void_p())) == INVALID
    before = L.so100_last_error()
    assert before == b"so100_create: num_envs must be >= 1"
    assert L.so100_envs_per_workgroup(None) == INVALID
    assert L.so100_destroy(None) is None and L.so100_learner_destroy(None) is None
    assert L.so100_obs_dim(0) == -1 and L.so100_state_field_index(None) == -1 and L.so100_state_field_index(b"nope") == -1
    L.so100_state_field_name.restype = C.c_char_p
    assert L.so100_state_field_name(-1) is None and L.so100_state_field_name(L.so100_num_state_fields()) is None
    assert L.so100_learner_num_params(7) == INVALID
    for fn in (L.so100_learner_param_offset, L.so100_learner_param_size):
        assert fn(15, b"nope") == INVALID and fn(15, None) == INVALID and fn(7, lib.POLICY_TENSORS[0].encode()) == INVALID
    assert L.so100_last_error() == before


def test_missing_device_is_an_error_of_both_creates(L):
    if not torch.cuda.is_available():
        h = C.c_void_p(1)
        assert L.so100_create(C.byref(sim_cfg()), C.byref(h)) == NODEVICE and not h.value
        assert L.so100_last_error() == b"so100_create: no HIP device available (this library has no CPU fallback)"
        h = C.c_void_p(1)
        assert L.so100_learner_create(C.byref(learner_cfg()), C.byref(h)) == NODEVICE and not h.value
        assert L.so100_last_error() == b"so100_learner_create: no HIP device available (this library has no CPU fallback)"
        # an argument check still answers before the device is looked for
        assert L.so100_create(C.byref(sim_cfg(flags=4 | 8)), C.byref(h)) == INVALID
        assert L.so100_learner_create(C.byref(learner_cfg(adam_eps=0.0)), C.byref(h)) == INVALID


def test_no_message_holds_a_stray_percent_sign(L):
    from so100_mujoco_rl_amd import lib
    msgs = [m for _, m in CREATE + CREATE_ORDER + LEARNER_CREATE] + [m for _, _, m in null_handle_calls(L)]
    assert len(set(msgs)) >= 30 and not [m for m in msgs if b"%" in m]
    for _, call, _ in null_handle_calls(L):
        call()
        assert b"%" not in L.so100_last_error()
    assert lib.ABI_VERSION == L.so100_abi_version() == 3


def test_message_slot_is_one_per_thread(L):
    """one slot for both headers, thread-local: a thread that never failed reads an empty string, its own failure does not
    disturb the message another thread holds"""
    assert L.so100_learner_create(C.byref(learner_cfg(obs_dim=7)), C.byref(C.c_void_p())) == INVALID
    mine = b"so100_learner_create: obs_dim must be 15 or 8, got 7"
    assert L.so100_last_error() == mine
    seen = {}

    def other():
        seen["fresh"] = L.so100_last_error()
        seen["rc"] = L.so100_reset(None, None, None, None, None)
        seen["own"] = L.so100_last_error()

    t = threading.Thread(target=other)
    t.start(); t.join()
    assert seen == {"fresh": b"", "rc": INVALID, "own": b"so100_reset: null handle"}
    assert L.so100_last_error() == mine
    assert L.so100_step(None, None, None) == INVALID and L.so100_last_error() == b"so100_step: null argument"      # the sim's failure replaces the learner's
