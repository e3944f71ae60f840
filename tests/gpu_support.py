"""What the test_gpu_* modules share (imported by them only: it needs torch and the HIP library): handles, state injection, the
GPU / oracle pair stepped on identical inputs, and the float references of the policy."""
import contextlib
import ctypes as C
import os

import numpy as np
import torch

from oracle import so100_oracle as O
from scenes import JS, L, M, fresh

LOG2PI_HALF = 0.9189385332046727


def make_sim(*a, **k):
    from so100_mujoco_rl_amd.lib import So100Sim
    return So100Sim(*a, **k)


@contextlib.contextmanager
def one_wave_step_kernel(on=True):
    """A handle created inside this block steps through the one-wave kernel so100_step_fused at every batch size instead of the 4-wave
    so100_step_mw: SO100_MW_MAX_ENVS = 0 is read by so100_create, so only the creation has to be inside.  The variable is put back as
    it was on the way out; on=False leaves everything alone (callers pass their mode test)."""
    if not on:
        yield
        return
    old = os.environ.get("SO100_MW_MAX_ENVS")
    os.environ["SO100_MW_MAX_ENVS"] = "0"
    try:
        yield
    finally:
        if old is None:
            del os.environ["SO100_MW_MAX_ENVS"]
        else:
            os.environ["SO100_MW_MAX_ENVS"] = old


def inject_state(sim, qpos, qvel):
    """qpos [n, 13], qvel [n, 12] (numpy) -> the handle's state rows, as contiguous float32 (after a reset every other row is at its
    post-reset value)"""
    sim.set_state(torch.from_numpy(np.ascontiguousarray(qpos.T, np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(qvel.T, np.float32)).cuda())


def policy_tensors(sd):
    """an SB3-keyed policy state dict as the kernels' tensors (So100Sim.set_policy)"""
    from so100_mujoco_rl_amd.lib import POLICY_TENSORS, SB3_STATE_DICT_KEYS
    return {k: sd[SB3_STATE_DICT_KEYS[k]].contiguous() for k in POLICY_TENSORS}


def oracle_step(qpos, qvel, act, flags, nsub=16):
    """raw oracle physics from the injected state: returns final qpos, qvel and the per-substep pad-contact counts.
    (ctrl is formed with an fp64 add here -- substep_harness.oracle_substep rounds the sum to fp32: they are not the same function)"""
    d = fresh()
    O.arr(d.qpos)[:] = qpos.astype(np.float32).astype(np.float64); O.arr(d.qvel)[:] = qvel.astype(np.float32).astype(np.float64)
    O.arr(d.ctrl)[:] = O.arr(d.qpos)[:6] + (act.astype(np.float32)*JS).astype(np.float64)      # env01_v1.py:18-24 in NumPy-2 promotion
    counts = []
    for _ in range(nsub):
        L.so100o_step(C.byref(M), C.byref(d), flags, -1, 1)
        counts.append((sum(1 for i in range(d.ncon) if d.con[i].kind == 1), sum(1 for i in range(d.ncon) if d.con[i].kind == 2)))
    return O.arr(d.qpos).copy(), O.arr(d.qvel).copy(), counts


def run_pair(kind, flags, n, steps, seed, action_scale=1.0, solver_iters=4, contact_iters=6, max_steps=0, inject=True, pad_iters=None):
    """Step n envs on the GPU and in the oracle with identical actions / uniforms; yield per-step results.
    Oracle solver: PGS on the dual to 1e-15 -- or its primal Newton when pad rows are simulated (PGS needs ~1e4 sweeps on them).
    pad_iters: (solver_iters, contact_iters) when pad rows are simulated (default: solver_iters, 30)."""
    rs = np.random.RandomState(seed)
    pads = (flags & (O.F_PADS_FLOOR | O.F_PADS_CUBE)) != 0
    if pads:
        solver_iters, contact_iters = pad_iters or (solver_iters, 30)
    sim = make_sim(kind, n, flags=flags, solver_iters=solver_iters, contact_iters=contact_iters, max_episode_steps=max_steps, seed=seed)
    orc = [O.OracleEnv(kind, flags=flags, iters=-1 if pads else 0, seed=seed, env_id=i) for i in range(n)]
    for e in orc:
        e.e.max_episode_steps = max_steps
    inj = rs.random_sample((n, 16)).astype(np.float32)
    obs_g = sim.reset(inject=torch.from_numpy(inj).cuda() if inject else None).cpu().numpy().copy()
    obs_o = np.stack([e.reset(inject=inj[i] if inject else None) for i, e in enumerate(orc)])
    yield -1, sim, orc, obs_g, obs_o, None, None, None, None
    for t in range(steps):
        a = np.clip(rs.uniform(-1, 1, (n, 6)) * action_scale, -1, 1).astype(np.float32)
        inj = rs.random_sample((n, 16)).astype(np.float32)
        og, rg, dg, tg = sim.step(torch.from_numpy(a).cuda(), inject=torch.from_numpy(inj).cuda() if inject else None)
        res = [e.step(a[i], inject=inj[i] if inject else None, autoreset=True) for i, e in enumerate(orc)]
        oo = np.stack([r[0] for r in res]); ro = np.array([r[1] for r in res])
        do = np.array([r[2] or r[3] for r in res]); to = np.array([r[3] and not r[2] for r in res])
        yield t, sim, orc, og.cpu().numpy().copy(), oo, (rg.cpu().numpy().copy(), ro), (dg.cpu().numpy().copy(), do), (tg.cpu().numpy().copy(), to), res


def state_err(sim, orc):
    qpos, qvel = sim.get_state()
    qpos = qpos.cpu().numpy().T; qvel = qvel.cpu().numpy().T
    qo = np.stack([O.arr(e.d.qpos).copy() for e in orc]); vo = np.stack([O.arr(e.d.qvel).copy() for e in orc])
    return np.abs(qpos - qo).max(), np.abs(qvel - vo).max()


def torch_policy(t, obs, noise):
    """(action, value, log-prob) of the policy in plain PyTorch, in the dtype of its arguments"""
    h = torch.tanh(obs @ t["pi_w0"].T + t["pi_b0"]); h = torch.tanh(h @ t["pi_w1"].T + t["pi_b1"])
    mean = h @ t["mu_w"].T + t["mu_b"]
    g = torch.tanh(obs @ t["vf_w0"].T + t["vf_b0"]); g = torch.tanh(g @ t["vf_w1"].T + t["vf_b1"])
    value = (g @ t["v_w"].T + t["v_b"]).squeeze(1)
    act = mean + t["log_std"].exp() * noise
    logp = (-0.5 * noise ** 2 - t["log_std"] - LOG2PI_HALF).sum(1)
    return act, value, logp
