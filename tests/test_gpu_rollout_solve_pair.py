"""The substep's solve and integration in pair form in the 32-row contact-disabled rollout kernels (csrc/so100_rollout.hpp: PSOLVE, DESIGN.md
section 8k): behind the peeled substep wave 0 holds q, v, qc and the integration increment as the joint pairs (0,1), (2,3), (4,5) round the
substep loop and the servo force across the mid-substep barrier; tau, the forward substitution and the integration run on the pairs, and the
pairs go back into the env state behind the loop.  What can go wrong: a half taken from the wrong joint, a pair packed from a stale q or v
(frame_skip 1 and 2 are the edges: the peeled substep alone -- packed and unpacked with no loop pass between -- and exactly one pass), a
state that is not unpacked before the step's epilogue or the auto-reset reads it, a clamp applied to the wrong half, dead lanes leaking.

Kinds 1, 2, 5; (envs per workgroup, n) = (32, 33): a workgroup with one live env, (32, 96): full workgroups, and as controls the kernels that
keep the text they had, (64, 65) and (16, 17); frame_skip 1, 2, 16; max_episode_steps = 2 and T = 3, so every episode ends inside the chunk.
The policy has zero head weights and std = 0 (log_std = -104), so the action is its bias row: "zeros" (the servo holds the reset pose, v = 0),
and "saturated": +-1 on alternating joints with the joint velocities set to -+(9 + env mod 5 / 2) rad/s behind the reset.  An action moves the
target by 0.075 rad at the most (3.75 N m of the 35 N m force range), so it is the damping term kv v >= 4.47 * 9 N m that takes the servo force
to its clamp on every joint, with the sign the action has; the clamped force then brakes the joint, and within the env step every joint leaves
the clamp again, so both sides of it are run.

Required: rows, terminal observations and the final state within test_persistent_rollout_equals_stepwise's bounds of the 4-wave and the
one-wave step kernel; one launch of three steps bit-equal to three launches of one; n = 33 bit-equal to the first 33 envs of n = 96.

The parent commit passes this file unchanged (all 72 cases: it computes the same bits on scalars)."""
import functools

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from gpu_support import make_sim, one_wave_step_kernel          # noqa: E402
from scenes import FREE                                         # noqa: E402
from test_gpu_rollout_prestep import KEYS, T, _policy           # noqa: E402

ACTIONS = {"zeros": [0.0, 0.0, 0.0, 0.0, 0.0, 0.0],
           "saturated": [100.0, -100.0, 100.0, -100.0, 100.0, -100.0]}      # the env sees +-1
KEYS_T = KEYS + ("tobs",)
KV_MIN, KP_STEP, FORCE = 4.47, 50.0*0.075, 35.0                 # smallest joint damping, kp times the largest target offset, the force range


def _constant_policy(obs_dim, device, action):
    t = _policy(obs_dim, device)
    t["mu_w"] = torch.zeros_like(t["mu_w"])
    t["mu_b"] = torch.tensor(ACTIONS[action], dtype=torch.float32, device=device)
    t["log_std"] = torch.full((6,), -104.0, dtype=torch.float32, device=device)       # expf underflows: std = 0, the raw action is the mean
    return t


@functools.lru_cache(maxsize=None)
def _run(kind, n, epw, frame_skip, action, mode):
    """mode: "persistent" (one so100_rollout launch of T steps), "chunks" (T launches of one step), "stepwise" (policy_forward + step, 4-wave
    step kernel), "one_wave" (the same with so100_step_fused).  Results are shared between cases and never written to."""
    with one_wave_step_kernel(mode == "one_wave"):
        sim = make_sim(kind, n, flags=FREE, frame_skip=frame_skip, seed=4, max_episode_steps=2, envs_per_workgroup=epw)
    assert sim.envs_per_workgroup == epw
    sim.set_policy(_constant_policy(sim.obs_dim, sim.device, action))
    sim.reset()
    if action == "saturated":
        q0, v0 = sim.get_state()
        q0, v0 = q0.clone(), v0.clone()
        speed = 9.0 + 0.5*(torch.arange(n, device=sim.device) % 5).float()
        assert KV_MIN*speed.min().item() - KP_STEP > FORCE     # the clamp is reached whatever sign the offset has
        sign = torch.tensor(ACTIONS[action], device=sim.device).sign()
        v0[:6] = -sign[:, None]*speed[None, :]
        sim.set_state(q0.contiguous(), v0.contiguous())
    buf = torch.zeros(T, n, sim.obs_dim + 10, device=sim.device)
    tobs = torch.zeros(T, n, sim.obs_dim, device=sim.device)
    if mode == "persistent":
        sim.rollout(buf, 0, terminal_obs_chunk=tobs)
    elif mode == "chunks":
        for t in range(T):
            sim.rollout(buf[t:t + 1], t, terminal_obs_chunk=tobs[t:t + 1])
    else:
        act = torch.zeros(n, 6, device=sim.device)
        for t in range(T):
            sim.policy_forward(sim.obs, act, t, rollout_row=buf[t])
            sim.step(act, rollout_row=buf[t], terminal_obs=tobs[t])
    q, v = sim.get_state()
    torch.cuda.synchronize()
    return dict(buf=buf.clone(), tobs=tobs.clone(), obs=sim.obs.clone(), rew=sim.rew.clone(), done=sim.done.clone(), trunc=sim.trunc.clone(),
                q=q.clone(), v=v.clone())


def _worst(a, b, od):
    """test_persistent_rollout_equals_stepwise's bounds: 1e-6 on everything but the rewards (2e-5), joint velocities 1e-5; the terminal
    observations are observations (1e-6).  Returned as difference / bound."""
    cols = torch.full((od + 10,), 1e-6, device=a["buf"].device); cols[od + 6] = 2e-5
    d = lambda k: (a[k] - b[k]).abs()
    return {"buf": (d("buf") / cols).max().item(), "tobs": d("tobs").max().item() / 1e-6, "obs": d("obs").max().item() / 1e-6,
            "rew": d("rew").max().item() / 2e-5, "q": d("q").max().item() / 1e-6, "v": d("v").max().item() / 1e-5}


@pytest.mark.parametrize("action", ["saturated", "zeros"])
@pytest.mark.parametrize("frame_skip", [1, 2, 16])
@pytest.mark.parametrize("epw,n", [(32, 33), (32, 96), (64, 65), (16, 17)])
@pytest.mark.parametrize("kind", [1, 2, 5])
def test_pair_form_solve_against_step_kernels(kind, epw, n, frame_skip, action):
    p1 = _run(kind, n, epw, frame_skip, action, "persistent")
    od = p1["obs"].shape[1]
    for k in KEYS_T:
        assert torch.isfinite(p1[k].float()).all(), k
    # ---- the action the policy was built for reached the env: the raw action is the bias row in every row
    assert torch.equal(p1["buf"][..., od:od + 6], torch.tensor(ACTIONS[action], device=p1["buf"].device).expand(T, n, 6))
    # ---- every episode ends at its second step: row 1 carries the done code, its terminal observation is written, row 2 starts from the reset
    assert (p1["buf"][1, :, od + 7] > 0).all() and (p1["buf"][0, :, od + 7] == 0).all() and (p1["buf"][2, :, od + 7] == 0).all()
    assert (p1["tobs"][1].abs().sum(1) > 0).all() and (p1["tobs"][0] == 0).all() and (p1["tobs"][2] == 0).all()
    # ---- one launch of three steps against three launches of one (the pairs are unpacked into the state every step either way)
    c = _run(kind, n, epw, frame_skip, action, "chunks")
    for k in KEYS_T:
        assert torch.equal(p1[k], c[k]), f"one launch of {T} steps and {T} launches of one step differ in {k}"
    # ---- dead lanes do not leak: the one-live-env workgroup of n = 33 against the same envs in full workgroups
    if (epw, n) == (32, 33):
        full = _run(kind, 96, 32, frame_skip, action, "persistent")
        assert torch.equal(p1["buf"], full["buf"][:, :n]), "rows of n = 33 differ from the first 33 envs' rows of n = 96"
        assert torch.equal(p1["tobs"], full["tobs"][:, :n])
        assert torch.equal(p1["q"], full["q"][..., :n]) and torch.equal(p1["v"], full["v"][..., :n])
    # ---- rows, terminal observations and the final state against both step kernels
    for mode in ("stepwise", "one_wave"):
        s = _run(kind, n, epw, frame_skip, action, mode)
        assert torch.equal(p1["buf"][0, :, :od], s["buf"][0, :, :od]), "the two do not start from the same reset observation"
        worst = _worst(p1, s, od)
        print(f"kind {kind} n {n} epw {epw} frame_skip {frame_skip} {action} vs {mode}: worst difference / bound " + "  ".join(f"{k} {x:.3f}" for k, x in worst.items()))
        assert all(x <= 1.0 for x in worst.values()), (mode, worst)
        assert torch.equal(p1["done"], s["done"]) and torch.equal(p1["trunc"], s["trunc"]), mode
