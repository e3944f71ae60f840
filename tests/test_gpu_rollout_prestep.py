"""Substep 0's state-only half beside the policy heads (csrc/so100_rollout.hpp: physics_phase_mw with PRE).  In the contact-disabled
rollout kernels waves 1 and 2 compute the exact sin/cos, the RNEA bias and the factorised mass matrix of a step's FIRST substep from the
(q, v) that wave 0 published at the end of the previous step, while wave 0 is still sampling the action.  The way this goes wrong is a
stale start state: the step after an auto-reset must start its substep 0 from the RESET q, v, and the first step of a launch from the
loaded ones.

Kinds 1, 2, 5 with the contact-disabled flags; 32 envs per workgroup with n = 33 (a one-env workgroup) and 96, 64 per workgroup with
n = 65; frame_skip 1 (the peeled substep is the only one), 2 and 16; max_episode_steps = 2 and T = 3, so every episode ends inside the
chunk.  The persistent rollout is compared row by row with stepwise policy_forward + step through the 4-wave step kernel and through the
one-wave kernel (SO100_MW_MAX_ENVS = 0), with the tolerances of test_gpu_parity.py::test_persistent_rollout_equals_stepwise; two
identical launches, and one T = 3 launch against three T = 1 launches from the same start (prologue path against in-loop path), must
agree bit for bit."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from gpu_support import make_sim, one_wave_step_kernel, policy_tensors   # noqa: E402
from scenes import FREE                                   # noqa: E402

T = 3
KEYS = ("buf", "obs", "rew", "done", "trunc", "q", "v")


def _policy(obs_dim, device):
    from so100_mujoco_rl_amd.collector import RolloutCollector
    sd = RolloutCollector.random_policy_state(obs_dim, device, seed=2)
    sd["log_std"] = sd["log_std"] - 0.5
    return policy_tensors(sd)


def _run(kind, n, epw, frame_skip, mode):
    """mode: "persistent" (one so100_rollout launch of T steps), "chunks" (T launches of one step), "stepwise" (policy_forward + step,
    4-wave step kernel), "one_wave" (the same with so100_step_fused: gpu_support.one_wave_step_kernel)"""
    with one_wave_step_kernel(mode == "one_wave"):
        sim = make_sim(kind, n, flags=FREE, frame_skip=frame_skip, seed=4, max_episode_steps=2, envs_per_workgroup=epw)
    assert sim.envs_per_workgroup == epw
    sim.set_policy(_policy(sim.obs_dim, sim.device))
    sim.reset()
    buf = torch.zeros(T, n, sim.obs_dim + 10, device=sim.device)
    if mode == "persistent":
        sim.rollout(buf, 0)
    elif mode == "chunks":
        for t in range(T):
            sim.rollout(buf[t:t + 1], t)
    else:
        act = torch.zeros(n, 6, device=sim.device)
        for t in range(T):
            sim.policy_forward(sim.obs, act, t, rollout_row=buf[t])
            sim.step(act, rollout_row=buf[t])
    q, v = sim.get_state()
    torch.cuda.synchronize()
    return dict(buf=buf.clone(), obs=sim.obs.clone(), rew=sim.rew.clone(), done=sim.done.clone(), trunc=sim.trunc.clone(), q=q, v=v)


def _close(a, b, od):
    """test_persistent_rollout_equals_stepwise's bounds: 1e-6 on everything but the rewards (2e-5), joint velocities 1e-5"""
    cols = torch.full((od + 10,), 1e-6, device=a["buf"].device); cols[od + 6] = 2e-5
    return {"buf": ((a["buf"] - b["buf"]).abs() / cols).max().item(),
            "obs": (a["obs"] - b["obs"]).abs().max().item() / 1e-6, "rew": (a["rew"] - b["rew"]).abs().max().item() / 2e-5,
            "q": (a["q"] - b["q"]).abs().max().item() / 1e-6, "v": (a["v"] - b["v"]).abs().max().item() / 1e-5}


@pytest.mark.parametrize("frame_skip", [1, 2, 16])
@pytest.mark.parametrize("epw,n", [(32, 33), (32, 96), (64, 65)])
@pytest.mark.parametrize("kind", [1, 2, 5])
def test_prestep_rollout_against_stepwise_kernels(kind, epw, n, frame_skip):
    p1 = _run(kind, n, epw, frame_skip, "persistent")
    p2 = _run(kind, n, epw, frame_skip, "persistent")
    for k in KEYS:
        assert torch.equal(p1[k], p2[k]), f"two identical launches differ in {k}"
    c = _run(kind, n, epw, frame_skip, "chunks")
    for k in KEYS:
        assert torch.equal(p1[k], c[k]), f"one launch of {T} steps and {T} launches of one step differ in {k}"
    od = p1["obs"].shape[1]
    assert p1["buf"][..., od + 7].sum() > 0                  # the 2-step TimeLimit ends every episode inside the chunk (auto-reset runs)
    for mode in ("stepwise", "one_wave"):
        s = _run(kind, n, epw, frame_skip, mode)
        worst = _close(p1, s, od)
        print(f"kind {kind} n {n} epw {epw} frame_skip {frame_skip} vs {mode}: worst difference / bound " + "  ".join(f"{k} {x:.3f}" for k, x in worst.items()))
        assert all(x <= 1.0 for x in worst.values()), (mode, worst)
        assert torch.equal(p1["done"], s["done"]) and torch.equal(p1["trunc"], s["trunc"]), mode
