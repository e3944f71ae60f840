"""The substep loop of the multi-wave kernels (csrc/so100_rollout.hpp: physics_phase_mw) at the loop lengths where a value wrongly
treated as dead, or wrongly carried, between its iterations would show: frame_skip 1 and 2 (first / second iteration) and 16 (shipped).

Env01, 96 and 64 envs at 32 envs per workgroup (three / two workgroups of the 32-row rollout kernel for the contact-disabled flags),
T = 3 steps.  The persistent rollout is compared row by row with the stepwise policy_forward + step sequence twice: through the 4-wave
step kernel (the same substep loop in another kernel) and through the one-wave so100_step_fused (physics_substeps: a loop of its own),
selected by the library's dispatch override.  Tolerances: those of test_gpu_parity.py::test_persistent_rollout_equals_stepwise.
Two identical launches must agree bit for bit."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from gpu_support import make_sim, one_wave_step_kernel, policy_tensors   # noqa: E402
from scenes import ARM, FREE, REFP                        # noqa: E402

T = 3
KEYS = ("buf", "obs", "rew", "done", "trunc", "q", "v")


def _policy(obs_dim, device):
    from so100_mujoco_rl_amd.collector import RolloutCollector
    sd = RolloutCollector.random_policy_state(obs_dim, device, seed=2)
    sd["log_std"] = sd["log_std"] - 0.5
    return policy_tensors(sd)


def _run(flags, n, frame_skip, mode):
    """mode: "persistent" (one so100_rollout launch), "stepwise" (policy_forward + step, 4-wave step kernel), "one_wave" (the same
    with so100_step_fused: gpu_support.one_wave_step_kernel)"""
    with one_wave_step_kernel(mode == "one_wave"):
        sim = make_sim(1, n, flags=flags, frame_skip=frame_skip, seed=4, max_episode_steps=2, envs_per_workgroup=32)
    assert sim.envs_per_workgroup == 32
    sim.set_policy(_policy(sim.obs_dim, sim.device))
    sim.reset()
    buf = torch.zeros(T, n, sim.obs_dim + 10, device=sim.device)
    if mode == "persistent":
        sim.rollout(buf, 0)
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
    worst = {"buf": ((a["buf"] - b["buf"]).abs() / cols).max().item(),
             "obs": (a["obs"] - b["obs"]).abs().max().item() / 1e-6, "rew": (a["rew"] - b["rew"]).abs().max().item() / 2e-5,
             "q": (a["q"] - b["q"]).abs().max().item() / 1e-6, "v": (a["v"] - b["v"]).abs().max().item() / 1e-5}
    return worst


@pytest.mark.parametrize("frame_skip", [1, 2, 16])
@pytest.mark.parametrize("n", [96, 64])
@pytest.mark.parametrize("flags", [FREE, ARM, REFP], ids=["free", "arm", "reference"])
def test_substep_loop_against_stepwise_kernels(flags, n, frame_skip):
    p1 = _run(flags, n, frame_skip, "persistent")
    p2 = _run(flags, n, frame_skip, "persistent")
    for k in KEYS:
        assert torch.equal(p1[k], p2[k]), f"two identical launches differ in {k}"
    od = p1["obs"].shape[1]
    assert p1["buf"][..., od + 7].sum() > 0                  # the 2-step TimeLimit ends every episode inside the chunk (auto-reset runs)
    for mode in ("stepwise", "one_wave"):
        s = _run(flags, n, frame_skip, mode)
        worst = _close(p1, s, od)
        print(f"flags {flags} n {n} frame_skip {frame_skip} vs {mode}: worst difference / bound " + "  ".join(f"{k} {x:.3f}" for k, x in worst.items()))
        assert all(x <= 1.0 for x in worst.values()), (mode, worst)
        assert torch.equal(p1["done"], s["done"]) and torch.equal(p1["trunc"], s["trunc"]), mode
