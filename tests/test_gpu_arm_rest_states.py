"""The arm dynamics on the device at the states where a term that csrc/so100_physics.hpp leaves out as "known to be zero" would show if it
were not zero, and where a random batch would hide it: the arm at rest at q = 0, v = 0 at random angles, every joint moving alone (both
signs), every joint at a limit, v = -0.0.  (tests/test_arm_zero_terms_cpu.py holds the same states bit for bit on the host.)

Env01, contact disabled (the benchmark's flags), 64 envs at 32 per workgroup, frame_skip 1 and 16, T = 2 steps.  The first 23 envs are put
into the special states through set_field after the reset; the other 41 keep their random reset states.  The persistent rollout (the pair
form of RNEA / CRBA, one wave each) is compared with the stepwise policy_forward + step sequence through the 4-wave step kernel and through
the one-wave so100_step_fused (the scalar form), under the bounds of test_gpu_substep_loop.py::_close: 1e-6, rewards 2e-5, joint velocities
1e-5.  Everything must be finite, and two identical launches must agree bit for bit."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from gpu_support import make_sim, one_wave_step_kernel    # noqa: E402
from scenes import FREE, JNT_HI, JNT_LO                   # noqa: E402
from test_gpu_substep_loop import KEYS, _close, _policy   # noqa: E402

N, T = 64, 2


def special_states():
    """(q [23, 6], v [23, 6]) float32: rest, 4 x v = 0, 12 x one joint moving, 4 x joints at their limits, 2 x v = -0.0"""
    rs = np.random.RandomState(11)
    rq = lambda: JNT_LO + (JNT_HI - JNT_LO)*rs.rand(6)
    q, v = [np.zeros(6)], [np.zeros(6)]
    for _ in range(4):
        q.append(rq()); v.append(np.zeros(6))
    for j in range(6):
        for sg in (-1.0, 1.0):
            vj = np.zeros(6); vj[j] = sg*rs.uniform(0.5, 4.0)
            q.append(rq()); v.append(vj)
    for pick in ([0]*6, [1]*6, [0, 1]*3, [1, 0]*3):
        q.append(np.where(np.array(pick) == 0, JNT_LO, JNT_HI)); v.append(rs.uniform(-4, 4, 6))
    for k in range(2):
        q.append(rq() if k else np.zeros(6)); v.append(np.full(6, -0.0))
    return np.array(q, np.float32), np.array(v, np.float32)


def _run(frame_skip, mode):
    """test_gpu_substep_loop._run with the special states written over the first envs between reset and the first step"""
    with one_wave_step_kernel(mode == "one_wave"):          # so100_step_fused instead of the 4-wave kernel
        sim = make_sim(1, N, flags=FREE, frame_skip=frame_skip, seed=4, envs_per_workgroup=32)
    assert sim.envs_per_workgroup == 32
    sim.set_policy(_policy(sim.obs_dim, sim.device))
    sim.reset()
    sq, sv = special_states()
    for i in range(6):
        for name, val in ((f"q{i}", sq[:, i]), (f"v{i}", sv[:, i])):
            row = sim.get_field(name)
            row[:len(val)] = torch.from_numpy(val).to(sim.device)
            sim.set_field(name, row)
    assert torch.signbit(sim.get_field("v0")[len(sq) - 1]).item()          # -0.0 arrives as -0.0
    buf = torch.zeros(T, N, sim.obs_dim + 10, device=sim.device)
    if mode == "persistent":
        sim.rollout(buf, 0)
    else:
        act = torch.zeros(N, 6, device=sim.device)
        for t in range(T):
            sim.policy_forward(sim.obs, act, t, rollout_row=buf[t])
            sim.step(act, rollout_row=buf[t])
    q, v = sim.get_state()
    torch.cuda.synchronize()
    return dict(buf=buf.clone(), obs=sim.obs.clone(), rew=sim.rew.clone(), done=sim.done.clone(), trunc=sim.trunc.clone(), q=q, v=v)


@pytest.mark.parametrize("frame_skip", [1, 16])
def test_rest_and_single_joint_states_against_stepwise_kernels(frame_skip):
    p1 = _run(frame_skip, "persistent")
    p2 = _run(frame_skip, "persistent")
    for k in KEYS:
        assert torch.equal(p1[k], p2[k]), f"two identical launches differ in {k}"
        assert torch.isfinite(p1[k].float()).all(), k
    od = p1["obs"].shape[1]
    for mode in ("stepwise", "one_wave"):
        s = _run(frame_skip, mode)
        for k in KEYS:
            assert torch.isfinite(s[k].float()).all(), (mode, k)
        worst = _close(p1, s, od)
        print(f"frame_skip {frame_skip} vs {mode}: worst difference / bound " + "  ".join(f"{k} {x:.3f}" for k, x in worst.items()))
        assert all(x <= 1.0 for x in worst.values()), (mode, worst)
        assert torch.equal(p1["done"], s["done"]) and torch.equal(p1["trunc"], s["trunc"]), mode
