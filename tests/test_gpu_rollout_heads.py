"""The policy heads of the 32-row contact-disabled rollout kernels on the matrix cores (csrc/so100_rollout.hpp: head_mfma), with no workgroup
barrier behind them.  Wave 0 runs the 6 x 64 mean head and wave 3 the value head as chains of 64 v_mfma_f32_4x4x1 over one accumulator, meant
to be, element by element, the k-ordered fmaf chain that the stand-alone policy kernel (so100_policy_forward_mfma) and the 64-row kernels run
on the VALU; meanwhile waves 1 and 2 already compute substep 0's state-only half.  What can go wrong: a wrong row / column / block mapping or
k order in the head, dead lanes leaking into live rows, and a race where the heads' barrier was.

Kinds 1, 2, 5 with the contact-disabled flags; (envs per workgroup, n) = (32, 33): a workgroup with one live env, (32, 96): full workgroups,
(16, 17): half of the 32-row tile live, (64, 65): the 64-row kernel, which keeps the VALU heads, as a control; frame_skip 1 and 16;
max_episode_steps = 2 and T = 3, so every episode ends inside the chunk and the pre-step after an auto-reset runs beside the heads.  Policies:
the random one of test_gpu_rollout_prestep.py, the saturating one of test_gpu_rollout_oracle.py (log_std -3 / +1), and one whose seven head
rows and biases all differ in magnitude, with signs alternating along k and a k-dependent size (no two terms of a chain are equal, so neither a
swapped row nor another summation order reproduces the result).

Same chain: at t = 0 the persistent kernel and policy_forward start from the same reset observation, and the raw-action, value and log-prob
columns of row 0 must be BIT-EQUAL between the two.  The parent commit (VALU heads in both kernels) passes this assertion in all 72 cases, so the
bound is zero.  Rows 1, 2 and the final state are held to test_persistent_rollout_equals_stepwise's bounds against the 4-wave and the one-wave
step kernel.  No race: two identical launches, and one T = 3 launch against three T = 1 launches, bit-equal in every output.  Dead lanes: the
rows of n = 33 are bit-equal to the first 33 envs' rows of n = 96 (slot = env in these variants and every random draw is keyed by the env's
index, so they are the same envs)."""
import functools

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from gpu_support import make_sim, one_wave_step_kernel, policy_tensors   # noqa: E402
from scenes import FREE                                                # noqa: E402
from test_gpu_rollout_oracle import _saturating_policy                 # noqa: E402
from test_gpu_rollout_prestep import KEYS, T, _close, _policy          # noqa: E402


def _ordered_heads_policy(obs_dim, device):
    """the random towers, under heads that are order-sensitive: row a of the mean head has magnitude ORDERED_MAG[a], the value row another, every
    bias its own; along k the sign alternates and the size runs through 64 different factors between 1 and 2 in a scrambled order.  Hidden
    activations are tanh values of random pre-activations, so the products lie between about 1e-10 and 0.12: normal fp32 numbers.  The outputs
    are of order 0.1 (the row bounds are absolute and presuppose outputs and gains of order one: see _saturating_heads_scaled)."""
    t = _policy(obs_dim, device)
    k = torch.arange(64, dtype=torch.float64)
    shape = (1.0 - 2.0*(k % 2))*(1.0 + ((37.0*k) % 64.0)/64.0)
    mag = torch.tensor(ORDERED_MAG, dtype=torch.float64)
    t["mu_w"] = (mag[:, None]*shape[None, :]*(1.0 + 0.01*torch.arange(6, dtype=torch.float64)[:, None]*k[None, :]/64.0)).float().to(device).contiguous()
    t["mu_b"] = torch.tensor([0.03, -0.0011, 0.07, 0.00023, -0.009, -0.0031]).to(device)
    t["v_w"] = (0.013*shape.flip(0))[None, :].float().to(device).contiguous()
    t["v_b"] = torch.tensor([0.41]).to(device)
    t["log_std"] = (mag.log() - 3.0).float().to(device)       # noise 5 % of a row's size: every bit of the mean shows in the raw action
    return t


def _saturating_heads_scaled(obs_dim, seed):
    """test_gpu_rollout_oracle.py's saturating policy (towers, biases, log_std -3 / +1) with the two head matrices scaled by HEAD_SCALE.
    Why: the row bounds below are absolute (1e-6) on rows whose observations already differ between the kernels by up to that much, so they
    presuppose a policy whose gain from observation to output is of order one, as the random policy's is.  With the head matrices at their
    original size (0.3 and 0.5 times a standard normal over towers with row scales up to 2) a last-bit difference of an observation moves a mean
    by more than that: the PARENT commit, VALU heads everywhere, misses the 1e-6 bound on rows 1, 2 by up to 2.4x in 5 of these 24 cases, the
    64-row control among them.  Saturation, the log_std pair and the bit-equality of row 0 are untouched by the scale."""
    t = _saturating_policy(obs_dim, seed)
    t["mu_w"] = (t["mu_w"]*HEAD_SCALE).contiguous(); t["v_w"] = (t["v_w"]*HEAD_SCALE).contiguous()
    return t


ORDERED_MAG = [0.02, 0.0007, 0.06, 0.00025, 0.007, 0.0021]     # a factor 2.8 apart at least; sums of 64 such terms stay of order 0.1
HEAD_SCALE = 0.05
POLICIES = {"random": lambda od, dev, kind, epw: _policy(od, dev),
            "saturating": lambda od, dev, kind, epw: _saturating_heads_scaled(od, 10*kind + epw),
            "ordered": lambda od, dev, kind, epw: _ordered_heads_policy(od, dev)}


@functools.lru_cache(maxsize=None)
def _run(kind, n, epw, frame_skip, policy, mode):
    """test_gpu_rollout_prestep.py's _run with the policy as an argument; results are shared between cases and never written to.
    mode: "persistent" (one so100_rollout launch of T steps), "again" (the same once more), "chunks" (T launches of one step), "stepwise"
    (policy_forward + step, 4-wave step kernel), "one_wave" (the same with so100_step_fused: gpu_support.one_wave_step_kernel)"""
    with one_wave_step_kernel(mode == "one_wave"):
        sim = make_sim(kind, n, flags=FREE, frame_skip=frame_skip, seed=4, max_episode_steps=2, envs_per_workgroup=epw)
    assert sim.envs_per_workgroup == epw
    sim.set_policy(POLICIES[policy](sim.obs_dim, sim.device, kind, epw))
    sim.reset()
    buf = torch.zeros(T, n, sim.obs_dim + 10, device=sim.device)
    if mode in ("persistent", "again"):
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
    return dict(buf=buf.clone(), obs=sim.obs.clone(), rew=sim.rew.clone(), done=sim.done.clone(), trunc=sim.trunc.clone(), q=q.clone(), v=v.clone())


@pytest.mark.parametrize("policy", ["random", "saturating", "ordered"])
@pytest.mark.parametrize("frame_skip", [1, 16])
@pytest.mark.parametrize("epw,n", [(32, 33), (32, 96), (16, 17), (64, 65)])
@pytest.mark.parametrize("kind", [1, 2, 5])
def test_rollout_heads_against_policy_kernel(kind, epw, n, frame_skip, policy):
    p1 = _run(kind, n, epw, frame_skip, policy, "persistent")
    od = p1["obs"].shape[1]
    assert torch.isfinite(p1["buf"]).all()
    assert p1["buf"][..., od + 7].sum() > 0                  # the 2-step TimeLimit ends every episode inside the chunk (auto-reset runs)
    # ---- no race where the barrier was
    p2 = _run(kind, n, epw, frame_skip, policy, "again")
    for k in KEYS:
        assert torch.equal(p1[k], p2[k]), f"two identical launches differ in {k}"
    c = _run(kind, n, epw, frame_skip, policy, "chunks")
    for k in KEYS:
        assert torch.equal(p1[k], c[k]), f"one launch of {T} steps and {T} launches of one step differ in {k}"
    # ---- dead lanes do not leak: the one-live-env workgroup of n = 33 against the same envs in full workgroups
    if (epw, n) == (32, 33):
        full = _run(kind, 96, 32, frame_skip, policy, "persistent")
        assert torch.equal(p1["buf"], full["buf"][:, :n]), "rows of n = 33 differ from the first 33 envs' rows of n = 96"
        assert torch.equal(p1["q"], full["q"][..., :n]) and torch.equal(p1["v"], full["v"][..., :n])
    # ---- same chain: row 0's raw action, value and log-prob against the stand-alone policy kernel's VALU heads, bit for bit
    for mode in ("stepwise", "one_wave"):
        s = _run(kind, n, epw, frame_skip, policy, mode)
        assert torch.equal(p1["buf"][0, :, :od], s["buf"][0, :, :od]), "the two do not start from the same reset observation"
        head = {"raw action": slice(od, od + 6), "value": slice(od + 8, od + 9), "log-prob": slice(od + 9, od + 10)}
        diff = {nm: (p1["buf"][0, :, c] - s["buf"][0, :, c]).abs().max().item() for nm, c in head.items()}
        print(f"kind {kind} n {n} epw {epw} frame_skip {frame_skip} {policy} vs {mode}: row 0 |difference| " + "  ".join(f"{k} {x:.3g}" for k, x in diff.items()))
        for nm, c in head.items():
            assert torch.equal(p1["buf"][0, :, c], s["buf"][0, :, c]), f"row 0 {nm}: persistent kernel and policy_forward differ by {diff[nm]:.3g} ({mode})"
        # ---- rows 1, 2 and the final state: test_persistent_rollout_equals_stepwise's bounds
        worst = _close(p1, s, od)
        print(f"kind {kind} n {n} epw {epw} frame_skip {frame_skip} {policy} vs {mode}: worst difference / bound " + "  ".join(f"{k} {x:.3f}" for k, x in worst.items()))
        assert all(x <= 1.0 for x in worst.values()), (mode, worst)
        assert torch.equal(p1["done"], s["done"]) and torch.equal(p1["trunc"], s["trunc"]), mode
