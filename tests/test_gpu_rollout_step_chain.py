"""Launch-invariant and state-only work off wave 0's chain in the 32-row contact-disabled rollout kernels (csrc/so100_rollout.hpp, DESIGN.md
section 8j): std = exp(log_std) is taken once per launch where the head weights go to LDS and the sampling stretch is straight-line code with one
`live` region round its stores; wave 0 computes the servo force in front of the mid-substep barrier and subtracts the bias behind it.  What can
go wrong: a std that is not the per-step exponential's bits (or a stale one, kept from an earlier launch), dead lanes leaking into live rows
now that every lane computes, a servo force rounded differently from arm_tau's or taken from the wrong substep's q, v (frame_skip 1 and 2
are the edges: no loop iteration at all / exactly one), and stale poses or a stale start state round an auto-reset.

Kinds 1, 2, 5; (envs per workgroup, n) = (32, 33): a workgroup with one live env, (32, 96): full workgroups, (16, 17): half of the 32-row
tile live, (64, 65): the 64-row kernel, which keeps the text it had, as a control; frame_skip 1, 2, 16; max_episode_steps = 2 and T = 3, so
every episode ends inside the chunk.  The policy is test_gpu_rollout_prestep.py's random one under three log_std rows: zeros; -3 / +1
alternating; and one with -104 and +89, where expf takes its underflow (std = 0: the raw action is the mean) and overflow (std = inf: the
raw action is +-inf, the action the env sees +-1) selects.

Row 0's raw action and log-prob are BIT-EQUAL to policy_forward's (the stand-alone policy kernel takes the exponential per call); rows 1, 2,
the terminal observations (the stale-pose observation of the step that ended an episode; row 1's reward is that step's, row 2's observation the
one after the reset) and the final state are held to test_persistent_rollout_equals_stepwise's bounds against the 4-wave and the one-wave step
kernel; one launch of three steps is bit-equal to three launches of one; a launch behind a set_policy that changes log_std only samples with the
new std.  Differences are taken where the two values are not equal, so +-inf in both is no difference and inf against anything else is.

The parent commit passes this file unchanged (all 114 cases: it computes the same bits the slow way)."""
import functools

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from gpu_support import make_sim, one_wave_step_kernel          # noqa: E402
from scenes import FREE                                         # noqa: E402
from test_gpu_rollout_prestep import KEYS, T, _policy           # noqa: E402

LOG_STD = {"zero": [0.0, 0.0, 0.0, 0.0, 0.0, 0.0],
           "mixed": [-3.0, 1.0, -3.0, 1.0, -3.0, 1.0],
           "extreme": [-104.0, 0.0, 89.0, -3.0, 1.0, -0.5]}      # expf: -104 underflows to 0 (below 2^-150), +89 overflows to inf (above FLT_MAX)
KEYS_T = KEYS + ("tobs",)


def _policy_with(obs_dim, device, log_std):
    t = _policy(obs_dim, device)
    t["log_std"] = torch.tensor(LOG_STD[log_std], dtype=torch.float32, device=device)
    return t


@functools.lru_cache(maxsize=None)
def _run(kind, n, epw, frame_skip, log_std, mode):
    """test_gpu_rollout_prestep.py's _run with the log_std row as an argument and the terminal observations beside the rows; results are shared
    between cases and never written to.  mode: "persistent" (one so100_rollout launch of T steps), "chunks" (T launches of one step),
    "stepwise" (policy_forward + step, 4-wave step kernel), "one_wave" (the same with so100_step_fused)"""
    with one_wave_step_kernel(mode == "one_wave"):
        sim = make_sim(kind, n, flags=FREE, frame_skip=frame_skip, seed=4, max_episode_steps=2, envs_per_workgroup=epw)
    assert sim.envs_per_workgroup == epw
    sim.set_policy(_policy_with(sim.obs_dim, sim.device, log_std))
    sim.reset()
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


def _diff(a, b):
    """|a - b| where a != b, 0 where they are equal (inf against the same inf); NaN anywhere fails every bound"""
    return torch.where(a == b, torch.zeros_like(a), (a - b).abs())


def _close(a, b, od):
    """test_persistent_rollout_equals_stepwise's bounds: 1e-6 on everything but the rewards (2e-5), joint velocities 1e-5; the terminal
    observations are observations (1e-6)"""
    cols = torch.full((od + 10,), 1e-6, device=a["buf"].device); cols[od + 6] = 2e-5
    return {"buf": (_diff(a["buf"], b["buf"]) / cols).max().item(), "tobs": _diff(a["tobs"], b["tobs"]).max().item() / 1e-6,
            "obs": _diff(a["obs"], b["obs"]).max().item() / 1e-6, "rew": _diff(a["rew"], b["rew"]).max().item() / 2e-5,
            "q": _diff(a["q"], b["q"]).max().item() / 1e-6, "v": _diff(a["v"], b["v"]).max().item() / 1e-5}


@pytest.mark.parametrize("log_std", ["zero", "mixed", "extreme"])
@pytest.mark.parametrize("frame_skip", [1, 2, 16])
@pytest.mark.parametrize("epw,n", [(32, 33), (32, 96), (16, 17), (64, 65)])
@pytest.mark.parametrize("kind", [1, 2, 5])
def test_step_chain_against_policy_and_step_kernels(kind, epw, n, frame_skip, log_std):
    p1 = _run(kind, n, epw, frame_skip, log_std, "persistent")
    od = p1["obs"].shape[1]
    raw, logp = slice(od, od + 6), slice(od + 9, od + 10)
    assert not torch.isnan(p1["buf"]).any() and not torch.isnan(p1["tobs"]).any()
    finite = torch.isfinite(p1["buf"])
    if log_std == "extreme":                                  # std = inf shows in that action's raw column and nowhere else; std = 0 leaves the mean
        assert not finite[..., od + 2].any() and finite[..., :od + 2].all() and finite[..., od + 3:].all()
    else:
        assert finite.all()
    # ---- every episode ends at its second step: row 1 carries the done code, its terminal observation is written, row 2 starts from the reset
    assert (p1["buf"][1, :, od + 7] > 0).all() and (p1["buf"][0, :, od + 7] == 0).all() and (p1["buf"][2, :, od + 7] == 0).all()
    assert (p1["tobs"][1].abs().sum(1) > 0).all() and (p1["tobs"][0] == 0).all() and (p1["tobs"][2] == 0).all()
    # ---- one launch of three steps against three launches of one (std per launch, prologue path against in-loop path)
    c = _run(kind, n, epw, frame_skip, log_std, "chunks")
    for k in KEYS_T:
        assert torch.equal(p1[k], c[k]), f"one launch of {T} steps and {T} launches of one step differ in {k}"
    # ---- dead lanes compute but do not leak: the one-live-env workgroup of n = 33 against the same envs in full workgroups
    if (epw, n) == (32, 33):
        full = _run(kind, 96, 32, frame_skip, log_std, "persistent")
        assert torch.equal(p1["buf"], full["buf"][:, :n]), "rows of n = 33 differ from the first 33 envs' rows of n = 96"
        assert torch.equal(p1["q"], full["q"][..., :n]) and torch.equal(p1["v"], full["v"][..., :n])
    for mode in ("stepwise", "one_wave"):
        s = _run(kind, n, epw, frame_skip, log_std, mode)
        # ---- row 0: same observation, same noise; std = exp(log_std) per launch against the policy kernel's per call, bit for bit
        assert torch.equal(p1["buf"][0, :, :od], s["buf"][0, :, :od]), "the two do not start from the same reset observation"
        for nm, col in (("raw action", raw), ("log-prob", logp)):
            d = _diff(p1["buf"][0, :, col], s["buf"][0, :, col]).max().item()
            print(f"kind {kind} n {n} epw {epw} frame_skip {frame_skip} {log_std} vs {mode}: row 0 {nm} |difference| {d:.3g}")
            assert torch.equal(p1["buf"][0, :, col], s["buf"][0, :, col]), f"row 0 {nm}: persistent kernel and policy_forward differ by {d:.3g} ({mode})"
        # ---- rows 1, 2, the terminal observations and the final state
        worst = _close(p1, s, od)
        print(f"kind {kind} n {n} epw {epw} frame_skip {frame_skip} {log_std} vs {mode}: worst difference / bound " + "  ".join(f"{k} {x:.3f}" for k, x in worst.items()))
        assert all(x <= 1.0 for x in worst.values()), (mode, worst)
        assert torch.equal(p1["done"], s["done"]) and torch.equal(p1["trunc"], s["trunc"]), mode


@pytest.mark.parametrize("epw,n", [(32, 33), (64, 65)])
@pytest.mark.parametrize("kind", [1, 2, 5])
def test_std_is_taken_per_launch(kind, epw, n, frame_skip=2):
    """Two launches with set_policy between them, log_std changed only: the second launch samples with the new std.  Its row 0 against
    policy_forward on the observation the first launch left, with the new and with the old policy."""
    sim = make_sim(kind, n, flags=FREE, frame_skip=frame_skip, seed=4, max_episode_steps=2, envs_per_workgroup=epw)
    od = sim.obs_dim
    old, new = _policy_with(od, sim.device, "zero"), _policy_with(od, sim.device, "mixed")
    sim.set_policy(old)
    sim.reset()
    buf = torch.zeros(T + 1, n, od + 10, device=sim.device)
    sim.rollout(buf[:T], 0)
    obs = sim.obs.clone()
    act = torch.zeros(n, 6, device=sim.device)
    ref = {}
    for name, pol in (("old", old), ("new", new)):             # the stand-alone policy kernel: it changes nothing in the env
        ref[name] = torch.zeros(n, od + 10, device=sim.device)
        sim.set_policy(pol)
        sim.policy_forward(obs, act, T, rollout_row=ref[name])
    sim.rollout(buf[T:], T)                                    # the policy is the new one
    torch.cuda.synchronize()
    row = buf[T]
    assert torch.equal(row[:, :od], obs) and torch.isfinite(row).all()
    raw, logp = slice(od, od + 6), slice(od + 9, od + 10)
    for nm, col in (("raw action", raw), ("log-prob", logp)):
        assert torch.equal(row[:, col], ref["new"][:, col]), f"{nm} of the launch behind set_policy is not the new policy's"
        assert (row[:, col] != ref["old"][:, col]).any(1).all(), f"{nm}: the old and the new log_std cannot be told apart"
    assert torch.equal(row[:, od + 8], ref["new"][:, od + 8]) and torch.equal(row[:, od + 8], ref["old"][:, od + 8])      # the value head did not change
