"""GPU parity of the finger-pad contacts (pad/floor: part of the reference physics; pad/cube: BASELINE.json configs[4]) against
the fp64 oracle, through the C ABI.  Physics states are INJECTED (so100_set_state): arm poses with the pads at the floor, a
cube between the closing jaws.  Comparisons run over one env step (16 substeps) -- across contact make / break events fp32 and
fp64 trajectories separate (tests/test_hostcheck_contacts.py), so envs in which the oracle's contact set changes during the
step are held to a looser bound than the ones with a steady set.  "parity unpinned (physics)": the oracle restates MuJoCo's
algorithm, MuJoCo itself is not available."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from gpu_support import inject_state, make_sim, oracle_step   # noqa: E402
from oracle import so100_oracle as O                      # noqa: E402  (the checker)
from scenes import C5, JS, L, M, NOPADS, REFP, SHIPPED, floor_batch, fresh, grasp_batch, idle_batch   # noqa: E402

STEADY_MIN = 18          # envs (of 96) whose contact set is steady over the 16 substeps of the injected step (measured: 24; the test prints the classes)


def _stale_envs(res, iters):
    """envs whose residual row exceeds 1e-2.  At 2 block-PGS sweeps that row is the max over the step's substeps of the Newton's residual
    (contact substeps) and of the last sweep's change (contact-free substeps: not the distance from the converged solve,
    tests/substep_harness.py check_residual); it is bounded per substep there.  Here those envs are counted and held to the same
    state bounds as every other env.  (4, 30): none allowed."""
    k = int((res >= 1e-2).sum())
    if iters != SHIPPED:
        assert k == 0
    return k


@pytest.mark.parametrize("n", [96, 8192, 16384, 16384 + 96])
def test_pad_floor_step_vs_oracle(n):
    _pad_floor_step_vs_oracle(n, (4, 30))


@pytest.mark.parametrize("n", [96, 8192, 16384, 16384 + 96])
def test_pad_floor_step_vs_oracle_at_shipped_settings(n):
    """test_pad_floor_step_vs_oracle at the shipped solver settings (solver_iters, contact_iters) = SHIPPED = (2, 20), with the same bounds"""
    _pad_floor_step_vs_oracle(n, SHIPPED)


def _pad_floor_step_vs_oracle(n, iters):
    """one env step from injected poses with the pads at the floor; n = 96 runs the 4-wave latency kernel with 16 envs per
    workgroup (contact wave: 4 cooperating lanes per env), 8192 with 32 (2 lanes per env), 16384 with 64 (one lane per env),
    n > 16384 the one-wave throughput kernel (the first 96 envs are the injected ones)"""
    m = 96
    qpos, qvel, act = floor_batch(m, 0)
    sim = make_sim(1, n, flags=REFP, solver_iters=iters[0], contact_iters=iters[1], max_episode_steps=0, seed=3)
    QP, QV = idle_batch(n)
    QP[:m] = qpos; QV[:m] = qvel
    A = np.zeros((n, 6), np.float32); A[:m] = act
    sim.reset(); inject_state(sim, QP, QV)
    sim.step(torch.from_numpy(A).cuda())
    gq, gv = sim.get_state(); gq = gq.cpu().numpy().T[:m]; gv = gv.cpu().numpy().T[:m]
    cstat = sim.get_field("contact_stat", dtype=torch.int32).cpu().numpy()[:m]
    res = sim.get_field("solver_residual").cpu().numpy()[:m]
    steady = 0; touched = 0; worst_steady = 0.0; worst_any = 0.0
    for i in range(m):
        oq, ov, counts = oracle_step(qpos[i], qvel[i], act[i], REFP)
        nmax = max(c[0] for c in counts)
        touched += nmax > 0
        eq = np.abs(gq[i, :6] - oq[:6]).max(); ev = np.abs(gv[i, :6] - ov[:6]).max()
        if len(set(counts)) == 1:                            # the same contact set in all 16 substeps
            steady += 1
            assert (cstat[i] & 255) == nmax
            worst_steady = max(worst_steady, eq, ev*1e-2)
        worst_any = max(worst_any, eq, ev*1e-2)
    stale = _stale_envs(res, iters)
    print(f"[pad/floor 16-substep step, n={n}, iters {iters}] envs {m}: touched {touched}, steady contact set over the 16 substeps {steady} (worst {worst_steady:.2e}), "
          f"make / break inside the step {m - steady} (worst over all {worst_any:.2e}); max residual {res.max():.1e}, envs with a residual >= 1e-2: {stale}")
    assert np.isfinite(gq).all() and np.isfinite(gv).all() and touched > 0.8*m and steady >= STEADY_MIN
    assert (cstat >> 8).max() == 0 and (stale > 0 or res.max() < 1e-2)     # nothing over the contact budget; the Newton solves converged
    assert worst_steady < 5e-6                               # steady contact set: angles 5e-6 rad, velocities 5e-4 rad/s
    # EVERY env, also the 72 of 96 in which a corner makes / breaks contact inside the step: measured 3.6e-7 on all four kernels -- since round 3's
    # solver rework fp32 and fp64 see these events in the same substep for this batch.  (2e-2 was round 2's bound for an event a substep apart;
    # 2e-5 = the north star's 1e-5 relative at |q| ~ 2 rad keeps the test unconditional without demanding what the physics cannot promise.)
    assert worst_any < 2e-5


def test_pads_keep_the_gripper_above_the_floor_at_full_size():
    """4096 envs (BASELINE per-GPU batch), reference physics, every arm servoed downwards into the floor for 40 env steps:
    with the pad/floor contacts no pad corner ends deeper than 1 mm (the impact itself dips < 3 mm), without them they sink
    centimetres; determinism and shard invariance of the contact path on the way."""
    n = 4096
    rs = np.random.RandomState(5)
    QP = np.zeros((n, 13)); QP[:, 9] = 1.0; QP[:, 6:9] = [0.2, -0.3, 0.0099]
    QP[:, :6] = np.array([0.0, -1.6, 1.9, 1.5, 0.0, 0.3]) + rs.uniform(-1, 1, (n, 6))*np.array([0.5, 0.05, 0.05, 0.2, 0.5, 0.2])
    QV = np.zeros((n, 12))
    act = np.zeros((n, 6), np.float32); act[:, 1] = 1.0     # shoulder down, 0.075 rad per step ahead of the measured angle

    def lowest_pad(qp):
        out = np.zeros(len(qp))
        for i in range(0, len(qp), 16):                     # a sample: every 16th env
            d = fresh(qp[i, :6]); L.so100o_kinematics(C.byref(M), C.byref(d))
            xp = O.arr(d.xpos); xm = O.arr(d.xmat); z = []
            for g in range(8):
                b = M.pad_body[g]; R = xm[b].reshape(3, 3)
                z.append((xp[b] + R @ np.array(M.pad_pos[g][:]))[2] - (np.abs(R[2])*np.array(M.pad_size[g][:])).sum())
            out[i] = min(z)
        return out[::16]

    def run(flags, n_envs, off, sl):
        sim = make_sim(1, n_envs, flags=flags, seed=9, env_id_offset=off, max_episode_steps=0)
        sim.reset(); inject_state(sim, QP[sl], QV[sl]); a = torch.from_numpy(act[sl]).cuda(); low = 1.0
        for t in range(40):
            sim.step(a)
            if t % 4 == 3:
                low = min(low, lowest_pad(sim.get_state()[0].cpu().numpy().T).min())
        q, v = sim.get_state()
        return q.clone(), v.clone(), low, lowest_pad(q.cpu().numpy().T), sim.get_field("contact_stat", dtype=torch.int32).clone()
    q, v, low, final, cs = run(REFP, n, 0, slice(0, n))
    q2, v2, _, _, cs2 = run(REFP, n, 0, slice(0, n))
    assert torch.equal(q, q2) and torch.equal(v, v2) and torch.equal(cs, cs2)               # bitwise deterministic
    qa, va, _, _, _ = run(REFP, n//2, 0, slice(0, n//2)); qb, vb, _, _, _ = run(REFP, n//2, n//2, slice(n//2, n))
    assert torch.equal(torch.cat([qa, qb], 1), q) and torch.equal(torch.cat([va, vb], 1), v)   # sharding leaves every env unchanged
    assert torch.isfinite(q).all() and torch.isfinite(v).all()
    assert low > -0.003 and final.min() > -0.001 and (cs & 255).max() >= 2 and (cs >> 8).max() == 0
    _, _, low0, final0, _ = run(NOPADS, n, 0, slice(0, n))
    assert final0.min() < -0.02                               # without the pad contacts the gripper is centimetres under the floor


@pytest.mark.parametrize("n", [64, 8192, 16384 + 64])
def test_pad_cube_grasp_vs_oracle(n):
    _pad_cube_grasp_vs_oracle(n, (4, 30))


@pytest.mark.parametrize("n", [64, 8192, 16384 + 64])
def test_pad_cube_grasp_vs_oracle_at_shipped_settings(n):
    """test_pad_cube_grasp_vs_oracle at the shipped solver settings (solver_iters, contact_iters) = SHIPPED = (2, 20), with the same bounds"""
    _pad_cube_grasp_vs_oracle(n, SHIPPED)


def _pad_cube_grasp_vs_oracle(n, iters):
    """BASELINE.json configs[4]: the jaw closes on a cube floating between the pads; arm and cube dofs are coupled in one
    12-unknown solve.  Step by step against the oracle for as long as both see the same pad/cube contact counts."""
    m = 64
    qpos, qvel, act = grasp_batch(m, 1)
    sim = make_sim(1, n, flags=C5, solver_iters=iters[0], contact_iters=iters[1], max_episode_steps=0, seed=3)
    QP, QV = idle_batch(n)
    QP[:m] = qpos; QV[:m] = qvel
    A = np.zeros((n, 6), np.float32); A[:m] = act
    sim.reset(); inject_state(sim, QP, QV)
    ds = []
    for i in range(m):
        d = fresh(); O.arr(d.qpos)[:] = qpos[i].astype(np.float32).astype(np.float64); ds.append(d)
    alive = np.ones(m, bool); compared = 0; coupled_steps = 0; worst = 0.0
    at = torch.from_numpy(A).cuda()
    for t in range(6):
        sim.step(at)
        gq, gv = sim.get_state(); gq = gq.cpu().numpy().T[:m]; gv = gv.cpu().numpy().T[:m]
        cstat = sim.get_field("contact_stat", dtype=torch.int32).cpu().numpy()[:m]
        assert np.isfinite(gq).all() and np.isfinite(gv).all() and (cstat >> 8).max() == 0
        for i in range(m):
            d = ds[i]
            O.arr(d.ctrl)[:] = O.arr(d.qpos)[:6] + (act[i]*JS).astype(np.float64)
            nmax = 0; ncub = 0
            for s in range(16):
                L.so100o_step(C.byref(M), C.byref(d), C5, -1, 1)
                nmax = max(nmax, d.ncon); ncub = max(ncub, sum(1 for k in range(d.ncon) if d.con[k].kind == 2))
            if not alive[i]:
                continue
            if (cstat[i] & 255) != nmax:                     # contact sets differ somewhere in this step: the runs have separated
                alive[i] = False; continue
            eq = max(np.abs(gq[i, :6] - O.arr(d.qpos)[:6]).max(), np.abs(gq[i, 6:9] - O.arr(d.qpos)[6:9]).max())
            ev = max(np.abs(gv[i, :6] - O.arr(d.qvel)[:6]).max(), np.abs(gv[i, 6:9] - O.arr(d.qvel)[6:9]).max())
            worst = max(worst, eq, ev*1e-2); compared += 1; coupled_steps += ncub > 0
    print(f"[grasp 16-substep steps, n={n}, iters {iters}] env-steps compared {compared} of {6*m} (an env leaves when its contact count differs from the oracle's), "
          f"coupled {coupled_steps}, envs still compared after 6 steps {int(alive.sum())}; worst {worst:.2e}")
    assert compared >= 6*m - 6 and coupled_steps > m//2      # (measured: all 384 env-steps compared -- no env's contact count ever differed from the oracle's)
    assert worst < 2e-5                                      # measured 3.4e-6: 2e-5 rad / m, 2e-3 per second through the impact of the closing jaw on an 8 g cube
    # physics, not parity: after 6 steps (0.19 s; free fall would be 18 cm) the same share of cubes is still between the pads
    # as in the oracle (Env01's ctrl = measured angle - 0.075 is a weak grip: tilted cubes slide out on both sides alike)
    held = (gq[:, 8] > qpos[:, 8] - 0.03).mean()
    held_o = np.mean([O.arr(d.qpos)[8] > qpos[i, 8] - 0.03 for i, d in enumerate(ds)])
    assert held > 0.3 and abs(held - held_o) < 0.1


@pytest.mark.parametrize("flags", [REFP, C5])
def test_contact_kernels_agree_with_each_other(flags):
    """the three kernels that can run a pad-contact step -- 4-wave latency kernel, one-wave throughput kernel, persistent rollout
    kernel (detection on the otherwise idle wave 3, contact records in LDS under the policy's activation images) -- produce the
    same physics from the same injected contact states."""
    from so100_mujoco_rl_amd.vec_env import So100VecEnv
    from so100_mujoco_rl_amd.collector import RolloutCollector
    m = 128
    if flags == C5:
        qpos, qvel, act = grasp_batch(m, 2)
    else:
        qpos, qvel, act = floor_batch(m, 2)
        act[:] = act[0]; act[:, 1] = 0.6                     # ONE action for the whole batch (shoulder down), so that the persistent kernel's
    outs = {}                                                # bias-only policy below can reproduce it: its rollout leg runs for both flag sets
    for name, n in (("mw", m), ("fused", 16384 + m)):
        sim = make_sim(1, n, flags=flags, contact_iters=12, max_episode_steps=0, seed=3)
        QP, QV = idle_batch(n)
        QP[:m] = qpos; QV[:m] = qvel; A = np.zeros((n, 6), np.float32); A[:m] = act
        sim.reset(); inject_state(sim, QP, QV)
        for t in range(3):
            sim.step(torch.from_numpy(A).cuda())
        q, v = sim.get_state()
        outs[name] = (q[:, :m].clone(), v[:, :m].clone(), sim.get_field("contact_stat", dtype=torch.int32)[:m].clone())
    # persistent kernel: a policy whose mean is the wanted action (zero weights, bias = action is not per-env; use zero noise + bias)
    env = So100VecEnv(1, m, flags=flags, contact_iters=12, max_episode_steps=0, seed=3)
    sd = RolloutCollector.random_policy_state(15, env.device, seed=1)
    sd["action_net.weight"].zero_(); sd["action_net.bias"].copy_(torch.from_numpy(act[0])); sd["log_std"].fill_(-30.0)
    col = RolloutCollector(env, sd, T=3, persistent=True, bootstrap_truncated=False)
    env.sim.reset(); inject_state(env.sim, qpos, qvel); col._started = True
    assert np.abs(act - act[0]).max() == 0                   # one action for all envs -> the rollout kernel is compared too
    col.collect(3)
    q, v = env.sim.get_state()
    outs["rollout"] = (q.clone(), v.clone(), env.sim.get_field("contact_stat", dtype=torch.int32).clone())
    assert set(outs) == {"mw", "fused", "rollout"}
    ref = outs["mw"]
    assert (ref[2] & 255).max() >= 2
    for name, o in outs.items():
        if name == "mw":
            continue
        same = (o[2] & 255) == (ref[2] & 255)
        print(f"[kernels agree, flags {flags}] {name} vs mw: same contact count in {float(same.float().mean()):.3f} of {m} envs")
        assert same.float().mean() > 0.9, name
        dq = (o[0] - ref[0]).abs().amax(0); dv = (o[1] - ref[1]).abs().amax(0)
        # the kernels differ in their Newton warm starts (the contact wave of the multi-wave kernels starts a lane's first contact
        # substep cold, the one-wave kernel carries the previous acceleration) and tiny steps are taken unverified, so they agree
        # to the solver tolerance per substep, and to the make / break bound of the module docstring over three env steps
        assert dq[same].max() < 2e-4 and dv[same].max() < 1e-1, (name, float(dq[same].max()), float(dv[same].max()))
        assert dq[same].median() < 5e-6 and dv[same].median() < 5e-4, (name, float(dq[same].median()), float(dv[same].median()))


@pytest.mark.parametrize("flags", [REFP, C5])
@pytest.mark.parametrize("epw", [16, 32, 64])
def test_tail_workgroups_with_pad_contacts(epw, flags):
    """batch sizes that are not a multiple of the envs-per-workgroup count: env by env the results must be BIT-IDENTICAL to the same envs
    inside a 256-env batch -- the contact wave's lane groups that belong to no env must not matter.  At 16 envs per workgroup (what the
    library chooses by itself at these sizes: 4 lanes of the contact wave per env), and pinned to 32 and 64 (2 lanes, 1 lane), which it
    chooses above 4096 and 8192 envs"""
    if epw == 16:
        auto = make_sim(1, 256, flags=flags, seed=5, max_episode_steps=25)
        assert auto.envs_per_workgroup == 16
        auto.close()
    for n in (1, epw + 1, 130):
        big = make_sim(1, 256, flags=flags, seed=5, max_episode_steps=25, envs_per_workgroup=epw)
        small = make_sim(1, n, flags=flags, seed=5, max_episode_steps=25, envs_per_workgroup=epw)
        assert big.envs_per_workgroup == epw and small.envs_per_workgroup == epw
        assert torch.equal(big.reset()[:n], small.reset())
        g = torch.Generator(device="cuda"); g.manual_seed(3); touched = 0
        for t in range(40):
            a = torch.rand(256, 6, device="cuda", generator=g)*2 - 1; a[:, 1] = 1.0      # shoulder down: the pads reach the floor within a few steps
            o1, r1, d1, _ = big.step(a); o2, r2, d2, _ = small.step(a[:n].contiguous())
            assert torch.equal(o1[:n], o2) and torch.equal(r1[:n], r2) and torch.equal(d1[:n], d2), (n, t)
            cs1 = big.get_field("contact_stat", dtype=torch.int32); cs2 = small.get_field("contact_stat", dtype=torch.int32)
            assert torch.equal(cs1[:n], cs2), (n, t)
            touched = max(touched, int((cs2 & 255).max()))
        q1, v1 = big.get_state(); q2, v2 = small.get_state()
        assert torch.equal(q1[:, :n], q2) and torch.equal(v1[:, :n], v2) and touched >= 2
        big.close(); small.close()


@pytest.mark.parametrize("kind,flags", [(1, REFP), (2, C5), (6, REFP)])
def test_whole_env_steps_with_pad_contacts_vs_oracle(kind, flags):
    _whole_env_steps_with_pad_contacts_vs_oracle(kind, flags, (4, 30))


@pytest.mark.parametrize("kind,flags", [(1, REFP), (2, C5), (6, REFP)])
def test_whole_env_steps_with_pad_contacts_vs_oracle_at_shipped_settings(kind, flags):
    """test_whole_env_steps_with_pad_contacts_vs_oracle at the shipped solver settings (solver_iters, contact_iters) = SHIPPED = (2, 20), with the same bounds"""
    _whole_env_steps_with_pad_contacts_vs_oracle(kind, flags, SHIPPED)


def _whole_env_steps_with_pad_contacts_vs_oracle(kind, flags, iters):
    """the full path -- task layer + physics with pad contacts -- of Env01 / Env02 / Env06 against the oracle's env step (its
    Newton solver) from reset, arms driven down until the pads are on the floor.  An env counts until a contact event lands a
    substep apart in fp32 and fp64 (its observation then jumps by > 1e-3); most envs never do within the run."""
    n, steps = 48, (40 if kind == 1 else 16)                  # (Env01 starts higher above the table)
    rs = np.random.RandomState(kind)
    sim = make_sim(kind, n, flags=flags, solver_iters=iters[0], contact_iters=iters[1], max_episode_steps=0, seed=11)
    orc = [O.OracleEnv(kind, flags=flags, iters=-1, seed=11, env_id=i) for i in range(n)]
    for e in orc:
        e.e.max_episode_steps = 0
    inj = rs.random_sample((n, 16)).astype(np.float32)
    og = sim.reset(inject=torch.from_numpy(inj).cuda()).cpu().numpy()
    oo = np.stack([e.reset(inject=inj[i]) for i, e in enumerate(orc)])
    np.testing.assert_allclose(og, oo, rtol=0, atol=1e-6)
    alive = np.ones(n, bool); worst = np.zeros(n); touched = np.zeros(n, bool)
    for t in range(steps):
        a = rs.uniform(-1, 1, (n, 6)).astype(np.float32); a[:, 1] = 1.0                 # shoulder down
        inj = rs.random_sample((n, 16)).astype(np.float32)
        ob, rw, dn, _ = sim.step(torch.from_numpy(a).cuda(), inject=torch.from_numpy(inj).cuda())
        ob = ob.cpu().numpy(); rw = rw.cpu().numpy()
        assert np.isfinite(ob).all() and np.isfinite(rw).all()
        touched |= (sim.get_field("contact_stat", dtype=torch.int32).cpu().numpy() & 255) > 0
        for i, e in enumerate(orc):
            if not alive[i]:
                continue
            o, r = e.step(a[i], inject=inj[i], autoreset=True)[:2]
            err = max(np.abs(ob[i] - o).max(), abs(rw[i] - r))
            if err > 1e-3:
                alive[i] = False
            else:
                worst[i] = max(worst[i], err)
    print(f"[whole env steps, kind {kind} flags {flags} iters {iters}] envs {n}: touched {int(touched.sum())}, never separated from the oracle by a contact event {int(alive.sum())}, "
          f"median / p90 error of those {np.median(worst[alive]):.2e} / {np.percentile(worst[alive], 90):.2e}")
    assert touched.mean() > (0.1 if kind == 1 else 0.5)      # the pads did reach the floor (Env01 starts high: fewer of its arms get there)
    assert alive.mean() >= 0.9                               # (measured: 45-48 of 48 never saw a contact event a substep apart)
    assert np.median(worst[alive]) < 1e-5 and np.percentile(worst[alive], 90) < 3e-5
