#!/usr/bin/env python3
"""A gradient-based planner (receding-horizon iLQR) for Env01 built on the derivatives query (needs a GPU): every step each env rolls its
current plan of `horizon` actions out with So100Sim.trajectory, So100Sim.derivatives linearises all N x horizon (state, action) pairs of
that rollout in one launch (the arm block of the tangent state: rows and columns 0..5 and 12..17 of A, rows of B), the cost |ee - cube|^2
summed over the horizon gets its Gauss-Newton terms from So100Sim.jacobian, a batched Riccati pass in torch on the device improves the
plan, and its first action is executed through step().  Printed next to the zero-action baseline, like examples/mppi_reach.py.
--backward query replaces the torch Riccati and forward loops by ONE So100Sim.lqr call (nx = 12: the arm block, read out of the unsliced A, B).
--forward closed replaces the LINEAR forward pass (the plan is u + du of the linear model, never checked against the physics) by the nonlinear
one with a line search: So100Sim.lqr gives k and K (whatever --backward says), ONE So100Sim.closed_loop call rolls the feedback law out on the
real dynamics at eight step sizes alpha = 0, 1, 1/2, .. 1/64, the true cost of every candidate is summed in torch, and each env takes the controls
of its cheapest candidate as the new plan.  alpha = 0 is the old plan, so the chosen plan's true cost never exceeds the old one's.
--cost query takes the cost's quadratic model (lx, lxx, lu, luu) from ONE So100Sim.cost_terms call in place of the Jacobian query and the torch
arithmetic behind it (cube target, nx = 12: So100Sim.lqr is then the backward pass, whatever --backward says), and with --forward closed the line
search's sum, mask, argmin and gather from ONE So100Sim.cost_select call with the old plan as the fallback: an iteration is then six calls on one
stream with no torch operation between them.
--reg adaptive (implies --forward closed --cost query) gives every env a regulariser of its own, a [N] tensor that lives across improvements and
control steps: So100Sim.lqr_reg starts each env's backward pass from it and, where the factor of Quu + reg I fails, runs that env's pass again
under a raised one inside the launch; after the line search ONE So100Sim.reg_schedule call lowers the reg of the envs whose plan improved and
raises the others'.  No result is looked at on the host in between: a bad linearisation or rollout becomes NaN gains, then a failed candidate,
then the old plan (the fallback) and a raised reg.  --control-cost and --damping set the weight of |a|^2 and the fixed reg (the adaptive one's
start); with both 0 the jaw's zero column of B gives Quu an exactly zero pivot, the fixed reg fails every env at the last step and the plan never
moves, and the adaptive one lifts itself to its floor.

    python examples/ilqr_reach.py [--envs 8] [--horizon 8] [--steps 100] [--iterations 2] [--backward {torch,query}] [--forward {linear,closed}]
                                  [--cost {torch,query}] [--reg {fixed,adaptive}] [--control-cost 1e-5] [--damping 1e-5]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from so100_mujoco_rl_amd.lib import ENV01, F_CUBE_PINNED, So100Sim   # noqa: E402

ARM = list(range(0, 6)) + list(range(12, 18))                  # the arm's block of the tangent state: dq 0..5, v 12..17
ALPHAS = (0.0,) + tuple(2.0**-i for i in range(7))             # the line search's candidates: the old plan, then 1, 1/2, .. 1/64
REG = dict(reg_min=1e-6, reg_max=1e4, reg_up=10.0)             # --reg adaptive: the floor, the ceiling and the factor up
REG_DOWN, REG_TRIES = 0.1, 8                                   # the factor down after an improvement; backward passes per env and improvement


class Ilqr:
    """policy(sim, obs) -> action [N, 6].  plan [N, horizon, 6] is the current action sequence, shifted by one step after every call;
    control_cost: the weight of |a|^2 beside |ee - cube|^2 (metres squared); damping: added to Q_uu (Levenberg-Marquardt); backward: "torch" (the
    loops below) or "query" (So100Sim.lqr: the same recursion in one launch); forward: "linear" (the linear model's u + du) or "closed" (the
    feedback law on the real dynamics at ALPHAS, the cheapest candidate per env; costs: per improve() the (chosen, alpha = 0) true costs [N]);
    cost: "torch" (the arithmetic below) or "query" (So100Sim.cost_terms and, with forward "closed", So100Sim.cost_select); reg: "fixed" (damping
    for every env) or "adaptive" (regs [N], one per env, starting from damping: So100Sim.lqr_reg and So100Sim.reg_schedule; forward and cost are then
    "closed" and "query")."""
    def __init__(self, horizon=8, iterations=2, control_cost=1e-5, damping=1e-5, backward="torch", forward="linear", cost="torch", reg="fixed"):
        self.H, self.iterations, self.control_cost, self.damping, self.backward, self.forward = horizon, iterations, control_cost, damping, backward, forward
        self.cost = cost
        self.adaptive = reg == "adaptive"
        if self.adaptive:
            self.forward, self.cost = "closed", "query"
        self.regs = None
        self.plan = None
        self.costs = []

    def improve(self, sim, q0, v0):
        N, H, dev = sim.n, self.H, sim.device
        U = self.plan
        roll = sim.trajectory(U.permute(1, 0, 2).contiguous(), q0, v0, mode="actions")           # row t: the state after action t
        Xq = torch.cat([q0[None], roll["qpos"][:-1]]); Xv = torch.cat([v0[None], roll["qvel"][:-1]])   # [H, N, .]: the state action t starts from
        d = sim.derivatives(U.permute(1, 0, 2).reshape(H*N, 6), Xq.reshape(H*N, 13), Xv.reshape(H*N, 12), mode="actions")
        if self.adaptive:
            self.improve_with_a_reg_per_env(sim, q0, v0, roll, d)
            return
        if bool(d["bad"].any()) or bool((roll["bad_step"] >= 0).any()):
            return
        if self.cost == "query":
            self.improve_with_cost_queries(sim, q0, v0, roll, d)
            return
        # Gauss-Newton terms of |ee(q) - cube|^2 at the states after each action
        qn = roll["qpos"]
        J = sim.jacobian(qn[..., :6].reshape(H*N, 6))["jacp"].reshape(H, N, 3, 6)
        r = roll["ee"] - qn[..., 6:9]
        lx = torch.zeros(H, N, 12, device=dev); lxx = torch.zeros(H, N, 12, 12, device=dev)
        lx[..., :6] = 2.0*torch.einsum("hnij,hni->hnj", J, r)
        lxx[..., :6, :6] = 2.0*torch.einsum("hnij,hnik->hnjk", J, J)
        eye = torch.eye(6, device=dev)
        if self.forward == "closed":
            Bq = d["B"].reshape(H, N, 24, 6).clone()
            Bq[..., 5] = 0.0                                         # the jaw does not move the end-effector point
            Ut = U.permute(1, 0, 2).contiguous()
            zero = torch.zeros(1, N, 12, device=dev)
            s = sim.lqr(d["A"].reshape(H, N, 24, 24), Bq, torch.cat([zero, lx]), torch.cat([zero[..., None].expand(1, N, 12, 12), lxx]),
                        lu=2.0*self.control_cost*Ut, luu=(2.0*self.control_cost*eye).expand(H, N, 6, 6), nx=12, reg=self.damping)
            if bool((s["bad"] >= 0).any()):
                return
            # the nonlinear forward pass at every step size in one launch; k's and K's jaw rows are zero (B's jaw column is), so the jaw keeps the plan's 0
            c = sim.closed_loop(Ut, roll["qpos"], roll["qvel"], s["K"], s["k"], alphas=ALPHAS, nx=12, qpos=q0, qvel=v0, mode="actions", clamp=(-1.0, 1.0))
            cube = q0[:, 6:9]                                        # pinned: where it is at the start
            cost = ((c["ee"] - cube[None, :, None]).square().sum(-1) + self.control_cost*c["u"].square().sum(-1)).sum(0)      # [N, L]
            cost = torch.where(c["bad_step"] >= 0, torch.full_like(cost, float("inf")), cost)
            best = cost.argmin(dim=1)
            env = torch.arange(N, device=dev)
            if bool(torch.isinf(cost[env, best]).any()):             # an env without a single candidate that got through: keep the plan
                return
            self.costs.append((cost[env, best].cpu(), cost[:, 0].cpu()))
            self.plan = c["u"][:, env, best].permute(1, 0, 2).contiguous()
            return
        if self.backward == "query":
            # one launch: A, B as the derivatives query wrote them (row t of the cost is the state BEFORE action t: a zero row in front)
            Bq = d["B"].reshape(H, N, 24, 6).clone()
            Bq[..., 5] = 0.0                                         # the jaw does not move the end-effector point
            Ut = U.permute(1, 0, 2).contiguous()
            zero = torch.zeros(1, N, 12, device=dev)
            s = sim.lqr(d["A"].reshape(H, N, 24, 24), Bq, torch.cat([zero, lx]), torch.cat([zero[..., None].expand(1, N, 12, 12), lxx]),
                        lu=2.0*self.control_cost*Ut, luu=(2.0*self.control_cost*eye).expand(H, N, 6, 6), nx=12, reg=self.damping, u=Ut, u_lo=-1.0, u_hi=1.0)
            if bool((s["bad"] >= 0).any()):
                return
            new = (Ut + s["du"]).permute(1, 0, 2).clone()
            new[..., 5] = 0.0
            self.plan = new
            return
        A = d["A"][:, ARM][:, :, ARM].reshape(H, N, 12, 12)
        B = d["B"][:, ARM].reshape(H, N, 12, 6).clone()
        B[..., 5] = 0.0                                              # the jaw does not move the end-effector point
        # the backward pass: V is the cost-to-go from the state after action t
        Vx, Vxx = lx[H - 1], lxx[H - 1]
        k = torch.zeros(H, N, 6, device=dev); K = torch.zeros(H, N, 6, 12, device=dev)
        for t in range(H - 1, -1, -1):
            At, Bt = A[t], B[t]
            Qx = torch.einsum("nij,ni->nj", At, Vx)
            Qu = 2.0*self.control_cost*U[:, t] + torch.einsum("nij,ni->nj", Bt, Vx)
            VA = Vxx @ At
            Qxx = At.transpose(1, 2) @ VA
            Qux = Bt.transpose(1, 2) @ VA
            Quu = Bt.transpose(1, 2) @ Vxx @ Bt + (2.0*self.control_cost + self.damping)*eye
            k[t] = -torch.linalg.solve(Quu, Qu[..., None])[..., 0]
            K[t] = -torch.linalg.solve(Quu, Qux)
            Vx = Qx + torch.einsum("nij,ni->nj", K[t], Qu + torch.einsum("nij,nj->ni", Quu, k[t])) + torch.einsum("nij,ni->nj", Qux, k[t])
            Vxx = Qxx + K[t].transpose(1, 2) @ Quu @ K[t] + K[t].transpose(1, 2) @ Qux + Qux.transpose(1, 2) @ K[t]
            Vxx = 0.5*(Vxx + Vxx.transpose(1, 2))
            if t > 0:
                Vx = Vx + lx[t - 1]; Vxx = Vxx + lxx[t - 1]
        # the forward pass on the linearisation, the actions kept in [-1, 1]
        dx = torch.zeros(N, 12, device=dev)
        new = U.clone()
        for t in range(H):
            new[:, t] = (U[:, t] + k[t] + torch.einsum("nij,nj->ni", K[t], dx)).clamp(-1.0, 1.0)
            new[:, t, 5] = 0.0
            dx = torch.einsum("nij,nj->ni", A[t], dx) + torch.einsum("nij,nj->ni", B[t], new[:, t] - U[:, t])
        self.plan = new

    def improve_with_cost_queries(self, sim, q0, v0, roll, d):
        """improve() from the rollout and its linearisation on, with the cost on the device: cost_terms -> lqr -> (closed_loop -> cost_select)"""
        N, H = sim.n, self.H
        Ut = self.plan.permute(1, 0, 2).contiguous()
        cost = dict(target_mode="cube", w_point=1.0, w_u=self.control_cost)
        Bq = d["B"].reshape(H, N, 24, 6).clone()
        Bq[..., 5] = 0.0                                             # the jaw does not move the end-effector point
        t = sim.cost_terms(roll["qpos"], roll["qvel"], Ut, nx=12, **cost)
        closed = self.forward == "closed"
        s = sim.lqr(d["A"].reshape(H, N, 24, 24), Bq, t["lx"], t["lxx"], lu=t["lu"], luu=t["luu"], nx=12, reg=self.damping,
                    **({} if closed else dict(u=Ut, u_lo=-1.0, u_hi=1.0)))
        if bool((s["bad"] >= 0).any()):
            return
        if not closed:
            new = (Ut + s["du"]).permute(1, 0, 2).clone()
            new[..., 5] = 0.0
            self.plan = new
            return
        c = sim.closed_loop(Ut, roll["qpos"], roll["qvel"], s["K"], s["k"], alphas=ALPHAS, nx=12, qpos=q0, qvel=v0, mode="actions", clamp=(-1.0, 1.0))
        # the pinned cube stays where it was at the start, so the cube target is the torch path's `cube`; an env without a single candidate that got
        # through keeps its plan (the fallback) with no look at the result on the host
        pick = sim.cost_select(c["qpos"], c["qvel"], c["u"], bad_step=c["bad_step"], u_fallback=Ut, **cost)
        self.costs.append((pick["best_cost"].cpu(), pick["cost"][:, 0].cpu()))
        self.plan = pick["u_best"].permute(1, 0, 2).contiguous()

    def improve_with_a_reg_per_env(self, sim, q0, v0, roll, d):
        """improve() from the rollout and its linearisation on, with no look at a result on the host: cost_terms -> lqr_reg -> closed_loop ->
        cost_select -> reg_schedule (with the two calls before them, seven on one stream).  A linearisation or rollout that is not finite gives NaN gains (bad = T), those a failed
        candidate at every step size, cost_select then keeps the old plan (best = -1), and reg_schedule raises that env's reg."""
        N, H = sim.n, self.H
        Ut = self.plan.permute(1, 0, 2).contiguous()
        cost = dict(target_mode="cube", w_point=1.0, w_u=self.control_cost)
        Bq = d["B"].reshape(H, N, 24, 6).clone()
        Bq[..., 5] = 0.0                                             # the jaw does not move the end-effector point
        t = sim.cost_terms(roll["qpos"], roll["qvel"], Ut, nx=12, **cost)
        s = sim.lqr_reg(d["A"].reshape(H, N, 24, 24), Bq, t["lx"], t["lxx"], lu=t["lu"], luu=t["luu"], nx=12, reg=self.regs, tries=REG_TRIES, **REG)
        c = sim.closed_loop(Ut, roll["qpos"], roll["qvel"], s["K"], s["k"], alphas=ALPHAS, nx=12, qpos=q0, qvel=v0, mode="actions", clamp=(-1.0, 1.0))
        pick = sim.cost_select(c["qpos"], c["qvel"], c["u"], bad_step=c["bad_step"], u_fallback=Ut, **cost)
        sim.reg_schedule(s["reg_used"], pick["best"], keep=0, reg_down=REG_DOWN, out=self.regs, **REG)      # ALPHAS[0] = 0: candidate 0 is the old plan
        self.costs.append((pick["best_cost"].cpu(), pick["cost"][:, 0].cpu()))
        self.plan = pick["u_best"].permute(1, 0, 2).contiguous()

    def __call__(self, sim, obs):
        if self.plan is None:
            self.plan = torch.zeros(sim.n, self.H, 6, device=sim.device)
        if self.adaptive and self.regs is None:
            self.regs = torch.full((sim.n,), float(self.damping), device=sim.device)
        qpos, qvel = sim.get_state()                                 # [13, N], [12, N]
        q0, v0 = qpos.t().contiguous(), qvel.t().contiguous()
        for _ in range(self.iterations):
            self.improve(sim, q0, v0)
        act = self.plan[:, 0].contiguous()
        self.plan = torch.cat([self.plan[:, 1:], torch.zeros(sim.n, 1, 6, device=sim.device)], dim=1)
        return act


def distance(sim):
    """mean |cube - ee| from the handle's state: the cube's position (rows 6..8 of qpos) against the end-effector point of the queries"""
    cube = sim.get_state()[0][6:9].t()
    return (cube - sim.kinematics()["ee"]).norm(dim=1).mean().item()


def run(sim, steps, policy):
    """(mean |cube - ee| at reset, the same after `steps` steps, mean reward per step) of `policy(sim, obs) -> action`, both distances
    read from the state"""
    obs = sim.reset()
    d0 = distance(sim)
    total = 0.0
    for _ in range(steps):
        obs, rew, _, _ = sim.step(policy(sim, obs))
        total += rew.mean().item()
    return d0, distance(sim), total/steps


def zero_action(sim, obs):
    return torch.zeros(sim.n, 6, device=sim.device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8); ap.add_argument("--horizon", type=int, default=8)
    ap.add_argument("--steps", type=int, default=100); ap.add_argument("--iterations", type=int, default=2)
    ap.add_argument("--backward", choices=("torch", "query"), default="torch")
    ap.add_argument("--forward", choices=("linear", "closed"), default="linear")
    ap.add_argument("--cost", choices=("torch", "query"), default="torch")
    ap.add_argument("--reg", choices=("fixed", "adaptive"), default="fixed")
    ap.add_argument("--control-cost", type=float, default=1e-5); ap.add_argument("--damping", type=float, default=1e-5)
    args = ap.parse_args()
    ilqr = Ilqr(args.horizon, args.iterations, args.control_cost, args.damping, backward=args.backward, forward=args.forward, cost=args.cost, reg=args.reg)
    for name, policy in (("iLQR", ilqr), ("zero action", zero_action)):
        sim = So100Sim(ENV01, args.envs, flags=F_CUBE_PINNED, max_episode_steps=0, seed=0)
        d0, d1, r = run(sim, args.steps, policy)
        print(f"{name:12s} mean |cube - ee|: {d0:.4f} m at reset -> {d1:.4f} m after {args.steps} steps; reward/step {r:+.4f}")
        sim.close()


if __name__ == "__main__":
    main()
