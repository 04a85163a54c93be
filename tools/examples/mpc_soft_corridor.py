"""Soft box constraints with ltvMpc(x_soft_l1=...): the moving, narrowing corridor of tools/examples/mpc_corridor.py with a gust.  16
quadcopters (the nonlinear model `models.QuadcopterEuler`) fly north through a corridor in the east position; at step 25 a gust throws
four of them 0.3 m through the right-hand wall.  The walls are a state box that differs at every stage, and from 0.3 m outside no input
within its bounds brings x_1 back inside: the hard QP of those vehicles has no solution.  The same hand loop

    relinearize(model, plan)  ->  update(x_lb=..., x_ub=...)  ->  solve(x, warm_start="shift")  ->  modelStep(model, x, u)

is flown twice.  The hard object loses the four vehicles to "infeasible" (they are left hovering at trim, outside the corridor); the object
with an l1 penalty on the corridor coordinate pays for the violation, keeps every solve "optimal" and flies them back inside.  Both counts
are printed.  The way back is flown at the limits of tilt and speed, where the vehicle (the nonlinear model) ends a hair beyond what the
linearisation planned: the other bounded states carry a large l1 as well (an exact penalty: they are held as if hard), so that a measured
state just outside them is solved from and not refused by the test on x0."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from zopt_amd import models, mpcUtils, pytrees  # noqa: E402

dt, N, steps, Bn = 0.1, 30, 60, 16
model = models.QuadcopterEuler(dt)
uTrim = np.asarray(models.QuadcopterEuler.uTrim, dtype=np.float64)
x_ub = np.array([1, 1, 1, 0.3, 0.3, 0.1, 0.5, 0.5, np.inf, np.inf, np.inf, np.inf])
u_ub = np.array([3.0, 3, 3, 3])
Q, R = np.eye(12), np.eye(4)
speed, NORTH, EAST = 0.5, 9, 10      # (states 9..11: the position, north / east / down)
GUST_STEP, GUST_VEHICLES, GUST_DEPTH = 25, slice(0, 4), 0.3
SOFT_L1 = np.where(np.arange(12) == EAST, 20.0, np.where(np.isfinite(x_ub), 200.0, np.inf))   # the corridor; the demo's box, held stiffly


def walls(north):
    """(centre, half-width) of the corridor in the east position at a north position"""
    return 0.6 * np.sin(0.8 * north), np.maximum(1.0 - 0.22 * north, 0.15)


def boxes(step):
    """x_lb, x_ub (N+1, 12) of MPC step `step`: the demo's box with the corridor's walls where the reference is at each stage; row 0, the
    test on the measured state, stays the demo's box"""
    north = speed * dt * (step + np.arange(N + 1))
    centre, half = walls(north)
    lb, ub = np.tile(-x_ub, (N + 1, 1)), np.tile(x_ub, (N + 1, 1))
    lb[1:, EAST], ub[1:, EAST] = (centre - half)[1:], (centre + half)[1:]
    return lb, ub


def window(step):
    north = speed * dt * (step + np.arange(N + 1))
    xRef = np.zeros((N + 1, 12))
    xRef[:, NORTH], xRef[:, 0], xRef[:, EAST] = north, speed, walls(north)[0]
    return xRef


opts = dict(eps_abs=1e-3, eps_rel=1e-3, max_iter=4000)
dev = dict(dtype=torch.float64, device="cuda")
trim = torch.as_tensor(uTrim, **dev)


def fly(soft):
    """the run with (soft) or without the l1 penalty on the east position -> (vehicle-steps lost to "infeasible", solves that were not
    "optimal", vehicles more than 1 cm outside the corridor at the end)"""
    rng = np.random.default_rng(0)
    x = torch.zeros((Bn, 12), **dev)
    x[:, EAST] = torch.as_tensor(rng.uniform(-0.8, 0.8, Bn), **dev)
    uRef = torch.as_tensor(np.tile(uTrim, (Bn, N, 1)), **dev)
    plan = pytrees.Trajectory(x[:, None, :].expand(Bn, N + 1, 12).contiguous(), uRef.clone())
    lb, ub = boxes(0)
    weights = dict(x_soft_l1=SOFT_L1) if soft else {}
    prob = mpcUtils.ltvMpc.fromModel(model, plan, Q, R, lb, ub, uTrim - u_ub, uTrim + u_ub, stage_varying=("x_lb", "x_ub"), **weights)
    lost = not_optimal = 0
    for i in range(steps):
        if i == GUST_STEP:                                               # the gust: through the right-hand wall
            centre, half = walls(x[GUST_VEHICLES, NORTH].cpu().numpy())
            x[GUST_VEHICLES, EAST] = torch.as_tensor(centre + half + GUST_DEPTH, **dev)
        prob.relinearize(model, plan)
        if i:
            lb, ub = boxes(i)
            prob.update(x_lb=lb, x_ub=ub)
        u, traj, status = prob.solve(x, xRef=window(i), uRef=uRef, warm_start="shift" if i else False, **opts)
        bad = torch.as_tensor(status == "infeasible", device="cuda")
        lost += int(bad.sum())
        not_optimal += int(np.sum(status != "optimal"))
        u = torch.where(bad[:, None], trim, u)                           # a vehicle without a solution hovers
        centre, half = walls(x[:, NORTH].cpu().numpy())
        gap = half - np.abs(x[:, EAST].cpu().numpy() - centre)
        if i in (GUST_STEP, GUST_STEP + 5, GUST_STEP + 15, steps - 1):
            print(f"  step {i:2d}: smallest gap to a wall {gap.min():+.3f} m, {int(np.sum(status == 'optimal'))}/{Bn} optimal, "
                  f"{int(bad.sum())} infeasible, {int(prob.last_iterations.max())} ADMM iterations")
        x = mpcUtils.modelStep(model, x, u)
        plan = pytrees.Trajectory(torch.cat([traj.xTraj[:, 1:], traj.xTraj[:, -1:]], dim=1), torch.cat([traj.uTraj[:, 1:], traj.uTraj[:, -1:]], dim=1))
    centre, half = walls(x[:, NORTH].cpu().numpy())
    outside = int(np.sum(half - np.abs(x[:, EAST].cpu().numpy() - centre) < -1e-2))
    return lost, not_optimal, outside


for soft in (False, True):
    print("soft walls (x_soft_l1 = 20 on the east position, 200 on the other bounded states):" if soft else "hard walls:")
    lost, not_optimal, outside = fly(soft)
    print(f"  {steps} steps x {Bn} vehicles: {lost} vehicle-steps lost to \"infeasible\", {not_optimal} solves not \"optimal\", "
          f"{outside} vehicles outside the corridor at the end")
