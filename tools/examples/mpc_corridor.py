"""A moving, narrowing corridor with ltvMpc(stage_varying=...): 16 quadcopters (the nonlinear model `models.QuadcopterEuler`, the weights and
bounds of the reference's demos/lqrMpc.py) fly north at 0.5 m/s through a corridor in the east position whose centre swings sideways and
whose half-width shrinks from 1.0 m to 0.15 m along the track.  The corridor is a state box that differs at every stage of the horizon:
stage k of step i sees the walls at the position the plan expects to be at then.  The loop is the real-time iteration written out -- the
one-call `realTimeIteration` keeps one box per problem and refuses a stage-varying object --:

    relinearize(model, plan)  ->  update(x_lb=..., x_ub=...)  ->  solve(x, warm_start="shift")  ->  modelStep(model, x, u)

`relinearize` writes only A_k, B_k, c_k; `update` with bounds rewrites the device boxes and keeps the tables, so a step costs the one
setup launch the new linearisation needs anyway.  Printed: how close the vehicles come to the walls, and that no vehicle leaves them."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from zopt_amd import models, mpcUtils, pytrees  # noqa: E402

dt, N, steps, Bn = 0.1, 30, 80, 16
model = models.QuadcopterEuler(dt)
uTrim = np.asarray(models.QuadcopterEuler.uTrim, dtype=np.float64)
x_ub = np.array([1, 1, 1, 0.3, 0.3, 0.1, 0.5, 0.5, np.inf, np.inf, np.inf, np.inf])
u_ub = np.array([3.0, 3, 3, 3])
Q, R = np.eye(12), np.eye(4)
speed, NORTH, EAST = 0.5, 9, 10      # (states 9..11: the position, north / east / down)


def walls(north):
    """(centre, half-width) of the corridor in the east position at a north position"""
    return 0.6 * np.sin(0.8 * north), np.maximum(1.0 - 0.22 * north, 0.15)


def boxes(step):
    """x_lb, x_ub (N+1, 12) of MPC step `step`: the demo's box with the corridor's walls where the reference is at each stage.  Row 0 is the
    test on the measured state: it stays the demo's box (a vehicle that has drifted outside must still be brought back)."""
    north = speed * dt * (step + np.arange(N + 1))
    centre, half = walls(north)
    lb, ub = np.tile(-x_ub, (N + 1, 1)), np.tile(x_ub, (N + 1, 1))
    lb[1:, EAST], ub[1:, EAST] = (centre - half)[1:], (centre + half)[1:]
    return lb, ub


def window(step):
    """xRef (N+1, 12): north along the track at `speed`; the east position is free inside the corridor (its reference is the centre line)"""
    north = speed * dt * (step + np.arange(N + 1))
    xRef = np.zeros((N + 1, 12))
    xRef[:, NORTH], xRef[:, 0], xRef[:, EAST] = north, speed, walls(north)[0]
    return xRef


opts = dict(eps_abs=1e-3, eps_rel=1e-3, max_iter=4000)
dev = dict(dtype=torch.float64, device="cuda")
rng = np.random.default_rng(0)
x = torch.zeros((Bn, 12), **dev)
x[:, EAST] = torch.as_tensor(rng.uniform(-0.8, 0.8, Bn), **dev)      # spread over the corridor's mouth
uRef = torch.as_tensor(np.tile(uTrim, (Bn, N, 1)), **dev)
plan = pytrees.Trajectory(x[:, None, :].expand(Bn, N + 1, 12).contiguous(), uRef.clone())       # the first expansion: hover at the start
lb, ub = boxes(0)
prob = mpcUtils.ltvMpc.fromModel(model, plan, Q, R, lb, ub, uTrim - u_ub, uTrim + u_ub, stage_varying=("x_lb", "x_ub"))

margin, outside = [], 0
for i in range(steps):
    prob.relinearize(model, plan)                                    # A_k, B_k, c_k on the device
    if i:
        lb, ub = boxes(i)
        prob.update(x_lb=lb, x_ub=ub)                                # the corridor as this step's horizon sees it; the tables stay
    u, traj, status = prob.solve(x, xRef=window(i), uRef=uRef, warm_start="shift" if i else False, **opts)
    centre, half = walls(x[:, NORTH].cpu().numpy())
    gap = half - np.abs(x[:, EAST].cpu().numpy() - centre)           # distance to the nearer wall where the vehicle is now
    margin.append(gap.min())
    outside += int(np.sum(gap < -1e-2))
    if i % 10 == 0 or i == steps - 1:
        print(f"step {i:2d}: north {float(x[:, NORTH].mean()):.2f} m, half-width {half.mean():.2f} m, smallest gap to a wall {gap.min():+.3f} m, "
              f"{int(prob.last_iterations.max())} ADMM iterations, {int(np.sum(status == 'optimal'))}/{Bn} optimal")
    x = mpcUtils.modelStep(model, x, u)                              # the vehicle: the nonlinear model
    plan = pytrees.Trajectory(torch.cat([traj.xTraj[:, 1:], traj.xTraj[:, -1:]], dim=1), torch.cat([traj.uTraj[:, 1:], traj.uTraj[:, -1:]], dim=1))

print(f"{steps} steps: smallest gap to a wall over the run {min(margin):+.3f} m; vehicle-steps more than 1 cm outside the corridor: {outside}")
try:
    prob.realTimeIteration(model, x, 1)
except NotImplementedError as e:
    print("realTimeIteration on this object:", str(e)[:95] + " ...")
