"""iLQR with user-written HARD constraints through the fused path: `models.TracedConstraint` records plain NumPy functions g(x, u, p) <= 0
once and the HIP kernels interpret the recording inside the penalty line search, the penalty expansion (dual numbers) and the multiplier
update of an augmented-Lagrangian loop around the fused iLQR (AL-iLQR).

512 kinematic cars, each driven to ITS goal past ITS disc: the centre and radius of the keep-out disc are per-vehicle parameters of
the constraint (`params`: no derivative is taken with respect to them), and a speed limit rides along as a second row.  The cost is a
`QuadraticCost` about the origin, so every car's frame is shifted to put its goal there (a traced model takes no `TrackingCost` yet).  A soft keep-out penalty (tools/examples/ilqr_traced_cost.py) guarantees nothing about
the solution; here every vehicle that is reported `converged` is outside its disc to `ctol`.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from zopt_amd import ilqrUtils, models  # noqa: E402


def car(x, u, dt=0.1, wheelbase=2.5):
    """state [px, py, heading, speed], control [steering angle, acceleration]"""
    px, py, th, v = x
    return np.array([px + dt * v * np.cos(th), py + dt * v * np.sin(th), th + dt * v * np.tan(u[0]) / wheelbase, v + dt * u[1]])


def keep_out(x, u, p):
    """p = [disc x, disc y, radius]: outside the disc, and no faster than 3 m/s"""
    return np.array([p[2] ** 2 - ((x[0] - p[0]) ** 2 + (x[1] - p[1]) ** 2), x[3] ** 2 - 9.0])


dev = dict(dtype=torch.float64, device="cuda")
rng = np.random.default_rng(0)
Bn, T = 512, 60
goal = rng.uniform(-4, 4, (Bn, 2))
disc = np.column_stack([0.5 * goal + rng.uniform(-0.2, 0.2, (Bn, 2)), rng.uniform(0.3, 0.6, Bn)])    # half way, a little off the line
shifted = disc - np.column_stack([goal, np.zeros(Bn)])             # the disc in the frame whose origin is the car's goal
cars = models.TracedConstraint(models.TracedModel(car, 4, 2), keep_out, 2, params=shifted, ctol=1e-4)
t = cars.stage_tape
print(f"constraint tape: {len(t.code)} instructions, {len(t.consts)} constants, {t.n_slots} slots, {len(t.outputs)} rows")
cost = models.QuadraticCost(np.diag([0.5, 0.5, 0.0, 0.05]), np.diag([0.2, 0.1]), np.diag([20.0, 20.0, 0.0, 2.0]))
x0 = torch.as_tensor(np.column_stack([-goal, np.arctan2(goal[:, 1], goal[:, 0]), np.ones(Bn)]), **dev)
uGuess = torch.zeros((Bn, T, 2), **dev)
traj, L, J, converged, info = ilqrUtils.constrainedIterativeLqr(cars, cost, cost, x0, uGuess)
xy = traj.xTraj[:, :, :2].cpu().numpy() + goal[:, None, :]
clearance = (np.linalg.norm(xy[:, :-1] - disc[:, None, :2], axis=2) - disc[:, None, 2]).min(1)
miss = np.linalg.norm(xy[:, -1] - goal, axis=1)
conv = converged.cpu().numpy()
print(f"constrainedIterativeLqr: {int(conv.sum())}/{Bn} cars done after at most {int(info.outerIterations.max())} outer iterations, "
      f"largest violation among them {float(info.violation[converged].max()):.2e}, distance to the goal at the end mean {miss.mean():.3f} m, "
      f"clearance to the disc's edge min {clearance[conv].min():.4f} m (a negative clearance c is a violation of about 2 r |c|), "
      f"{int((info.lam > 0).flatten(1).any(1).sum())} cars have an active row")
assert np.all(info.violation[converged].cpu().numpy() <= cars.ctol)
g, _ = cars.values(traj.xTraj, traj.uTraj)
assert bool((g[converged] <= cars.ctol).all()), "a converged vehicle is inside its disc"
print("every converged vehicle is outside its obstacle to ctol")
