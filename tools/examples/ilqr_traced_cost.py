"""iLQR and DDP with a user-written COST through the fused path: `models.TracedCost` records plain NumPy cost functions once and the HIP
kernels interpret the recordings inside the line search (next to the model step) and the expansion (dual and hyper-dual numbers) -- the
reference's `runningCost(x, u)`, `terminalCost(x)` callables (demos/iterativeLqr.py:35-36) without torch.func.

512 kinematic cars, each driven to ITS goal past ITS obstacle: the goal and the centre of the keep-out zone are per-vehicle parameters
(`params`: no derivative is taken with respect to them), the zone is a smooth penalty w / (d^2 + eps) -- neither a QuadraticCost nor a
TrackingCost.  The per-point cost Hessians are indefinite near the obstacle; the solve PD-projects them in every iteration, as the
reference does (ilqrUtils.py:309-313).  The dynamics are a `models.TracedModel`; a registered model works the same way.
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


def running_cost(x, u, p):
    """p = [goal x, goal y, obstacle x, obstacle y]"""
    to_goal = (x[0] - p[0]) ** 2 + (x[1] - p[1]) ** 2
    to_obstacle = (x[0] - p[2]) ** 2 + (x[1] - p[3]) ** 2
    return 0.5 * to_goal + 0.05 * x[3] ** 2 + 0.2 * u[0] ** 2 + 0.1 * u[1] ** 2 + 4.0 / (to_obstacle + 0.5)


def terminal_cost(x, p):
    return 20.0 * ((x[0] - p[0]) ** 2 + (x[1] - p[1]) ** 2) + 2.0 * x[3] ** 2


dev = dict(dtype=torch.float64, device="cuda")
rng = np.random.default_rng(0)
Bn, T = 512, 60
goal = rng.uniform(-4, 4, (Bn, 2))
obstacle = 0.5 * goal + rng.uniform(-0.3, 0.3, (Bn, 2))          # about half way, a little off the straight line
cost = models.TracedCost(running_cost, terminal_cost, 4, 2, params=np.concatenate([goal, obstacle], 1))
t = cost.running_tape
print(f"running-cost tape: {len(t.code)} instructions, {len(t.consts)} constants, {t.n_slots} slots, not affine in variables {t.mask:#x}")
cars = models.TracedModel(car, 4, 2)
x0 = torch.as_tensor(np.column_stack([np.zeros((Bn, 2)), np.arctan2(goal[:, 1], goal[:, 0]), np.ones(Bn)]), **dev)
uGuess = torch.zeros((Bn, T, 2), **dev)
for name, solve in (("iterativeLqr", ilqrUtils.iterativeLqr), ("differentialDynamicProgramming", ilqrUtils.differentialDynamicProgramming)):
    traj, L, J, converged = solve(cars, cost, cost, x0, uGuess)
    xy = traj.xTraj[:, :, :2].cpu().numpy()
    miss = np.linalg.norm(xy[:, -1] - goal, axis=1)
    clearance = np.linalg.norm(xy - obstacle[:, None, :], axis=2).min(1)
    print(f"{name}: {int(converged.sum())}/{Bn} cars converged, distance to the goal at the end mean {miss.mean():.3f} m, "
          f"closest approach to the obstacle mean {clearance.mean():.2f} m (min {clearance.min():.2f} m), "
          f"J == cost(traj): {bool(torch.allclose(cost(traj), J, rtol=1e-12))}")
