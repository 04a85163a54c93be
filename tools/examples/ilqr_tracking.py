"""iLQR with a tracking cost: a batch of quadcopters, each steered to its OWN goal position, with the input weight about hover
(uRef = uTrim) instead of about zero thrust -- `models.TrackingCost` on the fused `iterativeLqr`.  The goals are one row per
trajectory (`goal[:, None, :]`: read with a step stride of 0, nothing is tiled over the horizon).  The optimised trajectory is then
handed to `ltvMpc.fromModel` as the `plan` it linearises about, and one MPC solve tracks it under the demo's boxes."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from zopt_amd import ilqrUtils, models, mpcUtils, pytrees  # noqa: E402

dt, T, Bn = 0.1, 50, 256
model = models.QuadcopterEuler(dt)
uTrim = np.asarray(models.QuadcopterEuler.uTrim, dtype=np.float64)
Q, R, Qf = np.eye(12), np.eye(4), 10 * np.eye(12)
dev = dict(dtype=torch.float64, device="cuda")

rng = np.random.default_rng(0)
goal = torch.zeros((Bn, 12), **dev)
goal[:, 9:12] = torch.as_tensor(rng.uniform(-2, 2, (Bn, 3)), **dev)          # positions are states 9..11
x0 = torch.zeros((Bn, 12), **dev)
uGuess = torch.as_tensor(np.tile(uTrim, (Bn, T, 1)), **dev)

cost = models.TrackingCost(Q, R, Qf, xRef=goal[:, None, :], uRef=uTrim)
traj, L, J, converged = ilqrUtils.iterativeLqr(model, cost, cost, x0, uGuess)
miss = torch.linalg.norm(traj.xTraj[:, -1, 9:12] - goal[:, 9:12], dim=1)
print(f"iterativeLqr with a goal per trajectory: {int(converged.sum())}/{Bn} converged, distance to the goal at the end of the horizon "
      f"mean {float(miss.mean()):.3f} m max {float(miss.max()):.3f} m, thrust about hover: mean |u0 - g| "
      f"{float((traj.uTraj[:, :, 0] - uTrim[0]).abs().mean()):.3f}")

# the same weights about the origin (QuadraticCost) pull every vehicle to 0 and the thrust towards 0 instead of hover
plain = models.QuadraticCost(Q, R, Qf)
t0, _, _, _ = ilqrUtils.iterativeLqr(model, plain, plain, x0, uGuess)
print(f"QuadraticCost on the same starts: the vehicles sink {float(t0.xTraj[:, -1, 11].mean()):.2f} m (z points down), "
      f"mean thrust {float(t0.uTraj[:, :, 0].mean()):.2f} against hover's {uTrim[0]}")

# ---- the optimised trajectory as the plan of the time-varying MPC
N = 30
x_ub = np.array([1, 1, 1, 0.3, 0.3, 0.1, 0.5, 0.5, np.inf, np.inf, np.inf, np.inf])
u_ub = np.array([3.0, 3, 3, 3])
plan = pytrees.Trajectory(traj.xTraj[:, :N + 1].contiguous(), traj.uTraj[:, :N].contiguous())
prob = mpcUtils.ltvMpc.fromModel(model, plan, Q, R, -x_ub, x_ub, uTrim - u_ub, uTrim + u_ub)
u, mpc, status = prob.solve(x0, xRef=plan.xTraj, uRef=plan.uTraj, eps_abs=1e-3, eps_rel=1e-3, max_iter=4000)
print(f"ltvMpc about that plan: {int(np.sum(status == 'optimal'))}/{Bn} optimal, first input differs from the plan's by at most "
      f"{float((u - plan.uTraj[:, 0]).abs().max()):.3f}")
