"""iLQR with state bounds: a batch of quadcopters, each steered to its own goal with a `models.TrackingCost` about hover, under a
ceiling, a cap on the body velocities and thrust limits -- `models.StateBox` around `models.InputBox` around the model, solved by
`ilqrUtils.constrainedIterativeLqr` (an augmented-Lagrangian outer loop around the fused iLQR: a penalty per step and component on
the cost, a multiplier and penalty update between inner solves).  The same problem without the state box is solved next to it: its
states leave the bounds, the constrained run's stay inside to `ctol` wherever it reports `converged`."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from zopt_amd import ilqrUtils, models  # noqa: E402

dt, T, Bn = 0.1, 50, 256
model = models.QuadcopterEuler(dt)
uTrim = np.asarray(models.QuadcopterEuler.uTrim, dtype=np.float64)
lim = np.array([2.0, 0.05, 0.05, 0.05])
boxed = models.InputBox(model, uTrim - lim, uTrim + lim)
x_lb, x_ub = np.full(12, -np.inf), np.full(12, np.inf)
x_lb[11] = -1.5                                   # positions are states 9..11, z points down: a ceiling 1.5 m above the start
x_lb[0:3], x_ub[0:3] = -1.0, 1.0                  # body velocities within 1 m/s
dev = dict(dtype=torch.float64, device="cuda")

rng = np.random.default_rng(0)
goal = torch.zeros((Bn, 12), **dev)
goal[:, 9:12] = torch.as_tensor(rng.uniform(-2, 2, (Bn, 3)), **dev)
x0 = torch.zeros((Bn, 12), **dev)
uGuess = torch.as_tensor(np.tile(uTrim, (Bn, T, 1)), **dev)
cost = models.TrackingCost(np.eye(12), np.eye(4), 10 * np.eye(12), xRef=goal[:, None, :], uRef=uTrim)
lo, hi = torch.as_tensor(x_lb, **dev), torch.as_tensor(x_ub, **dev)


def worst(traj):
    return torch.clamp(torch.maximum(lo - traj.xTraj[:, 1:], traj.xTraj[:, 1:] - hi), min=0).flatten(1).max(1).values


sb = models.StateBox(boxed, x_lb, x_ub)
traj, L, J, converged, info = ilqrUtils.constrainedIterativeLqr(sb, cost, cost, x0, uGuess)
assert bool((info.violation[converged] <= sb.ctol).all()), "a converged trajectory violates its bounds by more than ctol"
assert torch.equal(worst(traj), info.violation)
miss = torch.linalg.norm(traj.xTraj[:, -1, 9:12] - goal[:, 9:12], dim=1)
print(f"with the state box   : {int(converged.sum())}/{Bn} done, mean cost {float(J.mean()):.3f}, largest violation "
      f"{float(info.violation.max()):.2e} (ctol {sb.ctol:g}), distance to the goal at the end mean {float(miss.mean()):.3f} m")
print(f"  outer iterations: mean {float(info.outerIterations.double().mean()):.2f}, max {int(info.outerIterations.max())}; inner iterations "
      f"in total: mean {float(info.innerIterations.sum(-1).double().mean()):.1f}, max {int(info.innerIterations.sum(-1).max())}; final mu up to "
      f"{float(info.mu.max()):g}; trajectories with an active bound: {int(((info.lam_ub > 0) | (info.lam_lb > 0)).flatten(1).any(1).sum())}")
free = ilqrUtils.iterativeLqr(boxed, cost, cost, x0, uGuess)
missf = torch.linalg.norm(free[0].xTraj[:, -1, 9:12] - goal[:, 9:12], dim=1)
print(f"without the state box: {int(free[3].sum())}/{Bn} converged, mean cost {float(free[2].mean()):.3f}, largest violation "
      f"{float(worst(free[0]).max()):.3f}, distance to the goal at the end mean {float(missf.mean()):.3f} m")
