"""iLQR with actuator limits that move along the horizon: a batch of quadcopters about hover, each steered to its own goal with a
`models.TrackingCost`, through `models.InputBox(model, u_lb, u_ub, stage_varying=True)` on the fused `iterativeLqr`.  The schedule:
  * the first two inputs are committed already (delay compensation in a receding-horizon loop): `u_lb[k] == u_ub[k]` for k < 2, a value
    per trajectory;
  * the thrust ceiling drops halfway along the horizon (uTrim + 2 before, uTrim + 0.5 from step T / 2 on); the moments stay within
    +- 0.05 throughout.
Every returned input lies inside the box of its own step."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from zopt_amd import ilqrUtils, models  # noqa: E402

dt, T, Bn, d = 0.1, 50, 256, 2
model = models.QuadcopterEuler(dt)
uTrim = np.asarray(models.QuadcopterEuler.uTrim, dtype=np.float64)
dev = dict(dtype=torch.float64, device="cuda")

rng = np.random.default_rng(0)
lim = np.array([2.0, 0.05, 0.05, 0.05])
u_lb = np.tile(uTrim - lim, (Bn, T, 1))                                       # (batch, T, m): a row per trajectory and step
u_ub = np.tile(uTrim + lim, (Bn, T, 1))
u_ub[:, T // 2:, 0] = uTrim[0] + 0.5                                          # the thrust ceiling drops halfway
committed = uTrim + np.array([0.5, 0.02, 0.02, 0.02]) * rng.uniform(-1, 1, (Bn, d, 4))
u_lb[:, :d], u_ub[:, :d] = committed, committed                               # the committed inputs: pinned

goal = torch.zeros((Bn, 12), **dev)
goal[:, 9:12] = torch.as_tensor(rng.uniform(-2, 2, (Bn, 3)), **dev)          # positions are states 9..11
x0 = torch.zeros((Bn, 12), **dev)
uGuess = torch.as_tensor(np.tile(uTrim, (Bn, T, 1)), **dev)
cost = models.TrackingCost(np.eye(12), np.eye(4), 10 * np.eye(12), xRef=goal[:, None, :], uRef=uTrim)

boxed = models.InputBox(model, u_lb, u_ub, stage_varying=True)
traj, L, J, converged = ilqrUtils.iterativeLqr(boxed, cost, cost, x0, uGuess)
lo, hi = torch.as_tensor(u_lb, **dev), torch.as_tensor(u_ub, **dev)
inside = bool(((traj.uTraj >= lo) & (traj.uTraj <= hi)).all())
pinned = bool((traj.uTraj[:, :d] == lo[:, :d]).all())
late = traj.uTraj[:, T // 2:, 0]
miss = torch.linalg.norm(traj.xTraj[:, -1, 9:12] - goal[:, 9:12], dim=1)
print(f"{int(converged.sum())}/{Bn} converged, mean cost {float(J.mean()):.3f}, distance to the goal at the end mean {float(miss.mean()):.3f} m")
print(f"every returned input inside its own step's box: {inside}; the first {d} inputs equal the committed ones: {pinned}")
print(f"largest thrust before step {T // 2}: {float(traj.uTraj[:, :T // 2, 0].max()):.3f} (ceiling {uTrim[0] + 2:.3f}), from it on: "
      f"{float(late.max()):.3f} (ceiling {uTrim[0] + 0.5:.3f}); inputs on a limit beyond the committed steps "
      f"{100 * float(((traj.uTraj[:, d:] == lo[:, d:]) | (traj.uTraj[:, d:] == hi[:, d:])).double().mean()):.1f} %")
assert inside and pinned
