"""iLQR with actuator limits: a batch of quadcopters, each steered to its own goal with a `models.TrackingCost` about hover, with
the thrust limited to uTrim +- 2 and the moments to +- 0.05 -- `models.InputBox` around the model on the fused `iterativeLqr`
(control-limited DDP: a box-constrained QP per step of the backward pass, clipped rollouts).  The same problem without the box is
solved next to it: its inputs leave the limits, the boxed run's never do."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from zopt_amd import ilqrUtils, models, simulator  # noqa: E402

dt, T, Bn = 0.1, 50, 256
model = models.QuadcopterEuler(dt)
uTrim = np.asarray(models.QuadcopterEuler.uTrim, dtype=np.float64)
lim = np.array([2.0, 0.05, 0.05, 0.05])
u_lb, u_ub = uTrim - lim, uTrim + lim
dev = dict(dtype=torch.float64, device="cuda")

rng = np.random.default_rng(0)
torch.manual_seed(0)
goal = torch.zeros((Bn, 12), **dev)
goal[:, 9:12] = torch.as_tensor(rng.uniform(-2, 2, (Bn, 3)), **dev)          # positions are states 9..11
x0 = torch.zeros((Bn, 12), **dev)
uGuess = torch.as_tensor(np.tile(uTrim, (Bn, T, 1)), **dev)
cost = models.TrackingCost(np.eye(12), np.eye(4), 10 * np.eye(12), xRef=goal[:, None, :], uRef=uTrim)
lo, hi = torch.as_tensor(u_lb, **dev), torch.as_tensor(u_ub, **dev)


def report(name, traj, J, converged):
    viol = torch.clamp(torch.maximum(lo - traj.uTraj, traj.uTraj - hi), min=0)
    miss = torch.linalg.norm(traj.xTraj[:, -1, 9:12] - goal[:, 9:12], dim=1)
    at = ((traj.uTraj == lo) | (traj.uTraj == hi)).double().mean()
    print(f"{name}: {int(converged.sum())}/{Bn} converged, mean cost {float(J.mean()):.3f}, distance to the goal at the end mean "
          f"{float(miss.mean()):.3f} m, largest violation of the limits {float(viol.max()):.4f} (thrust {float(viol[..., 0].max()):.4f}, "
          f"moments {float(viol[..., 1:].max()):.4f}), inputs on a limit {100 * float(at):.1f} %")


boxed = models.InputBox(model, u_lb, u_ub)
traj, L, J, converged = ilqrUtils.iterativeLqr(boxed, cost, cost, x0, uGuess)
report("with the box   ", traj, J, converged)
free = ilqrUtils.iterativeLqr(model, cost, cost, x0, uGuess)
report("without the box", free[0], free[2], free[3])

# the gains in closed loop from displaced starts, through the same box: the feedback rows of clamped inputs are zero, the rest clips
xd = x0.clone()
xd[:, 9:12] += 0.05 * torch.randn((Bn, 3), **dev)
sim = simulator.simulateTrackingController(boxed, xd, L, traj)
viol = torch.clamp(torch.maximum(lo - sim.uTraj, sim.uTraj - hi), min=0)
print(f"closed loop from starts displaced by 5 cm, through the box: largest violation {float(viol.max()):.4f}, distance to the goal at the end "
      f"mean {float(torch.linalg.norm(sim.xTraj[:, -1, 9:12] - goal[:, 9:12], dim=1).mean()):.3f} m")
