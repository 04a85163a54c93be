"""Real-time-iteration nonlinear MPC with ltvMpc: 64 quadcopters (the nonlinear model `models.QuadcopterEuler`, the weights and bounds of
the reference's demos/lqrMpc.py) each follow a position ramp, as tools/examples/mpc_tracking.py does.  At every step the model is
linearised about the SHIFTED PREVIOUS PLAN on the device (`relinearize`: A_k, B_k, c_k straight into the solver's arrays), one solve starts
from the shifted iterates of the previous one, and the vehicle takes the first input THROUGH THE NONLINEAR MODEL (`mpcUtils.modelStep`).
The loop is run twice: written out with those public calls, and as the one call `realTimeIteration`, which gives the same bits without
the host in the loop.  Next to it the same closed loop with lqrMpc on the model linearised once, at trim: its plan ignores how attitude
turns the thrust, so it tracks the ramp with a larger error."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from zopt_amd import models, mpcUtils, pytrees  # noqa: E402

dt, N, steps, Bn = 0.1, 30, 50, 64
model = models.QuadcopterEuler(dt)
uTrim = np.asarray(models.QuadcopterEuler.uTrim, dtype=np.float64)
x_ub = np.array([1, 1, 1, 0.3, 0.3, 0.1, 0.5, 0.5, np.inf, np.inf, np.inf, np.inf])
u_ub = np.array([3.0, 3, 3, 3])
Q, R = np.eye(12), np.eye(4)

rng = np.random.default_rng(0)
d = rng.standard_normal((Bn, 3))
d /= np.linalg.norm(d, axis=1, keepdims=True)
vel, p0 = d * rng.uniform(0.2, 0.6, (Bn, 1)), 2.5 * d          # ramp speed inside the velocity box, starting 2.5 m ahead


def window(step):
    """xRef (Bn, N+1, 12) of MPC step `step`: positions (states 9..11) on the ramp, velocities (states 0..2) its slope"""
    t = dt * (step + np.arange(N + 1))
    xRef = np.zeros((Bn, N + 1, 12))
    xRef[:, :, 9:12] = p0[:, None, :] + vel[:, None, :] * t[None, :, None]
    xRef[:, :, 0:3] = vel[:, None, :]
    return xRef


def reference(rows):
    """the first `rows` rows of the ramp: what `realTimeIteration` takes (steps + N rows); step i tracks rows i .. i + N"""
    t = dt * np.arange(rows)
    xRef = np.zeros((Bn, rows, 12))
    xRef[:, :, 9:12] = p0[:, None, :] + vel[:, None, :] * t[None, :, None]
    xRef[:, :, 0:3] = vel[:, None, :]
    return xRef


opts = dict(eps_abs=1e-2, eps_rel=1e-2, max_iter=4000)
dev = dict(dtype=torch.float64, device="cuda")
lo, hi = torch.as_tensor(-x_ub + 1e-6, **dev), torch.as_tensor(x_ub - 1e-6, **dev)
uRef = torch.as_tensor(np.tile(uTrim, (Bn, N, 1)), **dev)

# ---- the linear MPC of the demo: one linearisation, at trim (deviation coordinates in u)
lin = pytrees.AffineDynamics.from_function(model, np.zeros(12), uTrim)
lti = mpcUtils.lqrMpc(np.asarray(lin.f_x), np.asarray(lin.f_u), Q, R, N, -x_ub, x_ub, -u_ub, u_ub)
x = torch.zeros((Bn, 12), **dev)
err_lti = []
for i in range(steps):
    x = torch.minimum(torch.maximum(x, lo), hi)
    xRef = torch.as_tensor(window(i), **dev)
    err_lti.append(torch.linalg.norm(x[:, 9:12] - xRef[:, 0, 9:12], dim=1).cpu().numpy())
    u, traj, status = lti.solve(x, xRef=xRef, warm_start="shift" if i else False, **opts)
    x = mpcUtils.modelStep(model, x, u + torch.as_tensor(uTrim, **dev))

# ---- real-time iteration, written out: linearise about the shifted previous plan, solve, step the nonlinear model
x = torch.zeros((Bn, 12), **dev)
plan = pytrees.Trajectory(torch.zeros((Bn, N + 1, 12), **dev), uRef.clone())       # the first expansion: hover at the start
prob = mpcUtils.ltvMpc.fromModel(model, plan, Q, R, -x_ub, x_ub, uTrim - u_ub, uTrim + u_ub)
err_ltv, iters, xs, us = [], [], [], []
for i in range(steps):
    x = torch.minimum(torch.maximum(x, lo), hi)
    xs.append(x)
    prob.relinearize(model, plan)                                                  # A_k, B_k, c_k on the device, no host copy
    xRef = torch.as_tensor(window(i), **dev)
    err_ltv.append(torch.linalg.norm(x[:, 9:12] - xRef[:, 0, 9:12], dim=1).cpu().numpy())
    u, traj, status = prob.solve(x, xRef=xRef, uRef=uRef, warm_start="shift" if i else False, **opts)
    us.append(u)
    iters.append(int(prob.last_iterations.max()))
    if i % 10 == 0 or i == steps - 1:
        print(f"step {i:2d}: position error  ltvMpc mean {err_ltv[-1].mean():.3f} max {err_ltv[-1].max():.3f} m   |   trim-linearised lqrMpc "
              f"mean {err_lti[i].mean():.3f} max {err_lti[i].max():.3f} m;  {iters[-1]} ADMM iterations, "
              f"{int(np.sum(status == 'optimal'))}/{Bn} optimal")
    x = mpcUtils.modelStep(model, x, u)
    # the next expansion point: the plan moved on by one step, its last stage repeated
    plan = pytrees.Trajectory(torch.cat([traj.xTraj[:, 1:], traj.xTraj[:, -1:]], dim=1), torch.cat([traj.uTraj[:, 1:], traj.uTraj[:, -1:]], dim=1))
xs.append(torch.minimum(torch.maximum(x, lo), hi))

# ---- the same loop as one call: nothing but kernel launches between the first state and the last
prob1 = mpcUtils.ltvMpc.fromModel(model, pytrees.Trajectory(torch.zeros((Bn, N + 1, 12), **dev), uRef.clone()), Q, R, -x_ub, x_ub,
                                  uTrim - u_ub, uTrim + u_ub)
run = prob1.realTimeIteration(model, torch.zeros((Bn, 12), **dev), steps, xRef=reference(steps + N),
                              uRef=np.tile(uTrim, (Bn, steps + N - 1, 1)), **opts)
same = torch.equal(run.xTraj, torch.stack(xs, dim=1)) and torch.equal(run.uTraj, torch.stack(us, dim=1))
print(f"realTimeIteration against the loop of relinearize / solve / modelStep: states and inputs {'agree bit for bit' if same else 'DIFFER'}; "
      f"largest difference {float((run.xTraj - torch.stack(xs, dim=1)).abs().max()):.3g}")

tail = slice(steps // 2, None)
print(f"position error over the second half of the run: ltvMpc mean {np.mean(err_ltv[tail]):.4f} m, "
      f"trim-linearised lqrMpc mean {np.mean(err_lti[tail]):.4f} m")
