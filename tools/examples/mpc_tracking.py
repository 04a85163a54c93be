"""Receding-horizon MPC about a moving reference: 64 quadcopters (the linearisation and bounds of the reference's demos/lqrMpc.py) each
follow a position ramp; at every step the caller moves the reference window, the solve starts from the shifted iterates of the previous
one, and the vehicle takes the first planned step ("assume perfect tracking", demos/lqrMpc.py:47).  First the loop written out by hand
over `solve`, then the same run as one call, `simulate`, which takes the whole reference (steps + N rows) and moves the window itself."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from zopt_amd import models, mpcUtils, pytrees  # noqa: E402

dt, N, steps, Bn = 0.1, 30, 50, 64
lin = pytrees.AffineDynamics.from_function(models.QuadcopterEuler(dt), np.zeros(12), models.QuadcopterEuler.uTrim)
A, B = np.asarray(lin.f_x), np.asarray(lin.f_u)
x_ub = np.array([1, 1, 1, 0.3, 0.3, 0.1, 0.5, 0.5, np.inf, np.inf, np.inf, np.inf])
u_ub = np.array([3.0, 3, 3, 3])
prob = mpcUtils.lqrMpc(A, B, np.eye(12), np.eye(4), N, -x_ub, x_ub, -u_ub, u_ub)

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


opts = dict(eps_abs=1e-2, eps_rel=1e-2, max_iter=4000)

# by hand: a launch and its round trips per step
x = np.zeros((Bn, 12))
xs = []
for i in range(steps):
    x = np.clip(x, -x_ub + 1e-6, x_ub - 1e-6)
    xRef = window(i)
    xs.append(x)
    u, traj, status = prob.solve(x, xRef=xRef, warm_start="shift" if i else False, **opts)
    err = np.linalg.norm(x[:, 9:12] - xRef[:, 0, 9:12], axis=1)
    if i % 10 == 0 or i == steps - 1:
        print(f"step {i:2d}: position error mean {err.mean():.3f} max {err.max():.3f} m, {int(prob.last_iterations.max())} ADMM iterations, "
              f"{int(np.sum(status == 'optimal'))}/{Bn} optimal")
    x = traj.xTraj[:, 1]
xs.append(np.clip(x, -x_ub + 1e-6, x_ub - 1e-6))

# the same run as one call on the device: the reference of the whole run, row s + k = row k of step s's window
t = dt * np.arange(steps + N)
xRefAll = np.zeros((Bn, steps + N, 12))
xRefAll[:, :, 9:12] = p0[:, None, :] + vel[:, None, :] * t[None, :, None]
xRefAll[:, :, 0:3] = vel[:, None, :]
run = mpcUtils.lqrMpc(A, B, np.eye(12), np.eye(4), N, -x_ub, x_ub, -u_ub, u_ub).simulate(
    np.zeros((Bn, 12)), steps, xRef=xRefAll, clip_tol=1e-6, warm_start="shift", **opts)
err = np.linalg.norm(run.xTraj[:, -1, 9:12] - xRefAll[:, steps, 9:12], axis=1)
print(f"simulate: {steps} steps in one call, final position error mean {err.mean():.3f} max {err.max():.3f} m, "
      f"{int(np.sum(run.status == 'optimal'))}/{run.status.size} solves optimal, up to {int(run.iterations.max())} ADMM iterations; "
      f"largest difference from the hand-written loop's states {np.max(np.abs(run.xTraj - np.stack(xs, axis=1))):.1e}")
