"""A gust through a receding-horizon run, with hard and with soft position bounds.  16 quadcopters (the linearisation and bounds of the
reference's demos/lqrMpc.py, and a position box of +-2 m) hold station near the east wall of the box; at step 3 a gust shoves each of them
0.8 m further east, most of them through the wall.  `lqrMpc.simulate` runs the whole loop on the device in one call.

  hard walls, clip_tol = None : the state outside the box is "infeasible": those vehicle-steps are lost
  hard walls, clip_tol = 1e-6 : the demo's clip puts the state back on the wall before it is solved from -- every step is "optimal", but the
                                run that comes back is not the run the plant made (the vehicle was teleported)
  soft walls (`soften`)       : the position bounds pay l1 = 20 per metre outside instead of holding (the velocity and attitude bounds 200:
                                stiff, but a vehicle that returns at the velocity bound and overshoots it by a solver tolerance is not
                                lost either); the state is never moved, and the vehicles fly back inside."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from zopt_amd import models, mpcUtils, pytrees  # noqa: E402

dt, N, steps, Bn, gust_step, wall = 0.1, 30, 40, 16, 3, 2.0
lin = pytrees.AffineDynamics.from_function(models.QuadcopterEuler(dt), np.zeros(12), models.QuadcopterEuler.uTrim)
A, B = np.asarray(lin.f_x), np.asarray(lin.f_u)
x_ub = np.array([1, 1, 1, 0.3, 0.3, 0.1, 0.5, 0.5, np.inf, wall, wall, wall])     # states 9..11: the position
u_ub = np.array([3.0, 3, 3, 3])
build = lambda: mpcUtils.lqrMpc(A, B, np.eye(12), np.eye(4), N, -x_ub, x_ub, -u_ub, u_ub)

rng = np.random.default_rng(0)
x0 = np.zeros((Bn, 12))
x0[:, 9] = rng.uniform(1.2, 1.9, Bn)                                  # east of the origin, up to 0.1 m from the wall
x0[:, 10:12] = rng.uniform(-1.0, 1.0, (Bn, 2))
w = np.zeros((Bn, steps, 12))
w[:, gust_step, 9] = 0.8
opts = dict(eps_abs=1e-3, eps_rel=1e-3, max_iter=4000)


def report(name, run):
    status = np.asarray(run.status).astype(str)
    print(name)
    for s in (0, gust_step, gust_step + 1, gust_step + 2, gust_step + 5, gust_step + 10, steps - 1):
        kinds, counts = np.unique(status[:, s], return_counts=True)
        east = np.asarray(run.xTraj)[:, s, 9]
        print(f"  step {s:2d}: " + ", ".join(f"{c} {k}" for k, c in zip(kinds, counts)) + f"; easternmost vehicle {east.max() - wall:+.3f} m "
              f"from the wall; up to {int(np.asarray(run.iterations)[:, s].max())} ADMM iterations")
    return status


l1 = np.where(np.isfinite(x_ub), 200.0, np.inf)
l1[9:12] = 20.0
lost = report("hard walls, clip_tol = None:", build().simulate(x0, steps, disturbance=w, clip_tol=None, **opts))
print(f"  {steps} steps x {Bn} vehicles: {int(np.sum(lost != 'optimal'))} vehicle-steps not \"optimal\" "
      f"({int(np.sum(lost == 'infeasible'))} \"infeasible\")")

clipped = build().simulate(x0, steps, disturbance=w, return_predictions=True, **opts)
status = report("hard walls, clip_tol = 1e-6:", clipped)
plant = np.asarray(clipped.predictions.xTraj)[:, :, 1] + w            # where the plant went; xTraj[s + 1] is where the run says it is
moved = np.abs(plant - np.asarray(clipped.xTraj)[:, 1:]).max(axis=-1) > 1e-5
print(f"  {steps} steps x {Bn} vehicles: {int(np.sum(status != 'optimal'))} vehicle-steps not \"optimal\", {int(moved.sum())} vehicle-steps "
      f"teleported by the clip, by up to {np.abs(plant - np.asarray(clipped.xTraj)[:, 1:]).max():.3f} m")

soft = build().soften(x_soft_l1=l1).simulate(x0, steps, disturbance=w, **opts)
status = report("soft walls (x_soft_l1 = 20 on the position, 200 on the other bounded states):", soft)
excess = (np.abs(np.asarray(soft.xTraj)[:, :, 9:12]) - wall).max(axis=(0, 2))      # per step: the vehicle furthest outside
outside = np.flatnonzero(excess > 1e-3)
kinds, counts = np.unique(status[status != "optimal"], return_counts=True)
print(f"  {steps} steps x {Bn} vehicles: {int(np.sum(status != 'optimal'))} vehicle-steps not \"optimal\""
      + (" (" + ", ".join(f"{c} {k}" for k, c in zip(kinds, counts)) + ")" if kinds.size else "") + f"; the run leaves the box by up to "
      f"{max(excess.max(), 0.0):.3f} m" + (f" (steps {outside[0]} to {outside[-1]}) and every vehicle is back inside from step "
                                            f"{outside[-1] + 1} on" if outside.size else ""))
