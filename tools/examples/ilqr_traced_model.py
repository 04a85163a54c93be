"""iLQR and DDP on a user-written model through the fused path: `models.TracedModel` records a plain NumPy dynamics function once and
the HIP kernels interpret the recording on double, dual and hyper-dual numbers -- no registered device model, no torch.func.

Two vehicles the registered models do not cover, both NOT affine in a control (so DDP's f_ux, f_uu blocks are exercised):
  * a cart-pole (gantry crane): the swinging load is damped and the cart returned to the origin from a batch of perturbed starts (the
    force is divided by a mass that depends on the angle);
  * a kinematic car parked at the origin, 512 cars with 512 wheelbases as per-problem parameters (`params`: no derivative is taken
    with respect to them).
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from zopt_amd import ilqrUtils, models  # noqa: E402


def cartpole(x, u, dt=0.02, mc=1.0, mp=0.1, length=0.5, g=9.81):
    """state [position, angle from hanging, velocity, rate], control [force]"""
    pos, th, v, om = x
    s, c = np.sin(th), np.cos(th)
    den = mc + mp * s ** 2
    acc = (u[0] + mp * s * (length * om ** 2 + g * c)) / den
    alpha = (-u[0] * c - mp * length * om ** 2 * c * s - (mc + mp) * g * s) / (length * den)
    return np.array([pos + dt * v, th + dt * om, v + dt * acc, om + dt * alpha])


def car(x, u, p, dt=0.1):
    """state [px, py, heading, speed], control [steering angle, acceleration], parameter [wheelbase]"""
    px, py, th, v = x
    return np.array([px + dt * v * np.cos(th), py + dt * v * np.sin(th), th + dt * v * np.tan(u[0]) / p[0], v + dt * u[1]])


dev = dict(dtype=torch.float64, device="cuda")
rng = np.random.default_rng(0)

# ---- cart-pole: stop the swing and bring the cart home, 256 perturbed starts
Bn, T = 256, 100
pole = models.TracedModel(cartpole, 4, 1)
t = pole.tape
print(f"cart-pole tape: {len(t.code)} instructions, {len(t.consts)} constants, {t.n_slots} slots, not affine in variables {t.mask:#x}")
cost = models.QuadraticCost(np.diag([1.0, 10.0, 0.1, 0.1]), 0.01 * np.eye(1), 10 * np.eye(4))
x0 = torch.as_tensor(0.3 * rng.standard_normal((Bn, 4)), **dev)
uGuess = torch.zeros((Bn, T, 1), **dev)
for name, solve in (("iterativeLqr", ilqrUtils.iterativeLqr), ("differentialDynamicProgramming", ilqrUtils.differentialDynamicProgramming)):
    traj, L, J, converged = solve(pole, cost, cost, x0, uGuess)
    print(f"{name}: {int(converged.sum())}/{Bn} converged, |state| at the end of the horizon max {float(traj.xTraj[:, -1].abs().max()):.2e}, "
          f"peak force {float(traj.uTraj.abs().max()):.2f}")

# ---- car: 512 wheelbases, one solve
Bn, T = 512, 60
wheelbase = rng.uniform(2.0, 4.0, (Bn, 1))
cars = models.TracedModel(car, 4, 2, params=wheelbase)
cost = models.QuadraticCost(np.diag([1.0, 1.0, 0.5, 0.1]), np.diag([1.0, 0.1]), 50 * np.eye(4))
x0 = torch.as_tensor(np.column_stack([rng.uniform(-5, 5, Bn), rng.uniform(-2, 2, Bn), rng.uniform(-0.5, 0.5, Bn), np.ones(Bn)]), **dev)
uGuess = torch.zeros((Bn, T, 2), **dev)
for name, solve in (("iterativeLqr", ilqrUtils.iterativeLqr), ("differentialDynamicProgramming", ilqrUtils.differentialDynamicProgramming)):
    traj, L, J, converged = solve(cars, cost, cost, x0, uGuess)
    miss = torch.linalg.norm(traj.xTraj[:, -1, :2], dim=1)
    print(f"{name}: {int(converged.sum())}/{Bn} cars converged, distance to the origin at the end mean {float(miss.mean()):.3f} m, "
          f"steering within {float(traj.uTraj[:, :, 0].abs().max()):.2f} rad")
