"""The non-quadratic solve cases of models.TracedCost, shared by tests/test_traced_cost.py (which decides on the CPU that every start is
a fair comparison) and tests/test_traced_cost_gpu.py (which then excludes nothing).

A case: dynamics (a NumPy callable, or a registered model with its NumPy twin), cost callables written once for NumPy recording scalars
and torch tensors alike, parameter rows, starts, horizon, maxIter, tol.  The starts were chosen so that for each of them the NumPy
restatement (tests/traced_cost_ref.py) alone converges within maxIter, its two best line-search costs differ by more than
model_hp_ref.DETERMINED (relative) in every iteration, and a PD projection changes a Hessian somewhere in the set
(test_traced_cost.py::test_solve_cases_are_decided asserts all three).
"""
from typing import NamedTuple

import numpy as np

from oracle import zopt_oracle as zo


def _fn(x, name):
    """np.<name> or torch.<name> by the argument's type (the generic torch path runs the same callables)"""
    try:
        import torch
        if isinstance(x, torch.Tensor):
            return getattr(torch, name)
    except ImportError:                                  # pragma: no cover
        pass
    return getattr(np, name)


# ---- pendulum, 1 - cos(theta): the Hessian cos(theta) is negative beyond a quarter turn ----------------------------------------------
def pendulum_running(x, u):
    return 10.0 * (1.0 - _fn(x[0], "cos")(x[0])) + 0.5 * x[1] * x[1] + 0.1 * u[0] * u[0]


def pendulum_terminal(x):
    return 100.0 * (1.0 - _fn(x[0], "cos")(x[0])) + 10.0 * x[1] * x[1]


def pendulum_any(x, u):
    """a pendulum with a long Euler step (dt = 0.2: seven steps swing it through a large angle), for NumPy and torch alike"""
    import torch
    th, om = x[0], x[1]
    a, b = th + 0.2 * om, om + 0.2 * (u[0] - 9.81 * _fn(th, "sin")(th))
    return torch.stack([a, b]) if isinstance(x, torch.Tensor) else np.array([a, b])


# ---- car to a goal per vehicle past an obstacle: p = [goal x, goal y, centre x, centre y] ---------------------------------------------
def car_running(x, u, p):
    dx, dy, ox, oy = x[0] - p[0], x[1] - p[1], x[0] - p[2], x[1] - p[3]
    return 0.5 * (dx * dx + dy * dy) + 0.05 * x[3] * x[3] + 0.2 * u[0] * u[0] + 0.1 * u[1] * u[1] + 4.0 / (ox * ox + oy * oy + 0.5)


def car_terminal(x, p):
    dx, dy = x[0] - p[0], x[1] - p[1]
    return 20.0 * (dx * dx + dy * dy) + 2.0 * x[3] * x[3]


def car_any(x, u):
    import torch
    px, py, th, v = x[0], x[1], x[2], x[3]
    out = [px + 0.1 * v * _fn(th, "cos")(th), py + 0.1 * v * _fn(th, "sin")(th), th + 0.1 * v * _fn(u[0], "tan")(u[0]) / 2.5,
           v + 0.1 * u[1]]
    return torch.stack(out) if isinstance(x, torch.Tensor) else np.array(out)


# ---- quadcopter to the origin under a soft speed limit: a smooth hinge on |uvw|^2 - vmax^2 ---------------------------------------------
VMAX2 = 1.0


def quad_running(x, u):
    pos = x[9] * x[9] + x[10] * x[10] + x[11] * x[11]
    att = x[3] * x[3] + x[4] * x[4] + x[5] * x[5] + x[6] * x[6] + x[7] * x[7] + x[8] * x[8]
    over = x[0] * x[0] + x[1] * x[1] + x[2] * x[2] - VMAX2
    du = u[0] - 9.807
    return pos + att + 0.2 * (du * du + u[1] * u[1] + u[2] * u[2] + u[3] * u[3]) + 2.0 * (np.sqrt(over * over + 0.25) + over)


def quad_terminal(x):
    pos = x[9] * x[9] + x[10] * x[10] + x[11] * x[11]
    rest = x[0] * x[0] + x[1] * x[1] + x[2] * x[2] + x[3] * x[3] + x[4] * x[4] + x[5] * x[5] + x[6] * x[6] + x[7] * x[7] + x[8] * x[8]
    return 10.0 * pos + 10.0 * rest


class Case(NamedTuple):
    name: str
    n: int
    m: int
    step: object            # NumPy callable x+ = f(x, u)
    running: object
    terminal: object
    params: object          # (b, np) or None
    x0: np.ndarray          # (b, n)
    uGuess: np.ndarray      # (b, N, m)
    maxIter: int
    tol: float
    torch_twin: bool        # the callables also run on torch tensors (the generic path's comparison)

    def model(self, models, traced=True):
        """the device model: a TracedModel of `step`, or (traced=False) the registered quadcopter"""
        if self.name == "quadcopter" and not traced:
            return models.QuadcopterEuler(0.1)
        return models.TracedModel(self.step, self.n, self.m)

    def cost(self, models, rows=slice(None)):
        p = None if self.params is None else self.params[rows]
        return models.TracedCost(self.running, self.terminal, self.n, self.m, params=p)


def cases():
    N, tol = 7, 1.0        # (tol: the loop stops while its line search still has a clear winner -- see the module docstring)
    pend = Case("pendulum", 2, 1, pendulum_any, pendulum_running, pendulum_terminal, None,
                np.array([[-2.676, -0.7], [2.386, 2.065], [1.837, -1.101]]), np.zeros((3, N, 1)), 20, tol, True)
    goals = np.array([[1.245, -2.993, 0.625, -1.534], [1.105, -0.217, 0.386, -0.024], [2.186, -1.328, 1.061, -0.93]])
    car = Case("car", 4, 2, car_any, car_running, car_terminal, goals,
               np.array([[0.0, 0.0, 2.233, 0.546], [0.0, 0.0, 1.449, 2.186], [0.0, 0.0, 0.319, 0.766]]), np.zeros((3, N, 2)), 20, tol, True)
    x0q = np.zeros((3, 12))
    x0q[:, 0:3] = [[1.712, 1.559, -0.078], [1.296, -1.077, 1.484], [-1.23, 0.712, 0.007]]
    x0q[:, 6:8] = [[-0.045, 0.167], [0.005, 0.225], [0.049, -0.047]]
    x0q[:, 9:12] = [[-2.984, -1.829, -0.95], [-0.746, 1.241, -0.95], [1.138, -1.504, -2.607]]
    quad = Case("quadcopter", 12, 4, zo.quad_euler_step(0.1), quad_running, quad_terminal, None, x0q,
                np.tile(np.array([9.807, 0.0, 0.0, 0.0]), (3, N, 1)), 20, tol, False)
    return [pend, car, quad]


def by_name(name):
    return {c.name: c for c in cases()}[name]
