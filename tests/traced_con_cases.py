"""The cases of the traced-constraint tests (tests/test_traced_con.py on the CPU, tests/test_traced_con_gpu.py on the device), computed
once per process.  Every solve case carries the restatement's result and trace (tests/traced_con_ref.py); the CPU file asserts the
hygiene of every iteration (the best two of the 16 costs at least 1e-9 apart, relative), so that the GPU file may demand exact
agreement of the discrete quantities without skipping a comparison.

Shapes: the smallest at which each mechanism can go wrong -- n + m = 3 (idle lanes of a 16-lane group) and n + m = 16 (every lane,
lane 15 included); T = 1 (stage 0 and the terminal row only); a point count that is no multiple of the 4 points of a wave (5 x 12);
n_con = 1 and n_con = 8; a terminal-only constraint; rows that depend on u; rows that never become active; a start inside the
obstacle (never done)."""
import functools
from typing import Callable, NamedTuple

import numpy as np

from oracle import zopt_oracle as zo
from tests import ilqr_state_cases as scases
from tests import tape_ref as R
from tests import traced_con_ref as CR
from zopt_amd import models


class Case(NamedTuple):
    name: str
    model: Callable          # () -> the device model
    dyn: Callable            # NumPy f(x, u)
    n: int
    m: int
    T: int
    Q: np.ndarray
    R: np.ndarray
    Qf: np.ndarray
    x0: np.ndarray           # (b, n)
    ug: np.ndarray           # (b, T, m)
    g: object                # stage callable or None
    n_con: int
    terminal: object
    n_con_terminal: int
    params: object           # None or (b, np)
    goals: object            # None (QuadraticCost) or (b, n): a TrackingCost about a goal per trajectory, with uRef = ug[:, 0]
    kw: dict                 # TracedConstraint's settings
    tol: float = 1e-3
    maxIter: int = 100


# ---- (2, 1) LinearModel: the double integrator of the state-box tests ------------------------------------------------------------------
DI = scases._double_integrator()
HP_A, HP_B = np.array([0.3, 1.0]), 0.7          # a half-plane that is not axis-aligned: 0.3 position + velocity <= 0.7


def halfplane(x, u):
    return np.array([HP_A[0] * x[0] + HP_A[1] * x[1] - HP_B])


def terminal_band(x):
    """the final position within 0.05 of -0.5, the final speed at most 0.1: a terminal set"""
    return np.array([x[0] + 0.45, -0.55 - x[0], x[1] - 0.1])


def terminal_speed(x):
    """the final speed at most 0.1 (active: the cost asks for more), the final position at least -3.5 (never active)"""
    return np.array([x[1] - 0.1, -3.5 - x[0]])


def _lin(name, T, g, nc, term, nct, tol=1e-3):
    """maxIter = 1: one Newton step per outer iteration.  On a linear model the penalised problem is piecewise quadratic, so a second
    inner iteration would only confirm the first with a zero step, whose 16 rollouts coincide -- the tie that the hygiene rule forbids"""
    A, B = DI["A"], DI["B"]
    return Case(name, lambda: models.LinearModel(A, B), lambda x, u: A @ x + B @ u, 2, 1, T, DI["Q"], DI["R"], DI["Qf"],
                DI["x0"][None], np.zeros((1, T, 1)), g, nc, term, nct, None, None, dict(), tol=tol, maxIter=1)


# ---- (4, 2) traced car past a disc per trajectory ---------------------------------------------------------------------------------------
CAR_T, CAR_B = 12, 5


def disc(x, u, p):
    """keep out of the disc of centre (p0, p1) and radius p2"""
    dx, dy = x[0] - p[0], x[1] - p[1]
    return np.array([p[2] * p[2] - (dx * dx + dy * dy)])


def car_eight(x, u, p):
    """the disc, a speed band, steering and acceleration limits and a corridor that is not axis-aligned: 8 rows"""
    dx, dy = x[0] - p[0], x[1] - p[1]
    return np.array([p[2] * p[2] - (dx * dx + dy * dy), x[3] - 2.5, -0.5 - x[3], u[0] - 0.3, -0.3 - u[0], u[1] - 1.0, -1.0 - u[1],
                     0.5 * x[0] - x[1] - 1.5])


def _car(name, g, nc, b, params, outer):
    n, m = 4, 2
    x0 = np.zeros((b, n))
    x0[:, 1], x0[:, 3] = 0.4, 1.0               # beside the lane (y = 0 is the goal), rolling: the solver has to steer
    ug = np.zeros((b, CAR_T, m))
    Q = np.diag([0.0, 0.5, 0.1, 0.0])           # the lane and the heading; neither the distance covered nor the speed costs
    return Case(name, lambda: models.TracedModel(R.car, n, m), R.car, n, m, CAR_T, Q, np.diag([0.5, 0.1]), np.diag([0.0, 20.0, 1.0, 0.0]), x0,
                ug, g, nc, None, 0, params, None, dict(outer=outer))


CAR_DISCS = np.array([[0.6, 0.45, 0.25],       # in the way, a little to the left
                      [0.8, 0.3, 0.3],         # in the way, a little to the right
                      [0.5, 3.0, 0.5],         # far away: never active
                      [0.1, 0.4, 0.3],         # the start is inside: never done
                      [0.9, 0.42, 0.2]])


# ---- (2, 1) traced pendulum with rows that depend on u ----------------------------------------------------------------------------------
def pendulum_mixed(x, u):
    """a torque limit that tightens with the rate, and a power limit: both mixed in (x, u)"""
    return np.array([u[0] + 0.5 * x[1] - 4.0, u[0] * x[1] - 3.0])


def _pendulum():
    n, m, T = 2, 1, 10
    return Case("pendulum", lambda: models.TracedModel(R.pendulum, n, m), R.pendulum, n, m, T, np.diag([1.0, 0.1]), np.array([[0.01]]),
                np.diag([20.0, 2.0]), np.array([[-2.0, 0.0]]), np.zeros((1, T, m)), pendulum_mixed, 2, None, 0, None, None, dict())


# ---- (12, 4) registered quadcopter past a sphere per vehicle, with a tilt limit -------------------------------------------------------------
QUAD_T, QUAD_DT, QUAD_B = 10, 0.1, 3
QUAD_UTRIM = scases.QUAD_UTRIM
TILT = np.cos(0.1)


def quad_rows(x, u, p):
    """outside the sphere of centre p[0:3] and radius p[3] (positions are states 9..11); cos(phi) cos(theta) >= cos(0.1)"""
    d = x[9:12] - p[0:3]
    return np.array([p[3] * p[3] - d @ d, TILT - np.cos(x[6]) * np.cos(x[7])])


def _quad():
    n, m = 12, 4
    goals = np.zeros((QUAD_B, n))
    goals[:, 9:12] = [[1.5, 0.0, 0.0], [1.2, 0.0, 0.0], [1.0, 0.0, 0.0]]
    spheres = np.array([[0.8, 0.1, 0.0, 0.3], [0.6, -0.08, 0.05, 0.25], [0.5, 0.05, -0.1, 0.2]])
    x0 = np.zeros((QUAD_B, n))
    x0[:, 0] = [1.5, 1.2, 1.0]                  # flying forward, the sphere ahead and a little to the side
    return Case("quadcopter", lambda: models.QuadcopterEuler(QUAD_DT), zo.quad_euler_step(QUAD_DT), n, m, QUAD_T, np.eye(n), np.eye(m),
                10.0 * np.eye(n), x0, np.tile(QUAD_UTRIM, (QUAD_B, QUAD_T, 1)), quad_rows, 2, None, 0, spheres, goals,
                dict(mu0=10.0, ctol=1e-3, outer=6))


@functools.lru_cache(maxsize=None)
def cases():
    return (_lin("lin21_T9", 9, halfplane, 1, None, 0),
            _lin("lin21_T1", 1, halfplane, 1, terminal_speed, 2, tol=2e-3),
            _lin("lin21_terminal", 9, None, 0, terminal_band, 3),
            _car("car", disc, 1, CAR_B, CAR_DISCS, 6),
            _car("car8", car_eight, 8, 2, CAR_DISCS[:2], 4),
            _pendulum(),
            _quad())


NAMES = ("lin21_T9", "lin21_T1", "lin21_terminal", "car", "car8", "pendulum", "quadcopter")


def by_name(name):
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def constraint(name):
    """the models.TracedConstraint of a case (recorded once per process)"""
    c = by_name(name)
    return models.TracedConstraint(c.model(), c.g, c.n_con, c.terminal, c.n_con_terminal, params=c.params, **c.kw)


def references(c, b):
    """(xr (T + 1, n), ur (T, m)) of trajectory b: zeros for a QuadraticCost, the goal and the first guessed input for a TrackingCost"""
    if c.goals is None:
        return np.zeros((c.T + 1, c.n)), np.zeros((c.T, c.m))
    return np.tile(c.goals[b], (c.T + 1, 1)), np.tile(c.ug[b, 0], (c.T, 1))


@functools.lru_cache(maxsize=None)
def restatement(name, b):
    """the restatement's result and trace on trajectory b of a case"""
    c = by_name(name)
    xr, ur = references(c, b)
    trace = []
    out = CR.constrainedIterativeLqr(c.dyn, c.Q, c.R, c.Qf, c.x0[b], c.ug[b], constraint(name), None if c.params is None else c.params[b],
                                     xr=xr, ur=ur, maxIter=c.maxIter, tol=c.tol, trace=trace)
    out["trace"] = trace
    return out
