"""CPU restatement and cases for ltvMpc.realTimeIteration (zm_mpc_rti_f64); a helper module, not collected as a test.

`run` is the loop the one call replaces, for ONE instance, in NumPy:

    plan given;  x = x0
    for s in range(steps):
        x = clip(x);  states[s] = x
        A_k, B_k, c_k <- the model expanded about the plan            (oracle.zopt_oracle.affine_dynamics_from_trajectory: complex step)
        solve from x, tracking window s of the references             (tests/mpc_ltv_ref.py: admm_levels_ltv, tests/mpc_tracking_ref.py: linear_term)
        x = plant(x, u_0) + disturbance[s]                            (the step function itself, e.g. oracle.zopt_oracle.quad_euler_step)
        plan = rollout rows 1.., the last repeated
    states[steps] = clip(x)

A model is its step function (x, u) -> x+, written so that complex arguments pass (the oracle differentiates by the complex step).
The cases of tests/test_mpc_rti_gpu.py that are compared with this restatement are built here; their decisions are checked, without a GPU,
in tests/test_mpc_rti.py."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

from oracle import zopt_oracle as zo
from tests import mpc_ltv_ref as lr
from tests import mpc_tracking_ref as tr

QUAD_UTRIM = lr.QUAD_UTRIM


def quad_step(dt, wind_ned=(0.0, 0.0, 0.0)):
    if not np.any(wind_ned):
        return zo.quad_euler_step(dt)
    w = np.asarray(wind_ned, dtype=np.float64)
    return lambda x, u: x + dt * zo.quad_inertialDynamics(x, u, wind_ned=w)


def rigid_body_step(dt):
    return lambda x, u: x + dt * zo.quad_rigidBodyDynamics(x, u)


def linear_step(A, B):
    return lambda x, u: A @ x + B @ u


def expansion(step, xPlan, uPlan, perturb=0.0, rng=None):
    """A_k = f_x, B_k = f_u, c_k = f - f_x xbar_k - f_u ubar_k about the plan; perturb: every entry of f, f_x, f_u scaled by
    1 + perturb * (+-1) first (the decision-margin check)"""
    f, f_x, f_u = (np.asarray(v) for v in zo.affine_dynamics_from_trajectory(step, zo.Trajectory(xPlan, uPlan)))
    if perturb:
        f, f_x, f_u = (v * (1.0 + perturb * rng.choice([-1.0, 1.0], v.shape)) for v in (f, f_x, f_u))
    c = f - np.einsum("kij,kj->ki", f_x, xPlan[:-1]) - np.einsum("kij,kj->ki", f_u, uPlan)
    return f_x, f_u, c, f


def shift(x, u):
    return np.vstack([x[1:], x[-1:]]), np.vstack([u[1:], u[-1:]])


def run(step, data, N, x0, plan, steps, plant=None, xRef=None, uRef=None, disturbance=None, clip_tol=1e-6, warm="shift", rho=None,
        perturb=0.0, solve=lr.admm_levels_ltv, **kw):
    """One instance.  data = (Q, R, Qf, x_lb, x_ub, u_lb, u_ub); plan = (xPlan (N+1, n), uPlan (N, m)); xRef (steps + N, n), uRef
    (steps + N - 1, m) or None; kw: the options of admm_levels_ltv.  -> namespace(states (S+1, n), inputs (S, m), status, iters, level
    (S,), px (S, N+1, n), pu (S, N, m), results: the solves' own namespaces)"""
    Q, R, Qf, xl, xu, ul, uu = data
    n, m = Q.shape[0], R.shape[0]
    plant = plant or step
    rho = tr.default_rho(Q, R) if rho is None else rho
    rng = np.random.default_rng(12345)
    clip = (lambda v: v) if clip_tol is None else (lambda v: np.clip(v, xl + clip_tol, xu - clip_tol))
    x, (xP, uP) = np.asarray(x0, dtype=np.float64), plan
    out = SimpleNamespace(states=[], inputs=[], status=[], iters=[], level=[], px=[], pu=[], results=[])
    prev = None
    for s in range(steps):
        x = clip(x)
        out.states.append(x)
        A, B, c, _ = expansion(step, xP, uP, perturb, rng)
        g = None
        if xRef is not None or uRef is not None:
            xr = np.zeros((N + 1, n)) if xRef is None else xRef[s:s + N + 1]
            ur = np.zeros((N, m)) if uRef is None else uRef[s:s + N]
            g = tr.linear_term(Q, R, Qf, N, xr, ur)
        state = (prev.y, prev.lam, prev.level) if (s and warm and prev.status == "optimal") else None
        r = solve(A, B, c, Q, R, Qf, N, xl, xu, ul, uu, x, rho=rho, g=g, warm=state, shift=warm == "shift", **kw)
        prev = r
        out.results.append(r)
        out.inputs.append(r.u[0])
        out.status.append(r.status)
        out.iters.append(r.iters)
        out.level.append(r.level)
        out.px.append(r.x)
        out.pu.append(r.u)
        x = np.real(plant(x, r.u[0])) + (0.0 if disturbance is None else disturbance[s])
        xP, uP = shift(r.x, r.u)
    out.states.append(clip(x))
    for k in ("states", "inputs", "px", "pu"):
        setattr(out, k, np.stack(getattr(out, k)))
    out.plan = (xP, uP)
    return out


# ---- cases -------------------------------------------------------------------------------------------------------------------------------

EPS, MAX_ITER = 1e-6, 30000


def ramp(nb, rows, n, pos, vel, dt, seed):
    """a position ramp inside the velocity box: xRef (nb, rows, n) with positions `pos` on the ramp and velocities `vel` its slope"""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((nb, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    v = d * rng.uniform(0.1, 0.3, (nb, 1))
    t = dt * np.arange(rows)
    xRef = np.zeros((nb, rows, n))
    xRef[:, :, vel] = v[:, None, :]
    if pos is not None:
        xRef[:, :, pos] = 0.5 * d[:, None, :] + v[:, None, :] * t[None, :, None]
    return xRef


@functools.lru_cache(maxsize=None)
def quad_case(N=5, nb=5, S=3, seed=3):
    """QuadcopterEuler(0.1) with demos/lqrMpc.py's weights and bounds in absolute coordinates (inputs within 3 of trim), plans from
    tests/mpc_ltv_ref.py: quad_trajectories, starts next to the plans' heads, a position ramp to track with the trim input"""
    xT, uT = lr.quad_trajectories(N, nb, seed=seed)
    _, _, Q, R, Qf, xl, xu, ul, uu = tr.quad_data(N)
    x0 = xT[:, 0] + 0.02 * np.random.default_rng(5).standard_normal((nb, 12))
    xRef = ramp(nb, S + N, 12, slice(9, 12), slice(0, 3), lr.QUAD_DT, seed=8)
    xRef[:, :, 9:12] += xT[:, :1, 9:12]
    uRef = np.tile(QUAD_UTRIM, (nb, S + N - 1, 1))
    return SimpleNamespace(kind="quad", dt=lr.QUAD_DT, step=quad_step(lr.QUAD_DT), N=N, S=S, nb=nb, x0=x0, plan=(xT, uT), xRef=xRef,
                           uRef=uRef, data=(Q, R, Qf, xl, xu, QUAD_UTRIM + ul, QUAD_UTRIM + uu))


@functools.lru_cache(maxsize=None)
def rigid_body_case(N=4, nb=5, S=3, dt=0.05):
    """QuadcopterRigidBody(dt=0.05): the first eight states of the quadcopter's plans, unit weights, the demo's bounds on those states"""
    xT, uT = lr.quad_trajectories(N, nb, seed=4)
    xT = np.ascontiguousarray(xT[:, :, :8])
    _, _, _, _, _, xl, xu, ul, uu = tr.quad_data(N)
    x0 = xT[:, 0] + 0.02 * np.random.default_rng(6).standard_normal((nb, 8))
    xRef = ramp(nb, S + N, 8, None, slice(0, 3), dt, seed=9)
    uRef = np.tile(QUAD_UTRIM, (nb, S + N - 1, 1))
    return SimpleNamespace(kind="rb", dt=dt, step=rigid_body_step(dt), N=N, S=S, nb=nb, x0=x0, plan=(xT, uT), xRef=xRef, uRef=uRef,
                           data=(np.eye(8), np.eye(4), np.eye(8), xl[:8], xu[:8], QUAD_UTRIM + ul, QUAD_UTRIM + uu))


CASES = {"quad": quad_case, "rigid_body": rigid_body_case}
OPTS = dict(eps_abs=EPS, eps_rel=EPS, max_iter=MAX_ITER)


@functools.lru_cache(maxsize=None)
def reference(name, perturb=0.0):
    """[instance] -> `run` of the case, tight tolerance, shifted warm starts, adaptive penalty"""
    c = CASES[name]()
    return [run(c.step, c.data, c.N, c.x0[b], (c.plan[0][b], c.plan[1][b]), c.S, xRef=c.xRef[b], uRef=c.uRef[b], perturb=perturb, **OPTS)
            for b in range(c.nb)]
