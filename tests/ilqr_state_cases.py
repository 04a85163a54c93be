"""The cases of the state-box tests (tests/test_ilqr_state.py on the CPU, tests/test_ilqr_state_gpu.py on the device), computed once
per process.  The convex ones (a LinearModel with a quadratic cost: the problem is a QP) are the ones held to SciPy on the CPU; every
solve case carries the restatement's result and trace, whose hygiene the CPU file asserts so that the GPU file may demand exact
agreement of the discrete quantities (step indices, iteration counts, done flags)."""
import functools

import numpy as np

from oracle import zopt_oracle as zo
from tests import hp_reference as hp
from tests import ilqr_box_cases as bcases
from tests import ilqr_box_ref as br
from tests import ilqr_state_ref as sref
from tests import ilqr_tracking_ref as tref

INF = np.inf


def _double_integrator():
    dt = 0.2
    A = np.array([[1.0, dt], [0.0, 1.0]])
    B = np.array([[0.5 * dt * dt], [dt]])
    return dict(A=A, B=B, Q=np.diag([1.0, 0.1]), R=np.array([[0.1]]), Qf=10.0 * np.eye(2), T=20, x0=np.array([-3.0, 0.0]),
                x_lb=np.array([-INF, -INF]), x_ub=np.array([INF, 0.7]), u_lb=np.array([-1.5]), u_ub=np.array([1.5]))


def _random_system(n, m, T, rho, seed):
    """a random system of spectral radius rho with two-sided walls on every third state and input bounds, feasible by construction:
    z = 1/4 of the unconstrained optimum + 3/4 of the optimum under a 30 times heavier state weight is a trajectory from x0 (the
    dynamics are linear); the bounds are 1.02 of z's largest excursions, so z is strictly inside"""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, n))
    A *= rho / np.max(np.abs(np.linalg.eigvals(A)))
    B = rng.standard_normal((n, m)) / np.sqrt(n)
    Q, R, Qf = np.eye(n), 0.1 * np.eye(m), 5.0 * np.eye(n)
    x0 = rng.standard_normal(n)
    solve = lambda w: tref.iterativeLqr(lambda x, u: A @ x + B @ u, w * Q, R, w * Qf, np.zeros((T + 1, n)), np.zeros((T, m)), x0,   # noqa: E731
                                        np.zeros((T, m)), maxIter=50, tol=1e-12)[0]
    free, heavy = solve(1.0), solve(30.0)
    zx, zu = 0.25 * free.xTraj + 0.75 * heavy.xTraj, 0.25 * free.uTraj + 0.75 * heavy.uTraj
    x_lb, x_ub = np.full(n, -INF), np.full(n, INF)
    for i in range(0, n, 3):
        w = 1.02 * np.max(np.abs(zx[1:, i]))
        x_lb[i], x_ub[i] = -w, w
    ubnd = 1.02 * np.max(np.abs(zu), axis=0)
    return dict(A=A, B=B, Q=Q, R=R, Qf=Qf, T=T, x0=x0, x_lb=x_lb, x_ub=x_ub, u_lb=-ubnd, u_ub=ubnd)


QP_NAMES = ("dint", "stable5", "unstable5", "stable12", "unstable12")


@functools.lru_cache(maxsize=None)
def qp_problem(name):
    if name == "dint":
        return _double_integrator()
    n, m, T = (5, 2, 12) if name.endswith("5") else (12, 4, 8)
    return _random_system(n, m, T, 0.9 if name.startswith("stable") else 1.1, {"stable5": 11, "unstable5": 12, "stable12": 21,
                                                                                  "unstable12": 14}[name])


TIGHT = dict(tol=1e-10, ctol=1e-8, outer=20, maxIter=100)       # the settings of the comparison with SciPy
LOOSE = dict(tol=1e-3, ctol=1e-4, outer=10, maxIter=100)        # the defaults: the settings of the GPU solve cases


@functools.lru_cache(maxsize=None)
def qp_restatement(name, boxed, tight):
    """the restatement's result and trace on a QP case"""
    p = qp_problem(name)
    kw = dict(TIGHT if tight else LOOSE)
    trace = []
    out = sref.constrainedIterativeLqr(lambda x, u: p["A"] @ x + p["B"] @ u, p["Q"], p["R"], p["Qf"], p["x0"], np.zeros((p["T"], p["B"].shape[1])),
                                       p["x_lb"], p["x_ub"], u_lb=p["u_lb"] if boxed else None, u_ub=p["u_ub"] if boxed else None,
                                       trace=trace, **kw)
    out["trace"] = trace
    return out


def condensed(p):
    """x_{1..T} = Sx x0 + Su u (stacked), the cost's Hessian and gradient in u (no 1/2: J = u'Hu + 2 f'u + const)"""
    A, B, T = p["A"], p["B"], p["T"]
    n, m = B.shape
    Sx = np.zeros((T * n, n))
    Su = np.zeros((T * n, T * m))
    Ak = np.eye(n)
    for k in range(T):
        Ak = A @ Ak
        Sx[k * n:(k + 1) * n] = Ak
        for j in range(k + 1):
            Su[k * n:(k + 1) * n, j * m:(j + 1) * m] = np.linalg.matrix_power(A, k - j) @ B
    Qb = np.kron(np.eye(T), p["Q"])
    Qb[-n:, -n:] = p["Qf"]
    Rb = np.kron(np.eye(T), p["R"])
    H = Su.T @ Qb @ Su + Rb
    f = Su.T @ Qb @ (Sx @ p["x0"])
    return Sx, Su, H, f


@functools.lru_cache(maxsize=None)
def qp_scipy(name, boxed):
    """SciPy's solution of the condensed QP (SLSQP from the restatement-independent start u = 0): (uTraj (T, m), xTraj rows 1..T)"""
    from scipy.optimize import minimize
    p = qp_problem(name)
    n, m = p["B"].shape
    T = p["T"]
    Sx, Su, H, f = condensed(p)
    c0 = Sx @ p["x0"]
    lb, ub = np.tile(p["x_lb"], T), np.tile(p["x_ub"], T)
    rows_u, rows_l = np.isfinite(ub), np.isfinite(lb)
    G = np.vstack([-Su[rows_u], Su[rows_l]])                      # G u + d >= 0
    d = np.concatenate([ub[rows_u] - c0[rows_u], c0[rows_l] - lb[rows_l]])
    cons = [dict(type="ineq", fun=lambda u: G @ u + d, jac=lambda u: G)]
    bounds = list(zip(np.tile(p["u_lb"], T), np.tile(p["u_ub"], T))) if boxed else None
    for ftol in (1e-14, 1e-12, 1e-10):       # (SLSQP gives up on its own line search when asked for more than it can resolve)
        res = minimize(lambda u: u @ H @ u + 2 * f @ u, np.zeros(T * m), jac=lambda u: 2 * (H @ u + f), method="SLSQP", bounds=bounds,
                       constraints=cons, options=dict(ftol=ftol, maxiter=2000))
        if res.success:
            break
    assert res.success, res.message
    return res.x.reshape(T, m), (c0 + Su @ res.x).reshape(T, n)


# ---------------------------------------------------------------------------------------------------------------- solve cases (GPU)
# every solve case of tests/test_ilqr_state_gpu.py: name -> (QP case, with input bounds)
SOLVE_CASES = tuple((name, boxed) for name in QP_NAMES for boxed in (False, True))


def margins(out, x_lb, x_ub, tol, ctol):
    """the margins of a restatement run that decide whether a device run may be compared exactly: (the smallest relative gap between
    the best and the second-best of the 16 costs, the smallest |s| / (1 + mu) over finite bounds, the smallest distance of the inner
    test |dJ| - tol and of the outer test viol - ctol from zero, relative to tol and ctol)"""
    gap, smin, test = np.inf, np.inf, np.inf
    fin_u, fin_l = np.isfinite(x_ub), np.isfinite(x_lb)
    for o in out["trace"]:
        for it in o["inner"]:
            Js = np.sort(it["Js"])
            gap = min(gap, (Js[1] - Js[0]) / max(abs(Js[0]), 1e-300))
            s = np.concatenate([np.abs(it["su"][:, fin_u]).ravel(), np.abs(it["sl"][:, fin_l]).ravel()])
            if s.size:
                smin = min(smin, float(s.min()) / (1.0 + o["mu"]))
            test = min(test, abs(it["dJ"] - tol) / tol)
        test = min(test, abs(o["violation"] - ctol) / ctol)
    return gap, smin, test


# ------------------------------------------------------------------------------------------------------- quadcopter solve cases (GPU)
QUAD_T, QUAD_DT, QUAD_B = 20, 0.1, 3
QUAD_UTRIM = np.array([9.807, 0.0, 0.0, 0.0])            # models.QuadcopterEuler.uTrim
QUAD_SEED = 4
QUAD_KW = dict(tol=1e-3, maxIter=100, outer=10, ctol=1e-3, mu0=10.0)


@functools.lru_cache(maxsize=None)
def quad_case():
    """QuadcopterEuler (dt = 0.1, T = 20), a TrackingCost about hover with a goal per trajectory (positions are states 9..11, z points
    down), an altitude floor (z <= 0.4: no sinking more than 0.4 m below the start) and a cap of 0.4 m/s on the body velocities;
    the input box of the boxed twin: thrust within hover +- 1.5, moments within +- 0.05.  Trajectory 2's goal is 0.4 m away.
    Settings QUAD_KW: mu0 = 10 and ctol = 1e-3.  With the defaults (mu0 = 1, ctol = 1e-4) the loop runs two more outer iterations,
    whose inner solves start within 1e-5 of their optimum: their second iteration moves J by less than 1e-9 relative and the best
    two of its 16 costs are 1e-11 apart, which the hygiene rule (1e-9) forbids; these settings end the loop before that."""
    rng = np.random.default_rng(QUAD_SEED)
    n, m = 12, 4
    goals = np.zeros((QUAD_B, 1, n))
    goals[:, 0, 9:12] = rng.uniform(-2.0, 2.0, (QUAD_B, 3))
    goals[0, 0, 11] = 1.2                                  # below the floor: the floor is active at the end
    goals[2, 0, 9:12] = [0.3, -0.2, 0.1]
    x_lb, x_ub = np.full(n, -INF), np.full(n, INF)
    x_ub[11] = 0.4
    x_lb[0:3], x_ub[0:3] = -0.4, 0.4
    lim = np.array([1.5, 0.05, 0.05, 0.05])
    return dict(Q=np.eye(n), R=np.eye(m), Qf=10.0 * np.eye(n), goals=goals, x0=np.zeros((QUAD_B, n)), ug=np.tile(QUAD_UTRIM, (QUAD_B, QUAD_T, 1)),
                x_lb=x_lb, x_ub=x_ub, u_lb=QUAD_UTRIM - lim, u_ub=QUAD_UTRIM + lim)


@functools.lru_cache(maxsize=None)
def quad_restatement(boxed, b):
    """the restatement's result and trace on trajectory b of the quadcopter case (QUAD_KW)"""
    import warnings
    c = quad_case()
    xr, ur = np.tile(c["goals"][b], (QUAD_T + 1, 1)), np.tile(QUAD_UTRIM, (QUAD_T, 1))
    trace = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = sref.constrainedIterativeLqr(zo.quad_euler_step(QUAD_DT), c["Q"], c["R"], c["Qf"], c["x0"][b], c["ug"][b], c["x_lb"], c["x_ub"],
                                           u_lb=c["u_lb"] if boxed else None, u_ub=c["u_ub"] if boxed else None, xr=xr, ur=ur, trace=trace, **QUAD_KW)
    out["trace"] = trace
    return out


# ------------------------------------------------------------------------------------------------------------- sweep cases (GPU)
# the box tests' hard families and shapes (tests/ilqr_box_cases.py) with a diagonal addend h (batch, T+1, n), entries 0 .. 1e8
SWEEP_FAMILIES, SWEEP_SHAPES = bcases.SWEEP_FAMILIES, bcases.SWEEP_SHAPES


def materialised(cost, Vf, h):
    """(cost, Vf) with the per-step Hessians c_xx + diag h_k and the terminal v_xx + diag h_T"""
    c_xx, v_xx = np.asarray(cost[3]), np.asarray(Vf[2])
    T, n = c_xx.shape[1], c_xx.shape[-1]
    eye = np.eye(n)
    return tuple(cost[:3]) + (c_xx + h[:, :T, :, None] * eye,) + tuple(cost[4:]), tuple(Vf[:2]) + (v_xx + h[:, T, :, None] * eye,)


def _addend(seed, B, T, n, zeros=1 / 3):
    """entries 0 (a share `zeros` of them) or 10^U(-3, 8)"""
    rng = np.random.default_rng(seed)
    h = np.where(rng.random((B, T + 1, n)) < zeros, 0.0, 10.0 ** rng.uniform(-3, 8, (B, T + 1, n)))
    h[:, 0] = 0.0
    return h


@functools.lru_cache(maxsize=None)
def sweep_case(family, n, m, T, batch, per_traj):
    """the box sweep case of that family and shape with an addend h: dict(args = (dyn, cost, Vf, uTraj, lb, ub) as the box case has
    them, h, mat = (cost, Vf) materialised, ref = the long-double box sweep on them (l, L, clamped, margin), e_l, e_L = the fp64
    restatement's error, seed).  The addend's seed is the first of 0..399 at which every step of the reference keeps the
    strict-complementarity margin bcases.MARGIN and the fp64 restatement finds the same clamped sets."""
    args = bcases.sweep_case(family, n, m, T, batch, per_traj)["args"]
    dyn, cost, Vf, u, lb, ub = args
    for seed in range(400):      # (a quarter of the tries each with 1/3, 2/3, 0.9 and 0.97 of the entries zero)
        h = _addend(1000 * seed + 17 * n + T, batch, T, n, (1 / 3, 2 / 3, 0.9, 0.97)[seed // 100])
        costm, Vfm = materialised(cost, Vf, h)
        ref = br.box_backward_batch(dyn, costm, Vfm, u, lb, ub, ld=True)
        if float(np.min(ref["margin"])) < bcases.MARGIN:
            continue
        o = br.box_backward_batch(dyn, costm, Vfm, u, lb, ub)
        if not np.array_equal(o["clamped"], ref["clamped"]):
            continue
        return {"args": args, "h": h, "mat": (costm, Vfm), "ref": ref, "seed": seed, "e_l": float(hp.sweep_metric(o["l"], ref["l"]).max()),
                "e_L": float(hp.sweep_metric(o["L"], ref["L"]).max())}
    raise AssertionError(f"no addend seed keeps the margin for {family} {(n, m, T, batch, per_traj)}")


def sweep_bounds(family, n, m, T, batch, per_traj):
    """(bound on l, bound on L): hp.sweep_bounds from the restatement's error on the case and on the plain family with its addend"""
    c, p = sweep_case(family, n, m, T, batch, per_traj), sweep_case("plain", n, m, T, batch, per_traj)
    return hp.sweep_bounds(c["e_l"], p["e_l"]), hp.sweep_bounds(c["e_L"], p["e_L"])
