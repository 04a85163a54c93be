"""CPU checkers and cases for mpcUtils.ltvMpc (stage-varying dynamics x+ = A_k x + B_k u + c_k); a helper module, not collected as a test.

  * `admm_levels_ltv`     -- the whole solve of ONE instance restated in NumPy in the kernel's order (zopt_amd/csrc/mpc_solve_wave_ltv.h):
                             an adapter of the one body of every family, oracle.mpc_oracle.admm_levels_stage, which has the stage's own
                             A_k, B_k, the offset's share D_k = P_{k+1} c_k of the costate, c_k in the rollout and in the free response of
                             the infeasibility certificate, and the cycle guard on whenever g != 0 or c != 0.  The arguments of
                             oracle.mpc_oracle.admm_levels with A_k, B_k, c_k, and the same returned namespace, margins included.
  * `solve_reference_ltv` -- an independent solve, an adapter of oracle.mpc_oracle.solve_reference_stage: the QP condensed in u with the
                             offsets carried through, SciPy trust-constr.
  * the cases of tests/test_mpc_ltv.py (their decisions are checked there, without a GPU) and tests/test_mpc_ltv_gpu.py, with `reference`,
    `run_steps` and `compare` in the manner of tests/mpc_iterates_cases.py (whose `compare` is tied to its own cases: the rule is restated).
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

from oracle import mpc_oracle as mo
from tests import mpc_iterates_cases as mc
from tests import mpc_tracking_ref as tr


def admm_levels_ltv(A, B, c, Q, R, Qf, N, x_lb, x_ub, u_lb, u_ub, x0, rho=1.0, eps_abs=1e-5, eps_rel=1e-5, max_iter=10000,
                    eps_prim_inf=1e-4, alpha=1.6, n_levels=7, rho_step=5.0, g=None, warm=None, shift=False, guard=True):
    """oracle.mpc_oracle.admm_levels_stage (see there for the options, the order of an iteration and the returned namespace) for
    A (N, n, n), B (N, n, m), c (N, n) or None (zeros) with one set of weights and bounds, as constant rows, every component hard.
    g: tests/mpc_tracking_ref.py: linear_term.  The guard is then on when g != 0 or c != 0."""
    return mo.admm_levels_stage(A, B, c, *mo.stage_args(Q, R, Qf, N, x_lb, x_ub, u_lb, u_ub), x0, None, None, rho, eps_abs, eps_rel,
                                max_iter, eps_prim_inf, alpha, n_levels, rho_step, g, warm, shift, guard)


def solve_reference_ltv(A, B, c, Q, R, Qf, N, x_lb, x_ub, u_lb, u_ub, x0, xRef=None, uRef=None):
    """Independent reference: oracle.mpc_oracle.solve_reference_stage (the QP condensed in u with the offsets carried through, SciPy
    trust-constr) with one set of weights and bounds.  Returns (x, u, cost about the references, zero if None)."""
    x, u, _ = mo.solve_reference_stage(A, B, c, *mo.stage_args(Q, R, Qf, N, x_lb, x_ub, u_lb, u_ub), x0, xRef=xRef, uRef=uRef)
    xRef, uRef = np.zeros_like(x) if xRef is None else xRef, np.zeros_like(u) if uRef is None else uRef
    return x, u, tr.cost(Q, R, Qf, x, u, xRef, uRef)


# ---- cases -------------------------------------------------------------------------------------------------------------------------------

EPS, MAX_ITER = 1e-6, 30000
SCIPY_SHAPES = [(1, 1, 2), (2, 1, 4), (2, 2, 3), (4, 1, 5), (4, 2, 4), (8, 4, 3), (8, 4, 7)]
SHAPES = SCIPY_SHAPES + [(12, 4, 1), (12, 4, 2), (12, 4, 7)]
EMBEDDED = [(3, 2, 5), (9, 4, 7)]


def _seed(n, m, N):
    """(a seed that fails a condition of tests/test_mpc_ltv.py: test_gpu_cases_are_decisive is replaced here, never skipped)"""
    return 1000 * n + 10 * m + N


def recipe(n, m, N, nb, bad=None, seed=None):
    """The issue's case recipe: the random stable problem of tests/test_mpc_gpu.py (seed 1000 n + 10 m + N) perturbed per stage,
    A_k = A + 0.15 randn / sqrt(n), B_k = B + 0.15 randn, c_k = 0.3 randn; boxes 4 and 0.15; x0 ~ U(-1, 1) from default_rng(11).
    -> (A (N,n,n), B (N,n,m), c (N,n), Q, R, Qf, x_lb, x_ub, u_lb, u_ub), x0 (nb, n); instance `bad` starts outside its box."""
    from tests.test_mpc_gpu import _random_problem
    rng = np.random.default_rng(_seed(n, m, N) if seed is None else seed)
    A, B, Q, R, Qf = _random_problem(rng, n, m, N)
    Ak = A + 0.15 * rng.standard_normal((N, n, n)) / np.sqrt(n)
    Bk = B + 0.15 * rng.standard_normal((N, n, m))
    ck = 0.3 * rng.standard_normal((N, n))
    x_ub, u_ub = np.full(n, 4.0), np.full(m, 0.15)
    x0 = np.random.default_rng(11).uniform(-1.0, 1.0, (nb, n))
    if bad is not None:
        x0[bad, 0] = 5.0
    return (Ak, Bk, ck, Q, R, Qf, -x_ub, x_ub, -u_ub, u_ub), x0


def _kw(eps=EPS, max_iter=MAX_ITER, **more):
    return dict(eps_abs=eps, eps_rel=eps, max_iter=max_iter, **more)


def _case(inst, x0, N, shared, steps=None, **more):
    """inst: per instance (A, B, c, Q, R, Qf, xl, xu, ul, uu); shared: one problem (P = ()) for the whole batch, else P = (len(inst),)"""
    c = SimpleNamespace(inst=inst, x0=np.asarray(x0), N=N, shared=shared, steps=steps or [dict(kw=_kw(), warm=False, x0="given")], xRef=None,
                        uRef=None, updates={})
    c.__dict__.update(more)
    return c


def infeasible_data(offset):
    """A = B = I_2, Q = R = Qf = I, N = 3, |x| <= 1, |u| <= 0.1, x0 = (0.5, 0), rho = 2: c_k = (1.5, 0) pushes x_1 out of the box"""
    I, one = np.eye(2), np.ones(2)
    ck = np.tile(np.array([1.5, 0.0]) if offset else np.zeros(2), (3, 1))
    return (np.tile(I, (3, 1, 1)), np.tile(I, (3, 1, 1)), ck, I, I, I, -one, one, -0.1 * one, 0.1 * one), np.array([0.5, 0.0])


QUAD_DT = 0.1
QUAD_UTRIM = np.array([9.807, 0.0, 0.0, 0.0])


def quad_trajectories(N, nb, seed=3):
    """`nb` distinct non-equilibrium trajectories of the quadcopter in absolute coordinates: the hover-linearised model rolled out from a
    tilted, moving start under small random thrust / torque deviations from trim.  -> xTraj (nb, N+1, 12), uTraj (nb, N, 4)"""
    A, B = tr.quad_data(N)[:2]
    rng = np.random.default_rng(seed)
    x = np.zeros((nb, N + 1, 12))
    x[:, 0, 0:3] = rng.uniform(-0.4, 0.4, (nb, 3))       # velocities
    x[:, 0, 6:8] = rng.uniform(-0.15, 0.15, (nb, 2))     # roll, pitch
    x[:, 0, 9:12] = rng.uniform(-1.0, 1.0, (nb, 3))      # position
    du = 0.05 * rng.standard_normal((nb, N, 4))
    for k in range(N):
        x[:, k + 1] = x[:, k] @ A.T + du[:, k] @ B.T
    return x, QUAD_UTRIM + du


@functools.lru_cache(maxsize=None)
def quad_case(N, nb, track):
    """The quadcopter (demos/lqrMpc.py's weights and bounds, in absolute coordinates: inputs within 3 of trim) linearised about `nb`
    trajectories by the oracle's complex-step expansion -- the CPU twin of AffineDynamics.from_trajectory(models.QuadcopterEuler(dt), traj),
    which the GPU test hands to ltvMpc.fromExpansion.  The cost is taken about trim (uRef = uTrim); track: and about the references of
    tests/mpc_tracking_ref.py: quad_reference, which leave the box."""
    from oracle import zopt_oracle as zo
    xT, uT = quad_trajectories(N, nb)
    _, _, Q, R, Qf, xl, xu, ul, uu = tr.quad_data(N)
    inst = []
    for b in range(nb):
        dyn = zo.affine_dynamics_from_trajectory(zo.quad_euler_step(QUAD_DT), zo.Trajectory(xT[b], uT[b]))
        f, f_x, f_u = (np.asarray(v) for v in dyn)
        ck = f - np.einsum("kij,kj->ki", f_x, xT[b, :-1]) - np.einsum("kij,kj->ki", f_u, uT[b])
        inst.append((f_x, f_u, ck, Q, R, Qf, xl, xu, QUAD_UTRIM + ul, QUAD_UTRIM + uu))
    rng = np.random.default_rng(5)
    x0 = xT[:, 0] + 0.02 * rng.standard_normal((nb, 12))
    xRef, uRef = np.zeros((nb, N + 1, 12)), np.tile(QUAD_UTRIM, (nb, N, 1))
    if track:
        _, xRef, du = tr.quad_reference(N, nb=nb, seed=0)
        uRef = uRef + du
    c = _case(inst, x0, N, False, steps=[dict(kw=_kw(1e-5 if track else 1e-4), warm=False, x0="given")], xRef=xRef, uRef=uRef)
    c.traj = (xT, uT)
    return c


@functools.lru_cache(maxsize=None)
def build(name):
    kind, *arg = name.split(":")
    shape = tuple(int(v) for v in arg[0].split(",")) if arg else None
    if kind == "shape":       # one shared problem, batch 7: two waves, an idle group; instance 3 starts outside its box
        n, m, N = shape
        data, x0 = recipe(n, m, N, 7, bad=3)
        return _case([data] * 7, x0, N, True)
    if kind == "embedded":
        n, m, N = shape
        data, x0 = recipe(n, m, N, 5)
        return _case([data] * 5, x0, N, True)
    if kind == "perproblem":  # P = (5,): distinct A_k, B_k, c_k, weights and bounds
        n, m, N = shape
        inst, x0 = [], []
        for i in range(5):
            (Ak, Bk, ck, Q, R, Qf, xl, xu, ul, uu), x = recipe(n, m, N, 5, seed=_seed(n, m, N) + 89 * (i + 1))   # (97: instance 0 of (12, 4, 10) had a level decision 8e-5 from a tie)
            s = 1.0 + 0.2 * i
            inst.append((Ak, Bk, ck, s * Q, R / s, s * Qf, xl * (1 + 0.1 * i), xu * (1 + 0.05 * i), ul * (1 + 0.1 * i), uu * (1 + 0.2 * i)))
            x0.append(x[i])
        return _case(inst, np.stack(x0), N, False)
    if kind == "chain":       # cold -> warm -> shift, then update() with re-perturbed dynamics and a warm solve
        n, m, N = 12, 4, 10
        data, x0 = recipe(n, m, N, 5)
        rng = np.random.default_rng(77)
        Ak, Bk, ck = data[:3]
        new = (Ak + 0.02 * rng.standard_normal(Ak.shape) / np.sqrt(n), Bk + 0.02 * rng.standard_normal(Bk.shape),
               ck + 0.05 * rng.standard_normal(ck.shape))
        steps = [dict(kw=_kw(1e-4), warm=False, x0="given"), dict(kw=_kw(1e-6), warm=True, x0="given"),
                 dict(kw=_kw(1e-6), warm="shift", x0="x1"), dict(kw=_kw(1e-6), warm=True, x0="same")]
        return _case([data] * 5, x0, N, True, steps=steps, updates={3: new})
    if kind == "track":       # references that leave the box (tests/mpc_tracking_ref.py: random_case)
        n, m, N = shape
        data, x0 = recipe(n, m, N, 8)
        _, _, xRef, uRef = tr.random_case(n, m, N, seed=41, nb=8)
        return _case([data] * 8, x0, N, True, xRef=xRef, uRef=uRef)
    if kind == "quad":
        return quad_case(30, 5, False)
    if kind == "trackquad":
        return quad_case(30, 5, True)
    if kind == "infeasible":
        (d1, x0), (d0, _) = infeasible_data(True), infeasible_data(False)
        return _case([d1, d0], np.stack([x0, x0]), 3, False, rho=2.0)
    if kind == "ltvunstable":   # every A_k at spectral radius 1.3 (problems.hard_mpc: unstable), B_k, c_k = 0.3 f_k, the weights of stage 0 and
        n, m, N = shape         # the family's terminal one; inputs within 0.6, no state box; x0 = 0.8 randn is feasible with active bounds
        from tests import problems
        A, B, ck, Qs, Rs, _ = (X[0] for X in problems.hard_mpc("unstable", n, m, N))
        inf, u_ub = np.full(n, np.inf), np.full(m, 0.6)
        x0 = 0.8 * np.random.default_rng(_seed(n, m, N) + 360).standard_normal((5, n))
        return _case([(A, B, 0.3 * ck, Qs[0], Rs[0], Qs[N - 1], -inf, inf, -u_ub, u_ub)] * 5, x0, N, True)
    raise KeyError(name)


GROUPS = {
    "shapes": [f"shape:{n},{m},{N}" for n, m, N in SHAPES],
    "embedded": [f"embedded:{n},{m},{N}" for n, m, N in EMBEDDED],
    "per_problem": ["perproblem:4,2,6", "perproblem:12,4,10"],
    "chain": ["chain"],
    "tracking": ["track:4,1,8", "trackquad"],
    "quadcopter": ["quad"],
    "infeasible": ["infeasible"],
    "unstable": ["ltvunstable:8,4,30"],
}
ALL = [name for names in GROUPS.values() for name in names]


def make_problem(mpcUtils, c):
    """the ltvMpc object of a case (host side only)"""
    if c.shared:
        A, B, ck, Q, R, Qf, xl, xu, ul, uu = c.inst[0]
    else:
        A, B, ck, Q, R, Qf, xl, xu, ul, uu = (np.stack([d[i] for d in c.inst]) for i in range(10))
    return mpcUtils.ltvMpc(A, B, Q, R, c.N, xl, xu, ul, uu, Qf=Qf, c=ck)


def case_rho(mpcUtils, c):
    rho = getattr(c, "rho", None)
    return np.broadcast_to(make_problem(mpcUtils, c).rho if rho is None else rho, (len(c.x0),))


def reference_steps(c, rho, solve=admm_levels_ltv):
    """[step][instance] -> result of `solve`, each fed its own previous final state and, after an update, the new dynamics"""
    out = []
    inst = list(c.inst)
    for s, step in enumerate(c.steps):
        if s in c.updates:
            inst = [c.updates[s] + d[3:] for d in inst]
        row = []
        for b, (A, B, ck, Q, R, Qf, xl, xu, ul, uu) in enumerate(inst):
            prev = out[-1][b] if s else None
            x0 = prev.x[1] if step["x0"] == "x1" else (prev.x0 if step["x0"] == "same" else c.x0[b])
            warm = (prev.y, prev.lam, prev.level) if (step["warm"] and prev.status == "optimal") else None
            g = None if c.xRef is None else tr.linear_term(Q, R, Qf, c.N, c.xRef[b], c.uRef[b])
            r = solve(A, B, ck, Q, R, Qf, c.N, xl, xu, ul, uu, x0, rho=float(rho[b]), g=g, warm=warm, shift=step["warm"] == "shift",
                      **step["kw"])
            r.x0 = x0
            row.append(r)
        out.append(row)
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    from zopt_amd import mpcUtils
    c = build(name)
    return reference_steps(c, case_rho(mpcUtils, c))


def run_steps(prob, c, ref, update=None):
    """every solve of the case on one ltvMpc object -> [step] dict of arrays, as tests/mpc_iterates_cases.py: run_kernel returns them"""
    nb = len(c.x0)
    got = []
    for s, step in enumerate(c.steps):
        if s in c.updates:
            A, B, ck = c.updates[s]
            (update or prob.update)(A=A, B=B, c=ck)
        x0 = np.stack([r.x0 for r in ref[s]])
        extra = {} if c.xRef is None else dict(xRef=c.xRef, uRef=c.uRef)
        if getattr(c, "rho", None) is not None:
            extra["rho"] = c.rho
        _, traj, status = prob.solve(x0, warm_start=step["warm"], **extra, **step["kw"])
        y, lam, level, ok = mc.read_state(prob, nb, c.N)
        got.append(dict(x=np.asarray(traj.xTraj), u=np.asarray(traj.uTraj), status=np.asarray(status, dtype=str),
                        iters=prob.last_iterations.copy(), resid=prob.last_residuals.copy(), y=y, lam=lam, ok=ok, level=level))
    return got


def compare(at_name, ref, got):
    """the suite's rule (tests/mpc_iterates_cases.py: compare) against a given reference: same status, iteration count, final level and
    ok flag; x, u, y, lam and the residuals to 1e-9 max(1, |reference|).  Returns the largest deviation relative to its bound."""
    TOL = mc.TOL
    worst = 0.0
    for s, (row, g) in enumerate(zip(ref, got)):
        for b, r in enumerate(row):
            at = f"{at_name} step {s} instance {b}"
            assert g["status"][b] == r.status, (at, g["status"][b], r.status, int(g["iters"][b]), r.iters)
            assert int(g["iters"][b]) == r.iters, (at, int(g["iters"][b]), r.iters)
            scale = TOL * max(1.0, np.max(np.abs(r.x)), np.max(np.abs(r.u)))
            dev = {"x": np.max(np.abs(g["x"][b] - r.x)) / scale, "u": np.max(np.abs(g["u"][b] - r.u)) / scale,
                   "rp": abs(g["resid"][b, 0] - r.rp) / (2 * scale), "rd": abs(g["resid"][b, 1] - r.rd) / (2 * scale * r.rho_final),
                   "y": np.max(np.abs(g["y"][b] - r.y)) / (TOL * max(1.0, np.max(np.abs(r.y)))),
                   "lam": np.max(np.abs(g["lam"][b] - r.lam)) / (TOL * max(1.0, np.max(np.abs(r.lam))))}
            assert max(dev.values()) <= 1.0, (at, dev)
            assert g["ok"][b] == (1.0 if r.status == "optimal" else 0.0), at
            assert g["level"][b] == r.level, (at, g["level"][b], r.level)
            worst = max(worst, max(dev.values()))
    return worst
