"""CPU checkers and cases for mpcUtils.ltvMpc with stage_varying= (per-stage weights Q_k, R_k and per-stage boxes on top of the stage-varying
dynamics); a helper module, not collected as a test.

Stage form, as the kernels take it (zm_mpc_setup_ltv_stage_f64, zm_mpc_solve_ltv_stage_f64): Qs (N, n, n) with Qs[k] the weight of
x_{k+1} (row N - 1 is terminal), Rs (N, m, m), and the box as the constructor takes it, x_lb, x_ub (N + 1, n) -- row 0 is the test on x0 --
and u_lb, u_ub (N, m).

  * `admm_levels_ltv_stage`     -- the NumPy restatement of the whole solve, an adapter of the one body of every family
                                   (oracle.mpc_oracle.admm_levels_stage, which takes this form) with every component hard: per-stage
                                   weights in the tables and per-stage boxes in the clip, the x0 test and the support term of the
                                   certificate.  Same options and returned namespace as tests/mpc_ltv_ref.py: admm_levels_ltv.
  * `solve_reference_ltv_stage` -- the condensed SciPy trust-constr solve with per-stage weights and bounds, an adapter likewise.
  * the named cases of tests/test_mpc_ltv_stage.py (their decisions and their non-vacuity are checked there, without a GPU) and
    tests/test_mpc_ltv_stage_gpu.py, with `reference`, `run_steps` and the comparison rule of tests/mpc_ltv_ref.py.
  * the case glue (`make_problem`, `reference_steps`, `scipy_case`, `variant_case`) takes the per-problem penalty weights `soft` of
    tests/mpc_ltv_soft_ref.py, whose cases are these with weights: [(l1, l2)] per problem, each (n + m,) in the stacked layout [x ; u].
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

from oracle.mpc_oracle import admm_levels_stage, cost_stage, linear_term_stage, solve_reference_stage, stage_form  # noqa: F401
from tests import mpc_iterates_cases as mc
from tests import mpc_ltv_ref as lr

ALL_SIX = ("Q", "R", "x_lb", "x_ub", "u_lb", "u_ub")
SOFT = ("x_soft_l1", "x_soft_l2", "u_soft_l1", "u_soft_l2")     # the constructor's names of (l1, l2) of the states, of the inputs


def admm_levels_ltv_stage(A, B, c, Qs, Rs, N, x_lb, x_ub, u_lb, u_ub, x0, rho=1.0, eps_abs=1e-5, eps_rel=1e-5, max_iter=10000,
                          eps_prim_inf=1e-4, alpha=1.6, n_levels=7, rho_step=5.0, g=None, warm=None, shift=False, guard=True):
    """oracle.mpc_oracle.admm_levels_stage (see there for the options, the order of an iteration and the returned namespace) with every
    component hard"""
    return admm_levels_stage(A, B, c, Qs, Rs, N, x_lb, x_ub, u_lb, u_ub, x0, None, None, rho, eps_abs, eps_rel, max_iter, eps_prim_inf,
                             alpha, n_levels, rho_step, g, warm, shift, guard)


def solve_reference_ltv_stage(A, B, c, Qs, Rs, N, x_lb, x_ub, u_lb, u_ub, x0, xRef=None, uRef=None):
    """Independent reference: oracle.mpc_oracle.solve_reference_stage with every component hard, the QP in u alone.  Returns
    (x, u, cost)."""
    return solve_reference_stage(A, B, c, Qs, Rs, N, x_lb, x_ub, u_lb, u_ub, x0, xRef=xRef, uRef=uRef)


# ---- cases -------------------------------------------------------------------------------------------------------------------------------
# An instance's data: (A (N,n,n), B (N,n,m), c (N,n), Qs (N,n,n), Rs (N,m,m), x_lb (N+1,n), x_ub, u_lb (N,m), u_ub).  The horizons are
# those of the issue -- 2 (below the prefetch depth), 3 (its depth), 4 and 5 (the two tail branches of the three-stage loops), 7 (3 * 2 + 1)
# -- and the batches 1, 5 (idle groups) and 9.

EPS, MAX_ITER = lr.EPS, lr.MAX_ITER
HORIZONS, BATCHES = (2, 3, 4, 5, 7), (1, 5, 9)


def _base(n, m, N, nb, seed=None, u_box=0.5, c_scale=0.1, spread=0.05):
    """the recipe of tests/mpc_ltv_ref.py in stage form with constant rows, made roomy so that the boxes a case adds decide what is
    feasible: offsets scaled by c_scale, the input box u_box, and starts within `spread` of the recipe's first one"""
    (A, B, c, Q, R, Qf, xl, xu, ul, uu), x0 = lr.recipe(n, m, N, 1, seed=seed)
    s = u_box / 0.15
    x0 = x0[0] + spread * np.random.default_rng(17).standard_normal((nb, n))
    return [A, B, c_scale * c, *stage_form(Q, R, Qf, N, xl, xu, s * ul, s * uu)], x0


def _plan(d, x0, N, rho=1.0):
    """(x, u) of the problem as it stands, from x0: what a case places its boxes against"""
    r = admm_levels_ltv_stage(*d[:5], N, *d[5:], x0, rho=rho, eps_abs=1e-8, eps_rel=1e-8, max_iter=MAX_ITER)
    assert r.status == "optimal", r.status
    return r.x, r.u


def _case(inst, x0, N, shared, kind, share=1, steps=None, **more):
    """inst: the data per problem; shared: one problem (P = ()) for the whole batch, else P = (len(inst),) and `share` instances per
    problem (x0 then has share * len(inst) rows, instance i * len(inst) + p solves problem p).  kind: "box" / "weight" / "both" / None,
    which non-vacuity condition of tests/test_mpc_ltv_stage.py applies."""
    c = SimpleNamespace(inst=inst, x0=np.asarray(x0), N=N, shared=shared, share=share, kind=kind, xRef=None, uRef=None, rho=None,
                        steps=steps or [dict(kw=lr._kw(), warm=False, x0="given")], stage_varying=ALL_SIX)
    c.__dict__.update(more)
    return c


def problem_of(c, b):
    return 0 if c.shared else b % len(c.inst)


def gate_data(closed):
    """A = B = I_2, c = 0, Q = R = I, N = 3, |u| <= 0.1, |x| <= 1 from x0 = (0, 0): x_2 can reach at most 0.2 in any component, and a gate
    0.5 <= x_2[0] <= 0.6 at stage 2 cannot be reached; opened to -1 <= x_2[0] <= 0.6 it can."""
    I, one = np.eye(2), np.ones(2)
    Qs, Rs, xl, xu, ul, uu = stage_form(I, I, I, 3, -one, one, -0.1 * one, 0.1 * one)
    xl[2, 0] = 0.5 if closed else -1.0
    xu[2, 0] = 0.6
    return [np.tile(I, (3, 1, 1)), np.tile(I, (3, 1, 1)), np.zeros((3, 2)), Qs, Rs, xl, xu, ul, uu], np.zeros(2)


@functools.lru_cache(maxsize=None)
def build(name):
    if name == "moving_boxes":      # (4, 2), N = 7, one problem, batch 5: a corridor on state 0 that follows the plan, narrows, and has a
        n, m, N = 4, 2, 7           # gate at stage 4 that cuts into it; an input box that opens along the horizon
        d, x0 = _base(n, m, N, 5)
        x, u = _plan(d, x0[0], N)
        k = np.arange(N + 1)
        d[5][:, 0], d[6][:, 0] = x[:, 0] - 0.6 + 0.05 * k, x[:, 0] + 0.6 - 0.05 * k
        d[6][4, 0] = x[4, 0] - 0.1
        d[7][:, 1], d[8][:, 1] = -0.02 - 0.08 * k[:N], 0.02 + 0.08 * k[:N]
        return _case([d], x0, N, True, "box")
    if name == "terminal_box":      # (2, 1), N = 5, batch 9: the stage box 4, a terminal set of width 0.1 next to where the plan ends
        n, m, N = 2, 1, 5
        d, x0 = _base(n, m, N, 9, u_box=1.5)
        x, u = _plan(d, x0[0], N)
        d[5][N], d[6][N] = x[N] + 0.1, x[N] + 0.2
        return _case([d], x0, N, True, "box")
    if name == "infinite_stages":   # (8, 4), N = 4, batch 1: no state bound at stages 1 and 3, no input bound at stage 2 and none above
        n, m, N = 8, 4, 4           # on input 0 of stage 0; boxes at stages 2 and 4 that cut into the plan
        d, x0 = _base(n, m, N, 1)
        x, u = _plan(d, x0[0], N)
        d[5][[1, 3]], d[6][[1, 3]] = -np.inf, np.inf
        d[5][2], d[6][2] = x[2] - 0.5, x[2] + 0.5
        d[6][2, :3] = x[2, :3] - 0.05
        d[5][4, 3:5] = x[4, 3:5] + 0.05
        d[7][2], d[8][2] = -np.inf, np.inf
        d[8][0, 0] = np.inf
        return _case([d], x0, N, True, "box")
    if name == "waypoint_weights":  # (12, 4), N = 7, batch 5: Q_k = 0 but at a waypoint (x_4) and the end, R_k discounted.  (The default
        n, m, N = 12, 4, 7          # penalty is the median over stages whose Q is mostly zero: the case passes its own.)
        d, x0 = _base(n, m, N, 5, spread=0.3)
        for k in range(N):
            d[3][k] = d[3][k] * (5.0 if k == 3 else (1.0 if k == N - 1 else 0.0))
            d[4][k] = d[4][k] * 0.8 ** k
        d[5][1:], d[6][1:] = -np.inf, np.inf       # (no state box beyond x0's: the inputs' box alone is active)
        return _case([d], x0, N, True, "weight", rho=1.0)
    if name == "both_tracking":     # (3, 2) embedded in (4, 2), N = 3, batch 9: weights and boxes by stage, references that leave the box
        n, m, N = 3, 2, 3
        d, x0 = _base(n, m, N, 9, spread=0.3)
        k = np.arange(N + 1)
        d[5][:, 1], d[6][:, 1] = -2.0 + 0.4 * k, 2.0 - 0.4 * k
        d[8][:, 0] = 0.5 - 0.12 * k[:N]
        for j in range(N):
            d[3][j] = d[3][j] * (0.2 + j)
            d[4][j] = d[4][j] * (2.0 - 0.5 * j)
        rng = np.random.default_rng(9)
        xRef = 3.0 * np.sin(0.9 * k[None, :, None] + rng.uniform(0, 6, (9, 1, n)))
        uRef = 0.8 * np.sign(rng.standard_normal((9, 1, m))) * np.ones((9, N, m))
        return _case([d], x0, N, True, "both", xRef=xRef, uRef=uRef)
    if name == "gate":              # P = (2,): the closed gate and the opened one
        (d1, x0), (d0, _) = gate_data(True), gate_data(False)
        return _case([d1, d0], np.stack([x0, x0]), 3, False, None, rho=2.0)
    if name == "x0_outside_row0":   # (2, 2), N = 2, batch 5: row 0 of the state box is tighter than the rest; instance 3 is inside every
        n, m, N = 2, 2, 2           # later row and outside row 0
        d, x0 = _base(n, m, N, 5, spread=0.2)
        d[5][0], d[6][0] = x0[0] - 1.0, x0[0] + 1.0
        x0 = x0.copy()
        x0[3, 0] += 1.5
        return _case([d], x0, N, True, None)
    if name == "per_problem":       # (4, 1), N = 5, P = (5,): distinct dynamics, stage weights and stage boxes per problem
        n, m, N = 4, 1, 5
        inst, x0 = [], []
        for i in range(5):
            d, x = _base(n, m, N, 5, seed=lr._seed(n, m, N) + 89 * (i + 1), u_box=0.4 + 0.05 * i)
            for j in range(N):
                d[3][j] = d[3][j] * (1.0 + 0.3 * ((i + j) % 3))
                d[4][j] = d[4][j] * (1.0 + 0.2 * ((2 * i + j) % 4))
            xp, up = _plan(d, x[i], N)
            d[5][:, i % n], d[6][:, i % n] = xp[:, i % n] - 0.5, xp[:, i % n] + 0.5
            d[6][1 + i % N, i % n] = xp[1 + i % N, i % n] - 0.05 * (i + 1)
            d[8][i % N, 0] = up[i % N, 0] - 0.02
            inst.append(d)
            x0.append(x[i])
        return _case(inst, np.stack(x0), N, False, None)
    if name == "shared_problems":   # (2, 1), N = 4, P = (3,), three instances per problem: batch 9
        n, m, N = 2, 1, 4
        inst, starts = [], []
        for i in range(3):
            d, x = _base(n, m, N, 1, seed=lr._seed(n, m, N) + 61 * (i + 1))
            starts.append(x[0])
            xp, _ = _plan(d, x[0], N)
            d[6][:, 0] = xp[:, 0] + 0.5
            d[6][1 + i, 0] = xp[1 + i, 0] - 0.02
            d[3][N - 1] = d[3][N - 1] * (1.0 + i)
            inst.append(d)
        x0 = np.stack([starts[b % 3] for b in range(9)]) + 0.01 * np.random.default_rng(13).standard_normal((9, n))
        return _case(inst, x0, N, False, None, share=3)
    raise KeyError(name)


BOX_CASES = ["moving_boxes", "terminal_box", "infinite_stages"]
WEIGHT_CASES = ["waypoint_weights"]
ALL = BOX_CASES + WEIGHT_CASES + ["both_tracking", "gate", "x0_outside_row0", "per_problem", "shared_problems"]
SCIPY_GPU = ["moving_boxes", "waypoint_weights"]   # the two whose final solutions the GPU test holds to the SciPy solve


def scipy_instances(name):
    """the instances whose SciPy solve the tests run: the first two -- of waypoint_weights the first alone (trust-constr needs half a
    minute for its instance 1, whose inputs sit on many bounds at once)"""
    return (0,) if name == "waypoint_weights" else (0, 1)[:len(build(name).x0)]


def weights_of(c, soft=None):
    """per problem (l1, l2): `soft`, else the case's own (a case of tests/mpc_ltv_soft_ref.py), else all hard (None, None)"""
    return soft or getattr(c, "soft", None) or [(None, None)] * len(c.inst)


def make_problem(mpcUtils, c, stage_varying=None, soft=None):
    """the ltvMpc object of a case (host side only): Q as the constructor takes it, (N + 1, n, n) with a row 0 that nothing reads.
    soft: weights per problem; None: the object of the stage entry, every component hard, whatever the case's own weights"""
    sv = c.stage_varying if stage_varying is None else stage_varying

    def args(d, w):
        A, B, ck, Qs, Rs, xl, xu, ul, uu = d
        n = B.shape[-2]
        return (A, B, np.concatenate([Qs[:1], Qs]), Rs, xl, xu, ul, uu, ck) + (() if w is None else (w[0][:n], w[1][:n], w[0][n:], w[1][n:]))
    if c.shared:
        A, B, Q, R, xl, xu, ul, uu, ck, *w = args(c.inst[0], soft and soft[0])
    else:
        A, B, Q, R, xl, xu, ul, uu, ck, *w = (np.stack(v) for v in zip(*(args(d, soft and soft[p]) for p, d in enumerate(c.inst))))
    return mpcUtils.ltvMpc(A, B, Q, R, c.N, xl, xu, ul, uu, c=ck, stage_varying=sv, **dict(zip(SOFT, w)))


def case_rho(mpcUtils, c):
    """the penalty per instance: the case's own or the constructor's default, which the penalty weights do not enter"""
    nb = len(c.x0)
    if c.rho is not None:
        return np.full(nb, float(c.rho))
    rho = np.atleast_1d(make_problem(mpcUtils, c).rho)
    return np.array([rho[problem_of(c, b)] for b in range(nb)])


def reference_steps(c, rho, soft=None):
    """[step][instance] -> result of admm_levels_stage, each fed its own previous final state"""
    soft = weights_of(c, soft)
    out = []
    for s, step in enumerate(c.steps):
        row = []
        for b in range(len(c.x0)):
            A, B, ck, Qs, Rs, xl, xu, ul, uu = c.inst[problem_of(c, b)]
            prev = out[-1][b] if s else None
            x0 = prev.x[1] if step["x0"] == "x1" else (prev.x0 if step["x0"] == "same" else c.x0[b])
            warm = (prev.y, prev.lam, prev.level) if (step["warm"] and prev.status == "optimal") else None
            g = None if c.xRef is None else linear_term_stage(Qs, Rs, c.N, c.xRef[b], c.uRef[b])
            r = admm_levels_stage(A, B, ck, Qs, Rs, c.N, xl, xu, ul, uu, x0, *soft[problem_of(c, b)], rho=float(rho[b]), g=g, warm=warm,
                                  shift=step["warm"] == "shift", **step["kw"])
            r.x0 = x0
            row.append(r)
        out.append(row)
    return out


def reference_case(c):
    from zopt_amd import mpcUtils
    return reference_steps(c, case_rho(mpcUtils, c))


@functools.lru_cache(maxsize=None)
def reference(name):
    return reference_case(build(name))


def envelope(xl, xu, ul, uu):
    """every bound replaced by its envelope over the stages: the smallest lower and the largest upper bound of the component (rows 1 .. N
    of the state box; row 0, the test on x0, stays)"""
    N = len(ul)
    exl, exu = np.tile(xl[1:].min(axis=0), (N + 1, 1)), np.tile(xu[1:].max(axis=0), (N + 1, 1))
    exl[0], exu[0] = xl[0], xu[0]
    return exl, exu, np.tile(ul.min(axis=0), (N, 1)), np.tile(uu.max(axis=0), (N, 1))


def scipy_case(c, b=0, soft=None):
    """(x, u) of the SciPy solve of instance b of a case: the slack QP where a component is soft"""
    xr, ur = (None, None) if c.xRef is None else (c.xRef[b], c.uRef[b])
    p = problem_of(c, b)
    x, u, _ = solve_reference_stage(*c.inst[p][:5], c.N, *c.inst[p][5:], c.x0[b], *weights_of(c, soft)[p], xRef=xr, uRef=ur)
    return x, u


@functools.lru_cache(maxsize=None)
def scipy_solution(name, b=0):
    return scipy_case(build(name), b)


def variant_case(c, variant, b=0, soft=None, **kw):
    """the restatement's result for instance b of a case with one thing replaced -- what a case's solution must differ from for its data
    to matter:  "envelope": every bound by its envelope over the stages;  "mean": every weight by its mean over the stages;  "hard": every
    penalty weight by a hard component (the status may then be "infeasible");  "free": the bounds of the soft components by none.
    kw: options other than those of tests/mpc_ltv_ref.py: _kw"""
    from zopt_amd import mpcUtils
    p = problem_of(c, b)
    A, B, ck, Qs, Rs, xl, xu, ul, uu = c.inst[p]
    l1, l2 = weights_of(c, soft)[p]
    if variant == "envelope":
        xl, xu, ul, uu = envelope(xl, xu, ul, uu)
    elif variant == "mean":
        Qs, Rs = np.tile(Qs.mean(axis=0), (c.N, 1, 1)), np.tile(Rs.mean(axis=0), (c.N, 1, 1))
    elif variant == "hard":
        l1 = l2 = None
    else:
        n = B.shape[-2]
        fx, fu = np.isfinite(l1[:n]), np.isfinite(l1[n:])
        xl, xu, ul, uu = np.where(fx, -np.inf, xl), np.where(fx, np.inf, xu), np.where(fu, -np.inf, ul), np.where(fu, np.inf, uu)
    g = None if c.xRef is None else linear_term_stage(Qs, Rs, c.N, c.xRef[b], c.uRef[b])
    return admm_levels_stage(A, B, ck, Qs, Rs, c.N, xl, xu, ul, uu, c.x0[b], l1, l2, rho=float(case_rho(mpcUtils, c)[b]), g=g, **lr._kw(**kw))


def variant_solution(name, variant, b=0):
    """(x, u) of `variant_case` "envelope" or "mean", which has a solution"""
    r = variant_case(build(name), variant, b)
    assert r.status == "optimal", (name, variant, r.status)
    return r.x, r.u


def run_steps(prob, c, ref):
    """every solve of the case on one ltvMpc object -> [step] dict of arrays, as tests/mpc_ltv_ref.py: run_steps returns them.  With
    `share` instances per problem x0 goes in as (share, P, n), instance i * P + p in row (i, p)."""
    nb = len(c.x0)
    lead = (nb,) if c.share == 1 else (c.share, len(c.inst))
    got = []
    for s, step in enumerate(c.steps):
        x0 = np.stack([r.x0 for r in ref[s]]).reshape(lead + (-1,))
        extra = {} if c.xRef is None else dict(xRef=c.xRef.reshape(lead + c.xRef.shape[1:]), uRef=c.uRef.reshape(lead + c.uRef.shape[1:]))
        if c.rho is not None:
            extra["rho"] = c.rho
        _, traj, status = prob.solve(x0, warm_start=step["warm"], **extra, **step["kw"])
        y, lam, level, ok = mc.read_state(prob, nb, c.N)
        flat = lambda X: np.asarray(X).reshape((nb,) + np.asarray(X).shape[len(lead):])
        got.append(dict(x=flat(traj.xTraj), u=flat(traj.uTraj), status=flat(np.asarray(status, dtype=str)),
                        iters=flat(prob.last_iterations.copy()), resid=flat(prob.last_residuals.copy()), y=y, lam=lam, ok=ok, level=level))
    return got


compare = lr.compare   # the suite's rule, as tests/test_mpc_ltv_gpu.py applies it
