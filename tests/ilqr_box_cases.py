"""The cases of the input-box tests (tests/test_ilqr_box.py on the CPU, tests/test_ilqr_box_gpu.py on the device), computed once per
process: inputs, the long-double reference of tests/ilqr_box_ref.py, the fp64 restatement's own error against it and the bounds that
follow from it (`hp_reference.sweep_bounds`' rule).  The CPU file asserts every case's strict-complementarity margin, so the GPU file
may compare clamped sets exactly.

Box-QP problems are built from their solution: a clamped pattern, a point d* (free components strictly inside, clamped ones on
their bound) and multipliers of the right sign are chosen first, g = -sym(H) d* + multipliers follows, so every problem has a margin
by construction."""
import functools

import numpy as np

from oracle import zopt_oracle as zo
from tests import hp_reference as hp
from tests import ilqr_box_ref as br
from tests import problems

MARGIN = 1e-6          # the smallest strict-complementarity margin a case may have (relative to the step's scale, boxqp_enum)
QP_CAP = 24            # BOXQP_CAP of zopt_amd/csrc/boxqp4.h


# ------------------------------------------------------------------------------------------------------------------------ box-QP
def _spd(rng, m, cond=None):
    if cond is None:
        M = rng.standard_normal((m, m))
        return M @ M.T / m + np.eye(m)
    U = np.linalg.qr(rng.standard_normal((m, m)))[0]
    w = np.logspace(-np.log10(cond) / 2, np.log10(cond) / 2, m) if m > 1 else np.array([1.0])
    H = (U * w) @ U.T
    return (H + H.T) / 2


def _qp(rng, m, pattern, cond=None, D=None, antisym=0.0, inf_sides=False, fixed=()):
    """one problem with the clamped pattern `pattern` (0 free, 1 at its lower, 2 at its upper bound); components in `fixed` get lo == hi"""
    D = np.ones(m) if D is None else D
    Hs = _spd(rng, m, cond) * np.outer(D, D)
    N = rng.standard_normal((m, m))
    H = Hs + antisym * (N - N.T) * np.outer(D, D)
    d = rng.standard_normal(m) / D
    lo, hi, mult = np.empty(m), np.empty(m), np.zeros(m)
    lam = rng.uniform(0.2, 1.0, m) * (np.abs(Hs) @ np.abs(d) + D * 1e-3)
    for i, p in enumerate(pattern):
        a, b = rng.uniform(0.2, 1.0, 2) / D[i]
        if i in fixed:
            lo[i] = hi[i] = d[i]
            mult[i] = lam[i] * rng.choice([-1.0, 1.0])
        elif p == 0:
            lo[i], hi[i] = d[i] - a, d[i] + b
            if inf_sides:
                side = rng.integers(0, 3)
                lo[i], hi[i] = (-np.inf if side != 1 else lo[i]), (np.inf if side != 0 else hi[i])
        elif p == 1:
            lo[i], hi[i], mult[i] = d[i], (np.inf if inf_sides else d[i] + b), lam[i]
        else:
            lo[i], hi[i], mult[i] = (-np.inf if inf_sides else d[i] - a), d[i], -lam[i]
    g = -Hs @ d + mult
    return H, g, lo, hi


@functools.lru_cache(maxsize=None)
def qp_problems(m):
    """The box-QP table for m unknowns: dict(family (P,) names, H (P,m,m), g, lo, hi (P,m), d (P,m) long double, clamped (P,), margin
    (P,), err (P,) the fp64 enumerator's error on d, bound {family: bound on the error of d})."""
    rng = np.random.default_rng(100 + m)
    fam, probs = [], []

    def add(name, *a, **kw):
        fam.append(name)
        probs.append(_qp(rng, m, *a, **kw))

    pat = lambda: tuple(int(p) for p in rng.integers(0, 3, m))          # noqa: E731
    for _ in range(6):
        add("plain", (0,) * m)
    for _ in range(4):
        add("all", tuple(int(p) for p in rng.integers(1, 3, m)))
    for i in range(m):
        for side in (1, 2):
            add("single", tuple(side if j == i else 0 for j in range(m)))
    for _ in range(10):
        add("mixed", pat(), antisym=0.05)
    for _ in range(6):
        add("inf", pat(), inf_sides=True)
    for _ in range(5):
        p = pat()
        add("fixed", p, fixed=tuple(int(i) for i in rng.choice(m, size=rng.integers(1, m + 1), replace=False)))
    for cond in (1e4, 1e6, 1e8):
        for _ in range(2):
            add("cond", pat(), cond=cond)
    for _ in range(5):
        add("scaled", pat(), D=rng.permutation(10.0 ** np.linspace(-2, 2, m)) if m > 1 else np.array([1e2]))
    H, g, lo, hi = (np.stack([p[i] for p in probs]) for i in range(4))
    ref = [br.boxqp_enum(*p, ld=True) for p in probs]
    f64 = [br.boxqp_enum(*p) for p in probs]
    d = np.stack([r[0] for r in ref])
    err = qp_metric(np.stack([r[0] for r in f64]), d)
    fam = np.array(fam)
    plain = float(err[fam == "plain"].max())
    bound = {name: hp.sweep_bounds(err[fam == name], plain) for name in sorted(set(fam))}
    return {"family": fam, "H": H, "g": g, "lo": lo, "hi": hi, "d": d, "clamped": np.array([r[1] for r in ref]),
            "margin": np.array([r[2] for r in ref]), "clamped64": np.array([r[1] for r in f64]), "err": err, "bound": bound}


def qp_metric(out, ref):
    """per problem: max|out - ref| / max|ref|"""
    out, ref = np.asarray(out, dtype=hp.LD), np.asarray(ref, dtype=hp.LD)
    scale = np.max(np.abs(ref), axis=-1)
    return (np.max(np.abs(out - ref), axis=-1) / np.where(scale > 0, scale, 1)).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------------ sweeps
# (n, m, T, batch, a box per trajectory): every T of the prefetch's tails, every shape class of the kernel (KS = 1, 2, 3), both batches
SWEEP_SHAPES = ((3, 2, 1, 5, False), (3, 2, 5, 9, True), (8, 4, 2, 9, True), (8, 4, 7, 5, False), (12, 4, 3, 5, True),
                (12, 4, 7, 9, False))
SWEEP_FAMILIES = ("plain", "unstable", "cheap", "onbound")


def _sweep_inputs(family, n, m, T, batch, per_traj, seed):
    if family == "unstable":
        dyn, cost, Vf = problems.sweep_unstable(batch, T, n, m, seed)
    elif family == "cheap":      # cheap control: large gains, many clamps
        dyn, cost, Vf = problems.sweep_cheap_control(batch, T, n, m, seed)
    else:
        dyn, cost, Vf = problems.random_ilqr_model(batch, T, n, m, seed)
    rng = np.random.default_rng(seed + 1000)
    tight = 0.1 if family == "cheap" else 1.0                      # a narrow box there: most steps end on it
    w = tight * rng.uniform(0.3, 0.8, (batch, m) if per_traj else (m,))
    lb, ub = -w, w.copy()
    ub[..., -1] = np.inf                                           # one side without a bound
    u = np.clip(0.3 * tight * rng.standard_normal((batch, T, m)), np.expand_dims(lb, -2) if per_traj else lb,
                np.expand_dims(ub, -2) if per_traj else ub)
    if family == "onbound":      # u_k exactly on a bound: the gradient decides between clamped with l = 0 and free
        u[..., 0] = np.broadcast_to(np.expand_dims(lb, -2) if per_traj else lb, u.shape)[..., 0]
        if m > 2:                # (the last component has no upper bound)
            u[..., 1] = np.broadcast_to(np.expand_dims(ub, -2) if per_traj else ub, u.shape)[..., 1]
    return dyn, cost, Vf, u, lb, ub


@functools.lru_cache(maxsize=None)
def sweep_case(family, n, m, T, batch, per_traj):
    """dict(args = (dyn, cost, Vf, uTraj, lb, ub), ref = the long-double box sweep (l, L, clamped, margin), e_l, e_L = the fp64
    restatement's error (hp.sweep_metric, maximum), same64 = its clamped sets equal the reference's)"""
    args = _sweep_inputs(family, n, m, T, batch, per_traj, seed=17 * n + T + batch)
    ref = br.box_backward_batch(*args, ld=True)
    o = br.box_backward_batch(*args)
    return {"args": args, "ref": ref, "e_l": float(hp.sweep_metric(o["l"], ref["l"]).max()),
            "e_L": float(hp.sweep_metric(o["L"], ref["L"]).max()), "same64": bool(np.array_equal(o["clamped"], ref["clamped"]))}


def sweep_bounds(family, n, m, T, batch, per_traj):
    """(bound on l, bound on L): hp.sweep_bounds from the restatement's error on the case and on the plain family at the same shape"""
    c, p = sweep_case(family, n, m, T, batch, per_traj), sweep_case("plain", n, m, T, batch, per_traj)
    return hp.sweep_bounds(c["e_l"], p["e_l"]), hp.sweep_bounds(c["e_L"], p["e_L"])


@functools.lru_cache(maxsize=None)
def unbounded_case(n, m, T, batch):
    """the plain family without a box: hp.ilqr_backward_ld's reference and the oracle's error against it"""
    dyn, cost, Vf = problems.random_ilqr_model(batch, T, n, m, 17 * n + T + batch)
    ref = hp.ilqr_backward_ld(dyn, cost, Vf)
    o = zo.backwardPass_ilqr(zo.AffineDynamics(*dyn), zo.QuadraticCostFunction(*cost), zo.QuadraticValueFunction(*Vf))
    e_l, e_L = float(hp.sweep_metric(o.l, ref["l"]).max()), float(hp.sweep_metric(o.L, ref["L"]).max())
    return {"args": (dyn, cost, Vf), "ref": ref, "bound_l": hp.sweep_bounds(e_l, e_l), "bound_L": hp.sweep_bounds(e_L, e_L)}


# ------------------------------------------------------------------------------------------------------------------------ solves
U_TRIM = np.array([9.807, 0.0, 0.0, 0.0])
SOLVE_CASES = ("lin3", "rb", "quad_hover")


def solve_case(name):
    """-> dict(model = ("lin", A, B) | ("rb", dt) | ("quad", dt), step = the oracle's callable, Q, R, Qf, xRef, uRef (None: the cost
    about the origin), x0 (B, n), ug (B, T, m), lb, ub (m,), kw = dict(maxIter, tol)).  Batch 5, T = 7."""
    rng = np.random.default_rng(61)
    B, T = 5, 7
    if name == "lin3":
        n, m = 3, 2
        r5 = np.random.default_rng(5)
        A, Bm = np.eye(n) + 0.05 * r5.standard_normal((n, n)), 0.3 * r5.standard_normal((n, m))
        return dict(model=("lin", A, Bm), step=lambda x, u: A @ x + Bm @ u, Q=np.eye(n), R=np.eye(m), Qf=10 * np.eye(n), xRef=None,
                    uRef=None, x0=rng.standard_normal((B, n)), ug=np.zeros((B, T, m)), lb=np.array([-0.6, -0.6]),
                    ub=np.array([0.6, np.inf]),
                    kw=dict(maxIter=2, tol=1e-9))      # (a third iteration would search among 16 costs that are equal to rounding)
    if name == "rb":
        n, m = 8, 4
        x0 = 0.3 * rng.standard_normal((B, n))
        return dict(model=("rb", 0.1), step=lambda x, u: x + 0.1 * zo.quad_rigidBodyDynamics(x, u), Q=np.eye(n), R=0.5 * np.eye(m),
                    Qf=10 * np.eye(n), xRef=None, uRef=None, x0=x0, ug=np.tile(U_TRIM, (B, T, 1)),
                    lb=np.array([8.5, -0.05, -0.05, -0.05]), ub=np.array([11.0, 0.05, 0.05, np.inf]), kw=dict(maxIter=8, tol=1e-3))
    n, m = 12, 4                 # quadcopters to goals, the cost about hover, thrust and moment limits
    x0 = np.zeros((B, n))
    x0[:, 9:12] = rng.uniform(-3, 3, (B, 3))
    goal = np.zeros((B, 1, n))
    goal[:, 0, 9:12] = rng.uniform(-2, 2, (B, 3))
    return dict(model=("quad", 0.1), step=zo.quad_euler_step(0.1), Q=np.eye(n), R=0.5 * np.eye(m), Qf=10 * np.eye(n), xRef=goal,
                uRef=U_TRIM, x0=x0, ug=np.tile(U_TRIM, (B, T, 1)), lb=U_TRIM - np.array([2, 0.05, 0.05, 0.05]),
                ub=U_TRIM + np.array([2, 0.05, 0.05, 0.05]), kw=dict(maxIter=8, tol=1e-3))


@functools.lru_cache(maxsize=None)
def solve_reference(name):
    """the restatement's solve of every trajectory of the case: list of dict(traj, L, J, converged, its, trace)"""
    import warnings
    from tests import ilqr_tracking_ref as tref
    c = solve_case(name)
    B, T, m = c["ug"].shape
    n = c["x0"].shape[-1]
    out = []
    for b in range(B):
        xr, ur = tref.full_reference(c["xRef"], c["uRef"], T, n, m, b)
        tr = []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            traj, L, J, conv, its = br.iterativeLqr(c["step"], c["Q"], c["R"], c["Qf"], c["x0"][b], c["ug"][b], c["lb"], c["ub"], xr, ur,
                                                    return_iters=True, trace=tr, **c["kw"])
        out.append(dict(traj=traj, L=L, J=J, converged=conv, its=its, trace=tr))
    return out


# ------------------------------------------------------------------------------------------------------------------------ convex
CONVEX_CASES = ((3, 2, 7, 5, 0.6), (12, 4, 7, 5, 1.0))          # (n, m, N, seed, box)


def convex_case(n, m, N, seed, box):
    rng = np.random.default_rng(seed)
    A = np.eye(n) + 0.05 * rng.standard_normal((n, n))
    B = 0.3 * rng.standard_normal((n, m))
    x0 = rng.standard_normal(n)
    lb, ub = -box * np.ones(m), box * np.ones(m)
    ub[-1] = np.inf
    return dict(A=A, B=B, x0=x0, Q=np.eye(n), R=np.eye(m), Qf=10 * np.eye(n), ug=np.zeros((N, m)), lb=lb, ub=ub, tol=1e-12)


@functools.lru_cache(maxsize=None)
def convex_reference(n, m, N, seed, box):
    """the restatement's solve of a convex case and its certificate: dict(traj, J, its, trace, stat, at_bound)"""
    from oracle import mpc_oracle as mo
    c = convex_case(n, m, N, seed, box)
    tr = []
    traj, L, J, conv, its = br.iterativeLqr(lambda x, u: c["A"] @ x + c["B"] @ u, c["Q"], c["R"], c["Qf"], c["x0"], c["ug"], c["lb"],
                                            c["ub"], tol=c["tol"], return_iters=True, trace=tr)
    inf = np.full(n, np.inf)
    kkt = mo.kkt_residuals(c["A"], c["B"], c["Q"], c["R"], c["Qf"], N, -inf, inf, c["lb"], c["ub"], c["x0"], traj.xTraj, traj.uTraj)
    at_bound = (traj.uTraj <= c["lb"]) | (traj.uTraj >= c["ub"])
    return dict(traj=traj, J=J, its=its, converged=conv, trace=tr, stat=float(kkt["stat"]), at_bound=at_bound)
