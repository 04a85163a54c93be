"""NumPy restatement of control-limited iLQR / DDP with STAGE-VARYING input bounds (models.InputBox(..., stage_varying=True)): support
code of tests/test_ilqr_box_stage*.py.  It is tests/ilqr_box_ref.py and tests/ddp_box_ref.py with step k's row of the bounds handed to
each step -- the same pieces (`clip_nan`, `boxqp_enum`, `box_tail`, the DDP step's products and projection) in the same order, so that
with the same row at every step the results are those of the constant restatements bit for bit.

    rollout:        u_k = clip(alpha l_k + L_k (x_k - xPrev_k) + uPrev_k, lb_k, ub_k)
    backward step:  the box step of ilqr_box_ref.box_tail over lb_k - u_k <= d <= ub_k - u_k

lb, ub are (T, m) per trajectory everywhere in this file; `rows` broadcasts what a test holds to that."""
import functools

import numpy as np

from oracle import zopt_oracle as zo
from tests import ddp_box_ref as dr
from tests import hp_reference as hp
from tests import ilqr_box_cases as ibc
from tests import ilqr_box_ref as br
from tests import ilqr_tracking_ref as tref

LD = np.longdouble
_T, _mv = hp._T, hp._mv


def rows(b, lead, T, m):
    """a bound as the stage box takes it (scalar, (T, m) or (..., T, m)) -> lead + (T, m)"""
    return np.array(np.broadcast_to(np.asarray(b, dtype=np.float64), tuple(lead) + (T, m)))


def rollout(x0, dynFun, policy, trajPrev, lb, ub, alpha=1):
    """ilqr_box_ref.rollout with the row of the step"""
    xPrev, uPrev = trajPrev
    x = np.asarray(x0)
    xs, us = [x], []
    for k in range(np.shape(uPrev)[0]):
        u = br.clip_nan(alpha * policy.l[k] + policy.L[k] @ (x - xPrev[k]) + uPrev[k], lb[k], ub[k])
        x = dynFun(x, u)
        xs.append(x)
        us.append(u)
    return zo.Trajectory(np.stack(xs), np.stack(us))


def forward_pass(x0, dynFun, Q, R, Qf, xr, ur, policy, trajPrev, lb, ub):
    """ilqr_box_ref.forward_pass on `rollout` above: -> (traj, J, index, the 16 costs)"""
    Js, trajs = [], []
    for alpha in zo.LINESEARCH_ALPHAS:
        t = rollout(x0, dynFun, policy, trajPrev, lb, ub, alpha=alpha)
        trajs.append(t)
        Js.append(tref.trajectory_cost(Q, R, Qf, xr, ur, t))
    idx = int(np.argmin(np.asarray(Js)))
    return trajs[idx], Js[idx], idx, np.asarray(Js)


def box_backward(dyn, cost, Vf, uTraj, lb, ub, ld=False):
    """ilqr_box_ref.box_backward of ONE trajectory with lb, ub (T, m)"""
    dt = LD if ld else np.float64
    f_x, f_u = (np.asarray(t, dtype=dt) for t in dyn[1:3])
    c_x, c_u, c_xx, c_ux, c_uu = (np.asarray(t, dtype=dt) for t in cost[1:])
    v_x, v_xx = (np.asarray(t, dtype=dt) for t in Vf[1:])
    uTraj, lb, ub = (np.asarray(t, dtype=dt) for t in (uTraj, lb, ub))
    T, n, m = f_u.shape
    out = {"l": np.empty((T, m), dtype=dt), "L": np.empty((T, m, n), dtype=dt), "clamped": np.zeros(T, dtype=np.int64),
           "margin": np.empty(T)}
    for k in range(T - 1, -1, -1):
        fx, fu = f_x[k], f_u[k]
        Q_x = c_x[k] + fx.T @ v_x
        Q_u = c_u[k] + fu.T @ v_x
        Q_xx = c_xx[k] + (fx.T @ v_xx) @ fx
        Q_uu = c_uu[k] + (fu.T @ v_xx) @ fu
        Q_ux = c_ux[k] + (fu.T @ v_xx) @ fx
        v_x, v_xx, l, L, mask, margin = br.box_tail(Q_x, Q_u, Q_xx, Q_uu, Q_ux, lb[k] - uTraj[k], ub[k] - uTraj[k], ld)
        out["l"][k], out["L"][k], out["clamped"][k], out["margin"][k] = l, L, mask, margin
    return out


def box_backward_batch(dyn, cost, Vf, uTraj, lb, ub, ld=False):
    """`box_backward` over a leading batch axis; lb / ub (T, m) or (batch, T, m)"""
    b, T, m = np.asarray(uTraj).shape
    lb, ub = rows(lb, (b,), T, m), rows(ub, (b,), T, m)
    outs = [box_backward(tuple(None if t is None else np.asarray(t)[i] for t in dyn), tuple(np.asarray(t)[i] for t in cost),
                         tuple(np.asarray(t)[i] for t in Vf), np.asarray(uTraj)[i], lb[i], ub[i], ld) for i in range(b)]
    return {k: np.stack([o[k] for o in outs]) for k in outs[0]}


def ddp_box_backward(dyn, cost, Vf, uTraj, lb, ub, ld=False, eps=1e-3, perturb=None):
    """ddp_box_ref.ddp_box_backward of a batch with lb, ub (T, m) or (B, T, m); `perturb` as there"""
    dt = LD if ld else np.float64
    f_x, f_u, f_xx, f_ux, f_uu = (np.asarray(t, dtype=dt) for t in dyn[1:6])
    c_x, c_u, c_xx, c_ux, c_uu = (np.asarray(t, dtype=dt) for t in cost[1:])
    v_x, v_xx = (np.asarray(t, dtype=dt) for t in Vf[1:])
    B, T, n, m = f_u.shape
    u = np.asarray(uTraj, dtype=dt)
    lb, ub = rows(lb, (B,), T, m).astype(dt), rows(ub, (B,), T, m).astype(dt)
    out = {"l": np.empty((B, T, m), dtype=dt), "L": np.empty((B, T, m, n), dtype=dt), "clamped": np.zeros((B, T), dtype=np.int64),
           "margin": np.empty((B, T))}
    for k in range(T - 1, -1, -1):
        fx, fu = f_x[:, k], f_u[:, k]
        Q_x = c_x[:, k] + _mv(_T(fx), v_x)
        Q_u = c_u[:, k] + _mv(_T(fu), v_x)
        Q_xx = c_xx[:, k] + (_T(fx) @ v_xx) @ fx
        Q_uu = c_uu[:, k] + (_T(fu) @ v_xx) @ fu
        Q_ux = c_ux[:, k] + (_T(fu) @ v_xx) @ fx
        vf = [np.sum(v_x[:, :, None, None] * F[:, k], axis=-3) for F in (f_xx, f_ux, f_uu)]
        Z = np.concatenate([np.concatenate([vf[0], _T(vf[1])], axis=-1), np.concatenate([vf[1], vf[2]], axis=-1)], axis=-2)
        P = hp.psd_project_ld(Z, eps) if ld else zo.ensurePositiveDefinite(Z, eps)
        if perturb is not None:
            rel, rng = perturb
            E = rng.standard_normal(P.shape)
            E = E + _T(E)
            P = P + (E / np.max(np.abs(E), axis=(-1, -2), keepdims=True) * (rel * np.max(np.abs(P), axis=(-1, -2), keepdims=True))).astype(dt)
        Q_xx, Q_ux, Q_uu = Q_xx + P[:, :n, :n], Q_ux + P[:, n:, :n], Q_uu + P[:, n:, n:]
        v_x, v_xx = np.empty_like(v_x), np.empty_like(v_xx)
        for b in range(B):
            v_x[b], v_xx[b], l, L, mask, margin = br.box_tail(Q_x[b], Q_u[b], Q_xx[b], Q_uu[b], Q_ux[b], lb[b, k] - u[b, k],
                                                             ub[b, k] - u[b, k], ld)
            out["l"][b, k], out["L"][b, k], out["clamped"][b, k], out["margin"][b, k] = l, L, mask, margin
    return out


def ddp_box_backward_with_reruns(dyn, cost, Vf, uTraj, lb, ub, rels, seed=12345):
    """ddp_box_ref.ddp_box_backward_with_reruns on the stage form: the long-double pass and reruns with perturbed projections"""
    B, T, m = np.asarray(uTraj).shape
    k = len(rels) + 1
    rep = lambda t: tuple(None if x is None else np.concatenate([np.asarray(x)] * k, axis=0) for x in t)      # noqa: E731
    lbs, ubs = (np.concatenate([rows(t, (B,), T, m)] * k, axis=0) for t in (lb, ub))
    scale = np.repeat([0.0] + list(rels), B)[:, None, None]
    out = ddp_box_backward(rep(dyn), rep(cost), rep(Vf), np.concatenate([np.asarray(uTraj)] * k, axis=0), lbs, ubs, ld=True,
                           perturb=(scale, np.random.default_rng(seed)))
    cut = lambda i: {name: v[B * i:B * (i + 1)] for name, v in out.items()}      # noqa: E731
    return cut(0), [cut(i) for i in range(1, k)]


def solve(dynFun, Q, R, Qf, x0, uGuess, lb, ub, xr=None, ur=None, f_torch=None, maxIter=100, tol=1e-3, trace=None):
    """ilqr_box_ref.iterativeLqr (f_torch None) or ddp_box_ref.differentialDynamicProgramming_box (f_torch: the model's step in torch)
    with lb, ub (T, m).  -> (traj, L, J, converged, iterations); `trace` receives (J_new, winning index, the 16 costs, the backward
    pass's clamped masks (T,), its margins (T,)) per iteration."""
    Q, R, Qf = (np.asarray(t, dtype=np.float64) for t in (Q, R, Qf))
    x0, uGuess = np.asarray(x0, dtype=np.float64), np.asarray(uGuess, dtype=np.float64)
    n = x0.shape[0]
    N, m = uGuess.shape
    lb, ub = rows(lb, (), N, m), rows(ub, (), N, m)
    xr = np.zeros((N + 1, n)) if xr is None else xr
    ur = np.zeros((N, m)) if ur is None else ur
    policy = zo.AffinePolicy(uGuess, np.zeros((N, m, n)))
    traj = rollout(x0, dynFun, policy, zo.Trajectory(np.zeros((N + 1, n)), np.zeros((N, m))), lb, ub)
    J = tref.trajectory_cost(Q, R, Qf, xr, ur, traj)
    converged, it = False, 0
    while (not converged) and it < maxIter:
        cost = zo.conditionQuadraticCost(tref.cost_expansion(Q, R, xr, ur, traj))
        Vf = zo.conditionValueFunction(tref.terminal_expansion(Qf, xr, traj.xTraj[-1]))
        if f_torch is None:
            bw = box_backward(zo.affine_dynamics_from_trajectory(dynFun, traj), cost, Vf, traj.uTraj, lb, ub)
        else:
            one = lambda t: tuple(None if x is None else np.asarray(x)[None] for x in t)      # noqa: E731
            bw = ddp_box_backward(one(zo.quadratic_dynamics_from_trajectory(f_torch, traj)), one(cost), one(Vf), traj.uTraj[None], lb, ub)
            bw = {k: v[0] for k, v in bw.items()}
        policy = zo.AffinePolicy(bw["l"], bw["L"])
        traj_new, J_new, idx, Js = forward_pass(x0, dynFun, Q, R, Qf, xr, ur, policy, traj, lb, ub)
        if trace is not None:
            trace.append((J_new, idx, Js, bw["clamped"], bw["margin"]))
        converged = bool(abs(J - J_new) <= tol)
        traj, J = traj_new, J_new
        it += 1
    return traj, policy.L, J, converged, it


# ------------------------------------------------------------------------------------------------------------------------ cases
HORIZONS = (1, 2, 5, 12)
BATCH = 67              # one over a wave of line-search lanes' trajectories and three over a multiple of four


def stage_bounds(lb, ub, T, rng, u=None):
    """Per-step bounds from constant ones (m,) or (B, m): every row's half-width is rescaled by its own factor in 0.6 .. 1.4 about the
    row's centre (an infinite side stays infinite), so that rows differ per step, trajectory and component.  u (B, T, m) given: the
    rows are widened where needed so that u stays feasible (the sweeps' contract: uTraj lies inside its boxes)."""
    lb, ub = np.asarray(lb, dtype=np.float64), np.asarray(ub, dtype=np.float64)
    lbs = np.repeat(np.expand_dims(lb, -2), T, axis=-2)
    ubs = np.repeat(np.expand_dims(ub, -2), T, axis=-2)
    s = rng.uniform(0.6, 1.4, lbs.shape)
    fin = np.isfinite(lbs) & np.isfinite(ubs)
    with np.errstate(invalid="ignore"):
        c, w = np.where(fin, (lbs + ubs) / 2, 0.0), np.where(fin, (ubs - lbs) / 2, 0.0)
    lo = np.where(fin, c - s * w, np.where(np.isfinite(lbs), lbs * s, lbs))
    hi = np.where(fin, c + s * w, np.where(np.isfinite(ubs), ubs * s, ubs))
    lo, hi = np.minimum(lo, hi), np.maximum(lo, hi)
    if u is not None:
        lo, hi = np.minimum(lo, u), np.maximum(hi, u)
    return lo, hi


@functools.lru_cache(maxsize=None)
def sweep_case(family, n, m, T, batch, per_traj, ddp=False):
    """the hard family of tests/ilqr_box_cases.py (ddp: tests/ddp_box_cases.py) at a shape with per-step bounds (`stage_bounds` of the
    family's own box, u kept feasible; the `onbound` family keeps u_k ON its row's bound): dict(args = (dyn, cost, Vf, uTraj, lb, ub)
    with lb, ub (T, m) or (batch, T, m), ref = the long-double stage sweep, e_l, e_L = the fp64 stage restatement's own error against
    it, same64)"""
    from tests import ddp_box_cases as dbc
    if ddp:
        dyn, cost, Vf, u, lb, ub = dbc._sweep_inputs(family, n, m, T, batch, per_traj)
    else:
        dyn, cost, Vf, u, lb, ub = ibc._sweep_inputs(family, n, m, T, batch, per_traj, seed=17 * n + T + batch)
    rng = np.random.default_rng(1000 * n + 10 * T + batch + (7 if ddp else 0))
    on_lo, on_hi = u == np.expand_dims(np.broadcast_to(lb, (batch, m)), 1), u == np.expand_dims(np.broadcast_to(ub, (batch, m)), 1)
    if per_traj:
        slb, sub = stage_bounds(lb, ub, T, rng, u)
    else:       # one schedule for every trajectory: feasible for all of them
        slb, sub = stage_bounds(lb, ub, T, rng)
        slb, sub = np.minimum(slb, u.min(axis=0)), np.maximum(sub, u.max(axis=0))
    if family == "onbound" and per_traj:      # u_k exactly on its own row's bound, as the family means it
        u = np.where(on_lo, slb, np.where(on_hi, sub, u))
    args = (dyn, cost, Vf, u, slb, sub)
    if ddp:
        ref, reruns = ddp_box_backward_with_reruns(*args, rels=[dbc.SET_REL] + [dbc.SENS_REL] * dbc.SENS_SEEDS)
        o = ddp_box_backward(*args)
        s_l, s_L = (max(float(hp.sweep_metric(r[name], ref[name]).max()) for r in reruns[1:]) for name in ("l", "L"))
        stable = all(bool(np.array_equal(r["clamped"], ref["clamped"])) for r in reruns)
    else:
        ref, o, s_l, s_L, stable = box_backward_batch(*args, ld=True), box_backward_batch(*args), 0.0, 0.0, True
    return {"args": args, "ref": ref, "e_l": float(hp.sweep_metric(o["l"], ref["l"]).max()),
            "e_L": float(hp.sweep_metric(o["L"], ref["L"]).max()), "same64": bool(np.array_equal(o["clamped"], ref["clamped"])),
            "stable": stable, "s_l": s_l, "s_L": s_L}


def sweep_bounds(family, n, m, T, batch, per_traj, ddp=False):
    """(bound on l, bound on L) by the rule tests/test_ilqr_box_gpu.py and tests/test_ddp_box_gpu.py use (hp.sweep_bounds / hp.ddp_bounds:
    100 x the fp64 restatement's own error against long double on the case and on the plain family at the same shape)"""
    c, p = sweep_case(family, n, m, T, batch, per_traj, ddp), sweep_case("plain", n, m, T, batch, per_traj, ddp)
    if ddp:
        return hp.ddp_bounds(c["e_l"], p["e_l"], c["s_l"]), hp.ddp_bounds(c["e_L"], p["e_L"], c["s_L"])
    return hp.sweep_bounds(c["e_l"], p["e_l"]), hp.sweep_bounds(c["e_L"], p["e_L"])


# the sweeps' shapes: every (n, m) class, every horizon of HORIZONS, shared and per-trajectory schedules
SWEEP_SHAPES = ((3, 2, 1, 5, True), (3, 2, 12, 5, False), (8, 4, 2, 5, True), (8, 4, 5, 5, False), (12, 4, 5, 5, True), (12, 4, 12, 3, False))
DDP_SWEEP_SHAPES = ((3, 2, 1, 3, True), (3, 2, 5, 3, False), (8, 4, 2, 3, True), (12, 4, 5, 3, True), (12, 4, 12, 3, False))
DDP_SWEEP_FAMILIES = ("plain", "strongly_indefinite", "control_affine_8", "packed_pairs", "onbound")


def ddp_family_shapes(family):
    return tuple(s for s in DDP_SWEEP_SHAPES if family != "packed_pairs" or s[:2] == (12, 4))


# solves: the cases of tests/ilqr_box_cases.py / tests/ddp_box_cases.py (T = 7) with a schedule: the first two inputs pinned to
# committed values, the box narrowing from step 4 on, one infinite side kept; run to convergence (the base cases' maxIter = 8, tol =
# 1e-3: three or four iterations).  COST_GAP: the margin between the best two of the 16 costs every iteration of every trajectory must
# keep (tests/ddp_box_cases.py's figure: 10 x the 1e-9 to which costs are compared).  The gap shrinks by two orders per iteration as a
# solve converges, so the last search of some starts falls below it; STARTS names, per case, the base case's starts whose every
# search keeps it (all five where the case is not listed) -- found with the restatement alone, asserted in tests/test_ilqr_box_stage.py.
COST_GAP = 1e-8
STARTS = {("rb", False): (0, 1, 2, 4), ("quad_hover", False): (0, 1, 2, 4), ("rb", True): (1, 2, 4)}
SOLVE_CASES = (("lin3", False), ("rb", False), ("quad_hover", False), ("quad_hover", True), ("quad_origin", True), ("rb", True))


def solve_case(name, ddp):
    from tests import ddp_box_cases as dbc
    c = dict(dbc.solve_case(name)) if ddp else dict(ibc.solve_case(name))
    B, T, m = c["ug"].shape
    rng = np.random.default_rng(97)
    lb, ub = rows(c["lb"], (B,), T, m), rows(c["ub"], (B,), T, m)
    centre = np.where(np.isfinite(lb) & np.isfinite(ub), (lb + ub) / 2, c["ug"])
    # The base cases' boxes saturate nearly every input from the first iteration on; the 16 clipped rollouts then coincide and their
    # costs tie exactly (tests/ddp_box_cases.py says so of `rb`).  Wider boxes (10 x for the rigid body, 3 x for the quadcopter) leave
    # free inputs next to clamped ones in every iteration.
    widen = 10.0 if name == "rb" else 3.0 if name.startswith("quad") else 1.0
    with np.errstate(invalid="ignore"):
        half = widen * np.where(np.isfinite(ub - lb), (ub - lb) / 2, 0.0)
    lb, ub = np.where(np.isfinite(lb), centre - half, lb), np.where(np.isfinite(ub), centre + half, ub)
    pin = centre[:, :2] + 0.5 * half[:, :2] * rng.uniform(-1, 1, (B, 2, m))      # committed inputs, distinct per trajectory and step
    lb[:, :2], ub[:, :2] = pin, pin
    shrink = rng.uniform(0.5, 0.9, (B, T - 4, m))
    lb[:, 4:] = np.where(np.isfinite(lb[:, 4:]), centre[:, 4:] - shrink * half[:, 4:], lb[:, 4:])
    ub[:, 4:] = np.where(np.isfinite(ub[:, 4:]), centre[:, 4:] + shrink * half[:, 4:], ub[:, 4:])
    keep = list(STARTS.get((name, ddp), range(B)))
    c.update(lb=lb[keep], ub=ub[keep], x0=c["x0"][keep], ug=c["ug"][keep])
    if c["xRef"] is not None and np.ndim(c["xRef"]) == 3:
        c["xRef"] = c["xRef"][keep]
    if name == "lin3":
        c["kw"] = dict(maxIter=1, tol=1e-9)      # (an LQ problem: one iteration solves it, a second one would search among 16 costs
        #                                            that are equal to rounding -- its argmin is noise in any implementation)
    return c


@functools.lru_cache(maxsize=None)
def solve_reference(name, ddp):
    """the stage restatement's solve of every trajectory of the case: list of dict(traj, L, J, converged, its, trace)"""
    import warnings
    c = solve_case(name, ddp)
    B, T, m = c["ug"].shape
    n = c["x0"].shape[-1]
    out = []
    for b in range(B):
        xr, ur = tref.full_reference(c["xRef"], c["uRef"], T, n, m, b)
        tr = []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            traj, L, J, conv, its = solve(c["step"], c["Q"], c["R"], c["Qf"], c["x0"][b], c["ug"][b], c["lb"][b], c["ub"][b], xr, ur,
                                          f_torch=c["torch"] if ddp else None, trace=tr, **c["kw"])
        out.append(dict(traj=traj, L=L, J=J, converged=conv, its=its, trace=tr))
    return out


def cost_gap(Js):
    """relative distance between the best two of the line search's finite costs (tests/ddp_box_cases.cost_gap)"""
    s = np.sort(np.asarray(Js)[np.isfinite(Js)])
    return float((s[1] - s[0]) / abs(s[0])) if s.size > 1 else float("inf")
