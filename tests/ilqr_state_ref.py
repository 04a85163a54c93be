"""NumPy restatement of iLQR with state bounds by an augmented-Lagrangian outer loop (AL-iLQR): support code of
tests/test_ilqr_state*.py, built on tests/ilqr_tracking_ref.py (cost, expansions) and tests/ilqr_box_ref.py (clipped rollouts, box
backward pass) as those are built on `oracle.zopt_oracle`.

For k = 1..T, i < n (row 0 is never constrained), with pos(s) = s > 0 ? s : 0 (a NaN gives 0):
    s_ub = lam_ub + mu (x_i - ub_i),   s_lb = lam_lb + mu (lb_i - x_i)
    psi  = (pos(s_ub)^2 - lam_ub^2 + pos(s_lb)^2 - lam_lb^2) / (2 mu),   g_i = pos(s_ub) - pos(s_lb),   h_i = mu ((s_ub > 0) + (s_lb > 0))
    J_AL = J_cost + P,  P = sum_k sum_i psi (its own accumulator, k then i ascending, added once)
    expansion: c_x[k] += g_k (1 <= k < T), v_x += g_T; the conditioned c_xx[k] += diag h_k, the conditioned v_xx += diag h_T
    outer loop: inner iLQR on J_AL from the stored inputs with policy (u, L = 0); viol = max(0, max(x - ub), max(lb - x)) over k >= 1;
                done = inner converged and viol <= ctol; else, if another outer iteration follows, lam <- pos(s), mu <- min(mu growth, mu_max)
One trajectory per call, as the oracle.  `ld=True` runs the penalty line search (rollouts, costs, penalty) and the sweep in long double
(tests/hp_reference.ilqr_backward_ld, tests/ilqr_box_ref.box_backward(ld=True)); the expansions stay the oracle's.

`PenaltyReference` is tests/linesearch_hp_ref.Reference for the line search on J_AL (with or without an input box): the 16 rollouts
and costs in long double, the yardstick S (every term of the cost and of the penalty by its absolute value), the fp64 restatement's
own error against it and the bounds that follow by that file's rule; `check_linesearch` is its `check` with J_AL and J_cost."""
import numpy as np

from oracle import zopt_oracle as zo
from tests import hp_reference as hpr
from tests import ilqr_box_ref as bref
from tests import ilqr_tracking_ref as tref
from tests import linesearch_hp_ref as lhp
from tests import model_hp_ref as mhp

LD = np.longdouble


def pos(s):
    with np.errstate(invalid="ignore"):
        return np.where(s > 0, s, 0.0)


def slacks(x, lb, ub, lam_lb, lam_ub, mu):
    """(s_ub, s_lb) of rows x (..., n); infinite bounds give -inf (never a NaN for a finite x)"""
    with np.errstate(invalid="ignore"):
        return lam_ub + mu * (x - ub), lam_lb + mu * (lb - x)


def penalty(xTraj, lb, ub, lam_lb, lam_ub, mu, ld=False):
    """P: rows 1..T, accumulated k ascending, i ascending (ld: in long double)"""
    if ld:
        xTraj, lb, ub, lam_lb, lam_ub, mu = (np.asarray(t, dtype=LD) for t in (xTraj, lb, ub, lam_lb, lam_ub, mu))
    P = LD(0) if ld else 0.0
    for k in range(1, xTraj.shape[0]):
        su, sl = slacks(xTraj[k], lb, ub, lam_lb[k], lam_ub[k], mu)
        pu, pl = pos(su), pos(sl)
        for i in range(xTraj.shape[1]):
            P = P + (((pu[i] * pu[i] - lam_ub[k, i] * lam_ub[k, i]) + pl[i] * pl[i]) - lam_lb[k, i] * lam_lb[k, i]) / (2.0 * mu)
    return P


def penalty_expansion(xTraj, lb, ub, lam_lb, lam_ub, mu):
    """g, h (T+1, n), row 0 zero"""
    su, sl = slacks(xTraj, lb, ub, lam_lb, lam_ub, mu)
    g = pos(su) - pos(sl)
    with np.errstate(invalid="ignore"):
        h = mu * ((su > 0).astype(np.float64) + (sl > 0).astype(np.float64))
    g[0], h[0] = 0.0, 0.0
    return g, h


def violation(xTraj, lb, ub):
    x = xTraj[1:]
    if np.isnan(x).any():
        return float("nan")
    with np.errstate(invalid="ignore"):
        return float(max(0.0, np.max(x - ub), np.max(lb - x)))


def _forward_pass(x0, dynFun, Q, R, Qf, xr, ur, policy, trajPrev, u_lb, u_ub, pen, ld=False):
    """the 16-way search on J_AL; ld: rollouts (dynFun must take long-double arrays: a linear model does), costs and penalty in long
    double, the winner's trajectory and costs rounded to fp64 at the end"""
    Js, Jcs, trajs = [], [], []
    if ld:
        x0, Q, R, Qf, xr, ur = (np.asarray(t, dtype=LD) for t in (x0, Q, R, Qf, xr, ur))
        policy = zo.AffinePolicy(np.asarray(policy.l, dtype=LD), np.asarray(policy.L, dtype=LD))
        trajPrev = zo.Trajectory(np.asarray(trajPrev[0], dtype=LD), np.asarray(trajPrev[1], dtype=LD))
    inf = np.inf
    for alpha in zo.LINESEARCH_ALPHAS:
        t = (bref.rollout(x0, dynFun, policy, trajPrev, -inf if u_lb is None else u_lb, inf if u_ub is None else u_ub, alpha=alpha)
             if (ld or u_lb is not None) else zo.trajectoryRollout(x0, dynFun, policy, trajPrev, alpha=alpha))
        trajs.append(t)
        Jc = tref.trajectory_cost(Q, R, Qf, xr, ur, t)
        Jcs.append(Jc)
        Js.append(Jc + penalty(t.xTraj, *pen, ld=ld))
    idx = int(np.argmin(np.asarray(Js)))
    if ld:
        w = zo.Trajectory(np.asarray(trajs[idx].xTraj, dtype=np.float64), np.asarray(trajs[idx].uTraj, dtype=np.float64))
        return w, float(Js[idx]), float(Jcs[idx]), idx, np.asarray(Js, dtype=np.float64)
    return trajs[idx], Js[idx], Jcs[idx], idx, np.asarray(Js)


def backward(dyn, cost, Vf, uTraj, u_lb, u_ub, ld=False):
    """the sweep of one trajectory on the given expansion (the penalty terms already in it) -> AffinePolicy, fp64"""
    if u_lb is None:
        if not ld:
            return zo.backwardPass_ilqr(dyn, cost, Vf)
        r = hpr.ilqr_backward_ld(tuple(dyn[:3]), tuple(cost), tuple(Vf))
    else:
        r = bref.box_backward(dyn, cost, Vf, uTraj, u_lb, u_ub, ld)
    return zo.AffinePolicy(np.asarray(r["l"], dtype=np.float64), np.asarray(r["L"], dtype=np.float64))


def inner_solve(dynFun, Q, R, Qf, xr, ur, x0, uStart, u_lb, u_ub, pen, maxIter, tol, trace=None, ld=False):
    """tests/ilqr_tracking_ref.iterativeLqr / tests/ilqr_box_ref.iterativeLqr (u_lb is not None) on J_AL.
    -> (traj, L, J_AL, J_cost, converged, iterations); `trace` receives per iteration dict(J, Jcost, idx, Js, su, sl, dJ)"""
    n = x0.shape[0]
    N, m = uStart.shape
    lb, ub, lam_lb, lam_ub, mu = pen
    policy = zo.AffinePolicy(uStart, np.zeros((N, m, n)))
    prev = zo.Trajectory(np.zeros((N + 1, n)), np.zeros((N, m)))
    traj = zo.trajectoryRollout(x0, dynFun, policy, prev) if u_lb is None else bref.rollout(x0, dynFun, policy, prev, u_lb, u_ub)
    Jc = tref.trajectory_cost(Q, R, Qf, xr, ur, traj)
    J = Jc + penalty(traj.xTraj, *pen)
    converged, it = False, 0
    while (not converged) and it < maxIter:
        dyn = zo.affine_dynamics_from_trajectory(dynFun, traj)
        cost = zo.conditionQuadraticCost(tref.cost_expansion(Q, R, xr, ur, traj))
        Vf = zo.conditionValueFunction(tref.terminal_expansion(Qf, xr, traj.xTraj[-1]))
        g, h = penalty_expansion(traj.xTraj, lb, ub, lam_lb, lam_ub, mu)
        c_x = cost.c_x.copy()
        c_x[1:] += g[1:N]
        c_xx = cost.c_xx + np.stack([np.diag(h[k]) for k in range(N)])
        cost = cost._replace(c_x=c_x, c_xx=c_xx)
        Vf = Vf._replace(v_x=Vf.v_x + g[N], v_xx=Vf.v_xx + np.diag(h[N]))
        policy = backward(dyn, cost, Vf, traj.uTraj, u_lb, u_ub, ld)
        traj_new, J_new, Jc_new, idx, Js = _forward_pass(x0, dynFun, Q, R, Qf, xr, ur, policy, traj, u_lb, u_ub, pen, ld)
        if trace is not None:
            su, sl = slacks(traj_new.xTraj[1:], lb, ub, lam_lb[1:], lam_ub[1:], mu)
            trace.append(dict(J=J_new, Jcost=Jc_new, idx=idx, Js=Js, su=su, sl=sl, dJ=abs(J - J_new)))
        converged = bool(abs(J - J_new) <= tol)
        traj, J, Jc = traj_new, J_new, Jc_new
        it += 1
    return traj, policy.L, J, Jc, converged, it


def constrainedIterativeLqr(dynFun, Q, R, Qf, x0, uGuess, x_lb, x_ub, u_lb=None, u_ub=None, xr=None, ur=None, mu0=1.0, growth=10.0,
                            mu_max=1e8, outer=10, ctol=1e-4, maxIter=100, tol=1e-3, trace=None, ld=False):
    """-> dict(traj, L, J (plain cost), converged (done), violation, mu, lam_lb, lam_ub, outer (iterations run), inner (list of the
    inner-iteration counts)).  `trace` receives per outer iteration dict(inner=[per-iteration dicts], violation, mu (the one the
    inner solve ran with), converged (the inner solve's))."""
    Q, R, Qf = (np.asarray(t, dtype=np.float64) for t in (Q, R, Qf))
    x0, uGuess = np.asarray(x0, dtype=np.float64), np.asarray(uGuess, dtype=np.float64)
    n = x0.shape[0]
    N, m = uGuess.shape
    lb, ub = (np.broadcast_to(np.asarray(t, dtype=np.float64), (n,)) for t in (x_lb, x_ub))
    if u_lb is not None:
        u_lb, u_ub = (np.broadcast_to(np.asarray(t, dtype=np.float64), (m,)) for t in (u_lb, u_ub))
    xr = np.zeros((N + 1, n)) if xr is None else xr
    ur = np.zeros((N, m)) if ur is None else ur
    lam_lb, lam_ub, mu = np.zeros((N + 1, n)), np.zeros((N + 1, n)), float(mu0)
    u, inner, done, ran = uGuess, [], False, 0
    traj = L = Jc = viol = None
    for j in range(outer):
        itr = [] if trace is not None else None
        traj, L, _, Jc, conv, its = inner_solve(dynFun, Q, R, Qf, xr, ur, x0, u, u_lb, u_ub, (lb, ub, lam_lb, lam_ub, mu), maxIter, tol, itr, ld)
        inner.append(its)
        viol = violation(traj.xTraj, lb, ub)
        if trace is not None:
            trace.append(dict(inner=itr, violation=viol, mu=mu, converged=conv))
        ran = j + 1
        done = bool(conv and viol <= ctol)
        if done:
            break
        if j + 1 < outer:
            su, sl = slacks(traj.xTraj, lb, ub, lam_lb, lam_ub, mu)
            lam_ub, lam_lb = pos(su), pos(sl)
            lam_ub[0], lam_lb[0] = 0.0, 0.0
            mu = min(mu * growth, mu_max)
        u = traj.uTraj
    return dict(traj=traj, L=L, J=Jc, converged=done, violation=viol, mu=mu, lam_lb=lam_lb, lam_ub=lam_ub, outer=ran, inner=inner)


# ---- the long-double reference of the penalty line search ---------------------------------------------------------------------------
def _penalty_batch(x, lb, ub, lam_lb, lam_ub, mu, absolute=False):
    """(b,) long double: P of the trajectories x (b, N + 1, n); absolute: every term by its absolute value (the yardstick's part)"""
    x, lb, ub, lam_lb, lam_ub = (np.asarray(t, dtype=LD) for t in (x, lb, ub, lam_lb, lam_ub))
    mu = np.asarray(mu, dtype=LD)[:, None, None]
    with np.errstate(all="ignore"):
        su, sl = lam_ub + mu * (x - ub[:, None, :]), lam_lb + mu * (lb[:, None, :] - x)
        pu, pl = np.where(su > 0, su, 0), np.where(sl > 0, sl, 0)
        sgn = 1 if absolute else -1
        t = (pu * pu + sgn * lam_ub * lam_ub + pl * pl + sgn * lam_lb * lam_lb) / (2 * mu)
    return np.sum(t[:, 1:], axis=(1, 2))


class PenaltyReference(lhp.Reference):
    """lhp.Reference of problem `p` for the search on J_AL.  pen = (lb (b, n), ub (b, n), lam_lb, lam_ub (b, N + 1, n), mu (b,));
    box = None or (u_lb, u_ub) (m,).  Besides Reference's fields (J, S, e, E, bJ, C, argmin, determined of J_AL; x, u, pe, pb of the
    rollouts): Jc, Sc, bJc -- the same of the cost without the penalty."""

    def __init__(self, p, pen, box=None):
        self.p, self.pen, self.box = p, pen, box
        na, b, N = len(p.alphas), p.b, p.N
        lb, ub, lam_lb, lam_ub, mu = pen
        xr64, ur64 = p.refs(np.float64)
        sl, so = p.step_ld(), p.step_oracle()
        blo, bhi = (-np.inf, np.inf) if box is None else box
        self.x, self.u = [], []
        z = lambda dt=LD: np.zeros((na, b), dtype=dt)                     # noqa: E731
        self.J, self.S, self.Jc, self.Sc, self.Jo, self.Jco = z(), z(), z(), z(), z(np.float64), z(np.float64)
        self.pe = np.zeros((na, b, N))
        alive = np.ones((na, b), bool)
        for a, al in enumerate(p.alphas):
            ls = p.l * al if p.kind == "quad" else p.l        # (as Reference: the quadcopter's step sizes are exact powers of two)
            aa = LD(1.0 if p.kind == "quad" else al)
            xs, us = [p.x0.astype(LD)], []
            with np.errstate(all="ignore"):
                for k in range(N):
                    uk = aa * ls[:, k].astype(LD) + np.einsum("bij,bj->bi", p.L[:, k].astype(LD), xs[-1] - p.xPrev[:, k].astype(LD)) + p.uPrev[:, k].astype(LD)
                    uk = bref.clip_nan(uk, LD(1) * blo, LD(1) * bhi)
                    us.append(uk)
                    xs.append(sl(xs[-1], uk))
            x, u = mhp.fp64_range(np.stack(xs, axis=1), np.stack(us, axis=1))
            xo, uo = np.zeros((b, N + 1, p.n)), np.zeros((b, N, p.m))
            with np.errstate(all="ignore"):
                for i in range(b):
                    t = bref.rollout(p.x0[i], so, zo.AffinePolicy(p.l[i], p.L[i]), zo.Trajectory(p.xPrev[i], p.uPrev[i]), blo, bhi, alpha=al)
                    xo[i], uo[i] = t.xTraj, t.uTraj
                    self.Jco[a, i] = lhp.cost_oracle(p, xo[i] - xr64[i], uo[i] - ur64[i])
                    self.Jo[a, i] = self.Jco[a, i] + penalty(xo[i], lb[i], ub[i], lam_lb[i], lam_ub[i], mu[i])
            self.Jc[a], self.Sc[a] = lhp.cost_ld(p, x, u), lhp.cost_ld(p, x, u, absolute=True)
            self.J[a] = self.Jc[a] + _penalty_batch(x, *pen)
            self.S[a] = self.Sc[a] + _penalty_batch(x, *pen, absolute=True)
            self.pe[a] = lhp.prefix_errors(xo, uo, x, u)
            alive[a] = np.all(np.isfinite(x.astype(np.float64)), axis=(1, 2)) & np.all(np.isfinite(u.astype(np.float64)), axis=(1, 2))
            self.x.append(x), self.u.append(u)
        self.pb = np.maximum(mhp.FLOOR, 100.0 * self.pe)
        self.comparable = np.all(alive & np.all(self.pe <= mhp.DETERMINED, axis=2), axis=0)
        with np.errstate(all="ignore"):
            def bounds(J, S, Jo):
                Sp = np.where(S > 0, S, LD(1))
                e = np.where(alive, np.abs(Jo.astype(LD) - J) / Sp, np.inf).astype(np.float64)
                E = np.max(e, axis=0)
                return e, E, np.maximum(LD(mhp.FLOOR), 100 * E.astype(LD))[None, :] * S
            self.e, self.E, self.bJ = bounds(self.J, self.S, self.Jo)
            _, _, self.bJc = bounds(self.Jc, self.Sc, self.Jco)
            lo, hi = self.J - self.bJ, self.J + self.bJ
            c = self.comparable
            self.C = np.zeros((na, b), bool)
            self.C[:, c] = lo[:, c] <= np.min(hi[:, c], axis=0)
            self.argmin = np.zeros(b, dtype=int)
            self.argmin[c] = np.argmin(self.J[:, c].astype(LD), axis=0)
        self.determined = c & (self.C.sum(axis=0) == 1)


def check_linesearch(ref, xT, uT, J, Jc, idx, J16=None, what=""):
    """lhp.check on J_AL -- the choice inside the candidate set (the argmin where it is determined), J against the long-double J_AL at
    the chosen index, the returned trajectory's J_AL in long double against the returned J, the returned rows against the long-double
    rollout, the 16 costs of single-step-size calls -- plus J_cost against the long-double cost at the chosen index, under its own bound"""
    p = ref.p
    xT, uT, J, Jc = (np.asarray(t, np.float64) for t in (xT, uT, J, Jc))
    idx = np.asarray(idx).astype(int)
    rows = np.flatnonzero(ref.comparable)
    assert len(rows), f"{what}: no comparable trajectory"
    assert np.all((idx[rows] >= 0) & (idx[rows] < len(p.alphas))), f"{what}: idx out of range {idx}"
    ii = idx[rows]
    assert np.all(np.isfinite(J[rows])) and np.all(np.isfinite(Jc[rows])) and np.all(np.isfinite(xT[rows])) and np.all(np.isfinite(uT[rows])), f"{what}: not finite"
    assert np.all(ref.C[ii, rows]), f"{what}: idx {ii.tolist()} outside the candidate sets (argmin {ref.argmin[rows].tolist()})"
    det = ref.determined[rows]
    assert np.array_equal(ii[det], ref.argmin[rows][det]), f"{what}: idx {ii[det].tolist()} != determined argmin {ref.argmin[rows][det].tolist()}"
    bJ = ref.bJ[ii, rows]
    r2 = np.max(np.abs(J[rows].astype(LD) - ref.J[ii, rows]) / bJ)
    rc = np.max(np.abs(Jc[rows].astype(LD) - ref.Jc[ii, rows]) / ref.bJc[ii, rows])
    q = p.rows(rows)
    Jret = lhp.cost_ld(q, xT[rows], uT[rows]) + _penalty_batch(xT[rows], *[t[rows] for t in ref.pen])
    r3 = np.max(np.abs(Jret - J[rows].astype(LD)) / bJ)
    xr = np.stack([ref.x[a][i] for a, i in zip(ii, rows)])
    ur = np.stack([ref.u[a][i] for a, i in zip(ii, rows)])
    r4 = float(np.max(lhp.prefix_errors(xT[rows], uT[rows], xr, ur) / ref.pb[ii, rows]))
    assert np.array_equal(xT[rows, 0], p.x0[rows]), f"{what}: xTraj[0] is not x0"
    r5 = 0.0
    if J16 is not None:
        J16 = np.asarray(J16, np.float64)
        assert J16.shape == (len(p.alphas), p.b) and np.all(np.isfinite(J16[:, rows])), f"{what}: single-step-size costs not finite"
        r5 = float(np.max(np.abs(J16[:, rows].astype(LD) - ref.J[:, rows]) / ref.bJ[:, rows]))
    out = {"J_AL": float(r2), "J_cost": float(rc), "J_AL of returned trajectory": float(r3), "trajectory": r4, "16 costs": r5}
    print(f"{what} [{ref.summary()}]: worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in out.items()))
    assert r2 <= 1.0, f"{what}: |J_AL - J_ld[idx]| is {r2:.3g} x its bound"
    assert rc <= 1.0, f"{what}: |J_cost - J_cost,ld[idx]| is {rc:.3g} x its bound"
    assert r3 <= 1.0, f"{what}: the returned trajectory's J_AL is {r3:.3g} x the bound away from the returned J"
    assert r4 <= 1.0, f"{what}: the returned trajectory is {r4:.3g} x its bound away from the rollout at alphas[idx]"
    assert r5 <= 1.0, f"{what}: a single-step-size cost is {r5:.3g} x its bound away"
    return out


def linesearch_penalty(p, seed, scale=1e8, far=1e6):
    """multipliers and mu up to `scale` and bounds up to `far` from the origin for problem p, seeded: the trajectories' mu are 10^linspace(0, log scale)
    in a seeded order; per entry a bound within a few units of the previous trajectory's state (so that both signs of s occur) or `far` away or
    infinite, a multiplier 0 or 10^U(-2, log scale)"""
    rng = np.random.default_rng([seed, p.b, p.N, p.n])
    b, N, n = p.b, p.N, p.n
    sc = np.maximum(np.max(np.abs(p.xPrev), axis=1), 1e-3)                   # (b, n)
    mid = np.median(p.xPrev, axis=1)
    kind = rng.integers(0, 4, (2, b, n))
    off = sc * rng.uniform(0.05, 0.5, (2, b, n))
    lb = np.where(kind[0] == 0, -np.inf, np.where(kind[0] == 1, -far * rng.uniform(0.5, 1.0, (b, n)), mid - off[0]))
    ub = np.where(kind[1] == 0, np.inf, np.where(kind[1] == 1, far * rng.uniform(0.5, 1.0, (b, n)), mid + off[1]))
    ub = np.maximum(ub, lb)
    mu = rng.permutation(10.0 ** np.linspace(0, np.log10(scale), b))            # (the largest is `scale` itself)
    lam = [np.where(rng.random((b, N + 1, n)) < 0.5, 0.0, 10.0 ** rng.uniform(-2, np.log10(scale), (b, N + 1, n))) for _ in range(2)]
    for t in lam:
        t[:, 0] = 0.0
    lam[0][~np.isfinite(np.broadcast_to(lb[:, None], lam[0].shape))] = 0.0
    lam[1][~np.isfinite(np.broadcast_to(ub[:, None], lam[1].shape))] = 0.0
    return lb, ub, lam[0], lam[1], mu
