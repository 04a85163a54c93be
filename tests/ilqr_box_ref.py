"""NumPy restatement of control-limited iLQR (input box u_lb <= u <= u_ub; Tassa, Mansard, Todorov 2014): support code of
tests/test_ilqr_box*.py, built on `oracle.zopt_oracle`'s pieces as tests/ilqr_tracking_ref.py is.

    rollout:        u_k = clip(alpha l_k + L_k (x_k - xPrev_k) + uPrev_k, lb, ub)                    (the clip lets a NaN through)
    backward step:  l_k = argmin_d 1/2 d' sym(Q_uu) d + Q_u' d   over   lb - u_k <= d <= ub - u_k
                    C = components at a bound with a multiplier of the right sign (lb == ub: always), F = the rest
                    L_k[C,:] = 0,  L_k[F,:] = -Q_uu[F,F]^-1 Q_ux[F,:]
                    v_x' = Q_x + L'Q_u + Q_ux'l + L'Q_uu l,   v_xx' = Q_xx + L'Q_uu L + L'Q_ux + Q_ux'L     (valid for any C)

The box-QP is solved by ENUMERATION of the 3^m active sets (every component free, at its lower or at its upper bound): the pattern
that satisfies the KKT conditions is returned, with its strict-complementarity margin.  fp64 (np.linalg.solve) or long double
(tests/hp_reference.solve_ld)."""
import itertools

import numpy as np

from oracle import zopt_oracle as zo
from tests import hp_reference as hp
from tests import ilqr_tracking_ref as tref

LD = np.longdouble


def clip_nan(u, lb, ub):
    """u < lb ? lb : (u > ub ? ub : u): a NaN passes (np.clip / fmin / fmax would not let it)"""
    return np.where(u < lb, lb, np.where(u > ub, ub, u))


def _solve(M, y, ld):
    if M.shape[0] == 0:
        return np.zeros(y.shape, dtype=LD if ld else np.float64)
    if ld:
        return hp.solve_ld(M, y)
    return np.linalg.solve(M, y)


def boxqp_enum(H, g, lo, hi, ld=False):
    """d = argmin 1/2 d' sym(H) d + g' d over lo <= d <= hi by enumeration of the 3^m active sets.

    Returns (d, clamped, margin): `clamped` a bit mask (bit i: component i is clamped), `margin` the strict-complementarity margin of
    the returned pattern -- the smallest of the clamped components' |multiplier| relative to max|g| and of the free components'
    distance to their bounds relative to max(|d|, the finite bounds' magnitudes) (inf where there is nothing to measure).  A
    component with lo == hi is clamped whatever its multiplier and does not enter the margin.  Among the patterns that satisfy the
    KKT conditions (only degenerate problems have several) the one with the largest margin is returned.  NaN input: (NaN, 0, NaN)."""
    dt = LD if ld else np.float64
    H, g, lo, hi = (np.asarray(t, dtype=dt) for t in (H, g, lo, hi))
    m = g.shape[0]
    if not (np.all(np.isfinite(H)) and np.all(np.isfinite(g))) or np.any(np.isnan(lo)) or np.any(np.isnan(hi)):
        return np.full(m, np.nan, dtype=dt), 0, float("nan")
    Hs = (H + H.T) / 2
    tiny = np.finfo(np.float64).tiny
    gs = max(float(np.max(np.abs(g))), tiny)
    fixed = lo == hi
    # every pattern at once (0 free, 1 at lo, 2 at hi): the system whose clamped rows and columns are the identity's
    pats = np.array(list(itertools.product((0, 1, 2), repeat=m)))
    pats = pats[np.all(~(fixed & (pats != 1)) & ~((pats == 1) & ~np.isfinite(lo)) & ~((pats == 2) & ~np.isfinite(hi)), axis=1)]
    C = pats != 0
    with np.errstate(invalid="ignore"):
        dC = np.where(pats == 1, lo, np.where(pats == 2, hi, 0)).astype(dt)
    S = np.where(C[:, :, None] | C[:, None, :], np.eye(m, dtype=dt), Hs)
    rhs = np.where(C, dC, -(g + dC @ Hs.T))
    d = (hp.solve_ld(S, rhs[..., None]) if ld else np.linalg.solve(S, rhs[..., None]))[..., 0]
    d = np.where(C, dC, d)
    grad = d @ Hs.T + g
    mult = np.where(pats == 1, grad, -grad)
    ok = np.all(C | ((d >= lo) & (d <= hi)), axis=1) & np.all(~C | fixed | (mult >= 0), axis=1)
    if not np.any(ok):
        raise RuntimeError("boxqp_enum: no active set satisfies the KKT conditions (is H positive definite?)")
    finite = np.concatenate([np.abs(lo[np.isfinite(lo)]), np.abs(hi[np.isfinite(hi)]), [tiny]]).astype(np.float64)
    ds = np.maximum(np.max(np.abs(d), axis=1).astype(np.float64), float(np.max(finite)))
    m_mult = np.min(np.where(C & ~fixed, np.abs(mult).astype(np.float64) / gs, np.inf), axis=1)
    m_dist = np.min(np.where(~C, np.minimum(d - lo, hi - d).astype(np.float64) / ds[:, None], np.inf), axis=1)
    margin = np.where(ok, np.minimum(m_mult, m_dist), -np.inf)
    w = int(np.argmax(margin))
    return d[w], int(sum(1 << i for i in range(m) if C[w, i])), float(margin[w])


def box_tail(Q_x, Q_u, Q_xx, Q_uu, Q_ux, lo, hi, ld=False):
    """The box step after the Q's are formed (the counterpart of zo._riccati_tail): -> (v_x', v_xx', l, L, clamped, margin)"""
    dt = LD if ld else np.float64
    m, n = Q_ux.shape
    l, mask, margin = boxqp_enum(Q_uu, Q_u, lo, hi, ld)
    F = [i for i in range(m) if not (mask >> i) & 1]
    L = np.zeros((m, n), dtype=dt)
    if F:
        L[F] = -_solve(Q_uu[np.ix_(F, F)], Q_ux[F], ld)
    Quul = Q_uu @ l
    v_x = Q_x + L.T @ Q_u + Q_ux.T @ l + L.T @ Quul
    v_xx = Q_xx + (L.T @ Q_uu) @ L + L.T @ Q_ux + Q_ux.T @ L
    return v_x, v_xx, l, L, mask, margin


def box_backward(dyn, cost, Vf, uTraj, lb, ub, ld=False):
    """The box backward pass of ONE trajectory, in fp64 or (ld) in long double, in the style of hp_reference._sweep_ld: dyn = (f, f_x
    (T,n,n), f_u (T,n,m)), cost = (c, c_x, c_u, c_xx, c_ux, c_uu), Vf = (v, v_x, v_xx), uTraj (T, m), lb / ub (m,).
    Returns dict(l (T,m), L (T,m,n), clamped (T,) bit masks, margin (T,))."""
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
        v_x, v_xx, l, L, mask, margin = box_tail(Q_x, Q_u, Q_xx, Q_uu, Q_ux, lb - uTraj[k], ub - uTraj[k], ld)
        out["l"][k], out["L"][k], out["clamped"][k], out["margin"][k] = l, L, mask, margin
    return out


def box_backward_batch(dyn, cost, Vf, uTraj, lb, ub, ld=False):
    """`box_backward` over a leading batch axis; lb / ub (m,) or (batch, m)"""
    b = np.asarray(uTraj).shape[0]
    lb, ub = (np.broadcast_to(np.asarray(t, dtype=np.float64), (b, np.asarray(uTraj).shape[-1])) for t in (lb, ub))
    outs = [box_backward(tuple(None if t is None else np.asarray(t)[i] for t in dyn), tuple(np.asarray(t)[i] for t in cost),
                         tuple(np.asarray(t)[i] for t in Vf), np.asarray(uTraj)[i], lb[i], ub[i], ld) for i in range(b)]
    return {k: np.stack([o[k] for o in outs]) for k in outs[0]}


def rollout(x0, dynFun, policy, trajPrev, lb, ub, alpha=1):
    """zo.trajectoryRollout with the clip"""
    xPrev, uPrev = trajPrev
    x = np.asarray(x0)
    xs, us = [x], []
    for k in range(np.shape(uPrev)[0]):
        u = clip_nan(alpha * policy.l[k] + policy.L[k] @ (x - xPrev[k]) + uPrev[k], lb, ub)
        x = dynFun(x, u)
        xs.append(x)
        us.append(u)
    return zo.Trajectory(np.stack(xs), np.stack(us))


def forward_pass(x0, dynFun, Q, R, Qf, xr, ur, policy, trajPrev, lb, ub):
    """forwardPass2 (ilqrUtils.py:116-150) with clipped rollouts: -> (traj, J, index, the 16 costs)"""
    Js, trajs = [], []
    for alpha in zo.LINESEARCH_ALPHAS:
        t = rollout(x0, dynFun, policy, trajPrev, lb, ub, alpha=alpha)
        trajs.append(t)
        Js.append(tref.trajectory_cost(Q, R, Qf, xr, ur, t))
    idx = int(np.argmin(np.asarray(Js)))
    return trajs[idx], Js[idx], idx, np.asarray(Js)


def iterativeLqr(dynFun, Q, R, Qf, x0, uGuess, lb, ub, xr=None, ur=None, maxIter=100, tol=1e-3, return_iters=False, trace=None):
    """tests/ilqr_tracking_ref.iterativeLqr (zo.iterativeLqr's loop) with the box: clipped initial rollout, box backward pass,
    clipped 16-way search.  xr (T+1, n), ur (T, m): the tracking cost's reference (None: zeros, the cost about the origin).
    `trace` receives (J_new, winning index, the 16 costs, the backward pass's clamped masks (T,), its margins (T,)) per iteration."""
    Q, R, Qf = (np.asarray(t, dtype=np.float64) for t in (Q, R, Qf))
    x0, uGuess = np.asarray(x0, dtype=np.float64), np.asarray(uGuess, dtype=np.float64)
    n = x0.shape[0]
    N, m = uGuess.shape
    lb, ub = (np.broadcast_to(np.asarray(t, dtype=np.float64), (m,)) for t in (lb, ub))
    xr = np.zeros((N + 1, n)) if xr is None else xr
    ur = np.zeros((N, m)) if ur is None else ur
    policy = zo.AffinePolicy(uGuess, np.zeros((N, m, n)))
    traj_prev = zo.Trajectory(np.zeros((N + 1, n)), np.zeros((N, m)))
    traj = rollout(x0, dynFun, policy, traj_prev, lb, ub)
    J = tref.trajectory_cost(Q, R, Qf, xr, ur, traj)
    converged, it = False, 0
    while (not converged) and it < maxIter:
        dyn = zo.affine_dynamics_from_trajectory(dynFun, traj)
        cost = zo.conditionQuadraticCost(tref.cost_expansion(Q, R, xr, ur, traj))
        Vf = zo.conditionValueFunction(tref.terminal_expansion(Qf, xr, traj.xTraj[-1]))
        bw = box_backward(dyn, cost, Vf, traj.uTraj, lb, ub)
        policy = zo.AffinePolicy(bw["l"], bw["L"])
        traj_new, J_new, idx, Js = forward_pass(x0, dynFun, Q, R, Qf, xr, ur, policy, traj, lb, ub)
        if trace is not None:
            trace.append((J_new, idx, Js, bw["clamped"], bw["margin"]))
        converged = bool(abs(J - J_new) <= tol)
        traj, J = traj_new, J_new
        it += 1
    out = (traj, policy.L, J, converged)
    return out + (it,) if return_iters else out
