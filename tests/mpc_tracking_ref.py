"""CPU checkers for lqrMpc with references (xRef, uRef); a helper module, not collected as a test.

The tracking problem is the QP of mpcUtils.py:48-59 with the cost taken about a reference,
    sum_{k<N} (x_k - xr_k)'Q(x_k - xr_k) + (u_k - ur_k)'R(u_k - ur_k)  +  (x_N - xr_N)'Qf(x_N - xr_N),
i.e. the same quadratic form plus a linear term.  Three checkers, the tracking counterparts of oracle/mpc_oracle.py:

  * `admm`            -- NumPy restatement of the build's tracking ADMM for ONE instance: oracle.mpc_oracle.admm with the linear term
                         g in the backward sweep and the dual tolerance scaled by max(rho |lam|_inf, |g|_inf);
  * `solve_reference` -- independent solve: the condensed QP of mpc_oracle.condense with the reference's linear term, SciPy trust-constr;
  * `kkt_residuals`   -- the solver-independent optimality certificate of mpc_oracle.kkt_residuals with that gradient.
"""
from __future__ import annotations

import numpy as np
import scipy.optimize as spo

from oracle.mpc_oracle import CHECK_EVERY, condense, riccati_tables, rollout


def linear_term(Q, R, Qf, N, xRef, uRef):
    """g in the kernels' stage layout: gx[k] = -(W + W') xr_{k+1} (W = Q, Qf at k = N-1), gu[k] = -(R + R') ur_k."""
    gx = np.stack([-((Qf if k == N - 1 else Q) + (Qf if k == N - 1 else Q).T) @ xRef[k + 1] for k in range(N)])
    gu = np.stack([-(R + R.T) @ uRef[k] for k in range(N)])
    return gx, gu


def cost(Q, R, Qf, x, u, xRef, uRef):
    dx, du = x - xRef, u - uRef
    return sum(dx[k] @ Q @ dx[k] + du[k] @ R @ du[k] for k in range(u.shape[0])) + dx[-1] @ Qf @ dx[-1]


def condense_tracking(A, B, Q, R, Qf, N, x0, xRef, uRef):
    """mpc_oracle.condense plus the reference: cost = u'Hu + 2 g'u + const with
    g = g_regulator - sum_k Gam_k' (W + W')/2 xr_k - blockdiag((R + R')/2) ur."""
    n, m = B.shape
    Phi, Gam, H, g, c = condense(A, B, Q, R, Qf, N, x0)
    g = g.copy()
    for k in range(1, N + 1):
        W = Qf if k == N else Q
        g -= Gam[k].T @ (0.5 * (W + W.T)) @ xRef[k]
    for k in range(N):
        g[k * m:(k + 1) * m] -= 0.5 * (R + R.T) @ uRef[k]
    return Phi, Gam, H, g


def solve_reference(A, B, Q, R, Qf, N, x_lb, x_ub, u_lb, u_ub, x0, xRef, uRef):
    """Independent reference: condensed QP in u, linear inequality constraints on the states, SciPy trust-constr.
    Returns (x, u, tracking cost)."""
    n, m = B.shape
    Phi, Gam, H, g = condense_tracking(A, B, Q, R, Qf, N, x0, xRef, uRef)
    Hs = H + H.T
    rows, lo, hi = [], [], []
    for k in range(1, N + 1):
        off = Phi[k] @ x0
        for i in range(n):
            if np.isfinite(x_lb[i]) or np.isfinite(x_ub[i]):
                rows.append(Gam[k][i])
                lo.append(x_lb[i] - off[i])
                hi.append(x_ub[i] - off[i])
    cons = [spo.LinearConstraint(np.array(rows), np.array(lo), np.array(hi))] if rows else []
    res = spo.minimize(lambda u: u @ H @ u + 2 * g @ u, np.zeros(N * m), jac=lambda u: Hs @ u + 2 * g, hess=lambda u: Hs,
                       method="trust-constr", bounds=spo.Bounds(np.tile(u_lb, N), np.tile(u_ub, N)), constraints=cons,
                       options=dict(gtol=1e-12, xtol=1e-14, barrier_tol=1e-14, maxiter=5000))
    u = res.x.reshape(N, m)
    x = rollout(A, B, x0, u)
    return x, u, cost(Q, R, Qf, x, u, xRef, uRef)


def n_active(x, u, x_lb, x_ub, u_lb, u_ub, tol=1e-5):
    """number of bounds a candidate sits on (x_1..x_N and u_0..u_{N-1})"""
    return int(np.sum(x[1:] >= x_ub - tol) + np.sum(x[1:] <= x_lb + tol) + np.sum(u >= u_ub - tol) + np.sum(u <= u_lb + tol))


def kkt_residuals(A, B, Q, R, Qf, N, x_lb, x_ub, u_lb, u_ub, x0, x, u, xRef, uRef, act_tol=1e-6):
    """mpc_oracle.kkt_residuals for the tracking cost: dict(dyn, bound, stat) -- max dynamics defect, max bound violation, and the
    distance of the reduced gradient (condensed variables, with the reference's linear term) from the cone spanned by the outward
    normals of the active constraints, relative to the gradient's norm."""
    n, m = B.shape
    dyn = max(np.max(np.abs(x[k + 1] - (A @ x[k] + B @ u[k]))) for k in range(N))
    dyn = max(dyn, np.max(np.abs(x[0] - x0)))
    viol = max(np.max(np.maximum(x_lb - x, 0)), np.max(np.maximum(x - x_ub, 0)), np.max(np.maximum(u_lb - u, 0)),
               np.max(np.maximum(u - u_ub, 0)))
    Phi, Gam, H, g = condense_tracking(A, B, Q, R, Qf, N, x0, xRef, uRef)
    grad = (H + H.T) @ u.reshape(-1) + 2 * g
    normals = []
    for k in range(N):
        for j in range(m):
            e = np.zeros(N * m)
            e[k * m + j] = 1.0
            if u[k, j] >= u_ub[j] - act_tol:
                normals.append(e)
            if u[k, j] <= u_lb[j] + act_tol:
                normals.append(-e)
    for k in range(1, N + 1):
        for i in range(n):
            if x[k, i] >= x_ub[i] - act_tol:
                normals.append(Gam[k][i])
            if x[k, i] <= x_lb[i] + act_tol:
                normals.append(-Gam[k][i])
    stat = spo.nnls(np.array(normals).T, -grad)[1] if normals else np.linalg.norm(grad)
    return dict(dyn=dyn, bound=viol, stat=stat / max(1.0, np.linalg.norm(grad)))


def admm(A, B, Q, R, Qf, N, x_lb, x_ub, u_lb, u_ub, x0, xRef, uRef, rho=1.0, eps_abs=1e-5, eps_rel=1e-5, max_iter=10000,
         eps_prim_inf=1e-4, alpha=1.0):
    """NumPy restatement of the tracking kernels for ONE instance (fixed penalty): mpc_oracle.admm with z = -rho (y - lam) + g at the
    top of each backward stage and the dual tolerance eps_abs + eps_rel max(rho |lam|_inf, |g|_inf).  Returns (x, u, status, iters)."""
    n, m = B.shape
    if np.any(x0 < x_lb) or np.any(x0 > x_ub):
        return rollout(A, B, x0, np.zeros((N, m))), np.zeros((N, m)), "infeasible", 0
    gx, gu = linear_term(Q, R, Qf, N, xRef, uRef)
    gn = max(np.max(np.abs(gx)), np.max(np.abs(gu)))
    K, Mi, _ = riccati_tables(np.tile(A, (N, 1, 1)), np.tile(B, (N, 1, 1)), None, np.stack([Q] * (N - 1) + [Qf]), np.stack([R] * N), rho)
    yx, yu = np.zeros((N, n)), np.zeros((N, m))      # yx[k] is the copy of x_{k+1}
    lx, lu = np.zeros((N, n)), np.zeros((N, m))
    status, it = "user_limit", 0
    x, u = None, None
    for it in range(1, max_iter + 1):
        chk = (it % CHECK_EVERY) == 0
        zx, zu = -rho * (yx - lx) + gx, -rho * (yu - lu) + gu
        p = zx[N - 1]
        kf = np.zeros((N, m))
        for k in range(N - 1, -1, -1):
            qu = zu[k] + B.T @ p
            kf[k] = Mi[k] @ qu
            p = (zx[k - 1] if k >= 1 else 0.0) + A.T @ p - K[k].T @ qu
        xs, us = [x0], []
        for k in range(N):
            us.append(-K[k] @ xs[-1] - kf[k])
            xs.append(A @ xs[-1] + B @ us[-1])
        x, u = np.stack(xs), np.stack(us)
        xh, uh = alpha * x[1:] + (1.0 - alpha) * yx, alpha * u + (1.0 - alpha) * yu
        yxn = np.clip(xh + lx, x_lb, x_ub)
        yun = np.clip(uh + lu, u_lb, u_ub)
        rp = max(np.max(np.abs(x[1:] - yxn)), np.max(np.abs(u - yun)))
        rx, ru = xh - yxn, uh - yun
        rd = rho * max(np.max(np.abs(yxn - yx)), np.max(np.abs(yun - yu)))
        lx, lu = lx + rx, lu + ru
        yx, yu = yxn, yun
        ep = eps_abs + eps_rel * max(np.max(np.abs(x[1:])), np.max(np.abs(u)), np.max(np.abs(yx)), np.max(np.abs(yu)))
        ed = eps_abs + eps_rel * max(rho * max(np.max(np.abs(lx)), np.max(np.abs(lu))), gn)
        if rp <= ep and rd <= ed:
            status = "optimal"
            break
        if chk:   # the primal infeasibility certificate does not involve the cost: unchanged
            s = rx[N - 1].copy()
            gmax = 0.0
            for k in range(N - 1, -1, -1):
                gmax = max(gmax, np.max(np.abs(ru[k] + B.T @ s)))
                s = (rx[k - 1] if k >= 1 else 0.0) + A.T @ s
            sup = 0.0
            for r_, lo_, hi_ in ((rx, x_lb, x_ub), (ru, u_lb, u_ub)):
                lo_b, hi_b = np.broadcast_to(lo_, r_.shape), np.broadcast_to(hi_, r_.shape)
                pos, neg = r_ > 0, r_ < 0
                sup += np.sum(r_[pos] * hi_b[pos]) + np.sum(r_[neg] * lo_b[neg])
            dn = max(np.max(np.abs(rx)), np.max(np.abs(ru)))
            if gmax <= eps_prim_inf * dn and (s @ x0 - sup) > eps_prim_inf * dn:
                status = "infeasible"
                break
    return x, u, status, it


# ---- the problems and references the tracking tests share ------------------------------------------------------------------------

def default_rho(Q, R):
    """lqrMpc's penalty (zopt_amd/mpcUtils.py): geometric mean of the cost curvatures"""
    n, m = Q.shape[0], R.shape[0]
    return float(np.sqrt(max(np.trace(2 * Q) / n, 1e-12) * max(np.trace(2 * R) / m, 1e-12)))


def random_case(n, m, N, seed, nb=1):
    """the random stable problem of tests/test_mpc_gpu.py with its tight input bound 0.15, `nb` starts, and references that leave the
    box: a sinusoid of amplitude 6 (state box 4) on every state, a ramp to 0.4 (input box 0.15) on every control"""
    from tests.test_mpc_gpu import _random_problem
    rng = np.random.default_rng(seed)
    A, B, Q, R, Qf = _random_problem(rng, n, m, N)
    x_ub, u_ub = np.full(n, 4.0), np.full(m, 0.15)
    x0 = rng.uniform(-1.0, 1.0, (nb, n))
    t = np.arange(N + 1)
    ph = rng.uniform(0, 2 * np.pi, (nb, 1, n))
    xRef = 6.0 * np.sin(2 * np.pi * t[None, :, None] / N + ph)
    uRef = 0.4 * (t[None, :N, None] / N) * np.sign(rng.standard_normal((nb, 1, m)))
    return (A, B, Q, R, Qf, -x_ub, x_ub, -u_ub, u_ub), x0, xRef, uRef


def quad_data(N):
    """demos/lqrMpc.py data as tests/test_mpc_gpu.py builds it: (A, B, Q, R, Qf, x_lb, x_ub, u_lb, u_ub)"""
    from zopt_amd import mpcUtils
    from tests.test_mpc_gpu import _quad_mpc
    _, (A, B, Q, R, Qf, x_ub, u_ub) = _quad_mpc(mpcUtils, N)
    return A, B, Q, R, Qf, -x_ub, x_ub, -u_ub, u_ub


def quad_reference(N, nb=1, seed=0):
    """hover starts and references that leave the demo's box: a velocity ramp to 2 m/s (box 1 m/s) with the position that goes with
    it (dt = 0.1), a sinusoidal attitude reference of amplitude 0.8 rad (box 0.5) and a sinusoidal thrust reference"""
    rng = np.random.default_rng(seed)
    t = np.arange(N + 1)
    xRef = np.zeros((nb, N + 1, 12))
    v = 2.0 * t / N
    sgn = np.sign(rng.standard_normal((nb, 1)))
    xRef[:, :, 0] = sgn * v
    xRef[:, :, 9] = sgn * np.cumsum(np.concatenate([[0.0], 0.1 * v[:-1]]))
    xRef[:, :, 6] = 0.8 * np.sin(2 * np.pi * t[None, :] / N + rng.uniform(0, 2 * np.pi, (nb, 1)))
    uRef = np.zeros((nb, N, 4))
    uRef[:, :, 0] = 1.0 * np.sin(2 * np.pi * t[None, :N] / N)
    x0 = np.zeros((nb, 12))
    x0[:, 9:12] = rng.uniform(-0.5, 0.5, (nb, 3))
    return x0, xRef, uRef
