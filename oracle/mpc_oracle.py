"""CPU checkers for the box-constrained LQ-MPC path (TEST INFRASTRUCTURE ONLY).

The reference (zopt/mpcUtils.py:12-81) states the QP and hands it to cvxpy -> OSQP 1.0.4 (requirements.txt:13,52);
that solver is not part of the reference tree and not installed here, and the reference's own test pins only
`status == "optimal"` (tests/test_mpcUtils.py:23): NUMERIC PARITY IS UNPINNED for this row.  What is checked instead:

  * `kkt_residuals`      -- solver-independent optimality certificate of a candidate (x, u) for the QP of
                            mpcUtils.py:48-59 (dynamics, bounds, and the reduced-gradient / complementarity
                            condition in the condensed variables);
  * `solve_reference`    -- an independent high-accuracy solve (condensed QP, SciPy trust-constr) for small problems;
  * `riccati_tables`     -- the NumPy restatement of the setup kernels' tables K, Minv, D (one problem, one penalty, stage form), which
                            `admm` and `admm_levels_stage` use and tests/test_mpc_tables*.py hold to a long-double reference;
  * `admm`               -- a NumPy restatement of the build's own ADMM (zopt_amd/csrc/mpc.hip) for iterate-level checks;
  * `admm_levels_stage`  -- the restatement of the WHOLE solve, once for every MPC family (stage-varying dynamics, weights and boxes,
                            soft components): adaptive penalty levels, warm and shifted starts, the linear term and the cycle guard, the
                            stored state.  `admm_levels` (zopt_amd/csrc/mpc_solve_wave_body.h, lqrMpc's data) and the admm_levels_ltv*
                            of tests/mpc_ltv*_ref.py are its adapters;
  * `kkt_residuals_stage` -- `kkt_residuals` in the data of `admm_levels_stage` (stage-varying dynamics with offsets, weights and boxes);
  * `solve_reference_stage` -- the independent condensed solve of the LTV families in the same data, slacks for the soft components.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import scipy.optimize as spo

CHECK_EVERY = 8   # zopt_amd/csrc/mpc_common.h ZM_MPC_CHK: iterations between infeasibility-certificate checks


def condense(A, B, Q, R, Qf, N, x0):
    """x_k = Phi_k x0 + sum_j Gam[k,j] u_j ;  cost = u'Hu + 2 g'u + c  in the stacked control vector u (N*m)."""
    n, m = B.shape
    Phi = [np.eye(n)]
    for _ in range(N):
        Phi.append(A @ Phi[-1])
    Gam = np.zeros((N + 1, n, N * m))
    for k in range(1, N + 1):
        for j in range(k):
            Gam[k][:, j * m:(j + 1) * m] = Phi[k - 1 - j] @ B
    H = np.zeros((N * m, N * m))
    g = np.zeros(N * m)
    c = 0.0
    for k in range(N + 1):
        W = Qf if k == N else Q
        xk0 = Phi[k] @ x0
        H += Gam[k].T @ W @ Gam[k]
        g += Gam[k].T @ (0.5 * (W + W.T)) @ xk0
        c += xk0 @ W @ xk0
    for k in range(N):
        H[k * m:(k + 1) * m, k * m:(k + 1) * m] += R
    return Phi, Gam, H, g, c


def rollout(A, B, x0, u):
    x = [np.asarray(x0, dtype=np.float64)]
    for k in range(u.shape[0]):
        x.append(A @ x[-1] + B @ u[k])
    return np.stack(x)


def cost(Q, R, Qf, x, u):
    """mpcUtils.py:52-54."""
    return sum(x[k] @ Q @ x[k] + u[k] @ R @ u[k] for k in range(u.shape[0])) + x[-1] @ Qf @ x[-1]


def solve_reference(A, B, Q, R, Qf, N, x_lb, x_ub, u_lb, u_ub, x0):
    """Independent reference: condensed QP in u with linear inequality constraints on the states, SciPy trust-constr."""
    n, m = B.shape
    Phi, Gam, H, g, c = condense(A, B, Q, R, Qf, N, x0)
    Hs = H + H.T
    fun = lambda u: u @ H @ u + 2 * g @ u + c
    jac = lambda u: Hs @ u + 2 * g
    rows, lo, hi = [], [], []
    for k in range(1, N + 1):
        for i in range(n):
            if np.isfinite(x_lb[i]) or np.isfinite(x_ub[i]):
                rows.append(Gam[k][i])
                off = (Phi[k] @ x0)[i]
                lo.append(x_lb[i] - off)
                hi.append(x_ub[i] - off)
    cons = [spo.LinearConstraint(np.array(rows), np.array(lo), np.array(hi))] if rows else []
    bounds = spo.Bounds(np.tile(u_lb, N), np.tile(u_ub, N))
    res = spo.minimize(fun, np.zeros(N * m), jac=jac, hess=lambda u: Hs, method="trust-constr", bounds=bounds,
                       constraints=cons, options=dict(gtol=1e-12, xtol=1e-14, barrier_tol=1e-14, maxiter=5000))
    u = res.x.reshape(N, m)
    return rollout(A, B, x0, u), u, res.fun


def kkt_residuals(A, B, Q, R, Qf, N, x_lb, x_ub, u_lb, u_ub, x0, x, u, act_tol=1e-6):
    """Solver-independent certificate for a candidate (x (N+1,n), u (N,m)).

    Returns dict(dyn, bound, stat): max dynamics defect, max bound violation, and the stationarity defect: the norm
    of the projection of the reduced gradient (condensed variables) onto the cone of feasible directions of the
    constraints that are inactive / active at the candidate -- computed by a small non-negative least squares."""
    n, m = B.shape
    dyn = max(np.max(np.abs(x[k + 1] - (A @ x[k] + B @ u[k]))) for k in range(N))
    dyn = max(dyn, np.max(np.abs(x[0] - x0)))
    viol = max(np.max(np.maximum(x_lb - x, 0)), np.max(np.maximum(x - x_ub, 0)), np.max(np.maximum(u_lb - u, 0)),
               np.max(np.maximum(u - u_ub, 0)))
    Phi, Gam, H, g, c = condense(A, B, Q, R, Qf, N, x0)
    uv = u.reshape(-1)
    grad = (H + H.T) @ uv + 2 * g
    # active constraint normals (outward): grad + sum mu_i a_i = 0 with mu >= 0
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
    if normals:
        Nm = np.array(normals).T
        mu, rnorm = spo.nnls(Nm, -grad)
        stat = rnorm
    else:
        stat = np.linalg.norm(grad)
    return dict(dyn=dyn, bound=viol, stat=stat / max(1.0, np.linalg.norm(grad)))


def riccati_tables(A, B, c, Qs, Rs, rho):
    """The tables of the setup kernels (zopt_amd/csrc/mpc_setup_body.h and its two stage-varying copies in mpc.hip) for ONE problem at ONE
    penalty, in the stage form zm_mpc_setup_ltv_stage_f64 documents: A (N, n, n), B (N, n, m), c (N, n) or None (zeros), Qs (N, n, n) with
    Qs[k] the weight of x_{k+1} (row N - 1 is terminal), Rs (N, m, m); the weights are symmetric.

        P_N = 2 Qs_{N-1} + rho I;   k = N-1 .. 0:   D_k = P_{k+1} c_k;   Suu_k = 2 Rs_k + rho I + B_k' P B_k;   Minv_k = Suu_k^-1;
        K_k = Minv_k B_k' P A_k;    P <- sym((2 Qs_{k-1} + rho I) + A_k' P A_k - (B_k' P A_k)' K_k),   sym(X) = (X + X') / 2

    (the update that leaves stage 0 is read by nothing).  The value matrix is symmetrised whenever it is stored: the update's antisymmetric
    rounding error is propagated through A . A_cl rather than A_cl . A_cl, so on an open-loop-unstable plant it grows along the horizon
    unless it is removed at every stage.  Returns (K (N, m, n), Minv (N, m, m), D (N, n))."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    N, n, m = B.shape
    c = np.zeros((N, n)) if c is None else np.asarray(c, dtype=np.float64)
    P = 2 * Qs[N - 1] + rho * np.eye(n)
    K, Mi, D = np.empty((N, m, n)), np.empty((N, m, m)), np.empty((N, n))
    for k in range(N - 1, -1, -1):
        D[k] = P @ c[k]
        Suu = (2 * Rs[k] + rho * np.eye(m)) + B[k].T @ P @ B[k]
        Sux = B[k].T @ P @ A[k]
        Mi[k] = np.linalg.inv(Suu)
        K[k] = Mi[k] @ Sux
        P = (2 * Qs[max(k - 1, 0)] + rho * np.eye(n)) + A[k].T @ P @ A[k] - Sux.T @ K[k]
        P = 0.5 * (P + P.T)
    return K, Mi, D


def admm(A, B, Q, R, Qf, N, x_lb, x_ub, u_lb, u_ub, x0, rho=1.0, eps_abs=1e-5, eps_rel=1e-5, max_iter=10000,
         eps_prim_inf=1e-4, alpha=1.0):
    """NumPy restatement of zopt_amd/csrc/mpc.hip for ONE instance (fixed penalty).  `alpha` is OSQP's over-relaxation: the
    relaxed iterate alpha w + (1 - alpha) y_prev enters the projection and the dual update.  Returns (x, u, status, iters)."""
    n, m = B.shape
    if np.any(x0 < x_lb) or np.any(x0 > x_ub):
        return rollout(A, B, x0, np.zeros((N, m))), np.zeros((N, m)), "infeasible", 0
    K, Mi, _ = riccati_tables(np.tile(A, (N, 1, 1)), np.tile(B, (N, 1, 1)), None, np.stack([Q] * (N - 1) + [Qf]), np.stack([R] * N), rho)
    yx, yu = np.zeros((N, n)), np.zeros((N, m))      # yx[k] is the copy of x_{k+1}
    lx, lu = np.zeros((N, n)), np.zeros((N, m))
    status, it = "user_limit", 0
    x, u = None, None
    for it in range(1, max_iter + 1):
        chk = (it % CHECK_EVERY) == 0
        zx, zu = yx - lx, yu - lu
        p = -rho * zx[N - 1]
        kf = np.zeros((N, m))
        for k in range(N - 1, -1, -1):
            qu = -rho * zu[k] + B.T @ p
            kf[k] = Mi[k] @ qu
            p = (-rho * zx[k - 1] if k >= 1 else 0.0) + A.T @ p - K[k].T @ qu
        xs = [x0]
        us = []
        for k in range(N):
            us.append(-K[k] @ xs[-1] - kf[k])
            xs.append(A @ xs[-1] + B @ us[-1])
        x, u = np.stack(xs), np.stack(us)
        xh, uh = alpha * x[1:] + (1.0 - alpha) * yx, alpha * u + (1.0 - alpha) * yu     # relaxed iterates (alpha = 1: x, u)
        yxn = np.clip(xh + lx, x_lb, x_ub)
        yun = np.clip(uh + lu, u_lb, u_ub)
        rp = max(np.max(np.abs(x[1:] - yxn)), np.max(np.abs(u - yun)))                 # primal residual of the actual iterate
        rx, ru = xh - yxn, uh - yun                                                     # dual step
        rd = rho * max(np.max(np.abs(yxn - yx)), np.max(np.abs(yun - yu)))
        lx, lu = lx + rx, lu + ru
        yx, yu = yxn, yun
        ep = eps_abs + eps_rel * max(np.max(np.abs(x[1:])), np.max(np.abs(u)), np.max(np.abs(yx)), np.max(np.abs(yu)))
        ed = eps_abs + eps_rel * rho * max(np.max(np.abs(lx)), np.max(np.abs(lu)))
        if rp <= ep and rd <= ed:
            status = "optimal"
            break
        if chk:   # OSQP-style primal infeasibility certificate on v = w - y
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


def stage_form(Q, R, Qf, N, x_lb, x_ub, u_lb, u_ub):
    """one set of weights and bounds as constant rows: (Qs (N,n,n), Rs (N,m,m), x_lb (N+1,n), x_ub, u_lb (N,m), u_ub)"""
    Qs = np.stack([Q] * (N - 1) + [Qf])
    rows = lambda v, r: np.tile(np.asarray(v, dtype=np.float64), (r, 1))
    return Qs, np.stack([R] * N), rows(x_lb, N + 1), rows(x_ub, N + 1), rows(u_lb, N), rows(u_ub, N)


def stage_args(Q, R, Qf, N, x_lb, x_ub, u_lb, u_ub):
    """`stage_form` in the argument order of the stage functions: Qs, Rs, N, then the boxes"""
    st = stage_form(Q, R, Qf, N, x_lb, x_ub, u_lb, u_ub)
    return (*st[:2], N, *st[2:])


def linear_term_stage(Qs, Rs, N, xRef, uRef):
    """g in the kernels' stage layout: gx[k] = -(Qs_k + Qs_k') xr_{k+1}, gu[k] = -(Rs_k + Rs_k') ur_k"""
    gx = np.stack([-(Qs[k] + Qs[k].T) @ xRef[k + 1] for k in range(N)])
    gu = np.stack([-(Rs[k] + Rs[k].T) @ uRef[k] for k in range(N)])
    return gx, gu


def cost_stage(Qs, Rs, x, u, xRef, uRef):
    dx, du = x - xRef, u - uRef
    return sum(dx[k + 1] @ Qs[k] @ dx[k + 1] + du[k] @ Rs[k] @ du[k] for k in range(u.shape[0]))


def rollout_ltv(A, B, c, x0, u):
    x = [np.asarray(x0, dtype=np.float64)]
    for k in range(u.shape[0]):
        x.append(A[k] @ x[-1] + B[k] @ u[k] + c[k])
    return np.stack(x)


def violation(x, u, x_lb, x_ub, u_lb, u_ub):
    """the distance d of every (stage, stacked component) of [x_{k+1} ; u_k] from its box: (N, n + m)"""
    w, lo, hi = np.hstack([x[1:], u]), np.hstack([x_lb[1:], u_lb]), np.hstack([x_ub[1:], u_ub])
    return np.maximum(0.0, np.maximum(w - hi, lo - w))


def prox(v, lo, hi, t, a):
    """the y-update of zm_mpc_solve_ltv_soft_f64, written with its selects: t = l1 / rho, a = rho / (rho + 2 l2); t = +inf is the clip"""
    with np.errstate(invalid="ignore"):
        eh, el = a * ((v - hi) - t), a * ((lo - v) - t)
        return np.where(v > hi, np.where(eh > 0, hi + eh, hi), np.where(v < lo, np.where(el > 0, lo - el, lo), v))


def admm_levels_stage(A, B, c, Qs, Rs, N, x_lb, x_ub, u_lb, u_ub, x0, l1=None, l2=None, rho=1.0, eps_abs=1e-5, eps_rel=1e-5,
                      max_iter=10000, eps_prim_inf=1e-4, alpha=1.6, n_levels=7, rho_step=5.0, g=None, warm=None, shift=False, guard=True):
    """NumPy restatement of ONE instance of the solve kernels, every family in its most general data: the one body that `admm_levels`
    (zopt_amd/csrc/mpc_solve_wave_body.h and, with n_levels=1, mpc_solve_lane_body.h), tests/mpc_ltv_ref.py: admm_levels_ltv
    (mpc_solve_wave_ltv.h), tests/mpc_ltv_stage_ref.py: admm_levels_ltv_stage (zm_mpc_solve_ltv_stage_f64) and
    tests/mpc_ltv_soft_ref.py: admm_levels_ltv_soft (zm_mpc_solve_ltv_soft_f64) are adapters of.  In the kernels' order: backward sweep
    with z = -rho (y - lam) + g, rollout, relaxed iterate / projection / dual step / norms, termination test, then at every
    CHECK_EVERY-th iteration of an instance that goes on: the level rule (cycle guard first when it is on), then the primal infeasibility
    certificate on the dual step of that iteration.

    The data: A (N, n, n), B (N, n, m), c (N, n) or None (zeros): x+ = A_k x + B_k u + c_k.  Qs (N, n, n) with Qs[k] the weight of
    x_{k+1} (row N - 1 is terminal), Rs (N, m, m).  x_lb, x_ub (N + 1, n) -- row 0 is the test on x0 -- and u_lb, u_ub (N, m).
    l1, l2 (n + m,): the weights of the penalty l1 d + l2 d^2 on the distance d of a component of [x_{k+1} ; u_k] from its box, constant
    over the stages; l1 = +inf is a hard component, l1 None: all hard, l2 None: zeros.

    rho is the penalty of level `n_levels // 2`; level l runs rho * rho_step ** (l - n_levels // 2).  n_levels = 1: fixed penalty.
    g = (gx (N, n), gu (N, m)): the linear term of a tracking cost (`linear_term_stage`), None = 0.
    warm = (y (N, n + m), lam (N, n + m), level): the state a previous solve returned (the kernels keep it only after "optimal");
    shift: stage k starts from stage k + 1 of it, the last stage from itself.  guard=False switches the cycle guard off (tests only).

    What each generalisation does, as the kernels spell it:
        tables:      the recursion of mpc_setup_body.h with A_k, B_k:  P_N = 2 Qs_{N-1} + rho I;  Suu_k = 2 Rs_k + rho I + B_k' P B_k;
                     the value update leaving stage k >= 1 adds 2 Qs_{k-1} + rho I (the one leaving stage 0 is read by nothing);
                     D_k = P_{k+1} c_k from the value matrix on entering stage k
        backward:    p = p' + z_x + g_x + D_k;  Qu = z_u + g_u + B_k' p;  kf = Suu_k^-1 Qu;  p' = A_k' p - K_k' Qu
        forward:     u = -K_k x - kf;  x+ = A_k x + B_k u + c_k
        x0 test:     against row 0 of the state box; a soft state component (finite l1) is not tested
        projection:  [x_{k+1} ; u_k] into [x_lb[k+1] ; u_lb[k]], [x_ub[k+1] ; u_ub[k]] by the proximal map `prox` of the penalty, its
                     thresholds t = l1 / rho, a = rho / (rho + 2 l2) at the penalty the iteration runs at (a hard component: the clip)
        certificate: v.w(u=0) = s_0.x0 + sum_k sigma_k.c_k, sigma_k the adjoint vector on entering stage k of the adjoint sweep; the
                     support term with the stage's own bounds, a soft component with the bounds -inf / +inf
        guard:       on when g != 0, or c != 0, or any component is soft (and `guard`)
    The dual tolerance scales with max(rho |lam|, |g|): c does not enter it.

    The guard as the kernel spells it (mpc_wave.hip: ZM_TRK_LEVEL): a wanted move opposite in sign to the decision of the check before
    is a reversal; the third reversal in a row is refused and the level locked for the rest of the solve; any other decision (a
    decision not to move included, which also clears the remembered move) resets the count.

    No level move is taken at iteration max_iter: no iteration follows it, and the returned (x, u) is the rollout of the last iterate
    at the penalty that iterate was computed with.

    Returns a namespace: x (N+1, n), u (N, m), status, iters, rp, rd (of the last iteration), y, lam (N, n+m: [x_{k+1} ; u_k]), level,
    rho_final, moves [(iteration, from, to)], locked, and the decision margins of the run: level_margin = min over the level decisions
    of the distance of log(want) / log(rho_step) from the nearest half-integer, stop_margin = min over the iterations of
    |max(rp / ep, rd / ed) - 1|, near_margin = |max(rp / ep, rd / ed) / 10 - 1| of the last iteration (the test at the cap)."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    n, m = B.shape[-2:]
    c = np.zeros((N, n)) if c is None else np.asarray(c, dtype=np.float64)
    assert A.shape == (N, n, n) and B.shape == (N, n, m) and c.shape == (N, n)
    assert Qs.shape == (N, n, n) and Rs.shape == (N, m, m)
    assert x_lb.shape == x_ub.shape == (N + 1, n) and u_lb.shape == u_ub.shape == (N, m)
    l1 = np.full(n + m, np.inf) if l1 is None else np.asarray(l1, dtype=np.float64)
    l2 = np.zeros(n + m) if l2 is None else np.asarray(l2, dtype=np.float64)
    assert l1.shape == l2.shape == (n + m,) and np.all(l1 >= 0) and np.all(l2 >= 0) and not np.any((l2 > 0) & np.isinf(l1))
    l1x, l1u, l2x, l2u = l1[:n], l1[n:], l2[:n], l2[n:]
    soft_x, soft_u = np.isfinite(l1x), np.isfinite(l1u)
    xl, xu = x_lb[1:], x_ub[1:]
    # the bounds the certificate sees
    cxl, cxu = np.where(soft_x, -np.inf, xl), np.where(soft_x, np.inf, xu)
    cul, cuu = np.where(soft_u, -np.inf, u_lb), np.where(soft_u, np.inf, u_ub)
    level0 = n_levels // 2
    rho0 = float(rho)
    tabs = {}

    def tables(l):   # K_k, Suu_k^-1, D_k at the level's penalty (`riccati_tables`)
        if l not in tabs:
            r_ = rho0 * rho_step ** (l - level0)
            tabs[l] = (r_, *riccati_tables(A, B, c, Qs, Rs, r_))
        return tabs[l]

    lvl = level0
    yx, yu, lx, lu = np.zeros((N, n)), np.zeros((N, m)), np.zeros((N, n)), np.zeros((N, m))
    if warm is not None:
        wy, wl, wlvl = warm
        if n_levels > 1 and 0 <= int(wlvl) < n_levels:
            lvl = int(wlvl)
        ks = [k + 1 if (shift and k + 1 < N) else k for k in range(N)]
        wy, wl = np.asarray(wy, dtype=np.float64)[ks], np.asarray(wl, dtype=np.float64)[ks]
        yx, yu, lx, lu = wy[:, :n].copy(), wy[:, n:].copy(), wl[:, :n].copy(), wl[:, n:].copy()
    if g is None:
        gx, gu = np.zeros((N, n)), np.zeros((N, m))
    else:
        gx, gu = np.asarray(g[0], dtype=np.float64), np.asarray(g[1], dtype=np.float64)
    gn = max(np.max(np.abs(gx)), np.max(np.abs(gu)))
    guard_on = bool(guard) and (gn > 0.0 or np.max(np.abs(c)) > 0.0 or bool(np.any(soft_x) or np.any(soft_u)))
    rho_l, K, Mi, D = tables(lvl)
    kf = np.zeros((N, m))

    def roll(K, kf):
        xs, us = [np.asarray(x0, dtype=np.float64)], []
        for k in range(N):
            us.append(-K[k] @ xs[-1] - kf[k])
            xs.append(A[k] @ xs[-1] + B[k] @ us[-1] + c[k])
        return np.stack(xs), np.stack(us)

    out = SimpleNamespace(moves=[], locked=False, level_margin=np.inf, stop_margin=np.inf, near_margin=np.inf, rp=0.0, rd=0.0)
    status, it, near_ok = None, 0, False
    x, u = roll(K, kf)
    if np.any((x0 < x_lb[0]) & ~soft_x) or np.any((x0 > x_ub[0]) & ~soft_x):
        status = "infeasible"
    last, rev = 0, 0
    while status is None and it < max_iter:
        it += 1
        chk = (it % CHECK_EVERY) == 0
        zx, zu = -rho_l * (yx - lx) + gx, -rho_l * (yu - lu) + gu
        p = zx[N - 1] + D[N - 1]
        for k in range(N - 1, -1, -1):
            qu = zu[k] + B[k].T @ p
            kf[k] = Mi[k] @ qu
            p = ((zx[k - 1] + D[k - 1]) if k >= 1 else 0.0) + A[k].T @ p - K[k].T @ qu
        x, u = roll(K, kf)
        xh, uh = alpha * x[1:] + (1.0 - alpha) * yx, alpha * u + (1.0 - alpha) * yu
        yxn = prox(xh + lx, xl, xu, l1x / rho_l, rho_l / (rho_l + 2.0 * l2x))
        yun = prox(uh + lu, u_lb, u_ub, l1u / rho_l, rho_l / (rho_l + 2.0 * l2u))
        rp = max(np.max(np.abs(x[1:] - yxn)), np.max(np.abs(u - yun)))
        rx, ru = xh - yxn, uh - yun
        nrd = max(np.max(np.abs(yxn - yx)), np.max(np.abs(yun - yu)))
        rd = rho_l * nrd
        lx, lu = lx + rx, lu + ru
        yx, yu = yxn, yun
        nwy = max(np.max(np.abs(x[1:])), np.max(np.abs(u)), np.max(np.abs(yx)), np.max(np.abs(yu)))
        nl = max(np.max(np.abs(lx)), np.max(np.abs(lu)))
        ep = eps_abs + eps_rel * nwy
        ed = eps_abs + eps_rel * rho_l * nl
        if gn > rho_l * nl:
            ed = eps_abs + eps_rel * gn
        out.rp, out.rd = rp, rd
        near_ok = bool(rp <= 10.0 * ep and rd <= 10.0 * ed)
        if rp == rp:
            worst = max(rp / ep, rd / ed)
            out.stop_margin = min(out.stop_margin, abs(worst - 1.0))
            out.near_margin = abs(worst / 10.0 - 1.0)
        if rp <= ep and rd <= ed:
            status = "optimal"
            break
        if not (rp == rp):
            break                      # NaN iterates: the limit status
        if not chk:
            continue
        if n_levels > 1 and it < max_iter:
            tiny = 1e-300
            rpn = rp / max(nwy, tiny)
            rdn = rd / max(rho_l * nl, tiny)
            want = np.sqrt(rpn / max(rdn, tiny))
            dl = 0
            if want == want and want > 0.0:
                t = np.log(want) / np.log(rho_step)
                dl = int(np.rint(t))
                out.level_margin = min(out.level_margin, abs(abs(t - np.floor(t)) - 0.5))
            new = min(max(lvl + dl, 0), n_levels - 1)
            if guard_on:
                mv = new - lvl
                if out.locked:
                    new = lvl
                elif mv != 0 and last != 0 and ((mv > 0) != (last > 0)):
                    rev += 1
                    if rev >= 3:
                        out.locked = True
                        new = lvl
                else:
                    rev = 0
                last = new - lvl
            if new != lvl:
                out.moves.append((it, lvl, new))
                r_new, K, Mi, D = tables(new)
                sc = rho_l / r_new
                lx, lu = lx * sc, lu * sc
                rho_l, lvl = r_new, new
        # OSQP-style primal infeasibility certificate on the dual step of this iteration
        s = rx[N - 1].copy()
        gmax, vc = 0.0, 0.0
        for k in range(N - 1, -1, -1):
            vc += s @ c[k]
            gmax = max(gmax, np.max(np.abs(ru[k] + B[k].T @ s)))
            s = (rx[k - 1] if k >= 1 else 0.0) + A[k].T @ s
        sup = 0.0
        for r_, lo_, hi_ in ((rx, cxl, cxu), (ru, cul, cuu)):
            pos, neg = r_ > 0, r_ < 0
            sup += np.sum(r_[pos] * hi_[pos]) + np.sum(r_[neg] * lo_[neg])
        dn = max(np.max(np.abs(rx)), np.max(np.abs(ru)))
        if gmax <= eps_prim_inf * dn and (s @ x0 + vc - sup) > eps_prim_inf * dn:
            status = "infeasible"
    if status is None:
        status = "optimal_inaccurate" if near_ok else "user_limit"
    out.x, out.u, out.status, out.iters = x, u, status, it
    out.y, out.lam, out.level, out.rho_final = np.hstack([yx, yu]), np.hstack([lx, lu]), lvl, rho_l
    return out


def kkt_residuals_stage(A, B, c, Qs, Rs, N, x_lb, x_ub, u_lb, u_ub, x0, x, u, act_tol=1e-6):
    """`kkt_residuals` for the data of `admm_levels_stage` (hard bounds, no reference): dict(dyn, bound, stat) of a candidate (x (N+1, n),
    u (N, m)) -- the largest defect of x+ = A_k x + B_k u + c_k, the largest violation of the stage's own bounds (row 0 of the state box
    is not tested), and the distance of the reduced gradient from the cone of the active constraints' normals, relative to max(1, |grad|).
    The gradient by the adjoint sweep lam_N = 2 Qs_{N-1} x_N, grad_k = 2 Rs_k u_k + B_k' lam_{k+1}, lam_k = 2 Qs_{k-1} x_k + A_k' lam_{k+1}."""
    n, m = B.shape[-2:]
    c = np.zeros((N, n)) if c is None else c
    dyn = max(np.max(np.abs(x[0] - x0)), max(np.max(np.abs(x[k + 1] - (A[k] @ x[k] + B[k] @ u[k] + c[k]))) for k in range(N)))
    viol = float(np.max(violation(x, u, x_lb, x_ub, u_lb, u_ub)))
    Gam = [np.zeros((n, N * m))]
    for k in range(N):
        G = A[k] @ Gam[-1]
        G[:, k * m:(k + 1) * m] += B[k]
        Gam.append(G)
    grad = np.zeros((N, m))
    lam = (Qs[N - 1] + Qs[N - 1].T) @ x[N]
    for k in range(N - 1, -1, -1):
        grad[k] = (Rs[k] + Rs[k].T) @ u[k] + B[k].T @ lam
        lam = ((Qs[k - 1] + Qs[k - 1].T) @ x[k] if k >= 1 else 0.0) + A[k].T @ lam
    grad = grad.reshape(-1)
    normals = []
    for k in range(N):
        for j in range(m):
            e = np.zeros(N * m)
            e[k * m + j] = 1.0
            if u[k, j] >= u_ub[k, j] - act_tol:
                normals.append(e)
            if u[k, j] <= u_lb[k, j] + act_tol:
                normals.append(-e)
    for k in range(1, N + 1):
        for i in range(n):
            if x[k, i] >= x_ub[k, i] - act_tol:
                normals.append(Gam[k][i])
            if x[k, i] <= x_lb[k, i] + act_tol:
                normals.append(-Gam[k][i])
    stat = spo.nnls(np.array(normals).T, -grad)[1] if normals else np.linalg.norm(grad)
    return dict(dyn=dyn, bound=viol, stat=stat / max(1.0, np.linalg.norm(grad)))


def admm_levels(A, B, Q, R, Qf, N, x_lb, x_ub, u_lb, u_ub, x0, rho=1.0, eps_abs=1e-5, eps_rel=1e-5, max_iter=10000, eps_prim_inf=1e-4,
                alpha=1.6, n_levels=7, rho_step=5.0, g=None, warm=None, shift=False, guard=True):
    """`admm_levels_stage` (see there for the options, the order of an iteration and the returned namespace) for the time-invariant
    solve of lqrMpc: A (n, n), B (n, m) tiled over the stages, c = 0, one set of weights and bounds as constant rows, every component
    hard.  g: tests/mpc_tracking_ref.py: linear_term.  The guard is then on when g != 0, as in the tracking kernels."""
    return admm_levels_stage(np.tile(A, (N, 1, 1)), np.tile(B, (N, 1, 1)), None, *stage_args(Q, R, Qf, N, x_lb, x_ub, u_lb, u_ub), x0,
                             None, None, rho, eps_abs, eps_rel, max_iter, eps_prim_inf, alpha, n_levels, rho_step, g, warm, shift, guard)


def solve_reference_stage(A, B, c, Qs, Rs, N, x_lb, x_ub, u_lb, u_ub, x0, l1=None, l2=None, xRef=None, uRef=None):
    """Independent reference for the data of `admm_levels_stage`: x_k = phi_k + Gam_k u with the offsets inside the free response phi,
    the cost (about the references, zero if None) with the stage's own weights condensed in u, the stage's own bounds as linear
    constraints on the states (rows with a finite side only) and as bounds on the inputs, and one slack e >= 0 per soft (stage,
    component) that has a finite bound: lo - e <= w <= hi + e, cost + l1 e + l2 e^2; a soft input gets slacks instead of Bounds.  With no
    soft component this is the QP in u alone.  SciPy trust-constr.  x0 is not tested against row 0 here.  Returns (x, u, cost with the
    penalty)."""
    n, m = B.shape[-2:]
    c = np.zeros((N, n)) if c is None else c
    l1 = np.full(n + m, np.inf) if l1 is None else np.asarray(l1, dtype=np.float64)
    l2 = np.zeros(n + m) if l2 is None else np.asarray(l2, dtype=np.float64)
    xRef = np.zeros((N + 1, n)) if xRef is None else xRef
    uRef = np.zeros((N, m)) if uRef is None else uRef
    phi = [np.asarray(x0, dtype=np.float64)]
    Gam = [np.zeros((n, N * m))]
    for k in range(N):
        phi.append(A[k] @ phi[-1] + c[k])
        G = A[k] @ Gam[-1]
        G[:, k * m:(k + 1) * m] += B[k]
        Gam.append(G)
    H, gv = np.zeros((N * m, N * m)), np.zeros(N * m)
    for k in range(1, N + 1):
        Ws = 0.5 * (Qs[k - 1] + Qs[k - 1].T)
        H += Gam[k].T @ Ws @ Gam[k]
        gv += Gam[k].T @ Ws @ (phi[k] - xRef[k])
    for k in range(N):
        Rk = 0.5 * (Rs[k] + Rs[k].T)
        H[k * m:(k + 1) * m, k * m:(k + 1) * m] += Rk
        gv[k * m:(k + 1) * m] -= Rk @ uRef[k]
    # rows over u alone, each with its bounds and, soft, its weights: the slacks are numbered as the soft rows come
    rows = []    # (row over u, lo, hi, l1, l2)
    ulo, uhi = u_lb.reshape(-1).copy(), u_ub.reshape(-1).copy()
    for k in range(1, N + 1):
        for i in range(n):
            if np.isfinite(x_lb[k, i]) or np.isfinite(x_ub[k, i]):
                rows.append((Gam[k][i], x_lb[k, i] - phi[k][i], x_ub[k, i] - phi[k][i], l1[i], l2[i]))
    for k in range(N):
        for j in range(m):
            if np.isfinite(l1[n + j]) and (np.isfinite(u_lb[k, j]) or np.isfinite(u_ub[k, j])):
                e_ = np.zeros(N * m)
                e_[k * m + j] = 1.0
                rows.append((e_, u_lb[k, j], u_ub[k, j], l1[n + j], l2[n + j]))
                ulo[k * m + j], uhi[k * m + j] = -np.inf, np.inf
    ns = sum(1 for r in rows if np.isfinite(r[3]))
    nv = N * m + ns
    Cm, lo, hi = [], [], []
    w1, w2 = np.zeros(ns), np.zeros(ns)
    j = 0
    for row, lo_, hi_, a1, a2 in rows:
        if not np.isfinite(a1):
            Cm.append(np.concatenate([row, np.zeros(ns)]))
            lo.append(lo_)
            hi.append(hi_)
            continue
        e_ = np.zeros(ns)
        e_[j] = 1.0
        w1[j], w2[j] = a1, a2
        j += 1
        if np.isfinite(lo_):
            Cm.append(np.concatenate([row, e_]))
            lo.append(lo_)
            hi.append(np.inf)
        if np.isfinite(hi_):
            Cm.append(np.concatenate([row, -e_]))
            lo.append(-np.inf)
            hi.append(hi_)
    Hf = np.zeros((nv, nv))
    Hf[:N * m, :N * m] = H
    Hf[N * m:, N * m:] = np.diag(w2)
    gf = np.concatenate([gv, 0.5 * w1])
    cons = [spo.LinearConstraint(np.array(Cm), np.array(lo), np.array(hi))] if Cm else []
    bounds = spo.Bounds(np.concatenate([ulo, np.zeros(ns)]), np.concatenate([uhi, np.full(ns, np.inf)]))
    res = spo.minimize(lambda v: v @ Hf @ v + 2 * gf @ v, np.zeros(nv), jac=lambda v: 2 * (Hf @ v + gf), hess=lambda v: 2 * Hf,
                       method="trust-constr", bounds=bounds, constraints=cons,
                       options=dict(gtol=1e-12, xtol=1e-14, barrier_tol=1e-14, maxiter=5000))
    u = res.x[:N * m].reshape(N, m)
    x = rollout_ltv(A, B, c, x0, u)
    d = violation(x, u, x_lb, x_ub, u_lb, u_ub)
    fin = np.isfinite(l1)
    pen = np.sum(d[:, fin] * l1[fin] + d[:, fin] ** 2 * l2[fin])
    return x, u, cost_stage(Qs, Rs, x, u, xRef, uRef) + pen
