"""CPU checkers and cases for mpcUtils.ltvMpc with stage_varying= (per-stage weights Q_k, R_k and per-stage boxes on top of the stage-varying
dynamics); a helper module, not collected as a test.

Stage form, as the kernels take it (zm_mpc_setup_ltv_stage_f64, zm_mpc_solve_ltv_stage_f64): Qs (N, n, n) with Qs[k] the weight of
x_{k+1} (row N - 1 is terminal), Rs (N, m, m), and the box as the constructor takes it, x_lb, x_ub (N + 1, n) -- row 0 is the test on x0 --
and u_lb, u_ub (N, m).

  * `admm_levels_ltv_stage`     -- tests/mpc_ltv_ref.py: admm_levels_ltv restated with per-stage weights in the tables and per-stage boxes in
                                   the clip, the x0 test and the support term of the certificate.  Same options and returned namespace.
  * `solve_reference_ltv_stage` -- the condensed SciPy trust-constr solve with per-stage weights and bounds.
  * the named cases of tests/test_mpc_ltv_stage.py (their decisions and their non-vacuity are checked there, without a GPU) and
    tests/test_mpc_ltv_stage_gpu.py, with `reference`, `run_steps` and the comparison rule of tests/mpc_ltv_ref.py.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np
import scipy.optimize as spo

from oracle.mpc_oracle import CHECK_EVERY
from tests import mpc_iterates_cases as mc
from tests import mpc_ltv_ref as lr

ALL_SIX = ("Q", "R", "x_lb", "x_ub", "u_lb", "u_ub")


def stage_form(Q, R, Qf, N, x_lb, x_ub, u_lb, u_ub):
    """one set of weights and bounds as constant rows: (Qs (N,n,n), Rs (N,m,m), x_lb (N+1,n), x_ub, u_lb (N,m), u_ub)"""
    Qs = np.stack([Q] * (N - 1) + [Qf])
    rows = lambda v, r: np.tile(np.asarray(v, dtype=np.float64), (r, 1))
    return Qs, np.stack([R] * N), rows(x_lb, N + 1), rows(x_ub, N + 1), rows(u_lb, N), rows(u_ub, N)


def linear_term_stage(Qs, Rs, N, xRef, uRef):
    """g in the kernels' stage layout: gx[k] = -(Qs_k + Qs_k') xr_{k+1}, gu[k] = -(Rs_k + Rs_k') ur_k"""
    gx = np.stack([-(Qs[k] + Qs[k].T) @ xRef[k + 1] for k in range(N)])
    gu = np.stack([-(Rs[k] + Rs[k].T) @ uRef[k] for k in range(N)])
    return gx, gu


def cost_stage(Qs, Rs, x, u, xRef, uRef):
    dx, du = x - xRef, u - uRef
    return sum(dx[k + 1] @ Qs[k] @ dx[k + 1] + du[k] @ Rs[k] @ du[k] for k in range(u.shape[0]))


def admm_levels_ltv_stage(A, B, c, Qs, Rs, N, x_lb, x_ub, u_lb, u_ub, x0, rho=1.0, eps_abs=1e-5, eps_rel=1e-5, max_iter=10000,
                          eps_prim_inf=1e-4, alpha=1.6, n_levels=7, rho_step=5.0, g=None, warm=None, shift=False, guard=True):
    """tests/mpc_ltv_ref.py: admm_levels_ltv (see there for the order of an iteration and the returned namespace) with the data in stage
    form.  The differences, as the kernels spell them:
        tables:      P_N = 2 Qs_{N-1} + rho I;  Suu_k = 2 Rs_k + rho I + B_k' P B_k;  the value update leaving stage k >= 1 adds
                     2 Qs_{k-1} + rho I (the one leaving stage 0 is read by nothing)
        x0 test:     against row 0 of the state box
        projection:  [x_{k+1} ; u_k] into [x_lb[k+1] ; u_lb[k]], [x_ub[k+1] ; u_ub[k]]
        certificate: the support term with the stage's own bounds"""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    n, m = B.shape[-2:]
    c = np.zeros((N, n)) if c is None else np.asarray(c, dtype=np.float64)
    assert A.shape == (N, n, n) and B.shape == (N, n, m) and c.shape == (N, n)
    assert Qs.shape == (N, n, n) and Rs.shape == (N, m, m)
    assert x_lb.shape == x_ub.shape == (N + 1, n) and u_lb.shape == u_ub.shape == (N, m)
    xl, xu = x_lb[1:], x_ub[1:]
    level0 = n_levels // 2
    rho0 = float(rho)
    tabs = {}

    def tables(l):
        if l not in tabs:
            r_ = rho0 * rho_step ** (l - level0)
            P = 2 * Qs[N - 1] + r_ * np.eye(n)
            K, Mi, D = [None] * N, [None] * N, [None] * N
            for k in range(N - 1, -1, -1):
                D[k] = P @ c[k]
                Suu = (2 * Rs[k] + r_ * np.eye(m)) + B[k].T @ P @ B[k]
                Sux = B[k].T @ P @ A[k]
                Mi[k] = np.linalg.inv(Suu)
                K[k] = Mi[k] @ Sux
                P = (2 * Qs[max(k - 1, 0)] + r_ * np.eye(n)) + A[k].T @ P @ A[k] - Sux.T @ K[k]
            tabs[l] = (r_, K, Mi, D)
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
    guard_on = bool(guard) and (gn > 0.0 or np.max(np.abs(c)) > 0.0)
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
    if np.any(x0 < x_lb[0]) or np.any(x0 > x_ub[0]):
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
        yxn = np.clip(xh + lx, xl, xu)
        yun = np.clip(uh + lu, u_lb, u_ub)
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
            break
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
        s = rx[N - 1].copy()
        gmax, vc = 0.0, 0.0
        for k in range(N - 1, -1, -1):
            vc += s @ c[k]
            gmax = max(gmax, np.max(np.abs(ru[k] + B[k].T @ s)))
            s = (rx[k - 1] if k >= 1 else 0.0) + A[k].T @ s
        sup = 0.0
        for r_, lo_, hi_ in ((rx, xl, xu), (ru, u_lb, u_ub)):
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


def solve_reference_ltv_stage(A, B, c, Qs, Rs, N, x_lb, x_ub, u_lb, u_ub, x0, xRef=None, uRef=None):
    """Independent reference: tests/mpc_ltv_ref.py: solve_reference_ltv with the stage's own weights in the condensed cost and the
    stage's own bounds as the linear constraints on the states (rows with a finite side only) and the bounds on the inputs.  x0 is not
    tested against row 0 here.  Returns (x, u, cost)."""
    n, m = B.shape[-2:]
    c = np.zeros((N, n)) if c is None else c
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
    rows, lo, hi = [], [], []
    for k in range(1, N + 1):
        for i in range(n):
            if np.isfinite(x_lb[k, i]) or np.isfinite(x_ub[k, i]):
                rows.append(Gam[k][i])
                lo.append(x_lb[k, i] - phi[k][i])
                hi.append(x_ub[k, i] - phi[k][i])
    cons = [spo.LinearConstraint(np.array(rows), np.array(lo), np.array(hi))] if rows else []
    res = spo.minimize(lambda v: v @ H @ v + 2 * gv @ v, np.zeros(N * m), jac=lambda v: 2 * (H @ v + gv), hess=lambda v: 2 * H,
                       method="trust-constr", bounds=spo.Bounds(u_lb.reshape(-1), u_ub.reshape(-1)), constraints=cons,
                       options=dict(gtol=1e-12, xtol=1e-14, barrier_tol=1e-14, maxiter=5000))
    u = res.x.reshape(N, m)
    x = lr.rollout_ltv(A, B, c, x0, u)
    return x, u, cost_stage(Qs, Rs, x, u, xRef, uRef)


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


def make_problem(mpcUtils, c, stage_varying=None):
    """the ltvMpc object of a case (host side only): Q as the constructor takes it, (N + 1, n, n) with a row 0 that nothing reads"""
    sv = c.stage_varying if stage_varying is None else stage_varying

    def args(d):
        A, B, ck, Qs, Rs, xl, xu, ul, uu = d
        return A, B, ck, np.concatenate([Qs[:1], Qs]), Rs, xl, xu, ul, uu
    if c.shared:
        A, B, ck, Q, R, xl, xu, ul, uu = args(c.inst[0])
    else:
        A, B, ck, Q, R, xl, xu, ul, uu = (np.stack(v) for v in zip(*(args(d) for d in c.inst)))
    return mpcUtils.ltvMpc(A, B, Q, R, c.N, xl, xu, ul, uu, c=ck, stage_varying=sv)


def case_rho(mpcUtils, c):
    nb = len(c.x0)
    if c.rho is not None:
        return np.full(nb, float(c.rho))
    rho = np.atleast_1d(make_problem(mpcUtils, c).rho)
    return np.array([rho[problem_of(c, b)] for b in range(nb)])


def reference_steps(c, rho):
    """[step][instance] -> result of admm_levels_ltv_stage, each fed its own previous final state"""
    out = []
    for s, step in enumerate(c.steps):
        row = []
        for b in range(len(c.x0)):
            A, B, ck, Qs, Rs, xl, xu, ul, uu = c.inst[problem_of(c, b)]
            prev = out[-1][b] if s else None
            x0 = prev.x[1] if step["x0"] == "x1" else (prev.x0 if step["x0"] == "same" else c.x0[b])
            warm = (prev.y, prev.lam, prev.level) if (step["warm"] and prev.status == "optimal") else None
            g = None if c.xRef is None else linear_term_stage(Qs, Rs, c.N, c.xRef[b], c.uRef[b])
            r = admm_levels_ltv_stage(A, B, ck, Qs, Rs, c.N, xl, xu, ul, uu, x0, rho=float(rho[b]), g=g, warm=warm,
                                      shift=step["warm"] == "shift", **step["kw"])
            r.x0 = x0
            row.append(r)
        out.append(row)
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    from zopt_amd import mpcUtils
    c = build(name)
    return reference_steps(c, case_rho(mpcUtils, c))


def envelope(xl, xu, ul, uu):
    """every bound replaced by its envelope over the stages: the smallest lower and the largest upper bound of the component (rows 1 .. N
    of the state box; row 0, the test on x0, stays)"""
    N = len(ul)
    exl, exu = np.tile(xl[1:].min(axis=0), (N + 1, 1)), np.tile(xu[1:].max(axis=0), (N + 1, 1))
    exl[0], exu[0] = xl[0], xu[0]
    return exl, exu, np.tile(ul.min(axis=0), (N, 1)), np.tile(uu.max(axis=0), (N, 1))


@functools.lru_cache(maxsize=None)
def scipy_solution(name, b=0):
    """(x, u) of the SciPy solve of instance b"""
    c = build(name)
    xr, ur = (None, None) if c.xRef is None else (c.xRef[b], c.uRef[b])
    x, u, _ = solve_reference_ltv_stage(*c.inst[problem_of(c, b)][:5], c.N, *c.inst[problem_of(c, b)][5:], c.x0[b], xRef=xr, uRef=ur)
    return x, u


def variant_solution(name, variant, b=0):
    """the restatement's solution of instance b with every bound replaced by its envelope ("envelope") or every weight by its mean over
    the stages ("mean"): what a case's solution must differ from for its stage data to matter"""
    from zopt_amd import mpcUtils
    c = build(name)
    A, B, ck, Qs, Rs, xl, xu, ul, uu = c.inst[problem_of(c, b)]
    if variant == "envelope":
        xl, xu, ul, uu = envelope(xl, xu, ul, uu)
    else:
        Qs, Rs = np.tile(Qs.mean(axis=0), (c.N, 1, 1)), np.tile(Rs.mean(axis=0), (c.N, 1, 1))
    g = None if c.xRef is None else linear_term_stage(Qs, Rs, c.N, c.xRef[b], c.uRef[b])
    r = admm_levels_ltv_stage(A, B, ck, Qs, Rs, c.N, xl, xu, ul, uu, c.x0[b], rho=float(case_rho(mpcUtils, c)[b]), g=g, **lr._kw())
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
