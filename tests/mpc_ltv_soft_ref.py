"""CPU checkers and cases for mpcUtils.ltvMpc with soft box constraints (x_soft_l1, x_soft_l2, u_soft_l1, u_soft_l2: a penalty
l1 d + l2 d^2 on the distance d of a component of [x_{k+1} ; u_k] from its box, per problem and component, constant over the stages;
l1 = +inf is a hard component); a helper module, not collected as a test.

  * `admm_levels_ltv_soft`     -- tests/mpc_ltv_stage_ref.py: admm_levels_ltv_stage restated with the three changes of
                                  zm_mpc_solve_ltv_soft_f64 (x0 test, proximal map, support term) and its guard rule.  Same options and
                                  returned namespace.
  * `solve_reference_ltv_soft` -- the condensed SciPy trust-constr solve with one slack e >= 0 per soft (stage, component) that has a
                                  finite bound: lo - e <= w <= hi + e, cost + l1 e + l2 e^2.
  * the named cases of tests/test_mpc_ltv_soft.py and tests/test_mpc_ltv_soft_gpu.py, built from the recipes of
    tests/mpc_ltv_stage_ref.py, with its `run_steps` and comparison rule.

An instance's data is that of tests/mpc_ltv_stage_ref.py followed by the weights l1, l2, each (n + m,) in the stacked layout [x ; u].
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np
import scipy.optimize as spo

from oracle.mpc_oracle import CHECK_EVERY
from tests import mpc_ltv_ref as lr
from tests import mpc_ltv_stage_ref as sr

INF = np.inf


def prox(v, lo, hi, t, a):
    """the y-update of zm_mpc_solve_ltv_soft_f64, written with its selects: t = l1 / rho, a = rho / (rho + 2 l2); t = +inf is the clip"""
    with np.errstate(invalid="ignore"):
        eh, el = a * ((v - hi) - t), a * ((lo - v) - t)
        return np.where(v > hi, np.where(eh > 0, hi + eh, hi), np.where(v < lo, np.where(el > 0, lo - el, lo), v))


def admm_levels_ltv_soft(A, B, c, Qs, Rs, N, x_lb, x_ub, u_lb, u_ub, x0, l1, l2=None, rho=1.0, eps_abs=1e-5, eps_rel=1e-5,
                         max_iter=10000, eps_prim_inf=1e-4, alpha=1.6, n_levels=7, rho_step=5.0, g=None, warm=None, shift=False,
                         guard=True):
    """tests/mpc_ltv_stage_ref.py: admm_levels_ltv_stage (see there and tests/mpc_ltv_ref.py for the order of an iteration and the
    returned namespace) with the penalty weights l1, l2 (n + m,) of the stacked components [x ; u]; l2 None: zeros.  The differences:
        x0 test:     a soft state component (finite l1) is not tested against row 0 of the state box
        projection:  the proximal map `prox` of the penalty, its thresholds t = l1 / rho, a = rho / (rho + 2 l2) at the penalty the
                     iteration runs at
        certificate: in the support term a soft component has the bounds -inf / +inf
        guard:       also on when any component is soft"""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    n, m = B.shape[-2:]
    c = np.zeros((N, n)) if c is None else np.asarray(c, dtype=np.float64)
    assert A.shape == (N, n, n) and B.shape == (N, n, m) and c.shape == (N, n)
    assert Qs.shape == (N, n, n) and Rs.shape == (N, m, m)
    assert x_lb.shape == x_ub.shape == (N + 1, n) and u_lb.shape == u_ub.shape == (N, m)
    l1 = np.asarray(l1, dtype=np.float64)
    l2 = np.zeros(n + m) if l2 is None else np.asarray(l2, dtype=np.float64)
    assert l1.shape == l2.shape == (n + m,) and np.all(l1 >= 0) and np.all(l2 >= 0) and not np.any((l2 > 0) & np.isinf(l1))
    l1x, l1u, l2x, l2u = l1[:n], l1[n:], l2[:n], l2[n:]
    soft_x, soft_u = np.isfinite(l1x), np.isfinite(l1u)
    xl, xu = x_lb[1:], x_ub[1:]
    # the bounds the certificate sees
    cxl, cxu = np.where(soft_x, -INF, xl), np.where(soft_x, INF, xu)
    cul, cuu = np.where(soft_u, -INF, u_lb), np.where(soft_u, INF, u_ub)
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


def violation(x, u, x_lb, x_ub, u_lb, u_ub):
    """d of every (stage, stacked component): (N, n + m)"""
    w, lo, hi = np.hstack([x[1:], u]), np.hstack([x_lb[1:], u_lb]), np.hstack([x_ub[1:], u_ub])
    return np.maximum(0.0, np.maximum(w - hi, lo - w))


def solve_reference_ltv_soft(A, B, c, Qs, Rs, N, x_lb, x_ub, u_lb, u_ub, x0, l1, l2=None, xRef=None, uRef=None):
    """Independent reference: tests/mpc_ltv_stage_ref.py: solve_reference_ltv_stage over (u, e) with one slack e >= 0 per soft (stage,
    component) that has a finite bound, lo - e <= w <= hi + e and the cost + l1 e + l2 e^2; a soft input gets slacks instead of Bounds.
    x0 is not tested against row 0 here.  Returns (x, u, cost with the penalty)."""
    n, m = B.shape[-2:]
    c = np.zeros((N, n)) if c is None else c
    l2 = np.zeros(n + m) if l2 is None else np.asarray(l2, dtype=np.float64)
    l1 = np.asarray(l1, dtype=np.float64)
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
                ulo[k * m + j], uhi[k * m + j] = -INF, INF
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
            hi.append(INF)
        if np.isfinite(hi_):
            Cm.append(np.concatenate([row, -e_]))
            lo.append(-INF)
            hi.append(hi_)
    Hf = np.zeros((nv, nv))
    Hf[:N * m, :N * m] = H
    Hf[N * m:, N * m:] = np.diag(w2)
    gf = np.concatenate([gv, 0.5 * w1])
    cons = [spo.LinearConstraint(np.array(Cm), np.array(lo), np.array(hi))] if Cm else []
    bounds = spo.Bounds(np.concatenate([ulo, np.zeros(ns)]), np.concatenate([uhi, np.full(ns, INF)]))
    res = spo.minimize(lambda v: v @ Hf @ v + 2 * gf @ v, np.zeros(nv), jac=lambda v: 2 * (Hf @ v + gf), hess=lambda v: 2 * Hf,
                       method="trust-constr", bounds=bounds, constraints=cons,
                       options=dict(gtol=1e-12, xtol=1e-14, barrier_tol=1e-14, maxiter=5000))
    u = res.x[:N * m].reshape(N, m)
    x = lr.rollout_ltv(A, B, c, x0, u)
    d = violation(x, u, x_lb, x_ub, u_lb, u_ub)
    fin = np.isfinite(l1)
    pen = np.sum(d[:, fin] * l1[fin] + d[:, fin] ** 2 * l2[fin])
    return x, u, sr.cost_stage(Qs, Rs, x, u, xRef, uRef) + pen


# ---- the scalar problem with known answers -------------------------------------------------------------------------------------------------

def scalar_data():
    """x+ = x + u, Q = R = 1, N = 1, x0 = 1, x_1 <= 0: minimise x_1^2 + u^2 + l1 max(0, x_1) + l2 max(0, x_1)^2.  Hard: x_1 = 0 with
    multiplier 2, so any l1 > 2 is exact; l1 = 1: x_1 = 1/4; l1 = 0, l2 = 1: x_1 = 1/3."""
    one = np.ones((1, 1, 1))
    d = [one, one, np.zeros((1, 1)), one, one, np.full((2, 1), -INF), np.array([[INF], [0.0]]), np.full((1, 1), -INF), np.full((1, 1), INF)]
    return d, np.ones(1)


SCALAR = [((1.0, 0.0), 0.25), ((3.0, 0.0), 0.0), ((0.0, 1.0), 1.0 / 3.0)]     # ((l1, l2) on the state, x_1)


# ---- cases -------------------------------------------------------------------------------------------------------------------------------
# As in tests/mpc_ltv_stage_ref.py, with `soft`: per problem (l1, l2), each (n + m,) in the stacked layout.  `witness`: the instance the
# non-vacuity conditions of tests/test_mpc_ltv_soft.py are checked on.

EPS, MAX_ITER = sr.EPS, sr.MAX_ITER
HORIZONS, BATCHES = sr.HORIZONS, sr.BATCHES
problem_of = sr.problem_of


def _weights(n, m, x1=None, x2=None, u1=None, u2=None):
    """(l1, l2) from {component: weight} maps; a component in none is hard"""
    l1, l2 = np.full(n + m, INF), np.zeros(n + m)
    for src, dst, at in ((x1, l1, 0), (x2, l2, 0), (u1, l1, n), (u2, l2, n)):
        for i, w in (src or {}).items():
            dst[at + i] = w
    assert not np.any((l2 > 0) & np.isinf(l1))
    return l1, l2


def _case(inst, soft, x0, N, shared, witness=0, **more):
    c = sr._case(inst, x0, N, shared, None, **more)
    c.soft, c.witness = soft, witness
    return c


def _sequence():
    """a cold solve at a loose tolerance, a warm one from it, a shifted one from x_1"""
    return [dict(kw=lr._kw(eps=1e-3), warm=False, x0="given"), dict(kw=lr._kw(), warm=True, x0="same"),
            dict(kw=lr._kw(), warm="shift", x0="x1")]


@functools.lru_cache(maxsize=None)
def build(name):
    if name == "soft_gate":          # P = (2,): the closed gate of tests/mpc_ltv_stage_ref.py, hard, and its twin with l1 = 2 on state 0
        (d, x0) = sr.gate_data(True)
        return _case([d, [v.copy() for v in d]], [_weights(2, 2), _weights(2, 2, x1={0: 2.0})], np.stack([x0, x0]), 3, False, witness=1,
                     rho=2.0)
    if name == "soft_x0_outside":    # (2, 2), N = 2, batch 5: state 0 soft with a box of half-width 1 about the first start at every row,
        n, m, N = 2, 2, 2            # state 1 hard; instance 3 starts outside in state 0 (solved), instance 1 outside in state 1 (refused)
        d, x0 = sr._base(n, m, N, 5, spread=0.2)
        d[5][:, 0], d[6][:, 0] = x0[0, 0] - 1.0, x0[0, 0] + 1.0
        d[5][0, 1], d[6][0, 1] = x0[0, 1] - 1.0, x0[0, 1] + 1.0
        x0 = x0.copy()
        x0[3, 0] += 1.5
        x0[1, 1] += 1.5
        return _case([d], [_weights(n, m, x1={0: 0.3})], x0, N, True, witness=3)
    if name in ("soft_terminal", "soft_terminal_sequence", "soft_terminal_fixed"):
        n, m, N = 2, 1, 5            # (2, 1), N = 5, batch 9: the terminal set of terminal_box under an l1 too small to reach it
        d, x0 = sr._base(n, m, N, 9, u_box=1.5)
        x, u = sr._plan(d, x0[0], N)
        d[5][N], d[6][N] = x[N] + 0.1, x[N] + 0.2
        more = {}
        if name == "soft_terminal_sequence":
            more["steps"] = _sequence()
        if name == "soft_terminal_fixed":
            more["steps"] = [dict(kw=lr._kw(n_levels=1), warm=False, x0="given")]
        return _case([d], [_weights(n, m, x1={0: 0.05, 1: 0.08})], x0, N, True, **more)
    if name == "soft_quadratic":     # (4, 2), N = 7, batch 5: the corridor and gate of moving_boxes with l1 = 0, l2 > 0 on state 0 and on
        n, m, N = 4, 2, 7            # input 1, whose box opens along the horizon
        c = sr.build("moving_boxes")
        d = [v.copy() for v in c.inst[0]]
        return _case([d], [_weights(n, m, x1={0: 0.0}, x2={0: 3.0}, u1={1: 0.0}, u2={1: 1.5})], c.x0, N, True)
    if name == "soft_mixed":         # (8, 4), N = 4, batch 1: infinite_stages (+-inf at some stages) with l1 and l2 on the states its boxes
        n, m, N = 8, 4, 4            # cut at, and a soft input whose bound cuts into the plan
        c = sr.build("infinite_stages")
        d = [v.copy() for v in c.inst[0]]
        _, u = sr._plan(sr._base(n, m, N, 1)[0], c.x0[0], N)
        d[8][1, 1] = u[1, 1] - 0.05
        soft = _weights(n, m, x1={0: 0.05, 1: 0.2, 3: 0.0, 4: 0.02}, x2={1: 0.5, 3: 2.0}, u1={1: 0.01})
        return _case([d], [soft], c.x0, N, True)
    if name == "soft_tracking":      # (12, 4), N = 7, batch 5: references of amplitude 3 under soft boxes of half-width 0.6 on states 0..2
        n, m, N = 12, 4, 7
        d, x0 = sr._base(n, m, N, 5, spread=0.3)
        d[5][1:, :3], d[6][1:, :3] = -0.6, 0.6
        rng = np.random.default_rng(21)
        k = np.arange(N + 1)
        xRef = 3.0 * np.sin(0.7 * k[None, :, None] + rng.uniform(0, 6, (5, 1, n)))
        uRef = np.zeros((5, N, m))
        return _case([d], [_weights(n, m, x1={0: 1.0, 1: 0.5, 2: 2.0}, x2={1: 1.0})], x0, N, True, xRef=xRef, uRef=uRef)
    if name == "soft_embedded":      # (3, 2) embedded in (4, 2), N = 3, batch 9: both_tracking with state 1 (a shrinking box) and input 0 soft
        c = sr.build("both_tracking")
        d = [v.copy() for v in c.inst[0]]
        return _case([d], [_weights(3, 2, x1={1: 0.5}, u1={0: 0.2}, u2={0: 0.3})], c.x0, c.N, True, xRef=c.xRef, uRef=c.uRef)
    if name == "soft_per_problem":   # (4, 1), N = 5, P = (5,): per_problem with its own weights per problem (mostly quadratic: the bound
                                     # of problem 0 cuts in by 0.05, which an l1 either ignores or enforces); problem 2 is all hard
        c = sr.build("per_problem")
        inst = [[v.copy() for v in d] for d in c.inst]
        soft = []
        for i in range(5):
            soft.append(_weights(4, 1) if i == 2 else
                        _weights(4, 1, x1={i % 4: 0.5 * (i % 2)}, x2={i % 4: 40.0 + 10.0 * i}, u1={0: 0.05} if i >= 3 else None))
        return _case(inst, soft, c.x0, c.N, False)
    raise KeyError(name)


CASES = ["soft_gate", "soft_x0_outside", "soft_terminal", "soft_quadratic", "soft_mixed", "soft_tracking", "soft_embedded",
         "soft_per_problem"]
ALL = CASES + ["soft_terminal_sequence", "soft_terminal_fixed"]
SCIPY_GPU = ["soft_terminal", "soft_quadratic"]


def scipy_instances(name):
    """the instances whose slack QP the tests solve: the first two -- of soft_quadratic the first alone (trust-constr needs a quarter of
    a minute per instance there: 14 inputs and 14 slacks under 40 rows)"""
    return (0,) if name == "soft_quadratic" else (0, 1)[:len(build(name).x0)]


def make_problem(mpcUtils, c, soft=None):
    """the ltvMpc object of a case (host side only); soft: other weights per problem than the case's"""
    soft = c.soft if soft is None else soft

    def args(d, w):
        A, B, ck, Qs, Rs, xl, xu, ul, uu = d
        n = B.shape[-2]
        return A, B, ck, np.concatenate([Qs[:1], Qs]), Rs, xl, xu, ul, uu, w[0][:n], w[1][:n], w[0][n:], w[1][n:]
    if c.shared:
        A, B, ck, Q, R, xl, xu, ul, uu, x1, x2, u1, u2 = args(c.inst[0], soft[0])
    else:
        A, B, ck, Q, R, xl, xu, ul, uu, x1, x2, u1, u2 = (np.stack(v) for v in zip(*(args(d, w) for d, w in zip(c.inst, soft))))
    return mpcUtils.ltvMpc(A, B, Q, R, c.N, xl, xu, ul, uu, c=ck, stage_varying=sr.ALL_SIX, x_soft_l1=x1, x_soft_l2=x2, u_soft_l1=u1,
                           u_soft_l2=u2)


def case_rho(mpcUtils, c):
    nb = len(c.x0)
    if c.rho is not None:
        return np.full(nb, float(c.rho))
    rho = np.atleast_1d(make_problem(mpcUtils, c).rho)
    return np.array([rho[problem_of(c, b)] for b in range(nb)])


def reference_steps(c, rho, soft=None):
    """[step][instance] -> result of admm_levels_ltv_soft, each fed its own previous final state"""
    soft = c.soft if soft is None else soft
    out = []
    for s, step in enumerate(c.steps):
        row = []
        for b in range(len(c.x0)):
            A, B, ck, Qs, Rs, xl, xu, ul, uu = c.inst[problem_of(c, b)]
            l1, l2 = soft[problem_of(c, b)]
            prev = out[-1][b] if s else None
            x0 = prev.x[1] if step["x0"] == "x1" else (prev.x0 if step["x0"] == "same" else c.x0[b])
            warm = (prev.y, prev.lam, prev.level) if (step["warm"] and prev.status == "optimal") else None
            g = None if c.xRef is None else sr.linear_term_stage(Qs, Rs, c.N, c.xRef[b], c.uRef[b])
            r = admm_levels_ltv_soft(A, B, ck, Qs, Rs, c.N, xl, xu, ul, uu, x0, l1, l2, rho=float(rho[b]), g=g, warm=warm,
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


@functools.lru_cache(maxsize=None)
def scipy_solution(name, b=0):
    """(x, u) of the slack QP of instance b"""
    c = build(name)
    xr, ur = (None, None) if c.xRef is None else (c.xRef[b], c.uRef[b])
    p = problem_of(c, b)
    x, u, _ = solve_reference_ltv_soft(*c.inst[p][:5], c.N, *c.inst[p][5:], c.x0[b], *c.soft[p], xRef=xr, uRef=ur)
    return x, u


@functools.lru_cache(maxsize=None)
def variant_solution(name, variant, b=0):
    """the restatement's result for instance b with every component hard ("hard": its status may be "infeasible"), or with the bounds of
    the soft components removed ("free"): what a case's solution must differ from for its weights to matter"""
    from zopt_amd import mpcUtils
    c = build(name)
    p = problem_of(c, b)
    A, B, ck, Qs, Rs, xl, xu, ul, uu = c.inst[p]
    n = B.shape[-2]
    l1, l2 = c.soft[p]
    if variant == "hard":
        l1, l2 = np.full_like(l1, INF), np.zeros_like(l2)
    else:
        fx, fu = np.isfinite(l1[:n]), np.isfinite(l1[n:])
        xl, xu, ul, uu = np.where(fx, -INF, xl), np.where(fx, INF, xu), np.where(fu, -INF, ul), np.where(fu, INF, uu)
    g = None if c.xRef is None else sr.linear_term_stage(Qs, Rs, c.N, c.xRef[b], c.uRef[b])
    return admm_levels_ltv_soft(A, B, ck, Qs, Rs, c.N, xl, xu, ul, uu, c.x0[b], l1, l2, rho=float(case_rho(mpcUtils, c)[b]), g=g,
                                **lr._kw(max_iter=3000))


def run_steps(prob, c, ref):
    """tests/mpc_ltv_stage_ref.py: run_steps; a step whose options fix the penalty (n_levels = 1, the restatement's spelling) goes to
    `solve` as adaptive_rho=False"""
    def kw(step):
        k = dict(step["kw"])
        if k.pop("n_levels", None) == 1:
            k["adaptive_rho"] = False
        return k
    twin = SimpleNamespace(**{**c.__dict__, "steps": [dict(step, kw=kw(step)) for step in c.steps]})
    return sr.run_steps(prob, twin, ref)


compare = sr.compare
