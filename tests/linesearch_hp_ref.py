"""Long-double reference of the line search (forwardPass2, K6: the rollouts of the 16 step sizes, the cost J of each, the choice of
the winner) and the problem families of tests/test_linesearch_hard_gpu.py.  Built on tests/model_hp_ref.py: `rollout`, `euler_step_ld`,
`FLOOR`, `bound`, `fp64_range`, `DETERMINED` and the quadcopter's point families are the ones defined there.

For a problem (model, Q, R, Qf[, xRef, uRef], x0, l, L, xPrev, uPrev, alphas), per trajectory and per step size a (`Reference`):

    J_ld[a]  the rollout and  sum_k (x_k'Q x_k + u_k'R u_k) + x_T'Qf x_T  (about the references for a tracking cost) in long double;
             Q is used as given, never symmetrised
    S[a]     the same sum with every product replaced by its absolute value, sum |x_i||Q_ij||x_j| + ...: the yardstick (indefinite and
             nonsymmetric weights make |J| useless as a scale)
    e[a]     |J_oracle[a] - J_ld[a]| / S[a]  for the fp64 oracle (oracle.zopt_oracle.trajectoryRollout + trajectoryCost)
    E        max_a e[a]: the oracle's WORST error over the trajectory's step sizes
    b[a]     max(FLOOR, 100 E) S[a]: the project's convention (model_hp_ref.bound), 100 x the oracle's own worst error on the same
             points, floor 100 x 2^-52.  (Not 100 e[a], sample by sample: a rounding error is a sum of random signs and a single
             sample of it can lie far below its typical size -- on the tracking families, where x ~ 1e6 meets x - xRef ~ 1, e[a]
             ranges from 1e-16 to 1e-9 within one trajectory, and a mere reordering of the oracle's own sums then misses 100 e[a]
             by up to 12 x; tests/test_linesearch_hp_ref.py::test_a_reordered_fp64_evaluation_passes.  The worst of 16 samples is
             the family-wide rule of model_hp_ref.Case, kept per trajectory as in model_hp_ref.RolloutCase.)
    C        the candidate set {a : J_ld[a] - b[a] <= min_a' (J_ld[a'] + b[a'])}; the choice is *determined* when |C| = 1
    per trajectory and per PREFIX of steps, the oracle rollout's row-metric error against the long-double one and 100 x that as the
    bound of the returned trajectory (the construction of model_hp_ref.RolloutCase; `prefix_errors` here is its vectorised restatement).
    A trajectory is *comparable* when, for every step size, the oracle's own rollout error stays below model_hp_ref.DETERMINED over the
    whole horizon and the reference stays in the range of fp64 (always, for the linear families; counted, for the quadcopter's).

`check` holds what a kernel returned (xTraj, uTraj, J, idx[, the 16 costs of single-step-size calls]) to that; `check_exact` holds the
exact families (integers and powers of two: every fp64 evaluation order gives the same bits or the same non-finite class) bit for
bit to the fp64 oracle and to the winner known by construction.  `oracle_linesearch` is the fp64 oracle in the kernels' place, with
planted errors (tests/test_linesearch_hp_ref.py: the oracle passes on every family, every planted error is caught).

A note on two errors that CANNOT be planted: x'Qx = x'Q'x = x'((Q + Q')/2)x for every x, so a cost evaluated with Q transposed or
replaced by its symmetric part is the same function (it differs by rounding, ~1e-16 S, far below any bound) and is no error.  What a
kernel that wrongly assumes symmetry computes is the form of ONE TRIANGLE mirrored: `upper` (Q symmetrised from its upper triangle)
and `lower` (the same of Q', i.e. from the lower triangle) are planted instead; the literal forms are shown to pass.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import model_hp_ref as hp

LD = hp.LD
ALPHAS = 0.5 ** np.arange(16)


# ---- a problem -------------------------------------------------------------------------------------------------------------------
class Problem:
    """kind 'linear' (A, B) or 'quad' (the 12-state quadcopter, Euler step dt, still air).  xRef / uRef: None, or what
    zopt_amd.models.TrackingCost takes: (n,), (b, 1, n) -- a goal per trajectory -- or (b, N + 1, n); uRef (m,), (b, 1, m), (b, N, m).
    expect: the winner known by construction (exact families), else None."""

    def __init__(self, name, kind, x0, l, L, xPrev, uPrev, Q, R, Qf, alphas=ALPHAS, A=None, B=None, dt=hp.ROLLOUT_DT, xRef=None,
                 uRef=None, expect=None):
        f = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.float64))
        self.name, self.kind, self.dt, self.expect = name, kind, dt, expect
        self.x0, self.l, self.L, self.xPrev, self.uPrev = f(x0), f(l), f(L), f(xPrev), f(uPrev)
        self.Q, self.R, self.Qf, self.A, self.B, self.alphas = f(Q), f(R), f(Qf), f(A), f(B), f(alphas)
        self.xRef, self.uRef = f(xRef), f(uRef)
        self.b, self.N, self.m, self.n = self.L.shape
        assert self.x0.shape == (self.b, self.n) and self.l.shape == (self.b, self.N, self.m)
        assert self.xPrev.shape == (self.b, self.N + 1, self.n) and self.uPrev.shape == (self.b, self.N, self.m)

    @property
    def tracking(self):
        return self.xRef is not None or self.uRef is not None

    def refs(self, dtype=LD):
        """the references as (b, N + 1, n) and (b, N, m) arrays (zeros without one)"""
        xr = np.zeros((self.b, self.N + 1, self.n), dtype=dtype)
        ur = np.zeros((self.b, self.N, self.m), dtype=dtype)
        if self.xRef is not None:
            xr = xr + self.xRef.astype(dtype)
        if self.uRef is not None:
            ur = ur + self.uRef.astype(dtype)
        return xr, ur

    def with_alphas(self, alphas, expect=None):
        q = Problem.__new__(Problem)
        q.__dict__.update(self.__dict__)
        q.alphas, q.expect = np.ascontiguousarray(np.asarray(alphas, dtype=np.float64)), expect
        return q

    def rows(self, idx):
        """the sub-problem of the trajectories idx"""
        q = Problem.__new__(Problem)
        q.__dict__.update(self.__dict__)
        for k in ("x0", "l", "L", "xPrev", "uPrev"):
            setattr(q, k, np.ascontiguousarray(getattr(self, k)[idx]))
        for k in ("xRef", "uRef"):
            r = getattr(self, k)
            if r is not None and r.ndim == 3:
                setattr(q, k, np.ascontiguousarray(r[idx]))
        q.b = len(q.x0)
        return q

    # -- the two evaluators: long double, and the fp64 oracle -----------------------------------------------------------------------
    def step_ld(self):
        if self.kind == "quad":
            return hp.euler_step_ld((0.0, 0.0, 0.0), self.dt)
        A, B = self.A.astype(LD), self.B.astype(LD)
        return lambda x, u: np.einsum("ij,bj->bi", A, x) + np.einsum("ij,bj->bi", B, u)

    def step_oracle(self):
        from oracle import zopt_oracle as zo
        if self.kind == "quad":
            return zo.quad_euler_step(self.dt)
        A, B = self.A, self.B
        return lambda x, u: A @ x + B @ u


def cost_ld(p, x, u, absolute=False, weights=None):
    """(b,) long double: J of the trajectories (x (b, N + 1, n), u (b, N, m)) about the problem's references; absolute: S"""
    Q, R, Qf = (W.astype(LD) for W in (weights or (p.Q, p.R, p.Qf)))
    xr, ur = p.refs()
    f = np.abs if absolute else (lambda v: v)
    ex, eu = f(np.asarray(x, dtype=LD) - xr), f(np.asarray(u, dtype=LD) - ur)
    with np.errstate(all="ignore"):
        return (np.einsum("bki,ij,bkj->b", ex[:, :-1], f(Q), ex[:, :-1]) + np.einsum("bki,ij,bkj->b", eu, f(R), eu)
                + np.einsum("bi,ij,bj->b", ex[:, -1], f(Qf), ex[:, -1]))


def cost_oracle(p, x, u, weights=None):
    """fp64: oracle.zopt_oracle.trajectoryCost of one trajectory; a tracking cost is that of the differences, formed first"""
    from oracle import zopt_oracle as zo
    Q, R, Qf = weights or (p.Q, p.R, p.Qf)
    return zo.trajectoryCost(lambda xx, uu: xx @ Q @ xx + uu @ R @ uu, lambda xx: xx @ Qf @ xx, zo.Trajectory(x, u))


def prefix_errors(xT, uT, xr, ur):
    """model_hp_ref.prefix_errors, vectorised: (b, N) -- for trajectory i and every prefix of K = 1..N steps the row-metric error of
    (xT[i, :K + 1], uT[i, :K]) against the reference: max over components of max_k |got - ref| / max(1, max_k |ref|).  Where the
    reference is not finite `got` is free; a non-finite `got` elsewhere gives inf."""
    def one(g, r):
        g, r = np.asarray(g, dtype=LD), np.asarray(r, dtype=LD)
        fin = np.isfinite(r)
        with np.errstate(invalid="ignore"):
            d = np.where(fin, np.abs(g - r), 0)
        d = np.where(fin & ~np.isfinite(g), np.inf, d)
        a = np.where(fin, np.abs(r), 0)
        return np.maximum.accumulate(d, axis=1), np.maximum(1, np.maximum.accumulate(a, axis=1))
    dx, ax = one(xT, xr)
    du, au = one(uT, ur)
    ex = np.max(dx / ax, axis=2)[:, 1:]            # the prefix of K steps holds x_0 .. x_K
    eu = np.max(du / au, axis=2)
    return np.maximum(ex, eu).astype(np.float64)


class Reference:
    def __init__(self, p):
        from oracle import zopt_oracle as zo
        self.p = p
        na, b, N = len(p.alphas), p.b, p.N
        xr64, ur64 = p.refs(np.float64)
        sl, so = p.step_ld(), p.step_oracle()
        self.x, self.u, self.xo, self.uo = [], [], [], []
        self.J, self.S, self.Jo = np.zeros((na, b), dtype=LD), np.zeros((na, b), dtype=LD), np.zeros((na, b))
        self.pe = np.zeros((na, b, N))
        alive = np.ones((na, b), bool)
        for a, al in enumerate(p.alphas):
            ls = p.l * al if p.kind == "quad" else p.l        # (the quadcopter's step sizes are powers of two: exact, as RolloutCase)
            x, u = hp.rollout(p.x0.astype(LD), ls, p.L, p.xPrev, p.uPrev, 1.0 if p.kind == "quad" else al, sl)
            x, u = hp.fp64_range(x, u)
            xo, uo = np.zeros((b, N + 1, p.n)), np.zeros((b, N, p.m))
            with np.errstate(all="ignore"):
                for i in range(b):
                    t = zo.trajectoryRollout(p.x0[i], so, zo.AffinePolicy(p.l[i], p.L[i]), zo.Trajectory(p.xPrev[i], p.uPrev[i]), alpha=al)
                    xo[i], uo[i] = t.xTraj, t.uTraj
                    self.Jo[a, i] = cost_oracle(p, xo[i] - xr64[i], uo[i] - ur64[i])
            self.J[a], self.S[a] = cost_ld(p, x, u), cost_ld(p, x, u, absolute=True)
            self.pe[a] = prefix_errors(xo, uo, x, u)
            alive[a] = np.all(np.isfinite(x.astype(np.float64)), axis=(1, 2)) & np.all(np.isfinite(u.astype(np.float64)), axis=(1, 2))
            self.x.append(x), self.u.append(u), self.xo.append(xo), self.uo.append(uo)
        self.pb = np.maximum(hp.FLOOR, 100.0 * self.pe)
        # comparable: the oracle's own rollout is determined in fp64 over the whole horizon, for every step size (RolloutCase.determined)
        self.comparable = np.all(alive & np.all(self.pe <= hp.DETERMINED, axis=2), axis=0)
        with np.errstate(all="ignore"):
            S = np.where(self.S > 0, self.S, LD(1))
            self.e = np.where(alive, np.abs(self.Jo.astype(LD) - self.J) / S, np.inf).astype(np.float64)
            self.E = np.max(self.e, axis=0)                     # per trajectory: the oracle's worst error over the step sizes
            self.bJ = np.maximum(LD(hp.FLOOR), 100 * self.E.astype(LD))[None, :] * self.S
            lo, hi = self.J - self.bJ, self.J + self.bJ
            c = self.comparable
            self.C = np.zeros((na, b), bool)
            self.C[:, c] = lo[:, c] <= np.min(hi[:, c], axis=0)
            self.argmin = np.zeros(b, dtype=int)
            self.argmin[c] = np.argmin(self.J[:, c].astype(LD), axis=0)
        self.determined = c & (self.C.sum(axis=0) == 1)

    def summary(self):
        c = self.comparable
        return (f"{self.p.name}: {int(c.sum())}/{self.p.b} comparable, {int(self.determined.sum())} determined, oracle cost error up to "
                f"{(self.e[:, c].max() if c.any() else 0.0):.1e} S, rollout error up to {(self.pe[:, c].max() if c.any() else 0.0):.1e}, "
                f"winners {sorted(set(self.argmin[c].tolist()))}")


@functools.lru_cache(maxsize=None)
def _reference_cached(key):
    return Reference(problem(*key))


def reference(p):
    """the Reference of a problem; problems made by `problem(...)` carry their key and are computed once per process"""
    key = getattr(p, "key", None)
    return _reference_cached(key) if key is not None else Reference(p)


# ---- the checker -----------------------------------------------------------------------------------------------------------------
def check(ref, xT, uT, J, idx, J16=None, what=""):
    """the six assertions of the module docstring on the comparable trajectories; prints and returns the worst error-to-bound ratio of
    each.  J16: (n_alpha, b) costs of single-step-size calls, or None."""
    p = ref.p
    xT, uT, J, idx = np.asarray(xT, np.float64), np.asarray(uT, np.float64), np.asarray(J, np.float64), np.asarray(idx).astype(int)
    rows = np.flatnonzero(ref.comparable)
    assert len(rows), f"{what}: no comparable trajectory"
    assert np.all((idx[rows] >= 0) & (idx[rows] < len(p.alphas))), f"{what}: idx out of range {idx}"
    ii = idx[rows]
    # 6. finite where the reference is
    assert np.all(np.isfinite(J[rows])) and np.all(np.isfinite(xT[rows])) and np.all(np.isfinite(uT[rows])), f"{what}: not finite"
    # 1. the choice
    assert np.all(ref.C[ii, rows]), f"{what}: idx {ii.tolist()} outside the candidate sets (argmin {ref.argmin[rows].tolist()})"
    det = ref.determined[rows]
    assert np.array_equal(ii[det], ref.argmin[rows][det]), f"{what}: idx {ii[det].tolist()} != determined argmin {ref.argmin[rows][det].tolist()}"
    # 2. the winner's cost
    bJ = ref.bJ[ii, rows]
    r2 = np.max(np.abs(J[rows].astype(LD) - ref.J[ii, rows]) / bJ)
    # 3. the cost of the RETURNED trajectory, in long double, against the returned J
    q = p.rows(rows)
    r3 = np.max(np.abs(cost_ld(q, xT[rows], uT[rows]) - J[rows].astype(LD)) / bJ)
    # 4. the returned trajectory against the long-double rollout at alphas[idx]
    xr = np.stack([ref.x[a][i] for a, i in zip(ii, rows)])
    ur = np.stack([ref.u[a][i] for a, i in zip(ii, rows)])
    r4 = float(np.max(prefix_errors(xT[rows], uT[rows], xr, ur) / ref.pb[ii, rows]))
    assert np.array_equal(xT[rows, 0], p.x0[rows]), f"{what}: xTraj[0] is not x0"
    # 5. the costs of the single-step-size calls
    r5 = 0.0
    if J16 is not None:
        J16 = np.asarray(J16, np.float64)
        assert J16.shape == (len(p.alphas), p.b) and np.all(np.isfinite(J16[:, rows])), f"{what}: single-step-size costs not finite"
        r5 = float(np.max(np.abs(J16[:, rows].astype(LD) - ref.J[:, rows]) / ref.bJ[:, rows]))
    out = {"J": float(r2), "J of returned trajectory": float(r3), "trajectory": r4, "16 costs": r5}
    print(f"{what} [{ref.summary()}]: worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in out.items()))
    assert r2 <= 1.0, f"{what}: |J - J_ld[idx]| is {r2:.3g} x its bound"
    assert r3 <= 1.0, f"{what}: the returned trajectory's cost is {r3:.3g} x the bound away from the returned J"
    assert r4 <= 1.0, f"{what}: the returned trajectory is {r4:.3g} x its bound away from the rollout at alphas[idx]"
    assert r5 <= 1.0, f"{what}: a single-step-size cost is {r5:.3g} x its bound away"
    return out


def check_exact(p, xT, uT, J, idx, what=""):
    """exact families: the winner is np.argmin of the oracle's costs (NaN is the minimum, the first index wins) and the one known by
    construction; J and the trajectory equal the oracle's at that index bit for bit (NaN = NaN)"""
    o = oracle_linesearch(p)
    idx = np.asarray(idx).astype(int)
    assert np.array_equal(idx, o["idx"]), f"{what}: idx {idx.tolist()}, oracle {o['idx'].tolist()}"
    if p.expect is not None:
        assert np.all(o["idx"] == p.expect), f"{what}: the construction expects {p.expect}, the oracle finds {o['idx'].tolist()}"
    assert np.array_equal(np.asarray(J, np.float64), o["J"], equal_nan=True), f"{what}: J {J} != oracle {o['J']}"
    assert np.array_equal(np.asarray(xT, np.float64), o["xT"], equal_nan=True), f"{what}: xTraj differs from the oracle's"
    assert np.array_equal(np.asarray(uT, np.float64), o["uT"], equal_nan=True), f"{what}: uTraj differs from the oracle's"


# ---- the fp64 oracle in the kernels' place, with planted errors --------------------------------------------------------------------
def _triangle(Q, upper):
    """what a kernel that assumes symmetry and reads one triangle computes: that triangle mirrored"""
    T = np.triu(Q) if upper else np.tril(Q)
    return T + T.T - np.diag(np.diagonal(Q))


def reordered_costs(p):
    """(n_alpha, b): the 16 costs from a second fp64 evaluation that differs from the oracle's in nothing but the order of its sums
    (B u + A x with the columns reversed; (e'Q)e instead of e'(Qe)): whatever bound is in force must admit it"""
    from oracle import zopt_oracle as zo
    assert p.kind == "linear"
    A, B = p.A, p.B
    xr, ur = p.refs(np.float64)
    J = np.zeros((len(p.alphas), p.b))
    for a, al in enumerate(p.alphas):
        for i in range(p.b):
            t = zo.trajectoryRollout(p.x0[i], lambda x, u: B @ u + A[:, ::-1] @ x[::-1], zo.AffinePolicy(p.l[i], p.L[i]),
                                     zo.Trajectory(p.xPrev[i], p.uPrev[i]), alpha=al)
            ex, eu = t.xTraj - xr[i], t.uTraj - ur[i]
            J[a, i] = sum((ex[k] @ p.Q) @ ex[k] + (eu[k] @ p.R) @ eu[k] for k in range(p.N)) + (ex[-1] @ p.Qf) @ ex[-1]
    return J


def oracle_linesearch(p, plant=None):
    """{xT, uT, J, idx, J16} of the fp64 oracle's line search.  plant: None; 'symmetrised' / 'transposed' (no errors, see the module
    docstring); 'upper' / 'lower' (Q, R, Qf from one triangle); 'ties_last'; 'nan_as_inf'; 'next_J' (J of index idx + 1);
    'drop_offdiag' (the last non-zero off-diagonal entry of each weight dropped)."""
    from oracle import zopt_oracle as zo
    W = [p.Q, p.R, p.Qf]
    if plant == "symmetrised":
        W = [(M + M.T) / 2 for M in W]
    elif plant == "transposed":
        W = [M.T.copy() for M in W]
    elif plant in ("upper", "lower"):
        W = [_triangle(M, plant == "upper") for M in W]
    elif plant == "drop_offdiag":
        W = [M.copy() for M in W]
        for M in W:
            off = np.argwhere((M != 0) & ~np.eye(len(M), dtype=bool))
            if len(off):
                M[tuple(off[-1])] = 0.0
    na, b = len(p.alphas), p.b
    xr, ur = p.refs(np.float64)
    so = p.step_oracle()
    J16 = np.zeros((na, b))
    xs, us = np.zeros((na, b, p.N + 1, p.n)), np.zeros((na, b, p.N, p.m))
    with np.errstate(all="ignore"):
        for a, al in enumerate(p.alphas):
            for i in range(b):
                t = zo.trajectoryRollout(p.x0[i], so, zo.AffinePolicy(p.l[i], p.L[i]), zo.Trajectory(p.xPrev[i], p.uPrev[i]), alpha=al)
                xs[a, i], us[a, i] = t.xTraj, t.uTraj
                J16[a, i] = cost_oracle(p, t.xTraj - xr[i], t.uTraj - ur[i], weights=W)
    key = np.where(np.isnan(J16), np.inf, J16) if plant == "nan_as_inf" else J16
    idx = (na - 1 - np.argmin(key[::-1], axis=0)) if plant == "ties_last" else np.argmin(key, axis=0)
    r = np.arange(b)
    J = J16[np.minimum(idx + 1, na - 1), r] if plant == "next_J" else J16[idx, r]
    return {"xT": xs[idx, r], "uT": us[idx, r], "J": J, "idx": idx, "J16": J16, "xs": xs, "us": us}


# ---- the hard families (linear models) ------------------------------------------------------------------------------------------------
LINEAR_FAMILIES = ("index_j", "near_tie", "unstable", "scaled", "indefinite", "nonsymmetric", "one_offdiag", "permuted")
ONE_OFFDIAG = ("Q", "R", "Qf", "none")           # where the single off-diagonal entry sits; 'none': the truly diagonal cost next to it
TRACK_FORMS = ("step", "goal", "shared")         # xRef / uRef per step, per trajectory with step stride 0, one shared (n,) / (m,)


def _pd(rng, k, scale=1.0):
    M = rng.standard_normal((k, k))
    return scale * (M @ M.T / k + np.eye(k))


def _backward(A, B, Q, R, Qf, ex, eu):
    """the LQ backward pass (fp64) of cost sum e'Qe about the deviations (ex, eu) of the previous trajectory from the reference, with the
    symmetric parts made positive definite (|eigenvalues|): feed-forward l and gains L of one trajectory"""
    def spd(M):
        w, v = np.linalg.eigh((M + M.T) / 2)
        return (v * np.maximum(np.abs(w), 1e-9 * max(np.abs(w).max(), 1e-300))) @ v.T
    Q, R, Qf = spd(Q), spd(R), spd(Qf)
    N = len(eu)
    Vxx, vx = 2 * Qf, 2 * Qf @ ex[N]
    l, L = np.zeros((N, B.shape[1])), np.zeros((N, B.shape[1], len(A)))
    for k in range(N - 1, -1, -1):
        Qx, Qu = 2 * Q @ ex[k] + A.T @ vx, 2 * R @ eu[k] + B.T @ vx
        Qxx, Quu, Qux = 2 * Q + A.T @ Vxx @ A, 2 * R + B.T @ Vxx @ B, B.T @ Vxx @ A
        l[k], L[k] = -np.linalg.solve(Quu, Qu), -np.linalg.solve(Quu, Qux)
        vx = Qx + Qux.T @ l[k]
        Vxx = Qxx + Qux.T @ L[k]
        Vxx = (Vxx + Vxx.T) / 2
    return l, L


def _exact_step(p):
    """scale l (per trajectory) so that step size 1 is the exact minimiser of J along it: J(alpha) is a quadratic in alpha for a linear
    model, c0 + c1 alpha + c2 alpha^2, fitted in long double at alpha = 0, 1, 2; alpha* = -c1 / (2 c2) where c2 > 0 (else l stays)"""
    sl = p.step_ld()
    Js = [cost_ld(p, *hp.rollout(p.x0.astype(LD), p.l, p.L, p.xPrev, p.uPrev, a, sl)) for a in (0.0, 1.0, 2.0)]
    c2 = (Js[2] - 2 * Js[1] + Js[0]) / 2
    c1 = Js[1] - Js[0] - c2
    with np.errstate(all="ignore"):
        s = np.where(c2 > 0, -c1 / (2 * c2), 1.0).astype(np.float64)
    return p.l * s[:, None, None]


def linear_problem(family, n, m, N, b, variant=None, track=None, j0=0, seed=0):
    """a seeded problem of a family at one shape.  variant: for one_offdiag, where the entry sits (ONE_OFFDIAG); for the others 'diag'
    gives diagonal weights.  track: None or one of TRACK_FORMS (references ~1e6 from the origin, the state within a few units of them).
    j0: trajectory i scales l* by 2^((j0 + i) mod 16) (index_j, permuted), so that index (j0 + i) mod 16 is the minimiser."""
    fam = LINEAR_FAMILIES.index(family)
    rng = np.random.default_rng([seed, fam, n, m, N, b, ONE_OFFDIAG.index(variant) if variant in ONE_OFFDIAG else 9,
                                 TRACK_FORMS.index(track) if track else 9])
    rho = 1.3 if family == "unstable" else 0.9
    A = rng.standard_normal((n, n))
    A *= rho / np.max(np.abs(np.linalg.eigvals(A)))
    B = rng.standard_normal((n, m))
    # weights
    if family == "one_offdiag" or variant == "diag":
        Q, R, Qf = np.diag(rng.uniform(0.5, 2.0, n)), np.diag(rng.uniform(0.5, 2.0, m)), np.diag(rng.uniform(5.0, 20.0, n))
        if variant == "Q" and n > 1:
            Q[n - 1, 0] = 0.75
        elif variant == "R" and m > 1:
            R[0, m - 1] = -0.625
        elif variant == "Qf" and n > 1:
            Qf[1, 0] = 3.5
    elif family == "indefinite":
        def indef(k, s):
            v = np.linalg.qr(rng.standard_normal((k, k)))[0]
            w = s * rng.uniform(0.5, 2.0, k) * np.where(np.arange(k) % 2 == 0, 1.0, -1.0)
            M = (v * w) @ v.T
            return (M + M.T) / 2
        Q, R, Qf = indef(n, 1.0), _pd(rng, m), indef(n, 10.0)
    else:
        Q, R, Qf = _pd(rng, n), _pd(rng, m), _pd(rng, n, 10.0)
        if family == "nonsymmetric":          # a skew part as large as the symmetric part (Frobenius norm)
            def skewed(M):
                K = rng.standard_normal(M.shape)
                K = K - K.T
                nk = np.linalg.norm(K)
                return M + (K * (np.linalg.norm(M) / nk) if nk > 0 else K)
            Q, R, Qf = skewed(Q), skewed(R), skewed(Qf)
    # the previous trajectory: a rollout of the model under random inputs from a large state; x0 a small step away from its start
    xscale = 40.0 if family == "unstable" else 100.0
    xRef = uRef = None
    if track:
        g, h = 1e6 * rng.uniform(0.5, 1.5, n) * rng.choice([-1.0, 1.0], n), 1e6 * rng.uniform(0.5, 1.5, m) * rng.choice([-1.0, 1.0], m)
        A = A + np.outer(g - B @ h - A @ g, g) / (g @ g)              # (g, h) is a fixed point: A g + B h = g
        c = rng.uniform(0.5, 2.0, b) if track != "shared" else np.ones(b)
        gx, gu = c[:, None] * g, c[:, None] * h
        xscale = 0.3
    else:
        gx, gu = np.zeros((b, n)), np.zeros((b, m))
    uPrev = gu[:, None, :] + 0.3 * rng.standard_normal((b, N, m))
    xPrev = np.zeros((b, N + 1, n))
    xPrev[:, 0] = gx + xscale * rng.standard_normal((b, n))
    for k in range(N):
        xPrev[:, k + 1] = xPrev[:, k] @ A.T + uPrev[:, k] @ B.T
    x0 = xPrev[:, 0] + 1e-3 * xscale * rng.standard_normal((b, n))
    if track == "step":
        xRef, uRef = xPrev + 0.5 * rng.standard_normal(xPrev.shape), uPrev + 0.5 * rng.standard_normal(uPrev.shape)
    elif track == "goal":
        xRef, uRef = gx[:, None, :].copy(), gu[:, None, :].copy()
    elif track == "shared":
        xRef, uRef = gx[0].copy(), gu[0].copy()
    if family == "scaled":                    # x = D x~ with D = 10^(-6..6); weights D^-2 W D^-2: the terms of J span 24 decades
        d = 10.0 ** rng.integers(-6, 7, n)
        d[:2] = [1e-6, 1e6][:min(n, 2)]
        A, B = (A * d[:, None]) / d[None, :], B * d[:, None]
        Q, Qf = Q / np.outer(d * d, d * d), Qf / np.outer(d * d, d * d)
        xPrev, x0 = xPrev * d, x0 * d
        if xRef is not None:
            xRef = xRef * d
    p = Problem(family, "linear", x0, np.zeros((b, N, m)), np.zeros((b, N, m, n)), xPrev, uPrev, Q, R, Qf, A=A, B=B, xRef=xRef, uRef=uRef)
    xr, ur = p.refs(np.float64)
    for i in range(b):
        p.l[i], p.L[i] = _backward(A, B, Q, R, Qf, xPrev[i] - xr[i], uPrev[i] - ur[i])
    p.l = _exact_step(p)                      # l*: step size 1 is the exact minimiser
    i = np.arange(b)
    if family == "near_tie":                  # indices j and j + 1 agree to rounding: J(alpha) is symmetric about 1 in alpha (4/3) 2^j
        p.l = p.l * ((4.0 / 3.0) * 2.0 ** ((j0 + i) % 15))[:, None, None]
    else:
        p.l = p.l * (2.0 ** ((j0 + i) % 16))[:, None, None]
    if family == "permuted":
        p.alphas = np.ascontiguousarray(ALPHAS[np.random.default_rng([seed, 77, n, N]).permutation(16)])
    p.name = family + (f"[{variant}]" if variant else "") + (f"+track:{track}" if track else "") + f" ({n},{m},{N},{b})"
    return p


# ---- the quadcopter's families -------------------------------------------------------------------------------------------------------
def quad_problem(fam, N, diagonal=True):
    """model_hp_ref.rollout_problem(fam, N) with l of trajectory i scaled by 2^(i mod 16), so that the winners differ; diagonal weights
    (the two-pass search with the four-lane re-roll) or general nonsymmetric ones"""
    x0, l, L, xp, up = hp.rollout_problem(fam, N)
    rng = np.random.default_rng([3, int(diagonal)])
    Q, R, Qf = np.diag(rng.uniform(0.5, 2.0, 12)), np.diag(rng.uniform(0.5, 2.0, 4)), np.diag(rng.uniform(5.0, 20.0, 12))
    if not diagonal:
        Q, R, Qf = Q + 0.2 * rng.standard_normal((12, 12)), R + 0.2 * rng.standard_normal((4, 4)), Qf + 2.0 * rng.standard_normal((12, 12))
    l = l * (2.0 ** (np.arange(len(x0)) % 16))[:, None, None]
    p = Problem(f"quad:{fam} N={N} {'diagonal' if diagonal else 'general'}", "quad", x0, l, L, xp, up, Q, R, Qf)
    return p


def problem(kind, *args):
    """keyed constructor: problem('linear', family, n, m, N, b, variant, track, j0) or problem('quad', fam, N, diagonal); the key lets
    `reference` compute each Reference once per process"""
    p = linear_problem(*args) if kind == "linear" else quad_problem(*args)
    p.key = (kind,) + tuple(args)
    return p


# ---- the exact families ---------------------------------------------------------------------------------------------------------------
HUGE, OVER = 2.0 ** 500, 2.0 ** 1000
EXACT_CASES = ("l_zero", "B_zero_R_zero", "weights_zero", "duplicates", "zero_step", "nan_9", "nan_5_11", "nan_7_minf_2",
               "pinf_but_13", "pinf_all", "minf_5_9")
EXACT_SHORT = ("nan_first", "nan_last", "pinf_all")        # with n_alpha < 16: idx < n_alpha always


def exact_problem(case, n, m, N=3, b=3, n_alpha=16, ref=None):
    """LinearModel problems in small integers and powers of two.  The tie cases: integer data, step sizes from {1, 1/2, 1/4, 1/8, 0}
    -- every product and sum is exact in fp64, in any order, fused or not.  The non-finite cases (n, m >= 2): A = I, B = [I; 0], no
    gains, l non-zero at step 0 only, (1, 2^100) in its first two components, Q = R = 0, Qf = diag(+-1, -+1, 0, ...): x_T =
    alpha (1, 2^100, 0, ...).  A step size 2^-j gives a finite J; 2^500 gives ONE overflowing product (2^1200) next to finite ones:
    -+inf in any order, fused or not; 2^1000 makes alpha l itself infinite, 0 x inf then fills the state with NaN: J = NaN.
    ref: None, 'zero' or 'exact' -- a tracking reference of zeros, or one of small integers (the non-finite cases: zeros)."""
    rng = np.random.default_rng([11, EXACT_CASES.index(case) if case in EXACT_CASES else 20 + EXACT_SHORT.index(case), n, m])
    ints = lambda lo, hi, *s: rng.integers(lo, hi + 1, s).astype(np.float64)
    expect = None
    if case in ("l_zero", "B_zero_R_zero", "weights_zero", "duplicates", "zero_step"):
        A = np.eye(n) + (np.eye(n, k=1) if n > 1 else 0)
        B = np.zeros((n, m))
        B[np.arange(n), np.arange(n) % m] = 1.0
        B[0, :] = 1.0
        Q, R, Qf = np.diag(ints(1, 3, n)), np.diag(ints(1, 3, m)), np.diag(ints(1, 4, n))
        if n > 1:
            Q[n - 1, 0], Qf[0, n - 1] = 2.0, -1.0         # general (nonsymmetric) weights
        if m > 1:
            R[0, m - 1] = 1.0
        x0, l, L = ints(-3, 3, b, n), ints(-2, 2, b, N, m), ints(-1, 1, b, N, m, n) * (rng.random((b, N, m, n)) < 0.3)
        xp, up = ints(-2, 2, b, N + 1, n), ints(-2, 2, b, N, m)
        al = ALPHAS
        if case == "l_zero":
            l[:], expect = 0.0, 0
        elif case == "B_zero_R_zero":
            B[:], R[:], expect = 0.0, 0.0, 0
        elif case == "weights_zero":
            Q[:], R[:], Qf[:], expect = 0.0, 0.0, 0.0, 0
        elif case == "duplicates":        # every value twice or more; the first of the minimiser's positions wins
            al = np.array([1, 0.5, 0.25, 0.125] * 4)[rng.permutation(16)]
        else:
            al = np.array([1, 0.5, 0.25, 0.125, 0.0, 2.0, 4.0, 0.0625] * 2)[rng.permutation(16)]
        xRef = uRef = None
        if ref == "zero":
            xRef, uRef = np.zeros((b, N + 1, n)), np.zeros(m)
        elif ref == "exact":
            xRef, uRef = ints(-2, 2, b, N + 1, n), ints(-1, 1, b, 1, m)
        return Problem(f"exact:{case}", "linear", x0, l, L, xp, up, Q, R, Qf, alphas=al[:n_alpha], A=A, B=B, xRef=xRef, uRef=uRef, expect=expect)
    assert n >= 2 and m >= 2
    A, B = np.eye(n), np.eye(n, m)
    x0, L, xp, up = np.zeros((b, n)), np.zeros((b, N, m, n)), np.zeros((b, N + 1, n)), np.zeros((b, N, m))
    l = np.zeros((b, N, m))
    l[:, 0, 0], l[:, 0, 1] = 1.0, 2.0 ** 100
    sign = -1.0 if case.startswith("pinf") else 1.0        # Qf = diag(1, -1): the overflowing product is negative
    Qf = np.zeros((n, n))
    Qf[0, 0], Qf[1, 1] = sign, -sign
    al = ALPHAS.copy()
    if case == "nan_9":
        al[9], expect = OVER, 9
    elif case == "nan_5_11":
        al[[5, 11]], expect = OVER, 5
    elif case == "nan_7_minf_2":
        al[7], al[2], expect = OVER, HUGE, 7
    elif case == "pinf_but_13":
        al[:] = HUGE
        al[13], expect = 0.5, 13
    elif case == "pinf_all":
        al[:], expect = HUGE, 0
    elif case == "minf_5_9":
        al[[5, 9]], expect = HUGE, 5
    elif case == "nan_first":
        al[0], expect = OVER, 0
    elif case == "nan_last":
        al[n_alpha - 1], expect = OVER, n_alpha - 1
    else:
        raise KeyError(case)
    xRef = uRef = None
    if ref is not None:
        xRef, uRef = np.zeros((b, N + 1, n)), np.zeros(m)
    return Problem(f"exact:{case}", "linear", x0, l, L, xp, up, np.zeros((n, n)), np.zeros((m, m)), Qf, alphas=al[:n_alpha], A=A, B=B,
                   xRef=xRef, uRef=uRef, expect=expect)


# ---- the cases of tests/test_linesearch_hard_gpu.py: every form of the line search x its shapes x every family ------------------------
FORM_SHAPES = {
    "fast": [(12, 4, N, b) for N in (1, 2, 3, 4, 7, 9) for b in (1, 5)],
    "fast_diag": [(12, 4, 3, 5), (12, 4, 7, 5)],
    "generic": [(1, 1, 4, 1), (5, 3, 7, 5), (8, 4, 9, 67), (12, 1, 3, 3), (12, 4, 7, 5)],
    "wide": [(13, 4, 5, 3), (12, 5, 4, 2), (16, 16, 3, 2), (17, 3, 4, 2), (33, 5, 6, 2), (48, 16, 3, 2), (49, 1, 3, 2), (64, 16, 3, 2)],
    "list": [(12, 4, 7, 9), (5, 3, 4, 9), (33, 5, 3, 5)],
    "track": [(12, 4, 3, 5), (12, 4, 7, 5), (8, 4, 4, 5)],
    "python": [(12, 4, 7, 5), (33, 5, 6, 2)],
}
UNSTABLE_LONG = (12, 4, 30, 67)
TRACK_FAMILIES = ("index_j", "scaled", "nonsymmetric")
DIAG_FAMILIES = ("index_j", "near_tie", "unstable", "scaled", "permuted")
QUAD_HORIZONS = (1, 3, 7)
QUAD_ALL = ("nominal", "many_turns", "zeros")          # every trajectory comparable at N <= 3, QUAD_MIN_LONG of 17 at N = 7
QUAD_MIN, QUAD_MIN_LONG = 8, 14                        # the others: all 17 at N = 1, at least QUAD_MIN of 17 beyond


def form_cases(form):
    """the keys (arguments of `problem`) of a form's cases.  j0 of a shape is the number of trajectories of the shapes before it, so
    that the small batches cover all 16 winning indices between them."""
    keys, seen = [], 0
    for n, m, N, b in FORM_SHAPES[form]:
        j0, seen = seen % 16, seen + b
        if form == "track":
            keys += [("linear", fam, n, m, N, b, None, tr, j0) for fam in TRACK_FAMILIES for tr in TRACK_FORMS]
            continue
        if form == "fast_diag":
            keys += [("linear", fam, n, m, N, b, "diag", None, j0) for fam in DIAG_FAMILIES]
            keys.append(("linear", "one_offdiag", n, m, N, b, "none", None, j0))
            continue
        for fam in LINEAR_FAMILIES:
            if fam == "one_offdiag":      # (a variant whose matrix is 1 x 1 has no off-diagonal entry: it is the 'none' variant)
                keys += [("linear", fam, n, m, N, b, v, None, j0) for v in ONE_OFFDIAG if not ((v in ("Q", "Qf") and n == 1) or (v == "R" and m == 1))]
            else:
                keys.append(("linear", fam, n, m, N, b, None, None, j0))
    if form == "fast":
        keys.append(("linear", "unstable") + UNSTABLE_LONG + (None, None, 0))
    return keys


def quad_cases():
    return [("quad", fam, N, diag) for fam in hp.FAMILIES for N in QUAD_HORIZONS for diag in (True, False)]


def key_id(key):
    if key[0] == "quad":
        return f"{key[1]}-N{key[2]}-{'diag' if key[3] else 'general'}"
    _, fam, n, m, N, b, v, tr, j0 = key
    return f"{fam}{'-' + v if v else ''}{'-' + tr if tr else ''}-{n}x{m}x{N}x{b}"


def quad_required(fam, N):
    """how many of the 17 trajectories of a quadcopter case must be comparable: a case that would compare fewer fails"""
    if N == 1 or (fam in QUAD_ALL and N <= 3):
        return 17
    return QUAD_MIN_LONG if fam in QUAD_ALL else QUAD_MIN
