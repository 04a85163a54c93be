"""High-precision references for the Riccati tests: the finite-horizon recursion in long double and Newton-refined DARE / CARE
solutions (`care_refined` is `dare_refined`'s continuous-time counterpart: Newton-Kleinman steps on SciPy's solve_continuous_are).

The fp64 oracle (oracle/zopt_oracle.py) carries its own rounding error, which on hard inputs is of the same order as a kernel's.
These references sit well below both, so a test can tell the kernel's error from the oracle's:
  * `finite_horizon_ld`: the oracle's Joseph-form backward recursion computed in `np.longdouble` (80-bit extended on x86-64, eps 1.1e-19);
  * `dare_refined`: SciPy's `solve_discrete_are`, then Newton steps whose DARE residual is evaluated in long double and whose Stein
    correction `E - Acl^T E Acl = Res` is solved in fp64 (the correction is small, so fp64 suffices for it).
LAPACK has no long double, so the small solves here are a batched Gaussian elimination with partial pivoting.

For the iLQR / affine-LQR / DDP backward sweeps and the PD projection (second half of the file):
  * `ilqr_backward_ld`, `affine_lqr_ld`: the oracle's recursions, formula by formula, in long double;
  * `eigh_ld`, `psd_project_ld`: a long-double symmetric eigensolver (cyclic Jacobi) and V max(w, eps) V^T built on it;
  * `ddp_backward_hp`: the DDP sweep with that projection at every step;
  * `psd_from_spectrum_ld`: matrices with a planted spectrum, whose projection is known without an eigensolve;
  * `sweep_metric`, `sweep_bounds`, `ddp_bounds`: the metric and the bounds of the hard-family GPU tests, taken from the
    oracle's own error against these references, never from a kernel.
"""
from __future__ import annotations

import numpy as np
import scipy.linalg as spl

LD = np.longdouble


def _T(X):
    return np.swapaxes(X, -1, -2)


def solve_ld(M, Y):
    """X = M^-1 Y in long double by Gaussian elimination with partial pivoting, vectorised over the leading axes.
    M (..., k, k), Y (..., k, p)."""
    M = np.asarray(M, dtype=LD)
    Y = np.asarray(Y, dtype=LD)
    shp = np.broadcast_shapes(M.shape[:-2], Y.shape[:-2]) + Y.shape[-2:]
    k, p = shp[-2:]
    M = np.broadcast_to(M, shp[:-2] + (k, k)).reshape(-1, k, k).copy()
    Y = np.broadcast_to(Y, shp).reshape(-1, k, p).copy()
    b = np.arange(M.shape[0])
    for j in range(k):
        piv = j + np.argmax(np.abs(M[:, j:, j]), axis=1)
        Mj, Yj = M[b, j].copy(), Y[b, j].copy()
        M[b, j], Y[b, j] = M[b, piv], Y[b, piv]
        M[b, piv], Y[b, piv] = Mj, Yj
        f = M[:, j + 1:, j] / M[:, j, j][:, None]
        M[:, j + 1:, j:] -= f[:, :, None] * M[:, None, j, j:]
        Y[:, j + 1:] -= f[:, :, None] * Y[:, None, j]
    X = np.empty_like(Y)
    for j in range(k - 1, -1, -1):
        X[:, j] = (Y[:, j] - np.sum(M[:, j, j + 1:, None] * X[:, j + 1:], axis=1)) / M[:, j, j][:, None]
    return X.reshape(shp)


def finite_horizon_ld(A, B, Q, R, T):
    """`zopt_oracle.discreteFiniteHorizonLqr` in long double: V <- Q[T-1]; for k = T-1..0: L_k = solve(R_k + B_k^T V B_k, B_k^T V A_k),
    V = Q_k + L_k^T R_k L_k + (A_k - B_k L_k)^T V (A_k - B_k L_k).  A (..., T, n, n) etc.; returns L (..., T, m, n) in long double."""
    A, B, Q, R = (np.asarray(x, dtype=LD) for x in (A, B, Q, R))
    n, m = B.shape[-2:]
    V = Q[..., T - 1, :, :]
    L = np.empty(A.shape[:-3] + (T, m, n), dtype=LD)
    for k in range(T - 1, -1, -1):
        Ak, Bk, Qk, Rk = A[..., k, :, :], B[..., k, :, :], Q[..., k, :, :], R[..., k, :, :]
        BtV = _T(Bk) @ V
        Lk = solve_ld(Rk + BtV @ Bk, BtV @ Ak)
        Acl = Ak - Bk @ Lk
        V = Qk + (_T(Lk) @ Rk) @ Lk + (_T(Acl) @ V) @ Acl
        L[..., k, :, :] = Lk
    return L


def dare_gain_residual(A, B, Q, R, P):
    """Long double: the gain L = (R + B^T P B)^-1 B^T P A of a value matrix P, the closed loop A - B L and the DARE residual
    Q + A^T P A - A^T P B L - P (the Joseph form's fixed point: Q + L^T R L + Acl^T P Acl - P is the same matrix at any P)."""
    A, B, Q, R, P = (np.asarray(x, dtype=LD) for x in (A, B, Q, R, P))
    BtP = _T(B) @ P
    L = solve_ld(R + BtP @ B, BtP @ A)
    Acl = A - B @ L
    Res = Q + _T(L) @ R @ L + _T(Acl) @ P @ Acl - P
    return L, Acl, Res


def dare_refined(A, B, Q, R, rtol=1e-17, max_newton=4):
    """Stabilising DARE solution of ONE design to long-double accuracy: SciPy's solve_discrete_are, then Newton steps
    P <- P + E with E - Acl^T E Acl = Res(P) until max|E| <= rtol * max|P| (at most `max_newton`).

    Returns (L, P, rho_cl, res): the gain and value (long double), the closed loop's spectral radius and the final residual
    max|Res| / max|P| (long double arithmetic)."""
    A, B, Q, R = (np.asarray(x, dtype=np.float64) for x in (A, B, Q, R))
    P = spl.solve_discrete_are(A, B, Q, R).astype(LD)
    for _ in range(max_newton):
        _, Acl, Res = dare_gain_residual(A, B, Q, R, P)
        E = spl.solve_discrete_lyapunov(Acl.astype(np.float64).T, Res.astype(np.float64))
        P = P + E.astype(LD)
        if np.max(np.abs(E)) <= rtol * float(np.max(np.abs(P))):
            break
    L, Acl, Res = dare_gain_residual(A, B, Q, R, P)
    rho_cl = float(np.max(np.abs(np.linalg.eigvals(Acl.astype(np.float64)))))
    return L, P, rho_cl, np.max(np.abs(Res)) / np.max(np.abs(P))


def care_gain_residual(A, B, Q, R, P):
    """Long double: the gain K = R^-1 B^T P of a value matrix P, the closed loop A - B K and the CARE residual
    A^T P + P A - K^T R K + Q.  The quadratic term is formed through K: under cheap control (R = r I, r -> 0) B^T P is O(sqrt r) and
    K^T R K is O(1), whereas P (B R^-1 B^T) P multiplies by G ~ 1/r first and cancels eight digits in fp64."""
    A, B, Q, R, P = (np.asarray(x, dtype=LD) for x in (A, B, Q, R, P))
    K = solve_ld(R, _T(B) @ P)
    Acl = A - B @ K
    Res = _T(A) @ P + P @ A - (_T(K) @ R) @ K + Q
    return K, Acl, Res


def care_refined(A, B, Q, R, rtol=1e-17, max_newton=6):
    """Stabilising CARE solution of ONE design to long-double accuracy: SciPy's solve_continuous_are, then Newton-Kleinman steps
    P <- P + E with Acl^T E + E Acl = -Res(P) (fp64 Lyapunov solve of the long-double residual) until max|E| <= rtol * max|P|
    (at most `max_newton`).

    Returns (K, P, abscissa_cl, res): the gain and value (long double), the closed loop's spectral abscissa max Re eig(A - B K) and
    the final residual max|Res| / max|P| (long double arithmetic)."""
    A, B, Q, R = (np.asarray(x, dtype=np.float64) for x in (A, B, Q, R))
    P = spl.solve_continuous_are(A, B, Q, R).astype(LD)
    P = (P + _T(P)) / 2
    for _ in range(max_newton):
        _, Acl, Res = care_gain_residual(A, B, Q, R, P)
        Res = (Res + _T(Res)) / 2
        E = spl.solve_continuous_lyapunov(Acl.astype(np.float64).T, -Res.astype(np.float64))
        P = P + ((E + E.T) / 2).astype(LD)
        if np.max(np.abs(E)) <= rtol * float(np.max(np.abs(P))):
            break
    K, Acl, Res = care_gain_residual(A, B, Q, R, P)
    abscissa_cl = float(np.max(np.linalg.eigvals(Acl.astype(np.float64)).real))
    return K, P, abscissa_cl, np.max(np.abs(Res)) / np.max(np.abs(P))


def care_scipy_error(A, B, Q, R, K_ref, P_ref):
    """SciPy's own error on ONE design against the refined solution, in P and in K = solve(R, B^T P), each relative to max|ref|: the
    yardstick the hard-spectrum CARE tests scale their bound by (K needs its own: under cheap control it amplifies P's error)."""
    A, B, Q, R = (np.asarray(x, dtype=np.float64) for x in (A, B, Q, R))
    P = spl.solve_continuous_are(A, B, Q, R)
    K = np.linalg.solve(R, B.T @ P)
    Pr, Kr = np.asarray(P_ref, dtype=np.float64), np.asarray(K_ref, dtype=np.float64)
    return float(np.max(np.abs(P - Pr)) / np.max(np.abs(Pr))), float(np.max(np.abs(K - Kr)) / np.max(np.abs(Kr)))


def care_bounds(scipy_err_P, scipy_err_K, floor=1e-10, factor=100.0):
    """(bound on P, bound on K), relative to max|ref|, from `care_scipy_error`'s pair: max(floor, factor * SciPy's own error).
    Reference side only; the CPU pins and the GPU test both take their bound from here."""
    return max(floor, factor * scipy_err_P), max(floor, factor * scipy_err_K)


# ------------------------------------------------------------------------------------------------------------------------
# The iLQR / affine-LQR / DDP backward sweeps and the PD projection (ilqr_backward.hip, sweep_tiled_f64.hip, ns16.h, psd_tiled.hip).
def _mv(M, v):
    return (M @ v[..., None])[..., 0]


def _cond64(M):
    return np.linalg.cond(np.asarray(M, dtype=np.float64))


def _sweep_ld(dyn, cost, Vf, second=None, eps=1e-3, perturb=None):
    """`zo.riccatiStep_ilqr` / `riccatiStep_ddp` + `_riccati_tail` in long double over the horizon (time axis -3 of the matrices).
    second = (f_xx, f_ux, f_uu): the DDP step, `psd_project_ld` of the stacked vf_zz added to the Hessians.  perturb = (rel, rng): a
    symmetric random matrix with largest entry rel * max|P| is added to every step's projected matrix P (the sensitivity probe of
    `ddp_reference_and_sensitivity`; rel may be an array over the batch)."""
    f_x, f_u = (np.asarray(x, dtype=LD) for x in dyn[1:3])
    c_x, c_u, c_xx, c_ux, c_uu = (np.asarray(x, dtype=LD) for x in cost[1:])
    v_x, v_xx = (np.asarray(x, dtype=LD) for x in Vf[1:])
    if second is not None:
        f_xx, f_ux, f_uu = (np.asarray(x, dtype=LD) for x in second)
    T, n, m = f_u.shape[-3:]
    lead = f_u.shape[:-3]
    out = {"l": np.empty(lead + (T, m), dtype=LD), "L": np.empty(lead + (T, m, n), dtype=LD), "v_x": np.empty(lead + (T, n), dtype=LD),
           "v_xx": np.empty(lead + (T, n, n), dtype=LD), "cond_quu": np.empty(lead + (T,)), "spectrum": np.empty(lead + (T, n + m))}
    for k in range(T - 1, -1, -1):
        fx, fu = f_x[..., k, :, :], f_u[..., k, :, :]
        Q_x = c_x[..., k, :] + _mv(_T(fx), v_x)
        Q_u = c_u[..., k, :] + _mv(_T(fu), v_x)
        Q_xx = c_xx[..., k, :, :] + (_T(fx) @ v_xx) @ fx
        Q_uu = c_uu[..., k, :, :] + (_T(fu) @ v_xx) @ fu
        Q_ux = c_ux[..., k, :, :] + (_T(fu) @ v_xx) @ fx
        if second is not None:
            vf = [np.sum(v_x[..., :, None, None] * F[..., k, :, :, :], axis=-3) for F in (f_xx, f_ux, f_uu)]
            Z = np.concatenate([np.concatenate([vf[0], _T(vf[1])], axis=-1), np.concatenate([vf[1], vf[2]], axis=-1)], axis=-2)
            P, w = psd_project_ld(Z, eps, return_spectrum=True)
            fro = np.sqrt(np.sum((w - eps) ** 2, axis=-1, keepdims=True))
            out["spectrum"][..., k, :] = ((w - eps) / np.where(fro > 0, fro, 1)).astype(np.float64)
            if perturb is not None:
                rel, rng = perturb
                E = rng.standard_normal(P.shape)
                E = E + _T(E)
                P = P + (E / np.max(np.abs(E), axis=(-1, -2), keepdims=True) * (rel * np.max(np.abs(P), axis=(-1, -2), keepdims=True))).astype(LD)
            Q_xx, Q_ux, Q_uu = Q_xx + P[..., :n, :n], Q_ux + P[..., n:, :n], Q_uu + P[..., n:, n:]
        l = -solve_ld(Q_uu, Q_u[..., None])[..., 0]
        L = -solve_ld(Q_uu, Q_ux)
        Quul = _mv(Q_uu, l)
        v_x = Q_x - _mv(_T(L), Quul)
        v_xx = Q_xx - (_T(L) @ Q_uu) @ L
        out["l"][..., k, :], out["L"][..., k, :, :], out["v_x"][..., k, :], out["v_xx"][..., k, :, :] = l, L, v_x, v_xx
        out["cond_quu"][..., k] = _cond64(Q_uu)
    if second is None:
        del out["spectrum"]
    return out


def ilqr_backward_ld(dyn, cost, Vf):
    """`zo.backwardPass_ilqr` (riccatiStep_ilqr + _riccati_tail) in long double with `solve_ld`: the same formulas, v_x' = Q_x -
    L^T (Q_uu l) and v_xx' = Q_xx - (L^T Q_uu) L, no Joseph form and no symmetrisation; a nonsymmetric v_xx, c_xx or c_uu is used as
    it stands.  dyn = (f, f_x, f_u), cost = (c, c_x, c_u, c_xx, c_ux, c_uu), Vf = (v, v_x, v_xx) with any leading batch axes.
    Returns a dict: l (..., T, m), L (..., T, m, n), and per step the new v_x, v_xx (long double) and cond(Q_uu) (fp64)."""
    return _sweep_ld(dyn, cost, Vf)


def ddp_backward_hp(dyn, cost, Vf, eps=1e-3, perturb=None):
    """`zo.backwardPass_ddp` (riccatiStep_ddp) in long double: per step vf_zz = sum_i v_x[i] d2f_i stacked as [[xx, ux^T], [ux, uu]],
    `psd_project_ld` of it added to the Hessians, then the iLQR tail.  dyn = (f, f_x, f_u, f_xx, f_ux, f_uu).  Besides
    `ilqr_backward_ld`'s fields it returns `spectrum` (..., T, n + m): the eigenvalues of vf_zz - eps I relative to its Frobenius
    norm (what the matrix-sign iteration of ns16.h has to resolve), ascending."""
    return _sweep_ld(dyn[:3], cost, Vf, second=dyn[3:6], eps=eps, perturb=perturb)


def affine_lqr_ld(A, B, d, Q, R, H, q, r, T):
    """`zo.bilinearAffineLqr` in long double (q0 only feeds the constant v0, which no gain depends on).  Returns a dict: L (..., T, m,
    n), l (..., T, m), per step the new V, v and cond(Suu)."""
    A, B, d, Q, R, H, q, r = (np.asarray(x, dtype=LD) for x in (A, B, d, Q, R, H, q, r))
    n, m = B.shape[-2:]
    lead = A.shape[:-3]
    V, v = Q[..., T - 1, :, :], q[..., T - 1, :]
    out = {"L": np.empty(lead + (T, m, n), dtype=LD), "l": np.empty(lead + (T, m), dtype=LD), "V": np.empty(lead + (T, n, n), dtype=LD),
           "v": np.empty(lead + (T, n), dtype=LD), "cond_quu": np.empty(lead + (T,))}
    for k in range(T - 1, -1, -1):
        Ak, Bk, dk = A[..., k, :, :], B[..., k, :, :], d[..., k, :]
        Vd = _mv(V, dk)
        Su = r[..., k, :] + _mv(_T(Bk), v) + _mv(_T(Bk), _mv(_T(V), dk))
        Suu = R[..., k, :, :] + (_T(Bk) @ V) @ Bk
        Sux = H[..., k, :, :] + (_T(Bk) @ V) @ Ak
        L = solve_ld(Suu, Sux)
        l = solve_ld(Suu, Su[..., None])[..., 0]
        V, v = Q[..., k, :, :] + (_T(Ak) @ V) @ Ak - (_T(L) @ Suu) @ L, q[..., k, :] + _mv(_T(Ak), v + Vd) - _mv(_T(Sux), l)
        out["L"][..., k, :, :], out["l"][..., k, :], out["V"][..., k, :, :], out["v"][..., k, :] = L, l, V, v
        out["cond_quu"][..., k] = _cond64(Suu)
    return out


def _round_robin(k):
    """The k - 1 (k even) rounds of disjoint index pairs that together hold every pair once (the circle method)."""
    K = k + (k & 1)
    idx = list(range(K))
    rounds = []
    for _ in range(K - 1):
        pairs = [(min(idx[i], idx[K - 1 - i]), max(idx[i], idx[K - 1 - i])) for i in range(K // 2)]
        pairs = [(p, q) for p, q in pairs if q < k]
        rounds.append((np.array([p for p, _ in pairs]), np.array([q for _, q in pairs])))
        idx = [idx[0]] + [idx[-1]] + idx[1:-1]
    return rounds


def eigh_ld(a, rtol=1e-19, max_sweeps=60):
    """Eigen-decomposition of the symmetric (..., k, k) matrices `a` (their lower and upper halves averaged) in long double by cyclic
    Jacobi rotations, each round rotating k/2 disjoint pairs at once, until the off-diagonal Frobenius norm is <= rtol times the
    Frobenius norm.  Returns (w (..., k) ascending, V (..., k, k) with a = V diag(w) V^T).  LAPACK has no long double."""
    a = np.asarray(a, dtype=LD)
    k = a.shape[-1]
    lead = a.shape[:-2]
    A = ((a + _T(a)) / 2).reshape(-1, k, k).copy()
    V = np.broadcast_to(np.eye(k, dtype=LD), A.shape).copy()
    fro = np.sqrt(np.sum(A * A, axis=(1, 2)))
    rounds = _round_robin(k) if k > 1 else []
    dg = np.arange(k)
    for _ in range(max_sweeps):
        off = A.copy()
        off[:, dg, dg] = 0
        if np.all(np.sqrt(np.sum(off * off, axis=(1, 2))) <= rtol * fro):
            break
        for p, q in rounds:
            apq, app, aqq = A[:, p, q], A[:, p, p], A[:, q, q]
            nz = apq != 0
            theta = (aqq - app) / (2 * np.where(nz, apq, 1))
            t = np.where(nz, np.where(theta >= 0, 1, -1) / (np.abs(theta) + np.sqrt(theta * theta + 1)), 0)
            c = 1 / np.sqrt(t * t + 1)
            s = t * c
            Ap, Aq = A[:, p, :].copy(), A[:, q, :].copy()
            A[:, p, :], A[:, q, :] = c[:, :, None] * Ap - s[:, :, None] * Aq, s[:, :, None] * Ap + c[:, :, None] * Aq
            Ap, Aq = A[:, :, p].copy(), A[:, :, q].copy()
            A[:, :, p], A[:, :, q] = c[:, None, :] * Ap - s[:, None, :] * Aq, s[:, None, :] * Ap + c[:, None, :] * Aq
            A[:, p, q] = A[:, q, p] = 0
            A[:, p, p], A[:, q, q] = app - t * apq, aqq + t * apq
            Vp, Vq = V[:, :, p].copy(), V[:, :, q].copy()
            V[:, :, p], V[:, :, q] = c[:, None, :] * Vp - s[:, None, :] * Vq, s[:, None, :] * Vp + c[:, None, :] * Vq
    else:
        raise RuntimeError("eigh_ld: no convergence")
    w = A[:, dg, dg]
    order = np.argsort(w, axis=1)
    w = np.take_along_axis(w, order, axis=1)
    V = np.take_along_axis(V, order[:, None, :], axis=2)
    return w.reshape(lead + (k,)), V.reshape(lead + (k, k))


def psd_project_ld(a, eps=1e-3, return_spectrum=False):
    """`zo.ensurePositiveDefinite` in long double: V max(w, eps) V^T of (a + a^T) / 2, built on `eigh_ld`."""
    w, V = eigh_ld(a)
    P = (V * np.maximum(w, LD(eps))[..., None, :]) @ _T(V)
    P = (P + _T(P)) / 2
    return (P, w) if return_spectrum else P


def psd_from_spectrum_ld(k, w, seed, eps=1e-3):
    """A symmetric k x k matrix with the planted spectrum w: U diag(w) U^T, U the product of three random Householder reflectors
    formed in long double.  Returns (the matrix rounded to fp64, the long-double projection U max(w, eps) U^T, U): no eigensolve is
    involved, so the reference is exact up to the rounding of the fp64 matrix (the projection is 1-Lipschitz: <= 1e-16 |a|)."""
    rng = np.random.default_rng(seed)
    w = np.asarray(w, dtype=LD)
    U = np.eye(k, dtype=LD)
    for _ in range(3):
        h = rng.standard_normal(k).astype(LD)
        U = U - 2 * np.outer(U @ h, h) / (h @ h)
    a = (U * w) @ U.T
    P = (U * np.maximum(w, LD(eps))) @ U.T
    return ((a + a.T) / 2).astype(np.float64), (P + P.T) / 2, U


def sweep_metric(out, ref):
    """Per trajectory and per step: max|out_k - ref_k| / max_k' max|ref_k'| (the maximum over that trajectory's steps), so neither a
    large trajectory of the batch nor a large late step hides the others.  out, ref (batch, T, ...); returns (batch, T) fp64."""
    out, ref = np.asarray(out, dtype=LD), np.asarray(ref, dtype=LD)
    ax = tuple(range(2, ref.ndim))
    scale = np.max(np.abs(ref), axis=tuple(range(1, ref.ndim)))
    scale = np.where(scale > 0, scale, 1)
    return (np.max(np.abs(out - ref), axis=ax) / scale[:, None]).astype(np.float64)


def sweep_bounds(e_case, e_plain, factor=100.0):
    """Bound of the hard-family sweep tests on `sweep_metric`: factor * max(the fp64 oracle's error on the case, its error on the
    plain family at the same shape and horizon), each the maximum of `sweep_metric`.  `care_bounds`' factor; the plain family's error
    (~1e-15) takes the place of its fixed floor.  Reference side only."""
    return factor * max(float(np.max(e_case)), float(np.max(e_plain)))


def ddp_reference_and_sensitivity(dyn, cost, Vf, eps=1e-3, rel=2e-11, seeds=3):
    """`ddp_backward_hp`'s result, and how much the projection's documented resolution (2e-11 of max|P|, ns16.h) can move the DDP
    policy of this case: the sweep rerun with a symmetric random perturbation of that size on every step's projected matrix, the
    largest `sweep_metric` of l and of L against the unperturbed run over `seeds` draws.  The draws run as extra batch entries of
    one sweep.  Returns (ref, (s_l, s_L))."""
    b = np.asarray(dyn[1]).shape[0]
    rep = lambda t: tuple(np.concatenate([np.asarray(x)] * (seeds + 1), axis=0) for x in t)      # noqa: E731
    scale = np.repeat([0.0] + [rel] * seeds, b)[:, None, None]
    out = ddp_backward_hp(rep(dyn), rep(cost), rep(Vf), eps=eps, perturb=(scale, np.random.default_rng(12345)))
    ref = {k: v[:b] for k, v in out.items()}
    s = tuple(max(float(np.max(sweep_metric(out[name][b * i:b * (i + 1)], ref[name]))) for i in range(1, seeds + 1)) for name in ("l", "L"))
    return ref, s


def ddp_bounds(e_case, e_plain, s_case, factor=100.0, sens_factor=10.0, cap=1e-9):
    """Bound of the hard-family DDP tests: max(`sweep_bounds`, sens_factor * s_case), s_case from `ddp_reference_and_sensitivity`; the
    factor 10 covers the direction of the kernel's actual projection error, which is not random.  The sensitivity term is capped at
    1e-9, the tolerance of the DDP parity tests, so the allowance for the projection never exceeds what those tests allow.  The
    `sweep_bounds` term is NOT capped: it is 100 x the oracle's own error, which reaches ~2e-8 where cond(Q_uu) ~ 1e7 (`illcond_quu`);
    the parity tests on the plain family stay in the suite at their 1e-10 / 1e-9."""
    return max(sweep_bounds(e_case, e_plain, factor), min(sens_factor * float(s_case), cap))
