"""High-precision references for the Riccati tests: the finite-horizon recursion in long double and Newton-refined DARE / CARE
solutions (`care_refined` is `dare_refined`'s continuous-time counterpart: Newton-Kleinman steps on SciPy's solve_continuous_are).

The fp64 oracle (oracle/zopt_oracle.py) carries its own rounding error, which on hard inputs is of the same order as a kernel's.
These references sit well below both, so a test can tell the kernel's error from the oracle's:
  * `finite_horizon_ld`: the oracle's Joseph-form backward recursion computed in `np.longdouble` (80-bit extended on x86-64, eps 1.1e-19);
  * `dare_refined`: SciPy's `solve_discrete_are`, then Newton steps whose DARE residual is evaluated in long double and whose Stein
    correction `E - Acl^T E Acl = Res` is solved in fp64 (the correction is small, so fp64 suffices for it).
LAPACK has no long double, so the small solves here are a batched Gaussian elimination with partial pivoting.
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
