"""NumPy restatement of K1's m x m solve (zopt_amd/csrc/lqr_backward_dma.hip, m = 4), lane arithmetic and guard included.

Two solves of  Suu L = Sux  are modelled, each in the rounding order of the kernel:

  cofactor_solve   the product path.  Lane (g, c) expands the cofactor C[g][c & 3] of Suu (tile16_f64.h: cofactor3, with the sign
                   folded in by swapping the minor's last two rows), one v_mfma_f64_4x4x4_4b forms X = adj(Suu) [Sux | Suu], det is
                   X[0][N], L = X * fast_rcp(det).  The guard admits the result when det and 1/det are finite and the Suu columns of X
                   equal det I to |X - det I| <= 2^-45 |det|; otherwise the wave re-solves with partial pivoting.
  nopivot_solve    the previous product path: lu_solve4_nopivot (tile16_f64.h) with its growth check (every multiplier <= 4 and a
                   finite last reciprocal); a failed check re-solves with partial pivoting.

Every fused multiply-add of the kernel is an emulated fma here (exact product by Dekker's split, compensated sum: correctly rounded
except in double-rounding ties, within one ulp always).  The MFMA is modelled as a chain of fmas over k = 0..3 from a zero
accumulator.  v_rcp_f64 (measured relative error <= 4.6e-8) is modelled by 1/a rounded to fp32; fast_rcp's third-order correction
is then applied exactly as in the kernel.

reference_solve gives the exact answer to well below fp64 rounding for the matrices here: a fp64 solve refined twice with residuals
taken in long double.  riccati_blocks replays the oracle's recursion (oracle/zopt_oracle.py: discreteFiniteHorizonLqr) and returns
every step's (Suu, Sux).

    python tools/k1_solve_model.py       prints the guard's firing counts and the error ratios on the bench sets
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -53          # unit roundoff of fp64
TAU = 2.0 ** -45        # the kernel's residual threshold
_SPLIT = 134217729.0    # 2^27 + 1
_BIG = 1.7976931348623157e308


def _split(a):
    t = _SPLIT * a
    hi = t - (t - a)
    return hi, a - hi


def fma(a, b, c):
    """fl(a b + c) (see module doc).  Non-finite products and overflow fall back to the plain expression, as IEEE fma gives."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    with np.errstate(all="ignore"):
        p = a * b
        ah, al = _split(a)
        bh, bl = _split(b)
        e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
        s = p + c
        bb = s - p
        t = (p - (s - bb)) + (c - bb)
        r = s + (t + e)
        plain = p + c
    good = np.isfinite(r) & np.isfinite(p) & (np.abs(a) < 1e150) & (np.abs(b) < 1e150)
    return np.where(good, r, plain)


def v_rcp(a):
    with np.errstate(all="ignore"):
        return np.asarray(1.0 / np.asarray(a, np.float64), np.float32).astype(np.float64)


def fast_rcp(a):
    r = v_rcp(a)
    e = fma(-a, r, 1.0)
    return fma(r, fma(e, e, e), r)


def cofactor3(m):
    """tile16_f64.h cofactor3 on (..., 3, 3)."""
    with np.errstate(all="ignore"):
        t0 = fma(m[..., 1, 1], m[..., 2, 2], -(m[..., 1, 2] * m[..., 2, 1]))
        t1 = fma(m[..., 1, 0], m[..., 2, 2], -(m[..., 1, 2] * m[..., 2, 0]))
        t2 = fma(m[..., 1, 0], m[..., 2, 1], -(m[..., 1, 1] * m[..., 2, 0]))
        return fma(m[..., 0, 0], t0, fma(-m[..., 0, 1], t1, m[..., 0, 2] * t2))


def _minor_rows(g, cc):
    mr = [k + (k >= g) for k in range(3)]
    mc = [k + (k >= cc) for k in range(3)]
    if (g + cc) & 1:
        mr[1], mr[2] = mr[2], mr[1]
    return mr, mc


def cofactor_solve(Suu, Sux, details=False):
    """The product path on (..., 4, 4) and (..., 4, n).  Returns (L, admitted): L is the fast path's result wherever the guard
    admits and the pivoted re-solve elsewhere.  details: (L, admitted, ratio, L_fast) with the guard's residual ratio
    max|X - det I| / (TAU |det|) (the guard admits ratio <= 1; inf where det or 1/det is not finite) and the fast path's own result
    everywhere, admitted or not."""
    Suu = np.asarray(Suu, np.float64)
    Sux = np.asarray(Sux, np.float64)
    # signed cofactors C[g][cc] (lane (g, c) with c & 3 = cc)
    C = np.empty(Suu.shape)
    for g in range(4):
        for cc in range(4):
            mr, mc = _minor_rows(g, cc)
            C[..., g, cc] = cofactor3(Suu[..., mr, :][..., :, mc])
    S = np.concatenate([Sux, Suu], axis=-1)        # [Sux | Suu]: row g, column c
    n = Sux.shape[-1]
    # X[g][c] = sum_k adj[g][k] S[k][c], adj[g][k] = C[k][g]: fma chain over k from 0
    X = np.zeros(S.shape)
    for k in range(4):
        X = fma(C[..., k, :, None], S[..., k, None, :], X)
    det = X[..., 0, n]
    r = fast_rcp(det)
    with np.errstate(all="ignore"):
        L = X[..., :, :n] * r[..., None, None]
        eye = np.eye(4)
        res = np.abs(fma(-eye, det[..., None, None], X[..., :, n:]))
        finite = (np.abs(det) <= _BIG) & (np.abs(r) <= _BIG)
        ok = finite & np.all(res <= TAU * np.abs(det)[..., None, None], axis=(-2, -1))
        ratio = np.where(finite, np.max(res, axis=(-2, -1)) / (TAU * np.abs(det)), np.inf)
    if details:
        return _refit(L, ok, Suu, Sux), ok, np.where(np.isnan(ratio), np.inf, ratio), L
    return _refit(L, ok, Suu, Sux), ok


def nopivot_solve(Suu, Sux, details=False):
    """lu_solve4_nopivot on (..., 4, 4) and (..., 4, n), every right-hand side as in its own lane.  Returns (L, admitted); details:
    (L, admitted, L_fast) with the unpivoted result everywhere, whatever its check said."""
    S = np.asarray(Suu, np.float64)
    b = np.asarray(Sux, np.float64)
    lim = 4.0
    with np.errstate(all="ignore"):
        s = lambda i, j: S[..., i, j, None]
        r0 = fast_rcp(s(0, 0))
        f10, f20, f30 = s(1, 0) * r0, s(2, 0) * r0, s(3, 0) * r0
        ok = (np.abs(f10) <= lim) & (np.abs(f20) <= lim) & (np.abs(f30) <= lim)
        a11, a12, a13, b1 = fma(-f10, s(0, 1), s(1, 1)), fma(-f10, s(0, 2), s(1, 2)), fma(-f10, s(0, 3), s(1, 3)), fma(-f10, b[..., 0, :], b[..., 1, :])
        a21, a22, a23, b2 = fma(-f20, s(0, 1), s(2, 1)), fma(-f20, s(0, 2), s(2, 2)), fma(-f20, s(0, 3), s(2, 3)), fma(-f20, b[..., 0, :], b[..., 2, :])
        a31, a32, a33, b3 = fma(-f30, s(0, 1), s(3, 1)), fma(-f30, s(0, 2), s(3, 2)), fma(-f30, s(0, 3), s(3, 3)), fma(-f30, b[..., 0, :], b[..., 3, :])
        r1 = fast_rcp(a11)
        f21, f31 = a21 * r1, a31 * r1
        ok &= (np.abs(f21) <= lim) & (np.abs(f31) <= lim)
        c22, c23, d2 = fma(-f21, a12, a22), fma(-f21, a13, a23), fma(-f21, b1, b2)
        c32, c33, d3 = fma(-f31, a12, a32), fma(-f31, a13, a33), fma(-f31, b1, b3)
        r2 = fast_rcp(c22)
        f32 = c32 * r2
        ok &= np.abs(f32) <= lim
        e33, g3 = fma(-f32, c23, c33), fma(-f32, d2, d3)
        r3 = fast_rcp(e33)
        ok &= np.abs(r3) <= _BIG
        x3 = g3 * r3
        x2 = fma(-c23, x3, d2) * r2
        x1 = fma(-a13, x3, fma(-a12, x2, b1)) * r1
        x0 = fma(-s(0, 3), x3, fma(-s(0, 2), x2, fma(-s(0, 1), x1, b[..., 0, :]))) * r0
    L = np.stack([x0, x1, x2, x3], axis=-2)
    okw = np.all(ok, axis=-1)                      # the wave-uniform vote over the right-hand sides
    if details:
        return _refit(L, okw, Suu, Sux), okw, L
    return _refit(L, okw, Suu, Sux), okw


def _refit(L, ok, Suu, Sux):
    """L where the guard admitted, the pivoted re-solve elsewhere."""
    L = np.array(L)
    bad = ~ok
    if bad.any():
        L[bad] = pivoted_solve(Suu[bad], Sux[bad])
    return L


def pivoted_solve(Suu, Sux):
    """The re-solve (lu_solve4_fallback): LU with partial pivoting as getrf; a NaN anywhere in Suu gives all-NaN."""
    Suu = np.asarray(Suu, np.float64)
    Sux = np.asarray(Sux, np.float64)
    out = np.full(Sux.shape, np.nan)
    flat_S, flat_b, flat_o = Suu.reshape(-1, 4, 4), Sux.reshape(-1, 4, Sux.shape[-1]), out.reshape(-1, 4, Sux.shape[-1])
    has_nan = np.isnan(flat_S).any(axis=(-2, -1))
    for i in np.nonzero(~has_nan)[0]:
        flat_o[i] = _lu4(flat_S[i].copy(), flat_b[i].copy())
    return flat_o.reshape(Sux.shape)


def _lu4(S, b):
    with np.errstate(all="ignore"):
        for k in range(4):
            p = k + int(np.argmax(np.abs(S[k:, k])))
            if p != k:
                S[[k, p]] = S[[p, k]]
                b[[k, p]] = b[[p, k]]
            rinv = 1.0 / S[k, k]
            for i in range(k + 1, 4):
                f = S[i, k] * rinv
                S[i, k + 1:] = S[i, k + 1:] - f * S[k, k + 1:]
                b[i] = b[i] - f * b[k]
        x = np.empty_like(b)
        for k in range(3, -1, -1):
            x[k] = (b[k] - S[k, k + 1:] @ x[k + 1:]) / S[k, k]
    return x


def reference_solve(Suu, Sux, iters=2):
    """Suu^-1 Sux to well below fp64 rounding (condition numbers up to ~1e12): fp64 solve, refined with long-double residuals."""
    Suu = np.asarray(Suu, np.float64)
    Sux = np.asarray(Sux, np.float64)
    Sl, bl = Suu.astype(np.longdouble), Sux.astype(np.longdouble)
    X = np.linalg.solve(Suu, Sux).astype(np.longdouble)
    for _ in range(iters):
        res = bl - np.einsum("...ik,...kj->...ij", Sl, X)
        X = X + np.linalg.solve(Suu, res.astype(np.float64)).astype(np.longdouble)
    return X


def rel_err(L, Lref):
    """Per matrix: max |L - Lref| / max |Lref| (the project's normwise measure), in long double."""
    d = np.max(np.abs(L.astype(np.longdouble) - Lref), axis=(-2, -1))
    s = np.max(np.abs(Lref), axis=(-2, -1))
    return (d / np.maximum(s, np.longdouble(1e-300))).astype(np.float64)


def riccati_blocks(A, B, Q, R):
    """Every step's (Suu, Sux) of the oracle's recursion on (..., T, n, n) inputs: arrays (..., T, m, m) and (..., T, m, n)."""
    A, B, Q, R = (np.asarray(x, np.float64) for x in (A, B, Q, R))
    T = A.shape[-3]
    tr = lambda X: np.swapaxes(X, -1, -2)
    V = Q[..., -1, :, :]
    Suu = np.empty(R.shape)
    Sux = np.empty(B.shape[:-2] + (B.shape[-1], B.shape[-2]))
    with np.errstate(all="ignore"):
        for k in range(T - 1, -1, -1):
            Ak, Bk, Qk, Rk = A[..., k, :, :], B[..., k, :, :], Q[..., k, :, :], R[..., k, :, :]
            BtV = tr(Bk) @ V
            S, Sx = Rk + BtV @ Bk, BtV @ Ak
            Suu[..., k, :, :], Sux[..., k, :, :] = S, Sx
            Lk = np.linalg.solve(S, Sx)
            Acl = Ak - Bk @ Lk
            V = Qk + (tr(Lk) @ Rk) @ Lk + (tr(Acl) @ V) @ Acl
    return Suu, Sux


def bench_blocks(seed):
    """bench.py's default K1 inputs: problems.random_lti_systems(4096, 12, 4, seed) tiled over T = 50 (409 600 steps)."""
    from tests import problems
    A1, B1, Q1, R1 = problems.random_lti_systems(4096, 12, 4, seed=seed)
    Suu, Sux = riccati_blocks(*problems.tile_over_horizon(A1, B1, Q1, R1, 50))
    return Suu.reshape(-1, 4, 4), Sux.reshape(-1, 4, 12)


def main():
    for seed in (0, 1):
        Suu, Sux = bench_blocks(seed)
        Lc, okc = cofactor_solve(Suu, Sux)
        Ln, okn = nopivot_solve(Suu, Sux)
        Lr = reference_solve(Suu, Sux)
        ec, en = rel_err(Lc, Lr), rel_err(Ln, Lr)
        print(f"bench seed {seed}: {len(Suu)} matrices, cofactor guard fires on {int((~okc).sum())}, growth check on {int((~okn).sum())}; "
              f"max err cofactor {ec.max():.2e} nopivot {en.max():.2e}; "
              f"max err_cof / max(err_nopivot, u) {np.max(ec / np.maximum(en, U)):.2f}")


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    main()
