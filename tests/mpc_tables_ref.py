"""Long-double references for the Riccati tables of the MPC setup kernels (zm_mpc_setup_f64, zm_mpc_setup_batched_f64,
zm_mpc_setup_ltv_f64, zm_mpc_setup_ltv_stage_f64) and the cases of tests/test_mpc_tables.py / tests/test_mpc_tables_gpu.py, computed
once per process (TEST INFRASTRUCTURE ONLY; not collected by pytest).

  * `tables_ld`            -- the tables K, Minv, D in `np.longdouble` with the value update in Joseph form, symmetrised: the reference;
  * `tables_ld_plain`      -- the same tables with the symmetrised NON-Joseph update (the kernels' formula, symmetrised) in long double:
                              an independent formula the reference is cross-checked against;
  * `tables_unsymmetrised` -- the fp64 recursion WITHOUT symmetrisation, the formula the setup kernels had: kept for the one CPU test that
                              shows the unstable families tell the two recursions apart;
  * `lqr_rollout_ld`       -- the minimiser of the box-free problem (finite-horizon affine LQR) in long double, for the end-to-end tests;
  * `case`, `case_bound`   -- inputs, reference, the fp64 oracle's own error (`oracle.mpc_oracle.riccati_tables`, never a kernel) in
                              `hp_reference.sweep_metric` per (problem, level), and the bound `hp_reference.sweep_bounds` derived from it.

All in the stage form zm_mpc_setup_ltv_stage_f64 documents: A (P, N, n, n), B (P, N, n, m), c (P, N, n) or None, Qs (P, N, n, n) with
Qs[k] the weight of x_{k+1} (row N - 1 terminal), Rs (P, N, m, m), rho (P, L); K (P, L, N, m, n), Minv (P, L, N, m, m), D (P, L, N, n).
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import mpc_oracle as mo
from tests import problems
from tests.hp_reference import LD, _T, _mv, solve_ld, sweep_bounds, sweep_metric

CAP = 1e-7      # every admitted case's bound stays below this (tests/test_mpc_tables.py): an oracle that is itself wrong grants no bound


def _levels(A, B, c, Qs, Rs, rho):
    """The operands in long double with a level axis: (P, 1, N, ...) against rho (P, L)."""
    A, B, Qs, Rs = (np.asarray(X, dtype=LD)[:, None] for X in (A, B, Qs, Rs))
    n = A.shape[-1]
    c = np.zeros(A.shape[:3] + (n,), dtype=LD) if c is None else np.asarray(c, dtype=LD)[:, None]
    return A, B, c, Qs, Rs, np.asarray(rho, dtype=LD)


def _tables(A, B, c, Qs, Rs, rho, joseph):
    A, B, c, Qs, Rs, rho = _levels(A, B, c, Qs, Rs, rho)
    Pn, L = rho.shape
    N, n, m = B.shape[-3:]
    In, Im = np.eye(n, dtype=LD), np.eye(m, dtype=LD)
    rI = lambda I: rho[:, :, None, None] * I      # noqa: E731
    V = np.broadcast_to(2 * Qs[:, :, N - 1] + rI(In), (Pn, L, n, n))
    K, Mi, D = np.empty((Pn, L, N, m, n), dtype=LD), np.empty((Pn, L, N, m, m), dtype=LD), np.empty((Pn, L, N, n), dtype=LD)
    for k in range(N - 1, -1, -1):
        Ak, Bk = A[:, :, k], B[:, :, k]
        D[:, :, k] = _mv(V, np.broadcast_to(c[:, :, k], (Pn, L, n)))
        Hu = 2 * Rs[:, :, k] + rI(Im)
        BtV = _T(Bk) @ V
        Suu = Hu + BtV @ Bk
        Sux = BtV @ Ak
        Mi[:, :, k] = solve_ld(Suu, np.broadcast_to(Im, (Pn, L, m, m)))
        K[:, :, k] = Mi[:, :, k] @ Sux
        Hx = 2 * Qs[:, :, max(k - 1, 0)] + rI(In)
        if joseph:
            Acl = Ak - Bk @ K[:, :, k]
            V = Hx + (_T(K[:, :, k]) @ Hu) @ K[:, :, k] + (_T(Acl) @ V) @ Acl
        else:
            V = Hx + (_T(Ak) @ V) @ Ak - _T(Sux) @ K[:, :, k]
        V = (V + _T(V)) / 2
    return K, Mi, D


def tables_ld(A, B, c, Qs, Rs, rho):
    """The reference: P_N = 2 Qs_{N-1} + rho I;  D_k = P_{k+1} c_k;  Suu_k = 2 Rs_k + rho I + B_k' P B_k;  Minv_k = Suu_k^-1 (`solve_ld`);
    K_k = Minv_k B_k' P A_k;  P <- sym((2 Qs_{k-1} + rho I) + K_k' (2 Rs_k + rho I) K_k + A_cl' P A_cl), A_cl = A_k - B_k K_k -- the
    Joseph form, a sum of positive semidefinite terms, symmetrised.  Long double throughout; returns (K, Minv, D)."""
    return _tables(A, B, c, Qs, Rs, rho, True)


def tables_ld_plain(A, B, c, Qs, Rs, rho):
    """`tables_ld` with the value update P <- sym((2 Qs_{k-1} + rho I) + A_k' P A_k - (B_k' P A_k)' K_k): the other formula."""
    return _tables(A, B, c, Qs, Rs, rho, False)


def tables_unsymmetrised(A, B, c, Qs, Rs, rho):
    """fp64, P <- (2 Qs_{k-1} + rho I) + A_k' P A_k - (B_k' P A_k)' K_k with NO symmetrisation: the recursion the setup kernels ran before
    their value matrix was stored symmetrised.  For tests/test_mpc_tables.py: test_unsymmetrised_recursion_fails_on_lti_unstable only."""
    A, B, Qs, Rs = (np.asarray(X, dtype=np.float64) for X in (A, B, Qs, Rs))
    Pn, L = np.shape(rho)
    N, n, m = B.shape[-3:]
    c = np.zeros((Pn, N, n)) if c is None else np.asarray(c, dtype=np.float64)
    K, Mi, D = np.empty((Pn, L, N, m, n)), np.empty((Pn, L, N, m, m)), np.empty((Pn, L, N, n))
    for p in range(Pn):
        for l in range(L):
            r_ = rho[p][l]
            V = 2 * Qs[p, N - 1] + r_ * np.eye(n)
            for k in range(N - 1, -1, -1):
                D[p, l, k] = V @ c[p, k]
                Suu = (2 * Rs[p, k] + r_ * np.eye(m)) + B[p, k].T @ V @ B[p, k]
                Sux = B[p, k].T @ V @ A[p, k]
                Mi[p, l, k] = np.linalg.inv(Suu)
                K[p, l, k] = Mi[p, l, k] @ Sux
                V = (2 * Qs[p, max(k - 1, 0)] + r_ * np.eye(n)) + A[p, k].T @ V @ A[p, k] - Sux.T @ K[p, l, k]
    return K, Mi, D


def tables_oracle(A, B, c, Qs, Rs, rho):
    """`oracle.mpc_oracle.riccati_tables`, the fp64 restatement of the kernels, for every (problem, level)."""
    Pn, L = np.shape(rho)
    out = [[mo.riccati_tables(A[p], B[p], None if c is None else c[p], Qs[p], Rs[p], float(rho[p][l])) for l in range(L)] for p in range(Pn)]
    return tuple(np.stack([np.stack([out[p][l][i] for l in range(L)]) for p in range(Pn)]) for i in range(3))


def lqr_rollout_ld(A, B, c, Qs, Rs, x0):
    """The minimiser of sum_k x_{k+1}' Qs_k x_{k+1} + u_k' Rs_k u_k over x+ = A_k x + B_k u + c_k from x0, no box: the w-update of the ADMM
    at rho = 0, in long double.  ONE problem: A (N, n, n), B (N, n, m), c (N, n) or None, x0 (..., n).  Returns (x (..., N+1, n), u (..., N, m))
    in long double."""
    N, n, m = np.shape(B)
    K, Mi, D = (T[0, 0] for T in tables_ld(A[None], B[None], None if c is None else c[None], Qs[None], Rs[None], np.zeros((1, 1))))
    A, B = np.asarray(A, dtype=LD), np.asarray(B, dtype=LD)
    c = np.zeros((N, n), dtype=LD) if c is None else np.asarray(c, dtype=LD)
    kf = np.empty((N, m), dtype=LD)
    p = D[N - 1]
    for k in range(N - 1, -1, -1):
        qu = B[k].T @ p
        kf[k] = Mi[k] @ qu
        p = (D[k - 1] if k >= 1 else 0) + A[k].T @ p - K[k].T @ qu
    x = [np.asarray(x0, dtype=LD)]
    u = []
    for k in range(N):
        u.append(-_mv(K[k], x[-1]) - kf[k])
        x.append(_mv(A[k], x[-1]) + _mv(B[k], u[-1]) + c[k])
    return np.stack(x, axis=-2), np.stack(u, axis=-2)


def table_errors(name, n, out, ref):
    """(error of K, of Minv, of D), each (P * L, N): `sweep_metric` per (problem, level); K of `badly_scaled` measured as K diag(d) so that
    every column counts (as tests/hard_cases.py measures L)."""
    sc = problems.sweep_scaling(n) if name == "badly_scaled" else 1.0
    flat = lambda X: np.asarray(X).reshape((-1,) + np.shape(X)[2:])      # noqa: E731
    return (sweep_metric(flat(out[0] * sc), flat(ref[0] * sc)), sweep_metric(flat(out[1]), flat(ref[1])),
            sweep_metric(flat(out[2]), flat(ref[2])))


@functools.lru_cache(maxsize=None)
def case(name, n, m, N, P=2):
    """args: `problems.hard_mpc`; ref: `tables_ld`; e: the oracle's largest error on (K, Minv, D)."""
    args = problems.hard_mpc(name, n, m, N, P)
    ref = tables_ld(*args)
    e = tuple(float(np.max(x)) for x in table_errors(name, n, tables_oracle(*args), ref))
    return {"args": args, "ref": ref, "e": e}


def case_bound(name, n, m, N):
    """(bound on K, on Minv, on D): 100 x max(the oracle's error on the case, its error on `plain` at the same shape)."""
    c, p = case(name, n, m, N), case("plain", n, m, N)
    return tuple(sweep_bounds(c["e"][i], p["e"][i]) for i in range(3))


ALL_CASES = [(name, n, m, N) for (n, m, N) in problems.MPC_TABLE_SHAPES for name in problems.MPC_FAMILIES]
