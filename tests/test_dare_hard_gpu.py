"""GPU tests of discreteInfiniteHorizonLqr (zm_dare_f64) on hard spectra, through both of its kernels: the tile-16 register kernel
(n <= 12, m <= 4) and the fp64 tile kernel's DARE instantiation (lqr_tiled_core.h, DARE = true) beyond.

The reference is the Newton-refined DARE solution of tests/hp_reference.py (residual <= 1e-16, pinned by tests/test_hp_reference.py,
which also shows that every generator has its hard feature).  Value iteration stopped at max|V' - V| <= tol max|V'| leaves an
error of about tol / (1 - rho_cl^2) in V, so the bound per design is  max(1e-10, 1e-12 / (1 - rho_cl^2)) * max|ref|."""
import functools

import numpy as np
import pytest

from tests import hp_reference as hp
from tests import problems

pytestmark = pytest.mark.gpu

SMALL = [(12, 4), (8, 2)]                       # dare_t16_f64
TILED = [(16, 4), (12, 6), (33, 7), (64, 16)]   # lqr_backward_tiled<TileF64, NT, ..., DARE = true>


@pytest.fixture(scope="module")
def lqr():
    import torch
    assert torch.cuda.is_available()
    from zopt_amd import lqrUtils
    return lqrUtils


@functools.lru_cache(maxsize=None)
def _case(name, n, m):
    A, B, Q, R = problems.hard_dare(name, n, m)
    return (A, B, Q, R), [hp.dare_refined(A[i], B[i], Q[i], R[i]) for i in range(A.shape[0])]


def _rel(X, ref):
    return float(np.max(np.abs(X - ref)) / np.max(np.abs(ref)))


@pytest.mark.parametrize("name", sorted(problems.HARD_DARE))
@pytest.mark.parametrize("n,m", SMALL + TILED)
def test_hard_spectrum_matches_refined_dare(lqr, name, n, m):
    (A, B, Q, R), refs = _case(name, n, m)
    L, P, its = lqr.discreteInfiniteHorizonLqr(A, B, Q, R, return_value=True)
    for i, (Lr, Pr, rho, _) in enumerate(refs):
        tol = max(1e-10, 1e-12 / (1.0 - rho ** 2))
        eL, eP = _rel(L[i], Lr.astype(np.float64)), _rel(P[i], Pr.astype(np.float64))
        assert its[i] > 0, (i, its[i])
        assert eL <= tol and eP <= tol, (i, int(its[i]), eL, eP, rho)
        # the returned gain is the gain of the returned value matrix
        a, b, r = A[i], B[i], R[i]
        Lp = np.linalg.solve(r + b.T @ P[i] @ b, b.T @ P[i] @ a)
        assert np.max(np.abs(L[i] - Lp)) <= 1e-10 * np.max(np.abs(L[i])), (i, int(its[i]))


def test_cross_path_identity(lqr):
    """a (12, 4) design (tile-16 kernel) and the same design with a 5th input that B does not use and R = blockdiag(R, 1) (m = 5:
    the tiled kernel) have the same value and the same gain on the first four inputs; the unused input's gain is exactly 0"""
    A, B, Q, R = problems.random_lti_systems(3, 12, 4, seed=21, rho=0.95)
    B5 = np.concatenate([B, np.zeros((3, 12, 1))], axis=2)
    R5 = np.zeros((3, 5, 5))
    R5[:, :4, :4] = R
    R5[:, 4, 4] = 1.0
    L4, P4, k4 = lqr.discreteInfiniteHorizonLqr(A, B, Q, R, return_value=True)
    L5, P5, k5 = lqr.discreteInfiniteHorizonLqr(A, B5, Q, R5, return_value=True)
    assert np.all(k4 > 0) and np.all(k5 > 0)
    for i in range(3):
        assert _rel(L5[i, :4], L4[i]) <= 1e-12 and _rel(P5[i], P4[i]) <= 1e-12, (i, int(k4[i]), int(k5[i]))
        assert np.all(L5[i, 4] == 0)


def test_exact_cap_on_tiled_path(lqr):
    """convergence EXACTLY on the last allowed iteration is convergence on the tiled path too: a design that needs k iterations is
    accepted with maxIter = k and refused with maxIter = k - 8 (the test runs every 8th iteration)"""
    A, B, Q, R = problems.random_lti_systems(1, 16, 4, seed=3)
    L1, P1, k = lqr.discreteInfiniteHorizonLqr(A, B, Q, R, return_value=True)
    k = int(k[0])
    assert k > 16 and k % 8 == 0
    L2, P2, k2 = lqr.discreteInfiniteHorizonLqr(A, B, Q, R, maxIter=k, return_value=True)
    assert int(k2[0]) == k and np.array_equal(L1, L2) and np.array_equal(P1, P2)
    assert np.array_equal(lqr.discreteInfiniteHorizonLqr(A, B, Q, R, maxIter=k), L1)      # no LinAlgError
    _, _, k3 = lqr.discreteInfiniteHorizonLqr(A, B, Q, R, maxIter=k - 8, return_value=True)
    assert int(k3[0]) == -(k - 8)
    with pytest.raises(np.linalg.LinAlgError):
        lqr.discreteInfiniteHorizonLqr(A, B, Q, R, maxIter=k - 8)


@pytest.mark.parametrize("n,m", [(16, 4), (64, 16)])
def test_not_stabilizable_on_tiled_path(lqr, n, m):
    """an unstable mode (lambda = 2) that the input cannot reach: the value overflows while the gain has long converged; the
    iteration must not report that as convergence (SciPy raises LinAlgError there)"""
    A, B, Q, R = problems.slow_unreachable_mode(2, n, m, seed=8, lam=2.0)
    with pytest.raises(np.linalg.LinAlgError):
        lqr.discreteInfiniteHorizonLqr(A, B, Q, R)
