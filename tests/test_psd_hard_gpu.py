"""Hard-spectrum GPU tests of the stand-alone PD projection V max(w, eps) V^T: `ensurePositiveDefinite` on the one-tile kernel
(ns16.h, k <= 16) and on all three tile counts of psd_tiled.hip (16 < k <= 64), and `conditionQuadraticCost` on the same matrices split
into blocks, against an EXACT reference: the matrices are built from a planted spectrum (hp_reference.psd_from_spectrum_ld: U diag(w)
U^T with U a product of Householder reflectors in long double), so the projection U max(w, eps) U^T is known without any eigensolve.
The spectra are the eight adversarial kinds of tests/problems.py.  Bound: 2e-11 relative to max(max|ref|, eps), the project's figure
for the matrix-sign iteration (ns16.h), here at every tile count; and the smallest eigenvalue of every result is >= eps (1 - 1e-6).
Every second matrix is handed over NONSYMMETRIC -- its upper triangle doubled, its lower one zero, so that (a + a^T) / 2 is the planted
matrix bit for bit: `eigh` symmetrises its input, and so must the kernels."""
import functools

import numpy as np
import pytest

from tests import hp_reference as hp
from tests import problems

pytestmark = pytest.mark.gpu
EPS = 1e-3
RTOL = 2e-11
PER_CASE = 4


@pytest.fixture(scope="module")
def ilqr():
    import torch
    assert torch.cuda.is_available()
    from zopt_amd import ilqrUtils
    return ilqrUtils


@functools.lru_cache(maxsize=None)
def planted(kind, k):
    """(matrices (PER_CASE, k, k) fp64, long-double projections) of spectrum kind `kind`; "zero_rows": a planted block on the live
    indices, the others' rows and columns exactly zero (they project to eps on the diagonal)."""
    rng = np.random.default_rng(1000 * kind + k)
    A, P = np.zeros((PER_CASE, k, k)), np.zeros((PER_CASE, k, k), dtype=np.longdouble)
    for i in range(PER_CASE):
        live = np.arange(k)
        if problems.ADVERSARIAL_SPECTRA[kind] == "zero_rows":
            live = np.sort(rng.choice(k, size=k - max(1, k // 3), replace=False))
        a, p, _ = hp.psd_from_spectrum_ld(live.size, problems.adversarial_spectrum(kind, live.size, rng), int(rng.integers(1 << 31)), EPS)
        P[i] = EPS * np.eye(k)
        A[i][np.ix_(live, live)] = a
        P[i][np.ix_(live, live)] = p
    return A, P


def _one_sided(a):
    """2 triu(a, 1) + diag(a): nonsymmetric, and (x + x^T) / 2 == a exactly"""
    return 2 * np.triu(a, 1) + a * np.eye(a.shape[-1])


def _hold(what, kind, k, out, ref):
    err = [float(np.max(np.abs(o - r)) / max(float(np.max(np.abs(r))), EPS)) for o, r in zip(out, ref)]
    wmin = [float(np.min(np.linalg.eigvalsh(0.5 * (o + o.T)))) for o in np.asarray(out, dtype=np.float64)]
    print(f"HARD psd {what} {problems.ADVERSARIAL_SPECTRA[kind]} k={k}: kernel {max(err):.1e} | bound {RTOL:.0e} | min eig / eps {min(wmin) / EPS:.9f}")
    assert max(err) <= RTOL, err
    assert min(wmin) >= EPS * (1 - 1e-6), wmin


@pytest.mark.parametrize("kind", range(len(problems.ADVERSARIAL_SPECTRA)))
@pytest.mark.parametrize("k", problems.PSD_SIZES)
def test_ensurePositiveDefinite_planted_spectra(ilqr, k, kind):
    A, P = planted(kind, k)
    A = A.copy()
    A[1::2] = _one_sided(A[1::2])
    assert np.array_equal(0.5 * (A + np.swapaxes(A, -1, -2)), planted(kind, k)[0])
    out = ilqr.ensurePositiveDefinite(A)
    assert out.shape == A.shape
    _hold("project", kind, k, out, P)


@pytest.mark.parametrize("kind", range(len(problems.ADVERSARIAL_SPECTRA)))
@pytest.mark.parametrize("n,m", [(12, 4), (40, 8)])
def test_conditionQuadraticCost_planted_spectra(ilqr, n, m, kind):
    from zopt_amd import pytrees as pt
    A, P = planted(kind, n + m)
    z = np.zeros(PER_CASE)
    c_xx, c_ux, c_uu = (np.ascontiguousarray(X) for X in (A[:, :n, :n], A[:, n:, :n], A[:, n:, n:]))
    c_xx[1::2], c_uu[1::2] = _one_sided(c_xx[1::2]), _one_sided(c_uu[1::2])          # nonsymmetric diagonal blocks
    cost = pt.QuadraticCostFunction(z, np.zeros((PER_CASE, n)), np.zeros((PER_CASE, m)), c_xx, c_ux, c_uu)
    out = ilqr.conditionQuadraticCost(cost)
    Z = np.block([[np.asarray(out.c_xx), np.swapaxes(np.asarray(out.c_ux), -1, -2)], [np.asarray(out.c_ux), np.asarray(out.c_uu)]])
    _hold("condition-cost", kind, n + m, Z, P)
