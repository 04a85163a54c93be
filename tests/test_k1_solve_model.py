"""CPU model of K1's m x m solve (tools/k1_solve_model.py): the cofactor solve on v_mfma_f64_4x4x4_4b and its guard, against the
unpivoted LU it replaced, on every Riccati step of the bench inputs, of the K1 inputs of tests/test_lqr_gpu.py, of the hard-spectrum
families, and on graded, near-singular, singular and non-finite matrices.

Error measure: per matrix, max |L - L_ref| / max |L_ref| (the project's normwise measure), L_ref = Suu^-1 Sux from a fp64 solve
refined with long-double residuals (error <= kappa * 2^-64 + (kappa * 2^-53)^5 for condition number kappa: far below the errors
measured here on every matrix the guard admits).

The bound on every matrix the guard admits:  err_cofactor <= F * max(err_nopivot, u),  u = 2^-53,  F = TAU / u = 2^8.
  * The floor u: an error below one rounding of the output is not a property of either solve.  The fp64 output alone is off from
    L_ref by up to u/2 per entry, and an LU error that happens to cancel to below that says nothing about the method.
  * F = TAU / u: the guard admits a matrix only when the Suu columns of X = adj(Suu) [Sux | Suu] are det I to TAU |det|.  Those
    entries are computed by the same cofactors and the same MFMA sums as the Sux columns, so their deviation is the cofactor path's
    own rounding error relative to det, and an admitted matrix's gains carry a relative error of about TAU.  The test asserts that
    this a-posteriori estimate holds: no admitted matrix is worse than TAU / u roundings of the output, or than TAU / u times the
    unpivoted LU's error where that is larger.
  * TAU = 2^-45 itself comes from the model (tools/k1_solve_model.py): the largest residual on the 409 600 bench matrices is 87 u,
    so the smallest power of two that none of them reaches, 2^-46 = 128 u, is doubled for margin against the GPU's different
    rounding of Suu and Sux.
"""
import math
from fractions import Fraction

import numpy as np
import pytest

from tests import problems
from tools import k1_solve_model as km

U = 2.0 ** -53
F = km.TAU / U


def _check_admitted(Suu, Sux, label):
    Lc, okc = km.cofactor_solve(Suu, Sux)
    Ln, _ = km.nopivot_solve(Suu, Sux)
    Lr = km.reference_solve(Suu, Sux, iters=4)
    ec, en = km.rel_err(Lc, Lr), km.rel_err(Ln, Lr)
    ratio = np.where(okc, ec / np.maximum(en, U), 0.0)
    worst = int(np.argmax(ratio))
    print(f"{label}: {okc.size} matrices, guard fires on {int((~okc).sum())}; admitted: max err cofactor {ec[okc].max() if okc.any() else 0:.2e}, "
          f"nopivot {en[okc].max() if okc.any() else 0:.2e}; max err_cof / max(err_nopivot, u) = {ratio.max():.2f}")
    assert np.all(ratio <= F), (label, worst, ec[worst], en[worst])
    return okc


def test_fma_emulation_is_correctly_rounded():
    """The model's fma against exact rational arithmetic: within one ulp everywhere, and correctly rounded (Python's float() of a
    Fraction rounds to nearest even) on all but the rare double-rounding ties."""
    rng = np.random.default_rng(3)
    a, b, c = (rng.standard_normal(4000) * 10.0 ** rng.integers(-8, 8, 4000) for _ in range(3))
    got = km.fma(a, b, c)
    exact = np.array([float(Fraction(x) * Fraction(y) + Fraction(z)) for x, y, z in zip(a, b, c)])
    assert np.all(np.abs(got - exact) <= np.spacing(np.abs(exact)))
    assert np.mean(got == exact) >= 0.999


def test_cofactor_layout_gives_adjugate():
    """The lanes' minors and signs: on an integer matrix every step is exact, so X = adj(S) [Sux | Suu] has det(S) I in the Suu
    columns and the solve is exact."""
    S = np.array([[4.0, 1, 2, 0], [1, 5, 0, 2], [3, 0, 6, 1], [0, 2, 1, 7]])
    Sx = np.arange(48, dtype=np.float64).reshape(4, 12) - 20
    L, ok = km.cofactor_solve(S[None], Sx[None])
    assert ok[0]
    exact = np.linalg.solve(S, Sx)
    assert np.max(np.abs(L[0] - exact)) <= 4 * U * np.max(np.abs(exact))


@pytest.mark.parametrize("seed", [0, 1])
def test_bench_sets_never_take_the_fallback(seed):
    """bench.py's inputs (random_lti_systems(4096, 12, 4, seed) over T = 50): the guard admits all 204 800 steps of each set, so
    the pivoted re-solve never runs in the timed path, and the cofactor solve is within F of the unpivoted LU on every one."""
    Suu, Sux = km.bench_blocks(seed)
    ok = _check_admitted(Suu, Sux, f"bench seed {seed}")
    assert ok.size == 204800 and int((~ok).sum()) == 0


def _k1_inputs_of_test_lqr_gpu():
    """The inputs of tests/test_lqr_gpu.py that run K1 (n in {8, 12}, m = 4), built as that file builds them."""
    out = []
    for n, m, T, batch in [(12, 4, 50, 64), (8, 4, 100, 5), (12, 4, 1, 3), (12, 4, 2, 3), (12, 4, 3, 3), (12, 4, 4, 2)]:
        out.append((f"parity {n},{m},{T},{batch}", problems.random_time_varying(batch, T, n, m, seed=1000 * n + 10 * m + T)))
    out.append(("extra leading axes", problems.random_time_varying(6, 8, 12, 4, seed=9)))
    rng = np.random.default_rng(42)
    A, B, Q, R = problems.random_time_varying(16, 6, 12, 4, seed=77)
    P = np.eye(4)[[2, 0, 3, 1]]
    out.append(("permuted-dominant R", (A, B, Q, R @ P * 3.0 + 0.1 * rng.standard_normal(R.shape))))
    A1, B1, Q1, R1 = problems.random_lti_systems(8, 12, 4, seed=5, rho=1.2)
    R1[:] = 1e-6 * np.eye(4)
    out.append(("cheap control R = 1e-6 I", problems.tile_over_horizon(A1, B1, Q1, R1, 50)))
    out.append(("torch tensors", problems.random_time_varying(32, 20, 12, 4, seed=3)))
    return out


@pytest.mark.parametrize("label,inputs", _k1_inputs_of_test_lqr_gpu(), ids=lambda x: x if isinstance(x, str) else "")
def test_k1_inputs_of_the_gpu_tests(label, inputs):
    Suu, Sux = km.riccati_blocks(*inputs)
    _check_admitted(Suu.reshape(-1, 4, 4), Sux.reshape(-1, 4, Sux.shape[-1]), label)


@pytest.mark.parametrize("name", sorted(problems.HARD_DARE))
@pytest.mark.parametrize("n", [8, 12])
def test_hard_families(name, n):
    A1, B1, Q1, R1 = problems.HARD_DARE[name](64, n, 4, seed=1000 + 97 * n + 4)
    Suu, Sux = km.riccati_blocks(*problems.tile_over_horizon(A1, B1, Q1, R1, 50))
    _check_admitted(Suu.reshape(-1, 4, 4), Sux.reshape(-1, 4, n), f"{name} n={n}")


def _well(rng, k):
    M = rng.standard_normal((k, 4, 4))
    return M @ np.swapaxes(M, -1, -2) / 4 + np.eye(4)


def test_graded_matrices():
    """Rows and columns scaled over up to twelve decades: D S D and D S, S well conditioned."""
    rng = np.random.default_rng(11)
    Suu, Sux = [], []
    for e in (2, 4, 6, 8, 12):
        D = np.diag(np.logspace(0, -e, 4))
        for S in _well(rng, 200):
            Suu += [D @ S @ D, D @ S, S @ D]
            Sux += [rng.standard_normal((4, 12)) for _ in range(3)]
    _check_admitted(np.array(Suu), np.array(Sux), "graded")


def test_near_singular_matrices():
    """Condition numbers 1e2 .. 1e14 (random orthogonal factors), and one dominant direction (s v v^T + I, all rows nearly
    parallel): where the guard admits, the bound holds; from kappa = 1e10 on it fires on every matrix."""
    rng = np.random.default_rng(12)
    Suu, Sux, kap = [], [], []
    for e in range(2, 15):
        for _ in range(100):
            Q1, _ = np.linalg.qr(rng.standard_normal((4, 4)))
            Q2, _ = np.linalg.qr(rng.standard_normal((4, 4)))
            s = np.array([1.0, 10.0 ** (-e * rng.uniform(0, 1)), 10.0 ** (-e * rng.uniform(0, 1)), 10.0 ** -e])
            Suu.append(Q1 @ np.diag(s) @ Q2.T)
            Sux.append(rng.standard_normal((4, 12)))
            kap.append(10.0 ** e)
    for e in range(1, 9):
        for _ in range(100):
            v = rng.standard_normal(4)
            Suu.append(10.0 ** e * np.outer(v, v) + np.eye(4) + 0.1 * rng.standard_normal((4, 4)))
            Sux.append(rng.standard_normal((4, 12)))
            kap.append(0.0)
    Suu, Sux, kap = np.array(Suu), np.array(Sux), np.array(kap)
    ok = _check_admitted(Suu, Sux, "near-singular")
    assert not np.any(ok[kap >= 1e10])


def test_singular_and_nonfinite_fire_the_guard():
    """Exactly singular Suu (zero, rank 3, rank 1) and NaN / inf anywhere in Suu: the guard fires on every one, and the re-solve
    gives non-finite gains (test_lqr_gpu.py::test_singular_system_propagates_nonfinite_without_fault: R = 0, B = 0)."""
    rng = np.random.default_rng(13)
    Suu, Sux = [np.zeros((4, 4))], [np.zeros((4, 12))]
    for _ in range(50):
        M = rng.standard_normal((4, 3))
        Suu.append(M @ rng.standard_normal((3, 4)))
        v = rng.standard_normal(4)
        Suu.append(np.outer(v, v))
        Sux += [rng.standard_normal((4, 12)) for _ in range(2)]
    n_sing = len(Suu)
    for bad in (np.nan, np.inf, -np.inf):
        for _ in range(50):
            S = _well(rng, 1)[0]
            S[rng.integers(4), rng.integers(4)] = bad
            Suu.append(S)
            Sux.append(rng.standard_normal((4, 12)))
    Suu, Sux = np.array(Suu), np.array(Sux)
    L, ok = km.cofactor_solve(Suu, Sux)
    print(f"singular / non-finite: {ok.size} matrices, guard fires on {int((~ok).sum())}")
    assert not np.any(ok)
    assert not np.any(np.isfinite(L[0]))                   # Suu = 0 (the GPU test's case): all non-finite
    assert not np.any(np.isfinite(L[n_sing:][np.isnan(Suu[n_sing:]).any(axis=(1, 2))]))   # NaN in Suu: all NaN


def test_module_constants_match_the_kernel():
    """The model's threshold and the kernel's: 2^-45 in lqr_backward_dma.hip."""
    import os
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zopt_amd", "csrc", "lqr_backward_dma.hip")).read()
    assert "0x1p-45 * __builtin_fabs(det)" in src and km.TAU == math.ldexp(1.0, -45)
