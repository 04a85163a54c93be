"""CPU tests of the high-precision references (tests/hp_reference.py) and of the hard-spectrum generators (tests/problems.py).

The GPU tests of the DARE and of the tiled finite-horizon sweep judge the kernels against these references; here the references are
pinned by a known answer, by their own residuals, by the fp64 oracle on easy inputs and by an independent 40-digit computation, and
every generator is shown to have the hard feature it claims, so that the GPU tests cannot drift into easy problems."""
import functools

import numpy as np
import pytest

from oracle import zopt_oracle as zo
from tests import hp_reference as hp
from tests import problems

# the shapes of tests/test_dare_hard_gpu.py: (12, 4), (8, 2) take the tile-16 kernel, the others the tiled one
DARE_SHAPES = [(12, 4), (8, 2), (16, 4), (12, 6), (33, 7), (64, 16)]


@functools.lru_cache(maxsize=None)
def _refined(name, n, m):
    A, B, Q, R = problems.hard_dare(name, n, m)
    return (A, B, Q, R), [hp.dare_refined(A[i], B[i], Q[i], R[i]) for i in range(A.shape[0])]


def _pbh_margin(A, X, stack):
    """min over the eigenvalues |lam| >= 1 of A of the smallest singular value of [A - lam I, X] (stack='h': stabilisability)
    or [A - lam I; X] (stack='v': detectability), relative to the largest; 1.0 when A has no such eigenvalue."""
    n = A.shape[0]
    margin = 1.0
    for lam in np.linalg.eigvals(A):
        if abs(lam) < 1.0:
            continue
        M = np.hstack([A - lam * np.eye(n), X]) if stack == "h" else np.vstack([A - lam * np.eye(n), X])
        s = np.linalg.svd(M, compute_uv=False)
        margin = min(margin, s[n - 1] / s[0])
    return margin


def test_golden_ratio_known_answer():
    """A = B = Q = R = I2: P = phi I (phi = (1 + sqrt 5) / 2), L = phi / (phi + 1) I."""
    I = np.eye(2)
    L, P, rho, res = hp.dare_refined(I, I, I, I)
    phi = (1 + np.sqrt(np.longdouble(5))) / 2
    assert np.max(np.abs(P - phi * np.eye(2, dtype=np.longdouble))) <= 1e-15
    assert np.max(np.abs(L - phi / (phi + 1) * np.eye(2, dtype=np.longdouble))) <= 1e-15
    assert res <= 1e-18 and abs(rho - 1 / (phi + 1)) <= 1e-12


def test_solve_ld_pivots_and_beats_fp64():
    """the long-double solve needs its row exchanges (zero leading pivot) and is more accurate than fp64 on a Hilbert matrix"""
    M = np.array([[0.0, 1.0, 2.0], [1.0, 0.0, 3.0], [4.0, -3.0, 8.0]])
    Y = np.arange(6.0).reshape(3, 2)
    assert np.max(np.abs(hp.solve_ld(M, Y) - np.linalg.solve(M, Y))) <= 1e-14
    k = 8
    H = 1.0 / (np.arange(k)[:, None] + np.arange(k)[None, :] + 1.0)
    x = np.ones((k, 1))
    y = (H.astype(np.longdouble) @ x.astype(np.longdouble))
    e_ld = np.max(np.abs(hp.solve_ld(np.stack([H, H]), np.stack([y, y])) - 1.0))
    e_64 = np.max(np.abs(np.linalg.solve(H, y.astype(np.float64)) - 1.0))
    assert e_ld * 100 <= e_64


@pytest.mark.parametrize("n,m,T", [(6, 3, 20), (24, 8, 7), (5, 9, 4)])
def test_finite_horizon_ld_matches_oracle(n, m, T):
    """on well-conditioned time-varying inputs the long-double recursion and the fp64 oracle agree to fp64 rounding"""
    A, B, Q, R = problems.random_time_varying(3, T, n, m, seed=40 + n)
    L_ld = hp.finite_horizon_ld(A, B, Q, R, T)
    L_64 = zo.discreteFiniteHorizonLqr(A, B, Q, R, T)
    assert L_ld.dtype == np.longdouble and L_ld.shape == (3, T, m, n)
    assert np.max(np.abs(L_ld - L_64)) <= 1e-12 * np.max(np.abs(L_64))


def test_finite_horizon_ld_reaches_dare_gain():
    """an LTI problem over a long horizon: L_0 of the long-double recursion is the refined DARE gain"""
    A1, B1, Q1, R1 = problems.random_lti_systems(2, 7, 3, seed=9, rho=1.1)
    L = hp.finite_horizon_ld(*problems.tile_over_horizon(A1, B1, Q1, R1, 300), 300)
    for i in range(2):
        Linf, _, rho, _ = hp.dare_refined(A1[i], B1[i], Q1[i], R1[i])
        assert rho < 0.95
        assert np.max(np.abs(L[i, 0] - Linf)) <= 1e-17 * np.max(np.abs(Linf))


@pytest.mark.parametrize("name", sorted(problems.HARD_DARE))
@pytest.mark.parametrize("n,m", DARE_SHAPES)
def test_refined_residual_on_hard_problems(name, n, m):
    """Newton refinement brings every hard design's DARE residual (evaluated in long double) to <= 1e-16 relative"""
    _, refs = _refined(name, n, m)
    for L, P, rho, res in refs:
        assert res <= 1e-16, (res, rho)
        assert np.all(np.isfinite(L.astype(np.float64))) and rho < 1.0


@pytest.mark.parametrize("name", sorted(problems.HARD_DARE))
@pytest.mark.parametrize("n,m", DARE_SHAPES)
def test_generator_has_its_hard_feature(name, n, m):
    (A, B, Q, R), refs = _refined(name, n, m)
    assert A.shape == (2, n, n) and B.shape == (2, n, m) and Q.shape == (2, n, n) and R.shape == (2, m, m)
    assert not np.array_equal(A[0], A[1])
    for i, (L, P, rho, _) in enumerate(refs):
        a, b, q, r = A[i], B[i], Q[i], R[i]
        rho_a = np.max(np.abs(np.linalg.eigvals(a)))
        if name == "badly_scaled":      # the PBH margins are not invariant under the diagonal similarity: judge the unscaled system
            dd = np.logspace(-2, 2, n)
            stab = _pbh_margin(a / dd[:, None] * dd[None, :], b / dd[:, None], "h")
            det = _pbh_margin(a / dd[:, None] * dd[None, :], q * dd[:, None] * dd[None, :], "v")
        else:
            stab, det = _pbh_margin(a, b, "h"), _pbh_margin(a, q, "v")
        assert stab > 1e-6 and det > 1e-9 and rho < 1.0, (stab, det, rho)    # stabilisable, detectable: a stabilising P exists
        assert np.all(np.linalg.eigvalsh(r) > 0) and np.all(np.linalg.eigvalsh((q + q.T) / 2) >= -1e-12)
        Lf, Pf = L.astype(np.float64), P.astype(np.float64)
        if name in ("slow_unreachable", "slow_coupled"):
            assert np.all(b[n - 1] == 0) and np.all(a[n - 1, :n - 1] == 0) and a[n - 1, n - 1] == 0.999
            assert abs(rho - 0.999) <= 1e-12                                      # the unreachable slow mode IS the closed loop's
            assert np.argmax(np.abs(Pf)) == (n - 1) * n + (n - 1)                 # its value entry dominates P
            assert abs(Pf[n - 1, n - 1] - 1 / (1 - 0.999 ** 2)) <= 0.01 * Pf[n - 1, n - 1]
            if name == "slow_unreachable":                                        # ... and the gain does not see it
                assert np.all(a[:n - 1, n - 1] == 0) and np.max(np.abs(Lf[:, n - 1])) <= 1e-15 * np.max(np.abs(Lf))
            else:                                                                 # coupled: the gain does
                assert np.max(np.abs(Lf[:, n - 1])) >= 1e-5 * np.max(np.abs(Lf))
        elif name == "weakly_detectable":
            assert abs(rho_a - 1.001) <= 1e-12 and q[n - 1, n - 1] == 1e-6
            assert 0.995 <= rho < 1.0
            assert det <= 1e-5                                                    # only just detectable
        elif name == "marginally_stabilisable":
            assert abs(rho_a - 1.02) <= 1e-12 and np.count_nonzero(b[n - 1]) == 1
            assert 1e-6 <= stab <= 2e-2                                           # only just stabilisable (through B = 1e-2)
            assert np.argmax(np.abs(Pf)) == (n - 1) * n + (n - 1) and Pf[n - 1, n - 1] >= 1e3
        elif name == "cheap_control":
            assert abs(rho_a - 1.2) <= 1e-12 and np.array_equal(r, 1e-8 * np.eye(m))
        elif name == "expensive_control":
            assert abs(rho_a - 1.05) <= 1e-12 and np.array_equal(r, 1e8 * np.eye(m))
            assert rho >= 1 / 1.05 - 1e-3                                         # unstable modes only mirrored, not damped further
            assert np.max(np.abs(Lf)) <= 1.0
        elif name == "badly_scaled":
            d = np.abs(np.diag(Pf))
            assert abs(rho_a - 1.05) <= 1e-12 and d.max() / d.min() >= 1e6        # value entries over many decades


def _mp_newton_dare(A, B, Q, R, P0, dps=40, steps=6):
    """Newton on the DARE in mpmath at `dps` digits, the Stein correction E - Acl^T E Acl = Res solved by its Kronecker form"""
    import mpmath as mp
    mp.mp.dps = dps
    M = lambda X: mp.matrix([[mp.mpf(float(x)) for x in row] for row in np.asarray(X, dtype=np.float64)])   # noqa: E731
    Am, Bm, Qm, Rm, Pm = M(A), M(B), M(Q), M(R), M(P0)
    n = A.shape[0]
    for _ in range(steps):
        BtP = Bm.T * Pm
        Lm = mp.inverse(Rm + BtP * Bm) * (BtP * Am)
        Acl = Am - Bm * Lm
        Res = Qm + Lm.T * Rm * Lm + Acl.T * Pm * Acl - Pm
        K = mp.eye(n * n)       # vec (column-major) of E - Acl^T E Acl = (I - Acl^T (x) Acl^T) vec E
        for i in range(n):
            for j in range(n):
                for k in range(n):
                    for l in range(n):
                        K[j * n + i, l * n + k] -= Acl[k, i] * Acl[l, j]
        e = mp.lu_solve(K, mp.matrix([Res[i, j] for j in range(n) for i in range(n)]))
        for j in range(n):
            for i in range(n):
                Pm[i, j] += e[j * n + i]
    return np.array([[np.longdouble(mp.nstr(Pm[i, j], 30)) for j in range(n)] for i in range(n)])


def test_refined_dare_against_40_digit_newton():
    """independent check of dare_refined on the slow-unreachable-mode design (n = 4): 40-digit Newton agrees to 1e-16 relative,
    where fp64 SciPy alone is off by ~1e-14"""
    import scipy.linalg as spl
    A, B, Q, R = (x[0] for x in problems.slow_unreachable_mode(1, 4, 1, seed=5))
    _, P, rho, _ = hp.dare_refined(A, B, Q, R)
    P_mp = _mp_newton_dare(A, B, Q, R, spl.solve_discrete_are(A, B, Q, R))
    scale = np.max(np.abs(P_mp))
    assert abs(rho - 0.999) <= 1e-12
    assert np.max(np.abs(P - P_mp)) <= 1e-16 * scale


# ------------------------------------------------------------------------------------------------------------------------
# Continuous time: care_refined and the HARD_CARE generators, at the shapes of tests/test_care_hard_gpu.py
CARE_SHAPES = [(12, 4), (8, 2), (16, 16), (5, 3), (3, 7), (16, 1)]
CARE_CASES = [(name, n, m) for name in sorted(problems.HARD_CARE) for n, m in CARE_SHAPES
              if not (name == "integrator_chains" and (n, m) == (16, 1))]


@functools.lru_cache(maxsize=None)
def _care_refined(name, n, m):
    A, B, Q, R = problems.hard_care(name, n, m)
    return (A, B, Q, R), [hp.care_refined(A[i], B[i], Q[i], R[i]) for i in range(A.shape[0])]


def test_care_known_answer():
    """A = B = Q = R = I2: P = K = (1 + sqrt 2) I, closed loop -sqrt 2 I."""
    I = np.eye(2)
    K, P, absc, res = hp.care_refined(I, I, I, I)
    ref = (1 + np.sqrt(np.longdouble(2))) * np.eye(2, dtype=np.longdouble)
    assert P.dtype == np.longdouble and np.max(np.abs(P - ref)) <= 1e-18 and np.max(np.abs(K - ref)) <= 1e-18
    assert res <= 1e-18 and abs(absc + np.sqrt(2)) <= 1e-12


def test_care_residual_goes_through_the_gain():
    """cheap control: the residual formed as P G P cancels at the 1e-8 level in fp64, the one formed through K does not"""
    A, B, Q, R = (x[0] for x in problems.hard_care("cheap_control_1e-8", 8, 2))
    _, P, _, res = hp.care_refined(A, B, Q, R)
    Pf = P.astype(np.float64)
    G = B @ np.linalg.solve(R, B.T)
    naive = np.max(np.abs(A.T @ Pf + Pf @ A - Pf @ G @ Pf + Q)) / np.max(np.abs(Pf))
    assert res <= 1e-13 and naive >= 1e-11


@pytest.mark.parametrize("name,n,m", CARE_CASES)
def test_care_refined_residual_on_hard_problems(name, n, m):
    """Newton-Kleinman refinement brings every design's CARE residual (long double) at least 1000 x below the bound the GPU test
    applies to that design, max(1e-10, 100 x SciPy's own error); SciPy's error is recorded per design (run with -s)."""
    (A, B, Q, R), refs = _care_refined(name, n, m)
    for i, (K, P, absc, res) in enumerate(refs):
        eP, eK = hp.care_scipy_error(A[i], B[i], Q[i], R[i], K, P)
        bP, bK = hp.care_bounds(eP, eK)
        print(f"{name} ({n},{m}) design {i}: residual {float(res):.1e}  SciPy's error P {eP:.1e} K {eK:.1e}  bound P {bP:.1e} K {bK:.1e}")
        assert bP == max(1e-10, 100 * eP) and bK == max(1e-10, 100 * eK)
        assert res * 1000 <= min(bP, bK), (i, float(res))
        assert res <= (1e-13 if name.startswith("cheap_control") else 1e-16), (i, float(res))
        assert np.all(np.isfinite(K.astype(np.float64))) and absc < 0.0
        assert np.max(np.abs(P - np.swapaxes(P, -1, -2))) <= 1e-17 * np.max(np.abs(P))


@pytest.mark.parametrize("name,n,m", CARE_CASES)
def test_care_generator_has_its_hard_feature(name, n, m):
    (A, B, Q, R), refs = _care_refined(name, n, m)
    assert A.shape == (2, n, n) and B.shape == (2, n, m) and Q.shape == (2, n, n) and R.shape == (2, m, m)
    assert not np.array_equal(A[0], A[1]) or not np.array_equal(B[0], B[1])
    for i, (K, P, absc, _) in enumerate(refs):
        a, b, q, r = A[i], B[i], Q[i], R[i]
        Kf, Pf = K.astype(np.float64), P.astype(np.float64)
        assert np.all(np.linalg.eigvalsh(r) > 0) and np.all(np.linalg.eigvalsh((q + q.T) / 2) >= -1e-12 * np.max(np.abs(q)))
        assert np.array_equal(q, q.T) and np.array_equal(r, r.T)
        ham = np.block([[a, -b @ np.linalg.solve(r, b.T)], [-q, -a.T]])
        if name == "badly_scaled":     # judge the Hamiltonian in the balanced coordinates: its eigenvalues are the same
            dd = np.concatenate([np.logspace(-2, 2, n), 1 / np.logspace(-2, 2, n)])
            ham = ham / dd[:, None] * dd[None, :]
        assert np.min(np.abs(np.linalg.eigvals(ham).real)) >= 5e-4                # nothing on the imaginary axis
        assert absc < 0 and np.all(np.linalg.eigvalsh((Pf + Pf.T) / 2) >= -1e-12 * np.max(np.abs(Pf)))
        open_loop = np.max(np.linalg.eigvals(a).real)
        top = np.argmax(np.abs(Pf))
        if name == "slow_unreachable":
            assert np.all(b[n - 1] == 0) and np.all(a[n - 1, :n - 1] == 0) and a[n - 1, n - 1] == -1e-3
            assert abs(absc + 1e-3) <= 1e-12                                       # the unreachable slow mode IS the closed loop's
            assert top == (n - 1) * n + (n - 1) and abs(Pf[n - 1, n - 1] - 500.0) <= 5.0
        elif name == "weakly_detectable":
            assert a[n - 1, n - 1] == 1e-3 and abs(open_loop - 1e-3) <= 1e-12 and q[n - 1, n - 1] == 1e-6
            assert -5e-3 <= absc < 0                                               # only just mirrored
        elif name == "marginally_stabilisable":
            assert abs(open_loop - 0.02) <= 1e-12 and np.count_nonzero(b[n - 1]) == 1 and b[n - 1, 0] == 1e-2
            assert top == (n - 1) * n + (n - 1) and Pf[n - 1, n - 1] >= 500.0 and -0.03 <= absc
            assert np.argmax(np.max(np.abs(Kf), axis=0)) == n - 1                  # the gain's column n-1 is the large one
        elif name.startswith("cheap_control"):
            rr_ = float(name.split("_")[-1])
            assert np.array_equal(r, rr_ * np.eye(m)) and abs(open_loop - 0.2) <= 1e-12
            assert np.max(np.abs(Kf)) >= 0.5 / np.sqrt(rr_)                        # K = O(1 / sqrt r)
            assert np.max(np.abs(b.T @ Pf)) <= 20 * np.sqrt(rr_) * max(1.0, np.max(np.abs(Pf)))       # B^T P = O(sqrt r)
        elif name == "expensive_control":
            assert np.array_equal(r, 1e8 * np.eye(m)) and abs(open_loop - 0.05) <= 1e-12
            # unstable modes only mirrored, not damped further
            assert absc >= -0.051 and np.max(np.abs(Kf)) <= 1e-1 and np.max(np.abs(Pf)) >= 1e5
        elif name == "badly_scaled":
            d = np.abs(np.diag(Pf))
            assert abs(open_loop - 0.05) <= 1e-9 and d.max() / d.min() >= 1e6      # value entries over many decades
        elif name == "stiff":
            ev = np.abs(np.linalg.eigvals(a))
            assert np.max(np.abs(a - a.T)) <= 2e-2 and ev.max() / ev.min() >= (1e5 if n > 3 else 1e4)
        elif name == "integrator_chains":
            assert np.all(np.linalg.matrix_power(a, 4) == 0) and np.any(np.linalg.matrix_power(a, min(3, n - 1)) != 0)
            assert np.count_nonzero(b) == -(-n // 4)                               # one input per chain
        elif name == "light_oscillators":
            assert abs(open_loop + 1e-4) <= 1e-12 and np.max(np.abs(q)) <= 1e-3
            assert absc >= -0.05 and np.max(np.abs(Pf)) <= 0.1


def test_integrator_chains_refuse_more_chains_than_inputs():
    with pytest.raises(ValueError):
        problems.hard_care("integrator_chains", 16, 1)
    with pytest.raises(ValueError):
        problems.hard_care("integrator_chains", 9, 2)
