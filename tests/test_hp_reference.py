"""CPU tests of the high-precision references (tests/hp_reference.py) and of the hard-spectrum generators (tests/problems.py).

The GPU tests of the DARE, the CARE, the tiled finite-horizon sweep, the iLQR / affine / DDP backward sweeps and the PD projection judge
the kernels against these references; here the references are
pinned by a known answer, by their own residuals, by the fp64 oracle on easy inputs and by an independent 40-digit computation, and
every generator is shown to have the hard feature it claims, so that the GPU tests cannot drift into easy problems."""
import functools

import numpy as np
import pytest

from oracle import zopt_oracle as zo
from tests import hard_cases as hc
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


# ------------------------------------------------------------------------------------------------------------------------
# Backward sweeps and PD projection: the long-double references, HARD_SWEEP / HARD_DDP and the adversarial spectra, at the shapes and
# horizons of tests/test_sweeps_hard_gpu.py and tests/test_psd_hard_gpu.py
ORACLE_LIMIT = 1e-9        # a case whose fp64 oracle is further than this from the reference teaches nothing about a kernel
SWEEP_CASES = [(name, n, m) for name in sorted(problems.HARD_SWEEP) for n, m in problems.ILQR_ONE_TILE_SHAPES + problems.ILQR_TILED_SHAPES]
DDP_CASES = [(name, n, m) for name in sorted(problems.HARD_DDP) for n, m in problems.DDP_SHAPES]


@pytest.mark.parametrize("n,m,T", [(12, 4, 100), (5, 3, 40), (20, 6, 8)])
def test_sweep_references_match_their_oracles_on_the_plain_family(n, m, T):
    """ilqr_backward_ld, affine_lqr_ld and ddp_backward_hp (with eigh_ld inside) against zo.backwardPass_ilqr, zo.bilinearAffineLqr and
    zo.backwardPass_ddp on the plain family: 1e-13 in the tests' metric."""
    for case in (hc.ilqr_case("plain", n, m, T), hc.affine_case("plain", n, m, T), hc.ddp_case("plain", n, m, min(T, 6))):
        assert case["ref"]["L"].dtype == np.longdouble and case["ref"]["L"].shape[-2:] == (m, n)
        assert case["e_l"] <= 1e-13 and case["e_L"] <= 1e-13


def test_sweep_references_keep_the_reference_formulas():
    """One step by hand: v_x' = Q_x - L^T (Q_uu l), v_xx' = Q_xx - (L^T Q_uu) L with a NONSYMMETRIC v_xx, c_xx, c_uu used as they
    stand (no Joseph form, no symmetrisation), against zo.riccatiStep_ilqr."""
    dyn, cost, Vf = problems.hard_sweep("nonsymmetric", 5, 3, 1)
    ref = hp.ilqr_backward_ld(dyn, cost, Vf)
    for b in range(2):
        V, pol = zo.riccatiStep_ilqr(tuple(x[b, 0] for x in dyn), tuple(x[b, 0] for x in cost), tuple(x[b] for x in Vf))
        assert np.max(np.abs(V.v_xx - V.v_xx.T)) > 0.1                                         # really nonsymmetric
        assert np.max(np.abs(ref["v_xx"][b, 0] - V.v_xx)) <= 1e-13 * np.max(np.abs(V.v_xx))
        assert np.max(np.abs(ref["v_x"][b, 0] - V.v_x)) <= 1e-13 * np.max(np.abs(V.v_x))
        assert np.max(np.abs(ref["L"][b, 0] - pol.L)) <= 1e-13 * np.max(np.abs(pol.L))


@pytest.mark.parametrize("k", [1, 2, 7, 16, 33, 64])
def test_eigh_ld_recovers_a_planted_spectrum(k):
    """eigh_ld on U diag(w) U^T (long double, unrounded): the planted eigenvalues to 1e-17 of the largest, orthonormal vectors, and
    the decomposition reassembles the matrix; psd_project_ld of the fp64-rounded matrix is the planted projection to fp64 rounding."""
    rng = np.random.default_rng(k)
    w = rng.standard_normal(k) * 10.0 ** rng.uniform(-3, 3, k)
    a64, P, U = hp.psd_from_spectrum_ld(k, w, seed=k + 1)
    assert a64.dtype == np.float64 and P.dtype == np.longdouble and np.array_equal(a64, a64.T)
    assert np.max(np.abs(U.T @ U - np.eye(k))) <= 1e-17
    a = (U * w.astype(np.longdouble)) @ U.T
    wl, V = hp.eigh_ld(np.stack([a, a.T]))
    scale = np.max(np.abs(w))
    assert np.max(np.abs(wl[0] - np.sort(w))) <= 1e-17 * scale and np.array_equal(wl[0], wl[1])
    assert np.max(np.abs(V[0].T @ V[0] - np.eye(k))) <= 1e-17
    assert np.max(np.abs((V[0] * wl[0]) @ V[0].T - (a + a.T) / 2)) <= 1e-17 * scale
    assert np.max(np.abs(hp.psd_project_ld(a64) - P)) <= 1e-15 * max(scale, 1e-3)
    assert np.max(np.abs(hp.psd_project_ld(a64).astype(np.float64) - zo.ensurePositiveDefinite(a64))) <= 1e-12 * max(scale, 1e-3)


def test_eigh_ld_against_mpmath():
    """eigh_ld against mpmath.eigsy at 40 digits on three 16 x 16 matrices: dense random, a wide planted spectrum, a repeated
    eigenvalue."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 40
    rng = np.random.default_rng(3)
    M = rng.standard_normal((16, 16))
    wide = hp.psd_from_spectrum_ld(16, 10.0 ** rng.uniform(-10, 2, 16) * rng.choice([-1, 1], 16), 4)[0]
    rep = hp.psd_from_spectrum_ld(16, np.repeat([2.0, -1.0, 1e-3, 0.0], 4), 5)[0]
    for a in (M + M.T, wide, rep):
        w_mp = mp.eigsy(mp.matrix([[mp.mpf(float(x)) for x in row] for row in a]), eigvals_only=True)
        w_mp = np.sort(np.array([np.longdouble(mp.nstr(x, 30)) for x in w_mp]))
        w, _ = hp.eigh_ld(a)
        assert np.max(np.abs(w - w_mp)) <= 1e-17 * np.max(np.abs(w_mp))


def _max_multiplier(M):
    """the largest multiplier of Gaussian elimination WITHOUT row exchanges on M (fp64)"""
    M = np.array(M, dtype=np.float64)
    worst = 0.0
    for j in range(M.shape[0] - 1):
        f = M[j + 1:, j] / M[j, j]
        worst = max(worst, float(np.max(np.abs(f))))
        M[j + 1:] -= f[:, None] * M[j]
    return worst


@pytest.mark.parametrize("name,n,m", SWEEP_CASES)
def test_sweep_family_has_its_feature_and_is_well_posed(name, n, m):
    """Every HARD_SWEEP generator has the feature it names at every shape the GPU tests run, and on every such case (iLQR; affine where
    the shape is an affine one; shared Hessians at (12, 4)) the fp64 oracle is within 1e-9 of the long-double reference."""
    T = problems.sweep_horizon(name, n, m)
    case, plain = hc.ilqr_case(name, n, m, T), hc.ilqr_case("plain", n, m, T)
    (f, f_x, f_u), (c, c_x, c_u, c_xx, c_ux, c_uu), (v, v_x, v_xx) = case["args"]
    ref = case["ref"]
    print(f"{name} ({n},{m},{T}): oracle l {case['e_l']:.1e} L {case['e_L']:.1e}  cond(Q_uu) <= {ref['cond_quu'].max():.1e}")
    assert f_u.shape == (2, T, n, m) and not np.array_equal(f_x[0], f_x[1])
    assert max(case["e_l"], case["e_L"]) <= ORACLE_LIMIT and max(plain["e_l"], plain["e_L"]) <= 1e-13
    if (n, m) in problems.AFFINE_SHAPES:
        a = hc.affine_case(name, n, m, T)
        assert max(a["e_l"], a["e_L"]) <= ORACLE_LIMIT and np.all(a["args"][2] != 0)
    if (n, m) == (12, 4):
        s = hc.ilqr_case(name, n, m, T, shared=True)
        assert max(s["e_l"], s["e_L"]) <= ORACLE_LIMIT and np.array_equal(s["args"][1][3][1, 3], s["args"][1][3][0, 0])
    Lf = ref["L"].astype(np.float64)
    V_next = np.concatenate([ref["v_xx"][:, 1:], np.asarray(v_xx, dtype=np.longdouble)[:, None]], axis=1).astype(np.float64)
    fvf = np.swapaxes(f_u, -1, -2) @ V_next @ f_u                              # f_u^T v_xx f_u of every step
    if name == "unstable":
        assert np.all(np.abs(np.max(np.abs(np.linalg.eigvals(f_x)), axis=-1) - 1.3) <= 1e-9)
        if n > m and T >= 20:      # the value grows beyond the plain family's where one step cannot reach every direction
            assert np.max(np.abs(ref["v_xx"])) >= 2 * np.max(np.abs(plain["ref"]["v_xx"]))
    elif name == "cheap_control":
        assert np.max(np.abs(c_uu)) <= (1e-7 if m <= n else 1e-3)
        assert np.median(np.max(np.abs(fvf), axis=(-1, -2)) / np.max(np.abs(c_uu), axis=(-1, -2))) >= (1e6 if m <= n else 1e2)
    elif name == "expensive_control":
        assert np.min(np.abs(np.diagonal(c_uu, axis1=-1, axis2=-2))) >= 1e8 and np.max(np.abs(Lf)) <= 1e-6
    elif name == "illcond_quu":
        assert np.all(np.linalg.matrix_rank(f_u) == 1)
        if m > 1:
            assert 1e5 <= ref["cond_quu"].max() <= 1e8 and ref["cond_quu"].min() >= 1e3
    elif name == "pivoting":
        Quu = c_uu + fvf
        assert np.max(np.abs(c_uu - np.swapaxes(c_uu, -1, -2))) >= (1e3 if m > 1 else 0.0)
        if m > 1:      # every step's elimination without row exchanges exceeds the kernels' multiplier limit of 4 by far
            assert min(_max_multiplier(Quu[b, k]) for b in range(2) for k in range(T)) >= 50.0
            assert ref["cond_quu"].max() <= 10.0                                             # ... while Q_uu is well conditioned
    elif name == "badly_scaled":
        d = problems.sweep_scaling(n)
        assert np.max(np.abs(Lf * d - plain["ref"]["L"].astype(np.float64))) <= 1e-9 * np.max(np.abs(Lf * d))      # the plain policy, rescaled
        if n > 1:
            col = np.max(np.abs(Lf), axis=(0, 1, 2))
            assert d.max() / d.min() == pytest.approx(1e4) and col.max() / col.min() >= 1e3
    elif name == "nonsymmetric":
        for X in (c_xx, v_xx) + ((c_uu,) if m > 1 else ()):
            if X.shape[-1] > 1:
                assert np.max(np.abs(X - np.swapaxes(X, -1, -2))) >= 0.5
    elif name == "zero_gradient":
        assert not c_x.any() and not c_u.any() and not v_x.any() and not ref["l"].any() and np.max(np.abs(Lf)) > 0.01


def test_ring_horizon_cases_are_well_posed():
    for n in (12, 8):
        for T in problems.RING_HORIZONS:
            case = hc.ilqr_case("unstable", n, 4, T)
            assert max(case["e_l"], case["e_L"]) <= ORACLE_LIMIT


@pytest.mark.parametrize("name,n,m", DDP_CASES + [("packed_pairs", 12, 4)])
def test_ddp_family_has_its_feature_and_is_well_posed(name, n, m):
    """Every HARD_DDP generator has the feature it names -- the planted spectrum is what the terminal step projects, the zero rows are
    exactly zero -- and the fp64 oracle (eigh) is within 1e-9 of the long-double sweep on every case the GPU tests run."""
    T = problems.DDP_SHAPES[(n, m)]
    case = hc.ddp_case(name, n, m, T)
    (f, f_x, f_u, f_xx, f_ux, f_uu), cost, (v, v_x, v_xx) = case["args"]
    ref, planted = case["ref"], case["planted"]
    k, eps = n + m, problems.DDP_EPS
    print(f"{name} ({n},{m},{T}): oracle l {case['e_l']:.1e} L {case['e_L']:.1e}  sensitivity l {case['s_l']:.1e} L {case['s_L']:.1e}  "
          f"smallest |eig(vf_zz - eps I)| / |.|_F {np.min(np.abs(ref['spectrum'])):.1e}")
    assert max(case["e_l"], case["e_L"]) <= ORACLE_LIMIT
    assert np.array_equal(f_xx, np.swapaxes(f_xx, -1, -2)) and np.array_equal(f_uu, np.swapaxes(f_uu, -1, -2))
    term = np.einsum("bi,bijk->bjk", v_x, np.block([[f_xx[:, -1], np.swapaxes(f_ux[:, -1], -1, -2)], [f_ux[:, -1], f_uu[:, -1]]]))
    w_term = hp.eigh_ld(term)[0].astype(np.float64)                             # what the terminal step projects
    fro = np.sqrt(np.sum((w_term - eps) ** 2, axis=-1, keepdims=True))
    assert np.max(np.abs(ref["spectrum"][:, -1] - (w_term - eps) / np.where(fro > 0, fro, 1))) <= 1e-12
    if planted is not None:
        assert np.max(np.abs(w_term - np.sort(planted, axis=-1))) <= 1e-15 * max(1.0, np.max(np.abs(planted)))
    if name == "strongly_indefinite":
        assert np.all(np.abs(planted) >= 10) and np.all(np.abs(planted) <= 100) and np.any(planted < 0) and np.any(planted > 0)
        assert np.all(np.abs(np.max(np.abs(np.linalg.eigvals(f_x)), axis=-1) - 1.1) <= 1e-9)
    elif name == "hugging_eps":
        gap = np.abs(planted - eps)
        assert gap.min() >= 1e-9 * (1 - 1e-6) and gap.max() <= 1e-3 and np.any(planted < eps) and np.any(planted > eps)
    elif name == "half_at_eps":      # eigenvalues of vf_zz - eps I ~1e-8 of its norm next to O(1) ones: beyond a shortened sign iteration
        gap = np.abs(planted[:, k // 2:] - eps)
        assert gap.min() >= 1e-8 * (1 - 1e-6) and gap.max() <= 3e-8 and np.max(np.abs(planted[:, :k // 2])) >= 0.3
        small = np.sort(np.abs(ref["spectrum"][:, -1]), axis=-1)[:, :k - k // 2]
        assert small.min() >= 1e-9 and small.max() <= 2e-7
    elif name == "wide_decades":
        mag = np.abs(planted)
        assert mag.min() >= 1e-10 and mag.max() <= 1e2 and mag.max() / mag.min() >= (1e6 if k > 4 else 1e2) and np.any(planted < 0)
    elif name == "rank_one":
        assert np.all(np.count_nonzero(planted, axis=-1) == 1)
    elif name == "all_pd":
        assert planted.min() > eps and np.array_equal(np.sort(v_x, axis=-1)[:, -1], np.ones(2))
    elif name.startswith("control_affine") or name == "packed_pairs":
        r = min(9 if name == "packed_pairs" else int(name.split("_")[-1]), n)
        assert not f_ux.any() and not f_uu.any() and not f_xx[..., r:, :].any() and not f_xx[..., :, r:].any()
        assert np.all(np.any(f_xx[..., :r, :r] != 0, axis=(-1, -2)))
        if name == "packed_pairs":
            keep = np.zeros((n, n), dtype=bool)
            for a, b in problems.QUAD_HESSIAN_PAIRS:
                keep[a, b] = keep[b, a] = True
            assert len(set(problems.QUAD_HESSIAN_PAIRS)) == 28 and not f_xx[..., ~keep].any() and np.all(f_xx[0, 0, 0][keep] != 0)
            assert np.array_equal(cost[3][1, 2], cost[3][0, 0])                     # shared cost Hessians
    elif name == "vanishing":
        assert not v_x.any() and not cost[1].any() and not term.any()              # vf_zz = 0 exactly on the last step
        vf = np.abs(ref["v_x"].astype(np.float64))
        assert 0 < vf.max() <= 1e-10                                                # ... and ~1e-12 on the steps before
        assert np.all(np.abs(ref["spectrum"][:, :-1] + 1 / np.sqrt(k)) <= 1e-6)    # a - eps I is -eps I to many digits


@pytest.mark.parametrize("kind", range(len(problems.ADVERSARIAL_SPECTRA)))
def test_adversarial_spectra_have_their_feature(kind):
    eps = 1e-3
    for k in problems.PSD_SIZES:
        w = problems.adversarial_spectrum(kind, k, np.random.default_rng(kind + k))
        name = problems.ADVERSARIAL_SPECTRA[kind]
        assert w.shape == (k,) and np.array_equal(w, problems.adversarial_spectrum(name, k, np.random.default_rng(kind + k)))
        if name == "half_at_eps":
            assert np.all(np.abs(w[k // 2:] - eps) <= 1e-8)
        elif name == "sixteen_decades":
            assert np.abs(w).max() / np.abs(w).min() >= (1e6 if k > 2 else 1.0) and np.abs(w).min() >= 1e-14
        elif name == "rank_one":
            assert np.count_nonzero(w) == 1
        elif name == "dominant_pair":
            assert np.all(w[:2] == 1e3) and np.all(np.abs(w[2:]) <= 10)
        elif name == "hugging_eps":
            assert np.all(np.abs(w - eps) <= 1e-2) and np.all(np.abs(w - eps) >= 1e-16)
        elif name == "all_pd":
            assert w.min() >= 1e-2 > eps
