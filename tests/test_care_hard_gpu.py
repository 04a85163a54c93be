"""GPU tests of infiniteHorizonLqr / infiniteHorizonIntegralLqr (care_sda_kernel, zopt_amd/csrc/care.hip) on hard spectra, at the
shape edges, at the integral design's size limit, on designs without a stabilising solution and at the iteration cap.

The reference of the hard-spectrum test is the Newton-Kleinman-refined CARE solution of tests/hp_reference.py (residual at least
1000 x below the bound, pinned by tests/test_hp_reference.py, which also shows that every generator has its hard feature).  The bound
per design is  max(1e-10, 100 x SciPy's own error against the refined solution) x max|ref|,  for P and separately for K: the floor
is the one tests/test_dare_hard_gpu.py uses, the factor 100 the margin over SciPy that infiniteHorizonLqr's docstring claims, and K
needs its own yardstick because under cheap control K = R^-1 B^T P amplifies P's error.  The bound is computed from the reference
side only.

Worst deviation per family as a fraction of its bound, MI355X (the worst kernel error in P / in K, then the fraction; before: the
doubling iteration alone, the kernel as it was; after: with the Newton-Kleinman polish; SciPy's own error alongside) -- the record
is profiles/care_hard_spectrum.txt:
    family                    SciPy P / K         before P / K         of bound   after P / K          of bound
    badly_scaled              2.9e-15 / 1.2e-14   5.7e-11 / 1.9e-10    1.9        3.3e-16 / 1.7e-15    1.7e-5
    cheap_control_1e-2        4.1e-14 / 1.4e-13   5.5e-12 / 5.4e-12    0.055      1.1e-15 / 5.1e-14    5.1e-4
    cheap_control_1e-4        3.6e-13 / 2.4e-12   7.7e-10 / 7.1e-10    7.7        1.2e-15 / 3.7e-13    3.7e-3
    cheap_control_1e-6        3.5e-11 / 1.8e-10   3.5e-08 / 3.5e-08    350        4.8e-16 / 4.5e-12    1.9e-3
    cheap_control_1e-8        2.7e-09 / 2.2e-08   3.2e-06 / 3.7e-06    32000      4.9e-16 / 4.2e-11    1.3e-4
    expensive_control         1.8e-08 / 2.3e-08   2.8e-14 / 2.6e-14    1.8e-5     2.2e-15 / 2.0e-15    5.1e-7
    integrator_chains         2.7e-14 / 1.8e-14   1.4e-15 / 1.7e-15    1.7e-5     4.6e-16 / 3.5e-16    4.6e-6
    light_oscillators         1.5e-12 / 1.6e-12   2.0e-13 / 2.2e-13    1.5e-3     5.8e-16 / 7.0e-16    6.2e-6
    marginally_stabilisable   5.4e-13 / 5.2e-13   8.0e-14 / 8.2e-14    8.2e-4     8.6e-16 / 6.9e-16    8.6e-6
    slow_unreachable          2.2e-12 / 1.3e-13   1.2e-12 / 2.8e-15    0.012      1.1e-16 / 4.4e-16    4.4e-6
    stiff                     1.1e-09 / 4.9e-10   2.3e-10 / 1.8e-10    0.14       9.0e-13 / 3.3e-12    1.2e-3
    weakly_detectable         3.2e-14 / 8.0e-15   4.4e-14 / 1.0e-14    4.4e-4     4.7e-16 / 7.2e-16    7.2e-6
Before the polish 19 of the 142 designs were over their bound (11 of the 71 cases below: cheap control at r <= 1e-4, and
badly_scaled at (12, 4) in the scaled metric); with it none is, and the worst stands at 0.37 % of its bound."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import zopt_oracle as zo
from tests import hp_reference as hp
from tests import problems

pytestmark = pytest.mark.gpu

SHAPES = [(12, 4), (8, 2), (16, 16), (5, 3), (3, 7), (16, 1)]
CASES = [(name, n, m) for name in sorted(problems.HARD_CARE) for n, m in SHAPES
         if not (name == "integrator_chains" and (n, m) == (16, 1))]       # the single-input 16-chain has no usable reference
WORST = {}      # family -> worst deviation / bound seen so far (printed as the tests run)


@pytest.fixture(scope="module")
def lqr():
    import torch
    assert torch.cuda.is_available()
    from zopt_amd import lqrUtils
    return lqrUtils


@functools.lru_cache(maxsize=None)
def _case(name, n, m):
    A, B, Q, R = problems.hard_care(name, n, m)
    refs = [hp.care_refined(A[i], B[i], Q[i], R[i]) for i in range(A.shape[0])]
    yard = [hp.care_scipy_error(A[i], B[i], Q[i], R[i], refs[i][0], refs[i][1]) for i in range(A.shape[0])]
    return (A, B, Q, R), refs, yard


def _rel(X, ref):
    return float(np.max(np.abs(X - ref)) / np.max(np.abs(ref)))


def _raw_care(A, B, Q, R, tol=1e-14, max_iter=60):
    """zm_care_f64 through the C ABI, without the wrapper's raising rule: (K, P, info) as NumPy arrays"""
    import torch
    from zopt_amd import _arrays as arr
    from zopt_amd import _lib
    batch, n, m = B.shape
    dA, dB, dQ, dR = (torch.as_tensor(np.ascontiguousarray(X), dtype=torch.float64, device="cuda") for X in (A, B, Q, R))
    dK = torch.empty((batch, m, n), dtype=torch.float64, device="cuda")
    dP = torch.empty((batch, n, n), dtype=torch.float64, device="cuda")
    info = torch.ones(batch, dtype=torch.int32, device="cuda")
    rc = _lib.lib().zm_care_f64(dA.data_ptr(), dB.data_ptr(), dQ.data_ptr(), dR.data_ptr(), dK.data_ptr(), dP.data_ptr(),
                                info.data_ptr(), batch, n, m, float(tol), int(max_iter), ctypes.c_void_p(arr.stream_ptr(dA)))
    _lib.check(rc, "zm_care_f64")
    return dK.cpu().numpy(), dP.cpu().numpy(), info.cpu().numpy()


@pytest.mark.parametrize("name,n,m", CASES)
def test_hard_spectrum_matches_refined_care(lqr, name, n, m):
    (A, B, Q, R), refs, yard = _case(name, n, m)
    K, P, its = lqr.infiniteHorizonLqr(A, B, Q, R, return_value=True)
    assert K.shape == (2, m, n) and P.shape == (2, n, n)
    fails = []
    for i, ((Kr, Pr, absc, _), (sP, sK)) in enumerate(zip(refs, yard)):
        Kr, Pr = Kr.astype(np.float64), Pr.astype(np.float64)
        bP, bK = hp.care_bounds(sP, sK)
        eP, eK = _rel(P[i], Pr), _rel(K[i], Kr)
        frac = max(eP / bP, eK / bK)
        if name == "badly_scaled":      # entry-wise in the scaled metric |dP_ij| / sqrt(P_ii P_jj): the small-coordinate entries count
            d = np.sqrt(np.diag(Pr))
            eS = float(np.max(np.abs(P[i] - Pr) / (d[:, None] * d[None, :])))
            frac = max(frac, eS / bP)
        else:
            eS = 0.0
        WORST[name] = max(WORST.get(name, 0.0), frac)
        print(f"{name} ({n},{m}) design {i}: doubling steps {int(its[i])}  kernel P {eP:.1e} K {eK:.1e}"
              + (f" scaled P {eS:.1e}" if name == "badly_scaled" else "")
              + f"  SciPy P {sP:.1e} K {sK:.1e}  bound P {bP:.1e} K {bK:.1e}  worst/bound {frac:.2g}  (family so far {WORST[name]:.2g})")
        assert its[i] > 0, (i, int(its[i]))
        if frac > 1.0:
            fails.append((i, int(its[i]), eP, bP, eK, bK, eS))
        assert np.all(np.linalg.eigvals(A[i] - B[i] @ K[i]).real < 0), i                     # the stabilising solution
        Kp = np.linalg.solve(R[i], B[i].T @ P[i])                                             # the gain of the returned value
        assert np.max(np.abs(K[i] - Kp)) <= 1e-10 * np.max(np.abs(K[i])), i
        assert np.array_equal(P[i], P[i].T)
    assert not fails, fails


def _benign(batch, n, m, seed):
    """random well-conditioned designs: A = G / sqrt(n) - 1.5 I (abscissa about -0.5: stable, so that a single input suffices),
    Q, R = SPD + I"""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((batch, n, n)) / np.sqrt(n) - 1.5 * np.eye(n)
    B = rng.standard_normal((batch, n, m))
    M = rng.standard_normal((batch, n, n))
    Q = M @ np.swapaxes(M, -1, -2) / n + np.eye(n)
    M = rng.standard_normal((batch, m, m))
    R = M @ np.swapaxes(M, -1, -2) / m + np.eye(m)
    return A, B, Q, R


@pytest.mark.parametrize("n,m", [(1, 16), (3, 7), (13, 16), (16, 1), (2, 5)])
def test_shape_edges_match_scipy(lqr, n, m):
    """m > n (B's tile is wider than the state, the R^-1 B^T solve is m x m with m > n), the single state, the single input and the
    ragged n = 13: random well-conditioned designs against SciPy at 1e-9, as tests/test_continuous_lqr_gpu.py does for m <= n"""
    batch = 4
    A, B, Q, R = _benign(batch, n, m, seed=31 * n + m)
    K, P, it = lqr.infiniteHorizonLqr(A, B, Q, R, return_value=True)
    assert K.shape == (batch, m, n) and P.shape == (batch, n, n)
    for b in range(batch):
        Kr, Pr = zo.infiniteHorizonLqr(A[b], B[b], Q[b], R[b])
        Kh, Ph, _, res = hp.care_refined(A[b], B[b], Q[b], R[b])
        assert res <= 1e-16 and max(hp.care_scipy_error(A[b], B[b], Q[b], R[b], Kh, Ph)) <= 1e-12      # well-conditioned indeed
        assert _rel(P[b], Pr) <= 1e-9 and _rel(K[b], Kr) <= 1e-9, (b, _rel(P[b], Pr), _rel(K[b], Kr))
        assert np.all(np.linalg.eigvals(A[b] - B[b] @ K[b]).real < 0)
    assert np.all(it > 0) and np.all(it <= 30)


@pytest.mark.parametrize("n,ni,m", [(12, 4, 4), (15, 1, 2)])
def test_integral_design_at_the_size_limit(lqr, n, ni, m):
    """n + ni = 16 fills the tile; the augmented system has ni eigenvalues at 0"""
    rng = np.random.default_rng(100 * n + ni)
    A, B, Q, R = (X[0] for X in _benign(1, n, m, seed=7 * n + ni))
    Ci = rng.standard_normal((ni, n))
    Qi = 0.5 * np.eye(ni)
    Ki, Kp = lqr.infiniteHorizonIntegralLqr(A, B, Q, R, Qi, Ci)
    Kir, Kpr = zo.infiniteHorizonIntegralLqr(A, B, Q, R, Qi, Ci)
    assert Ki.shape == (m, ni) and Kp.shape == (m, n)
    # the oracle's own error on the augmented design is far below the bound
    Aw = np.block([[np.zeros((ni, ni)), Ci], [np.zeros((n, ni)), A]])
    Bw = np.vstack([np.zeros((ni, m)), B])
    Qw = np.block([[Qi, np.zeros((ni, n))], [np.zeros((n, ni)), Q]])
    Kh, Ph, absc, res = hp.care_refined(Aw, Bw, Qw, R)
    assert res <= 1e-16 and absc < 0 and max(hp.care_scipy_error(Aw, Bw, Qw, R, Kh, Ph)) <= 1e-11
    Kw = np.concatenate([Ki, Kp], axis=1)
    assert _rel(Kw, np.concatenate([Kir, Kpr], axis=1)) <= 1e-9
    assert _rel(Kw, Kh.astype(np.float64)) <= 1e-10
    assert np.all(np.linalg.eigvals(Aw - Bw @ Kw).real < 0)


def test_integral_design_beyond_the_size_limit(lqr):
    A, B, Q, R = (X[0] for X in _benign(1, 13, 2, seed=3))
    with pytest.raises(ValueError):
        lqr.infiniteHorizonIntegralLqr(A, B, Q, R, np.eye(4), np.ones((4, 13)))      # n + ni = 17


@pytest.mark.parametrize("n,m", [(12, 4), (16, 16)])
def test_unreachable_unstable_mode_is_refused(lqr, n, m):
    """an unstable mode (+0.5) that B cannot reach: no stabilising solution (SciPy raises LinAlgError there)"""
    A, B, Q, R = problems.care_slow_unreachable(2, n, m, seed=8, lam=0.5)
    with pytest.raises(np.linalg.LinAlgError):
        lqr.infiniteHorizonLqr(A, B, Q, R)
    with pytest.raises(np.linalg.LinAlgError):
        lqr.infiniteHorizonLqr(A, B, Q, R, return_value=True)
    _, _, info = _raw_care(A, B, Q, R)
    assert np.all(info < 0)


def test_one_bad_design_in_a_batch(lqr):
    """One design of three has an unreachable unstable mode.  The wrapper raises for the whole batch, with or without return_value
    (its raising rule, pinned here as it is); the kernel itself flags only the bad design and solves the other two."""
    good = problems.care_slow_unreachable(3, 12, 4, seed=5)
    bad = problems.care_slow_unreachable(3, 12, 4, seed=5, lam=0.5)
    A, B, Q, R = (np.stack([g[0], b_[1], g[2]]) for g, b_ in zip(good, bad))
    for rv in (False, True):
        with pytest.raises(np.linalg.LinAlgError, match="1 of 3 designs"):
            lqr.infiniteHorizonLqr(A, B, Q, R, return_value=rv)
    K, P, info = _raw_care(A, B, Q, R)
    assert info[0] > 0 and info[1] < 0 and info[2] > 0
    for i in (0, 2):
        Kr, Pr, absc, _ = hp.care_refined(A[i], B[i], Q[i], R[i])
        assert _rel(P[i], Pr.astype(np.float64)) <= 1e-10 and _rel(K[i], Kr.astype(np.float64)) <= 1e-10
    Kg, Pg, ig = lqr.infiniteHorizonLqr(A[[0, 2]], B[[0, 2]], Q[[0, 2]], R[[0, 2]], return_value=True)       # and bit-equal to a clean batch
    assert np.array_equal(Kg, K[[0, 2]]) and np.array_equal(Pg, P[[0, 2]]) and np.array_equal(ig, info[[0, 2]])


def test_exact_iteration_cap(lqr):
    """convergence EXACTLY on the last allowed doubling step is convergence: a design that needs k steps is accepted with maxIter = k
    and refused with maxIter = k - 1"""
    A, B, Q, R = _benign(1, 12, 4, seed=11)
    K1, P1, k = lqr.infiniteHorizonLqr(A, B, Q, R, return_value=True)
    k = int(k[0])
    assert 3 <= k <= 30
    K2, P2, k2 = lqr.infiniteHorizonLqr(A, B, Q, R, maxIter=k, return_value=True)
    assert int(k2[0]) == k and np.array_equal(K1, K2) and np.array_equal(P1, P2)
    assert np.array_equal(lqr.infiniteHorizonLqr(A, B, Q, R, maxIter=k), K1)          # no LinAlgError
    with pytest.raises(np.linalg.LinAlgError):
        lqr.infiniteHorizonLqr(A, B, Q, R, maxIter=k - 1)
    _, _, info = _raw_care(A, B, Q, R, max_iter=k - 1)
    assert int(info[0]) == -1
