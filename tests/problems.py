"""Seeded synthetic problem generators shared by tests, bench.py and the golden script.

SURVEY.md section 8(d) "Synthetic inputs per config".  NumPy only (no reference, no oracle).
"""
from __future__ import annotations

import numpy as np


def random_lti_systems(batch: int, n: int, m: int, seed: int = 0, rho: float = 0.95, dtype=np.float64):
    """Per system: G~N(0,1), A = rho*G/spectral_radius(G); B~N(0,1); Q = MM^T/n + I; R = NN^T/m + I."""
    rng = np.random.default_rng(seed)
    A = np.empty((batch, n, n))
    B = np.empty((batch, n, m))
    Q = np.empty((batch, n, n))
    R = np.empty((batch, m, m))
    for i in range(batch):
        G = rng.standard_normal((n, n))
        A[i] = rho * G / np.max(np.abs(np.linalg.eigvals(G)))
        B[i] = rng.standard_normal((n, m))
        M = rng.standard_normal((n, n))
        N = rng.standard_normal((m, m))
        Q[i] = M @ M.T / n + np.eye(n)
        R[i] = N @ N.T / m + np.eye(m)
    return A.astype(dtype), B.astype(dtype), Q.astype(dtype), R.astype(dtype)


def tile_over_horizon(A, B, Q, R, T: int):
    """Materialise (b,T,.,.) time-varying tensors from per-system LTI matrices (the layout the
    reference API takes: demos/discreteFiniteHorizonLqr.py:30-34 tiles LTI matrices over T)."""
    def rep(X):
        return np.ascontiguousarray(np.repeat(X[:, None], T, axis=1))
    return rep(A), rep(B), rep(Q), rep(R)


def random_time_varying(batch: int, T: int, n: int, m: int, seed: int = 0, dtype=np.float64):
    """Fully time-varying well-conditioned problems: every (trajectory, step) has its own matrices."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((batch, T, n, n)) * (0.9 / np.sqrt(n))
    B = rng.standard_normal((batch, T, n, m))
    M = rng.standard_normal((batch, T, n, n))
    N = rng.standard_normal((batch, T, m, m))
    Q = M @ np.swapaxes(M, -1, -2) / n + np.eye(n)
    R = N @ np.swapaxes(N, -1, -2) / m + np.eye(m)
    return A.astype(dtype), B.astype(dtype), Q.astype(dtype), R.astype(dtype)


def random_ilqr_model(batch: int, T: int, n: int, m: int, seed: int = 0):
    """Random quadratic model along a trajectory for the iLQR backward pass: (AffineDynamics, QuadraticCost, Vf) fields.

    f_x ~ contraction-ish, f_u ~ N(0,1); stacked cost Hessian H = M M^T/(n+m) + I (positive definite); random
    gradients; terminal v_xx = M M^T/n + I."""
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((batch, T, n))
    f_x = rng.standard_normal((batch, T, n, n)) * (0.9 / np.sqrt(n))
    f_u = rng.standard_normal((batch, T, n, m))
    M = rng.standard_normal((batch, T, n + m, n + m))
    H = M @ np.swapaxes(M, -1, -2) / (n + m) + np.eye(n + m)
    c = rng.standard_normal((batch, T))
    c_x = rng.standard_normal((batch, T, n))
    c_u = rng.standard_normal((batch, T, m))
    c_xx = np.ascontiguousarray(H[..., :n, :n])
    c_ux = np.ascontiguousarray(H[..., n:, :n])
    c_uu = np.ascontiguousarray(H[..., n:, n:])
    Mv = rng.standard_normal((batch, n, n))
    v_xx = Mv @ np.swapaxes(Mv, -1, -2) / n + np.eye(n)
    v_x = rng.standard_normal((batch, n))
    v = rng.standard_normal(batch)
    return (f, f_x, f_u), (c, c_x, c_u, c_xx, c_ux, c_uu), (v, v_x, v_xx)


# ------------------------------------------------------------------------------------------------------------------------
# Hard-spectrum designs for the DARE and the finite-horizon sweep: each generator returns (A, B, Q, R), float64 arrays with a leading
# batch axis, with ONE known hard feature (tests/test_hp_reference.py asserts that each generator has it).
def _stable_block(rng, k, rho):
    G = rng.standard_normal((k, k))
    return rho * G / np.max(np.abs(np.linalg.eigvals(G)))


def _spd(rng, k):
    M = rng.standard_normal((k, k))
    return M @ M.T / k + np.eye(k)


def slow_unreachable_mode(batch: int, n: int, m: int, seed: int = 0, lam: float = 0.999, coupling: float = 0.0):
    """A random stable block (rho = 0.6) on states 0..n-2 plus a slow stable mode lam on state n-1 that the input cannot reach
    (B[n-1] = 0, A[n-1, :n-1] = 0); Q = R = I.  Its value entry 1/(1 - lam^2) ~ 500 dominates P, but with coupling = 0 the gain does
    not see it at all.  coupling > 0: the slow state drives the block (A[:n-1, n-1] ~ coupling), so the gain converges as slowly."""
    rng = np.random.default_rng(seed)
    A = np.zeros((batch, n, n))
    B = np.zeros((batch, n, m))
    for i in range(batch):
        A[i, :n - 1, :n - 1] = _stable_block(rng, n - 1, 0.6)
        A[i, :n - 1, n - 1] = coupling * rng.standard_normal(n - 1)
        A[i, n - 1, n - 1] = lam
        B[i, :n - 1] = rng.standard_normal((n - 1, m))
    return A, B, np.tile(np.eye(n), (batch, 1, 1)), np.tile(np.eye(m), (batch, 1, 1))


def weakly_detectable_unstable(batch: int, n: int, m: int, seed: int = 0, lam: float = 1.001, q: float = 1e-6):
    """An unstable mode lam on state n-1, reached by B, weighted by only q in Q: the optimal loop mirrors it to ~1/lam, so the closed
    loop's spectral radius is ~0.999 and value iteration converges slowly after a long transient."""
    rng = np.random.default_rng(seed)
    A = np.zeros((batch, n, n))
    B = rng.standard_normal((batch, n, m))
    Q = np.zeros((batch, n, n))
    R = np.empty((batch, m, m))
    for i in range(batch):
        A[i, :n - 1, :n - 1] = _stable_block(rng, n - 1, 0.6)
        A[i, n - 1, n - 1] = lam
        Q[i, :n - 1, :n - 1] = _spd(rng, n - 1)
        Q[i, n - 1, n - 1] = q
        R[i] = _spd(rng, m)
    return A, B, Q, R


def marginally_stabilisable(batch: int, n: int, m: int, seed: int = 0, lam: float = 1.02, b: float = 1e-2):
    """An unstable mode lam on state n-1 that only input 0 reaches, through B[n-1, 0] = b: stabilising it costs ~1/b^2, so its value
    entry is large and the gain's column n-1 is large."""
    rng = np.random.default_rng(seed)
    A = np.zeros((batch, n, n))
    B = np.empty((batch, n, m))
    Q = np.empty((batch, n, n))
    R = np.empty((batch, m, m))
    for i in range(batch):
        A[i, :n - 1, :n - 1] = _stable_block(rng, n - 1, 0.6)
        A[i, n - 1, n - 1] = lam
        B[i, :n - 1] = rng.standard_normal((n - 1, m))
        B[i, n - 1] = 0.0
        B[i, n - 1, 0] = b
        Q[i] = _spd(rng, n)
        R[i] = _spd(rng, m)
    return A, B, Q, R


def cheap_control(batch: int, n: int, m: int, seed: int = 0):
    """R = 1e-8 I on an unstable random system (rho(A) = 1.2): R + B^T V B is dominated by B^T V B."""
    A, B, Q, _ = random_lti_systems(batch, n, m, seed=seed, rho=1.2)
    return A, B, Q, np.tile(1e-8 * np.eye(m), (batch, 1, 1))


def expensive_control(batch: int, n: int, m: int, seed: int = 0):
    """R = 1e8 I on an unstable random system (rho(A) = 1.05): the gain is tiny and the unstable modes are only just mirrored."""
    A, B, Q, _ = random_lti_systems(batch, n, m, seed=seed, rho=1.05)
    return A, B, Q, np.tile(1e8 * np.eye(m), (batch, 1, 1))


def badly_scaled(batch: int, n: int, m: int, seed: int = 0, rho: float = 1.05):
    """A random system in coordinates x' = D x, D = diag(logspace(-2, 2, n)): D A D^-1, D B, D^-T Q D^-1, R.  The solution is
    P' = D^-1 P D^-1, L' = L D^-1: entries over eight decades."""
    A, B, Q, R = random_lti_systems(batch, n, m, seed=seed, rho=rho)
    d = np.logspace(-2, 2, n)
    return A * d[:, None] / d[None, :], B * d[:, None], Q / d[:, None] / d[None, :], R


# name -> generator (batch, n, m, seed) of the hard-spectrum families above
HARD_DARE = {
    "slow_unreachable": slow_unreachable_mode,
    "slow_coupled": lambda batch, n, m, seed=0: slow_unreachable_mode(batch, n, m, seed=seed, coupling=1e-3),
    "weakly_detectable": weakly_detectable_unstable,
    "marginally_stabilisable": marginally_stabilisable,
    "cheap_control": cheap_control,
    "expensive_control": expensive_control,
    "badly_scaled": badly_scaled,
}


def hard_dare(name: str, n: int, m: int, batch: int = 2):
    """The seeded batch of HARD_DARE[name] at (n, m) that both the CPU property tests and the GPU tests use."""
    return HARD_DARE[name](batch, n, m, seed=1000 + 97 * n + m)


# ------------------------------------------------------------------------------------------------------------------------
# Hard-spectrum designs for the continuous-time Riccati equation (care.hip): the counterparts of HARD_DARE.  Each returns
# (A, B, Q, R) with a leading batch axis and ONE hard feature (tests/test_hp_reference.py asserts it); none has Hamiltonian
# eigenvalues on the imaginary axis, so the stabilising solution exists and is unique.
def _abscissa_block(rng, k, alpha):
    """A random k x k block G / sqrt(k), shifted so that its spectral abscissa max Re(eig) is alpha."""
    G = rng.standard_normal((k, k)) / np.sqrt(k)
    return G + (alpha - np.max(np.linalg.eigvals(G).real)) * np.eye(k)


def care_slow_unreachable(batch: int, n: int, m: int, seed: int = 0, lam: float = -1e-3):
    """A stable random block (abscissa -0.5) on states 0..n-2 plus a mode lam on state n-1 that B does not reach; Q = R = I.  The
    mode stays in the closed loop and its value entry -1 / (2 lam) = 500 dominates P.  lam > 0: no stabilising solution."""
    rng = np.random.default_rng(seed)
    A = np.zeros((batch, n, n))
    B = np.zeros((batch, n, m))
    for i in range(batch):
        A[i, :n - 1, :n - 1] = _abscissa_block(rng, n - 1, -0.5)
        A[i, n - 1, n - 1] = lam
        B[i, :n - 1] = rng.standard_normal((n - 1, m))
    return A, B, np.tile(np.eye(n), (batch, 1, 1)), np.tile(np.eye(m), (batch, 1, 1))


def care_weakly_detectable(batch: int, n: int, m: int, seed: int = 0, lam: float = 1e-3, q: float = 1e-6):
    """An unstable mode lam on state n-1, reached by B, weighted by only q in Q: the optimal loop mirrors it to about -lam, so the
    Hamiltonian has eigenvalues ~1e-3 from the imaginary axis."""
    rng = np.random.default_rng(seed)
    A = np.zeros((batch, n, n))
    B = rng.standard_normal((batch, n, m))
    Q = np.zeros((batch, n, n))
    R = np.empty((batch, m, m))
    for i in range(batch):
        A[i, :n - 1, :n - 1] = _abscissa_block(rng, n - 1, -0.5)
        A[i, n - 1, n - 1] = lam
        Q[i, :n - 1, :n - 1] = _spd(rng, n - 1)
        Q[i, n - 1, n - 1] = q
        R[i] = _spd(rng, m)
    return A, B, Q, R


def care_marginally_stabilisable(batch: int, n: int, m: int, seed: int = 0, lam: float = 0.02, b: float = 1e-2):
    """An unstable mode lam on state n-1 that only input 0 reaches, through B[n-1, 0] = b: stabilising it costs ~ 2 lam / b^2, so its
    value entry and the gain's column n-1 are large."""
    rng = np.random.default_rng(seed)
    A = np.zeros((batch, n, n))
    B = np.empty((batch, n, m))
    Q = np.empty((batch, n, n))
    R = np.empty((batch, m, m))
    for i in range(batch):
        A[i, :n - 1, :n - 1] = _abscissa_block(rng, n - 1, -0.5)
        A[i, n - 1, n - 1] = lam
        B[i, :n - 1] = rng.standard_normal((n - 1, m))
        B[i, n - 1] = 0.0
        B[i, n - 1, 0] = b
        Q[i] = _spd(rng, n)
        R[i] = _spd(rng, m)
    return A, B, Q, R


def _care_random(batch, n, m, seed, alpha):
    rng = np.random.default_rng(seed)
    A = np.stack([_abscissa_block(rng, n, alpha) for _ in range(batch)])
    B = rng.standard_normal((batch, n, m))
    Q = np.stack([_spd(rng, n) for _ in range(batch)])
    R = np.stack([_spd(rng, m) for _ in range(batch)])
    return A, B, Q, R


def care_cheap_control(batch: int, n: int, m: int, seed: int = 0, r: float = 1e-8):
    """R = r I on an unstable random system (abscissa +0.2): G = B R^-1 B^T ~ 1/r, B^T P = O(sqrt r), K = O(1 / sqrt r)."""
    A, B, Q, _ = _care_random(batch, n, m, seed, 0.2)
    return A, B, Q, np.tile(r * np.eye(m), (batch, 1, 1))


def care_expensive_control(batch: int, n: int, m: int, seed: int = 0):
    """R = 1e8 I on an unstable random system (abscissa +0.05): the gain is tiny, the unstable modes are only just mirrored."""
    A, B, Q, _ = _care_random(batch, n, m, seed, 0.05)
    return A, B, Q, np.tile(1e8 * np.eye(m), (batch, 1, 1))


def care_badly_scaled(batch: int, n: int, m: int, seed: int = 0):
    """A random system (abscissa +0.05) in coordinates x' = D x, D = diag(logspace(-2, 2, n)): D A D^-1, D B, D^-T Q D^-1, R.  The
    solution is P' = D^-1 P D^-1, K' = K D^-1: entries over eight decades."""
    A, B, Q, R = _care_random(batch, n, m, seed, 0.05)
    d = np.logspace(-2, 2, n)
    return A * d[:, None] / d[None, :], B * d[:, None], Q / (d[:, None] * d[None, :]), R        # (d_i d_j: Q stays exactly symmetric)


def care_stiff(batch: int, n: int, m: int, seed: int = 0):
    """A symmetric A with eigenvalues -logspace(-3, 3, n) in a random orthogonal basis plus a 1e-3 perturbation: time scales over six
    decades, so the Cayley shift gamma ~ |A| maps the slow modes to 1 - O(1e-6) and the doubling iteration needs ~20 steps."""
    rng = np.random.default_rng(seed)
    A = np.empty((batch, n, n))
    for i in range(batch):
        U, _ = np.linalg.qr(rng.standard_normal((n, n)))
        lam = -np.logspace(-3, 3, n) if n > 1 else np.array([-1.0])
        A[i] = (U * lam) @ U.T + 1e-3 * rng.standard_normal((n, n))
    B = rng.standard_normal((batch, n, m))
    Q = np.stack([_spd(rng, n) for _ in range(batch)])
    R = np.stack([_spd(rng, m) for _ in range(batch)])
    return A, B, Q, R


def care_integrator_chains(batch: int, n: int, m: int, seed: int = 0):
    """Nilpotent integrator chains of length 4 (the last one shorter when 4 does not divide n), one input per chain at its end, the
    couplings drawn from [0.5, 1.5]: every open-loop eigenvalue is 0 and defective.  Inputs beyond the chains are unused (zero
    columns of B).  More chains than inputs is refused: the single-input 16-chain has |P| ~ 1e35 and no usable reference."""
    chains = -(-n // 4)
    if m < chains:
        raise ValueError(f"integrator_chains needs m >= ceil(n / 4) = {chains} inputs, got {m}")
    rng = np.random.default_rng(seed)
    A = np.zeros((batch, n, n))
    B = np.zeros((batch, n, m))
    for i in range(batch):
        for c in range(chains):
            lo, hi = 4 * c, min(4 * c + 4, n)
            for j in range(lo, hi - 1):
                A[i, j, j + 1] = rng.uniform(0.5, 1.5)
            B[i, hi - 1, c] = rng.uniform(0.5, 1.5)
    Q = np.stack([_spd(rng, n) for _ in range(batch)])
    R = np.stack([_spd(rng, m) for _ in range(batch)])
    return A, B, Q, R


def care_light_oscillators(batch: int, n: int, m: int, seed: int = 0, damping: float = 1e-4, q: float = 1e-4):
    """2 x 2 rotation blocks [[-d, w], [-w, -d]], d = 1e-4, w in [0.5, 3] (a last state -d when n is odd), Q = q * SPD: the
    Hamiltonian's eigenvalues sit ~1e-2 |w| from the imaginary axis."""
    rng = np.random.default_rng(seed)
    A = np.zeros((batch, n, n))
    for i in range(batch):
        for j in range(0, n - 1, 2):
            w = rng.uniform(0.5, 3.0)
            A[i, j:j + 2, j:j + 2] = [[-damping, w], [-w, -damping]]
        if n % 2:
            A[i, n - 1, n - 1] = -damping
    B = rng.standard_normal((batch, n, m))
    Q = q * np.stack([_spd(rng, n) for _ in range(batch)])
    R = np.stack([_spd(rng, m) for _ in range(batch)])
    return A, B, Q, R


def _cheap(r):
    return lambda batch, n, m, seed=0: care_cheap_control(batch, n, m, seed=seed, r=r)


# name -> generator (batch, n, m, seed) of the continuous-time hard-spectrum families above
HARD_CARE = {
    "slow_unreachable": care_slow_unreachable,
    "weakly_detectable": care_weakly_detectable,
    "marginally_stabilisable": care_marginally_stabilisable,
    "cheap_control_1e-2": _cheap(1e-2),
    "cheap_control_1e-4": _cheap(1e-4),
    "cheap_control_1e-6": _cheap(1e-6),
    "cheap_control_1e-8": _cheap(1e-8),
    "expensive_control": care_expensive_control,
    "badly_scaled": care_badly_scaled,
    "stiff": care_stiff,
    "integrator_chains": care_integrator_chains,
    "light_oscillators": care_light_oscillators,
}


def hard_care(name: str, n: int, m: int, batch: int = 2):
    """The seeded batch of HARD_CARE[name] at (n, m) that both the CPU property tests and the GPU tests use."""
    return HARD_CARE[name](batch, n, m, seed=2000 + 97 * n + m)
