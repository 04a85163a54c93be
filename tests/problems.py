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


# ------------------------------------------------------------------------------------------------------------------------
# Hard quadratic models for the iLQR / affine-LQR / DDP backward sweeps (ilqr_backward.hip, sweep_tiled_f64.hip): each generator
# (batch, T, n, m, seed) -> (dyn, cost, Vf) starts from `random_ilqr_model` and gives it ONE hard feature
# (tests/test_hp_reference.py asserts that it has it).
def _sT(X):
    return np.swapaxes(X, -1, -2)


def _antisym(rng, shape, scale):
    N = rng.standard_normal(shape)
    return scale * (N - _sT(N))


def sweep_unstable(batch, T, n, m, seed=0, growth=1.3):
    """Every step's f_x is a random matrix scaled to the spectral radius `growth` > 1: the value grows along the sweep."""
    (f, f_x, f_u), cost, Vf = random_ilqr_model(batch, T, n, m, seed)
    rho = np.max(np.abs(np.linalg.eigvals(f_x)), axis=-1)
    return (f, f_x * (growth / rho)[..., None, None], f_u), cost, Vf


def sweep_cheap_control(batch, T, n, m, seed=0, r=None):
    """c_uu scaled by r = 1e-8 (c_ux and c_u by sqrt r, so the stacked Hessian stays positive definite): Q_uu is dominated by
    f_u^T v_xx f_u and Q_xx - L^T Q_uu L cancels what the controls reach.  With more controls than states f_u^T v_xx f_u is singular and
    cond(Q_uu) ~ 1 / r: r = 1e-4 there keeps the problem well posed in fp64."""
    r = (1e-8 if m <= n else 1e-4) if r is None else r
    dyn, (c, c_x, c_u, c_xx, c_ux, c_uu), Vf = random_ilqr_model(batch, T, n, m, seed)
    return dyn, (c, c_x, c_u * np.sqrt(r), c_xx, c_ux * np.sqrt(r), c_uu * r), Vf


def sweep_expensive_control(batch, T, n, m, seed=0, r=1e8):
    """c_uu scaled by 1e8: tiny gains."""
    dyn, (c, c_x, c_u, c_xx, c_ux, c_uu), Vf = random_ilqr_model(batch, T, n, m, seed)
    return dyn, (c, c_x, c_u, c_xx, c_ux, c_uu * r), Vf


def sweep_illcond_quu(batch, T, n, m, seed=0, r=None):
    """f_u of rank one (an outer product) and c_uu scaled by r = 1e-4 (1e-3 beyond m = 6): f_u^T v_xx f_u has rank one, so cond(Q_uu)
    ~ |f_u|^2 |v_xx| / r ~ 1e6..1e7 -- as ill conditioned as the fp64 oracle itself resolves to 1e-9 (m = 1: a rank-one f_u has full
    rank, only the small c_uu remains)."""
    r = (1e-4 if m <= 6 else 1e-3) if r is None else r
    (f, f_x, f_u), (c, c_x, c_u, c_xx, c_ux, c_uu), Vf = random_ilqr_model(batch, T, n, m, seed)
    rng = np.random.default_rng(seed + 1)
    f_u = rng.standard_normal((batch, T, n, 1)) * rng.standard_normal((batch, T, 1, m))
    return (f, f_x, f_u), (c, c_x, c_u * np.sqrt(r), c_xx, c_ux * np.sqrt(r), c_uu * r), Vf


def sweep_pivoting(batch, T, n, m, seed=0, scale=1e4):
    """c_uu + scale * (diag(c_uu) P), P a cyclic column shift, at every step: nonsymmetric, with entries ~scale off the diagonal
    and O(10) on it, so the elimination without row exchanges meets multipliers in the hundreds -- far above the kernels' limit of
    4 -- loses that many digits and must be abandoned, while Q_uu itself is well conditioned (m = 1: no permutation exists, the
    family is the plain one with a large c_uu)."""
    dyn, (c, c_x, c_u, c_xx, c_ux, c_uu), Vf = random_ilqr_model(batch, T, n, m, seed)
    dg = c_uu * np.eye(m)
    return dyn, (c, c_x, c_u, c_xx, c_ux, c_uu + scale * np.roll(dg, 1, axis=-1)), Vf


def sweep_scaling(n):
    """The diagonal of `sweep_badly_scaled`'s coordinate change x' = D x."""
    return np.logspace(-2, 2, n)


def sweep_badly_scaled(batch, T, n, m, seed=0):
    """The plain model in coordinates x' = D x, D = diag(logspace(-2, 2, n)), every operand transformed consistently: D f_x D^-1,
    D f_u, D^-1 c_x, D^-1 c_xx D^-1, c_ux D^-1, D^-1 v_x, D^-1 v_xx D^-1.  The policy is l' = l, L' = L D^-1: columns over four
    decades (c_xx and v_xx, scaled on both sides, over eight)."""
    (f, f_x, f_u), (c, c_x, c_u, c_xx, c_ux, c_uu), (v, v_x, v_xx) = random_ilqr_model(batch, T, n, m, seed)
    d = sweep_scaling(n)
    return ((f * d, f_x * d[:, None] / d[None, :], f_u * d[:, None]),
            (c, c_x / d, c_u, c_xx / (d[:, None] * d[None, :]), c_ux / d[None, :], c_uu),
            (v, v_x / d, v_xx / (d[:, None] * d[None, :])))


def sweep_nonsymmetric(batch, T, n, m, seed=0):
    """O(1) antisymmetric parts in c_xx, c_uu and v_xx: the reference's formulas do not symmetrise, so the kernels may not either."""
    dyn, (c, c_x, c_u, c_xx, c_ux, c_uu), (v, v_x, v_xx) = random_ilqr_model(batch, T, n, m, seed)
    rng = np.random.default_rng(seed + 2)
    return (dyn, (c, c_x, c_u, c_xx + _antisym(rng, c_xx.shape, 0.5), c_ux, c_uu + _antisym(rng, c_uu.shape, 0.5)),
            (v, v_x, v_xx + _antisym(rng, v_xx.shape, 0.5)))


def sweep_zero_gradient(batch, T, n, m, seed=0):
    """c_x = c_u = v_x = 0: l must be exactly 0 at every step."""
    dyn, (c, c_x, c_u, c_xx, c_ux, c_uu), (v, v_x, v_xx) = random_ilqr_model(batch, T, n, m, seed)
    return dyn, (c, 0 * c_x, 0 * c_u, c_xx, c_ux, c_uu), (v, 0 * v_x, v_xx)


# name -> generator (batch, T, n, m, seed); "plain" is the yardstick family the bounds' floor comes from, not a hard one
HARD_SWEEP = {
    "unstable": sweep_unstable,
    "cheap_control": sweep_cheap_control,
    "expensive_control": sweep_expensive_control,
    "illcond_quu": sweep_illcond_quu,
    "pivoting": sweep_pivoting,
    "badly_scaled": sweep_badly_scaled,
    "nonsymmetric": sweep_nonsymmetric,
    "zero_gradient": sweep_zero_gradient,
}


# The long horizon of every shape the GPU tests run, and the (family, shape) pairs that need a shorter one for the fp64 oracle's own error
# to stay below 1e-9 (tests/test_hp_reference.py asserts it): the value of `unstable` grows along directions one step cannot reach,
# that of `nonsymmetric` grows through its antisymmetric part.
SWEEP_T = {(12, 4): 100, (8, 4): 100, (5, 3): 40, (1, 1): 40, (11, 1): 40, (3, 4): 40, (16, 4): 12, (20, 6): 8, (33, 9): 5, (48, 16): 4}
SWEEP_T_SHORTER = {("unstable", 12, 4): 60, ("unstable", 8, 4): 60, ("nonsymmetric", 12, 4): 20, ("nonsymmetric", 8, 4): 20}


def sweep_horizon(name: str, n: int, m: int):
    return SWEEP_T_SHORTER.get((name, n, m), SWEEP_T[(n, m)])


def hard_sweep(name: str, n: int, m: int, T: int, batch: int = 2, shared: bool = False):
    """The seeded batch of HARD_SWEEP[name] (or of the plain family, name "plain") at (n, m, T) that the CPU property tests and the
    GPU tests both use; shared: with `share_hessians`."""
    gen = random_ilqr_model if name == "plain" else HARD_SWEEP[name]
    out = gen(batch, T, n, m, 3000 + 97 * n + 13 * m + T)
    return share_hessians(*out) if shared else out


def hard_affine(name: str, n: int, m: int, T: int, batch: int = 2):
    """The `bilinearAffineLqr` operands (A, B, d, Q, R, H, q, r, q0) of `hard_sweep(name, ...)`: A = f_x, B = f_u, Q = c_xx, R = c_uu,
    H = c_ux, q = c_x, r = c_u, q0 = c and a non-zero offset d (in `badly_scaled`'s coordinates where that is the family).  The
    recursion starts from Q[T-1], q[T-1]; the model's terminal value is not used."""
    (f, f_x, f_u), (c, c_x, c_u, c_xx, c_ux, c_uu), _ = hard_sweep(name, n, m, T, batch)
    d = 0.5 * np.random.default_rng(4000 + 97 * n + 13 * m + T).standard_normal((batch, T, n))
    if name == "badly_scaled":
        d = d * sweep_scaling(n)
    return f_x, f_u, d, c_xx, c_uu, c_ux, c_x, c_u, c


# ------------------------------------------------------------------------------------------------------------------------
# Hard time-varying problems for the finite-horizon Riccati sweep `discreteFiniteHorizonLqr` (lqr_backward_dma.hip, lqr_backward.hip,
# lqr_tiled_core.h, lqr_backward_lds_f64.hip): each generator (batch, T, n, m, seed) -> (A, B, Q, R) starts from `random_time_varying` and
# gives it ONE hard feature (tests/test_lqr_hard.py asserts that it has it).  Several of them are built to leave the kernels' fast m x m
# solve: K1's cofactor solve behind its residual guard, the unpivoted elimination of the other kernels behind its growth check.
def _pow2_span(k, decades):
    """k powers of two spread evenly (in the exponent) over 10^-decades .. 10^decades; a single one is 1."""
    e = np.round(np.linspace(-decades, decades, k) * np.log2(10.0)) if k > 1 else np.zeros(1)
    return 2.0 ** e


def lqr_units(n, m):
    """The diagonals (D, E) of `lqr_input_units`' coordinate change x' = D x, u' = E u: powers of two over 1e-2 .. 1e2 and 1e-3 .. 1e3."""
    return _pow2_span(n, 2), _pow2_span(m, 3)


def lqr_mildly_unstable(batch, T, n, m, seed=0, rho=1.05):
    """Every A_k scaled to the spectral radius rho (the problem that `lqr_input_units` writes in other units; rho = 1.3: `unstable`)."""
    A, B, Q, R = random_time_varying(batch, T, n, m, seed)
    return A * (rho / np.max(np.abs(np.linalg.eigvals(A)), axis=-1))[..., None, None], B, Q, R


def lqr_input_units(batch, T, n, m, seed=0):
    """`lqr_mildly_unstable` in the coordinates x' = D x, u' = E u of `lqr_units`: D A D^-1, D B E^-1, D^-1 Q D^-1, E^-1 R E^-1.  Suu' =
    E^-1 Suu E^-1 is graded over twelve decades (its entries, not its condition after scaling), the gain is L' = E L D^-1: undoing the
    units, E^-1 L' D, is exact."""
    A, B, Q, R = lqr_mildly_unstable(batch, T, n, m, seed)
    d, e = lqr_units(n, m)
    return A * d[:, None] / d[None, :], B * d[:, None] / e[None, :], Q / (d[:, None] * d[None, :]), R / (e[:, None] * e[None, :])


def lqr_dominant_input(batch, T, n, m, seed=0, r=1.0, every=1):
    """B_k = u_k v_k^T of rank one and R_k scaled by r on the steps k = 0 mod `every` (plain elsewhere): B^T V B = (u^T V u) v v^T has
    rank one and dominates Suu = r R + B^T V B, whose rows are then nearly parallel."""
    A, B, Q, R = random_time_varying(batch, T, n, m, seed)
    rng = np.random.default_rng(seed + 1)
    B1 = rng.standard_normal((batch, T, n, 1)) * rng.standard_normal((batch, T, 1, m))
    hit = (np.arange(T) % every == 0)[None, :, None, None]
    return A, np.where(hit, B1, B), Q, np.where(hit, r * R, R)


def lqr_permuted_R(batch, T, n, m, seed=0):
    """B scaled by 0.02 and R_k = (a cyclic column shift of I) + 0.01 noise, nonsymmetric: Suu ~ R_k is well conditioned (a perturbed
    permutation), but its leading entry is ~0.01, so the elimination without row exchanges meets multipliers ~100 at the first column
    (m = 1: no permutation exists, R = 1 + noise)."""
    A, B, Q, _ = random_time_varying(batch, T, n, m, seed)
    rng = np.random.default_rng(seed + 2)
    R = np.roll(np.eye(m), 1, axis=-1) + 0.01 * rng.standard_normal((batch, T, m, m))
    return A, 0.02 * B, Q, R


def lqr_nonsymmetric(batch, T, n, m, seed=0):
    """O(1) antisymmetric parts in every Q_k and R_k: the reference's recursion does not symmetrise, so the kernels may not either."""
    A, B, Q, R = random_time_varying(batch, T, n, m, seed)
    rng = np.random.default_rng(seed + 3)
    return A, B, Q + _antisym(rng, Q.shape, 0.5), R + _antisym(rng, R.shape, 0.5)


def lqr_cheap(batch, T, n, m, seed=0, r=None):
    """R_k scaled by r = 1e-8 on unstable dynamics (every A_k at the spectral radius 1.2, as `cheap_control`): Suu is dominated by B^T V B,
    and a value update that subtracts (the Schur form) instead of the Joseph form loses digits along the horizon.  With more controls
    than states B^T V B is singular and cond(Suu) ~ 1 / r: r = 1e-4 there keeps the problem well posed in fp64 (`sweep_cheap_control`)."""
    r = (1e-8 if m <= n else 1e-4) if r is None else r
    A, B, Q, R = lqr_mildly_unstable(batch, T, n, m, seed, rho=1.2)
    return A, B, Q, r * R


def lqr_expensive(batch, T, n, m, seed=0, r=1e8):
    """R_k scaled by 1e8: Suu is dominated by R, the gains are ~1e-7."""
    A, B, Q, R = random_time_varying(batch, T, n, m, seed)
    return A, B, Q, r * R


# name -> generator (batch, T, n, m, seed); "plain" is the yardstick family the bounds' floor comes from, not a hard one
HARD_LQR = {
    "plain": random_time_varying,
    "input_units": lqr_input_units,
    "dominant_input": lqr_dominant_input,
    "dominant_input_1e-2": lambda batch, T, n, m, seed=0: lqr_dominant_input(batch, T, n, m, seed, r=1e-2),
    "dominant_every_3": lambda batch, T, n, m, seed=0: lqr_dominant_input(batch, T, n, m, seed, r=1e-2, every=3),
    "permuted_R": lqr_permuted_R,
    "unstable": lambda batch, T, n, m, seed=0: lqr_mildly_unstable(batch, T, n, m, seed, rho=1.3),
    "cheap": lqr_cheap,
    "expensive": lqr_expensive,
    "nonsymmetric": lqr_nonsymmetric,
}


# (family, n, m, T) -> seed offset, in thousands, of the cases whose first seed leaves a step of K1's model within a factor 8 of the guard's
# threshold (tests/test_lqr_hard.py asserts the margins): there the GPU's rounding of Suu could decide the branch the other way
LQR_SEED_BUMP = {("input_units", 12, 4, 7): 1, ("dominant_input_1e-2", 8, 4, 11): 1}


def hard_lqr(name: str, n: int, m: int, T: int, batch: int = 5):
    """The seeded batch of HARD_LQR[name] at (n, m, T) that the CPU property tests and the GPU tests both use."""
    return HARD_LQR[name](batch, T, n, m, hard_lqr_seed(name, n, m, T))


def hard_lqr_seed(name: str, n: int, m: int, T: int):
    return 9000 + 97 * n + 13 * m + T + 1000 * LQR_SEED_BUMP.get((name, n, m, T), 0)


# ------------------------------------------------------------------------------------------------------------------------
# Spectra that stress the PD projection V max(w, eps) V^T (ns16.h, psd_tiled.hip), shared by the stand-alone projection tests.
ADVERSARIAL_SPECTRA = ("scaled_normal", "half_at_eps", "sixteen_decades", "rank_one", "dominant_pair", "hugging_eps", "zero_rows",
                       "all_pd")


def adversarial_spectrum(kind, k: int, rng):
    """Eigenvalues (k,) of kind ADVERSARIAL_SPECTRA[kind] (or its name), drawn from `rng`, for the clamp eps = 1e-3: many decades of
    magnitude, eigenvalues hugging eps from both sides, rank one, a dominant pair, everything already PD.  "zero_rows" is a plain
    wide spectrum; its caller zeroes rows and columns of the assembled matrix."""
    kind = ADVERSARIAL_SPECTRA.index(kind) if isinstance(kind, str) else kind
    if kind == 0:
        return rng.standard_normal(k) * 10 ** rng.uniform(-3, 3)
    if kind == 1:
        return np.concatenate([rng.standard_normal(k // 2), 1e-3 + rng.standard_normal(k - k // 2) * 1e-9])
    if kind == 2:
        return 10.0 ** rng.uniform(-14, 2, k) * rng.choice([-1, 1], k)
    if kind == 3:
        lam = np.zeros(k)
        lam[0] = rng.standard_normal()
        return lam
    if kind == 4:
        lam = rng.standard_normal(k)
        lam[:2] = 1e3
        return lam
    if kind == 5:
        return 1e-3 + 10.0 ** rng.uniform(-16, -2, k) * rng.choice([-1, 1], k)
    if kind == 6:
        return rng.standard_normal(k) * 10 ** rng.uniform(0, 2)
    return 10.0 ** rng.uniform(-2, 4, k)


# ------------------------------------------------------------------------------------------------------------------------
# Second-derivative families for the DDP sweep: (f_xx, f_ux, f_uu) stacked on a plain or an unstable model such that the matrix the
# sweep projects, vf_zz = sum_i v_x[i] d2f_i, has a planted spectrum at the terminal step: the terminal v_x is the unit vector of
# state I0, the slice I0 of every step holds a matrix with a planted spectrum (tests.hp_reference.psd_from_spectrum_ld), the other
# slices are small.  Earlier steps project whatever the sweep makes of it; hp_reference.ddp_backward_hp reports that spectrum.
DDP_I0 = 1
DDP_EPS = 1e-3


def ddp_spectrum(name: str, k: int, rng):
    """The planted eigenvalues (k,) of the DDP family `name`."""
    if name == "strongly_indefinite":
        return rng.uniform(10, 100, k) * rng.choice([-1, 1], k)
    if name == "hugging_eps":
        return DDP_EPS + 10.0 ** rng.uniform(-9, -3, k) * rng.choice([-1, 1], k)
    if name == "wide_decades":
        return 10.0 ** rng.uniform(-10, 2, k) * rng.choice([-1, 1], k)
    if name == "half_at_eps":
        lam = rng.standard_normal(k)
        lam[k // 2:] = DDP_EPS + 1e-8 * rng.uniform(1, 3, k - k // 2) * rng.choice([-1, 1], k - k // 2)
        return lam
    if name == "rank_one":
        lam = np.zeros(k)
        lam[0] = rng.uniform(0.5, 2) * rng.choice([-1, 1])
        return lam
    if name == "all_pd":
        return DDP_EPS + 10.0 ** rng.uniform(-2, 1, k)
    raise KeyError(name)


def _ddp_planted(name, other, model=random_ilqr_model):
    def gen(batch, T, n, m, seed=0):
        from tests import hp_reference as hp
        (f, f_x, f_u), (c, c_x, c_u, c_xx, c_ux, c_uu), (v, v_x, v_xx) = model(batch, T, n, m, seed)
        rng = np.random.default_rng(seed + 5)
        k = n + m
        Z = other * rng.standard_normal((batch, T, n, k, k))
        Z = Z + _sT(Z)
        planted = np.empty((batch, T, k))
        for b in range(batch):
            for t in range(T):
                planted[b, t] = ddp_spectrum(name, k, rng)
                Z[b, t, DDP_I0 % n] = hp.psd_from_spectrum_ld(k, planted[b, t], int(rng.integers(1 << 31)), DDP_EPS)[0]
        v_x = np.zeros((batch, n))
        v_x[:, DDP_I0 % n] = 1.0
        f_xx, f_ux, f_uu = (np.ascontiguousarray(X) for X in (Z[..., :n, :n], Z[..., n:, :n], Z[..., n:, n:]))
        return (f, f_x, f_u, f_xx, f_ux, f_uu), (c, c_x, c_u, c_xx, c_ux, c_uu), (v, v_x, v_xx), planted[:, T - 1]
    return gen


def _ddp_control_affine(rows):
    def gen(batch, T, n, m, seed=0):
        """f_ux = f_uu = 0 exactly and f_xx non-zero only among the first `rows` states (a model that is affine in its controls and
        in its other states): exactly zero rows / columns in vf_zz, and the projection's row-group dispatch."""
        dyn, cost, Vf = random_ilqr_model(batch, T, n, m, seed)
        rng = np.random.default_rng(seed + 5)
        r = min(rows, n)
        f_xx = np.zeros((batch, T, n, n, n))
        blk = 0.2 * rng.standard_normal((batch, T, n, r, r))
        f_xx[..., :r, :r] = blk + _sT(blk)
        return dyn + (f_xx, np.zeros((batch, T, n, m, n)), np.zeros((batch, T, n, m, m))), cost, Vf, None
    return gen


def ddp_vanishing(batch, T, n, m, seed=0):
    """v_x = 0 at the terminal step and c_x = 0, so vf_zz = 0 exactly on the last step (the projection has nothing to iterate on);
    c_u ~ 1e-12 makes v_x, and with it vf_zz, ~1e-12 on the steps before: a - eps I is -eps I to twelve digits."""
    (f, f_x, f_u), (c, c_x, c_u, c_xx, c_ux, c_uu), (v, v_x, v_xx) = random_ilqr_model(batch, T, n, m, seed)
    rng = np.random.default_rng(seed + 5)
    sym = lambda X: X + _sT(X)      # noqa: E731
    second = (sym(0.2 * rng.standard_normal((batch, T, n, n, n))), 0.2 * rng.standard_normal((batch, T, n, m, n)),
              sym(0.2 * rng.standard_normal((batch, T, n, m, m))))
    return (f, f_x, f_u) + second, (c, 0 * c_x, 1e-12 * c_u, c_xx, c_ux, c_uu), (v, 0 * v_x, v_xx), None


def ddp_plain(batch, T, n, m, seed=0):
    """The yardstick family of the DDP bounds: `random_ilqr_model` with 0.2 randn second derivatives (the existing parity tests')."""
    dyn, cost, Vf = random_ilqr_model(batch, T, n, m, seed)
    rng = np.random.default_rng(seed + 5)
    sym = lambda X: 0.5 * (X + _sT(X))      # noqa: E731
    return (dyn + (0.2 * sym(rng.standard_normal((batch, T, n, n, n))), 0.2 * rng.standard_normal((batch, T, n, m, n)),
                   0.2 * sym(rng.standard_normal((batch, T, n, m, m)))), cost, Vf, None)


# name -> generator (batch, T, n, m, seed) -> (dyn with second derivatives, cost, Vf, planted terminal spectrum (batch, n + m) or None)
HARD_DDP = {
    "strongly_indefinite": _ddp_planted("strongly_indefinite", 1e-2, model=lambda *a: sweep_unstable(*a, growth=1.1)),
    "hugging_eps": _ddp_planted("hugging_eps", 1e-6),
    "half_at_eps": _ddp_planted("half_at_eps", 1e-12),
    "wide_decades": _ddp_planted("wide_decades", 1e-3),
    "rank_one": _ddp_planted("rank_one", 1e-3),
    "control_affine_4": _ddp_control_affine(4),
    "control_affine_8": _ddp_control_affine(8),
    "control_affine_9": _ddp_control_affine(9),
    "vanishing": ddp_vanishing,
    "all_pd": _ddp_planted("all_pd", 0.0),
}


def share_hessians(dyn, cost, Vf):
    """The same model with ONE cost Hessian for every trajectory and step (c_xx[0, 0] etc., and v_xx[0]): the time-invariant quadratic
    cost the sweeps take as single matrices (`shared_hessian = 1`)."""
    c, c_x, c_u, c_xx, c_ux, c_uu = cost
    v, v_x, v_xx = Vf
    bc = lambda X, lead: np.broadcast_to(X[(0,) * lead], X.shape).copy()      # noqa: E731
    return dyn, (c, c_x, c_u, bc(c_xx, 2), bc(c_ux, 2), bc(c_uu, 2)), (v, v_x, bc(v_xx, 1))


# the 28 variable pairs (a <= b, all among the first 9 states) in which the registered quadcopter model has a second derivative
# (zm_model_hessian_pairs; tests/test_sweeps_hard_gpu.py checks this copy against the library's)
QUAD_HESSIAN_PAIRS = [(0, 0), (1, 1), (2, 2), (2, 4), (1, 5), (0, 5), (2, 3), (1, 3), (0, 4), (6, 6), (6, 7), (7, 7), (6, 8), (7, 8), (8, 8),
                      (0, 6), (0, 7), (0, 8), (1, 6), (1, 7), (1, 8), (2, 6), (2, 7), (2, 8), (4, 6), (4, 7), (5, 6), (5, 7)]


def ddp_packed_pairs(batch, T, n, m, seed=0):
    """`control_affine_9` at the quadcopter's shape with f_xx restricted to the model's 28 declared pairs and shared cost Hessians: the
    numbers the packed-pairs sweep (zm_ddp_backward_pairs_list_f64, LDS-ring form) takes as H[b, t, p, i] = f_xx[b, t, i, a_p, b_p]."""
    assert (n, m) == (12, 4)
    dyn, cost, Vf, _ = _ddp_control_affine(9)(batch, T, n, m, seed)
    keep = np.zeros((n, n))
    for a, b in QUAD_HESSIAN_PAIRS:
        keep[a, b] = keep[b, a] = 1.0
    (f, f_x, f_u), cost, Vf = share_hessians(dyn[:3], cost, Vf)
    return (f, f_x, f_u, dyn[3] * keep, dyn[4], dyn[5]), cost, Vf, None


def hard_ddp(name: str, n: int, m: int, T: int, batch: int = 2):
    """The seeded batch of HARD_DDP[name] (or of `ddp_plain`, name "plain"; of `ddp_packed_pairs`, name "packed_pairs") at (n, m, T) that the CPU property tests and the GPU
    tests both use."""
    gen = {"plain": ddp_plain, "packed_pairs": ddp_packed_pairs}.get(name) or HARD_DDP[name]
    return gen(batch, T, n, m, 5000 + 97 * n + 13 * m + T)


# The (n, m) the hard-family GPU tests run on each path (T from `sweep_horizon`; the DDP horizons stay short: every step costs the
# reference a long-double eigensolve).
ILQR_ONE_TILE_SHAPES = [(12, 4), (8, 4), (5, 3), (1, 1), (11, 1), (3, 4)]
ILQR_TILED_SHAPES = [(16, 4), (20, 6), (33, 9), (48, 16)]
AFFINE_SHAPES = [(12, 4), (8, 4), (5, 3), (20, 6), (48, 16)]
DDP_SHAPES = {(12, 4): 8, (5, 3): 6, (2, 2): 5, (16, 4): 4, (20, 6): 3}      # (n, m) -> T
RING_HORIZONS = [1, 2, 3, 4, 7]                                               # around the DMA ring's depth, on `unstable`
PSD_SIZES = [2, 7, 16, 17, 32, 33, 48, 49, 64]


# ------------------------------------------------------------------------------------------------------------------------
# Hard families for the MPC setup kernels (mpc_setup_body.h and its stage-varying copies in mpc.hip): the Riccati tables K, Minv, D of a
# problem at its penalty levels.  Every family has Q >= 0, R > 0, symmetric weights and a non-zero offset c; each has ONE hard feature
# (tests/test_mpc_tables.py asserts that it has it).  Stage form, as zm_mpc_setup_ltv_stage_f64 documents it: Qs[k] weights x_{k+1} (row
# N - 1 is terminal), Rs[k] weights u_k; the cost's Hessians are 2 Qs, 2 Rs, so Qs = sym(c_xx) / 2 and Rs = sym(c_uu) / 2 of a sweep model.
MPC_SWEEP_FAMILIES = ("plain", "unstable", "cheap_control", "expensive_control", "illcond_quu", "badly_scaled")
MPC_LTI_FAMILIES = ("lti_unstable", "lti_marginal")           # constant A, B, Q, R (+ a terminal Qf): what zm_mpc_setup_f64 takes
MPC_FAMILIES = MPC_SWEEP_FAMILIES + MPC_LTI_FAMILIES + ("stage_weights",)
MPC_LTI_RADIUS = {"lti_unstable": 1.3, "lti_marginal": 1.05}
MPC_N_LEVELS, MPC_RHO_STEP = 7, 5.0                             # lqrMpc.N_LEVELS, RHO_STEP

# (n, m, N): the smallest shapes that still show the defect of an unsymmetrised recursion, the horizon edges, the <24, 8> instantiation of
# the time-invariant kernels (the stage-varying entry points stop at (12, 4)), and a shape that does not fill the <12, 4> template
MPC_TABLE_SHAPES = [(12, 4, 75), (8, 4, 75), (4, 2, 75), (2, 1, 75), (1, 1, 75), (12, 4, 1), (12, 4, 2), (13, 2, 40), (24, 8, 40), (5, 3, 20)]


def _sym(X):
    return 0.5 * (X + _sT(X))


def mpc_penalty(Qs, Rs):
    """mpcUtils' rule for the penalty of level `n_levels // 2`, per problem: the geometric mean of the mean curvatures of 2 Qs_k and
    2 Rs_k (each floored at 1e-12), then the median over the stages.  Qs (P, N, n, n), Rs (P, N, m, m) -> (P,)"""
    tq = np.trace(2 * Qs, axis1=-2, axis2=-1) / Qs.shape[-1]
    tr = np.trace(2 * Rs, axis1=-2, axis2=-1) / Rs.shape[-1]
    return np.median(np.sqrt(np.maximum(tq, 1e-12) * np.maximum(tr, 1e-12)), axis=-1)


def mpc_levels(rho):
    """(P,) -> (P, L): the penalty of every level, rho * 5^(l - 3), as the host layer tabulates them"""
    fac = np.array([MPC_RHO_STEP ** (l - MPC_N_LEVELS // 2) for l in range(MPC_N_LEVELS)])
    return np.asarray(rho, dtype=np.float64).reshape(-1, 1) * fac[None, :]


def hard_mpc(name: str, n: int, m: int, N: int, P: int = 2):
    """The seeded batch of P problems of the MPC family `name` at (n, m, N) that the CPU property tests and the GPU tests both use:
    (A (P, N, n, n), B (P, N, n, m), c (P, N, n), Qs (P, N, n, n), Rs (P, N, m, m), rho (P, L)), rho from `mpc_penalty` and `mpc_levels`.

        the MPC_SWEEP_FAMILIES   the model of `hard_sweep` (its generator at the horizon N): A = f_x, B = f_u, c = f, Qs = sym(c_xx) / 2,
                                 Rs = sym(c_uu) / 2, all stage-varying
        lti_unstable, _marginal  ONE random A per problem scaled to the spectral radius 1.3 / 1.05, one B, Q, R for every stage and a
                                 terminal Qf; c varies by stage
        stage_weights            the plain dynamics with Q_k = 0 at most stages (every tenth keeps its weight), a terminal weight 100
                                 times the plain one, and R_k growing by 1e4 along the horizon"""
    seed = 7000 + 97 * n + 13 * m + N
    if name in MPC_SWEEP_FAMILIES:
        gen = random_ilqr_model if name == "plain" else HARD_SWEEP[name]
        (f, f_x, f_u), (_, _, _, c_xx, _, c_uu), _ = gen(P, N, n, m, seed)
        A, B, c, Qs, Rs = f_x, f_u, f, _sym(c_xx) / 2, _sym(c_uu) / 2
    elif name in MPC_LTI_FAMILIES:
        (f, f_x, f_u), (_, _, _, c_xx, _, c_uu), (_, _, v_xx) = random_ilqr_model(P, N, n, m, seed)
        A0 = f_x[:, 0] * (MPC_LTI_RADIUS[name] / np.max(np.abs(np.linalg.eigvals(f_x[:, 0])), axis=-1))[:, None, None]
        rep = lambda X: np.array(np.broadcast_to(X[:, None], (P, N) + X.shape[1:]))      # noqa: E731
        A, B, c, Qs, Rs = rep(A0), rep(f_u[:, 0]), f, rep(_sym(c_xx[:, 0]) / 2), rep(_sym(c_uu[:, 0]) / 2)
        Qs[:, N - 1] = _sym(v_xx) / 2
    elif name == "stage_weights":
        (f, f_x, f_u), (_, _, _, c_xx, _, c_uu), _ = random_ilqr_model(P, N, n, m, seed)
        keep = (np.arange(N) % 10 == 9).astype(np.float64)
        keep[N - 1] = 100.0
        grow = 10.0 ** (4.0 * np.arange(N) / max(N - 1, 1))
        A, B, c = f_x, f_u, f
        Qs, Rs = _sym(c_xx) / 2 * keep[None, :, None, None], _sym(c_uu) / 2 * grow[None, :, None, None]
    else:
        raise KeyError(name)
    A, B, c, Qs, Rs = (np.ascontiguousarray(X, dtype=np.float64) for X in (A, B, c, Qs, Rs))
    return A, B, c, Qs, Rs, mpc_levels(mpc_penalty(Qs, Rs))
