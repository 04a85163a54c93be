"""NumPy restatement of riccati_ode_kernel (zopt_amd/csrc/care.hip), step for step, and the cases the step-pinned tests run.

The kernel integrates dV/ds = Q + V A + A^T V - (V S) V, S = (B R_inv) B^T, in reversed time s = T - t from V(0) = Qf with an adaptive
Dormand-Prince 5(4) pair.  `riccati_ode` restates every decision the kernel takes -- the tableau and FSAL, the Hairer first-step rule
with its 1e-5 / 1e-15 branches, the tolerance-scaled RMS norm over the n^2 entries, `err <= 1` acceptance, the controller
min(10, max(err < 1 ? 1 : 0.2, 0.9 err^-0.2)), clipping onto the output times (a clipped accepted step does not change h), the linear
interpolation of sampled coefficients at ns > 1, `max_steps` and the NaN exit -- so that the kernel's step count (`K.info`) can be
compared with it exactly, not only its global error.  It takes a `dtype`: run in np.longdouble it shows how far fp64 rounding alone
moves the result (delta_case) and whether any accept / reject decision is close enough to err = 1 to flip (`margin`).

tests/test_riccati_ode_ref.py pins the restatement and admits the cases; tests/test_riccati_ode_steps_gpu.py runs the kernel on them."""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np


class OdeRun(NamedTuple):
    V: np.ndarray        # (N, n, n) in `dtype`: V at the output times linspace(0, T, N); NaN where the integration did not arrive
    info: int            # attempted steps, or -1 (max_steps exceeded) / -2 (NaN error estimate), as the kernel reports
    steps: int           # attempted steps (accepted + rejected)
    rejected: int
    margin: float        # min |err - 1| over all attempted steps: the distance of the closest accept / reject decision


def riccati_ode(A_s, B_s, Ri_s, Q_s, Qf, T, N, rtol=1.4e-8, atol=1.4e-8, max_steps=100000, dtype=np.float64) -> OdeRun:
    """ONE design: coefficient samples A_s (ns, n, n), B_s (ns, n, m), Ri_s (ns, m, m), Q_s (ns, n, n) at linspace(0, T, ns) (ns = 1:
    time-invariant), terminal value Qf (n, n), N output times."""
    D = dtype
    A_s, B_s, Ri_s, Q_s, y = (np.asarray(x, dtype=D) for x in (A_s, B_s, Ri_s, Q_s, Qf))
    ns, n = A_s.shape[0], A_s.shape[-1]
    T, rtol, atol = D(T), D(rtol), D(atol)
    fr = lambda p, q: D(p) / D(q)        # noqa: E731
    a21 = fr(1, 5)
    a31, a32 = fr(3, 40), fr(9, 40)
    a41, a42, a43 = fr(44, 45), fr(-56, 15), fr(32, 9)
    a51, a52, a53, a54 = fr(19372, 6561), fr(-25360, 2187), fr(64448, 6561), fr(-212, 729)
    a61, a62, a63, a64, a65 = fr(9017, 3168), fr(-355, 33), fr(46732, 5247), fr(49, 176), fr(-5103, 18656)
    b1, b3, b4, b5, b6 = fr(35, 384), fr(500, 1113), fr(125, 192), fr(-2187, 6784), fr(11, 84)
    e1, e3, e4 = fr(35, 384) - fr(1951, 21600), fr(500, 1113) - fr(22642, 50085), fr(125, 192) - fr(451, 720)
    e5, e6, e7 = fr(-2187, 6784) + fr(12231, 42400), fr(11, 84) - fr(649, 6300), fr(-1, 60)
    c2, c3, c4, c5 = fr(1, 5), fr(3, 10), fr(4, 5), fr(8, 9)

    S0 = (B_s[0] @ Ri_s[0]) @ B_s[0].T

    def coef(tau):
        if ns == 1:
            return A_s[0], S0, Q_s[0]
        u = tau / T * D(ns - 1)
        u = min(max(u, D(0)), D(ns - 1))
        i0 = min(int(u), ns - 2)
        w = u - D(i0)
        lerp = lambda X: X[i0] + w * (X[i0 + 1] - X[i0])        # noqa: E731
        B, Ri = lerp(B_s), lerp(Ri_s)
        return lerp(A_s), (B @ Ri) @ B.T, lerp(Q_s)

    def f(s, V):
        A, S, Q = coef(T - s)
        return (Q + V @ A + A.T @ V) - (V @ S) @ V

    def rms(v):
        return np.sqrt(np.sum(v * v) / D(n * n))

    V = np.full((N, n, n), np.nan, dtype=D)
    V[N - 1] = y
    if N == 1:
        return OdeRun(V, 0, 0, 0, np.inf)
    k1 = f(D(0), y)
    # first step (Hairer, Norsett, Wanner II.4)
    sc = atol + rtol * np.abs(y)
    d0, d1 = rms(y / sc), rms(k1 / sc)
    h0 = D(1e-6) if (d0 < 1e-5 or d1 < 1e-5) else D(0.01) * d0 / d1
    k2 = f(h0, y + h0 * k1)
    d2 = rms((k2 - k1) / sc) / h0
    dm = max(d1, d2)
    h1 = max(D(1e-6), h0 * D(1e-3)) if dm <= 1e-15 else np.power(D(0.01) / dm, D(0.2))
    h = min(D(100) * h0, h1)

    s = D(0)
    steps = rejected = 0
    margin = np.inf
    hgrid = T / D(N - 1)
    for j in range(1, N):
        s_end = T if j == N - 1 else D(j) * hgrid
        while s < s_end:
            steps += 1
            if steps > max_steps:
                return OdeRun(V, -1, steps, rejected, margin)
            hs = min(h, s_end - s)
            last = hs >= s_end - s
            k2 = f(s + c2 * hs, y + hs * (a21 * k1))
            k3 = f(s + c3 * hs, y + hs * (a31 * k1 + a32 * k2))
            k4 = f(s + c4 * hs, y + hs * (a41 * k1 + a42 * k2 + a43 * k3))
            k5 = f(s + c5 * hs, y + hs * (a51 * k1 + a52 * k2 + a53 * k3 + a54 * k4))
            k6 = f(s + hs, y + hs * (a61 * k1 + a62 * k2 + a63 * k3 + a64 * k4 + a65 * k5))
            yn = y + hs * (b1 * k1 + b3 * k3 + b4 * k4 + b5 * k5 + b6 * k6)
            k7 = f(s + hs, yn)
            e = hs * (e1 * k1 + e3 * k3 + e4 * k4 + e5 * k5 + e6 * k6 + e7 * k7)
            err = rms(e / (atol + rtol * np.maximum(np.abs(y), np.abs(yn))))
            if not (err == err):
                return OdeRun(V, -2, steps, rejected, margin)
            margin = min(margin, abs(float(err) - 1.0))
            if err <= 1:
                s = s_end if last else s + hs
                y, k1 = yn, k7
            else:
                rejected += 1
            fac = D(10) if err == 0 else min(D(10), max(D(1) if err < 1 else D(0.2), D(0.9) * np.power(err, D(-0.2))))
            if not (last and err <= 1 and fac >= 1):
                h = hs * fac
        V[N - 1 - j] = y
    return OdeRun(V, steps, steps, rejected, margin)


# ------------------------------------------------------------------------------------------------------------------------
# The cases.  Each is a dict: callables A, B, Q, R_inv of time returning (batch, ., .) arrays, Qf (batch, n, n), T, N and `ns`, the
# n_samples the GPU test passes to finiteHorizonLqr (1: time-invariant; > 1: coefficients piecewise linear in t with their kinks at
# the ns sample times, which the kernel's linear interpolation between the samples reproduces exactly, so the oracle can integrate
# the callables themselves).  `_ltv` is linear over the whole interval: any pair of samples extrapolates to the same line, so it
# cannot see which interval the kernel picks.  `_ltv_kinked` draws every sample afresh: a wrong interval gives other coefficients.
# Its sample times are output times (N - 1 a multiple of ns - 1): steps are clipped there, so the coefficients are smooth within
# every step, the pair keeps its order and the 2e-6 against DOP853 still holds (with kinks inside the steps a third of the steps
# is rejected and the global error reaches 3e-6).
BATCH = 2


def _lti(n, m, T, N, seed, qf=1.0, scale=0.5, stiff=False):
    rng = np.random.default_rng(seed)
    A = scale * rng.standard_normal((BATCH, n, n))
    if stiff:
        A = A - np.diag(np.logspace(-1, 2.5, n))
    B = rng.standard_normal((BATCH, n, m))
    Qf = qf * np.eye(n) + 0.1 * rng.standard_normal((BATCH, n, n))        # nonsymmetric: the formula as written, with a general V
    Q = np.broadcast_to(np.eye(n), (BATCH, n, n)).copy()
    Ri = np.broadcast_to(np.eye(m), (BATCH, m, m)).copy()
    return dict(A=lambda t: A, B=lambda t: B, Q=lambda t: Q, R_inv=lambda t: Ri, Qf=Qf, T=T, N=N, ns=1)


def _ltv(n, m, T, N, ns, seed):
    rng = np.random.default_rng(seed)
    A0, A1 = 0.5 * rng.standard_normal((2, BATCH, n, n))
    B0, B1 = rng.standard_normal((2, BATCH, n, m))
    Qc = np.broadcast_to(np.eye(n), (BATCH, n, n)).copy()
    Rc = np.broadcast_to(np.eye(m), (BATCH, m, m)).copy()
    Qf = np.eye(n) + 0.1 * rng.standard_normal((BATCH, n, n))
    return dict(A=lambda t: A0 + (t / T) * (A1 - A0), B=lambda t: B0 + (t / T) * (B1 - B0), Q=lambda t: (1.0 + t) * Qc,
                R_inv=lambda t: (2.0 - 0.5 * t) * Rc, Qf=Qf, T=T, N=N, ns=ns)


def _ltv_kinked(n, m, T, N, ns, seed):
    rng = np.random.default_rng(seed)
    A0 = 0.5 * rng.standard_normal((BATCH, n, n))
    B0 = rng.standard_normal((BATCH, n, m))
    A_s = A0 + 0.1 * rng.standard_normal((ns, BATCH, n, n))
    B_s = B0 + 0.2 * rng.standard_normal((ns, BATCH, n, m))
    M = rng.standard_normal((ns, BATCH, n, n))
    Q_s = np.eye(n) + 0.2 * M @ np.swapaxes(M, -1, -2) / n                     # SPD at the samples, so SPD in between
    M = rng.standard_normal((ns, BATCH, m, m))
    Ri_s = np.eye(m) + 0.2 * M @ np.swapaxes(M, -1, -2) / m
    Qf = np.eye(n) + 0.1 * rng.standard_normal((BATCH, n, n))

    def pl(X):
        def f(t):
            u = min(max(t / T * (ns - 1), 0.0), float(ns - 1))
            if abs(u - round(u)) < 1e-9:                                       # a sample time: the sample itself
                return X[int(round(u))]
            i0 = min(int(u), ns - 2)
            return X[i0] + (u - i0) * (X[i0 + 1] - X[i0])
        return f

    return dict(A=pl(A_s), B=pl(B_s), Q=pl(Q_s), R_inv=pl(Ri_s), Qf=Qf, T=T, N=N, ns=ns)


def _known_answer():
    I = np.broadcast_to(np.eye(2), (1, 2, 2)).copy()
    c = lambda t: I        # noqa: E731
    return dict(A=c, B=c, Q=c, R_inv=c, Qf=I, T=1.0, N=4, ns=1)


def _long_horizon():
    """(8, 4), A = 0.5 G - I, Q = R = I, Qf = I, T = 8: the closed loop's abscissa is below -1, so V(0) has converged to the CARE
    solution to exp(-2 * 8) ~ 1e-7, while the horizon is still short enough for the fp64 and long-double runs to take the same steps
    (at T = 40 they do not: 158 against 160)."""
    rng = np.random.default_rng(84)
    n, m = 8, 4
    A = 0.5 * rng.standard_normal((BATCH, n, n)) - np.eye(n)
    B = rng.standard_normal((BATCH, n, m))
    I, Im = np.broadcast_to(np.eye(n), (BATCH, n, n)).copy(), np.broadcast_to(np.eye(m), (BATCH, m, m)).copy()
    return dict(A=lambda t: A, B=lambda t: B, Q=lambda t: I, R_inv=lambda t: Im, Qf=I, T=8.0, N=9, ns=1)


CASES = {
    "known_answer_2x2": _known_answer,
    "full_tile_16x16": lambda: _lti(16, 16, 2.0, 9, seed=1616),
    "single_input_16x1": lambda: _lti(16, 1, 3.0, 5, seed=1601),
    "wide_3x7": lambda: _lti(3, 7, 2.0, 6, seed=307),
    "ragged_13x16": lambda: _lti(13, 16, 1.0, 3, seed=1316),
    "large_Qf_8x2": lambda: _lti(8, 2, 2.0, 7, seed=802, qf=1e3),
    "stiff_12x4": lambda: _lti(12, 4, 1.0, 6, seed=1204, stiff=True),
    "time_varying_6x2": lambda: _ltv(6, 2, 2.0, 9, 17, seed=602),
    "time_varying_16x16": lambda: _ltv(16, 16, 1.0, 5, 9, seed=1617),
    "kinked_6x2": lambda: _ltv_kinked(6, 2, 2.0, 9, 9, seed=603),             # a kink at every output time
    "kinked_16x16": lambda: _ltv_kinked(16, 16, 1.0, 9, 5, seed=1618),        # a kink at every other one
    "long_horizon_8x4": _long_horizon,
}
TOLERANCE_CASE = "large_Qf_8x2"      # rerun at rtol = atol in TOLERANCES
TOLERANCES = (1e-6, 1e-8, 1e-10)


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def samples(c):
    """The case's coefficient samples as the wrapper takes them with n_samples = c['ns']: (batch, ns, ., .) arrays."""
    ts = np.linspace(0.0, c["T"], c["ns"])
    return tuple(np.stack([np.asarray(c[k](float(t)), dtype=np.float64) for t in ts], axis=1) for k in ("A", "B", "R_inv", "Q"))


@functools.lru_cache(maxsize=None)
def runs(name, tol=1.4e-8, dtype=np.float64):
    """The restatement on every design of the case at rtol = atol = tol: a list of OdeRun."""
    c = case(name)
    A_s, B_s, Ri_s, Q_s = samples(c)
    return [riccati_ode(A_s[b], B_s[b], Ri_s[b], Q_s[b], c["Qf"][b], c["T"], c["N"], rtol=tol, atol=tol, dtype=dtype)
            for b in range(c["Qf"].shape[0])]


def delta_case(name, tol=1.4e-8):
    """max over the case's designs of max|V_fp64 - V_longdouble| / max|V_longdouble|: what fp64 rounding alone does to the result."""
    return max(float(np.max(np.abs(r64.V - rld.V)) / np.max(np.abs(rld.V)))
               for r64, rld in zip(runs(name, tol), runs(name, tol, np.longdouble)))
