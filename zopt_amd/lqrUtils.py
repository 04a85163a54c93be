"""Drop-in for ``zopt.lqrUtils`` (hot-path functions), running on MI355X HIP kernels.

Same names, positional arguments and return shapes as the reference; arrays may carry extra
LEADING batch axes (new).  NumPy in -> NumPy out; torch ROCm tensors in -> torch ROCm tensors out
(asynchronous on the current stream).
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _arrays as arr
from . import _lib

try:
    import torch
except Exception:  # pragma: no cover
    torch = None


def _check_operands(rows, lead, N=None):
    """`rows`: (name, array, tail).  Without `N` an operand has exactly the shape lead + tail; with a horizon `N` it is time-indexed,
    lead + (T,) + tail with T >= N (a longer one gets the carry step of `_carry_step`)."""
    for name, X, tail in rows:
        s, k = arr.shape(X), len(lead)
        if N is None:
            if s != lead + tail:
                raise ValueError(f"{name} has shape {s}, expected {lead + tail}")
        elif len(s) != k + 1 + len(tail) or s[:k] != lead or s[k + 1:] != tail or s[k] < N:
            raise ValueError(f"{name} has shape {s}, expected {lead + ('>=N',) + tail} with N={N}")


def _carry_step(dev, fills, ax, N):
    """The reference scans the first N steps but starts from the carry (Q[-1], ...) of the WHOLE arrays (lqrUtils.py:172, :261).  The
    kernels take the last step's cost as terminal value, so operands longer than N get one extra step along the time axis `ax` that
    hands that carry to step N-1 and returns a zero gain: per operand `fills` names it -- "zero", "last" (the array's last step) or
    "eye".  -> (operands, number of steps the kernel runs); the caller trims the extra step off the outputs (`_first_steps`)."""
    if all(t.shape[ax] == N for t in dev):
        return dev, N

    def extra(t, fill):
        if fill == "last":
            return t.narrow(ax, t.shape[ax] - 1, 1)
        if fill == "eye":
            return torch.eye(t.shape[-1], dtype=t.dtype, device=t.device).expand(tuple(t.shape[:ax]) + (1,) + tuple(t.shape[-2:]))
        return torch.zeros_like(t.narrow(ax, 0, 1))

    return [torch.cat([t.narrow(ax, 0, N), extra(t, fill)], ax).contiguous() for t, fill in zip(dev, fills)], N + 1


def _first_steps(outs, ax, N):
    return [t if t.shape[ax] == N else t.narrow(ax, 0, N).contiguous() for t in outs]


def _call(who, entry, batch, *args):
    """The C entry `entry` on the current stream of its first operand's device, unless the batch is empty; a refusal raises as `who`."""
    if batch:
        ptrs = [a.data_ptr() if arr.is_torch(a) else a for a in args]
        _lib.check(getattr(_lib.lib(), entry)(*ptrs, ctypes.c_void_p(arr.stream_ptr(args[0]))), who)


def _like(template, *outs):
    """The outputs in the caller's array family and precision: the entries compute in fp64, an fp32 caller gets fp32 back."""
    if arr.is_fp32(template):
        outs = [t.to(torch.float32) if t.is_floating_point() else t for t in outs]
    return [arr.result_like(t, template) for t in outs]


def discreteFiniteHorizonLqr(A, B, Q, R, N):
    """Finite-horizon discrete LQR gains by backward Riccati recursion (reference lqrUtils.py:144-173).

    ```
    J = sum_k(x^T Q x + u^T R u);   xNew = A x + B u;   uLqr = -L x
    ```

    Arguments
    ---------
        A : (..., N, n, n) state matrices, time along axis -3: `A[k]`
        B : (..., N, n, m)
        Q : (..., N, n, n)   (terminal value is `Q[-1]`, as in the reference, lqrUtils.py:172)
        R : (..., N, m, m)
        N : horizon

    Returns
    -------
        L : (..., N, m, n) optimal gains `L[k]`
    """
    shp = arr.shape(B)
    if len(shp) < 3:
        raise ValueError("B must have shape (..., N, n, m)")
    lead, (n, m) = shp[:-3], shp[-2:]
    _check_operands((("A", A, (n, n)), ("B", B, (n, m)), ("Q", Q, (n, n)), ("R", R, (m, m))), lead, N)
    if N < 1:
        raise ValueError("N must be >= 1")
    # dtype follows the input arrays (quirk Q8).  fp32 inputs go to zm_lqr_backward_f32 as they are: the fast-path shapes (n in {8, 12},
    # m = 4) run K1 on fp32 storage with fp64 arithmetic, larger ones (n <= 64, m <= 16) the fp32 MFMA tile kernel; the remaining small
    # shapes are computed in fp64 on the tile-16 kernel and rounded once on output.
    native32 = arr.is_fp32(A) and (n > 12 or m > 4 or ((n in (8, 12)) and m == 4))
    dt = torch.float32 if native32 else torch.float64
    # the extra step of over-long inputs (A = 0, B = 0, Q = Q[-1], R = I) returns L = 0 and hands V = Q[-1] to step N-1
    dev, Tk = _carry_step([arr.to_device(X, dt) for X in (A, B, Q, R)], ("zero", "zero", "last", "eye"), len(lead), N)
    batch = arr.batch(lead)
    dL = torch.empty(lead + (Tk, m, n), dtype=dt, device=dev[0].device)
    _call("discreteFiniteHorizonLqr", "zm_lqr_backward_f32" if native32 else "zm_lqr_backward_f64", batch, *dev, dL, batch, Tk, n, m)
    return _like(A, *_first_steps([dL], len(lead), N))[0]


def discreteInfiniteHorizonLqr(A, B, Q, R, tol=1e-14, maxIter=200000, return_value=False):
    """Discrete-time infinite-horizon LQR gains (reference lqrUtils.py:176-204: SciPy `solve_discrete_are` + one solve).

    ```
    J = sum_k(x^T Q x + u^T R u);   xNew = A x + B u;   uLqr = -L x
    ```
    Here: Riccati value iteration from V = Q on the GPU, one wave per system, until `max|V' - V| <= tol * max|V'|`.
    Accuracy: the fixed point is SciPy's stabilising solution for stabilizable / detectable designs (tested to 1e-10 against
    `solve_discrete_are`); value iteration converges linearly at the closed loop's spectral radius squared, so marginally
    stabilizable designs need many iterations.  Like SciPy (`LinAlgError`), a design whose iteration has not converged within
    `maxIter` steps or whose gain is not finite (not stabilizable) raises `numpy.linalg.LinAlgError` instead of returning a
    non-stationary gain (with `return_value=True` nothing is raised: the caller gets `iterations` and decides).

    Arguments
    ---------
        A : (..., n, n)    B : (..., n, m)    Q : (..., n, n)    R : (..., m, m)     (n <= 64, m <= 16: the tile-16 register
            kernel up to n <= 12, m <= 4, the fp64 MFMA tile kernel on time-invariant operands beyond; both stop when the VALUE no
            longer changes, `max|V' - V| <= tol max|V'|`)

    Returns
    -------
        L : (..., m, n) optimal LQR gains `u = -L x`   (with `return_value=True`: (L, V, iterations), iterations < 0 where the
            cap ended the iteration before its stopping test was met)
    """
    def failed(its, dL, batch):
        if return_value:      # the caller receives `iterations` and judges convergence itself
            return
        # the kernel reports convergence explicitly (iters < 0: the cap ended the loop); a design that meets the tolerance exactly on
        # its last allowed iteration is converged
        bad = (its.reshape(-1) <= 0) | ~torch.isfinite(dL.reshape(batch, -1)).all(dim=1)
        nbad = int(bad.sum())
        if nbad:   # SciPy's solve_discrete_are raises LinAlgError('Failed to find a finite solution.') there (lqrUtils.py:202)
            raise np.linalg.LinAlgError(f"discreteInfiniteHorizonLqr: no converged finite solution for {nbad} of {batch} designs "
                                        f"within maxIter={int(maxIter)} (not stabilizable, or increase maxIter)")

    return _riccati_design("discreteInfiniteHorizonLqr", "zm_dare_f64", A, B, Q, R, tol, maxIter, return_value, symmetric=False,
                           status=torch.empty, failed=failed)


def _check_symmetric(name, X):
    """scipy.linalg.solve_continuous_are rejects nonsymmetric q / r with a ValueError (its _are_validate_args)."""
    if X.numel() and float((X - X.transpose(-1, -2)).abs().max()) > 100 * np.finfo(np.float64).eps * max(float(X.abs().max()), 1.0):
        raise ValueError(f"Matrix {name} should be symmetric/hermitian.")


def _riccati_design(who, entry, A, B, Q, R, tol, maxIter, return_value, symmetric, status, failed):
    """The two algebraic Riccati designs: four operands of exact shape uploaded as fp64, a gain, a value and an int32 status per design
    (`status`: how it is allocated), `entry(..., tol, maxIter)`, `failed(status, gain, batch)` raising LinAlgError where the entry's
    status says so, the outputs in the caller's precision.  `symmetric`: Q and R must be symmetric, as SciPy's CARE solver demands."""
    shp = arr.shape(B)
    if len(shp) < 2:
        raise ValueError("B must have shape (..., n, m)")
    lead, (n, m) = shp[:-2], shp[-2:]
    _check_operands((("A", A, (n, n)), ("B", B, (n, m)), ("Q", Q, (n, n)), ("R", R, (m, m))), lead)
    dt = torch.float64
    dA, dB, dQ, dR = [arr.to_device(X, dt) for X in (A, B, Q, R)]
    if symmetric:
        _check_symmetric("q", dQ)
        _check_symmetric("r", dR)
    batch = arr.batch(lead)
    dK = torch.empty(lead + (m, n), dtype=dt, device=dA.device)
    dP = torch.empty(lead + (n, n), dtype=dt, device=dA.device)
    info = status(lead, dtype=torch.int32, device=dA.device)
    _call(who, entry, batch, dA, dB, dQ, dR, dK, dP, info, batch, n, m, float(tol), int(maxIter))
    if batch:
        failed(info, dK, batch)
    outs = _like(A, *((dK, dP, info) if return_value else (dK,)))
    return tuple(outs) if return_value else outs[0]


def infiniteHorizonLqr(A, B, Q, R, tol=1e-14, maxIter=60, return_value=False):
    """Continuous-time infinite-horizon LQR gains (reference lqrUtils.py:13-36: SciPy `solve_continuous_are` + one solve).

    ```
    J = int_t(x^T Q x + u^T R u);   xDot = A x + B u;   uLqr = -K x
    ```
    Here: the stabilising solution of the algebraic Riccati equation by the structure-preserving doubling algorithm on the GPU,
    one wave per design (quadratically convergent: ~10 doubling steps, `maxIter` caps them), followed by one or two Newton-Kleinman
    steps on the Riccati residual formed through `K` (the doubling iteration forms `G = B R^-1 B^T` and inverts `I + G H`, which
    under cheap control, `R = r I` with small r, costs up to eight digits of `P`; the Newton step restores them); `K = R^-1 B^T P`.
    Accuracy (tests/test_care_hard_gpu.py: 142 hard designs -- unreachable slow and barely detectable / stabilisable modes, cheap
    control down to r = 1e-8, expensive control, badly scaled and stiff systems, integrator chains, light oscillators -- at six
    shapes up to 16 x 16, against a Newton-refined long-double solution): every design within max(1e-10, 100 x SciPy's own error)
    in `P` and in `K`; measured on an MI355X (profiles/care_hard_spectrum.txt): the worst design at 0.4 % of that bound, the error
    relative to max|P| at most 3e-15 in `P` in every family but the stiff one (9e-13, SciPy 1e-9), and in `K` at most 4e-11 (cheap
    control at r = 1e-8, SciPy 2e-8; 5e-12 at r = 1e-6, below 1e-12 elsewhere but for stiff, 3e-12) -- each family's worst at or below
    SciPy's worst on it.  Without the Newton-Kleinman steps the doubling iteration alone was up to 3e-6 off under cheap control.
    Against SciPy's Schur-based solver on random designs (tools/fuzz_care.py, 1272 designs, n <= 16) the median deviation is 1e-14.
    Designs without a finite stabilising solution raise `numpy.linalg.LinAlgError` as SciPy does.

    Arguments
    ---------
        A : (..., n, n)    B : (..., n, m)    Q : (..., n, n)    R : (..., m, m)     (n <= 16, m <= 16; Q, R symmetric)

    Returns
    -------
        K : (..., m, n) LQR gains   (with `return_value=True`: (K, P, doubling steps))
    """
    def failed(info, dK, batch):
        if int(info.min()) < 0:    # SciPy: LinAlgError('Failed to find a finite solution.')
            raise np.linalg.LinAlgError("infiniteHorizonLqr: failed to find a finite stabilising solution "
                                        f"({int((info < 0).sum())} of {batch} designs)")

    return _riccati_design("infiniteHorizonLqr", "zm_care_f64", A, B, Q, R, tol, maxIter, return_value, symmetric=True,
                           status=torch.ones, failed=failed)


def infiniteHorizonIntegralLqr(A, B, Q, R, Qi, Ci):
    """Infinite-horizon LQR with integral states (reference lqrUtils.py:101-141).

    ```
    J = int_t(z^T Q_i z + x^T Q x + u^T R u);   zDot = C_i x;   xDot = A x + B u
    ```
    The integral-augmented system `[[0, Ci], [0, A]]`, `[[0], [B]]`, `blkdiag(Qi, Q)` (:129-132) goes through `infiniteHorizonLqr`.

    Arguments
    ---------
        A : (..., n, n)   B : (..., n, m)   Q : (..., n, n)   R : (..., m, m)   Qi : (..., ni, ni)
        Ci : (..., ni, n)  -- or (..., n) for a single integral state, as the reference's own test passes it     (ni + n <= 16)

    Returns
    -------
        Ki : (..., m, ni) integral gains      Kp : (..., m, n) proportional gains
    """
    dt = torch.float64
    dA, dB, dQ, dR, dQi, dCi = [arr.to_device(X, dt) for X in (A, B, Q, R, Qi, Ci)]
    if dB.dim() < 2 or dQi.dim() < 2:
        raise ValueError("B must have shape (..., n, m) and Qi (..., ni, ni)")
    n, m = dB.shape[-2:]
    ni = dQi.shape[-1]
    lead = tuple(dB.shape[:-2])
    if dCi.dim() == len(lead) + 1:       # np.block promotes a 1-D Ci to one row (:129)
        dCi = dCi.unsqueeze(-2)
    _check_operands((("A", dA, (n, n)), ("Q", dQ, (n, n)), ("R", dR, (m, m)), ("Qi", dQi, (ni, ni)), ("Ci", dCi, (ni, n))), lead)
    z = lambda r, c: torch.zeros(lead + (r, c), dtype=dt, device=dA.device)
    Aw = torch.cat([torch.cat([z(ni, ni), dCi], -1), torch.cat([z(n, ni), dA], -1)], -2)
    Bw = torch.cat([z(ni, m), dB], -2)
    Qw = torch.cat([torch.cat([dQi, z(ni, n)], -1), torch.cat([z(n, ni), dQ], -1)], -2)
    K = infiniteHorizonLqr(Aw.contiguous(), Bw.contiguous(), Qw.contiguous(), dR)
    return arr.result_like(K[..., :, :ni].contiguous(), A), arr.result_like(K[..., :, ni:].contiguous(), A)


class _GainSchedule:
    """`K(t) = R_inv(t) @ B(t).T @ V(t)` with V linearly interpolated between the N grid values, clipped at the ends
    (reference lqrUtils.py:94-97, jaxUtils.py:7-24).  `t`, `V` hold the grid (N,) and the value function (..., N, n, n)."""

    def __init__(self, t, V, B, R_inv, T):
        self.t, self.V, self._B, self._Ri, self._T = t, V, B, R_inv, float(T)

    def value(self, tq):
        N = self.V.shape[-3]
        if N == 1:
            return self.V[..., 0, :, :]
        u = min(max(float(tq) / self._T, 0.0), 1.0) * (N - 1)
        i0 = min(int(u), N - 2)
        w = u - i0
        return self.V[..., i0, :, :] + w * (self.V[..., i0 + 1, :, :] - self.V[..., i0, :, :])

    def __call__(self, tq):
        B, Ri = self._B(tq), self._Ri(tq)
        V = self.value(tq)
        if arr.is_torch(V):
            B, Ri = arr.to_device(B, V.dtype, V.device), arr.to_device(Ri, V.dtype, V.device)
            return Ri @ B.transpose(-1, -2) @ V
        return np.asarray(Ri) @ np.swapaxes(np.asarray(B), -1, -2) @ V


def finiteHorizonLqr(A, B, Q, R_inv, Qf, T, N=50, n_samples=None, rtol=1.4e-8, atol=1.4e-8, max_steps=100000, coef_rtol=1e-6,
                     max_refinements=7):
    """Continuous-time finite-horizon LQR gains by integrating the LQR Hamilton-Jacobi-Bellman (Riccati) equation
    (reference lqrUtils.py:39-98).

    ```
    J = xf^T Qf xf + int_t(x^T Q x + u^T R u);   xDot = A x + B u;   uLqr = -K(t) x
    ```
    Here: `dV/dt = -Q + V B R_inv B^T V - V A - A^T V` backwards from `V(T) = Qf` on the GPU, one wave per design, with the
    adaptive Dormand-Prince 5(4) pair and tolerances of `jax.experimental.ode.odeint` (the reference's integrator), stepping
    exactly onto the output times `linspace(0, T, N)`.  The coefficient callables are host Python (the reference evaluates them
    inside the integrator's right-hand side): they are sampled at `linspace(0, T, n_samples)` and the kernel interpolates linearly
    in between -- exact for time-invariant coefficients (the reference's demos and tests; a single sample then) and for
    piecewise-linear ones.  For other time-varying coefficients the sampling is REFINED until it no longer matters: starting
    from `8 (N - 1) + 1` samples the spacing is halved (interpolation error / 4 each time) until the value function changes by
    less than `coef_rtol * max|V|` between two refinements (default 1e-6: the level at which two runs of the adaptive integrator
    differ anyway), at most `max_refinements` times (`K.n_samples` / `K.coef_change`
    report what was reached).  An explicit `n_samples` switches the refinement off.

    Arguments
    ---------
        A, B, Q, R_inv : callables of time returning (..., n, n), (..., n, m), (..., n, n), (..., m, m)      (n <= 16, m <= 16)
        Qf : (..., n, n) terminal state cost matrix
        T : time horizon;  N : number of output times

    Returns
    -------
        K : callable `K(t)` -> (..., m, n);  `K.t` (N,) and `K.V` (..., N, n, n) expose the integrated value function
    """
    T = float(T)
    N = int(N)
    if not (T > 0.0) or N < 1:
        raise ValueError("T must be > 0 and N >= 1")
    ns0 = int(n_samples) if n_samples is not None else 8 * (N - 1) + 1
    if ns0 < 1:
        raise ValueError("n_samples must be >= 1")
    dt = torch.float64
    dev = arr.to_device(Qf, dt).device
    dQf = arr.to_device(Qf, dt, dev).contiguous()

    def integrate(ns):
        ts = np.linspace(0.0, T, ns)

        def sample(f):
            vals = [arr.to_device(f(float(tk)), dt, dev) for tk in ts]
            if all(v.shape == vals[0].shape and bool((v == vals[0]).all()) for v in vals[1:]):
                vals = vals[:1]           # time-invariant
            return vals

        sA, sB, sQ, sRi = sample(A), sample(B), sample(Q), sample(R_inv)
        cnt = max(len(sA), len(sB), len(sQ), len(sRi))
        stack = lambda v: torch.stack(v if len(v) == cnt else v * cnt, dim=-3).contiguous()
        dA, dB, dQ, dRi = stack(sA), stack(sB), stack(sQ), stack(sRi)
        if dB.dim() < 3:
            raise ValueError("B(t) must have shape (..., n, m)")
        n, m = dB.shape[-2:]
        lead = tuple(dB.shape[:-3])
        # every stack holds `cnt` samples along axis -3: the shapes of one sample are what is checked and reported
        _check_operands((("A(t)", dA[..., 0, :, :], (n, n)), ("Q(t)", dQ[..., 0, :, :], (n, n)), ("R_inv(t)", dRi[..., 0, :, :], (m, m)),
                         ("Qf", dQf, (n, n))), lead)
        batch = arr.batch(lead)
        dV = torch.empty(lead + (N, n, n), dtype=dt, device=dev)
        info = torch.ones(lead, dtype=torch.int32, device=dev)
        _call("finiteHorizonLqr", "zm_riccati_ode_f64", batch, dA, dB, dRi, dQ, dQf, dV, info, batch, n, m, cnt, N, T, float(rtol),
              float(atol), int(max_steps))
        return dV, info, cnt

    ns = ns0
    dV, info, cnt = integrate(ns)
    change = 0.0
    if n_samples is None and cnt > 1 and dV.numel():
        # time-varying coefficients: halve the sample spacing until the linear interpolation no longer shows in V
        for _ in range(int(max_refinements)):
            ns = 2 * (ns - 1) + 1
            dV2, info2, _ = integrate(ns)
            fin = torch.isfinite(dV2) & torch.isfinite(dV)
            scale = float(dV2[fin].abs().max()) if bool(fin.any()) else 0.0
            change = float((dV2 - dV)[fin].abs().max()) if bool(fin.any()) else 0.0
            dV, info = dV2, info2
            if change <= float(coef_rtol) * max(scale, 1e-300):
                break
    K = _GainSchedule(np.linspace(0.0, T, N), arr.result_like(dV, Qf), B, R_inv, T)
    K.info = arr.result_like(info, Qf)
    K.n_samples = ns if cnt > 1 else 1
    K.coef_change = change
    return K


def bilinearAffineLqr(A, B, d, Q, R, H, q, r, q0, N):
    """Finite Horizon LQR with bilinear cost and affine dynamics (reference lqrUtils.py:207-262).

    Arguments
    ---------
        A : (..., N, n, n)    B : (..., N, n, m)    d : (..., N, n)
        Q : (..., N, n, n)    R : (..., N, m, m)    H : (..., N, m, n)
        q : (..., N, n)       r : (..., N, m)       q0 : (..., N)   (does not influence the gains, accepted for parity)
        N : horizon depth

    Returns
    -------
        L : (..., N, m, n) optimal lqr gains `L[k]`
        l : (..., N, m) optimal lqr offsets `l[k]`          (law `u = -L x - l`, demos/bilinearLqrControl.py:14)
    """
    shp = arr.shape(B)
    if len(shp) < 3:
        raise ValueError("B must have shape (..., N, n, m)")
    lead, (n, m) = shp[:-3], shp[-2:]
    spec = (("A", A, (n, n)), ("B", B, (n, m)), ("d", d, (n,)), ("Q", Q, (n, n)), ("R", R, (m, m)), ("H", H, (m, n)),
            ("q", q, (n,)), ("r", r, (m,)))
    _check_operands(spec, lead, N)
    if N < 1:
        raise ValueError("N must be >= 1")
    dt = torch.float64
    # the extra step of over-long inputs (A = B = d = H = r = 0, Q = Q[-1], q = q[-1], R = I) reproduces the carry (Q[-1], q[-1])
    dev, Tk = _carry_step([arr.to_device(X, dt) for name, X, tail in spec],
                          ("zero", "zero", "zero", "last", "eye", "zero", "last", "zero"), len(lead), N)
    batch = arr.batch(lead)
    dL = torch.empty(lead + (Tk, m, n), dtype=dt, device=dev[0].device)
    dl = torch.empty(lead + (Tk, m), dtype=dt, device=dev[0].device)
    _call("bilinearAffineLqr", "zm_lqr_backward_affine_f64", batch, *dev, dL, dl, batch, Tk, n, m)
    return tuple(_like(A, *_first_steps([dL, dl], len(lead), N)))


def proportionalFeedbackController(x, x0, u0, K):
    """`u = -K (x - x0) + u0` (reference lqrUtils.py:266-269); no controller states."""
    control = -K @ (x - x0) + u0
    dxCtrl = np.array([])
    return control, dxCtrl
