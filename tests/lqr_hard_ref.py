"""Cases, reference, bounds and checker of the hard-family tests of `discreteFiniteHorizonLqr` (tests/test_lqr_hard.py on the CPU,
tests/test_lqr_hard_gpu.py on the GPU).

Reference   `hp.finite_horizon_ld`: the oracle's Joseph-form recursion in long double.
Metric      `hp.sweep_metric`: per trajectory and per step, max|L_k - ref_k| over the largest gain of that trajectory.
fp64 bound  `hp.sweep_bounds(e_case, e_plain)` = 100 x max(the fp64 oracle's error on the case, its error on `plain` at the same shape,
            horizon and batch): the rule and the margin of the sweeps' hard tests.  Nothing here comes from a kernel.
fp32        K1 on fp32 storage (fp64 arithmetic, rounded once): |L - L_ld| <= 0.5 ulp32(L_ld) + bound64 * scale, L_ld the long-double
            result on the fp32-rounded inputs.  The fp32 tile kernel: 100 x max(case, plain) of the error of NumPy's fp32 recursion
            against that L_ld; only the families whose yardstick stays below 1e-3 run (`tile32_families`).

`input_units` is compared after undoing its units (E^-1 L' D, exact: powers of two), reference and oracle error included, so the
small rows of L' are held at their own scale.

The predictions of which steps leave the fast m x m solve come from CPU models: `guard_ratio` (tools/k1_solve_model.py, K1's
cofactor solve and its residual guard) and `growth` (the elimination without row exchanges of the register and tile kernels).
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

from oracle import zopt_oracle as zo
from tests import hp_reference as hp
from tests import problems
from tools import k1_solve_model as km

LD = np.longdouble
FAMILIES = tuple(problems.HARD_LQR)
# the nine families of the issue's table, one trajectory each in the mixed batch (`dominant_input` at r = 1: it mixes both solves)
MIXED = tuple(f for f in FAMILIES if f != "dominant_input_1e-2")

K1_SHAPES = [(12, 4), (8, 4)]
K1_T = [1, 2, 3, 4, 7, 11]                 # every phase of the DMA ring, and a horizon that is no multiple of its depth
K1_T_F32 = [1, 2, 7, 11]
REG_SPECIAL_T = [1, 2, 3, 4, 7]            # the specialised register kernel at the K1 shapes (operands the ring refuses)
REG_SHAPES = [(4, 1), (1, 1), (3, 4), (5, 2), (7, 3), (9, 1), (11, 4), (12, 3)]       # (4, 1) specialised; generic KS = 1, 2, 3
REG_T = [1, 2, 5]
TILE_SHAPES = [(5, 9), (16, 16), (13, 3), (24, 8), (33, 7), (48, 16), (49, 5), (64, 16)]   # 1 .. 4 tile rows, edges and interiors
TILE_T = [1, 2, 6]
TILE_BATCH = 3
CHILD_SHAPES = {"lds": [(13, 3), (24, 8), (64, 16)], "reg": [(12, 4)]}                # ZOPT_AMD_LQR_PATH = lds / reg
CHILD_T = [1, 6]
BATCH = 5

ORACLE_LIMIT = 1e-9         # a case whose fp64 oracle error exceeds this is rejected: its bound would no longer discriminate
YARDSTICK32_LIMIT = 1e-3    # the fp32 tile kernel runs the families whose fp32 yardstick stays below this
FIRES, ADMITS = 8.0, 1.0 / 8.0     # margins of the guard predictions on the residual ratio (the guard's own threshold is 1)


def _T(X):
    return np.swapaxes(X, -1, -2)


def undo_units(L, name):
    """E^-1 L D for `input_units` (exact), L itself for every other family.  L (..., m, n)."""
    if name != "input_units":
        return L
    d, e = problems.lqr_units(L.shape[-1], L.shape[-2])
    return L * d.astype(L.dtype)[None, :] / e.astype(L.dtype)[:, None]


def _batch(n, m):
    return TILE_BATCH if (n > 12 or m > 4) else BATCH


@functools.lru_cache(maxsize=None)
def case(name, n, m, T, batch=None, storage="f64"):
    """One seeded case: .args (A, B, Q, R) in fp64 (storage "f32": fp32 arrays), .ref the long-double gains on exactly those numbers
    (units undone), .scale (batch,) each trajectory's largest reference gain, .e_case / .e_plain the fp64 oracle's `sweep_metric`
    maxima on the case and on `plain`, .bound = `hp.sweep_bounds` of the two."""
    batch = _batch(n, m) if batch is None else batch
    args = problems.hard_lqr(name, n, m, T, batch)
    if storage == "f32":
        args = tuple(X.astype(np.float32) for X in args)
    a64 = tuple(X.astype(np.float64) for X in args)
    ref = undo_units(hp.finite_horizon_ld(*a64, T), name)
    e_case = float(hp.sweep_metric(undo_units(zo.discreteFiniteHorizonLqr(*a64, T), name), ref).max())
    e_plain = e_case if name == "plain" else case("plain", n, m, T, batch, storage).e_case
    scale = np.max(np.abs(ref), axis=(1, 2, 3)).astype(np.float64)
    c = SimpleNamespace(name=name, n=n, m=m, T=T, batch=batch, storage=storage, args=args, ref=ref, scale=scale, e_case=e_case,
                        e_plain=e_plain, bound=hp.sweep_bounds(e_case, e_plain))
    if storage == "f32":
        # the fp32 tile kernel's yardstick: NumPy's fp32 recursion on the same fp32 arrays
        with np.errstate(all="ignore"):
            try:
                L32 = zo.discreteFiniteHorizonLqr(*args, T)
                c.e32_case = float(np.nan_to_num(hp.sweep_metric(undo_units(L32, name), ref), nan=np.inf).max())
            except np.linalg.LinAlgError:
                c.e32_case = np.inf
        c.e32_plain = c.e32_case if name == "plain" else case("plain", n, m, T, batch, storage).e32_case
        c.bound32 = hp.sweep_bounds(c.e32_case, c.e32_plain)
    return c


def tile32_families(n, m, T):
    """The families the fp32 tile kernel is held to at (n, m, T): those whose fp32 yardstick stays below YARDSTICK32_LIMIT."""
    return [f for f in FAMILIES if case(f, n, m, T, storage="f32").e32_case <= YARDSTICK32_LIMIT]


def _fail(what, c, err, bound):
    b, k = np.unravel_index(int(np.argmax(np.nan_to_num(err, nan=np.inf))), err.shape)
    raise AssertionError(f"{what}: {c.name} (n, m, T) = ({c.n}, {c.m}, {c.T}) trajectory {b} step {k}: {err[b, k]:.3e} > bound {bound:.3e} "
                         f"(oracle error {c.e_case:.2e}, on plain {c.e_plain:.2e})")


def check_gains(L, c, bound=None):
    """Hold the fp64 gains L (batch, T, m, n) of case c to its bound on every trajectory and step.  Returns the largest error."""
    L = np.asarray(L)
    assert L.shape == c.ref.shape, (L.shape, c.ref.shape)
    bound = c.bound if bound is None else bound
    err = hp.sweep_metric(undo_units(L, c.name), c.ref)
    if not (np.all(np.isfinite(L)) and np.all(err <= bound)):
        _fail("gains", c, err, bound)
    return float(err.max())


def check_gains_f32_storage(L, c):
    """K1 on fp32 storage: fp64 arithmetic rounded once, so within half an fp32 ulp of the long-double result on the same fp32 inputs,
    plus the case's fp64 bound.  Returns the largest excess over the half ulp, in units of the trajectory's scale."""
    assert c.storage == "f32" and L.dtype == np.float32 and L.shape == c.ref.shape
    Lu = undo_units(L, c.name).astype(LD)
    ulp = np.spacing(np.abs(c.ref).astype(np.float32)).astype(LD)
    excess = ((np.abs(Lu - c.ref) - 0.5 * ulp) / c.scale[:, None, None, None].astype(LD)).astype(np.float64).max(axis=(2, 3))
    if not (np.all(np.isfinite(L)) and np.all(excess <= c.bound)):
        _fail("fp32-storage gains beyond half an ulp", c, excess, c.bound)
    return float(excess.max())


def check_gains_f32_tile(L, c):
    """The fp32 tile kernel against 100 x NumPy's fp32 recursion.  Returns (largest error, its ratio to the yardstick)."""
    assert c.storage == "f32" and L.dtype == np.float32
    check_gains(L, c, bound=c.bound32)
    err = float(hp.sweep_metric(undo_units(L, c.name), c.ref).max())
    return err, err / max(c.e32_case, c.e32_plain)


# ------------------------------------------------------------------------------------------------------------------ the CPU models
def guard_ratio(args):
    """K1's model on every step of an m = 4 case: the residual ratio of the cofactor solve (batch, T); the guard fires above 1."""
    Suu, Sux = km.riccati_blocks(*(np.asarray(X, np.float64) for X in args))
    return km.cofactor_solve(Suu, Sux, details=True)[2]


def growth(Suu):
    """The elimination WITHOUT row exchanges on (..., m, m), as the register and tile kernels run it: returns (the largest multiplier,
    the largest sum over a column of the squared multipliers).  The kernels abandon it above 4 (register kernel, fp64 tile kernel)
    or above 16 (fp32 tile kernel, squared sum).  A zero pivot gives inf."""
    S = np.array(Suu, dtype=np.float64)
    m = S.shape[-1]
    big, sq = np.zeros(S.shape[:-2]), np.zeros(S.shape[:-2])
    with np.errstate(all="ignore"):
        for k in range(m - 1):
            f = S[..., k + 1:, k] / S[..., k, k, None]
            f = np.where(np.isnan(f), np.inf, f)
            big = np.maximum(big, np.max(np.abs(f), axis=-1))
            sq = np.maximum(sq, np.sum(f * f, axis=-1))
            S[..., k + 1:, :] -= f[..., None] * S[..., k, None, :]
    return big, sq


def growth_of(args):
    """`growth` on every step of a case: two (batch, T) arrays."""
    return growth(km.riccati_blocks(*(np.asarray(X, np.float64) for X in args))[0])


# ------------------------------------------------------------------------------------------------- fp64 evaluations, honest and planted
def riccati64(A, B, Q, R, T, solve=np.linalg.solve, reorder=False, value="joseph", symmetrise_Q=False, trace=None):
    """The recursion in fp64 with the m x m solve, the order of the products and the value update exchangeable:
    reorder: B^T (V B) and B^T (V A) in place of (B^T V) B, (B^T V) A (an honest evaluation);
    value "schur": V' = Q + A^T V A - Sux^T L in place of the Joseph form;  symmetrise_Q: (Q + Q^T) / 2 in place of Q;
    trace: a list that receives max|V| (batch,) after every update, k = T-1 first."""
    A, B, Q, R = (np.asarray(X, np.float64) for X in (A, B, Q, R))
    if symmetrise_Q:
        Q = (Q + _T(Q)) / 2
    V = Q[:, T - 1]
    L = np.empty(B.shape[:1] + (T,) + (B.shape[-1], B.shape[-2]))
    for k in range(T - 1, -1, -1):
        Ak, Bk, Qk, Rk = A[:, k], B[:, k], Q[:, k], R[:, k]
        if reorder:
            Suu, Sux = Rk + _T(Bk) @ (V @ Bk), _T(Bk) @ (V @ Ak)
        else:
            Suu, Sux = Rk + (_T(Bk) @ V) @ Bk, (_T(Bk) @ V) @ Ak
        Lk = solve(Suu, Sux)
        if value == "schur":
            V = Qk + (_T(Ak) @ V) @ Ak - _T(Sux) @ Lk
        else:
            Acl = Ak - Bk @ Lk
            V = Qk + (_T(Lk) @ Rk) @ Lk + (_T(Acl) @ V) @ Acl
        L[:, k] = Lk
        if trace is not None:
            trace.append(np.abs(V).max(axis=(-2, -1)))
    return L


def cofactor_unguarded(Suu, Sux):
    """K1's cofactor solve with its guard taken out: the fast path's result whatever the residual says."""
    return km.cofactor_solve(Suu, Sux, details=True)[3]


def nopivot_unchecked(Suu, Sux):
    """The 4 x 4 elimination without row exchanges with its growth check taken out."""
    return km.nopivot_solve(Suu, Sux, details=True)[2]
