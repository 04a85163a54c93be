"""`discreteFiniteHorizonLqr` on the GPU, every path, against the long-double recursion on the hard families of `problems.HARD_LQR`
(cases, bounds and checker: tests/lqr_hard_ref.py; their CPU proofs: tests/test_lqr_hard.py).

Per trajectory and per step, bound = 100 x the fp64 oracle's own error (about 1e-13 on the well-conditioned families).  The families
`input_units`, `dominant_input*` leave K1's cofactor solve for the pivoted re-solve on steps the CPU model predicts with margin;
`permuted_R` and `dominant_input*` leave the unpivoted elimination of the register and tile kernels.  The product library counts
neither, so that prediction is the evidence that the branch ran, and the bound is what holds its result.

    path                                   reached by                                       test
    K1 ring, fp64                          aligned fp64 arrays at (12, 4), (8, 4)           test_k1_ring_fp64
    K1 ring, fp32 storage                  fp32 arrays there                                test_k1_ring_fp32_storage
    register kernel, specialised           A 8 bytes off a 16-byte boundary (C ABI)         test_register_kernel_at_the_k1_shapes
    register kernel, (4, 1) and generic    small shapes                                     test_register_kernel_small_shapes
    fp64 tile kernel, 1-4 tile rows        n > 12 or m > 4                                  test_fp64_tile_kernel
    fp32 tile kernel                       fp32 arrays there                                test_fp32_tile_kernel
    LDS coverage kernel; register (12, 4)  ZOPT_AMD_LQR_PATH=lds / =reg in a child process  test_environment_switched_paths
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import hp_reference as hp
from tests import lqr_hard_ref as ref
from tests import problems

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "lqr_hard_child.py")


@pytest.fixture(scope="module")
def lqr():
    import torch
    assert torch.cuda.is_available()
    from zopt_amd import lqrUtils
    return lqrUtils


def _sweep_path(run, label, shapes_T, families=lambda n, m, T: ref.FAMILIES, storage="f64", check=ref.check_gains, bound_of=lambda c: c.bound):
    """check(run(case), case) on every family of every (n, m, T); prints the worst error / bound per family"""
    worst = {}
    for n, m, T in shapes_T:
        for f in families(n, m, T):
            c = ref.case(f, n, m, T, storage=storage)
            e = check(run(c), c)
            bound = bound_of(c)
            if e / bound >= worst.get(f, (-np.inf,))[0]:
                worst[f] = (e / bound, e, bound, (n, m, T))
    print(f"{label}: worst error / bound per family (ratio, error, bound, case):")
    for f, w in worst.items():
        print(f"    {f:20s} {w[0]:9.3g} {w[1]:9.2e} {w[2]:9.2e} {w[3]}")
    return worst


def _api(lqr):
    return lambda c: lqr.discreteFiniteHorizonLqr(*c.args, c.T)


# ------------------------------------------------------------------------------------------------------------------------------ K1
@pytest.mark.parametrize("n,m", ref.K1_SHAPES, ids=str)
def test_k1_ring_fp64(lqr, n, m):
    """The ring kernel on every family at every ring phase (T = 1, 2, 3, 4, 7, 11), and `cheap` at T = 30, where a value update that is
    not the Joseph form is outside the bound (tests/test_lqr_hard.py)"""
    _sweep_path(_api(lqr), f"K1 fp64 ({n}, {m})", [(n, m, T) for T in ref.K1_T])
    c = ref.case("cheap", n, m, 30)
    print(f"cheap T = 30: {ref.check_gains(_api(lqr)(c), c):.2e} of {c.bound:.2e}")


@pytest.mark.parametrize("n,m", ref.K1_SHAPES, ids=str)
def test_k1_ring_fp32_storage(lqr, n, m):
    """fp32 arrays at the K1 shapes: fp64 arithmetic rounded once, so half an fp32 ulp of the long-double gains of the same fp32
    inputs plus the case's own fp64 bound"""
    _sweep_path(_api(lqr), f"K1 fp32 storage ({n}, {m}) [excess over half an ulp]", [(n, m, T) for T in ref.K1_T_F32], storage="f32",
                check=ref.check_gains_f32_storage)


def _misaligned(lqr):
    """zm_lqr_backward_f64 with A starting 8 bytes off a 16-byte boundary: the ring kernel refuses it, the register kernel runs"""
    import torch
    from zopt_amd import _lib
    lib = _lib.lib()

    def run(c):
        d = [torch.as_tensor(np.ascontiguousarray(X), device="cuda") for X in c.args]
        buf = torch.zeros(d[0].numel() + 3, dtype=torch.float64, device="cuda")
        off = 1 if buf.data_ptr() % 16 == 0 else 2
        A = buf[off:off + d[0].numel()].view(d[0].shape)
        A.copy_(d[0])
        assert A.data_ptr() % 16 == 8 and all(t.data_ptr() % 16 == 0 for t in d[1:])
        L = torch.full((c.batch, c.T, c.m, c.n), 7.0, dtype=torch.float64, device="cuda")
        rc = lib.zm_lqr_backward_f64(A.data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), L.data_ptr(), c.batch, c.T, c.n, c.m, None)
        assert rc == 0, lib.zm_last_error()
        torch.cuda.synchronize()
        return L.cpu().numpy()
    return run


@pytest.mark.parametrize("n,m", ref.K1_SHAPES, ids=str)
def test_register_kernel_at_the_k1_shapes(lqr, n, m):
    """The specialised register kernel (unpivoted 4 x 4 elimination under its growth check, pivoted re-solve behind it) on operands the
    ring kernel refuses"""
    _sweep_path(_misaligned(lqr), f"register kernel ({n}, {m})", [(n, m, T) for T in ref.REG_SPECIAL_T])


@pytest.mark.parametrize("n,m", ref.REG_SHAPES, ids=str)
def test_register_kernel_small_shapes(lqr, n, m):
    """(4, 1) specialised, and the generic register kernel with one, two and three row tiles, m = 1 .. 4"""
    _sweep_path(_api(lqr), f"register kernel ({n}, {m})", [(n, m, T) for T in ref.REG_T])


# --------------------------------------------------------------------------------------------------------------------------- tiles
@pytest.mark.parametrize("n,m", ref.TILE_SHAPES, ids=str)
def test_fp64_tile_kernel(lqr, n, m):
    _sweep_path(_api(lqr), f"fp64 tile kernel ({n}, {m})", [(n, m, T) for T in ref.TILE_T])


@pytest.mark.parametrize("n,m", ref.TILE_SHAPES, ids=str)
def test_fp32_tile_kernel(lqr, n, m):
    """fp32 arithmetic: 100 x the error of NumPy's fp32 recursion, on the families that yardstick resolves to 1e-3"""
    ratios = []

    def check(L, c):
        e, r = ref.check_gains_f32_tile(L, c)
        ratios.append(r)
        return e
    _sweep_path(_api(lqr), f"fp32 tile kernel ({n}, {m})", [(n, m, T) for T in ref.TILE_T], families=ref.tile32_families, storage="f32",
                check=check, bound_of=lambda c: c.bound32)
    print(f"fp32 tile kernel ({n}, {m}): error / yardstick over {len(ratios)} cases: median {np.median(ratios):.2f}, max {max(ratios):.2f}")


# ------------------------------------------------------------------------------------------------------- environment-switched paths
def child(mode):
    """python tests/lqr_hard_child.py MODE with ZOPT_AMD_LQR_PATH=MODE in the environment (read once per process)"""
    assert os.environ.get("ZOPT_AMD_LQR_PATH") == mode
    from zopt_amd import lqrUtils
    _sweep_path(_api(lqrUtils), f"ZOPT_AMD_LQR_PATH={mode}", [(n, m, T) for n, m in ref.CHILD_SHAPES[mode] for T in ref.CHILD_T])
    print("LQR-HARD-CHILD-OK")


@pytest.mark.parametrize("mode", sorted(ref.CHILD_SHAPES))
def test_environment_switched_paths(mode):
    """lds: the LDS coverage kernel at (13, 3), (24, 8), (64, 16); reg: the register kernel at the aligned (12, 4)"""
    r = subprocess.run([sys.executable, CHILD, mode], env=dict(os.environ, ZOPT_AMD_LQR_PATH=mode), capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    print(r.stdout)
    assert r.returncode == 0 and "LQR-HARD-CHILD-OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


# --------------------------------------------------------------------------------------------------------------- exact properties
def _mixed_batch(n, m, T, dtype):
    """One trajectory of each family, a singular one (R = 0, B = 0) and one with a NaN in A[T-1]"""
    rows = [tuple(X[0] for X in ref.case(f, n, m, T).args) for f in ref.MIXED]
    rows.append((np.repeat(np.eye(n)[None], T, 0), np.zeros((T, n, m)), np.repeat(np.eye(n)[None], T, 0), np.zeros((T, m, m))))
    A, B, Q, R = (X[1].copy() for X in ref.case("plain", n, m, T).args)
    A[T - 1, 0, n - 1] = np.nan
    rows.append((A, B, Q, R))
    return tuple(np.ascontiguousarray(np.stack([r[i] for r in rows]), dtype=dtype) for i in range(4))


@pytest.mark.parametrize("n,m,T,dtype", [(12, 4, 7, np.float64), (8, 4, 7, np.float64), (12, 4, 7, np.float32), (24, 8, 6, np.float64),
                                         (24, 8, 6, np.float32)], ids=str)
def test_mixed_batch_returns_every_trajectory_as_solved_alone(lqr, n, m, T, dtype):
    """One launch over a mixed batch: every finite trajectory comes back with the bits it has when it is solved alone (the re-solve is
    decided per wave; a neighbour's guard, NaN or singular matrix moves nobody's bits), the singular and the NaN trajectory
    non-finite.  The fp64 results are also inside their bounds (trajectory 0 of each case)."""
    args = _mixed_batch(n, m, T, dtype)
    nf = len(ref.MIXED)
    assert args[0].shape[0] == nf + 2
    L = lqr.discreteFiniteHorizonLqr(*args, T)
    assert L.dtype == dtype
    for i, f in enumerate(ref.MIXED):
        alone = lqr.discreteFiniteHorizonLqr(*(X[i:i + 1] for X in args), T)
        assert np.all(np.isfinite(alone)) or dtype == np.float32, f
        assert np.array_equal(L[i:i + 1], alone, equal_nan=True), (f, float(np.max(np.abs(L[i:i + 1] - alone))))
        if dtype == np.float64:
            c = ref.case(f, n, m, T)
            err = hp.sweep_metric(ref.undo_units(L[i:i + 1], f), c.ref[:1])
            assert np.all(err <= c.bound), (f, float(err.max()), c.bound)
    assert not np.any(np.isfinite(L[nf]))
    assert not np.any(np.isfinite(L[nf + 1, :T - 1])) and not np.any(np.isfinite(L[nf + 1, T - 1, :, n - 1]))


@pytest.mark.parametrize("n,m", ref.K1_SHAPES, ids=str)
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_horizon_prefix_bits(lqr, n, m, dtype):
    """The last k gains of a sweep over T = 11 steps are, bit for bit, the sweep over the last k steps' operands (k = 1, 2, 3: other
    ring phases, same arithmetic), on a family that stays on the cofactor solve and on two that leave it"""
    T = 11
    for f in ("plain", "dominant_input", "input_units"):
        args = tuple(X.astype(dtype) for X in ref.case(f, n, m, T).args)
        L = lqr.discreteFiniteHorizonLqr(*args, T)
        for k in (1, 2, 3):
            Lk = lqr.discreteFiniteHorizonLqr(*(np.ascontiguousarray(X[:, T - k:]) for X in args), k)
            assert np.array_equal(L[:, T - k:], Lk), (f, k)


@pytest.mark.parametrize("n,m,T", [(12, 4, 11), (8, 4, 7), (5, 2, 5), (24, 8, 6)], ids=str)
def test_input_units_gains_undo_to_the_unscaled_problem(lqr, n, m, T):
    """E^-1 L' D of the GPU's gains on `input_units` against the long-double gains of the problem in its own units, within the case's
    bound: the twelve decades of Suu' cost nothing"""
    c = ref.case("input_units", n, m, T)
    base = problems.lqr_mildly_unstable(c.batch, T, n, m, problems.hard_lqr_seed("input_units", n, m, T))
    Lb = hp.finite_horizon_ld(*base, T)
    L = ref.undo_units(lqr.discreteFiniteHorizonLqr(*c.args, T), "input_units")
    err = hp.sweep_metric(L, Lb)
    assert np.all(err <= c.bound), (float(err.max()), c.bound)
