"""Hard-family GPU tests of the backward sweeps: `backwardPass_ilqr` / zm_ilqr_backward_ex_f64 (ilqr_backward.hip: LDS-DMA ring and
register kernel; sweep_tiled_f64.hip beyond n = 12, m = 4), `bilinearAffineLqr`, and the DDP sweeps (`backwardPass_ddp` dense, the
packed-pairs list sweep, the step-by-step large shapes) against LONG-DOUBLE references (tests/hp_reference.py) on the families of
tests/problems.py: HARD_SWEEP and HARD_DDP, each with one known difficulty.

Metric: per trajectory and per step, max|out_k - ref_k| / max_k' max|ref_k'| over that trajectory's steps, l and L separately (L D for
`badly_scaled`).  Every trajectory and every step is asserted.  Bounds come from the reference side only (hard_cases.case_bounds):
100 x max(the fp64 oracle's own error on the case, its error on the plain family at the same shape and horizon); for the DDP sweeps
additionally 10 x the case's sensitivity to a 2e-11 perturbation of every projected matrix, the projection's documented resolution
(that term capped at 1e-9, the tolerance of the parity tests these supersede).
tests/test_hp_reference.py asserts that every family has its feature and that the oracle's error stays <= 1e-9 on every case run here.
Each test prints its figures (run with -s); DESIGN.md tabulates them."""
import ctypes

import numpy as np
import pytest

from tests import hard_cases as hc
from tests import hp_reference as hp
from tests import problems

pytestmark = pytest.mark.gpu
FAMILIES = sorted(problems.HARD_SWEEP)
DDP_FAMILIES = sorted(problems.HARD_DDP)


@pytest.fixture(scope="module")
def mods():
    import torch
    assert torch.cuda.is_available()
    from zopt_amd import _lib, ilqrUtils, lqrUtils, models
    return ilqrUtils, lqrUtils, _lib, models


def _hold(what, case_fn, name, n, m, T, l, L, exact_zero_l=True, **kw):
    """Assert the policy (l, L) of `case_fn(name, n, m, T)` against its long-double reference at the case's bounds."""
    c = case_fn(name, n, m, T, **kw)
    el, eL = hc.policy_errors(name, n, l, L, c["ref"])
    bl, bL = hc.case_bounds(case_fn, name, n, m, T, **kw)
    print(f"HARD {what} {name} ({n},{m},{T}): kernel l {el.max():.1e} L {eL.max():.1e} | oracle l {c['e_l']:.1e} L {c['e_L']:.1e} | "
          f"bound l {bl:.1e} L {bL:.1e}")
    assert el.shape == eL.shape == np.asarray(l).shape[:2]
    assert np.all(el <= bl), (float(el.max()), bl)
    assert np.all(eL <= bL), (float(eL.max()), bL)
    if name == "zero_gradient" and exact_zero_l:
        assert not np.asarray(l).any()                  # c_x = c_u = v_x = 0: l is exactly zero


@pytest.mark.parametrize("name", FAMILIES)
@pytest.mark.parametrize("n,m", problems.ILQR_ONE_TILE_SHAPES + problems.ILQR_TILED_SHAPES)
def test_backwardPass_ilqr_hard_families(mods, n, m, name):
    """The public call at every shape: the LDS-DMA ring at (12, 4) and (8, 4), the register kernel at the other one-tile shapes, the
    tile sweep beyond; the long horizon of each (family, shape)."""
    T = problems.sweep_horizon(name, n, m)
    pol = mods[0].backwardPass_ilqr(*hc.ilqr_case(name, n, m, T)["args"])
    _hold("ilqr", hc.ilqr_case, name, n, m, T, pol.l, pol.L)


def _ilqr_ex(lib, args, shift, shared):
    """zm_ilqr_backward_ex_f64 with every operand at a 16-B aligned address (shift 0: the DMA ring) or at +8 B (shift 1: the register
    kernel); shared: the Hessians handed over as single matrices."""
    import torch
    (f, f_x, f_u), (c, c_x, c_u, c_xx, c_ux, c_uu), (v, v_x, v_xx) = args
    batch, T, n, m = f_u.shape
    host = [f_x, f_u, c_x, c_u] + ([c_xx[0, 0], c_ux[0, 0], c_uu[0, 0]] if shared else [c_xx, c_ux, c_uu]) + [v_x, v_xx[0] if shared else v_xx]
    dev = []
    for X in host:
        buf = torch.zeros(X.size + 2, dtype=torch.float64, device="cuda")
        buf[shift:shift + X.size] = torch.as_tensor(np.ascontiguousarray(X).ravel(), device="cuda")
        t = buf[shift:shift + X.size]
        assert t.data_ptr() % 16 == 8 * shift
        dev.append(t)
    dl = torch.full((batch, T, m), np.nan, dtype=torch.float64, device="cuda")
    dL = torch.full((batch, T, m, n), np.nan, dtype=torch.float64, device="cuda")
    rc = lib.lib().zm_ilqr_backward_ex_f64(*[t.data_ptr() for t in dev], None, 1 if shared else 0, dl.data_ptr(), dL.data_ptr(), batch, T,
                                           n, m, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    lib.check(rc, "zm_ilqr_backward_ex_f64")
    torch.cuda.synchronize()
    return dl.cpu().numpy(), dL.cpu().numpy()


@pytest.mark.parametrize("name", FAMILIES)
@pytest.mark.parametrize("n", [12, 8])
def test_ring_and_register_kernels_hard_families(mods, n, name):
    """(12, 4) and (8, 4): the same numbers through the LDS-DMA ring (16-B aligned operands) and through the register kernel
    (operands at +8 B), each held to the reference on its own."""
    T = problems.sweep_horizon(name, n, 4)
    args = hc.ilqr_case(name, n, 4, T)["args"]
    for shift, what in ((0, "ilqr-ring"), (1, "ilqr-register")):
        l, L = _ilqr_ex(mods[2], args, shift, False)
        _hold(what, hc.ilqr_case, name, n, 4, T, l, L)


@pytest.mark.parametrize("name", FAMILIES)
def test_shared_hessians_hard_families(mods, name):
    """(12, 4) with one cost Hessian for every trajectory and step, handed over as single matrices (`shared_hessian = 1`), ring and
    register kernel."""
    T = problems.sweep_horizon(name, 12, 4)
    args = hc.ilqr_case(name, 12, 4, T, shared=True)["args"]
    for shift, what in ((0, "ilqr-shared-ring"), (1, "ilqr-shared-register")):
        l, L = _ilqr_ex(mods[2], args, shift, True)
        _hold(what, hc.ilqr_case, name, 12, 4, T, l, L, shared=True)


@pytest.mark.parametrize("T", problems.RING_HORIZONS)
@pytest.mark.parametrize("n", [12, 8])
def test_horizons_around_the_ring_depth(mods, n, T):
    """`unstable` at T = 1, 2, 3, 4, 7: every phase of the ring's fill and drain, ring and register kernel."""
    args = hc.ilqr_case("unstable", n, 4, T)["args"]
    for shift, what in ((0, "ilqr-ring"), (1, "ilqr-register")):
        l, L = _ilqr_ex(mods[2], args, shift, False)
        _hold(what, hc.ilqr_case, "unstable", n, 4, T, l, L)


@pytest.mark.parametrize("name", FAMILIES)
@pytest.mark.parametrize("n,m", problems.AFFINE_SHAPES)
def test_bilinearAffineLqr_hard_families(mods, n, m, name):
    """`bilinearAffineLqr` on the same families with a non-zero offset d (l is then non-zero in `zero_gradient` too, so its exact-zero
    assertion belongs to the iLQR tests): ring at (12, 4) and (8, 4), register kernel at (5, 3), tile sweep at (20, 6) and (48, 16)."""
    T = problems.sweep_horizon(name, n, m)
    c = hc.affine_case(name, n, m, T)
    L, l = mods[1].bilinearAffineLqr(*c["args"], T)
    _hold("affine", hc.affine_case, name, n, m, T, l, L, exact_zero_l=False)


@pytest.mark.parametrize("name", DDP_FAMILIES)
@pytest.mark.parametrize("n,m", list(problems.DDP_SHAPES))
def test_backwardPass_ddp_hard_families(mods, n, m, name):
    """`backwardPass_ddp`: the one-tile sweep with the matrix-sign projection inside at (12, 4), (5, 3), (2, 2); step by step (torch
    contraction, tiled projection, tile sweep) at (16, 4) and (20, 6)."""
    T = problems.DDP_SHAPES[(n, m)]
    pol = mods[0].backwardPass_ddp(*hc.ddp_case(name, n, m, T)["args"])
    _hold("ddp", hc.ddp_case, name, n, m, T, pol.l, pol.L)


def test_packed_pairs_sweep_hard_family(mods):
    """zm_ddp_backward_pairs_list_f64 on `packed_pairs` (f_ux = f_uu = 0, f_xx on the quadcopter's 28 declared pairs, shared cost
    Hessians): with per-step Hessian arrays it runs the register kernel, with `shared_hessian = 1` the LDS-ring kernel that takes the
    contracted vf_zz from its ring (the form the fused DDP driver runs).  The register form is bit for bit the dense zm_ddp_backward_f64
    on the same numbers -- with zero tensors and with NULL for f_ux / f_uu -- and every call is held to the long-double reference.
    The ring form is held to the reference ALONE: the dense entry point always runs the register kernel, whose Riccati arithmetic is
    ordered differently from the ring kernel's (the iLQR ring and register kernels likewise agree to rounding, not in bits), so there
    is no dense call with the ring kernel's bits to compare with."""
    import torch
    ilqr, _, _lib, models = mods
    lib = _lib.lib()
    n, m, T = 12, 4, problems.DDP_SHAPES[(12, 4)]
    md = models.QuadcopterEuler(0.1).c_struct()
    pmd = ctypes.addressof(md)
    npairs, pairs = ctypes.c_int32(0), (ctypes.c_int32 * 64)()
    _lib.check(lib.zm_model_hessian_pairs(pmd, ctypes.addressof(pairs), ctypes.addressof(npairs)), "pairs")
    assert [tuple(pairs[2 * p:2 * p + 2]) for p in range(npairs.value)] == problems.QUAD_HESSIAN_PAIRS
    (f, f_x, f_u, f_xx, f_ux, f_uu), (c, c_x, c_u, c_xx, c_ux, c_uu), (v, v_x, v_xx) = hc.ddp_case("packed_pairs", n, m, T)["args"]
    b = f_x.shape[0]
    assert not f_ux.any() and not f_uu.any()
    H = np.stack([f_xx[:, :, :, a, bb] for a, bb in problems.QUAD_HESSIAN_PAIRS], axis=2)          # (b, T, 28, 12)
    t = lambda X: torch.as_tensor(np.ascontiguousarray(X), device="cuda")      # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    dfx, dfu, dcx, dcu, dvx, dH, dfxx, dfux, dfuu = (t(X) for X in (f_x, f_u, c_x, c_u, v_x, H, f_xx, f_ux, f_uu))
    for shared in (0, 1):
        hess = [t(X[0, 0] if shared else X) for X in (c_xx, c_ux, c_uu)]
        dvxx = t(v_xx[0] if shared else v_xx)
        ptrs = [dcx.data_ptr(), dcu.data_ptr()] + [h.data_ptr() for h in hess] + [dvx.data_ptr(), dvxx.data_ptr()]
        assert all(p % 16 == 0 for p in ptrs + [dfx.data_ptr(), dfu.data_ptr(), dH.data_ptr()])      # the ring kernel applies
        outs = []
        for kind in ("zeros", "null", "packed"):
            l = torch.full((b, T, m), np.nan, dtype=torch.float64, device="cuda")
            L = torch.full((b, T, m, n), np.nan, dtype=torch.float64, device="cuda")
            if kind == "packed":
                rc = lib.zm_ddp_backward_pairs_list_f64(pmd, dfx.data_ptr(), dfu.data_ptr(), dH.data_ptr(), *ptrs, None, 0, None, shared,
                                                        l.data_ptr(), L.data_ptr(), b, T, st)
            else:
                rc = lib.zm_ddp_backward_f64(dfx.data_ptr(), dfu.data_ptr(), dfxx.data_ptr(), dfux.data_ptr() if kind == "zeros" else None,
                                             dfuu.data_ptr() if kind == "zeros" else None, *ptrs, None, shared, l.data_ptr(), L.data_ptr(),
                                             b, T, n, m, st)
            _lib.check(rc, kind)
            torch.cuda.synchronize()
            outs.append((l.cpu().numpy(), L.cpu().numpy()))
            _hold(f"ddp-{kind}-shared{shared}", hc.ddp_case, "packed_pairs", n, m, T, *outs[-1])
        # zero tensors against NULL: always the same bits.  Packed against dense: the same bits on the register kernel (the contraction
        # runs in the same order); the ring kernel orders its Riccati arithmetic differently and is held to the reference above.
        for l, L in outs[1:2 if shared else 3]:
            assert np.array_equal(l, outs[0][0]) and np.array_equal(L, outs[0][1])
