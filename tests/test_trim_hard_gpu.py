"""zm_quadcopter_trim_f64 pushed: every output (`resid`, `ok`), the `wind_body` argument, the failing path and Quadcopter.trim's
"Trim failed", on operating points up to 19 m/s -- against the residual of the reference model re-evaluated in long double at the
returned point (tests/model_hp_ref.py), with the wind the call was given.

Required family (tests/trim_ref.py): 300 seeded uvw with |(fa_0, fa_1)| <= 0.9 m g and |w| <= 19, hover and the axis points; the NumPy
restatement of the kernel's iteration converges on all of it within 6 iterations (tests/test_trim_hard.py), so the kernel must.
Failing points: (25, 0, 0) and (21, 0, 0), whose drag no tilt can carry; the second walks the iterate to theta = -pi/2."""
import ctypes

import numpy as np
import pytest

from tests import trim_ref as tr

pytestmark = pytest.mark.gpu
BATCHES = [1, 63, 64, 65, 300]
TOLS = [1e-9, 1e-6]


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available()
    from zopt_amd import _lib, models
    return torch, _lib, models


def _trim(gpu, uvw, wind, tol):
    """the C call with every output: (xTrim (b, 8), uTrim (b, 4), resid (b,), ok (b,)); wind None: the NULL pointer"""
    torch, _lib, _ = gpu
    b = len(uvw)
    v = torch.as_tensor(np.ascontiguousarray(uvw, dtype=np.float64), device="cuda")
    xT = torch.full((b, 8), float("nan"), dtype=torch.float64, device="cuda")
    uT = torch.full((b, 4), float("nan"), dtype=torch.float64, device="cuda")
    res = torch.full((b,), float("nan"), dtype=torch.float64, device="cuda")
    ok = torch.full((b,), -1, dtype=torch.int32, device="cuda")
    wb = None if wind is None else (ctypes.c_double * 3)(*wind)               # a host array: the entry reads it before the launch
    rc = _lib.lib().zm_quadcopter_trim_f64(v.data_ptr(), None if wb is None else ctypes.addressof(wb), xT.data_ptr(), uT.data_ptr(),
                                           res.data_ptr(), ok.data_ptr(), b, float(tol), None)
    _lib.check(rc, "trim")
    torch.cuda.synchronize()
    return xT.cpu().numpy(), uT.cpu().numpy(), res.cpu().numpy(), ok.cpu().numpy()


def _check_converged(uvw, wind, tol, out):
    xT, uT, res, ok = out
    assert np.array_equal(xT[:, :3].view(np.uint64), np.ascontiguousarray(uvw).view(np.uint64))       # bitwise uvw
    assert np.all(np.isfinite(xT)) and np.all(np.isfinite(uT)) and np.all(np.isfinite(res))
    true = tr.residual_ld(xT, uT, wind).astype(np.float64)
    worst = int(np.argmax(true))
    print(f"wind {wind} tol {tol:g} batch {len(uvw)}: worst residual {true[worst]:.2e} at uvw = {uvw[worst]}, |resid - true| <= "
          f"{np.max(np.abs(res - true)):.1e}")
    assert np.array_equal(ok, np.ones(len(uvw), dtype=np.int32)), uvw[ok != 1][:5]
    assert np.all(true <= tol), (uvw[worst], true[worst])
    assert np.max(np.abs(res - true)) <= 1e-12
    assert np.array_equal(ok == 1, res <= tol)


@pytest.mark.parametrize("tol", TOLS)
@pytest.mark.parametrize("wind", tr.WINDS, ids=lambda w: "wind=%g,%g,%g" % w)
def test_required_family_converges(gpu, wind, tol):
    """batches 1, 63, 64, 65 and 300 (a wave is 64 instances) of the family; still air is also run with the NULL wind pointer"""
    F = tr.family()
    for b in BATCHES:
        uvw = F[13:13 + b]                              # the seeded points (the first 13 are hover and the axis points)
        out = _trim(gpu, uvw, wind, tol)
        _check_converged(uvw, wind, tol, out)
    out = _trim(gpu, F, wind, tol)                      # all 313: hover and the axis points too
    _check_converged(F, wind, tol, out)
    if not any(wind):
        null = _trim(gpu, F, None, tol)
        assert all(np.array_equal(a, b) for a, b in zip(out, null))


def test_quadcopter_trim_returns_the_same_points(gpu):
    _, _, models = gpu
    F = tr.family()
    X, U = models.Quadcopter().trim(F.reshape(313, 3))
    xT, uT, _, _ = _trim(gpu, F, None, 1e-9)
    assert np.array_equal(X, xT) and np.array_equal(U, uT)


@pytest.mark.parametrize("tol", TOLS)
def test_failing_points_report_failure_and_do_not_leak(gpu, tol):
    """(25, 0, 0) and (21, 0, 0) at lanes 0, 31 and 63 of a wave of otherwise easy points: ok == 0 and a finite resid > 1e-3 for them
    (the second one's iterate ends at theta = -pi/2, where tan theta is ~1e16), everything as required for the 62 or 63 others"""
    F = tr.family()
    for bad in tr.FAILING:
        for lanes in ([0], [31], [63], [0, 31, 63]):
            uvw = F[20:84].copy()
            uvw[lanes] = bad
            xT, uT, res, ok = _trim(gpu, uvw, None, tol)
            good = np.setdiff1d(np.arange(64), lanes)
            assert np.all(ok[lanes] == 0) and np.all(np.isfinite(res[lanes])) and np.all(res[lanes] > 1e-3), (bad, lanes, res[lanes])
            assert np.array_equal(xT[:, :3], uvw)
            assert np.array_equal(ok == 1, res <= tol)
            _check_converged(uvw[good], (0.0, 0.0, 0.0), tol, (xT[good], uT[good], res[good], ok[good]))
            # the returned resid of a failing point is the residual at the returned point, too, wherever that point is finite
            for i in lanes:
                if np.all(np.isfinite(xT[i])) and np.all(np.isfinite(uT[i])):
                    true = float(tr.residual_ld(xT[i], uT[i], (0, 0, 0))[0])
                    assert abs(res[i] - true) <= 1e-9 * max(1.0, true), (bad, i, res[i], true)


def test_quadcopter_trim_raises_for_a_batch_with_a_failing_point(gpu):
    _, _, models = gpu
    ac = models.Quadcopter()
    for bad in tr.FAILING:
        uvw = tr.family()[:65].copy()
        uvw[40] = bad
        with pytest.raises(RuntimeError, match="Trim failed"):
            ac.trim(uvw)
        with pytest.raises(RuntimeError, match="Trim failed"):
            ac.trim(bad)
    X, U = ac.trim(tr.family()[:65])                    # and not without one
    assert np.all(np.isfinite(X)) and np.all(np.isfinite(U))
