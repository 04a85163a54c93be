"""Full-size gates of the tiled finite-horizon sweep (lqr_tiled_core.h): BASELINE configs[4]'s tile shape (n = 64, m = 16, T = 200) at
a batch whose A and Q pass 2^31 elements (fp32) or 2^32 bytes (fp64), and hard numerics against the long-double reference.

At full size every trajectory is distinct (random LTI systems, tiled over the horizon on the device) and is checked three ways:
sampled trajectories around the 1024-wave and 2^31-element boundaries against the fp64 oracle, L[:, 0] of EVERY trajectory
against the DARE gain of its system (a long horizon reaches it), and the one-launch result against four launches over contiguous
quarters of the batch through the C ABI with offset pointers (bit for bit)."""
import ctypes

import numpy as np
import pytest

from oracle import zopt_oracle as zo
from tests import hp_reference as hp
from tests import problems
from tests.test_lqr_tiled_gpu import _check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lqr():
    import torch
    assert torch.cuda.is_available()
    from zopt_amd import lqrUtils
    return lqrUtils


def _device_horizon(A1, B1, Q1, R1, T):
    """upload the per-system matrices only and tile them over the horizon on the device: (b, T, ., .) contiguous tensors"""
    import torch
    out = []
    for X in (A1, B1, Q1, R1):
        t = torch.as_tensor(X, device="cuda")
        out.append(t[:, None].expand(t.shape[0], T, *t.shape[1:]).contiguous())
        del t
    return out


def _free():
    import torch
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def test_fp32_config4_beyond_2_31_elements(lqr):
    import torch
    from zopt_amd import _lib
    n, m, T, batch = 64, 16, 200, 2688
    per = T * n * n
    assert batch * per > 2 ** 31 and 2621 * per < 2 ** 31 < 2622 * per     # trajectory 2621 straddles element 2^31 of A and Q
    A1, B1, Q1, R1 = problems.random_lti_systems(batch, n, m, seed=2688, dtype=np.float32)
    A, B, Q, R = _device_horizon(A1, B1, Q1, R1, T)
    L = lqr.discreteFiniteHorizonLqr(A, B, Q, R, T)
    assert isinstance(L, torch.Tensor) and L.dtype == torch.float32 and L.shape == (batch, T, m, n)
    # (iii) four launches over contiguous quarters, offset pointers through the C ABI: the same bits
    L4 = torch.empty_like(L)
    lib, q = _lib.lib(), batch // 4
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for c in range(4):
        lo, hi = c * q, (c + 1) * q
        rc = lib.zm_lqr_backward_f32(A[lo:hi].data_ptr(), B[lo:hi].data_ptr(), Q[lo:hi].data_ptr(), R[lo:hi].data_ptr(),
                                     L4[lo:hi].data_ptr(), hi - lo, T, n, m, stream)
        _lib.check(rc, "zm_lqr_backward_f32")
    torch.cuda.synchronize()
    same = torch.equal(L, L4)
    del A, B, Q, R, L4
    _free()
    assert same
    picks = (0, 1, 1023, 1024, 1343, 2621, 2622, 2687)
    Lp, L0 = L[list(picks)].cpu().numpy(), L[:, 0].cpu().numpy()
    del L
    _free()
    # (i) trajectories at the wave-slot and 2^31 boundaries against the fp64 oracle
    for j, t in enumerate(picks):
        _check(Lp[j:j + 1], *problems.tile_over_horizon(A1[t:t + 1], B1[t:t + 1], Q1[t:t + 1], R1[t:t + 1], T), T)
    # (ii) every trajectory: L_0 of the 200-step horizon is the infinite-horizon gain of its system (zm_dare_f64 on fp64 inputs)
    Ld = lqr.discreteInfiniteHorizonLqr(*(x.astype(np.float64) for x in (A1, B1, Q1, R1)))
    err = np.max(np.abs(L0 - Ld), axis=(1, 2)) / np.max(np.abs(Ld), axis=(1, 2))
    assert np.all(err <= 5e-4), (int(np.argmax(err)), float(err.max()))


def test_fp64_config4_shape_beyond_2_32_bytes(lqr):
    import torch
    n, m, T, batch = 64, 16, 200, 700
    assert batch * T * n * n * 8 > 2 ** 32
    A1, B1, Q1, R1 = problems.random_lti_systems(batch, n, m, seed=700)
    A, B, Q, R = _device_horizon(A1, B1, Q1, R1, T)
    L = lqr.discreteFiniteHorizonLqr(A, B, Q, R, T)
    assert L.dtype == torch.float64 and L.shape == (batch, T, m, n)
    del A, B, Q, R
    picks = (0, 349, 699)
    Lp, L0 = L[list(picks)].cpu().numpy(), L[:, 0].cpu().numpy()
    del L
    _free()
    for j, t in enumerate(picks):
        Lo = zo.discreteFiniteHorizonLqr(*problems.tile_over_horizon(A1[t:t + 1], B1[t:t + 1], Q1[t:t + 1], R1[t:t + 1], T), T)
        assert np.max(np.abs(Lp[j] - Lo[0])) <= 1e-10 * np.max(np.abs(Lo)), t
    Ld = lqr.discreteInfiniteHorizonLqr(A1, B1, Q1, R1)
    err = np.max(np.abs(L0 - Ld), axis=(1, 2)) / np.max(np.abs(Ld), axis=(1, 2))
    assert np.all(err <= 1e-8), (int(np.argmax(err)), float(err.max()))


@pytest.mark.parametrize("name", ["cheap_control", "expensive_control", "badly_scaled"])
@pytest.mark.parametrize("n,m", [(24, 8), (48, 16), (64, 16)])
def test_hard_numerics_against_long_double(lqr, name, n, m):
    """fp64 tiled sweep on cheap / expensive control and badly scaled coordinates: its error against the long-double recursion is
    at most 1e-10 of the gain's scale, or 4x the fp64 oracle's own error where that is larger"""
    T, batch = 50, 3
    A1, B1, Q1, R1 = problems.HARD_DARE[name](batch, n, m, seed=500 + n)
    A, B, Q, R = problems.tile_over_horizon(A1, B1, Q1, R1, T)
    Lg = lqr.discreteFiniteHorizonLqr(A, B, Q, R, T)
    Lhp = hp.finite_horizon_ld(A, B, Q, R, T)
    Lo = zo.discreteFiniteHorizonLqr(A, B, Q, R, T)
    assert np.all(np.isfinite(Lg))
    for i in range(batch):
        scale = float(np.max(np.abs(Lhp[i])))
        e_gpu, e_or = float(np.max(np.abs(Lg[i] - Lhp[i]))), float(np.max(np.abs(Lo[i] - Lhp[i])))
        assert e_gpu <= max(1e-10 * scale, 4 * e_or), (i, e_gpu / scale, e_or / scale)
