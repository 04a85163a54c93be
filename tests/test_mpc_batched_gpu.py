"""GPU tests of lqrMpc with per-problem data: one batched setup + one batched solve must give, instance by instance, exactly the
bits of the single-problem object solving that instance alone (same tables, same penalty, same ADMM), on every dispatch path."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import mpc_oracle as mo
from tests.test_mpc_batched import _family

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mpc():
    import torch
    assert torch.cuda.is_available()
    from zopt_amd import mpcUtils
    return mpcUtils


def _x0(xu, seed, scale=0.15):
    return scale * xu * np.random.default_rng(seed).uniform(-1, 1, xu.shape)


def _assert_same_as_loop(mpc, data, N, x0, out, prob, kw, idx=None):
    """instance i of the batched result == the single-problem solve of problem p(i) at x0[i]"""
    A, B, Q, R, xl, xu, ul, uu = data
    u, traj, status = out
    P = prob.P
    lead = status.shape
    x0b = np.broadcast_to(x0, lead + (x0.shape[-1],))
    pmap = np.broadcast_to(np.arange(int(np.prod(P))).reshape(P), lead)
    flat = lambda X, k: np.broadcast_to(X, P + X.shape[X.ndim - k:]).reshape((-1,) + X.shape[X.ndim - k:])
    fA, fB, fQ, fR, fxl, fxu, ful, fuu = (flat(X, k) for X, k in zip(data, (2, 2, 2, 2, 1, 1, 1, 1)))
    cache = {}
    for i in (np.ndindex(lead) if idx is None else idx):
        p = int(pmap[i])
        if p not in cache:
            cache[p] = mpc.lqrMpc(fA[p], fB[p], fQ[p], fR[p], N, fxl[p], fxu[p], ful[p], fuu[p])
        one = cache[p]
        u1, t1, s1 = one.solve(x0b[i], warm_start=False, **kw)
        assert np.array_equal(traj.xTraj[i], t1.xTraj), i
        assert np.array_equal(traj.uTraj[i], t1.uTraj), i
        assert np.array_equal(u[i], u1), i
        assert status[i] == s1, i
        assert prob.last_iterations[i] == one.last_iterations, i
        assert np.array_equal(prob.last_residuals[i], one.last_residuals), i


@pytest.mark.parametrize("adaptive", [True, False])
@pytest.mark.parametrize("eps", [1e-2, 1e-6])
def test_bitwise_equal_to_the_single_problem_solver(mpc, adaptive, eps):
    data = _family((37,), 12, 4, seed=11)                   # 37: the last wave of the 4-instances-per-wave kernel is partly empty
    prob = mpc.lqrMpc(*data[:4], 30, *data[4:])
    x0 = _x0(data[5], 1, scale=0.3)                         # some instances infeasible: both outcomes compared
    kw = dict(eps_abs=eps, eps_rel=eps, adaptive_rho=adaptive, max_iter=4000)
    out = prob.solve(x0, **kw)
    assert isinstance(out[2], np.ndarray) and out[2].shape == (37,)
    assert np.mean(out[2] == "optimal") > 0.5
    _assert_same_as_loop(mpc, data, 30, x0, out, prob, kw)


@pytest.mark.parametrize("n, m, N, P", [(3, 2, 20, 6), (9, 4, 20, 6), (16, 5, 10, 3), (24, 8, 10, 3), (4, 2, 80, 5)])
def test_bitwise_equal_on_every_dispatch_path(mpc, n, m, N, P):
    """embedded shapes on the 16-lane kernel; the lane kernel for (16, 5) / (24, 8) and beyond the LDS horizon (N = 80)"""
    data = _family((P,), n, m, seed=n * m + N)
    prob = mpc.lqrMpc(*data[:4], N, *data[4:])
    x0 = _x0(data[5], 2)
    kw = dict(eps_abs=1e-4, eps_rel=1e-4, max_iter=1500)
    _assert_same_as_loop(mpc, data, N, x0, prob.solve(x0, **kw), prob, kw)


def test_forced_lane_path_in_a_child_process():
    env = dict(os.environ, ZOPT_AMD_MPC_PATH="lane")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mpc_batched_lane_child.py")], env=env, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0 and "MPC-BATCHED-OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


def test_broadcasting_of_x0_and_of_shared_data(mpc):
    import torch
    data = _family((5,), 4, 2, seed=3)
    prob = mpc.lqrMpc(*data[:4], 15, *data[4:])
    kw = dict(eps_abs=1e-5, eps_rel=1e-5)
    # (S, P, n): S states per problem;  (n,): one state for every problem
    x0 = np.stack([_x0(data[5], s) for s in range(3)])
    out = prob.solve(x0, **kw)
    assert out[2].shape == (3, 5) and out[1].xTraj.shape == (3, 5, 16, 4) and out[0].shape == (3, 5, 2)
    _assert_same_as_loop(mpc, data, 15, x0, out, prob, kw)
    x1 = 0.1 * np.ones(4)
    out = prob.solve(x1, **kw)
    assert out[2].shape == (5,)
    _assert_same_as_loop(mpc, data, 15, x1, out, prob, kw)
    # device tensors in, device tensors out
    tout = prob.solve(torch.as_tensor(x0, device="cuda"), warm_start=False, **kw)
    assert tout[1].xTraj.is_cuda and np.array_equal(tout[1].xTraj.cpu().numpy(), prob.solve(x0, warm_start=False, **kw)[1].xTraj)
    # mixed sharing (A, B batched; Q, R shared; bounds batched) == the fully materialised batch
    A, B, Q, R, xl, xu, ul, uu = data
    mixed = mpc.lqrMpc(A, B, Q[0], R[0], 15, xl, xu, ul, uu)
    full = mpc.lqrMpc(A, B, np.broadcast_to(Q[0], Q.shape), np.broadcast_to(R[0], R.shape), 15, xl, xu, ul, uu)
    om, of = mixed.solve(x0, **kw), full.solve(x0, **kw)
    assert np.array_equal(mixed.rho, full.rho)
    assert np.array_equal(om[1].xTraj, of[1].xTraj) and np.array_equal(om[1].uTraj, of[1].uTraj)
    assert np.array_equal(om[2], of[2]) and np.array_equal(mixed.last_iterations, full.last_iterations)
    # empty problem set / empty batch of initial states: shaped empty results
    empty = mpc.lqrMpc(A[:0], B[:0], Q[0], R[0], 15, xl[:0], xu[:0], ul[:0], uu[:0])
    u, traj, status = empty.solve(np.zeros(4), **kw)
    assert status.shape == (0,) and traj.xTraj.shape == (0, 16, 4) and u.shape == (0, 2)
    u, traj, status = prob.solve(np.zeros((0, 5, 4)), **kw)
    assert status.shape == (0, 5) and traj.uTraj.shape == (0, 5, 15, 2) and prob.last_iterations.shape == (0, 5)


def _quad_family(P, seed=0):
    """distinct QuadcopterEuler(0.1) linearisations: attitudes and velocities spread around hover, the demo's bounds"""
    from zopt_amd import models, pytrees
    rng = np.random.default_rng(seed)
    X = np.zeros((P, 12))
    X[:, 3:6] = rng.uniform(-0.15, 0.15, (P, 3))
    X[:, 6:12] = rng.uniform(-0.5, 0.5, (P, 6))
    U = np.broadcast_to(models.QuadcopterEuler.uTrim, (P, 4)).copy()
    lin = pytrees.AffineDynamics.from_function(models.QuadcopterEuler(0.1), X, U)
    A, B = np.asarray(lin.f_x), np.asarray(lin.f_u)
    x_ub = np.array([1, 1, 1, 0.3, 0.3, 0.1, 0.5, 0.5, np.inf, np.inf, np.inf, np.inf])
    u_ub = np.array([3.0, 3, 3, 3])
    x0 = np.clip(0.03 * rng.standard_normal((P, 12)), -x_ub + 1e-6, x_ub - 1e-6)
    x0[:, 9:12] = rng.uniform(-3, 3, (P, 3))
    return A, B, np.eye(12), np.eye(4), x_ub, u_ub, x0


def test_quadcopter_family_at_scale(mpc):
    P, N = 1024, 30
    A, B, Q, R, x_ub, u_ub, x0 = _quad_family(P)
    assert A.shape == (P, 12, 12) and not np.array_equal(A[0], A[1])
    prob = mpc.lqrMpc(A, B, Q, R, N, -x_ub, x_ub, -u_ub, u_ub)
    kw = dict(eps_abs=1e-6, eps_rel=1e-6, max_iter=20000)
    u, traj, status = prob.solve(x0, **kw)
    ok = np.flatnonzero(status == "optimal")
    assert len(ok) > 0.9 * P
    for b in ok:
        kkt = mo.kkt_residuals(A[b], B[b], Q, R, Q, N, -x_ub, x_ub, -u_ub, u_ub, x0[b], traj.xTraj[b], traj.uTraj[b], act_tol=1e-3)
        assert kkt["dyn"] <= 1e-12 and kkt["bound"] <= 1e-5 and kkt["stat"] <= 1e-4, (b, kkt)
    for b in ok[:: max(1, len(ok) // 4)][:4]:
        xr, ur, fr = mo.solve_reference(A[b], B[b], Q, R, Q, N, -x_ub, x_ub, -u_ub, u_ub, x0[b])
        assert np.max(np.abs(traj.uTraj[b] - ur)) <= 2e-4, b
    pick = np.random.default_rng(5).choice(P, 8, replace=False)
    data = (A, B, Q, R, -x_ub, x_ub, -u_ub, u_ub)
    _assert_same_as_loop(mpc, data, N, x0, (u, traj, status), prob, kw, idx=[(int(b),) for b in pick])


def test_receding_horizon_loop_over_a_family(mpc):
    P, N, steps = 16, 30, 8
    A, B, Q, R, x_ub, u_ub, x0 = _quad_family(P, seed=2)
    lo, hi = -x_ub + 1e-6, x_ub - 1e-6
    kw = dict(eps_abs=1e-3, eps_rel=1e-3, max_iter=4000)

    def loop(solve_fn, x, warm):
        its, xs = 0, []
        for _ in range(steps):
            x = np.minimum(np.maximum(x, lo), hi)
            res, it = solve_fn(x, warm)
            its += it
            xs.append(res)
            x = res[1].xTraj[..., 1, :]
        return its, xs

    def batched(warm):
        prob = mpc.lqrMpc(A, B, Q, R, N, -x_ub, x_ub, -u_ub, u_ub)

        def f(x, w):
            out = prob.solve(x, warm_start=w, **kw)
            return out, int(prob.last_iterations.sum())
        return loop(f, x0, warm)
    cold_its, _ = batched(False)
    warm_its, warm_xs = batched("shift")
    assert warm_its <= cold_its
    for b in (0, 7, 15):
        one = mpc.lqrMpc(A[b], B[b], Q, R, N, -x_ub, x_ub, -u_ub, u_ub)

        def f(x, w):
            out = one.solve(x, warm_start=w, **kw)
            return out, int(one.last_iterations)
        _, xs1 = loop(f, x0[b], "shift")
        for k in range(steps):
            assert np.array_equal(warm_xs[k][1].xTraj[b], xs1[k][1].xTraj), (b, k)
            assert np.array_equal(warm_xs[k][1].uTraj[b], xs1[k][1].uTraj), (b, k)
            assert warm_xs[k][2][b] == xs1[k][2], (b, k)


def test_mixed_statuses_in_one_batch(mpc):
    data = list(_family((8,), 4, 2, seed=9))
    xl, xu = data[4].copy(), data[5].copy()
    xl[5, 1], xu[5, 1] = 0.5, -0.5                          # problem 5: an empty box
    data[4], data[5] = xl, xu
    x0 = _x0(np.abs(data[5]), 4)
    x0[2, 0] = 2.0 * data[5][2, 0]                          # problem 2: x0 outside its box
    prob = mpc.lqrMpc(*data[:4], 12, *data[4:])
    kw = dict(eps_abs=1e-5, eps_rel=1e-5)
    out = prob.solve(x0, **kw)
    assert out[2][2] == "infeasible" and out[2][5] == "infeasible"
    assert all(out[2][i] == "optimal" for i in (0, 1, 3, 4, 6, 7))
    _assert_same_as_loop(mpc, tuple(data), 12, x0, out, prob, kw)


def test_problem_index_outside_the_problem_set_is_refused(mpc):
    import ctypes
    import torch
    from zopt_amd import _lib
    data = _family((3,), 4, 2, seed=1)
    prob = mpc.lqrMpc(*data[:4], 5, *data[4:])
    d, (K, Mi, nl, l0, drho, _) = prob._device_problem_batched(prob.rho, True)
    B = 4
    x0 = torch.zeros((B, 4), dtype=torch.float64, device="cuda")
    ws = torch.empty(4 * B * 5 * 6, dtype=torch.float64, device="cuda")
    xT = torch.empty((B, 6, 4), dtype=torch.float64, device="cuda")
    uT = torch.empty((B, 5, 2), dtype=torch.float64, device="cuda")
    st = torch.empty(B, dtype=torch.int32, device="cuda")
    for bad in (3, -1):
        pm = torch.tensor([0, 1, bad, 2], dtype=torch.int32, device="cuda")
        rc = _lib.lib().zm_mpc_solve_batched_f64(d["A"].data_ptr(), d["B"].data_ptr(), K.data_ptr(), Mi.data_ptr(), nl, l0, 5.0, 1.6,
                                                  d["x_lb"].data_ptr(), d["x_ub"].data_ptr(), d["u_lb"].data_ptr(),
                                                  d["u_ub"].data_ptr(), x0.data_ptr(), drho.data_ptr(), pm.data_ptr(), 3, 1e-5, 1e-5,
                                                  1e-4, 100, 0, ws.data_ptr(), xT.data_ptr(), uT.data_ptr(), st.data_ptr(), None,
                                                  None, B, 5, 4, 2, ctypes.c_void_p(0))
        assert rc == _lib.ZM_EINVAL and b"outside [0, 3)" in _lib.lib().zm_last_error()
