"""GPU tests of lqrMpc.solve(x0, xRef=..., uRef=...): reference tracking through the ADMM kernels (zm_mpc_solve_tracking_f64).

The checkers are those of tests/mpc_tracking_ref.py (NumPy restatement of the tracking ADMM, independent SciPy solve of the condensed
tracking QP, tracking KKT certificate).  Every problem used here has at least one bound active in the independent solution."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import mpc_tracking_ref as tr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mpc():
    import torch
    assert torch.cuda.is_available()
    from zopt_amd import mpcUtils
    return mpcUtils


# ---- 1. zero reference == the regulator, bit for bit --------------------------------------------------------------------------------

def test_zero_reference_equals_the_regulator_wave_path(mpc):
    data = tr.quad_data(30)
    prob = mpc.lqrMpc(*data[:4], 30, *data[5:])
    rng = np.random.default_rng(1)
    x0 = np.clip(0.03 * rng.standard_normal((64, 12)), data[5] + 1e-6, data[6] - 1e-6)
    x0[:, 9:12] = rng.uniform(-10, 10, (64, 3))
    for kw in (dict(eps_abs=1e-4, eps_rel=1e-4, max_iter=4000), dict(eps_abs=1e-3, eps_rel=1e-3, adaptive_rho=False, max_iter=500)):
        plain = prob.solve(x0, warm_start=False, **kw)
        its = prob.last_iterations.copy()
        zero = prob.solve(x0, xRef=np.zeros((64, 31, 12)), uRef=np.zeros((64, 30, 4)), warm_start=False, **kw)
        assert np.array_equal(zero[1].xTraj, plain[1].xTraj) and np.array_equal(zero[1].uTraj, plain[1].uTraj)
        assert np.array_equal(zero[2], plain[2]) and np.array_equal(prob.last_iterations, its)
        only_x = prob.solve(x0, xRef=np.zeros((31, 12)), warm_start=False, **kw)          # uRef = None: zeros; xRef broadcast
        assert np.array_equal(only_x[1].uTraj, plain[1].uTraj) and np.array_equal(prob.last_iterations, its)
    assert np.any(plain[2] == "optimal") and its.max() > 8


def test_zero_reference_equals_the_regulator_lane_path(mpc):
    from tests.test_mpc_gpu import _random_problem
    rng = np.random.default_rng(248)
    n, m, N = 24, 8, 4
    A, B, Q, R, Qf = _random_problem(rng, n, m, N)
    x_ub, u_ub = np.full(n, 4.0), np.full(m, 0.15)
    prob = mpc.lqrMpc(A, B, Q, R, N, -x_ub, x_ub, -u_ub, u_ub, Qf=Qf)
    x0 = rng.uniform(-1.0, 1.0, (4, n))
    kw = dict(eps_abs=1e-6, eps_rel=1e-6, max_iter=30000, warm_start=False)
    plain = prob.solve(x0, **kw)
    its = prob.last_iterations.copy()
    zero = prob.solve(x0, xRef=np.zeros((4, N + 1, n)), uRef=np.zeros((4, N, m)), **kw)
    assert np.array_equal(zero[1].xTraj, plain[1].xTraj) and np.array_equal(zero[1].uTraj, plain[1].uTraj)
    assert np.array_equal(zero[2], plain[2]) and np.array_equal(prob.last_iterations, its)
    assert np.all(plain[2] == "optimal") and np.max(np.abs(plain[1].uTraj)) >= 0.15 - 1e-5


def test_zero_reference_equals_the_regulator_per_problem(mpc):
    from tests.test_mpc_batched import _family
    data = _family((9,), 12, 4, seed=16)
    prob = mpc.lqrMpc(*data[:4], 30, *data[4:])
    x0 = 0.3 * data[5] * np.random.default_rng(12).uniform(-1, 1, (9, 12))
    kw = dict(eps_abs=1e-5, eps_rel=1e-5, max_iter=3000, warm_start=False)
    plain = prob.solve(x0, **kw)
    its = prob.last_iterations.copy()
    zero = prob.solve(x0, xRef=np.zeros((9, 31, 12)), uRef=np.zeros((30, 4)), **kw)
    assert np.array_equal(zero[1].xTraj, plain[1].xTraj) and np.array_equal(zero[1].uTraj, plain[1].uTraj)
    assert np.array_equal(zero[2], plain[2]) and np.array_equal(prob.last_iterations, its)


# ---- 2. iterate-level parity with the NumPy tracking ADMM ---------------------------------------------------------------------------

def test_iterates_equal_the_numpy_tracking_admm(mpc):
    """tests/test_mpc_gpu.py:112-120 with a reference: the same number of ADMM iterations and the same iterate to 1e-9, with and without
    over-relaxation, on the quadcopter with a reference that leaves the box."""
    N = 25
    data = tr.quad_data(N)
    A, B, Q, R, Qf, x_lb, x_ub, u_lb, u_ub = data
    x0, xRef, uRef = tr.quad_reference(N)
    xs, us, _ = tr.solve_reference(A, B, Q, R, Qf, N, x_lb, x_ub, u_lb, u_ub, x0[0], xRef[0], uRef[0])
    assert tr.n_active(xs, us, x_lb, x_ub, u_lb, u_ub) >= 1
    prob = mpc.lqrMpc(A, B, Q, R, N, x_lb, x_ub, u_lb, u_ub)
    for alpha in (1.6, 1.0):
        _, tra, sta = prob.solve(x0, xRef=xRef, uRef=uRef, eps_abs=1e-4, eps_rel=1e-4, max_iter=100000, adaptive_rho=False, alpha=alpha,
                                 warm_start=False)
        xo, uo, so, ito = tr.admm(A, B, Q, R, Qf, N, x_lb, x_ub, u_lb, u_ub, x0[0], xRef[0], uRef[0], rho=prob.rho, eps_abs=1e-4,
                                  eps_rel=1e-4, max_iter=100000, alpha=alpha)
        ex, eu = np.max(np.abs(tra.xTraj[0] - xo)), np.max(np.abs(tra.uTraj[0] - uo))
        print(f"alpha {alpha}: numpy {ito} iterations, kernel {int(prob.last_iterations[0])}, |dx| {ex:.2e} |du| {eu:.2e}")
        assert so == "optimal" and sta[0] == "optimal" and ito == int(prob.last_iterations[0])
        assert eu <= 1e-9 and ex <= 1e-9


# ---- 3. independent solve and KKT certificate ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,m,N", [(2, 1, 6), (2, 2, 5), (4, 2, 6), (4, 1, 8), (1, 1, 4), (13, 2, 6)])
def test_tracking_against_independent_solve(mpc, n, m, N):
    """the shapes of test_constrained_small_problems_against_independent_solve on the 16-lane kernel and one ((13, 2): embedded in
    (24, 8)) on the lane kernel, default (adaptive) options at eps = 1e-6, that test's bounds.

    (4, 1, 8), instance 0 is the case the cycle guard of the tracking kernel exists for (mpc_wave.hip: ZM_TRK_LEVEL): without it the
    adaptive penalty ping-pongs between its two top levels and the instance ends "user_limit" at 30000 iterations."""
    nb = 4 if n > 12 else 8
    data, x0, xRef, uRef = tr.random_case(n, m, N, seed=10 * n + m, nb=nb)
    A, B, Q, R, Qf, x_lb, x_ub, u_lb, u_ub = data
    prob = mpc.lqrMpc(A, B, Q, R, N, x_lb, x_ub, u_lb, u_ub, Qf=Qf)
    u0, traj, status = prob.solve(x0, xRef=xRef, uRef=uRef, eps_abs=1e-6, eps_rel=1e-6, max_iter=30000)
    assert np.all(status == "optimal")
    max_ref = 1 if n > 12 else 3
    n_act = n_ref = 0
    for b in range(nb):
        x, u = traj.xTraj[b], traj.uTraj[b]
        kkt = tr.kkt_residuals(A, B, Q, R, Qf, N, x_lb, x_ub, u_lb, u_ub, x0[b], x, u, xRef[b], uRef[b], act_tol=1e-4)
        assert kkt["dyn"] <= 1e-12 and kkt["bound"] <= 1e-4 and kkt["stat"] <= 1e-3, (b, kkt)
        active = tr.n_active(x, u, x_lb, x_ub, u_lb, u_ub) >= 1
        n_act += int(active)
        if active and n_ref < max_ref:
            n_ref += 1
            xr, ur, fr = tr.solve_reference(A, B, Q, R, Qf, N, x_lb, x_ub, u_lb, u_ub, x0[b], xRef[b], uRef[b])
            assert tr.n_active(xr, ur, x_lb, x_ub, u_lb, u_ub) >= 1
            err = np.max(np.abs(u - ur))
            print(f"({n}, {m}, {N}) instance {b}: |u - u_scipy| = {err:.2e}, kkt {kkt}")
            assert err <= 2e-3
            assert tr.cost(Q, R, Qf, x, u, xRef[b], uRef[b]) <= fr + 1e-4 * max(1.0, abs(fr))
    assert n_act >= 1 and n_ref == min(max_ref, n_act)


# ---- 4. a constant reference at an equilibrium == the regulator in shifted coordinates ---------------------------------------------

def test_equilibrium_reference_equals_the_shifted_regulator(mpc):
    from tests.test_mpc_gpu import _random_problem
    rng = np.random.default_rng(77)
    n, m, N, nb = 4, 2, 10, 8
    A, B, Q, R, Qf = _random_problem(rng, n, m, N)
    us = np.array([0.1, -0.05])
    xs = np.linalg.solve(np.eye(n) - A, B @ us)                  # A xs + B us = xs
    assert np.max(np.abs(A @ xs + B @ us - xs)) <= 1e-14
    x_ub, u_ub = np.full(n, 4.0), np.full(m, 0.15)
    x0 = rng.uniform(-1.0, 1.0, (nb, n))
    kw = dict(eps_abs=1e-6, eps_rel=1e-6, max_iter=30000)
    track = mpc.lqrMpc(A, B, Q, R, N, -x_ub, x_ub, -u_ub, u_ub, Qf=Qf)
    _, tt, st = track.solve(x0, xRef=np.tile(xs, (N + 1, 1)), uRef=np.tile(us, (N, 1)), **kw)
    shifted = mpc.lqrMpc(A, B, Q, R, N, -x_ub - xs, x_ub - xs, -u_ub - us, u_ub - us, Qf=Qf)
    _, ts, ss = shifted.solve(x0 - xs, **kw)
    assert np.all(st == "optimal") and np.all(ss == "optimal")
    ex, eu = np.max(np.abs(tt.xTraj - (ts.xTraj + xs))), np.max(np.abs(tt.uTraj - (ts.uTraj + us)))
    print(f"shift equivalence: |dx| {ex:.2e} |du| {eu:.2e}")
    assert ex <= 2e-3 and eu <= 2e-3
    xr, ur, _ = tr.solve_reference(A, B, Q, R, Qf, N, -x_ub, x_ub, -u_ub, u_ub, x0[0], np.tile(xs, (N + 1, 1)), np.tile(us, (N, 1)))
    assert tr.n_active(xr, ur, -x_ub, x_ub, -u_ub, u_ub) >= 1
    assert np.max(np.abs(tt.uTraj[0] - ur)) <= 2e-3


# ---- 5. per-problem data: every instance == its single-problem tracking solve, bit for bit ---------------------------------------

def test_per_problem_tracking_equals_the_single_problem_solves(mpc):
    """the family of the README example (64 trimmed forward speeds of models.Quadcopter, dt = 0.05, N = 20), a reference per instance"""
    from zopt_amd import models
    ac = models.Quadcopter()
    uvw = np.stack([np.linspace(0.0, 4.0, 64), np.zeros(64), np.zeros(64)], -1)
    xTrim, uTrim = ac.trim(uvw)
    A, B = ac.linearize(xTrim, uTrim, dt=0.05)
    A, B = np.asarray(A), np.asarray(B)
    N, P = 20, 64
    x_ub, u_ub = np.full(8, 5.0), np.full(4, 3.0)
    Q, R = np.eye(8), np.eye(4)
    rng = np.random.default_rng(64)
    t = np.arange(N + 1)
    xRef = 7.0 * np.sin(2 * np.pi * t[None, :, None] / N + rng.uniform(0, 2 * np.pi, (P, 1, 8)))     # leaves the box (5)
    uRef = rng.uniform(-1, 1, (P, 1, 4)) * np.ones((1, N, 1))
    uRef[:, :, 0] = 6.0 * np.sign(rng.standard_normal((P, 1)))       # twice the input box (3): that input sits on its bound
    x0 = 0.1 * np.ones((P, 8))
    kw = dict(eps_abs=1e-5, eps_rel=1e-5, max_iter=4000, warm_start=False)
    prob = mpc.lqrMpc(A, B, Q, R, N, -x_ub, x_ub, -u_ub, u_ub)
    u, traj, status = prob.solve(x0, xRef=xRef, uRef=uRef, **kw)
    assert np.mean(status == "optimal") > 0.9
    for i in range(P):
        one = mpc.lqrMpc(A[i], B[i], Q, R, N, -x_ub, x_ub, -u_ub, u_ub)
        u1, t1, s1 = one.solve(x0[i], xRef=xRef[i], uRef=uRef[i], **kw)
        assert np.array_equal(traj.xTraj[i], t1.xTraj) and np.array_equal(traj.uTraj[i], t1.uTraj) and np.array_equal(u[i], u1), i
        assert status[i] == s1 and prob.last_iterations[i] == one.last_iterations, i
        assert np.array_equal(prob.last_residuals[i], one.last_residuals), i
    i = int(np.flatnonzero(status == "optimal")[0])
    xr, ur, _ = tr.solve_reference(A[i], B[i], Q, R, Q, N, -x_ub, x_ub, -u_ub, u_ub, x0[i], xRef[i], uRef[i])
    assert tr.n_active(xr, ur, -x_ub, x_ub, -u_ub, u_ub) >= 1
    assert np.max(np.abs(traj.uTraj[i] - ur)) <= 2e-3


# ---- 6. receding horizon about a moving reference -------------------------------------------------------------------------------

def _ramp_window(p0, vel, step, N, dt=0.1):
    """(B, N+1, 12) window of a position ramp p0 + vel t (positions: states 9..11, their rates: states 0..2 at hover) from MPC step `step`"""
    tt = dt * (step + np.arange(N + 1))
    xRef = np.zeros((p0.shape[0], N + 1, 12))
    xRef[:, :, 9:12] = p0[:, None, :] + vel[:, None, :] * tt[None, :, None]
    xRef[:, :, 0:3] = vel[:, None, :]
    return xRef


def test_receding_horizon_follows_a_position_ramp(mpc):
    """demos/lqrMpc.py:40-47 (clip, solve, x <- xTraj[1]) with the window of a position ramp moved at every step, warm_start="shift"."""
    N, Bn, steps, eps = 30, 64, 50, 1e-2
    data = tr.quad_data(N)
    A, B, Q, R, Qf, x_lb, x_ub, u_lb, u_ub = data
    prob = mpc.lqrMpc(A, B, Q, R, N, x_lb, x_ub, u_lb, u_ub)
    rng = np.random.default_rng(6)
    d = rng.standard_normal((Bn, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    vel = d * rng.uniform(0.2, 0.6, (Bn, 1))                     # |speed| <= 0.6 < 1: inside the velocity box
    p0 = 2.5 * d                                                 # the ramp starts 2.5 m ahead of the vehicle
    x = np.zeros((Bn, 12))
    # at least one bound is active in the independent solution of the first window
    xr, ur, _ = tr.solve_reference(A, B, Q, R, Qf, N, x_lb, x_ub, u_lb, u_ub, x[0], _ramp_window(p0, vel, 0, N)[0], np.zeros((N, 4)))
    assert tr.n_active(xr, ur, x_lb, x_ub, u_lb, u_ub) >= 1
    err = []
    for i in range(steps):
        x = np.clip(x, x_lb + 1e-6, x_ub - 1e-6)
        xRef = _ramp_window(p0, vel, i, N)
        u, traj, status = prob.solve(x, xRef=xRef, eps_abs=eps, eps_rel=eps, max_iter=4000, warm_start="shift" if i else False)
        assert np.all(status == "optimal"), (i, status)
        tol = eps + eps * max(np.max(np.abs(traj.xTraj)), np.max(np.abs(traj.uTraj))) + 1e-9    # eps_abs + eps_rel |w|
        assert np.max(np.maximum(traj.xTraj - x_ub, 0)) <= tol and np.max(np.maximum(x_lb - traj.xTraj, 0)) <= tol
        assert np.max(np.maximum(traj.uTraj - u_ub, 0)) <= tol and np.max(np.maximum(u_lb - traj.uTraj, 0)) <= tol
        err.append(np.linalg.norm(x[:, 9:12] - xRef[:, 0, 9:12], axis=1))
        x = traj.xTraj[:, 1]
    print(f"position error: first step {err[0].max():.3f} (max), last step {err[-1].max():.3f}")
    assert np.all(err[-1] < err[0])


# ---- 7. arguments -----------------------------------------------------------------------------------------------------------------

def test_reference_arguments(mpc):
    import torch
    from zopt_amd.pytrees import Trajectory
    data, x0, xRef, uRef = tr.random_case(4, 2, 6, seed=7, nb=5)
    A, B, Q, R, Qf, x_lb, x_ub, u_lb, u_ub = data
    prob = mpc.lqrMpc(A, B, Q, R, 6, x_lb, x_ub, u_lb, u_ub, Qf=Qf)
    kw = dict(eps_abs=1e-6, eps_rel=1e-6, warm_start=False)
    for bad in (dict(xRef=np.zeros((5, 6, 4))), dict(xRef=np.zeros((5, 7, 3))), dict(uRef=np.zeros((5, 7, 2))), dict(uRef=np.zeros((6,))),
                dict(xRef=np.zeros((3, 7, 4))), dict(xRef=np.zeros((5, 7, 4)), uRef=np.zeros((2, 6, 2))),
                dict(xRef=Trajectory(xRef, uRef), uRef=uRef)):
        with pytest.raises(ValueError):
            prob.solve(x0, **bad, **kw)
    with pytest.raises(TypeError):
        prob.solve(x0, xref=xRef, **kw)
    base = prob.solve(x0, xRef=xRef, uRef=uRef, **kw)
    its = prob.last_iterations.copy()
    assert isinstance(base[1].xTraj, np.ndarray) and base[1].xTraj.shape == (5, 7, 4) and base[0].shape == (5, 2)
    as_traj = prob.solve(x0, xRef=Trajectory(xRef, uRef), **kw)
    assert np.array_equal(as_traj[1].uTraj, base[1].uTraj) and np.array_equal(prob.last_iterations, its)
    # one state against a batch of references; one reference for a batch of states
    fan = prob.solve(x0[0], xRef=xRef, uRef=uRef[0], **kw)
    assert fan[1].uTraj.shape == (5, 6, 2)
    one = prob.solve(x0[0], xRef=xRef[0], uRef=uRef[0], **kw)
    assert one[2] == "optimal" and np.array_equal(fan[1].uTraj[0], one[1].uTraj)
    # device tensors stay on the device
    dev = prob.solve(torch.as_tensor(x0, device="cuda"), xRef=torch.as_tensor(xRef, device="cuda"), uRef=uRef, **kw)
    assert dev[1].xTraj.is_cuda and np.array_equal(dev[1].xTraj.cpu().numpy(), base[1].xTraj)
    # per-problem object: references broadcast against the problem shape, and must be broadcastable against it
    from tests.test_mpc_batched import _family
    fam = _family((3,), 4, 2, seed=5)
    pp = mpc.lqrMpc(*fam[:4], 6, *fam[4:])
    out = pp.solve(np.zeros(4), xRef=0.2 * xRef[0], **kw)
    assert out[2].shape == (3,) and out[1].xTraj.shape == (3, 7, 4)
    with pytest.raises(ValueError, match="inconsistent shapes"):
        pp.solve(np.zeros(4), xRef=xRef[:2], **kw)


# ---- 8. ZOPT_AMD_MPC_PATH=lane selects the lane tracking kernel ------------------------------------------------------------------

def test_forced_lane_path_in_a_child_process(mpc, tmp_path):
    """The child (tests/mpc_tracking_lane_child.py) runs the lane-per-instance tracking kernels: per-problem == single-problem bit for
    bit there too, and its shared-problem solution agrees with the 16-lane kernel's.  The lane kernel runs the fixed penalty of level0,
    the 16-lane kernel the adaptive levels, and the suite holds fixed against adaptive solutions at the default tolerance to 5e-3
    (tests/test_mpc_gpu.py: test_adaptive_rho_default_options): that bound."""
    from tests.mpc_tracking_lane_child import shared_case
    out_file = str(tmp_path / "lane.npz")
    env = dict(os.environ, ZOPT_AMD_MPC_PATH="lane")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mpc_tracking_lane_child.py"), out_file], env=env,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "MPC-TRACKING-LANE-OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    lane = np.load(out_file)
    data, x0, xRef, uRef, N = shared_case()
    prob = mpc.lqrMpc(*data[:4], N, *data[5:], Qf=data[4])
    u, traj, status = prob.solve(x0, xRef=xRef, uRef=uRef, warm_start=False)
    assert np.all(status == "optimal") and np.all(lane["status"] == "optimal")
    assert tr.n_active(traj.xTraj[0], traj.uTraj[0], *data[5:]) >= 1
    ex, eu = np.max(np.abs(lane["xTraj"] - traj.xTraj)), np.max(np.abs(lane["uTraj"] - traj.uTraj))
    print(f"lane vs 16-lane kernel: |dx| {ex:.2e} |du| {eu:.2e}; iterations {lane['iters'].max()} vs {prob.last_iterations.max()}")
    assert ex <= 5e-3 and eu <= 5e-3
    xr, ur, _ = tr.solve_reference(*data[:5], N, *data[5:], x0[0], xRef[0], uRef[0])
    assert tr.n_active(xr, ur, *data[5:]) >= 1
    assert np.max(np.abs(lane["uTraj"][0] - ur)) <= 5e-3
