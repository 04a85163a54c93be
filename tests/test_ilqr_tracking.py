"""CPU checks of the tracking cost of the fused iLQR / DDP drivers (models.TrackingCost, zm_trackcost_t): the NumPy restatement the GPU
tests compare against (tests/ilqr_tracking_ref.py) is held to the oracle loop, to a complex-step derivative and to the shifted
problem; the Python class's shapes and refusals; the sites that used to test for QuadraticCost; the C ABI's refusals."""
import ctypes

import numpy as np
import pytest

from oracle import zopt_oracle as zo
from tests import ilqr_tracking_ref as tref


def _quad_problem(T=12, seed=0):
    rng = np.random.default_rng(seed)
    x0 = np.zeros(12)
    x0[9:12] = rng.uniform(-3, 3, 3)
    ug = np.tile([9.807, 0.0, 0.0, 0.0], (T, 1))
    return x0, ug, np.eye(12), 0.5 * np.eye(4), 10 * np.eye(12)


def test_zero_reference_is_the_oracle_loop():
    """with a zero reference the restatement IS oracle.zopt_oracle.iterativeLqr: every output and the trace, with =="""
    x0, ug, Q, R, Qf = _quad_problem()
    step = zo.quad_euler_step(0.1)
    xr, ur = tref.full_reference(None, None, 12, 12, 4)
    ta, tb = [], []
    a = tref.iterativeLqr(step, Q, R, Qf, xr, ur, x0, ug, maxIter=6, return_iters=True, trace=ta)
    b = zo.iterativeLqr(step, Q, R, Qf, x0, ug, maxIter=6, return_iters=True, trace=tb)
    assert np.array_equal(a[0].xTraj, b[0].xTraj) and np.array_equal(a[0].uTraj, b[0].uTraj) and np.array_equal(a[1], b[1])
    assert a[2] == b[2] and a[3] == b[3] and a[4] == b[4] and len(ta) == len(tb) > 0
    for (Ja, ia, Jsa), (Jb, ib, Jsb) in zip(ta, tb):
        assert Ja == Jb and ia == ib and np.array_equal(Jsa, Jsb)
    # a linear model with full (nonsymmetric) weights
    rng = np.random.default_rng(3)
    A, B = np.eye(3) + 0.1 * rng.standard_normal((3, 3)), rng.standard_normal((3, 2))
    Q3, R2, Qf3 = rng.standard_normal((3, 3)), rng.standard_normal((2, 2)), rng.standard_normal((3, 3))
    Q3, R2, Qf3 = Q3 @ Q3.T + 0.3 * rng.standard_normal((3, 3)), R2 @ R2.T + np.eye(2), Qf3 @ Qf3.T
    f = lambda x, u: A @ x + B @ u
    xr, ur = tref.full_reference(None, None, 5, 3, 2)
    a = tref.iterativeLqr(f, Q3, R2, Qf3, xr, ur, rng.standard_normal(3), np.zeros((5, 2)), maxIter=4)
    b = zo.iterativeLqr(f, Q3, R2, Qf3, a[0].xTraj[0], np.zeros((5, 2)), maxIter=4)
    assert np.array_equal(a[0].uTraj, b[0].uTraj) and np.array_equal(a[1], b[1]) and a[2] == b[2]


def test_gradients_match_a_complex_step_derivative_of_the_cost():
    rng = np.random.default_rng(1)
    T, n, m = 4, 5, 2
    Q, R, Qf = rng.standard_normal((n, n)), rng.standard_normal((m, m)), rng.standard_normal((n, n))      # nonsymmetric on purpose
    xr, ur = rng.standard_normal((T + 1, n)), rng.standard_normal((T, m))
    traj = zo.Trajectory(rng.standard_normal((T + 1, n)), rng.standard_normal((T, m)))
    ex = tref.cost_expansion(Q, R, xr, ur, traj)
    h = 1e-30
    for k in range(T):
        c = tref.running_cost(Q, R, xr, ur, k)
        assert abs(ex.c[k] - c(traj.xTraj[k], traj.uTraj[k])) <= 1e-13 * max(1.0, abs(ex.c[k]))
        for j in range(n):
            xp = traj.xTraj[k].astype(complex)
            xp[j] += 1j * h
            assert abs(np.imag(c(xp, traj.uTraj[k].astype(complex))) / h - ex.c_x[k, j]) <= 1e-13 * max(1.0, np.max(np.abs(ex.c_x[k])))
        for j in range(m):
            up = traj.uTraj[k].astype(complex)
            up[j] += 1j * h
            assert abs(np.imag(c(traj.xTraj[k].astype(complex), up)) / h - ex.c_u[k, j]) <= 1e-13 * max(1.0, np.max(np.abs(ex.c_u[k])))
        assert np.array_equal(ex.c_xx[k], Q + Q.T) and np.array_equal(ex.c_uu[k], R + R.T) and not ex.c_ux[k].any()
    vf = tref.terminal_expansion(Qf, xr, traj.xTraj[-1])
    cf = tref.terminal_cost(Qf, xr)
    assert abs(vf.v - cf(traj.xTraj[-1])) <= 1e-13 * max(1.0, abs(vf.v)) and np.array_equal(vf.v_xx, Qf + Qf.T)
    for j in range(n):
        xp = traj.xTraj[-1].astype(complex)
        xp[j] += 1j * h
        assert abs(np.imag(cf(xp)) / h - vf.v_x[j]) <= 1e-13 * max(1.0, np.max(np.abs(vf.v_x)))


def test_a_position_goal_is_the_shifted_problem():
    """Still air: the quadcopter's dynamics do not read its position states 9..11, so steering to a goal in them is the problem with
    x0 - goal and no reference, shifted back.  Rollout costs at 1e-12 relative (the project's bound for like quantities)."""
    T = 10
    x0, ug, Q, R, Qf = _quad_problem(T, seed=4)
    goal = np.zeros(12)
    goal[9:12] = [1.5, -2.0, 0.7]
    step = zo.quad_euler_step(0.1)
    xr, ur = tref.full_reference(goal, zo.QUAD_G * np.array([1.0, 0, 0, 0]), T, 12, 4)
    z, uz = tref.full_reference(None, zo.QUAD_G * np.array([1.0, 0, 0, 0]), T, 12, 4)
    ta, tb = [], []
    a = tref.iterativeLqr(step, Q, R, Qf, xr, ur, x0, ug, maxIter=5, tol=0.0, trace=ta)
    b = tref.iterativeLqr(step, Q, R, Qf, z, uz, x0 - goal, ug, maxIter=5, tol=0.0, trace=tb)
    assert len(ta) == len(tb) == 5
    for (Ja, ia, Jsa), (Jb, ib, Jsb) in zip(ta, tb):
        assert ia == ib and abs(Ja - Jb) <= 1e-12 * abs(Jb) and np.max(np.abs(Jsa - Jsb) / np.abs(Jsb)) <= 1e-12
    assert np.max(np.abs(a[0].xTraj - (b[0].xTraj + goal))) <= 1e-9 and np.max(np.abs(a[0].uTraj - b[0].uTraj)) <= 1e-9
    assert a[2] < tref.trajectory_cost(Q, R, Qf, xr, ur, zo.trajectoryRollout(
        x0, step, zo.AffinePolicy(ug, np.zeros((T, 4, 12))), zo.Trajectory(np.zeros((T + 1, 12)), np.zeros((T, 4)))))


def test_TrackingCost_shapes_and_refusals():
    from zopt_amd import models
    Q, R = np.eye(3), np.eye(2)
    c = models.TrackingCost(Q, R)
    assert (c.n, c.m) == (3, 2) and c.xRef is None and c.uRef is None and np.array_equal(c.Qf, Q)
    assert not isinstance(c, models.QuadraticCost)          # code that knows only QuadraticCost must not take it for one
    c = models.TrackingCost(Q, R, 2 * Q, xRef=[1.0, 2.0, 3.0], uRef=np.ones((7, 4, 2)))
    assert c.xRef.shape == (3,) and c.uRef.shape == (7, 4, 2) and c.xRef.dtype == np.float64
    models.TrackingCost(Q, R, xRef=np.zeros((7, 1, 3)))      # a goal per trajectory: goal[:, None, :]
    for bad in (dict(xRef=np.zeros(2)), dict(xRef=np.zeros((5, 4))), dict(uRef=np.zeros(3)), dict(uRef=np.zeros((4, 0, 2))),
                dict(xRef=np.float64(1.0))):
        with pytest.raises(ValueError, match="TrackingCost"):
            models.TrackingCost(Q, R, **bad)
    with pytest.raises(ValueError):
        models.TrackingCost(Q, np.eye(3)[:2])
    # the host-side callables: the cost of a point about the reference row
    c = models.TrackingCost(Q, R, 2 * Q, xRef=np.arange(12.0).reshape(4, 3), uRef=[1.0, -1.0])
    x, u = np.array([1.0, 0.0, 2.0]), np.array([0.5, 0.5])
    assert c.runningCost(x, u, 2) == pytest.approx(np.sum((x - [6, 7, 8]) ** 2) + 0.25 + 2.25)
    assert c.terminalCost(x) == pytest.approx(2 * np.sum((x - [9, 10, 11]) ** 2))
    # beyond the fused drivers' shapes: refused with a clear message before anything touches a device
    wide = models.TrackingCost(np.eye(13), np.eye(4), xRef=np.zeros(13))
    with pytest.raises(ValueError, match=r"n <= 12, m <= 4"):
        wide.track_struct((5,), 10)
    with pytest.raises(ValueError, match=r"n <= 12, m <= 4"):
        models.TrackingCost(np.eye(4), np.eye(5)).track_struct((), 3)


def test_reference_views_broadcast_without_a_copy_per_step():
    """strides of the device view (needs no kernel, but device tensors: skipped logic on a host without a GPU is the loud failure)"""
    import torch
    from zopt_amd import _lib, models
    c = models.TrackingCost(np.eye(3), np.eye(2), xRef=np.zeros((5, 1, 3)), uRef=np.ones(2))
    if not torch.cuda.is_available():
        with pytest.raises(_lib.ZoptAmdError):
            c.track_struct((5,), 4)
        return
    st = c.track_struct((5,), 4)
    assert (st.xref_traj_stride, st.xref_step_stride, st.uref_traj_stride, st.uref_step_stride) == (3, 0, 0, 0)
    goal = torch.zeros((5, 3), dtype=torch.float64, device="cuda")
    st = models.TrackingCost(np.eye(3), np.eye(2), xRef=goal[:, None, :]).track_struct((5,), 4)
    assert st.xRef == goal.data_ptr() and st.uRef is None and (st.xref_traj_stride, st.xref_step_stride) == (3, 0)      # in place
    full = torch.zeros((5, 6, 3), dtype=torch.float64, device="cuda")
    st = models.TrackingCost(np.eye(3), np.eye(2), xRef=full[:, :5]).track_struct((5,), 4)
    assert st.xRef == full.data_ptr() and (st.xref_traj_stride, st.xref_step_stride) == (18, 3)                       # a strided view, in place
    st = models.TrackingCost(np.eye(3), np.eye(2), xRef=full[0, :5]).track_struct((5,), 4)
    assert (st.xref_traj_stride, st.xref_step_stride) == (0, 3)                                                        # one reference for all
    st = models.TrackingCost(np.eye(3), np.eye(2), xRef=full[:, :5]).track_struct((5,), 1, terminal=True)
    assert st.xRef == full.data_ptr() + 8 * 4 * 3 and st.xref_step_stride == 0                                         # the row x_T
    with pytest.raises(ValueError, match="steps"):
        models.TrackingCost(np.eye(3), np.eye(2), xRef=full).track_struct((5,), 4)
    with pytest.raises(ValueError, match="broadcast"):
        models.TrackingCost(np.eye(3), np.eye(2), xRef=full[:, :5]).track_struct((4,), 4)


def test_every_site_that_tested_for_QuadraticCost_honours_the_reference_or_raises():
    """ilqrUtils._rollout, _torch_costs, _rollout_generic, _registered_cost, pytrees._expand: none of them may silently drop a
    reference.  The two generic-callable sites raise a TypeError that names TrackingCost; _registered_cost hands the cost on to the
    fused drivers; _rollout and _expand run the tracking kernels (values: tests/test_ilqr_tracking_gpu.py) -- without a GPU they fail
    loudly instead of falling into the generic path."""
    import torch
    from zopt_amd import _lib, ilqrUtils, models, pytrees
    n, m, T = 3, 2, 4
    tc = models.TrackingCost(np.eye(n), np.eye(m), xRef=np.ones(n))
    qc = models.QuadraticCost(np.eye(n), np.eye(m))
    for args in ((tc, tc), (tc.runningCost, tc.terminalCost), (qc.runningCost, tc.terminalCost)):
        with pytest.raises(TypeError, match="TrackingCost"):
            ilqrUtils._torch_costs(*args)
    pol = pytrees.AffinePolicy(np.zeros((T, m)), np.zeros((T, m, n)))
    prev = pytrees.Trajectory(np.zeros((T + 1, n)), np.zeros((T, m)))
    with pytest.raises(TypeError, match="TrackingCost"):
        ilqrUtils._rollout_generic(np.zeros(n), lambda x, u: x, pol, prev, ilqrUtils.LINESEARCH_ALPHAS, tc)
    with pytest.raises(TypeError, match="TrackingCost"):                   # the public way into that site
        ilqrUtils.forwardPass2(np.zeros(n), lambda x, u: x, tc, pol, prev)
    with pytest.raises(TypeError, match="TrackingCost"):                   # ... and the drivers with a callable model
        ilqrUtils.iterativeLqr(lambda x, u: x, tc, tc, np.zeros(n), np.zeros((T, m)))
    assert ilqrUtils._registered_cost(tc, tc) is tc and ilqrUtils._registered_cost(tc.runningCost, tc.terminalCost) is tc
    with pytest.raises(TypeError, match="same TrackingCost"):
        ilqrUtils._registered_cost(tc.runningCost, qc.terminalCost)
    with pytest.raises(TypeError, match="TrackingCost"):
        ilqrUtils._registered_cost(lambda x, u: 0.0, lambda x: 0.0)
    model = models.LinearModel(np.eye(n), np.ones((n, m)))
    xT, uT = np.zeros((T + 1, n)), np.zeros((T, m))
    if torch.cuda.is_available():
        _, J = ilqrUtils._rollout(np.zeros(n), model, pol, prev, [1.0], tc)
        assert J == pytest.approx((T + 1) * n)                            # x stays 0, the goal is 1: not the 0 of a dropped reference
        c = pytrees._expand("cost", tc, xT, uT)[0]
        assert np.array_equal(c, np.full(T, float(n)))
        v = pytrees._expand("terminal", tc.terminalCost, xT, None)[0]
        assert np.array_equal(v, np.full(1, float(n)))
    else:
        with pytest.raises(_lib.ZoptAmdError):
            ilqrUtils._rollout(np.zeros(n), model, pol, prev, [1.0], tc)
        with pytest.raises(_lib.ZoptAmdError):
            pytrees._expand("cost", tc, xT, uT)
    with pytest.raises((TypeError, _lib.ZoptAmdError)):
        pytrees._expand("affine", tc, xT, uT)


class _Track(ctypes.Structure):
    _fields_ = [("Q", ctypes.c_void_p), ("R", ctypes.c_void_p), ("Qf", ctypes.c_void_p), ("diagonal", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("xRef", ctypes.c_void_p), ("uRef", ctypes.c_void_p), ("xts", ctypes.c_int64),
                ("xss", ctypes.c_int64), ("uts", ctypes.c_int64), ("uss", ctypes.c_int64)]


def test_c_abi_refuses_bad_arguments_without_a_gpu():
    from zopt_amd import _lib, models
    lib, d = _lib.lib(), 0x1000
    assert ctypes.sizeof(models.zm_trackcost_t) == ctypes.sizeof(_Track) == 80
    good = _Track(d, d, d, 0, 0, d, None, 12, 0, 0, 0)
    quad = models.QuadcopterEuler(0.1).c_struct()
    pm, pc = ctypes.addressof(quad), ctypes.addressof(good)

    def rollout(model=pm, cost=pc, x0=d, n_alpha=16, batch=4, T=5, J=d):
        return lib.zm_rollout_linesearch_tracking_f64(model, cost, x0, d, d, d, d, d, n_alpha, None, d, d, J, d, batch, T, None)

    def rollout_list(count, lst=d, batch=4):
        return lib.zm_rollout_linesearch_tracking_list_f64(pm, pc, d, d, d, d, d, d, 16, lst, count, None, d, d, d, d, batch, 5, None)

    def expand(cost=pc, n=12, m=4, x=d, batch=4, T=5, count=None):
        if count is None:
            return lib.zm_quadratize_cost_tracking_f64(cost, n, m, x, d, None, d, d, d, d, d, None, None, None, None, batch, T, None)
        return lib.zm_quadratize_cost_tracking_list_f64(cost, n, m, x, d, d, count, None, d, d, d, d, d, None, None, None, None, batch, T,
                                                        None)

    def solve(model=pm, cost=pc, x0=d, ws=d, nws=1 << 40, batch=4, T=5, max_iter=3, sync=4, trace=False):
        common = (model, cost, x0, d, 0, max_iter, 1e-3, sync, ws, nws, d, d, d, d, d, d, None, batch, T, None)
        return lib.zm_ilqr_solve_tracking_trace_f64(*common, d, d) if trace else lib.zm_ilqr_solve_tracking_f64(*common)

    # the cost record
    for fn in (rollout, expand, solve):
        assert fn(cost=None) == _lib.ZM_EINVAL and b"tracking cost needs Q, R, Qf" in lib.zm_last_error()
        for hole in ("Q", "R", "Qf"):
            bad = _Track(d, d, d, 0, 0, d, d, 12, 0, 4, 0)
            setattr(bad, hole, None)
            assert fn(cost=ctypes.addressof(bad)) == _lib.ZM_EINVAL, hole
        for stride in ("xts", "xss", "uts", "uss"):
            bad = _Track(d, d, d, 0, 0, d, d, 12, 0, 4, 0)
            setattr(bad, stride, -1)
            assert fn(cost=ctypes.addressof(bad)) == _lib.ZM_EINVAL and b"negative reference stride" in lib.zm_last_error(), stride
    # null pointers, sizes
    assert rollout(model=None) == _lib.ZM_EINVAL and rollout(x0=None) == _lib.ZM_EINVAL and b"null pointer" in lib.zm_last_error()
    assert rollout(n_alpha=0) == _lib.ZM_EINVAL and rollout(n_alpha=17) == _lib.ZM_EINVAL and rollout(batch=-1) == _lib.ZM_EINVAL
    assert rollout(T=-1) == _lib.ZM_EINVAL and rollout(batch=0, x0=None) == _lib.ZM_OK
    assert rollout_list(5) == _lib.ZM_EINVAL and b"bad list length" in lib.zm_last_error() and rollout_list(-1) == _lib.ZM_EINVAL
    assert rollout_list(0) == _lib.ZM_OK
    assert expand(x=None) == _lib.ZM_EINVAL and expand(T=0) == _lib.ZM_EINVAL and expand(batch=-1) == _lib.ZM_EINVAL
    assert expand(count=5) == _lib.ZM_EINVAL and expand(count=-1) == _lib.ZM_EINVAL
    assert solve(model=None) == _lib.ZM_EINVAL and solve(x0=None) == _lib.ZM_EINVAL and solve(ws=None) == _lib.ZM_EINVAL
    assert solve(T=0) == _lib.ZM_EINVAL and solve(batch=-1) == _lib.ZM_EINVAL and solve(max_iter=-1) == _lib.ZM_EINVAL
    assert solve(sync=0) == _lib.ZM_EINVAL and solve(trace=True, x0=None) == _lib.ZM_EINVAL
    assert solve(nws=8) == _lib.ZM_EINVAL and b"workspace" in lib.zm_last_error()
    assert solve(batch=0, x0=None) == _lib.ZM_OK
    # shapes: the tracking cost stops at n <= 12, m <= 4 -- the wide linear rollouts have no tracking form
    wide = models.zm_model_t(models.ZM_MODEL_LINEAR, 24, 8, 0, 0.0, d, d)
    pw = ctypes.addressof(wide)
    assert rollout(model=pw) == _lib.ZM_EUNSUPPORTED and b"tracking cost: n<=12, m<=4" in lib.zm_last_error()
    assert solve(model=pw) == _lib.ZM_EUNSUPPORTED and b"tracking cost: n<=12, m<=4" in lib.zm_last_error()
    assert expand(n=13) == _lib.ZM_EUNSUPPORTED and expand(m=5) == _lib.ZM_EUNSUPPORTED and expand(n=0) == _lib.ZM_EUNSUPPORTED
    unknown = models.zm_model_t(9, 12, 4, 0, 0.1, None, None)
    assert rollout(model=ctypes.addressof(unknown)) == _lib.ZM_EUNSUPPORTED
