"""CPU tests of stage-varying input bounds (models.InputBox(..., stage_varying=True); zm_inputbox_t.step_stride): shapes, broadcasts and
refusals of the Python surface, the C ABI's refusal of bad (stride, step_stride) pairs from host code, the stage restatement
tests/ilqr_box_stage_ref.py against the constant one (bit for bit with constant rows) and against an independent SciPy solve on convex
cases, and the properties of every case the GPU file (tests/test_ilqr_box_stage_gpu.py) relies on: strict-complementarity margins of
the sweeps, a determined line search in every iteration of the solves.  No GPU."""
import ctypes
import warnings

import numpy as np
import pytest

from oracle import zopt_oracle as zo
from tests import ddp_box_cases as dbc
from tests import ddp_box_ref as dr
from tests import ilqr_box_cases as ibc
from tests import ilqr_box_ref as br
from tests import ilqr_box_stage_ref as sr
from tests import ilqr_tracking_ref as tref

INF = np.inf


def _lin(n=3, m=2):
    from zopt_amd import models
    return models.LinearModel(np.eye(n), np.ones((n, m)))


# ------------------------------------------------------------------------------------------------------------------------------- 1
def test_stage_varying_is_a_new_argument():
    """fails without the feature: the parent's InputBox takes no `stage_varying`"""
    from zopt_amd import models
    box = models.InputBox(_lin(), -np.ones((5, 2)), np.ones((5, 2)), stage_varying=True)
    assert box.stage_varying and box.steps == 5 and box.u_lb.shape == (5, 2)
    plain = models.InputBox(_lin(), -1.0, 1.0)
    assert not plain.stage_varying and plain.u_lb.shape == (2,)          # stage_varying=False is today's object


def test_shapes_and_broadcasts():
    from zopt_amd import models
    lin = _lin()
    T, m = 4, 2
    rng = np.random.default_rng(1)
    ub = rng.uniform(0.5, 1, (T, m))
    b = models.InputBox(lin, -INF, ub, stage_varying=True)              # a scalar next to a (T, m) array
    assert b.u_lb.shape == (T, m) and np.all(b.u_lb == -INF) and np.array_equal(b.u_ub, ub)
    b = models.InputBox(lin, -ub[None].repeat(3, 0), ub, stage_varying=True)      # (3, T, m) next to (T, m)
    assert b.u_lb.shape == (3, T, m) and b.steps == T
    b = models.InputBox(lin, -ub[None, None] * np.ones((2, 1, 1, 1)), ub[None] * np.ones((3, 1, 1)), stage_varying=True)
    assert b.u_lb.shape == (2, 3, T, m)
    pinned = models.InputBox(lin, ub, ub, stage_varying=True)           # lb == ub per entry is allowed
    u = rng.standard_normal((6, T, m))
    assert np.array_equal(pinned.clip(u), np.broadcast_to(ub, (6, T, m)))
    box = models.InputBox(lin, -ub, ub, stage_varying=True)
    assert np.array_equal(box.clip(u), np.minimum(np.maximum(u, -ub), ub))       # clip broadcasts over the step axis
    import torch
    tb = models.InputBox(lin, torch.as_tensor(-ub), torch.as_tensor(ub), stage_varying=True)
    assert np.array_equal(tb.u_ub, ub)
    s = models.InputBox.for_shape(3, 2, -ub, ub, stage_varying=True)
    assert s.model is None and s.steps == T


def test_refusals():
    from zopt_amd import models
    lin = _lin()
    T, m = 4, 2
    lb, ub = -np.ones((T, m)), np.ones((T, m))
    bad = lb.copy()
    bad[2, 1] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        models.InputBox(lin, bad, ub, stage_varying=True)
    bad = lb.copy()
    bad[2, 1] = 2.0
    with pytest.raises(ValueError, match="u_lb > u_ub at step 2"):
        models.InputBox(lin, bad, ub, stage_varying=True)
    with pytest.raises(ValueError, match="step axis"):
        models.InputBox(lin, -1.0, 1.0, stage_varying=True)
    with pytest.raises(ValueError, match=r"expected a scalar, \(N, 2\)"):
        models.InputBox(lin, -np.ones(m), ub, stage_varying=True)       # (m,) has no step axis
    with pytest.raises(ValueError, match="expected a scalar"):
        models.InputBox(lin, -np.ones((T, 3)), ub, stage_varying=True)
    with pytest.raises(ValueError, match="4 steps and u_ub 5"):
        models.InputBox(lin, lb, np.ones((5, m)), stage_varying=True)
    box = models.InputBox(lin, lb, ub, stage_varying=True)
    with pytest.raises(ValueError, match="4 steps.*horizon of 7"):       # names both lengths, before anything touches the device
        box.box_struct((3,), 7)
    with pytest.raises(ValueError, match="4 steps.*horizon of None"):
        box.box_struct((3,))
    with pytest.raises(TypeError, match="stage-varying InputBox inside a StateBox is the follow-up"):
        models.StateBox(box, -1.0, 1.0)
    models.StateBox(models.InputBox(lin, -1.0, 1.0), -1.0, 1.0)          # the constant box inside a StateBox stays accepted


def test_a_wrong_horizon_is_refused_by_the_drivers_before_the_device():
    from zopt_amd import ilqrUtils, models, pytrees
    lin = _lin()
    cost = models.QuadraticCost(np.eye(3), np.eye(2))
    box = models.InputBox(lin, -np.ones((4, 2)), np.ones((4, 2)), stage_varying=True)
    z = lambda *s: np.zeros(s)      # noqa: E731
    with pytest.raises(ValueError, match="4 steps.*horizon of 6"):
        ilqrUtils.trajectoryRollout(z(3), box, pytrees.AffinePolicy(z(6, 2), z(6, 2, 3)), pytrees.Trajectory(z(7, 3), z(6, 2)))
    with pytest.raises(ValueError, match="4 steps.*horizon of 6"):
        ilqrUtils.forwardPass2(z(3), box, cost, pytrees.AffinePolicy(z(6, 2), z(6, 2, 3)), pytrees.Trajectory(z(7, 3), z(6, 2)))
    dyn, cst, Vf = (None, z(6, 3, 3), z(6, 3, 2)), (None, z(6, 3), z(6, 2), z(6, 3, 3), z(6, 2, 3), z(6, 2, 2)), (None, z(3), z(3, 3))
    with pytest.raises(ValueError, match="4 steps.*horizon of 6"):
        ilqrUtils.backwardPass_ilqr_box(dyn, cst, Vf, z(6, 2), -np.ones((4, 2)), np.ones((4, 2)), stage_varying=True)


# ------------------------------------------------------------------------------------------------------------------------------- 2
def test_the_struct_mirror_and_three_field_callers():
    from zopt_amd import models
    assert [f[0] for f in models.zm_inputbox_t._fields_] == ["lb", "ub", "stride", "step_stride"]
    assert ctypes.sizeof(models.zm_inputbox_t) == 32
    assert models.zm_inputbox_t(1, 2, 3).step_stride == 0                # a struct built from three fields: the constant form


def test_the_c_abi_refuses_bad_stride_pairs_before_any_launch():
    """(stride, step_stride): every pair but (0 | m, 0) and (0 | T m, m) is ZM_EINVAL from host code, in the sweeps (whose last check
    before the launch is the box's) and in the line search; the four good pairs pass the line search's box check, which then refuses
    the call for a later reason.  Fake pointers: no check dereferences them, nothing is launched."""
    from zopt_amd import _lib, models
    lib = _lib.lib()
    p = ctypes.addressof((ctypes.c_double * 2)())
    T, n, m = 4, 12, 4
    box = lambda stride, step: ctypes.addressof(_keep(models.zm_inputbox_t(p, p, stride, step)))      # noqa: E731
    held = []

    def _keep(s):
        held.append(s)
        return s

    ilqr = lambda bx: lib.zm_ilqr_backward_box_list_f64(p, p, p, p, p, p, p, p, p, p, bx, None, 0, None, 0, p, p, None, 4, T, n, m, None)      # noqa: E731
    ddp = lambda bx: lib.zm_ddp_backward_box_list_f64(p, p, p, p, p, p, p, p, p, p, p, p, p, bx, None, 0, None, 0, p, p, None, 4, T, n, m,      # noqa: E731
                                                      None)
    md = models.QuadcopterEuler(0.1).c_struct()                   # (12, 4); its struct needs no device
    ls = lambda bx: lib.zm_rollout_linesearch_box_list_f64(ctypes.addressof(md), None, None, bx, p, p, p, p, p, p, 16, p, 0, None, p, p, p,      # noqa: E731
                                                           None, 4, T, None)
    good = [(0, 0), (m, 0), (0, m), (T * m, m)]
    bad = [(m, m), (T * m, 0), (3, 0), (0, 1), (0, T * m), (T * m + 1, m), (m, 2 * m), (-m, m), (0, -m)]
    for stride, step in bad:
        for call in (ilqr, ddp, ls):
            assert call(box(stride, step)) == _lib.ZM_EINVAL, (stride, step)
            msg = lib.zm_last_error()
            assert b"box stride" in msg or b"step_stride" in msg, (stride, step, msg)
    for stride, step in good:
        assert ls(box(stride, step)) == _lib.ZM_EINVAL and b"needs a cost" in lib.zm_last_error()      # 16 step sizes without a cost
    # the state entries take the constant form only
    sb = models.zm_statebox_t(p, p, 0, p, p, p)
    rc = lib.zm_ilqr_backward_state_list_f64(p, p, p, p, p, p, p, p, p, p, p, box(0, m), None, 0, None, 0, p, p, None, 4, T, n, m, None)
    assert rc == _lib.ZM_EUNSUPPORTED and b"stage-varying input bounds" in lib.zm_last_error()
    cs = models.zm_quadcost_t(p, p, p, 0)
    rc = lib.zm_rollout_linesearch_state_list_f64(ctypes.addressof(md), ctypes.addressof(cs), None, box(T * m, m), ctypes.addressof(sb), p, p,
                                                  p, p, p, p, 16, None, 0, None, p, p, p, None, None, 4, T, None)
    assert rc == _lib.ZM_EUNSUPPORTED and b"stage-varying input bounds" in lib.zm_last_error()


# ------------------------------------------------------------------------------------------------------------------------------- 3
def test_constant_rows_give_the_constant_restatement_bit_for_bit():
    """the stage restatement with the same row at every step against tests/ilqr_box_ref.py / tests/ddp_box_ref.py: sweeps (fp64 and
    long double), line search, iLQR and DDP solves"""
    for shape in ((3, 2, 5, 9, True), (8, 4, 2, 9, True), (12, 4, 7, 9, False)):
        dyn, cost, Vf, u, lb, ub = ibc.sweep_case("cheap", *shape)["args"]
        T = shape[2]
        tile = lambda b: np.repeat(np.expand_dims(b, -2), T, axis=-2)      # noqa: E731
        for ld in (False, True):
            a, b = sr.box_backward_batch(dyn, cost, Vf, u, tile(lb), tile(ub), ld), br.box_backward_batch(dyn, cost, Vf, u, lb, ub, ld)
            for k in a:
                assert np.array_equal(a[k], b[k]), (shape, ld, k)
    for shape in ((3, 2, 5, 5, True), (12, 4, 3, 5, True)):
        dyn, cost, Vf, u, lb, ub = dbc.sweep_case("plain", *shape)["args"]
        T = shape[2]
        tile = lambda b: np.repeat(np.expand_dims(b, -2), T, axis=-2)      # noqa: E731
        a, b = sr.ddp_box_backward(dyn, cost, Vf, u, tile(lb), tile(ub)), dr.ddp_box_backward(dyn, cost, Vf, u, lb, ub)
        for k in a:
            assert np.array_equal(a[k], b[k]), (shape, k)
    for name in ("lin3", "quad_hover"):
        c = ibc.solve_case(name)
        B, T, m = c["ug"].shape
        n = c["x0"].shape[-1]
        for b in (0, 3):
            xr, ur = tref.full_reference(c["xRef"], c["uRef"], T, n, m, b)
            ta, tb = [], []
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                x = sr.solve(c["step"], c["Q"], c["R"], c["Qf"], c["x0"][b], c["ug"][b], np.tile(c["lb"], (T, 1)), np.tile(c["ub"], (T, 1)), xr, ur,
                             trace=ta, **c["kw"])
                y = br.iterativeLqr(c["step"], c["Q"], c["R"], c["Qf"], c["x0"][b], c["ug"][b], c["lb"], c["ub"], xr, ur, return_iters=True,
                                    trace=tb, **c["kw"])
            assert np.array_equal(x[0].xTraj, y[0].xTraj) and np.array_equal(x[0].uTraj, y[0].uTraj) and np.array_equal(x[1], y[1])
            assert x[2] == y[2] and x[3] == y[3] and x[4] == y[4]
            assert all(p[0] == q[0] and p[1] == q[1] and np.array_equal(p[2], q[2]) for p, q in zip(ta, tb))
    c = dbc.solve_case("quad_hover")
    B, T, m = c["ug"].shape
    xr, ur = tref.full_reference(c["xRef"], c["uRef"], T, 12, m, 1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        x = sr.solve(c["step"], c["Q"], c["R"], c["Qf"], c["x0"][1], c["ug"][1], np.tile(c["lb"], (T, 1)), np.tile(c["ub"], (T, 1)), xr, ur,
                     f_torch=c["torch"], maxIter=2)
        y = dr.differentialDynamicProgramming_box(c["step"], c["torch"], c["Q"], c["R"], c["Qf"], c["x0"][1], c["ug"][1], c["lb"], c["ub"], xr, ur,
                                                  maxIter=2, return_iters=True)
    assert np.array_equal(x[0].uTraj, y[0].uTraj) and np.array_equal(x[1], y[1]) and x[2] == y[2]


# ------------------------------------------------------------------------------------------------------------------------------- 4
def _scipy_solve(A, B, Q, R, Qf, x0, lb, ub):
    """min sum_k x_k'Q x_k + u_k'R u_k + x_N'Qf x_N over lb_k <= u_k <= ub_k for x+ = A x + B u, as a bounded linear least-squares
    problem in the stacked inputs (scipy.optimize.lsq_linear); pinned entries (lb == ub) are eliminated"""
    from scipy.optimize import lsq_linear
    N, m = lb.shape
    n = x0.shape[0]
    Phi = np.stack([np.linalg.matrix_power(A, k) for k in range(N + 1)])                     # x_k = Phi_k x0 + sum_j A^(k-1-j) B u_j
    G = np.zeros((N + 1, n, N, m))
    for k in range(1, N + 1):
        for j in range(k):
            G[k, :, j] = Phi[k - 1 - j] @ B
    sq = lambda M: np.linalg.cholesky(M).T      # noqa: E731
    rows_x = np.concatenate([(sq(Q if k < N else Qf) @ G[k].reshape(n, N * m)) for k in range(N + 1)])
    rhs_x = -np.concatenate([sq(Q if k < N else Qf) @ Phi[k] @ x0 for k in range(N + 1)])
    M = np.concatenate([rows_x, np.kron(np.eye(N), sq(R))])
    y = np.concatenate([rhs_x, np.zeros(N * m)])
    lo, hi = lb.reshape(-1), ub.reshape(-1)
    pinned = lo == hi
    u = np.where(pinned, lo, 0.0)
    free = ~pinned
    res = lsq_linear(M[:, free], y - M[:, pinned] @ u[pinned], bounds=(lo[free], hi[free]), method="bvls", tol=1e-14, max_iter=500)
    u[free] = res.x
    return u.reshape(N, m)


@pytest.mark.parametrize("case", ibc.CONVEX_CASES, ids=lambda c: f"n{c[0]}m{c[1]}")
def test_convex_cases_against_scipy(case):
    """a linear model, a quadratic cost and a schedule of bounds (two pinned steps, a ceiling that drops halfway, an infinite side):
    the stage restatement's solve against the bounded least-squares solve of the condensed problem"""
    n, m, N, seed, box = case
    c = ibc.convex_case(*case)
    rng = np.random.default_rng(seed + 50)
    lb, ub = np.tile(c["lb"], (N, 1)), np.tile(c["ub"], (N, 1))
    lb[:2] = ub[:2] = rng.uniform(-0.3, 0.3, (2, m))
    ub[N // 2:, :m - 1] *= 0.4
    lb[N // 2:, 0] = -INF
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        traj, L, J, conv, its = sr.solve(lambda x, u: c["A"] @ x + c["B"] @ u, c["Q"], c["R"], c["Qf"], c["x0"], c["ug"], lb, ub, tol=c["tol"])
    want = _scipy_solve(c["A"], c["B"], c["Q"], c["R"], c["Qf"], c["x0"], lb, ub)
    assert conv and np.all(traj.uTraj >= lb) and np.all(traj.uTraj <= ub)
    assert np.array_equal(traj.uTraj[:2], lb[:2])
    assert np.max(np.abs(traj.uTraj - want)) <= 1e-7 * max(1.0, np.max(np.abs(want))), np.max(np.abs(traj.uTraj - want))
    at = (traj.uTraj == lb) | (traj.uTraj == ub)
    assert at[2:].any() and not at[2:].all()                           # the schedule binds somewhere beyond the pinned steps, not everywhere


# ------------------------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("family", ibc.SWEEP_FAMILIES)
def test_sweep_cases_have_a_margin(family):
    """every step of every iLQR sweep case of the GPU file: a strict-complementarity margin, fp64 and long double agree on the clamped
    sets, the rows differ along the horizon and uTraj is feasible in its own step's box"""
    clamped = 0
    for shape in sr.SWEEP_SHAPES:
        c = sr.sweep_case(family, *shape)
        u, lb, ub = c["args"][3:]
        assert c["ref"]["margin"].min() >= ibc.MARGIN and c["same64"], (family, shape)
        assert np.all(u >= lb) and np.all(u <= ub)
        if shape[2] > 1:
            assert np.any(lb[..., 0, :] != lb[..., 1, :])
        clamped += int(np.count_nonzero(c["ref"]["clamped"]))
    assert clamped > 0


@pytest.mark.parametrize("family", sr.DDP_SWEEP_FAMILIES)
def test_ddp_sweep_cases_have_a_margin_and_stable_sets(family):
    """the DDP sweep cases: the margin, and clamped sets that the projection's resolution cannot move (tests/test_ddp_box.py's rule)"""
    for shape in sr.ddp_family_shapes(family):
        c = sr.sweep_case(family, *shape, ddp=True)
        u, lb, ub = c["args"][3:]
        assert c["ref"]["margin"].min() >= dbc.MARGIN and c["same64"] and c["stable"], (family, shape)
        assert np.all(u >= lb) and np.all(u <= ub)


@pytest.mark.parametrize("case", sr.SOLVE_CASES, ids=lambda c: f"{c[0]}-{'ddp' if c[1] else 'ilqr'}")
def test_solve_cases_have_a_determined_line_search(case):
    """every iteration of every trajectory of the solve cases: the best two of the 16 costs are COST_GAP apart and every backward step
    has its margin -- decided here, by the restatement alone, so that the GPU file follows the trace without skipping anything; the
    first two inputs are the pinned ones and the schedule binds beyond them somewhere"""
    name, ddp = case
    c = sr.solve_case(name, ddp)
    beyond = 0
    refs = sr.solve_reference(name, ddp)
    assert len(refs) >= 3
    if name != "lin3":       # run to convergence, over several iterations
        assert all(r["converged"] and r["its"] >= 2 for r in refs), [r["its"] for r in refs]
        assert max(r["its"] for r in refs) >= 3 or case == ("quad_hover", False), [r["its"] for r in refs]
    for b, r in enumerate(refs):
        assert r["its"] >= 1
        for J_new, idx, Js, masks, margins in r["trace"]:
            assert sr.cost_gap(Js) >= sr.COST_GAP, (case, b, sr.cost_gap(Js))
            assert margins.min() >= ibc.MARGIN, (case, b)
            assert Js[idx] == J_new
        u = r["traj"].uTraj
        assert np.all(u >= c["lb"][b]) and np.all(u <= c["ub"][b])
        assert np.array_equal(u[:2], c["lb"][b][:2]) and np.array_equal(c["lb"][b][:2], c["ub"][b][:2])
        beyond += int(np.count_nonzero((u[2:] == c["lb"][b][2:]) | (u[2:] == c["ub"][b][2:])))
    assert beyond > 0, case
