"""CPU tests of the state box (iLQR with state bounds by an augmented-Lagrangian outer loop): the NumPy restatement
tests/ilqr_state_ref.py against SciPy on convex cases and against the restatements without state bounds; the margins of every solve
case the GPU tests use (tests/ilqr_state_cases.py); the host layer -- symbols, argument checks, refusals, StateBox broadcasting.
No GPU."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest

from tests import ilqr_box_ref as br
from tests import ilqr_state_cases as cases
from tests import ilqr_state_ref as sref
from tests import ilqr_tracking_ref as tref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.inf
NEW_SYMBOLS = ("zm_rollout_linesearch_state_f64", "zm_rollout_linesearch_state_list_f64", "zm_state_penalty_expand_list_f64",
               "zm_ilqr_backward_state_f64", "zm_ilqr_backward_state_list_f64", "zm_state_multiplier_update_f64",
               "zm_ilqr_solve_state_workspace_f64", "zm_ilqr_solve_state_f64", "zm_ilqr_solve_state_trace_f64")
# The distance of the restatement's inputs to SciPy's (SLSQP on the condensed QP), max |u - u_scipy| over the ten cases at the tight
# settings: measured 2.0e-07 (stable5 without input bounds; the others 3e-9 .. 1.6e-7) -- SLSQP's own accuracy at the tolerance it can
# resolve.  The bound is ten times that.
SCIPY_DISTANCE = 2.0e-6


def test_the_new_symbols_are_in_the_header_the_library_and_the_ctypes_table():
    from zopt_amd import _lib, ilqrUtils, models
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zopt_amd.h")).read(), flags=re.S)
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} not declared in include/zopt_amd.h"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in _lib.SYMBOLS, f"{name} has no ctypes signature"
    assert "typedef struct zm_statebox_t" in hdr
    assert [f[0] for f in models.zm_statebox_t._fields_] == ["lb", "ub", "stride", "lam_lb", "lam_ub", "mu"]
    assert callable(ilqrUtils.constrainedIterativeLqr) and ilqrUtils.ConstraintInfo._fields == (
        "violation", "mu", "lam_lb", "lam_ub", "outerIterations", "innerIterations")
    import inspect
    assert list(inspect.signature(ilqrUtils.constrainedIterativeLqr).parameters) == list(inspect.signature(ilqrUtils.iterativeLqr).parameters)
    d = inspect.signature(models.StateBox.__init__).parameters
    assert [d[k].default for k in ("mu0", "growth", "mu_max", "outer", "ctol")] == [1.0, 10.0, 1e8, 10, 1e-4]


@pytest.mark.parametrize("name", cases.QP_NAMES)
@pytest.mark.parametrize("boxed", [False, True])
def test_restatement_against_scipy(name, boxed):
    """tight settings (tol = 1e-10, ctol = 1e-8, outer = 20) on a QP: done; feasible to ctol; the multipliers are >= 0 and positive
    only on (nearly) active bounds, never on both sides of a component with lb < ub; the Lagrangian with the returned multipliers is
    stationary in the inputs (projected onto the input box) up to what the inner tolerance and the last multiplier step allow:
    sqrt(2 tol lambda_max) + mu max(violation, active gap) |Su|_1; and the inputs are SciPy's to SCIPY_DISTANCE"""
    p = cases.qp_problem(name)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        o = cases.qp_restatement(name, boxed, True)
        us, xs = cases.qp_scipy(name, boxed)
    assert o["converged"] and o["violation"] <= cases.TIGHT["ctol"]
    x, u = o["traj"].xTraj[1:], o["traj"].uTraj
    lu, ll = o["lam_ub"], o["lam_lb"]
    assert np.all(lu >= 0) and np.all(ll >= 0) and not lu[0].any() and not ll[0].any()
    assert not np.any((lu > 0) & (ll > 0) & (p["x_lb"] < p["x_ub"]))
    gap = max(np.max(np.where(lu[1:] > 0, np.abs(x - p["x_ub"]), 0.0)), np.max(np.where(ll[1:] > 0, np.abs(x - p["x_lb"]), 0.0)))
    scale = np.max(np.abs(x))
    assert gap <= 10 * cases.TIGHT["ctol"] * max(scale, 1.0), gap                     # complementarity
    Sx, Su, H, f = cases.condensed(p)
    grad = 2 * (H @ u.ravel() + f) + Su.T @ (lu - ll)[1:].ravel()
    if boxed:
        assert np.all(u >= p["u_lb"]) and np.all(u <= p["u_ub"])
        at_l, at_u = (u <= p["u_lb"]).ravel(), (u >= p["u_ub"]).ravel()
        grad = np.where(at_l, np.minimum(grad, 0.0), np.where(at_u, np.maximum(grad, 0.0), grad))
    allow = np.sqrt(2 * cases.TIGHT["tol"] * np.linalg.eigvalsh(2 * H)[-1]) + o["mu"] * max(o["violation"], gap) * np.max(np.sum(np.abs(Su), axis=0))
    dist = float(np.max(np.abs(u - us)))
    print(f"state box {name} boxed={boxed}: outer {o['outer']} inner {o['inner']} violation {o['violation']:.2e} mu {o['mu']:.0e} "
          f"active {int((lu > 0).sum() + (ll > 0).sum())} stationarity {np.max(np.abs(grad)):.2e} (allowed {allow:.2e}) distance to SciPy {dist:.2e}")
    assert np.max(np.abs(grad)) <= allow
    assert dist <= SCIPY_DISTANCE


def test_the_convex_cases_touch_their_bounds():
    """every family has active state bounds, and the double integrator's wall is active on several steps and its input bound too"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for name in cases.QP_NAMES:
            o = cases.qp_restatement(name, False, True)
            assert (o["lam_ub"] > 0).sum() + (o["lam_lb"] > 0).sum() >= 1, name
        o = cases.qp_restatement("dint", True, True)
    p = cases.qp_problem("dint")
    assert (o["lam_ub"][:, 1] > 0).sum() >= 5 and np.any(o["traj"].uTraj == p["u_ub"])


@pytest.mark.parametrize("name", ["dint", "unstable5", "stable12"])
def test_infinite_bounds_follow_the_restatements_without_state_bounds(name):
    """infinite state bounds: one outer iteration whose inner solve is tests/ilqr_tracking_ref.iterativeLqr (no input bounds) or
    tests/ilqr_box_ref.iterativeLqr (with them) iterate by iterate -- the same J (bits), the same step index, the same inputs"""
    p = cases.qp_problem(name)
    n, m = p["B"].shape
    step = lambda x, u: p["A"] @ x + p["B"] @ u                                        # noqa: E731
    ug = np.zeros((p["T"], m))
    xr, ur = np.zeros((p["T"] + 1, n)), np.zeros((p["T"], m))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for boxed in (False, True):
            tr, tq = [], []
            o = sref.constrainedIterativeLqr(step, p["Q"], p["R"], p["Qf"], p["x0"], ug, np.full(n, -INF), np.full(n, INF),
                                             u_lb=p["u_lb"] if boxed else None, u_ub=p["u_ub"] if boxed else None, trace=tr)
            if boxed:
                q = br.iterativeLqr(step, p["Q"], p["R"], p["Qf"], p["x0"], ug, p["u_lb"], p["u_ub"], return_iters=True, trace=tq)
            else:
                q = tref.iterativeLqr(step, p["Q"], p["R"], p["Qf"], xr, ur, p["x0"], ug, return_iters=True, trace=tq)
            assert o["outer"] == 1 and o["inner"] == [q[4]] and o["converged"] == q[3] and o["violation"] == 0.0 and o["mu"] == 1.0
            assert [(it["J"], it["idx"]) for it in tr[0]["inner"]] == [(t[0], t[1]) for t in tq]
            assert o["J"] == q[2] and np.array_equal(o["traj"].uTraj, q[0].uTraj) and not o["lam_ub"].any() and not o["lam_lb"].any()


GPU_SCALES = (1.0, 0.6, 0.0)       # tests/test_ilqr_state_gpu.py: SCALES


@pytest.mark.parametrize("name,boxed", cases.SOLVE_CASES)
def test_case_hygiene(name, boxed):
    """every solve case the GPU file compares exactly, over all iterations of the restatement: |s_ub|, |s_lb| of finite bounds are
    >= 1e-7 (1 + mu); the inner test |dJ| - tol and the outer test viol - ctol are 1e-6 relative away from zero; the best and the
    second-best of the 16 costs are 1e-9 relative apart in every iteration that moves -- the confirming iteration of a
    linear-quadratic inner solve has a zero step, its 16 rollouts coincide (J moves by less than 1e-12 relative) and any index names
    the same trajectory, which is what the GPU file then asks for"""
    p = cases.qp_problem(name)
    m = p["B"].shape[1]
    for s in GPU_SCALES:
        tr = []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            o = sref.constrainedIterativeLqr(lambda x, u: p["A"] @ x + p["B"] @ u, p["Q"], p["R"], p["Qf"], s * p["x0"], np.zeros((p["T"], m)),
                                             p["x_lb"], p["x_ub"], u_lb=p["u_lb"] if boxed else None, u_ub=p["u_ub"] if boxed else None,
                                             trace=tr, **cases.LOOSE)
        o["trace"] = tr
        _, smin, test = cases.margins(o, p["x_lb"], p["x_ub"], cases.LOOSE["tol"], cases.LOOSE["ctol"])
        assert smin >= 1e-7 and test >= 1e-6, (name, boxed, s, smin, test)
        for out in tr:
            for it in out["inner"]:
                srt = np.sort(it["Js"])
                if srt[1] - srt[0] < 1e-9 * abs(srt[0]) or srt[0] == 0.0:
                    assert it["dJ"] <= 1e-12 * max(abs(it["J"]), 1.0), (name, boxed, s, it["dJ"])
                    assert np.max(it["Js"]) - srt[0] <= 1e-9 * max(abs(srt[0]), 1e-300) or srt[0] == 0.0


def _model12():
    from zopt_amd import models
    return models.LinearModel(np.eye(3), np.ones((3, 2)))


def test_statebox_broadcasting_strides_and_refusals():
    from zopt_amd import ilqrUtils, models, pytrees
    model = _model12()
    sb = models.StateBox(model, -1.0, np.array([1.0, INF, 2.0]))
    assert sb.x_lb.shape == (3,) and sb.bounds_rows((4,))[2] == 0 and sb.bounds_rows(())[2] == 0
    per = models.StateBox(model, -np.ones((4, 1, 3)), np.ones(3))
    lb, ub, stride = per.bounds_rows((4, 2))
    assert stride == 3 and lb.shape == (8, 3) and ub.shape == (8, 3) and lb.flags.writeable
    with pytest.raises(ValueError, match="do not broadcast to the batch"):
        per.bounds_rows((5, 2))
    for bad in ((-np.ones(2), np.ones(3)), (np.ones(3), -np.ones(3)), (np.array([np.nan, 0, 0]), np.ones(3))):
        with pytest.raises(ValueError):
            models.StateBox(model, *bad)
    for kw in (dict(mu0=0.0), dict(growth=0.5), dict(outer=0), dict(mu_max=0.1), dict(ctol=-1.0)):
        with pytest.raises(ValueError):
            models.StateBox(model, -1.0, 1.0, **kw)
    models.StateBox(model, np.zeros(3), np.zeros(3))                                   # lb == ub is allowed
    inner = models.InputBox(model, -1.0, 1.0)
    assert models.StateBox(inner, -1.0, 1.0).model is inner
    with pytest.raises(TypeError, match="outer wrapper"):
        models.InputBox(sb, -1.0, 1.0)
    with pytest.raises(TypeError):
        models.StateBox(sb, -1.0, 1.0)
    with pytest.raises(TypeError, match="registered device model"):
        models.StateBox(lambda x, u: x, -1.0, 1.0)                                     # a torch-callable model
    cost = models.QuadraticCost(np.eye(3), np.eye(2), np.eye(3))
    x0, ug = np.zeros(3), np.zeros((4, 2))
    # refused before the device is touched (this machine has none: anything later would raise ZoptAmdError)
    with pytest.raises(ValueError, match="follow-up"):
        ilqrUtils.differentialDynamicProgramming(sb, cost, cost, x0, ug)
    with pytest.raises(ValueError, match="penalty"):
        ilqrUtils.forwardPass2(x0, sb, cost, pytrees.AffinePolicy(ug, np.zeros((4, 2, 3))), pytrees.Trajectory(np.zeros((5, 3)), ug))
    with pytest.raises(TypeError, match="StateBox"):
        ilqrUtils.constrainedIterativeLqr(model, cost, cost, x0, ug)


def test_bad_arguments_return_codes_without_gpu():
    from zopt_amd import _lib, models
    lib = _lib.lib()
    d = 0x1000
    md = models.zm_model_t(models.ZM_MODEL_LINEAR, 3, 2, 0, 0.0, d, d)          # (c_struct() would upload A, B: no device here)
    big = models.zm_model_t(models.ZM_MODEL_LINEAR, 13, 2, 0, 0.0, d, d)
    pm, pb = ctypes.addressof(md), ctypes.addressof(big)
    qc = models.zm_quadcost_t(d, d, d, 0, 0)
    pc = ctypes.addressof(qc)
    sb = models.zm_statebox_t(d, d, 0, d, d, d)
    ps = ctypes.addressof(sb)

    def solve(model=pm, cost=pc, track=None, sbox=ps, mu0=1.0, growth=10.0, mu_max=1e8, outer=10, ctol=1e-4, ddp=0, x0=d, batch=1, T=3, ws=10 ** 9):
        return lib.zm_ilqr_solve_state_f64(model, cost, track, None, sbox, mu0, growth, mu_max, outer, ctol, x0, d, ddp, 10, 1e-3, 4, d, ws, d,
                                           d, d, d, d, d, d, None, None, None, None, batch, T, None)
    assert solve(batch=0) == _lib.ZM_OK
    assert solve(x0=None) == _lib.ZM_EINVAL and b"null" in lib.zm_last_error()
    assert solve(cost=None) == _lib.ZM_EINVAL and solve(track=d) == _lib.ZM_EINVAL              # exactly one of cost and track
    assert solve(ddp=1) == _lib.ZM_EUNSUPPORTED and b"DDP" in lib.zm_last_error()
    for kw in (dict(mu0=0.0), dict(mu0=-1.0), dict(growth=0.5), dict(outer=0), dict(mu0=float("nan")), dict(T=0), dict(batch=-1)):
        assert solve(**kw) == _lib.ZM_EINVAL, kw
    assert solve(model=pb) == _lib.ZM_EUNSUPPORTED
    bad = models.zm_statebox_t(d, d, 2, d, d, d)                                                 # stride neither 0 nor n
    assert solve(sbox=ctypes.addressof(bad)) == _lib.ZM_EINVAL and b"stride" in lib.zm_last_error()
    nomu = models.zm_statebox_t(d, d, 0, d, d, None)
    assert solve(sbox=ctypes.addressof(nomu)) == _lib.ZM_EINVAL
    assert solve(ws=10) == _lib.ZM_EINVAL and b"workspace" in lib.zm_last_error()
    noq = models.zm_quadcost_t(None, d, d, 0, 0)                                                 # checked before the first launch
    assert solve(cost=ctypes.addressof(noq)) == _lib.ZM_EINVAL and b"Q, R, Qf" in lib.zm_last_error()
    noa = models.zm_model_t(models.ZM_MODEL_LINEAR, 3, 2, 0, 0.0, None, d)
    assert solve(model=ctypes.addressof(noa)) == _lib.ZM_EINVAL and b"A, B" in lib.zm_last_error()
    odd = models.zm_model_t(77, 3, 2, 0, 0.0, d, d)
    assert solve(model=ctypes.addressof(odd)) == _lib.ZM_EUNSUPPORTED
    assert lib.zm_ilqr_solve_state_workspace_f64(pm, 5, 7) == lib.zm_ilqr_solve_workspace_f64(pm, 5, 7, 0) + 5 * 8 * 3 + 6 + 4 + 2
    # the array-level entries
    assert lib.zm_state_penalty_expand_list_f64(ps, d, None, 0, None, d, d, None, 1, 3, 3, None) == _lib.ZM_EINVAL
    assert lib.zm_state_penalty_expand_list_f64(ps, d, None, 0, None, d, d, d, 1, 3, 13, None) == _lib.ZM_EUNSUPPORTED
    assert lib.zm_state_penalty_expand_list_f64(ps, d, d, 2, None, d, d, d, 1, 3, 3, None) == _lib.ZM_EINVAL       # list longer than the batch
    assert lib.zm_state_multiplier_update_f64(ps, d, d, d, d, None, None, 1e-4, 0.5, 1e8, 1, 1, 3, 3, None) == _lib.ZM_EINVAL
    assert lib.zm_state_multiplier_update_f64(ps, d, None, d, d, None, None, 1e-4, 10.0, 1e8, 1, 1, 3, 3, None) == _lib.ZM_EINVAL
    args9 = [d] * 9
    assert lib.zm_ilqr_backward_state_f64(*args9, None, None, None, 1, d, d, None, 1, 3, 3, 2, None) == _lib.ZM_EINVAL          # no h
    assert lib.zm_ilqr_backward_state_f64(*args9, d, d, None, 1, d, d, None, 1, 3, 3, 2, None) == _lib.ZM_EINVAL                # uTraj without box
    assert lib.zm_ilqr_backward_state_f64(*args9, d, None, None, 1, d, d, None, 1, 3, 13, 2, None) == _lib.ZM_EUNSUPPORTED
    assert lib.zm_rollout_linesearch_state_f64(pm, pc, d, None, ps, d, d, d, d, d, d, 16, None, d, d, d, None, None, 1, 3, None) == _lib.ZM_EINVAL
    assert lib.zm_rollout_linesearch_state_f64(pm, None, None, None, ps, d, d, d, d, d, d, 16, None, d, d, d, None, None, 1, 3, None) == _lib.ZM_EINVAL


def test_quadcopter_case_hygiene():
    """the quadcopter solve cases of the GPU file (tests/ilqr_state_cases.quad_case, without and with the input box) by the rule as
    written, over all iterations of the restatement: the best and the second-best of the 16 costs >= 1e-9 relative apart, |s_ub|,
    |s_lb| of finite bounds >= 1e-7 (1 + mu), the inner and the outer test 1e-6 relative away from zero; the floor or the speed cap
    is active on two of the three trajectories, the third never touches a bound, and the boxed twin has inputs on their bounds"""
    c = cases.quad_case()
    for boxed in (False, True):
        active = []
        for b in range(cases.QUAD_B):
            o = cases.quad_restatement(boxed, b)
            gap, smin, test = cases.margins(o, c["x_lb"], c["x_ub"], cases.QUAD_KW["tol"], cases.QUAD_KW["ctol"])
            assert gap >= 1e-9 and smin >= 1e-7 and test >= 1e-6, (boxed, b, gap, smin, test)
            assert o["converged"] and o["violation"] <= cases.QUAD_KW["ctol"]
            active.append(int((o["lam_ub"] > 0).sum() + (o["lam_lb"] > 0).sum()))
            if boxed:
                u = o["traj"].uTraj
                assert np.all(u >= c["u_lb"]) and np.all(u <= c["u_ub"]) and np.any((u == c["u_lb"]) | (u == c["u_ub"]))
        assert active[2] == 0 and active[0] > 0 and (boxed or active[1] > 0), (boxed, active)


def test_sweep_cases_keep_the_complementarity_margin():
    """every sweep case of the GPU file (the box tests' hard families and shapes with an addend of entries 0 .. 1e8): every step of
    the long-double reference has the strict-complementarity margin of tests/ilqr_box_cases.py, the fp64 restatement finds the same
    clamped sets, the addend reaches 1e7 and holds exact zeros, and the bounds stay meaningful"""
    from tests import ilqr_box_cases as bcases
    clamped = 0
    for family in cases.SWEEP_FAMILIES:
        for shape in cases.SWEEP_SHAPES:
            c = cases.sweep_case(family, *shape)
            assert c["ref"]["margin"].min() >= bcases.MARGIN, (family, shape)
            assert c["h"].max() >= 1e7 and (c["h"][:, 1:] == 0).any() and not c["h"][:, 0].any()
            assert max(cases.sweep_bounds(family, *shape)) <= 1e-4, (family, shape)
            clamped += int(np.count_nonzero(c["ref"]["clamped"]))
    assert clamped >= 100


def test_long_double_restatement_and_line_search_reference():
    """`ld=True` (long-double line search and sweep) follows the fp64 restatement on a convex case with and without input bounds --
    the same counts and step indices where the costs decide them, J to 1e-10; and tests/ilqr_state_ref.PenaltyReference /
    check_linesearch accept the fp64 restatement's own line search at multipliers and mu up to 1e8 and catch a planted error (the
    penalty of the terminal row left out)"""
    from tests import linesearch_hp_ref as lhp
    from oracle import zopt_oracle as zo
    p = cases.qp_problem("dint")
    step = lambda x, u: p["A"] @ x + p["B"] @ u                                        # noqa: E731
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for boxed in (False, True):
            kw = dict(u_lb=p["u_lb"], u_ub=p["u_ub"]) if boxed else {}
            a = sref.constrainedIterativeLqr(step, p["Q"], p["R"], p["Qf"], p["x0"], np.zeros((p["T"], 1)), p["x_lb"], p["x_ub"], **kw)
            b = sref.constrainedIterativeLqr(step, p["Q"], p["R"], p["Qf"], p["x0"], np.zeros((p["T"], 1)), p["x_lb"], p["x_ub"], ld=True, **kw)
            assert a["outer"] == b["outer"] and a["inner"] == b["inner"] and a["converged"] == b["converged"]
            assert abs(a["J"] - b["J"]) <= 1e-10 * abs(a["J"]) and np.max(np.abs(a["lam_ub"] - b["lam_ub"])) <= 1e-8 * np.max(a["lam_ub"])
        q = lhp.problem("linear", "index_j", 5, 2, 6, 5, None, None, 0)
        pen = sref.linesearch_penalty(q, 1)
        assert np.max(pen[4]) > 1e6 and np.max(pen[3]) > 1e7
        for box in (None, (-1.05 * np.max(np.abs(q.uPrev), axis=(0, 1)), 1.02 * np.max(np.abs(q.uPrev), axis=(0, 1)))):
            ref = sref.PenaltyReference(q, pen, box)
            assert ref.comparable.all() and ref.determined.sum() >= 3
            xr, ur = q.refs(np.float64)
            outs = [sref._forward_pass(q.x0[i], q.step_oracle(), q.Q, q.R, q.Qf, xr[i], ur[i], zo.AffinePolicy(q.l[i], q.L[i]),
                                       zo.Trajectory(q.xPrev[i], q.uPrev[i]), None if box is None else box[0], None if box is None else box[1],
                                       tuple(t[i] for t in pen)) for i in range(q.b)]
            xT, uT = np.stack([o[0].xTraj for o in outs]), np.stack([o[0].uTraj for o in outs])
            J, Jc, idx = np.array([o[1] for o in outs]), np.array([o[2] for o in outs]), np.array([o[3] for o in outs])
            J16 = np.stack([o[4] for o in outs], axis=1)
            sref.check_linesearch(ref, xT, uT, J, Jc, idx, J16, what="fp64 restatement")
            last = np.array([sref.penalty(np.concatenate([xT[i][:1], xT[i][-1:]]), *[t[i] if t[i].ndim < 2 else t[i][[0, -1]] for t in pen]) for i in range(q.b)])
            assert np.any(last != 0)
            with pytest.raises(AssertionError):
                sref.check_linesearch(ref, xT, uT, J - last, Jc, idx, None, what="terminal penalty left out")
