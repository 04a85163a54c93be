"""GPU tests of stage-varying input bounds (models.InputBox(..., stage_varying=True); zm_inputbox_t.step_stride == m): the stage forms
of the generic and the (12, 4) fast box line search, of the iLQR box sweep and of the DDP box sweep (full tensors and packed pairs), and
the iLQR / DDP box solves on them -- against the constant forms (constant rows: bit for bit), against the restatement of
tests/ilqr_box_stage_ref.py in fp64 and long double, and against each other.

Shapes: lin3 (3, 2), the rigid body (8, 4) and the quadcopter (12, 4: the fast line search), T in {1, 2, 5, 12} (the fast kernel's four
rotating register sets with every tail, the sweeps' prefetch tails), batch 67 (one over a wave's worth of line-search groups and three
over a multiple of four), one schedule for all and one per trajectory.  tests/test_ilqr_box_stage.py asserts on the CPU what the cases
need: margins of the sweeps' box-QPs, a determined line search in every iteration of the solves."""
import ctypes

import numpy as np
import pytest

from oracle import zopt_oracle as zo
from tests import ddp_box_cases as dbc
from tests import hp_reference as hp
from tests import ilqr_box_cases as ibc
from tests import ilqr_box_stage_ref as sr
from tests import ilqr_tracking_ref as tref
from tests.test_ilqr_box_gpu import _p, _pattern, _registered
from tests.test_ilqr_tracking_gpu import _agreement, _dev, _model, _point, _reference, _rel, _weights

pytestmark = pytest.mark.gpu
INF = np.inf
FILL = 7.0
B67 = sr.BATCH
U_TRIM = ibc.U_TRIM


@pytest.fixture(scope="module")
def mods():
    import torch
    assert torch.cuda.is_available()
    from zopt_amd import _lib, ilqrUtils, models, pytrees
    return ilqrUtils, models, pytrees, _lib


def _tile(b, T):
    """constant bounds (m,) or (B, m) as rows (T, m) or (B, T, m)"""
    return np.repeat(np.expand_dims(np.asarray(b, dtype=np.float64), -2), T, axis=-2)


def _box(models, lb, ub, T, m, stage):
    """-> (zm_inputbox_t, the arrays behind it).  stage: lb / ub (T, m) (stride 0) or (B, T, m) (stride T m), step_stride m; else the
    constant form, (m,) (stride 0) or (B, m) (stride m)"""
    lb, ub = np.asarray(lb, dtype=np.float64), np.asarray(ub, dtype=np.float64)
    dl, du = _dev(lb), _dev(ub)
    if stage:
        assert lb.shape[-2:] == (T, m) and ub.shape == lb.shape
        return models.zm_inputbox_t(dl.data_ptr(), du.data_ptr(), 0 if lb.ndim == 2 else T * m, m), (dl, du)
    return models.zm_inputbox_t(dl.data_ptr(), du.data_ptr(), 0 if lb.ndim == 1 else m), (dl, du)


def _linesearch(_lib, models, model, cost, lb, ub, x0, l, L, xp, up, stage=True, ids=None, act=None, n_alpha=16):
    """zm_rollout_linesearch_box[_list]_f64 -> (xTraj, uTraj, J, idx); untouched rows keep the fill value"""
    import torch
    lib = _lib.lib()
    B, T, m, n = L.shape
    tracking = isinstance(cost, models.TrackingCost)
    md = model.c_struct()
    cs = None if cost is None else (cost.track_struct((B,), T) if tracking else cost.c_struct())
    pcs = None if cs is None else ctypes.addressof(cs)
    bs, keep = _box(models, lb, ub, T, m, stage)
    d = [_dev(a) for a in (x0, l, L, xp, up, 0.5 ** np.arange(n_alpha))]
    xT, uT, J = (torch.full(s, FILL, dtype=torch.float64, device="cuda") for s in ((B, T + 1, n), (B, T, m), (B,)))
    idx = torch.full((B,), 77, dtype=torch.int32, device="cuda")
    dact = None if act is None else _dev(act, torch.int32)
    head = (ctypes.addressof(md), None if tracking else pcs, pcs if tracking else None, ctypes.addressof(bs)) + tuple(_p(t) for t in d) + (n_alpha,)
    tail = (_p(xT), _p(uT), _p(J), _p(idx), B, T, None)
    if ids is None:
        rc = lib.zm_rollout_linesearch_box_f64(*head, _p(dact), *tail)
    else:
        dids = _dev(np.asarray(ids), torch.int32)
        rc = lib.zm_rollout_linesearch_box_list_f64(*head, _p(dids), len(ids), _p(dact), *tail)
    assert rc == 0, lib.zm_last_error()
    torch.cuda.synchronize()
    return xT.cpu().numpy(), uT.cpu().numpy(), J.cpu().numpy(), idx.cpu().numpy()


def _sweep(_lib, models, dyn, cost, Vf, u, lb, ub, stage=True, form="ilqr", ids=None, act=None):
    """the box sweeps -> (l, L, qp_capped).  form "ilqr": zm_ilqr_backward_box_list_f64; "full" / "null" / "pairs": the DDP box sweep on
    the three tensors, with f_ux = f_uu = NULL, or on the quadcopter's pair rows.  Untouched rows keep the fill value."""
    import torch
    lib = _lib.lib()
    B, T, n, m = np.asarray(dyn[2]).shape
    d = [_dev(np.asarray(a, dtype=np.float64)) for a in (cost[1], cost[2], cost[3], cost[4], cost[5], Vf[1], Vf[2], u)]
    fx, fu = _dev(np.asarray(dyn[1])), _dev(np.asarray(dyn[2]))
    bs, keep = _box(models, lb, ub, T, m, stage)
    l = torch.full((B, T, m), FILL, dtype=torch.float64, device="cuda")
    L = torch.full((B, T, m, n), FILL, dtype=torch.float64, device="cuda")
    cap = torch.zeros(B, dtype=torch.int32, device="cuda")
    dids = None if ids is None else _dev(np.asarray(ids), torch.int32)
    dact = None if act is None else _dev(act, torch.int32)
    tail = (ctypes.addressof(bs), _p(dids), 0 if ids is None else len(ids), _p(dact), 0, _p(l), _p(L), _p(cap), B, T)
    if form == "ilqr":
        rc = lib.zm_ilqr_backward_box_list_f64(_p(fx), _p(fu), *[_p(t) for t in d], *tail, n, m, None)
    elif form == "pairs":
        assert (n, m) == (12, 4)
        md = models.QuadcopterEuler(0.1).c_struct()
        H = _dev(dbc.pair_rows(np.asarray(dyn[3])))
        rc = lib.zm_ddp_backward_pairs_box_list_f64(ctypes.addressof(md), _p(fx), _p(fu), _p(H), *[_p(t) for t in d], *tail, None)
    else:
        fxx = _dev(np.asarray(dyn[3]))
        fux, fuu = (None, None) if form == "null" else (_dev(np.asarray(dyn[4])), _dev(np.asarray(dyn[5])))
        rc = lib.zm_ddp_backward_box_list_f64(_p(fx), _p(fu), _p(fxx), _p(fux), _p(fuu), *[_p(t) for t in d], *tail, n, m, None)
    assert rc == 0, lib.zm_last_error()
    torch.cuda.synchronize()
    return l.cpu().numpy(), L.cpu().numpy(), cap.cpu().numpy()


def _ddp_form(dyn):
    return "full" if (np.any(dyn[4]) or np.any(dyn[5])) else "null"


def _solve(ilqr, models, c, ddp, stage=True, **over):
    """the case through iterativeLqr / differentialDynamicProgramming(InputBox(model, lb, ub[, stage_varying])) with the trace on
    -> (xTraj, uTraj, L, J, converged, J_trace, alpha_trace, qp_capped)"""
    model = _registered(models, c["model"])
    cost = models.QuadraticCost(c["Q"], c["R"], c["Qf"]) if c["xRef"] is None else models.TrackingCost(c["Q"], c["R"], c["Qf"], c["xRef"], c["uRef"])
    lb, ub = over.pop("lb", c["lb"]), over.pop("ub", c["ub"])
    x0, ug = over.pop("x0", c["x0"]), over.pop("ug", c["ug"])
    ilqr._TRACE = []
    try:
        fn = ilqr.differentialDynamicProgramming if ddp else ilqr.iterativeLqr
        traj, L, J, conv = fn(models.InputBox(model, lb, ub, stage_varying=stage), cost, cost, x0, ug, **c["kw"])
        rec = dict(ilqr._TRACE)
    finally:
        ilqr._TRACE = None
    return traj.xTraj, traj.uTraj, L, J, conv, rec["J_trace"], rec["alpha_trace"], rec["qp_capped"]


def _const_bounds(rng, name, B, m, per):
    """a narrow box about the trim / zero input: (m,) or (B, m), one side infinite, one input fixed (tests/test_ilqr_box_gpu.py's)"""
    u0 = U_TRIM if name in ("quad", "rb") else np.zeros(m)
    w = rng.uniform(0.02, 0.08, (B, m) if per else (m,))
    lb, ub = u0 - w, u0 + w
    ub[..., -1] = INF
    lb[..., 0] = ub[..., 0] = u0[0] + 0.01
    return lb, ub


def _stage_bounds(rng, name, B, T, m, per):
    """rows that change per step (and per trajectory with `per`), with -inf / +inf entries and pinned entries"""
    u0 = U_TRIM if name in ("quad", "rb") else np.zeros(m)
    shp = (B, T, m) if per else (T, m)
    w = rng.uniform(0.01, 0.08, shp)
    lb, ub = u0 - w * rng.uniform(0.2, 1.0, shp), u0 + w
    kind = rng.integers(0, 6, shp)                               # 0: lb = -inf, 1: ub = +inf, 2: pinned, else a two-sided row
    lb, ub = np.where(kind == 0, -INF, lb), np.where(kind == 1, INF, ub)
    pin = u0 + 0.03 * rng.standard_normal(shp)
    return np.where(kind == 2, pin, lb), np.where(kind == 2, pin, ub)


# ------------------------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("name", ["quad", "lin12", "rb", "lin3"])
def test_constant_rows_line_search_bit_for_bit(mods, name):
    """the same row at every step: xTraj, uTraj, J and the index of the constant form, bit for bit -- the fast kernel (quad, lin12; the
    diagonal-only and the general instantiation) and the generic one (rb, lin3), 16 step sizes and one, QuadraticCost and
    TrackingCost, one schedule for all and one per trajectory"""
    _, models, _, _lib = mods
    model, _, n, m = _model(models, name)
    rng = np.random.default_rng(171)
    for T, per, diag in zip(sr.HORIZONS, (0, 1, 1, 0), (1, 0, 1, 0)):
        Q, R, Qf = _weights(n, m, diag)
        pt = _point(rng, name, B67, T, n, m)
        lb, ub = _const_bounds(rng, name, B67, m, per)
        costs = (models.QuadraticCost(Q, R, Qf), models.TrackingCost(Q, R, Qf, *_reference(rng, "full", B67, T, n, m)))
        for cost in costs:
            for n_alpha in (16, 1):
                want = _linesearch(_lib, models, model, cost, lb, ub, *pt, stage=False, n_alpha=n_alpha)
                got = _linesearch(_lib, models, model, cost, _tile(lb, T), _tile(ub, T), *pt, n_alpha=n_alpha)
                for a, b in zip(got, want):
                    assert np.array_equal(a, b, equal_nan=True), (name, T, per, type(cost).__name__, n_alpha)
                assert np.any((want[1] == np.expand_dims(np.broadcast_to(lb, (B67, m)), 1))[..., 1:])      # the box binds


def test_constant_rows_sweeps_bit_for_bit(mods):
    """the three sweeps (iLQR box, DDP box on the tensors, DDP box on the packed pairs) with the case's box tiled over the steps: l, L
    and qp_capped of the constant form, bit for bit, shared and per-trajectory bounds, every KS"""
    _, models, _, _lib = mods
    for shape in ibc.SWEEP_SHAPES:
        dyn, cost, Vf, u, lb, ub = ibc.sweep_case("cheap", *shape)["args"]
        T = shape[2]
        for a, b in zip(_sweep(_lib, models, dyn, cost, Vf, u, _tile(lb, T), _tile(ub, T)), _sweep(_lib, models, dyn, cost, Vf, u, lb, ub, stage=False)):
            assert np.array_equal(a, b, equal_nan=True), ("ilqr", shape)
    for family in ("plain", "control_affine_8", "packed_pairs"):
        for shape in dbc.family_shapes(family):
            dyn, cost, Vf, u, lb, ub = dbc.sweep_case(family, *shape)["args"]
            T = shape[2]
            for form in ((_ddp_form(dyn),) if family != "packed_pairs" else ("full", "pairs")):
                got = _sweep(_lib, models, dyn, cost, Vf, u, _tile(lb, T), _tile(ub, T), form=form)
                want = _sweep(_lib, models, dyn, cost, Vf, u, lb, ub, stage=False, form=form)
                for a, b in zip(got, want):
                    assert np.array_equal(a, b, equal_nan=True), (family, shape, form)


@pytest.mark.parametrize("case", [("lin3", False), ("quad_hover", False), ("quad_hover", True), ("rb", True)], ids=lambda c: f"{c[0]}-{'ddp' if c[1] else 'ilqr'}")
def test_constant_rows_solves_bit_for_bit(mods, case):
    """iterativeLqr / differentialDynamicProgramming on InputBox(model, lb, ub) and on the same box tiled over the horizon as a stage
    box: trajectories, gains, costs, flags and the per-iteration trace, bit for bit; batch 67, shared and per-trajectory bounds"""
    ilqr, models, _, _ = mods
    name, ddp = case
    c = dict(dbc.solve_case(name) if ddp else ibc.solve_case(name))
    B, T, m = c["ug"].shape
    rng = np.random.default_rng(173)
    pick = rng.integers(0, B, B67)
    c.update(x0=c["x0"][pick] * rng.uniform(0.8, 1.2, (B67, 1)), ug=c["ug"][pick])
    if c["xRef"] is not None and np.ndim(c["xRef"]) == 3:
        c["xRef"] = c["xRef"][pick]
    for per in (False, True):
        lb, ub = (np.tile(c["lb"], (B67, 1)), np.tile(c["ub"], (B67, 1))) if per else (c["lb"], c["ub"])
        want = _solve(ilqr, models, c, ddp, stage=False, lb=lb, ub=ub)
        got = _solve(ilqr, models, c, ddp, lb=_tile(lb, T), ub=_tile(ub, T))
        for a, b in zip(got, want):
            assert np.array_equal(a, b, equal_nan=True), (case, per)
        assert np.any((want[1] == c["lb"]) | (want[1] == c["ub"]))


# ------------------------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("name", ["quad", "rb", "lin3"])
def test_pinned_rows_are_stored_exactly(mods, name):
    """lb_k == ub_k == r_k, distinct per step, trajectory and component: the stored uTraj IS r, for every horizon, with 16 step sizes
    (both passes of the fast kernel) and with one.  Then one tight row at a single step k*, k* = 0 .. T-1, every other row far away:
    step k* alone stores r -- a row read one step early or late shows at once."""
    _, models, _, _lib = mods
    model, _, n, m = _model(models, name)
    Q, R, Qf = _weights(n, m, 1)
    cost = models.QuadraticCost(Q, R, Qf)
    rng = np.random.default_rng(181)
    u0 = U_TRIM if name in ("quad", "rb") else np.zeros(m)
    for T in sr.HORIZONS:
        pt = _point(rng, name, B67, T, n, m)
        r = u0 + 0.01 * (1 + np.arange(B67 * T * m, dtype=np.float64).reshape(B67, T, m)) / (B67 * T * m)
        for n_alpha in (16, 1):
            assert np.array_equal(_linesearch(_lib, models, model, cost, r, r, *pt, n_alpha=n_alpha)[1], r), (name, T, n_alpha)
        assert np.array_equal(_linesearch(_lib, models, model, cost, r[5], r[5], *pt)[1], np.broadcast_to(r[5], r.shape)), (name, T)      # one schedule for all
        for ks in range(T):
            lb, ub = np.full((B67, T, m), -1e6), np.full((B67, T, m), 1e6)
            lb[:, ks], ub[:, ks] = r[:, ks], r[:, ks]
            uT = _linesearch(_lib, models, model, cost, lb, ub, *pt)[1]
            assert np.array_equal(uT[:, ks], r[:, ks]), (name, T, ks)
            assert not np.any(np.delete(uT, ks, axis=1) == np.delete(r, ks, axis=1)), (name, T, ks)


@pytest.mark.parametrize("form", ["ilqr", "full", "pairs"])
def test_a_single_pinned_row_in_the_sweeps(mods, form):
    """lb_k* == ub_k* == u_k* at one step, no bounds elsewhere: l_k* == 0 and L_k* == 0 exactly at that step and at no other, for
    k* = 0 .. T-1, per-trajectory schedules -- the sweeps walk the rows backwards from T-1, an offset would show"""
    _, models, _, _lib = mods
    shapes = ((3, 2, 5, 5, True), (8, 4, 2, 9, True), (12, 4, 7, 9, False)) if form == "ilqr" else \
        ((3, 2, 5, 5, True), (12, 4, 6, 3, False)) if form == "full" else ((12, 4, 6, 3, False), (12, 4, 3, 5, True))
    for shape in shapes:
        src = ibc.sweep_case("plain", *shape) if form == "ilqr" else dbc.sweep_case("packed_pairs" if form == "pairs" else "plain", *shape)
        dyn, cost, Vf, u = src["args"][:4]
        B, T, m = u.shape
        for ks in range(T):
            lb, ub = np.full((B, T, m), -INF), np.full((B, T, m), INF)
            lb[:, ks], ub[:, ks] = u[:, ks], u[:, ks]
            l, L, cap = _sweep(_lib, models, dyn, cost, Vf, u, lb, ub, form=form)
            zero = ~np.any(L != 0, axis=(-1, -2)) & ~np.any(l != 0, axis=-1)            # (B, T)
            want = np.zeros((B, T), dtype=bool)
            want[:, ks] = True
            assert np.array_equal(zero, want) and not cap.any(), (form, shape, ks)


# ------------------------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("name", ["quad", "lin12", "rb", "lin3"])
def test_stage_line_search_against_the_restatement(mods, name):
    """rows that change per step, with -inf / +inf and pinned entries, one schedule for all and one per trajectory: the winner's index
    exactly, J at 1e-10 and the trajectory at 1e-9 (tests/test_ilqr_box_gpu.py's tolerances), every stored input inside its own
    step's box exactly -- and on it somewhere; with one step size the clipped rollout"""
    _, models, _, _lib = mods
    model, step, n, m = _model(models, name)
    rng = np.random.default_rng(191)
    on_box = 0
    for T, per, diag, layout in zip(sr.HORIZONS, (1, 0, 1, 0), (1, 0, 0, 1), ("full", "goal", "shared", "full")):
        Q, R, Qf = _weights(n, m, diag)
        xRef, uRef = _reference(rng, layout, B67, T, n, m)
        x0, l, L, xp, up = _point(rng, name, B67, T, n, m)
        lb, ub = _stage_bounds(rng, name, B67, T, m, per)
        lbb, ubb = sr.rows(lb, (B67,), T, m), sr.rows(ub, (B67,), T, m)
        for cost in (models.QuadraticCost(Q, R, Qf), models.TrackingCost(Q, R, Qf, xRef, uRef)):
            xT, uT, J, idx = _linesearch(_lib, models, model, cost, lb, ub, x0, l, L, xp, up)
            one = _linesearch(_lib, models, model, cost, lb, ub, x0, l, L, xp, up, n_alpha=1)
            for u_out in (uT, one[1]):
                assert np.all(u_out >= lbb) and np.all(u_out <= ubb), (name, T)
            assert np.array_equal(uT[lbb == ubb], lbb[lbb == ubb])
            on_box += int(np.sum(((uT == lbb) | (uT == ubb)) & (lbb != ubb)))
            for b in range(B67):
                xr, ur = tref.full_reference(xRef, uRef, T, n, m, b) if isinstance(cost, models.TrackingCost) else (np.zeros((T + 1, n)), np.zeros((T, m)))
                pol, prev = zo.AffinePolicy(l[b], L[b]), zo.Trajectory(xp[b], up[b])
                rt, rJ, ridx, rJs = sr.forward_pass(x0[b], step, Q, R, Qf, xr, ur, pol, prev, lbb[b], ubb[b])
                assert idx[b] == ridx, (name, T, b, rJs)
                assert abs(J[b] - rJ) <= 1e-10 * abs(rJ), (name, T, b)
                assert _rel(xT[b], rt.xTraj) <= 1e-9 and _rel(uT[b], rt.uTraj) <= 1e-9
                r1 = sr.rollout(x0[b], step, pol, prev, lbb[b], ubb[b])
                assert _rel(one[0][b], r1.xTraj) <= 1e-9 and _rel(one[1][b], r1.uTraj) <= 1e-9
        roll = _linesearch(_lib, models, model, None, lb, ub, x0, l, L, xp, up, n_alpha=1)       # no cost: the generic kernel's plain rollout
        assert _rel(roll[0], one[0]) <= 1e-9 and np.all(roll[1] >= lbb) and np.all(roll[1] <= ubb)
        lnan = l.copy()                                                                         # the NaN-passing clip, on a two-sided row
        lnan[1, T - 1, m - 1] = np.nan
        lb2, ub2 = lbb.copy(), ubb.copy()
        lb2[1, T - 1, m - 1], ub2[1, T - 1, m - 1] = -1.0, 1.0
        xT, uT, J, idx = _linesearch(_lib, models, model, models.QuadraticCost(Q, R, Qf), lb2, ub2, x0, lnan, L, xp, up)
        assert np.isnan(J[1]) and idx[1] == 0 and np.isnan(uT[1, T - 1, m - 1]) and np.isfinite(np.delete(J, 1)).all()
    assert on_box > 0


# ------------------------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("family", ibc.SWEEP_FAMILIES)
def test_stage_sweep_against_the_long_double_stage_sweep(mods, family):
    """the hard families of tests/ilqr_box_cases.py with per-step bounds: the clamped sets (the zero rows of L) exactly, l and L within
    hp.sweep_bounds' rule -- 100 x the fp64 restatement's own error against long double, tests/test_ilqr_box_gpu.py's bound; no QP
    capped; u + l inside the step's box"""
    _, models, _, _lib = mods
    report = []
    for shape in sr.SWEEP_SHAPES:
        c = sr.sweep_case(family, *shape)
        bl, bL = sr.sweep_bounds(family, *shape)
        l, L, cap = _sweep(_lib, models, *c["args"])
        el, eL = float(hp.sweep_metric(l, c["ref"]["l"]).max()), float(hp.sweep_metric(L, c["ref"]["L"]).max())
        report.append((shape, el, bl, eL, bL))
        assert np.array_equal(_pattern(L), c["ref"]["clamped"]), (family, shape)
        assert not cap.any()
        assert el <= bl and eL <= bL, (family, report[-1])
        u, lb, ub = c["args"][3:]
        assert np.all(l >= lb - u) and np.all(l <= ub - u), (family, shape)
    print(f"stage box sweep {family}: (shape, error of l, bound, error of L, bound)", report)


@pytest.mark.parametrize("family", sr.DDP_SWEEP_FAMILIES)
def test_stage_ddp_sweep_against_the_long_double_stage_ddp_sweep(mods, family):
    """the DDP second-derivative families of tests/ddp_box_cases.py with per-step bounds, on the tensors (f_ux = f_uu = NULL where they
    vanish) and, for `packed_pairs`, on the pair rows too: clamped sets exactly, l and L within hp.ddp_bounds' rule
    (tests/test_ddp_box_gpu.py's bound)"""
    _, models, _, _lib = mods
    report = []
    for shape in sr.ddp_family_shapes(family):
        c = sr.sweep_case(family, *shape, ddp=True)
        bl, bL = sr.sweep_bounds(family, *shape, ddp=True)
        for form in ((_ddp_form(c["args"][0]),) if family != "packed_pairs" else ("full", "pairs")):
            l, L, cap = _sweep(_lib, models, *c["args"], form=form)
            el, eL = float(hp.sweep_metric(l, c["ref"]["l"]).max()), float(hp.sweep_metric(L, c["ref"]["L"]).max())
            report.append((shape, form, el, bl, eL, bL))
            assert np.array_equal(_pattern(L), c["ref"]["clamped"]), (family, shape, form)
            assert not cap.any()
            assert el <= bl and eL <= bL, (family, report[-1])
            u, lb, ub = c["args"][3:]
            assert np.all(l >= lb - u) and np.all(l <= ub - u), (family, shape)
    print(f"stage box DDP sweep {family}: (shape, form, error of l, bound, error of L, bound)", report)


# ------------------------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("case", sr.SOLVE_CASES, ids=lambda c: f"{c[0]}-{'ddp' if c[1] else 'ilqr'}")
def test_stage_solves_follow_the_restatement_in_every_iteration(mods, case):
    """the solves with a schedule (two pinned steps, a box that narrows from step 4 on, per trajectory): the restatement's cost (1e-9
    relative) and step index (exactly) in EVERY iteration of every trajectory -- the CPU file has shown each line search determined,
    nothing is skipped -- then J at 1e-7, uTraj at 1e-6, L at 1e-5, the same clamped sets and the same flag.  Every stored input is
    inside its own step's box, the pinned ones on their values exactly; no QP was capped."""
    ilqr, models, _, _ = mods
    name, ddp = case
    c = sr.solve_case(name, ddp)
    xT, uT, L, J, conv, Jtr, atr, cap = _solve(ilqr, models, c, ddp)
    assert np.all(uT >= c["lb"]) and np.all(uT <= c["ub"]) and not cap.any()
    assert np.array_equal(uT[:, :2], c["lb"][:, :2])
    for b, r in enumerate(sr.solve_reference(name, ddp)):
        agree = _agreement(Jtr[:, b], atr[:, b], [t[:3] for t in r["trace"]])
        assert agree == r["its"], (case, b, agree, r["its"], Jtr[:, b], [t[:2] for t in r["trace"]])
        assert bool(conv[b]) == r["converged"] and abs(J[b] - r["J"]) <= 1e-7 * abs(r["J"]), (case, b)
        assert _rel(uT[b], r["traj"].uTraj) <= 1e-6 and _rel(L[b], r["L"]) <= 1e-5, (case, b)
        assert np.array_equal(_pattern(L[b][None])[0], r["trace"][-1][3]), (case, b)


# ------------------------------------------------------------------------------------------------------------------------------- 6
def test_list_and_active_forms_write_nothing_else(mods):
    """an id list with gaps and an `active` mask, per-trajectory schedules: listed, active trajectories get bit for bit what the dense
    call writes (their rows are read by trajectory id, not by slot), every other row keeps its fill value -- both line-search
    kernels, the iLQR sweep, the DDP sweep on tensors and on pairs"""
    _, models, _, _lib = mods
    rng = np.random.default_rng(211)
    ids = [66, 2, 31, 0, 64, 17]
    act = np.ones(B67, dtype=np.int32)
    act[31] = 0
    live = [66, 2, 0, 64, 17]
    for name in ("quad", "lin3"):
        model, _, n, m = _model(models, name)
        Q, R, Qf = _weights(n, m, 1)
        cost = models.QuadraticCost(Q, R, Qf)
        T = 5
        pt = _point(rng, name, B67, T, n, m)
        lb, ub = _stage_bounds(rng, name, B67, T, m, 1)
        dense = _linesearch(_lib, models, model, cost, lb, ub, *pt)
        part = _linesearch(_lib, models, model, cost, lb, ub, *pt, ids=ids, act=act)
        masked = _linesearch(_lib, models, model, cost, lb, ub, *pt, act=act)
        for a, d, mk in zip(part, dense, masked):
            for b in range(B67):
                assert np.array_equal(a[b], d[b]) if b in live else np.all((a[b] == FILL) | (a[b] == 77)), (name, b)
                assert np.array_equal(mk[b], d[b]) if b != 31 else np.all((mk[b] == FILL) | (mk[b] == 77)), (name, b)
    jobs = [("ilqr", sr.sweep_case("plain", 8, 4, 2, 5, True), [4, 1, 3], 3), ("full", sr.sweep_case("plain", 12, 4, 5, 3, True, True), [2, 0], 0),
            ("pairs", sr.sweep_case("packed_pairs", 12, 4, 5, 3, True, True), [2, 0], 0)]
    for form, c, lst, off in jobs:
        B = c["args"][3].shape[0]
        a_ = np.ones(B, dtype=np.int32)
        a_[off] = 0
        form = _ddp_form(c["args"][0]) if form == "full" else form
        dense = _sweep(_lib, models, *c["args"], form=form)
        part = _sweep(_lib, models, *c["args"], form=form, ids=lst, act=a_)
        for b in range(B):
            for a, d in zip(part[:2], dense[:2]):
                assert np.array_equal(a[b], d[b]) if (b in lst and b != off) else np.all(a[b] == FILL), (form, b)


# ------------------------------------------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize("case", [("quad_hover", False), ("quad_hover", True), ("lin3", False)], ids=lambda c: f"{c[0]}-{'ddp' if c[1] else 'ilqr'}")
def test_a_batch_member_solved_alone(mods, case):
    """per-trajectory stage bounds: a member of the batch solved alone with its own schedule gives its row of the batch, bit for bit
    (trace included)"""
    ilqr, models, _, _ = mods
    name, ddp = case
    c = sr.solve_case(name, ddp)
    full = _solve(ilqr, models, c, ddp)
    for b in (0, 3):
        xr = c["xRef"] if (c["xRef"] is None or np.ndim(c["xRef"]) == 1) else c["xRef"][b:b + 1]
        alone = _solve(ilqr, models, dict(c, xRef=xr), ddp, x0=c["x0"][b:b + 1], ug=c["ug"][b:b + 1], lb=c["lb"][b:b + 1], ub=c["ub"][b:b + 1])
        for a, f in zip(alone[:5], full[:5]):
            assert np.array_equal(a[0], f[b], equal_nan=True), (case, b)
        its = alone[5].shape[0]
        assert np.array_equal(alone[5][:, 0], full[5][:its, b], equal_nan=True) and np.array_equal(alone[6][:, 0], full[6][:its, b]), (case, b)
        shared = _solve(ilqr, models, dict(c, xRef=xr), ddp, x0=c["x0"][b:b + 1], ug=c["ug"][b:b + 1], lb=c["lb"][b], ub=c["ub"][b])      # (T, m): stride 0
        for a, f in zip(shared[:5], alone[:5]):
            assert np.array_equal(a, f, equal_nan=True), (case, b)


# ------------------------------------------------------------------------------------------------------------------------------- 8
def test_wrappers_take_a_stage_box(mods):
    """forwardPass2, trajectoryRollout, the simulator and backwardPass_ilqr_box / backwardPass_ddp_box through the Python layer: the
    array-level results; the device copy of the bounds is made once per batch shape"""
    ilqr, models, pytrees, _lib = mods
    from zopt_amd import simulator
    model, step, n, m = _model(models, "lin3")
    rng = np.random.default_rng(291)
    B, T = 9, 5
    Q, R, Qf = _weights(n, m, 1)
    x0, l, L, xp, up = _point(rng, "lin3", B, T, n, m)
    lb, ub = _stage_bounds(rng, "lin3", B, T, m, 1)
    box, cost = models.InputBox(model, lb, ub, stage_varying=True), models.QuadraticCost(Q, R, Qf)
    ref = _linesearch(_lib, models, model, cost, lb, ub, x0, l, L, xp, up)
    traj, J = ilqr.forwardPass2(x0, box, cost, pytrees.AffinePolicy(l, L), pytrees.Trajectory(xp, up))
    assert np.array_equal(traj.xTraj, ref[0]) and np.array_equal(traj.uTraj, ref[1]) and np.array_equal(J, ref[2])
    held = box._dev[(B,)]
    one = _linesearch(_lib, models, model, None, lb, ub, x0, l, L, xp, up, n_alpha=1)
    roll = ilqr.trajectoryRollout(x0, box, pytrees.AffinePolicy(l, L), pytrees.Trajectory(xp, up))
    assert np.array_equal(roll.xTraj, one[0]) and np.array_equal(roll.uTraj, one[1])
    assert box._dev[(B,)] is held and len(box._dev) == 1                  # copied once per batch shape, never per call
    sim = simulator.simulateTrackingController(box, x0, L, pytrees.Trajectory(xp, up))
    assert np.all(sim.uTraj >= lb) and np.all(sim.uTraj <= ub) and np.any((sim.uTraj == ub) | (sim.uTraj == lb))
    part = models.InputBox(model, lb[:1], ub[0], stage_varying=True)     # (1, T, m) next to (T, m): broadcast to the batch
    t2, _ = ilqr.forwardPass2(x0, part, cost, pytrees.AffinePolicy(l, L), pytrees.Trajectory(xp, up))
    ref2 = _linesearch(_lib, models, model, cost, lb[0], ub[0], x0, l, L, xp, up)
    assert np.array_equal(t2.uTraj, ref2[1])
    c = sr.sweep_case("plain", 3, 2, 12, 5, False)
    dyn, cst, Vf, u, slb, sub = c["args"]
    pol = ilqr.backwardPass_ilqr_box(pytrees.AffineDynamics(*dyn), pytrees.QuadraticCostFunction(*cst), pytrees.QuadraticValueFunction(*Vf), u,
                                     slb, sub, stage_varying=True)
    raw = _sweep(_lib, models, dyn, cst, Vf, u, slb, sub)
    assert np.array_equal(pol.l, raw[0]) and np.array_equal(pol.L, raw[1])
    c = sr.sweep_case("plain", 3, 2, 5, 3, False, True)
    dyn, cst, Vf, u, slb, sub = c["args"]
    pol = ilqr.backwardPass_ddp_box(pytrees.QuadraticDynamics(*dyn), pytrees.QuadraticCostFunction(*cst), pytrees.QuadraticValueFunction(*Vf), u,
                                    slb, sub, stage_varying=True)
    raw = _sweep(_lib, models, dyn, cst, Vf, u, slb, sub, form=_ddp_form(dyn))
    assert np.array_equal(pol.l, raw[0]) and np.array_equal(pol.L, raw[1])
