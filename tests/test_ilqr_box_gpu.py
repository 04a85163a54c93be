"""GPU tests of the input box (models.InputBox, zm_inputbox_t; control-limited iLQR): the device box-QP (boxqp4.h), the box sweep
(ilqr_backward.hip), the box line search (rollout.hip, rollout_fast.hip) and the box solve (ilqr_solve.hip) against the long-double
and fp64 restatement of tests/ilqr_box_ref.py, against the kernels without a box (infinite bounds) and against each other.

The cases and their bounds come from tests/ilqr_box_cases.py; tests/test_ilqr_box.py asserts on the CPU that every one of them has a
strict-complementarity margin, so clamped sets are compared exactly here.  Shapes are the smallest that reach the seams: (n, m) in
{(3, 2), (8, 4), (12, 4)}, T in {1, 2, 3, 5, 7} (the prefetch depths), batches of 5 and 9 (a partial four-trajectory wave in the line
search, an idle group), shared and per-trajectory bounds."""
import ctypes

import numpy as np
import pytest

from oracle import mpc_oracle as mo
from oracle import zopt_oracle as zo
from tests import hp_reference as hp
from tests import ilqr_box_cases as cases
from tests import ilqr_box_ref as br
from tests import ilqr_tracking_ref as tref
from tests.test_ilqr_tracking_gpu import _agreement, _dev, _linesearch, _model, _point, _reference, _rel, _weights

pytestmark = pytest.mark.gpu
INF = np.inf


@pytest.fixture(scope="module")
def mods():
    import torch
    assert torch.cuda.is_available()
    from zopt_amd import _lib, ilqrUtils, models, pytrees
    return ilqrUtils, models, pytrees, _lib


def _p(t):
    return None if t is None else t.data_ptr()


def _box(models, lb, ub, m):
    """-> (zm_inputbox_t, the arrays behind it): (m,) bounds are shared (stride 0), (B, m) ones per trajectory (stride m)"""
    dl, du = _dev(np.asarray(lb, dtype=np.float64)), _dev(np.asarray(ub, dtype=np.float64))
    return models.zm_inputbox_t(dl.data_ptr(), du.data_ptr(), 0 if np.ndim(lb) == 1 else m), (dl, du)


def _boxqp(_lib, H, g, lo, hi):
    import torch
    P, m = g.shape
    d = [_dev(a) for a in (H, g, lo, hi)]
    out = torch.full((P, m), 7.0, dtype=torch.float64, device="cuda")
    cl, it = (torch.full((P,), -1, dtype=torch.int32, device="cuda") for _ in range(2))
    rc = _lib.lib().zm_boxqp_f64(*[_p(t) for t in d], _p(out), _p(cl), _p(it), P, m, None)
    assert rc == 0, _lib.lib().zm_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy(), cl.cpu().numpy(), it.cpu().numpy()


def _box_sweep(_lib, models, dyn, cost, Vf, u, lb, ub, ids=None, act=None, shared=False):
    """zm_ilqr_backward_box[_list]_f64 -> (l, L, qp_capped); untouched rows keep the fill value 7 (qp_capped: 0)"""
    import torch
    lib = _lib.lib()
    B, T, n, m = np.asarray(dyn[2]).shape
    ops = [dyn[1], dyn[2], cost[1], cost[2], cost[3], cost[4], cost[5], Vf[1], Vf[2], u]
    if shared:               # one time-invariant Hessian set: the first step's of the first trajectory
        ops[4:7] = [np.asarray(cost[i])[0, 0] for i in (3, 4, 5)]
        ops[8] = np.asarray(Vf[2])[0]
    d = [_dev(np.asarray(a, dtype=np.float64)) for a in ops]
    bs, keep = _box(models, lb, ub, m)
    l = torch.full((B, T, m), 7.0, dtype=torch.float64, device="cuda")
    L = torch.full((B, T, m, n), 7.0, dtype=torch.float64, device="cuda")
    cap = torch.zeros(B, dtype=torch.int32, device="cuda")
    dids = None if ids is None else _dev(np.asarray(ids), torch.int32)
    dact = None if act is None else _dev(act, torch.int32)
    rc = lib.zm_ilqr_backward_box_list_f64(*[_p(t) for t in d], ctypes.addressof(bs), _p(dids), 0 if ids is None else len(ids), _p(dact),
                                           1 if shared else 0, _p(l), _p(L), _p(cap), B, T, n, m, None)
    assert rc == 0, lib.zm_last_error()
    torch.cuda.synchronize()
    return l.cpu().numpy(), L.cpu().numpy(), cap.cpu().numpy()


def _pattern(L):
    """the clamped sets read from the zero rows of L: (B, T) bit masks"""
    zero = ~np.any(np.asarray(L) != 0, axis=-1)                   # (B, T, m)
    return np.sum(zero.astype(np.int64) << np.arange(zero.shape[-1]), axis=-1)


def _box_linesearch(_lib, models, model, cost, lb, ub, x0, l, L, xp, up, ids=None, act=None, n_alpha=16):
    """zm_rollout_linesearch_box[_list]_f64 on a QuadraticCost, a TrackingCost or no cost; untouched rows keep the fill value 7"""
    import torch
    lib = _lib.lib()
    B, T, m, n = L.shape
    tracking = isinstance(cost, models.TrackingCost)
    md = model.c_struct()
    cs = None if cost is None else (cost.track_struct((B,), T) if tracking else cost.c_struct())
    pcs = None if cs is None else ctypes.addressof(cs)
    bs, keep = _box(models, lb, ub, m)
    d = [_dev(a) for a in (x0, l, L, xp, up, 0.5 ** np.arange(n_alpha))]
    xT, uT, J = (torch.full(s, 7.0, dtype=torch.float64, device="cuda") for s in ((B, T + 1, n), (B, T, m), (B,)))
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


def _registered(models, spec):
    if spec[0] == "lin":
        return models.LinearModel(spec[1], spec[2])
    return models.QuadcopterRigidBody(spec[1]) if spec[0] == "rb" else models.QuadcopterEuler(spec[1])


# ------------------------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("m", [1, 2, 3, 4])
def test_boxqp_against_the_long_double_enumerator(mods, m):
    """zm_boxqp_f64 on the table of tests/ilqr_box_cases.py (families: none clamped, all clamped, each single component at its lower or
    upper bound, mixed with a nonsymmetric H, infinite sides, lb == ub, cond(H) up to 1e8, badly scaled g): the clamped set exactly,
    d within hp.sweep_bounds' rule (100 x the larger of the fp64 enumerator's error on the family and on the plain one), the passes
    below the cap; clamped components sit on their bound exactly and d is feasible"""
    _, _, _, _lib = mods
    t = cases.qp_problems(m)
    d, cl, it = _boxqp(_lib, t["H"], t["g"], t["lo"], t["hi"])
    err = cases.qp_metric(d, t["d"])
    worst = {f: (float(err[t["family"] == f].max()), t["bound"][f]) for f in t["bound"]}
    print(f"boxqp m={m}: passes max {it.max()}, (error, bound) per family {worst}")
    assert np.array_equal(cl, t["clamped"]), (t["family"][cl != t["clamped"]], cl[cl != t["clamped"]], t["clamped"][cl != t["clamped"]])
    assert np.all((it >= 1) & (it < cases.QP_CAP)), it.max()
    assert np.all(d >= t["lo"]) and np.all(d <= t["hi"])
    bits = (cl[:, None] >> np.arange(m)) & 1
    assert np.all((d == t["lo"]) | (d == t["hi"]) | (bits == 0))
    for f, (e, b) in worst.items():
        assert e <= b, (f, e, b)


def test_boxqp_nan_returns(mods):
    """a NaN in g (or in H) ends after a pass or two and yields NaN: nothing spins"""
    _, _, _, _lib = mods
    t = cases.qp_problems(4)
    g = t["g"][:8].copy()
    g[:4, 1] = np.nan
    H = t["H"][:8].copy()
    H[4:, 2, 2] = np.nan
    d, cl, it = _boxqp(_lib, H, g, t["lo"][:8], t["hi"][:8])
    assert np.all(it <= cases.QP_CAP)
    assert np.all(np.isnan(d).any(axis=1))


# ------------------------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("family", cases.SWEEP_FAMILIES)
def test_box_sweep_against_the_long_double_box_sweep(mods, family):
    """l, L and the clamped pattern (the zero rows of L), per trajectory and per step, with hp.sweep_metric / hp.sweep_bounds; no QP
    reaches its cap"""
    _, models, _, _lib = mods
    report = []
    for shape in cases.SWEEP_SHAPES:
        c = cases.sweep_case(family, *shape)
        bl, bL = cases.sweep_bounds(family, *shape)
        l, L, cap = _box_sweep(_lib, models, *c["args"])
        el, eL = float(hp.sweep_metric(l, c["ref"]["l"]).max()), float(hp.sweep_metric(L, c["ref"]["L"]).max())
        report.append((shape, el, bl, eL, bL))
        assert np.array_equal(_pattern(L), c["ref"]["clamped"]), (family, shape)
        assert not cap.any()
        assert el <= bl and eL <= bL, (family, report[-1])
        u, lb, ub = c["args"][3:]
        lo = np.expand_dims(np.broadcast_to(lb, (shape[3], shape[1])), 1) - u
        hi = np.expand_dims(np.broadcast_to(ub, (shape[3], shape[1])), 1) - u
        assert np.all(l >= lo) and np.all(l <= hi), (family, shape)                    # u + l stays inside the box
    print(f"box sweep {family}: (shape, error of l, bound, error of L, bound)", report)


def test_box_sweep_with_infinite_bounds_is_the_plain_sweep(mods):
    """no bound: nothing is clamped and l, L agree with the long-double sweep without a box under the bound the plain kernel
    (zm_ilqr_backward_list_f64) is held to -- which is asserted for that kernel on the same inputs; also with shared Hessians"""
    import torch
    _, models, _, _lib = mods
    lib = _lib.lib()
    for (n, m, T, B, _) in cases.SWEEP_SHAPES:
        c = cases.unbounded_case(n, m, T, B)
        dyn, cost, Vf = c["args"]
        u = np.zeros((B, T, m))
        l, L, cap = _box_sweep(_lib, models, dyn, cost, Vf, u, np.full(m, -INF), np.full(m, INF))
        d = [_dev(np.asarray(a)) for a in (dyn[1], dyn[2], cost[1], cost[2], cost[3], cost[4], cost[5], Vf[1], Vf[2])]
        pl, pL = torch.empty((B, T, m), dtype=torch.float64, device="cuda"), torch.empty((B, T, m, n), dtype=torch.float64, device="cuda")
        assert lib.zm_ilqr_backward_list_f64(*[_p(t) for t in d], None, 0, None, 0, _p(pl), _p(pL), B, T, n, m, None) == 0
        torch.cuda.synchronize()
        for out_l, out_L in ((l, L), (pl.cpu().numpy(), pL.cpu().numpy())):
            assert hp.sweep_metric(out_l, c["ref"]["l"]).max() <= c["bound_l"], (n, m, T, B)
            assert hp.sweep_metric(out_L, c["ref"]["L"]).max() <= c["bound_L"], (n, m, T, B)
        assert not _pattern(L).any() and not cap.any()
        ls, Ls, _ = _box_sweep(_lib, models, dyn, cost, Vf, u, np.full(m, -INF), np.full(m, INF), shared=True)
        sh = [d[0], d[1], d[2], d[3], _dev(np.asarray(cost[3])[0, 0]), _dev(np.asarray(cost[4])[0, 0]), _dev(np.asarray(cost[5])[0, 0]), d[7],
              _dev(np.asarray(Vf[2])[0])]
        assert lib.zm_ilqr_backward_list_f64(*[_p(t) for t in sh], None, 0, None, 1, _p(pl), _p(pL), B, T, n, m, None) == 0
        torch.cuda.synchronize()
        assert _rel(ls, pl.cpu().numpy()) <= 1e-9 and _rel(Ls, pL.cpu().numpy()) <= 1e-9, (n, m, T, B)


def test_box_sweep_list_and_mask(mods):
    """a list with gaps and an `active` mask: listed, active trajectories get bit for bit what the dense call writes, every other row
    keeps its fill value; per-trajectory bounds are read by trajectory id, not by slot"""
    _, models, _, _lib = mods
    for shape in ((3, 2, 5, 9, True), (12, 4, 7, 9, False)):
        c = cases.sweep_case("plain", *shape)
        dense = _box_sweep(_lib, models, *c["args"])
        ids, act = [7, 2, 5, 0], np.ones(9, dtype=np.int32)
        act[5] = 0
        part = _box_sweep(_lib, models, *c["args"], ids=ids, act=act)
        for b in range(9):
            for a, d in zip(part[:2], dense[:2]):
                assert np.array_equal(a[b], d[b]) if b in (7, 2, 0) else np.all(a[b] == 7.0), (shape, b)
        masked = _box_sweep(_lib, models, *c["args"], act=act)
        assert np.array_equal(masked[0][act == 1], dense[0][act == 1]) and np.all(masked[0][5] == 7.0)


# ------------------------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("diag", [1, 0], ids=["diagonal", "full"])
@pytest.mark.parametrize("name", ["quad", "lin12", "rb", "lin3"])
def test_box_line_search_with_infinite_bounds_bit_for_bit(mods, name, diag):
    """infinite bounds: xTraj, uTraj, J and the index of zm_rollout_linesearch_f64 / _tracking_f64 bit for bit, with 16 step sizes and
    with one, on the (12, 4) fast kernel (quad, lin12) and on the generic one (rb, lin3), with an id list and a mask too"""
    _, models, _, _lib = mods
    model, _, n, m = _model(models, name)
    Q, R, Qf = _weights(n, m, diag)
    rng = np.random.default_rng(71)
    none = (np.full(m, -INF), np.full(m, INF))
    for T, B, layout in zip((1, 2, 3, 5, 7), (5, 9, 5, 9, 5), ("shared", "goal", "full", "full", "goal")):
        pt = _point(rng, name, B, T, n, m)
        per = (np.full((B, m), -INF), np.full((B, m), INF))
        for cost in (models.QuadraticCost(Q, R, Qf), models.TrackingCost(Q, R, Qf, *_reference(rng, layout, B, T, n, m))):
            for n_alpha in (16, 1):
                ref = _linesearch(_lib, model, cost, *pt, n_alpha=n_alpha)
                for bounds in (none, per):
                    for a, b in zip(_box_linesearch(_lib, models, model, cost, *bounds, *pt, n_alpha=n_alpha), ref):
                        assert np.array_equal(a, b, equal_nan=True), (T, B, type(cost).__name__, n_alpha)
            ids, act = [3, 0, 4], np.ones(B, dtype=np.int32)
            act[4] = 0
            ref = _linesearch(_lib, model, cost, *pt, ids=ids, act=act)
            for a, b in zip(_box_linesearch(_lib, models, model, cost, *none, *pt, ids=ids, act=act), ref):
                assert np.array_equal(a, b), (T, B, "list")


@pytest.mark.parametrize("diag", [1, 0], ids=["diagonal", "full"])
@pytest.mark.parametrize("name", ["quad", "lin12", "rb", "lin3"])
def test_box_line_search_against_the_restatement(mods, name, diag):
    """finite bounds (shared and per trajectory, one side infinite, one input fixed): the winner's index exactly, J at 1e-10 and the
    trajectory at 1e-9 (tests/test_ilqr_tracking_gpu.py::test_line_search_and_expansion_against_the_restatement's tolerances), every
    stored u inside the box exactly -- and on it somewhere; a NaN in l gives J = NaN, which wins"""
    _, models, _, _lib = mods
    model, step, n, m = _model(models, name)
    Q, R, Qf = _weights(n, m, diag)
    rng = np.random.default_rng(72 + diag)
    u0 = np.array([9.807, 0, 0, 0]) if name in ("quad", "rb") else np.zeros(m)
    on_box = 0
    for T, B, layout, per in zip((1, 2, 3, 5, 7), (5, 9, 5, 9, 5), ("shared", "goal", "full", "full", "goal"), (0, 1, 0, 1, 1)):
        xRef, uRef = _reference(rng, layout, B, T, n, m)
        x0, l, L, xp, up = _point(rng, name, B, T, n, m)
        w = rng.uniform(0.02, 0.08, (B, m) if per else (m,))
        lb, ub = u0 - w, u0 + w
        ub[..., -1] = INF
        lb[..., 0] = ub[..., 0] = u0[0] + 0.01                     # lb == ub fixes the first input
        for cost in (models.QuadraticCost(Q, R, Qf), models.TrackingCost(Q, R, Qf, xRef, uRef)):
            xT, uT, J, idx = _box_linesearch(_lib, models, model, cost, lb, ub, x0, l, L, xp, up)
            one = _box_linesearch(_lib, models, model, cost, lb, ub, x0, l, L, xp, up, n_alpha=1)
            lbb, ubb = (np.broadcast_to(t, (B, m))[:, None, :] for t in (lb, ub))
            for u_out in (uT, one[1]):
                assert np.all(u_out >= lbb) and np.all(u_out <= ubb), (T, B)
            on_box += int(np.sum((uT[..., 1:] == lbb[..., 1:]) | (uT[..., 1:] == ubb[..., 1:])))
            assert np.all(uT[..., 0] == u0[0] + 0.01)
            for b in range(B):
                xr, ur = tref.full_reference(xRef, uRef, T, n, m, b) if isinstance(cost, models.TrackingCost) else (np.zeros((T + 1, n)), np.zeros((T, m)))
                lbt, ubt = np.broadcast_to(lb, (B, m))[b], np.broadcast_to(ub, (B, m))[b]
                rt, rJ, ridx, rJs = br.forward_pass(x0[b], step, Q, R, Qf, xr, ur, zo.AffinePolicy(l[b], L[b]), zo.Trajectory(xp[b], up[b]), lbt, ubt)
                assert idx[b] == ridx, (T, B, layout, b, rJs)
                assert abs(J[b] - rJ) <= 1e-10 * abs(rJ), (T, B, layout, b)
                assert _rel(xT[b], rt.xTraj) <= 1e-9 and _rel(uT[b], rt.uTraj) <= 1e-9
                r1 = br.rollout(x0[b], step, zo.AffinePolicy(l[b], L[b]), zo.Trajectory(xp[b], up[b]), lbt, ubt)
                assert _rel(one[0][b], r1.xTraj) <= 1e-9 and _rel(one[1][b], r1.uTraj) <= 1e-9
        # a NaN in l: the clip lets it through, J = NaN wins the argmin (index 0: every step size meets it)
        lnan = l.copy()
        lnan[1, T - 1, m - 1] = np.nan
        xT, uT, J, idx = _box_linesearch(_lib, models, model, models.QuadraticCost(Q, R, Qf), lb, ub, x0, lnan, L, xp, up)
        assert np.isnan(J[1]) and idx[1] == 0 and np.isnan(uT[1, T - 1, m - 1]) and np.isfinite(np.delete(J, 1)).all()
        # no cost at all: the plain clipped rollout (trajectoryRollout)
        roll = _box_linesearch(_lib, models, model, None, lb, ub, x0, l, L, xp, up, n_alpha=1)
        assert _rel(roll[0], one[0]) <= 1e-9 and _rel(roll[1], one[1]) <= 1e-9      # (the generic kernel also where `one` ran the fast one)
        assert np.all(roll[1] >= lbb) and np.all(roll[1] <= ubb)
    assert on_box > 0


# ------------------------------------------------------------------------------------------------------------------------------- 4
def _box_solve(ilqr, models, c, box=True, **over):
    """the case through iterativeLqr(InputBox(model, lb, ub), ...) -> _solve's tuple + qp_capped"""
    model = _registered(models, c["model"])
    cost = models.QuadraticCost(c["Q"], c["R"], c["Qf"]) if c["xRef"] is None else models.TrackingCost(c["Q"], c["R"], c["Qf"], c["xRef"], c["uRef"])
    lb, ub = over.pop("lb", c["lb"]), over.pop("ub", c["ub"])
    x0, ug = over.pop("x0", c["x0"]), over.pop("ug", c["ug"])
    kw = over.pop("kw", c["kw"])
    ilqr._TRACE = []
    try:
        traj, L, J, conv = ilqr.iterativeLqr(models.InputBox(model, lb, ub) if box else model, cost, cost, x0, ug, **kw)
        rec = dict(ilqr._TRACE)
    finally:
        ilqr._TRACE = None
    return traj.xTraj, traj.uTraj, L, J, conv, rec["J_trace"], rec["alpha_trace"], rec.get("qp_capped")


@pytest.mark.parametrize("name", cases.SOLVE_CASES)
def test_box_solves_follow_the_restatement_iteration_by_iteration(mods, name):
    """zm_ilqr_solve_box_trace_f64 through iterativeLqr(InputBox(...)) against the restatement: the cost to 1e-9 relative and the
    step index exactly for as many iterations as the two agree (tests/test_ilqr_tracking_gpu.py's _agreement), and that count at
    least what the same check reaches for the twin of the case without a box (kernel against tests/ilqr_tracking_ref.py) --
    measured here, per trajectory; where they stay together to the end: J at 1e-7, uTraj at 1e-6, L at 1e-5 and the same clamped
    sets (the zero rows of L).  Every stored input is feasible, no QP was capped."""
    import warnings
    ilqr, models, _, _ = mods
    c = cases.solve_case(name)
    B, T, m = c["ug"].shape
    n = c["x0"].shape[-1]
    xT, uT, L, J, conv, Jtr, atr, cap = _box_solve(ilqr, models, c)
    _, _, _, _, _, Jtrq, atrq, _ = _box_solve(ilqr, models, c, box=False)
    assert np.all(uT >= c["lb"]) and np.all(uT <= c["ub"]) and not cap.any()
    assert np.any((uT == c["lb"]) | (uT == c["ub"]))
    report = []
    for b, r in enumerate(cases.solve_reference(name)):
        xr, ur = tref.full_reference(c["xRef"], c["uRef"], T, n, m, b)
        trq = []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            itsq = tref.iterativeLqr(c["step"], c["Q"], c["R"], c["Qf"], xr, ur, c["x0"][b], c["ug"][b], return_iters=True, trace=trq, **c["kw"])[4]
        agree = _agreement(Jtr[:, b], atr[:, b], [t[:3] for t in r["trace"]])
        twin = _agreement(Jtrq[:, b], atrq[:, b], trq)
        report.append((b, agree, r["its"], twin, itsq))
        assert agree >= 1 and agree >= min(twin, r["its"]), (name, report)
        if agree == r["its"]:
            assert bool(conv[b]) == r["converged"] and abs(J[b] - r["J"]) <= 1e-7 * abs(r["J"]), (name, b)
            assert _rel(uT[b], r["traj"].uTraj) <= 1e-6 and _rel(L[b], r["L"]) <= 1e-5, (name, b)
            assert np.array_equal(_pattern(L[b][None])[0], r["trace"][-1][3]), (name, b)
    print(f"box solve {name}: (trajectory, iterations in agreement, restatement iterations, unboxed twin's agreement, its iterations)", report)


@pytest.mark.parametrize("name", ["lin3", "quad_hover"])
def test_a_batch_member_solved_alone_and_per_trajectory_bounds(mods, name):
    """a member of the batch solved alone gives the same bits (trace included); so does the batch with the shared box written out
    per trajectory -- and then each trajectory follows its own box"""
    ilqr, models, _, _ = mods
    c = cases.solve_case(name)
    B, T, m = c["ug"].shape
    full = _box_solve(ilqr, models, c)
    for b in (0, 3):
        xr = c["xRef"] if (c["xRef"] is None or np.ndim(c["xRef"]) == 1) else c["xRef"][b:b + 1]
        alone = _box_solve(ilqr, models, dict(c, xRef=xr), x0=c["x0"][b:b + 1], ug=c["ug"][b:b + 1])
        for a, f in zip(alone[:5], full[:5]):
            assert np.array_equal(a[0], f[b], equal_nan=True), (name, b)
        its = alone[5].shape[0]
        assert np.array_equal(alone[5][:, 0], full[5][:its, b], equal_nan=True), (name, b)
    per = _box_solve(ilqr, models, c, lb=np.tile(c["lb"], (B, 1)), ub=np.tile(c["ub"], (B, 1)))
    for a, f in zip(per[:7], full[:7]):
        assert np.array_equal(a, f, equal_nan=True), name
    lb2, ub2 = np.tile(c["lb"], (B, 1)), np.tile(c["ub"], (B, 1))
    lb2[1], ub2[1] = -INF, INF                                   # trajectory 1 without a box: it leaves the others' alone
    mixed = _box_solve(ilqr, models, c, lb=lb2, ub=ub2)
    free = _box_solve(ilqr, models, c, lb=-INF, ub=INF)
    for a, f, g in zip(mixed[:5], full[:5], free[:5]):
        assert np.array_equal(np.delete(a, 1, axis=0), np.delete(f, 1, axis=0), equal_nan=True) and np.array_equal(a[1], g[1], equal_nan=True)


def test_box_solve_list_form_equals_dense_form(mods):
    """ZOPT_AMD_ILQR_SYNC only changes how often the id list is rebuilt: a solve that syncs every iteration (the list always exact)
    and one that never rebuilds it (the dense list of the first iteration with the mask; it runs to maxIter) give the same bits"""
    import os
    ilqr, models, _, _ = mods
    c = cases.solve_case("quad_hover")
    keep = os.environ.get("ZOPT_AMD_ILQR_SYNC")
    try:
        os.environ["ZOPT_AMD_ILQR_SYNC"] = "1"
        every = _box_solve(ilqr, models, c)
        os.environ["ZOPT_AMD_ILQR_SYNC"] = "1000"
        never = _box_solve(ilqr, models, c)
    finally:
        if keep is None:
            os.environ.pop("ZOPT_AMD_ILQR_SYNC", None)
        else:
            os.environ["ZOPT_AMD_ILQR_SYNC"] = keep
    for a, b in zip(every[:5], never[:5]):
        assert np.array_equal(a, b, equal_nan=True)
    its = every[5].shape[0]
    assert its <= never[5].shape[0] and np.array_equal(every[5], never[5][:its], equal_nan=True)


# ------------------------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("case", cases.CONVEX_CASES, ids=lambda c: f"n{c[0]}m{c[1]}")
def test_convex_cases_on_the_device(mods, case):
    """the two convex cases of tests/test_ilqr_box.py: the KKT certificate's stat <= 100 x the restatement's own (or 1e-12), J within
    1e-9 relative of the restatement's, the same inputs at a bound"""
    ilqr, models, _, _ = mods
    n, m, N, seed, box = case
    c, r = cases.convex_case(*case), cases.convex_reference(*case)
    cost = models.QuadraticCost(c["Q"], c["R"], c["Qf"])
    traj, L, J, conv = ilqr.iterativeLqr(models.InputBox(models.LinearModel(c["A"], c["B"]), c["lb"], c["ub"]), cost, cost, c["x0"], c["ug"],
                                         tol=c["tol"])
    inf = np.full(n, INF)
    kkt = mo.kkt_residuals(c["A"], c["B"], c["Q"], c["R"], c["Qf"], N, -inf, inf, c["lb"], c["ub"], c["x0"], traj.xTraj, traj.uTraj)
    print(f"convex {case} on the device: stat {kkt['stat']:.2e} (restatement {r['stat']:.2e}), J {J!r} (restatement {r['J']!r})")
    assert kkt["stat"] <= max(100 * r["stat"], 1e-12)
    assert abs(J - r["J"]) <= 1e-9 * abs(r["J"])
    assert np.array_equal((traj.uTraj <= c["lb"]) | (traj.uTraj >= c["ub"]), r["at_bound"])
    assert kkt["bound"] == 0.0 and kkt["dyn"] <= 1e-12


# ------------------------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize("name", cases.SOLVE_CASES)
def test_infinite_bounds_through_iterativeLqr(mods, name):
    """iterativeLqr(InputBox(model, -inf, inf), ...) against the plain iterativeLqr at the iterate-by-iterate rule: the step index
    exactly and the cost to 1e-9 relative in every iteration both ran, then J at 1e-7, uTraj at 1e-6, L at 1e-5"""
    ilqr, models, _, _ = mods
    c = cases.solve_case(name)
    # (lin3 without a box is an LQ problem: one iteration solves it, a second one would search among 16 costs equal to rounding)
    kw = dict(c["kw"], maxIter=1) if name == "lin3" else c["kw"]
    box = _box_solve(ilqr, models, c, lb=-INF, ub=INF, kw=kw)
    plain = _box_solve(ilqr, models, c, box=False, kw=kw)
    assert box[5].shape == plain[5].shape and not box[7].any()
    for b in range(c["ug"].shape[0]):
        its = box[5].shape[0]
        assert _agreement(box[5][:, b], box[6][:, b], [(J, a, None) for J, a in zip(plain[5][:, b], plain[6][:, b])]) == its, (name, b)
        assert bool(box[4][b]) == bool(plain[4][b]) and abs(box[3][b] - plain[3][b]) <= 1e-7 * abs(plain[3][b])
        assert _rel(box[1][b], plain[1][b]) <= 1e-6 and _rel(box[2][b], plain[2][b]) <= 1e-5


def test_wrappers_take_an_input_box(mods):
    """forwardPass2, trajectoryRollout, the simulator and backwardPass_ilqr_box through the Python layer: the array-level results"""
    ilqr, models, pytrees, _lib = mods
    from zopt_amd import simulator
    model, step, n, m = _model(models, "lin3")
    rng = np.random.default_rng(91)
    B, T = 5, 5
    Q, R, Qf = _weights(n, m, 1)
    x0, l, L, xp, up = _point(rng, "lin3", B, T, n, m)
    lb, ub = np.array([-0.03, -INF]), np.array([0.02, 0.04])
    box, cost = models.InputBox(model, lb, ub), models.QuadraticCost(Q, R, Qf)
    ref = _box_linesearch(_lib, models, model, cost, lb, ub, x0, l, L, xp, up)
    traj, J = ilqr.forwardPass2(x0, box, cost, pytrees.AffinePolicy(l, L), pytrees.Trajectory(xp, up))
    assert np.array_equal(traj.xTraj, ref[0]) and np.array_equal(traj.uTraj, ref[1]) and np.array_equal(J, ref[2])
    one = _box_linesearch(_lib, models, model, None, lb, ub, x0, l, L, xp, up, n_alpha=1)
    roll = ilqr.trajectoryRollout(x0, box, pytrees.AffinePolicy(l, L), pytrees.Trajectory(xp, up))
    assert np.array_equal(roll.xTraj, one[0]) and np.array_equal(roll.uTraj, one[1])
    sim = simulator.simulateTrackingController(box, x0, L, pytrees.Trajectory(xp, up))
    assert np.all(sim.uTraj >= lb) and np.all(sim.uTraj <= ub) and np.any(sim.uTraj == ub)
    c = cases.sweep_case("plain", 3, 2, 5, 9, True)
    dyn, cst, Vf, u, slb, sub = c["args"]
    pol = ilqr.backwardPass_ilqr_box(pytrees.AffineDynamics(*dyn), pytrees.QuadraticCostFunction(*cst), pytrees.QuadraticValueFunction(*Vf), u, slb, sub)
    raw = _box_sweep(_lib, models, dyn, cst, Vf, u, slb, sub)
    assert np.array_equal(pol.l, raw[0]) and np.array_equal(pol.L, raw[1])
