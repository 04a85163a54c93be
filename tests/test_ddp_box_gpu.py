"""GPU tests of DDP with an input box (control-limited DDP with the second-order dynamics terms): the box DDP sweep
(ddp_backward_box_t16_f64 behind zm_ddp_backward_box[_list]_f64 and zm_ddp_backward_pairs_box_list_f64) and the box DDP solve
(zm_ilqr_solve_box_f64 with ddp = 1, through differentialDynamicProgramming(InputBox(...))) against the long-double and fp64
restatement of tests/ddp_box_ref.py, against the sweep without a box (infinite bounds) and against each other.

The cases and their bounds come from tests/ddp_box_cases.py; tests/test_ddp_box.py asserts on the CPU that every one of them has a
strict-complementarity margin and clamped sets that the projection's resolution cannot move, so clamped sets are compared exactly
here.  Batches <= 5, horizons <= 7."""
import ctypes

import numpy as np
import pytest

from tests import ddp_box_cases as cases
from tests import hp_reference as hp
from tests import problems
from tests.test_ilqr_box_gpu import _box, _p, _pattern
from tests.test_ilqr_tracking_gpu import _dev

pytestmark = pytest.mark.gpu
INF = np.inf
FILL = 7.0


@pytest.fixture(scope="module")
def mods():
    import torch
    assert torch.cuda.is_available()
    from zopt_amd import _lib, ilqrUtils, models, pytrees
    return ilqrUtils, models, pytrees, _lib


def _sweep(_lib, models, dyn, cost, Vf, u, lb, ub, ids=None, act=None, shared=False, form="full"):
    """zm_ddp_backward_box_list_f64 (form "full": the three tensors, "null": f_ux = f_uu = NULL) or zm_ddp_backward_pairs_box_list_f64
    (form "pairs": f_xx as the quadcopter's pair rows) -> (l, L, qp_capped); untouched rows keep the fill value (qp_capped: 0)"""
    import torch
    lib = _lib.lib()
    B, T, n, m = np.asarray(dyn[2]).shape
    ops = [cost[1], cost[2], cost[3], cost[4], cost[5], Vf[1], Vf[2], u]
    if shared:               # one time-invariant Hessian set: the first step's of the first trajectory
        ops[2:5] = [np.asarray(cost[i])[0, 0] for i in (3, 4, 5)]
        ops[6] = np.asarray(Vf[2])[0]
    d = [_dev(np.asarray(a, dtype=np.float64)) for a in ops]
    fx, fu = _dev(np.asarray(dyn[1])), _dev(np.asarray(dyn[2]))
    bs, keep = _box(models, lb, ub, m)
    l = torch.full((B, T, m), FILL, dtype=torch.float64, device="cuda")
    L = torch.full((B, T, m, n), FILL, dtype=torch.float64, device="cuda")
    cap = torch.zeros(B, dtype=torch.int32, device="cuda")
    dids = None if ids is None else _dev(np.asarray(ids), torch.int32)
    dact = None if act is None else _dev(act, torch.int32)
    tail = (ctypes.addressof(bs), _p(dids), 0 if ids is None else len(ids), _p(dact), 1 if shared else 0, _p(l), _p(L), _p(cap), B, T)
    if form == "pairs":
        assert (n, m) == (12, 4)
        md = models.QuadcopterEuler(0.1).c_struct()
        H = _dev(cases.pair_rows(np.asarray(dyn[3])))
        rc = lib.zm_ddp_backward_pairs_box_list_f64(ctypes.addressof(md), _p(fx), _p(fu), _p(H), *[_p(t) for t in d], *tail, None)
    else:
        fxx = _dev(np.asarray(dyn[3]))
        fux, fuu = (None, None) if form == "null" else (_dev(np.asarray(dyn[4])), _dev(np.asarray(dyn[5])))
        rc = lib.zm_ddp_backward_box_list_f64(_p(fx), _p(fu), _p(fxx), _p(fux), _p(fuu), *[_p(t) for t in d], *tail, n, m, None)
    assert rc == 0, lib.zm_last_error()
    torch.cuda.synchronize()
    return l.cpu().numpy(), L.cpu().numpy(), cap.cpu().numpy()


def _form(dyn):
    return "full" if (np.any(dyn[4]) or np.any(dyn[5])) else "null"


# ------------------------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("family", cases.SWEEP_FAMILIES)
def test_box_ddp_sweep_against_the_long_double_box_ddp_sweep(mods, family):
    """l, L and the clamped pattern (the zero rows of L), per trajectory and per step, with hp.sweep_metric / hp.ddp_bounds; no QP
    reaches its cap; u + l stays inside the box"""
    _, models, _, _lib = mods
    report = []
    for shape in cases.family_shapes(family):
        c = cases.sweep_case(family, *shape)
        bl, bL = cases.sweep_bounds(family, *shape)
        l, L, cap = _sweep(_lib, models, *c["args"], form=_form(c["args"][0]))
        el, eL = float(hp.sweep_metric(l, c["ref"]["l"]).max()), float(hp.sweep_metric(L, c["ref"]["L"]).max())
        report.append((shape, el, bl, eL, bL))
        print(f"box DDP sweep {family} {shape}: error of l {el:.2e} (bound {bl:.2e}), of L {eL:.2e} (bound {bL:.2e})")
        assert np.array_equal(_pattern(L), c["ref"]["clamped"]), (family, shape)
        assert not cap.any()
        assert el <= bl and eL <= bL, (family, report[-1])
        u, lb, ub = c["args"][3:]
        lo = np.expand_dims(np.broadcast_to(lb, (shape[3], shape[1])), 1) - u
        hi = np.expand_dims(np.broadcast_to(ub, (shape[3], shape[1])), 1) - u
        assert np.all(l >= lo) and np.all(l <= hi), (family, shape)


# ------------------------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("family", ["plain", "strongly_indefinite", "control_affine_8"])
def test_box_ddp_sweep_with_infinite_bounds_is_the_ddp_sweep(mods, family):
    """no bound: nothing is clamped and l, L agree with the long-double DDP sweep without a box under the bound the unboxed kernel
    (zm_ddp_backward_list_f64) is held to -- which is asserted for that kernel on the same inputs"""
    import torch
    _, models, _, _lib = mods
    lib = _lib.lib()
    for (n, m, T, B, _) in cases.SWEEP_SHAPES:
        c = cases.unbounded_case(family, n, m, T, B)
        bl, bL = cases.unbounded_bounds(family, n, m, T, B)
        dyn, cost, Vf = c["args"]
        l, L, cap = _sweep(_lib, models, dyn, cost, Vf, np.zeros((B, T, m)), np.full(m, -INF), np.full(m, INF), form=_form(dyn))
        d = [_dev(np.asarray(a)) for a in (dyn[1], dyn[2], dyn[3], dyn[4], dyn[5], cost[1], cost[2], cost[3], cost[4], cost[5], Vf[1], Vf[2])]
        pl, pL = torch.empty((B, T, m), dtype=torch.float64, device="cuda"), torch.empty((B, T, m, n), dtype=torch.float64, device="cuda")
        assert lib.zm_ddp_backward_list_f64(*[_p(t) for t in d], None, 0, None, 0, _p(pl), _p(pL), B, T, n, m, None) == 0
        torch.cuda.synchronize()
        for who, out_l, out_L in (("box", l, L), ("plain", pl.cpu().numpy(), pL.cpu().numpy())):
            el, eL = float(hp.sweep_metric(out_l, c["ref"]["l"]).max()), float(hp.sweep_metric(out_L, c["ref"]["L"]).max())
            print(f"infinite bounds {family} {(n, m, T, B)} {who}: error of l {el:.2e} (bound {bl:.2e}), of L {eL:.2e} (bound {bL:.2e})")
            assert el <= bl and eL <= bL, (family, (n, m, T, B), who)
        assert not _pattern(L).any() and not cap.any()


# ------------------------------------------------------------------------------------------------------------------------------- 6
def test_forms_of_the_second_derivatives_agree_bit_for_bit(mods):
    """the pairs entry against the full-tensor entry on `packed_pairs` (the same summation order, as include/zopt_amd.h promises), with
    per-step and with shared cost Hessians; NULL f_ux / f_uu against explicit zero tensors on `control_affine_8`; shared Hessians
    against per-step copies of the same matrices"""
    _, models, _, _lib = mods
    for shape in cases.family_shapes("packed_pairs"):
        a = cases.sweep_case("packed_pairs", *shape)["args"]
        for shared in (False, True):
            full = _sweep(_lib, models, *a, shared=shared, form="full")
            pairs = _sweep(_lib, models, *a, shared=shared, form="pairs")
            for x, y in zip(pairs, full):
                assert np.array_equal(x, y), ("pairs", shape, shared)
            assert _pattern(full[1]).any()
    for shape in cases.family_shapes("control_affine_8"):
        a = cases.sweep_case("control_affine_8", *shape)["args"]
        assert not np.any(a[0][4]) and not np.any(a[0][5])
        for x, y in zip(_sweep(_lib, models, *a, form="null"), _sweep(_lib, models, *a, form="full")):
            assert np.array_equal(x, y), ("null", shape)
    for shape in ((3, 2, 5, 5, True), (12, 4, 6, 3, False)):
        dyn, cost, Vf, u, lb, ub = cases.sweep_case("plain", *shape)["args"]
        _, cost1, Vf1 = problems.share_hessians(dyn[:3], cost, Vf)
        for x, y in zip(_sweep(_lib, models, dyn, cost1, Vf1, u, lb, ub, shared=True), _sweep(_lib, models, dyn, cost1, Vf1, u, lb, ub)):
            assert np.array_equal(x, y), ("shared", shape)


# ------------------------------------------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize("shape", [(3, 2, 5, 5, True), (12, 4, 3, 5, True)], ids=lambda s: f"n{s[0]}m{s[1]}")
def test_box_ddp_sweep_list_and_mask(mods, shape):
    """a list with a gap and an `active` mask: listed, active trajectories get bit for bit what the dense call writes, every other
    row keeps its fill value; per-trajectory bounds are read by trajectory id, not by slot"""
    _, models, _, _lib = mods
    c = cases.sweep_case("plain", *shape)
    dense = _sweep(_lib, models, *c["args"])
    ids, act = [4, 1, 3, 0], np.ones(5, dtype=np.int32)
    act[3] = 0
    part = _sweep(_lib, models, *c["args"], ids=ids, act=act)
    for b in range(5):
        for a, d in zip(part[:2], dense[:2]):
            assert np.array_equal(a[b], d[b]) if b in (4, 1, 0) else np.all(a[b] == FILL), (shape, b)
    masked = _sweep(_lib, models, *c["args"], act=act)
    for a, d in zip(masked[:2], dense[:2]):
        assert np.array_equal(a[act == 1], d[act == 1]) and np.all(a[3] == FILL)
    lb, ub = c["args"][4:]
    assert not np.array_equal(lb[4], lb[1])                      # (the bounds do differ between the trajectories)


# ------------------------------------------------------------------------------------------------------------------------------- 8
def _solve(ilqr, models, c, ddp=True, box=True, **over):
    """the case through differentialDynamicProgramming (or iterativeLqr) on InputBox(model, lb, ub) (or the bare model)
    -> (xTraj, uTraj, L, J, converged, J_trace, alpha_trace, qp_capped, iterations)"""
    model = (models.QuadcopterRigidBody if c["model"][0] == "rb" else models.QuadcopterEuler)(c["model"][1])
    xRef = over.pop("xRef", c["xRef"])
    cost = models.QuadraticCost(c["Q"], c["R"], c["Qf"]) if xRef is None else models.TrackingCost(c["Q"], c["R"], c["Qf"], xRef, c["uRef"])
    lb, ub = over.pop("lb", c["lb"]), over.pop("ub", c["ub"])
    x0, ug = over.pop("x0", c["x0"]), over.pop("ug", c["ug"])
    ilqr._TRACE = []
    try:
        drive = ilqr.differentialDynamicProgramming if ddp else ilqr.iterativeLqr
        traj, L, J, conv = drive(models.InputBox(model, lb, ub) if box else model, cost, cost, x0, ug, **c["kw"])
        rec = dict(ilqr._TRACE)
    finally:
        ilqr._TRACE = None
    return traj.xTraj, traj.uTraj, L, J, conv, rec["J_trace"], rec["alpha_trace"], rec.get("qp_capped"), rec["iterations"]


@pytest.mark.parametrize("name", cases.SOLVE_CASES)
def test_box_ddp_solves_follow_the_restatement_iteration_by_iteration(mods, name):
    """zm_ilqr_solve_box_trace_f64 with ddp = 1 against the restatement, per trajectory: the same `converged`, the same number of
    iterations (the cost is frozen from the restatement's last iteration on), in every iteration the winning step index and the
    accepted cost to 1e-9 relative; every stored input inside the box, no QP capped.  `rb` is the rigid-body model, which declares no
    Hessian pairs: the full-tensor branch of the solve (f_ux, f_uu through the workspace); its index is compared wherever the
    restatement's two best costs do not tie (tests/ddp_box_cases.py)."""
    ilqr, models, _, _ = mods
    c = cases.solve_case(name)
    xT, uT, L, J, conv, Jtr, atr, cap, its = _solve(ilqr, models, c)
    assert np.all(uT >= c["lb"]) and np.all(uT <= c["ub"]) and not cap.any()
    assert np.any((uT == c["lb"]) | (uT == c["ub"]))
    ref = cases.solve_reference(name)
    assert its >= max(r["its"] for r in ref)
    for b, r in enumerate(ref):
        print(f"box DDP solve {name} trajectory {b}: restatement iterations {r['its']}, converged {r['converged']}; device costs "
              f"{Jtr[:, b].tolist()}, indices {atr[:, b].tolist()}; restatement {[(t[0], t[1]) for t in r['trace']]}")
        assert bool(conv[b]) == r["converged"], (name, b)
        for k, (J_new, idx, _, _, _) in enumerate(r["trace"]):
            if cases.index_comparable(r["trace"][k][2]):              # (rb: not where the two best costs tie exactly)
                assert int(atr[k, b]) == idx, (name, b, k)
            assert abs(Jtr[k, b] - J_new) <= 1e-9 * abs(J_new), (name, b, k, Jtr[k, b], J_new)
        assert np.all(Jtr[r["its"] - 1:, b] == Jtr[r["its"] - 1, b]), (name, b)          # it iterated no further
        assert J[b] == Jtr[r["its"] - 1, b]
        assert np.array_equal(_pattern(L[b][None])[0], r["trace"][-1][3]), (name, b)


# ------------------------------------------------------------------------------------------------------------------------------- 9
@pytest.mark.parametrize("name", cases.SOLVE_CASES)
def test_infinite_bounds_through_differentialDynamicProgramming(mods, name):
    """differentialDynamicProgramming(InputBox(model, -inf, inf), ...) follows the plain DDP solve of the same problem: J_trace to
    1e-9 relative, alpha_trace and the iteration count equal"""
    ilqr, models, _, _ = mods
    c = cases.solve_case(name)
    box = _solve(ilqr, models, c, lb=-INF, ub=INF)
    plain = _solve(ilqr, models, c, box=False)
    print(f"infinite bounds {name}: iterations {box[8]} / {plain[8]}, largest relative cost difference "
          f"{np.max(np.abs(box[5] - plain[5]) / np.abs(plain[5])) if box[5].shape == plain[5].shape else None}")
    assert box[8] == plain[8] and box[5].shape == plain[5].shape and not box[7].any()
    assert np.all(np.abs(box[5] - plain[5]) <= 1e-9 * np.abs(plain[5]))
    assert np.array_equal(box[6], plain[6])
    assert np.array_equal(box[4], plain[4])


# ------------------------------------------------------------------------------------------------------------------------------ 10
@pytest.mark.parametrize("name", ["quad_hover", "rb"])
def test_a_batch_member_solved_alone_and_per_trajectory_bounds(mods, name):
    """a member of the batch solved alone gives the same bits (trace included); so does the batch with the shared box written out
    per trajectory -- and then each trajectory follows its own box.  Every stored input is feasible, no QP capped."""
    ilqr, models, _, _ = mods
    c = cases.solve_case(name)
    B = c["ug"].shape[0]
    full = _solve(ilqr, models, c)
    assert np.all(full[1] >= c["lb"]) and np.all(full[1] <= c["ub"]) and not full[7].any()
    for b in (0, 3):
        alone = _solve(ilqr, models, c, xRef=None if c["xRef"] is None else c["xRef"][b:b + 1], x0=c["x0"][b:b + 1], ug=c["ug"][b:b + 1])
        for a, f in zip(alone[:5], full[:5]):
            assert np.array_equal(a[0], f[b], equal_nan=True), b
        its = alone[5].shape[0]
        assert np.array_equal(alone[5][:, 0], full[5][:its, b], equal_nan=True), b
    per = _solve(ilqr, models, c, lb=np.tile(c["lb"], (B, 1)), ub=np.tile(c["ub"], (B, 1)))
    for a, f in zip(per[:7], full[:7]):
        assert np.array_equal(a, f, equal_nan=True)
    lb2, ub2 = np.tile(c["lb"], (B, 1)), np.tile(c["ub"], (B, 1))
    lb2[1], ub2[1] = -INF, INF                                   # trajectory 1 without a box: it leaves the others' alone
    mixed = _solve(ilqr, models, c, lb=lb2, ub=ub2)
    free = _solve(ilqr, models, c, lb=-INF, ub=INF)
    for a, f, g in zip(mixed[:5], full[:5], free[:5]):
        assert np.array_equal(np.delete(a, 1, axis=0), np.delete(f, 1, axis=0), equal_nan=True) and np.array_equal(a[1], g[1], equal_nan=True)


# ------------------------------------------------------------------------------------------------------------------------------ 11
def test_backwardPass_ddp_box(mods):
    """the array-level wrapper with NumPy and with torch inputs, with a leading batch axis and without, with f_ux = f_uu = None: the
    bits of the C entry"""
    import torch
    ilqr, models, pytrees, _lib = mods
    for shape in ((3, 2, 5, 5, True), (12, 4, 6, 3, False)):
        dyn, cost, Vf, u, lb, ub = cases.sweep_case("plain", *shape)["args"]
        raw = _sweep(_lib, models, dyn, cost, Vf, u, lb, ub)
        on = lambda f, tup: [None if t is None else f(t) for t in tup]      # noqa: E731
        wrap = lambda f: (pytrees.QuadraticDynamics(*on(f, dyn)), pytrees.QuadraticCostFunction(*on(f, cost)),      # noqa: E731
                          pytrees.QuadraticValueFunction(*on(f, Vf)), f(u))
        pol = ilqr.backwardPass_ddp_box(*wrap(np.asarray), lb, ub)
        assert isinstance(pol.l, np.ndarray) and np.array_equal(pol.l, raw[0]) and np.array_equal(pol.L, raw[1])
        tpol = ilqr.backwardPass_ddp_box(*wrap(lambda t: torch.as_tensor(np.asarray(t), device="cuda")), lb, ub)
        assert torch.is_tensor(tpol.L) and np.array_equal(tpol.l.cpu().numpy(), raw[0]) and np.array_equal(tpol.L.cpu().numpy(), raw[1])
        b = 2
        one = ilqr.backwardPass_ddp_box(*wrap(lambda t: np.asarray(t)[b]), lb[b] if np.ndim(lb) == 2 else lb, ub[b] if np.ndim(ub) == 2 else ub)
        assert one.l.shape == raw[0][b].shape and np.array_equal(one.l, raw[0][b]) and np.array_equal(one.L, raw[1][b])
    # dynamics affine in the controls: f_ux = f_uu = None go through as NULL
    dyn, cost, Vf, u, lb, ub = cases.sweep_case("control_affine_8", 8, 4, 5, 3, False)["args"]
    raw = _sweep(_lib, models, dyn, cost, Vf, u, lb, ub, form="null")
    pol = ilqr.backwardPass_ddp_box(pytrees.QuadraticDynamics(*dyn[:4], None, None), pytrees.QuadraticCostFunction(*cost),
                                    pytrees.QuadraticValueFunction(*Vf), u, lb, ub)
    assert np.array_equal(pol.l, raw[0]) and np.array_equal(pol.L, raw[1])
    with pytest.raises(ValueError, match="together"):
        ilqr.backwardPass_ddp_box(pytrees.QuadraticDynamics(*dyn[:5], None), pytrees.QuadraticCostFunction(*cost),
                                  pytrees.QuadraticValueFunction(*Vf), u, lb, ub)
