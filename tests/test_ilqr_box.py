"""CPU tests of the input box (control-limited iLQR): the NumPy restatement tests/ilqr_box_ref.py against closed forms, against the
oracle without bounds and against an independent QP solver; the strict-complementarity margins of every case the GPU tests use
(tests/ilqr_box_cases.py); the host-side refusals of models.InputBox and the drivers.  No GPU."""
import numpy as np
import pytest

from oracle import mpc_oracle as mo
from oracle import zopt_oracle as zo
from tests import ilqr_box_cases as cases
from tests import ilqr_box_ref as br
from tests import problems


def test_one_input_closed_form():
    """m = 1: l = clip(-Q_u / Q_uu, lb - u, ub - u), and L = 0 where it is clamped, -Q_ux / Q_uu where it is not"""
    rng = np.random.default_rng(3)
    seen = set()
    for _ in range(60):
        n = 3
        Q_uu, Q_u, Q_ux = np.array([[rng.uniform(0.5, 3)]]), rng.standard_normal(1) * 2, rng.standard_normal((1, n))
        Q_x, M = rng.standard_normal(n), rng.standard_normal((n, n))
        Q_xx = M @ M.T + np.eye(n)
        lo, hi = np.array([-rng.uniform(0.1, 1)]), np.array([rng.uniform(0.1, 1)])
        for ld in (False, True):
            v_x, v_xx, l, L, mask, margin = br.box_tail(Q_x, Q_u, Q_xx, Q_uu, Q_ux, lo, hi, ld)
            free = -Q_u[0] / Q_uu[0, 0]
            want = min(max(free, lo[0]), hi[0])
            assert abs(float(l[0]) - want) <= 1e-15 * max(1, abs(want))
            clamped = free < lo[0] or free > hi[0]
            assert mask == int(clamped)
            if clamped:
                assert not np.any(L) and float(l[0]) in (lo[0], hi[0])
                assert np.allclose(np.asarray(v_x, dtype=float), Q_x + Q_ux[0] * want, rtol=1e-14, atol=1e-14)
                assert np.allclose(np.asarray(v_xx, dtype=float), Q_xx, rtol=1e-14, atol=1e-14)
            else:
                assert np.allclose(np.asarray(L, dtype=float), -Q_ux / Q_uu[0, 0], rtol=1e-14)
            seen.add((clamped, free < 0))
    assert len(seen) == 4                                        # both bounds and both signs of a free step were met


def test_enumeration_returns_the_planted_solution():
    """every box-QP of the GPU table: the long-double enumerator finds the pattern and the point the problem was built from, the fp64
    one the same pattern; every margin is at least cases.MARGIN"""
    total = 0
    for m in (1, 2, 3, 4):
        t = cases.qp_problems(m)
        total += len(t["family"])
        assert np.all(t["margin"] >= cases.MARGIN), (m, t["family"][t["margin"] < cases.MARGIN], t["margin"].min())
        assert np.array_equal(t["clamped"], t["clamped64"])
        inside = (t["d"] >= t["lo"]) & (t["d"] <= t["hi"])
        assert inside.all()
        assert set(t["family"]) == {"plain", "all", "single", "mixed", "inf", "fixed", "cond", "scaled"}
        assert not t["clamped"][t["family"] == "plain"].any()
        assert np.all(t["clamped"][t["family"] == "all"] == (1 << m) - 1)
        assert sorted(t["clamped"][t["family"] == "single"]) == sorted([1 << i for i in range(m)] * 2)
        assert max(t["bound"].values()) <= 1e-4                  # cond(H) = 1e8 at the worst: the bounds stay meaningful
        if m > 1:
            assert max(np.linalg.cond(H) for H in t["H"][t["family"] == "cond"]) >= 0.9e8
    assert 150 <= total <= 250
    d, mask, margin = br.boxqp_enum(np.eye(2), np.array([np.nan, 1.0]), -np.ones(2), np.ones(2))
    assert np.isnan(d).all() and mask == 0


def test_infinite_bounds_reproduce_the_oracle():
    """no bound: the box backward pass is zo.backwardPass_ilqr (same pattern: nothing clamped; same policy to rounding), and the box
    loop follows zo.iterativeLqr iteration by iteration -- the same step indices, the costs to 1e-12"""
    for n, m, T in ((3, 2, 5), (12, 4, 7)):
        dyn, cost, Vf = problems.random_ilqr_model(3, T, n, m, seed=n)
        pol = zo.backwardPass_ilqr(zo.AffineDynamics(*dyn), zo.QuadraticCostFunction(*cost), zo.QuadraticValueFunction(*Vf))
        o = br.box_backward_batch(dyn, cost, Vf, np.zeros((3, T, m)), np.full(m, -np.inf), np.full(m, np.inf))
        assert not o["clamped"].any() and np.all(np.isinf(o["margin"]))
        assert np.max(np.abs(o["l"] - pol.l)) <= 1e-11 * np.max(np.abs(pol.l))
        assert np.max(np.abs(o["L"] - pol.L)) <= 1e-11 * np.max(np.abs(pol.L))
    rng = np.random.default_rng(8)
    step = zo.quad_euler_step(0.1)
    Q, R, Qf = np.eye(12), 0.5 * np.eye(4), 10 * np.eye(12)
    x0 = np.zeros(12)
    x0[9:12] = rng.uniform(-2, 2, 3)
    ug = np.tile(cases.U_TRIM, (7, 1))
    tr, trb = [], []
    ref = zo.iterativeLqr(step, Q, R, Qf, x0, ug, maxIter=6, tol=1e-6, return_iters=True, trace=tr)
    box = br.iterativeLqr(step, Q, R, Qf, x0, ug, -np.inf, np.inf, maxIter=6, tol=1e-6, return_iters=True, trace=trb)
    assert ref[4] == box[4] and ref[3] == box[3] and len(tr) == len(trb)
    for (J, idx, _), (Jb, idxb, _, mask, _) in zip(tr, trb):
        assert idx == idxb and abs(J - Jb) <= 1e-12 * abs(J) and not mask.any()
    assert np.max(np.abs(ref[0].uTraj - box[0].uTraj)) <= 1e-9


@pytest.mark.parametrize("case", cases.CONVEX_CASES, ids=lambda c: f"n{c[0]}m{c[1]}")
def test_convex_problem_against_an_independent_solver(case):
    """a linear model with a quadratic cost and a box is a convex QP: the loop's answer satisfies the KKT conditions (mpc_oracle's
    certificate, no state bounds) to 1e-12, its cost is not above the optimum SciPy's trust-constr finds, every step of every
    backward pass has a margin of at least 1e-3.  Figures of the two cases: 4 resp. 6 iterations, 7 of 14 resp. 4 of 28 inputs at a
    bound, winning step indices all 0 resp. 1, 1, 1, 0, 0, 0, stat <= 1.4e-14, J below SciPy's by ~1e-7."""
    n, m, N, seed, box = case
    c, r = cases.convex_case(*case), cases.convex_reference(*case)
    inf = np.full(n, np.inf)
    _, _, J_ref = mo.solve_reference(c["A"], c["B"], c["Q"], c["R"], c["Qf"], N, -inf, inf, c["lb"], c["ub"], c["x0"])
    margin = min(float(np.min(t[4])) for t in r["trace"])
    print(f"convex {case}: iterations {r['its']}, at a bound {int(r['at_bound'].sum())} of {r['at_bound'].size}, indices "
          f"{[t[1] for t in r['trace']]}, stat {r['stat']:.2e}, margin {margin:.2e}, J - J_scipy {r['J'] - J_ref:.2e}")
    assert r["converged"]
    assert r["stat"] < 1e-12
    assert r["J"] <= J_ref
    assert margin >= 1e-3
    assert r["at_bound"].any() and not r["at_bound"].all()
    assert np.all(r["traj"].uTraj >= c["lb"]) and np.all(r["traj"].uTraj <= c["ub"])
    assert (r["its"], int(r["at_bound"].sum())) == ((4, 7) if n == 3 else (6, 4))
    assert [t[1] for t in r["trace"]] == ([0, 0, 0, 0] if n == 3 else [1, 1, 1, 0, 0, 0])


@pytest.mark.parametrize("family", cases.SWEEP_FAMILIES)
def test_sweep_cases_have_a_margin(family):
    """every step of every trajectory of the GPU sweep table: margin >= MARGIN in the long-double reference, and the fp64 restatement
    finds the same clamped sets.  The families do what they are there for."""
    clamped_steps = free_on_bound = clamped_on_bound = comps = 0
    for shape in cases.SWEEP_SHAPES:
        c = cases.sweep_case(family, *shape)
        assert np.all(c["ref"]["margin"] >= cases.MARGIN), (family, shape, c["ref"]["margin"].min())
        assert c["same64"], (family, shape)
        bl, bL = cases.sweep_bounds(family, *shape)
        assert bl <= 1e-6 and bL <= 1e-6, (family, shape, bl, bL)
        n, m = shape[:2]
        mask = c["ref"]["clamped"]
        bits = np.stack([(mask >> i) & 1 for i in range(m)])        # (m, batch, T)
        clamped_steps += int(bits.sum())
        comps += bits.size
        if family == "onbound":
            l0 = np.asarray(c["ref"]["l"][..., 0], dtype=float)
            clamped_on_bound += int(np.sum((bits[0] == 1) & (l0 == 0.0)))   # (a clamped one may also have crossed to the upper bound)
            free_on_bound += int(np.sum(bits[0] == 0))
            assert np.all(l0[bits[0] == 0] > 0.0)
    assert 0 < clamped_steps < comps
    if family == "cheap":
        assert clamped_steps > 0.3 * comps                       # many clamps
    if family == "onbound":
        assert clamped_on_bound > 0 and free_on_bound > 0        # the gradient pushed outward and inward


@pytest.mark.parametrize("name", cases.SOLVE_CASES)
def test_solve_cases_have_a_margin(name):
    """every backward step the restatement takes on the GPU solve table: margin >= MARGIN, and every line search is decided by more
    than rounding (so the GPU test may compare step indices); the box is active somewhere and every stored input is feasible"""
    c = cases.solve_case(name)
    clamps = 0
    for b, r in enumerate(cases.solve_reference(name)):
        for (Jn, idx, Js, mask, margin) in r["trace"]:
            assert np.all(margin >= cases.MARGIN), (name, b, margin.min())
            # ... and the line search has a winner: the best cost is below the next one by more than the kernels' rounding
            # (step sizes whose rollouts clip to the same inputs tie exactly, in every implementation: the first of them wins)
            assert np.all((Js == Jn) | (Js - Jn >= 1e-9 * abs(Jn))), (name, b, idx, np.sort(Js)[:3] - Jn)
            clamps += int(np.count_nonzero(mask))
        assert np.all(r["traj"].uTraj >= c["lb"]) and np.all(r["traj"].uTraj <= c["ub"])
        assert 1 <= r["its"] <= 8
    assert clamps > 0
    for case in cases.CONVEX_CASES:
        assert min(float(np.min(t[4])) for t in cases.convex_reference(*case)["trace"]) >= cases.MARGIN


def test_host_side_refusals():
    from zopt_amd import ilqrUtils, models
    lin = models.LinearModel(np.eye(3), np.ones((3, 2)))
    with pytest.raises(ValueError, match="u_lb > u_ub"):
        models.InputBox(lin, [0.0, 1.0], [1.0, 0.5])
    with pytest.raises(ValueError, match="NaN"):
        models.InputBox(lin, [0.0, np.nan], [1.0, 1.0])
    with pytest.raises(ValueError, match="NaN"):
        models.InputBox(lin, -1.0, np.array([1.0, np.nan]))
    with pytest.raises(ValueError, match="shape"):
        models.InputBox(lin, np.zeros(3), np.ones(3))
    with pytest.raises(TypeError, match="registered device model"):
        models.InputBox(lambda x, u: x, -1.0, 1.0)
    with pytest.raises(TypeError, match="InputBox already"):
        models.InputBox(models.InputBox(lin, -1.0, 1.0), -1.0, 1.0)
    with pytest.raises(ValueError, match="not covered"):
        models.InputBox(models.LinearModel(np.eye(13), np.ones((13, 2))), -1.0, 1.0)
    with pytest.raises(ValueError, match="not covered"):
        models.InputBox(models.LinearModel(np.eye(6), np.ones((6, 5))), -1.0, 1.0)
    box = models.InputBox(lin, -np.inf, [1.0, np.inf])            # scalars broadcast; lb == ub is allowed
    assert box.u_lb.shape == (2,) and box.n == 3 and box.m == 2
    models.InputBox(lin, [0.5, -1.0], [0.5, 1.0])
    assert np.array_equal(models.InputBox(lin, -1.0, 1.0).clip(np.array([-3.0, 0.5])), [-1.0, 0.5])
    cost = models.QuadraticCost(np.eye(3), np.eye(2))
    with pytest.raises(ValueError, match="takes no InputBox"):
        ilqrUtils.differentialDynamicProgramming(box, cost, cost, np.zeros(3), np.zeros((4, 2)))
    with pytest.raises(ValueError, match="do not broadcast"):
        models.InputBox(lin, np.zeros((3, 2)), np.ones((4, 2)))
    assert not hasattr(box, "c_struct") and not callable(box)    # nothing that knows no box takes one for a model or a callable
    with pytest.raises(ValueError, match="not covered"):
        ilqrUtils.backwardPass_ilqr_box((None, np.zeros((2, 13, 13)), np.zeros((2, 13, 2))), (None,) * 6, (None,) * 3, None, -1.0, 1.0)
