"""CPU tests of oracle.mpc_oracle.admm_levels, the NumPy restatement of the whole lqrMpc solve (adaptive penalty levels, warm and shifted
starts, tracking term and cycle guard) that tests/test_mpc_iterates_gpu.py holds the kernels to.  Without these the GPU tests would rest on
an unpinned reference: (a) with one level and no warm state it IS the two older fixed-penalty restatements, (b) its adaptive answers are
optimal by solver-independent checks, (c) it replays the documented history of the tracking kernel's cycle guard, (d) every input of the
GPU tests keeps the reference clear of rounding-sensitive decisions and covers what its test claims."""
import numpy as np
import pytest

from oracle import mpc_oracle as mo
from tests import mpc_iterates_cases as ic
from tests import mpc_tracking_ref as tr


# ---- a. one level, no warm state == the fixed-penalty restatements ---------------------------------------------------------------

def _quad_start():
    """instance 0 of tests/test_mpc_gpu.py: test_quadcopter_config3_batch"""
    x_ub = tr.quad_data(30)[6]
    rng = np.random.default_rng(1)
    x0 = np.clip(0.03 * rng.standard_normal((1024, 12)), -x_ub + 1e-6, x_ub - 1e-6)
    x0[:, 9:12] = rng.uniform(-10, 10, (1024, 3))
    return x0[0]


@pytest.mark.parametrize("alpha", [1.6, 1.0])
def test_one_level_equals_the_fixed_penalty_admm(alpha):
    """the inputs of test_quadcopter_config3_batch (300 iterations of them: the iterate, not the end, is compared), a small problem run to
    its end, and the dynamically infeasible problem of test_infeasible_instances: same iterates, same counts, exactly -- the two functions
    spell the same sums in the same order"""
    data = tr.quad_data(30)
    rho = tr.default_rho(data[2], data[3])
    x0 = _quad_start()
    kw = dict(rho=rho, eps_abs=1e-4, eps_rel=1e-4, max_iter=300, alpha=alpha)
    xo, uo, so, ito = mo.admm(*data[:5], 30, *data[5:], x0, **kw)
    r = mo.admm_levels(*data[:5], 30, *data[5:], x0, n_levels=1, **kw)
    assert ito == r.iters == 300 and so == "user_limit" and r.status in ("user_limit", "optimal_inaccurate") and not r.moves
    assert np.array_equal(r.x, xo) and np.array_equal(r.u, uo)
    data, x0s = ic._random(4, 2, 6, 42, 3)
    rho = tr.default_rho(data[2], data[3])
    for x0 in x0s:
        kw = dict(rho=rho, eps_abs=1e-6, eps_rel=1e-6, max_iter=30000, alpha=alpha)
        xo, uo, so, ito = mo.admm(*data[:5], 6, *data[5:], x0, **kw)
        r = mo.admm_levels(*data[:5], 6, *data[5:], x0, n_levels=1, **kw)
        assert so == r.status == "optimal" and ito == r.iters and ito > mo.CHECK_EVERY
        assert np.array_equal(r.x, xo) and np.array_equal(r.u, uo)
    I, one = np.eye(2), np.ones(2)
    bad = (2 * I, I, I, I, I, 3, -one, one, -0.1 * one, 0.1 * one, np.array([0.9, 0.9]))
    xo, uo, so, ito = mo.admm(*bad, rho=2.0, alpha=alpha)
    r = mo.admm_levels(*bad, rho=2.0, alpha=alpha, n_levels=1)
    assert so == r.status == "infeasible" and ito == r.iters and ito % mo.CHECK_EVERY == 0
    assert np.array_equal(r.x, xo) and np.array_equal(r.u, uo)


@pytest.mark.parametrize("alpha", [1.6, 1.0])
def test_one_level_equals_the_fixed_penalty_tracking_admm(alpha):
    """the inputs of test_iterates_equal_the_numpy_tracking_admm (300 iterations) and a small tracking problem run to its end.  The two
    spell the dual tolerance differently where rho |lam| dominates, eps_rel (rho |lam|) there and (eps_rel rho) |lam| here as the kernels
    do: one rounding of a threshold, which no iterate depends on"""
    N = 25
    data = tr.quad_data(N)
    x0, xRef, uRef = tr.quad_reference(N)
    rho = tr.default_rho(data[2], data[3])
    kw = dict(rho=rho, eps_abs=1e-4, eps_rel=1e-4, max_iter=300, alpha=alpha)
    xo, uo, so, ito = tr.admm(*data[:5], N, *data[5:], x0[0], xRef[0], uRef[0], **kw)
    r = mo.admm_levels(*data[:5], N, *data[5:], x0[0], n_levels=1, g=tr.linear_term(*data[2:5], N, xRef[0], uRef[0]), **kw)
    assert ito == r.iters == 300 and np.array_equal(r.x, xo) and np.array_equal(r.u, uo)
    data, x0, xRef, uRef = tr.random_case(4, 2, 6, seed=7, nb=3)
    rho = tr.default_rho(data[2], data[3])
    for b in range(3):
        kw = dict(rho=rho, eps_abs=1e-6, eps_rel=1e-6, max_iter=30000, alpha=alpha)
        xo, uo, so, ito = tr.admm(*data[:5], 6, *data[5:], x0[b], xRef[b], uRef[b], **kw)
        r = mo.admm_levels(*data[:5], 6, *data[5:], x0[b], n_levels=1, g=tr.linear_term(*data[2:5], 6, xRef[b], uRef[b]), **kw)
        assert so == r.status == "optimal" and ito == r.iters
        assert np.array_equal(r.x, xo) and np.array_equal(r.u, uo)


# ---- b. the adaptive answers are optimal by independent checks ---------------------------------------------------------------------

@pytest.mark.parametrize("n,m,N", [(2, 1, 6), (4, 2, 6)])
def test_adaptive_solutions_are_optimal(n, m, N):
    """the thresholds of test_constrained_small_problems_against_independent_solve (eps = 1e-6) and its 2e-3 against the SciPy solve"""
    data, x0s = ic._random(n, m, N, 10 * n + m, 4)
    rho = tr.default_rho(data[2], data[3])
    n_ref = 0
    for x0 in x0s:
        r = mo.admm_levels(*data[:5], N, *data[5:], x0, rho=rho, eps_abs=1e-6, eps_rel=1e-6, max_iter=30000)
        assert r.status == "optimal"
        kkt = mo.kkt_residuals(*data[:5], N, *data[5:], x0, r.x, r.u, act_tol=1e-4)
        assert kkt["dyn"] <= 1e-12 and kkt["bound"] <= 1e-4 and kkt["stat"] <= 1e-3, kkt
        if tr.n_active(r.x, r.u, *data[5:]) >= 1 and n_ref < 2:
            n_ref += 1
            xr, ur, fr = mo.solve_reference(*data[:5], N, *data[5:], x0)
            assert np.max(np.abs(r.u - ur)) <= 2e-3
    assert n_ref >= 1


# ---- c. the documented history of the cycle guard ------------------------------------------------------------------------------------

def test_cycle_guard_history():
    """mpc_wave.hip: ZM_TRK_LEVEL -- (4, 1, 8) seed 41, instance 0: with the guard the levels go 3 4 5 6 5 6, the next reversal is refused,
    the level locks and the solve ends "optimal"; without it levels 5 and 6 ask for each other at every check until the cap"""
    data, x0, xRef, uRef = tr.random_case(4, 1, 8, seed=41, nb=8)
    rho = tr.default_rho(data[2], data[3])
    g = tr.linear_term(*data[2:5], 8, xRef[0], uRef[0])
    kw = dict(rho=rho, eps_abs=1e-6, eps_rel=1e-6, g=g)
    on = mo.admm_levels(*data[:5], 8, *data[5:], x0[0], max_iter=30000, **kw)
    off = mo.admm_levels(*data[:5], 8, *data[5:], x0[0], max_iter=3000, guard=False, **kw)
    print(f"guard on: {on.status} in {on.iters} iterations, moves {on.moves}; off: {off.status}, {len(off.moves)} moves")
    assert on.locked and on.status == "optimal"
    assert [(a, b) for _, a, b in on.moves] == [(3, 4), (4, 5), (5, 6), (6, 5), (5, 6)]
    assert off.status == "user_limit" and not off.locked and off.iters == 3000
    assert {(a, b) for _, a, b in off.moves[-20:]} == {(5, 6), (6, 5)}


# ---- d. conditions on every input of tests/test_mpc_iterates_gpu.py -----------------------------------------------------------------

@pytest.mark.parametrize("group", list(ic.GROUPS))
def test_gpu_inputs_are_decisive_and_cover_their_claims(group):
    """Kernel and NumPy differ by ~1e-12 relative per iteration; a reference that never comes within 1e-4 of a level decision's rounding
    point nor within 1e-6 of the stopping threshold leaves four or more decades."""
    names, claimed = ic.GROUPS[group]
    seen, up, down, active, lm, sm = set(), 0, 0, 0, np.inf, np.inf
    for name in names:
        c = ic.build(name)
        for s, row in enumerate(ic.reference(name)):
            for b, r in enumerate(row):
                assert r.level_margin >= 1e-4 and r.stop_margin >= 1e-6, (name, s, b, r.level_margin, r.stop_margin)
                lm, sm = min(lm, r.level_margin), min(sm, r.stop_margin)
                seen.add(r.status)
                up += sum(b_ > a_ for _, a_, b_ in r.moves)
                down += sum(b_ < a_ for _, a_, b_ in r.moves)
                if r.status in ("optimal", "optimal_inaccurate"):
                    active += tr.n_active(r.x, r.u, *c.inst[b][5:]) >= 1
                if r.status in ("optimal_inaccurate", "user_limit"):    # the test at the cap is a decision too
                    assert r.near_margin >= 1e-6, (name, s, b)
    print(f"{group}: smallest level_margin {lm:.1e}, stop_margin {sm:.1e}; moves up {up}, down {down}; statuses {sorted(seen)}")
    assert seen == claimed and active >= 1
    if ic.build(names[0]).n_levels > 1:
        assert up >= 1 and down >= 1
    if group == "shapes":       # every compiled shape at two horizons of different N mod 3; N = 1, 2 at (12, 4)
        for shape in {(n, m) for n, m, _ in ic.SHAPES}:
            assert len({N % 3 for n, m, N in ic.SHAPES if (n, m) == shape}) >= 2
        assert {(12, 4, 1), (12, 4, 2)} <= set(ic.SHAPES) and {N for _, _, N in ic.SHAPES} == {1, 2, 3, 4, 5, 7}
        assert all(r[3].status == "infeasible" and r[3].iters == 0 for name in names for r in ic.reference(name))
    if group == "warm":         # exactly one slot is held back by the first call's cap and restarts cold; the others restart warm
        for name in names:
            first = ic.reference(name)[0]
            assert sum(r.status != "optimal" for r in first) == 1
    if group == "per_problem":  # the problems of one wave differ
        for name in names:
            A = ic.build(name).ctor[0]
            assert all(not np.array_equal(A[i], A[j]) for i in range(4) for j in range(i))
    if group == "tracking":     # instance 0 of the (4, 1, 8) batch locks, nothing else does
        locked = [(name, b) for name in names for b, r in enumerate(ic.reference(name)[0]) if r.locked]
        assert locked == [("track:4,1,8", 0)]
    if group == "infeasible":
        assert ic.reference(names[0])[0][0].iters % mo.CHECK_EVERY == 0
