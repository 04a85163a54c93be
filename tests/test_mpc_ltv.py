"""CPU checks for mpcUtils.ltvMpc (stage-varying dynamics x+ = A_k x + B_k u + c_k): the NumPy restatement of the kernels
(tests/mpc_ltv_ref.py: admm_levels_ltv) against the restatement of the time-invariant solve and against an independent SciPy solve,
the infeasibility certificate through the offset, the cycle guard, the decisiveness of every input of tests/test_mpc_ltv_gpu.py, and the
host-side checks of the constructor.  No GPU."""
import numpy as np
import pytest

from oracle import mpc_oracle as mo
from tests import mpc_ltv_ref as lr
from tests import mpc_tracking_ref as tr
from tests.test_mpc_gpu import _random_problem
from zopt_amd import mpcUtils


def _lti(n, m, N, nb=3):
    rng = np.random.default_rng(1000 * n + 10 * m + N)
    A, B, Q, R, Qf = _random_problem(rng, n, m, N)
    x_ub, u_ub = np.full(n, 4.0), np.full(m, 0.15)
    return (A, B, Q, R, Qf, -x_ub, x_ub, -u_ub, u_ub), rng.uniform(-1.0, 1.0, (nb, n))


def _same(a, b):
    assert a.status == b.status and a.iters == b.iters and a.moves == b.moves and a.level == b.level and a.locked == b.locked
    for k in ("x", "u", "y", "lam"):
        assert np.max(np.abs(getattr(a, k) - getattr(b, k))) <= 1e-12, k


@pytest.mark.parametrize("n,m,N", [(4, 2, 4), (12, 4, 7), (2, 1, 5)])
def test_constant_dynamics_and_zero_offset_are_the_time_invariant_solve(n, m, N):
    """constant A_k, B_k and c = 0: admm_levels_ltv is admm_levels -- status, iterations, level moves, and x, u, y, lam to 1e-12; cold, then
    a warm and a shifted solve each fed its own previous state.  (Both are adapters of oracle.mpc_oracle.admm_levels_stage now: this
    holds the tiling of A, B and c = None to the stage-varying data.)"""
    (A, B, Q, R, Qf, xl, xu, ul, uu), x0 = _lti(n, m, N)
    Ak, Bk = np.tile(A, (N, 1, 1)), np.tile(B, (N, 1, 1))
    rho = tr.default_rho(Q, R)
    for b in range(len(x0)):
        kw = dict(rho=rho, eps_abs=1e-6, eps_rel=1e-6, max_iter=30000)
        ref = mo.admm_levels(A, B, Q, R, Qf, N, xl, xu, ul, uu, x0[b], **kw)
        got = lr.admm_levels_ltv(Ak, Bk, None, Q, R, Qf, N, xl, xu, ul, uu, x0[b], **kw)
        assert ref.status == "optimal"
        _same(got, ref)
        if b == 0:   # cold (loose) -> warm -> shift
            kw0 = dict(kw, eps_abs=1e-3, eps_rel=1e-3)
            r0, g0 = (f(*a, x0[b], **kw0) for f, a in ((mo.admm_levels, (A, B, Q, R, Qf, N, xl, xu, ul, uu)),
                                                       (lr.admm_levels_ltv, (Ak, Bk, None, Q, R, Qf, N, xl, xu, ul, uu))))
            _same(g0, r0)
            r1 = mo.admm_levels(A, B, Q, R, Qf, N, xl, xu, ul, uu, x0[b], warm=(r0.y, r0.lam, r0.level), **kw)
            g1 = lr.admm_levels_ltv(Ak, Bk, None, Q, R, Qf, N, xl, xu, ul, uu, x0[b], warm=(g0.y, g0.lam, g0.level), **kw)
            _same(g1, r1)
            r2 = mo.admm_levels(A, B, Q, R, Qf, N, xl, xu, ul, uu, r1.x[1], warm=(r1.y, r1.lam, r1.level), shift=True, **kw)
            g2 = lr.admm_levels_ltv(Ak, Bk, None, Q, R, Qf, N, xl, xu, ul, uu, g1.x[1], warm=(g1.y, g1.lam, g1.level), shift=True, **kw)
            _same(g2, r2)


def test_constant_dynamics_with_a_reference_are_the_tracking_solve():
    """g != 0: the linear term and the cycle guard as admm_levels has them"""
    n, m, N = 4, 1, 8
    (A, B, Q, R, Qf, xl, xu, ul, uu), x0, xRef, uRef = tr.random_case(n, m, N, seed=41, nb=3)
    Ak, Bk = np.tile(A, (N, 1, 1)), np.tile(B, (N, 1, 1))
    for b in range(3):
        g = tr.linear_term(Q, R, Qf, N, xRef[b], uRef[b])
        kw = dict(rho=tr.default_rho(Q, R), eps_abs=1e-6, eps_rel=1e-6, max_iter=30000, g=g)
        _same(lr.admm_levels_ltv(Ak, Bk, None, Q, R, Qf, N, xl, xu, ul, uu, x0[b], **kw),
              mo.admm_levels(A, B, Q, R, Qf, N, xl, xu, ul, uu, x0[b], **kw))


@pytest.mark.parametrize("n,m,N", lr.SCIPY_SHAPES)
def test_solutions_agree_with_an_independent_solve(n, m, N):
    """the recipe's stage-varying problems with offsets: the ADMM's solution is the QP's (condensed SciPy solve), to the tolerance of
    tests/test_mpc_levels_oracle.py::test_adaptive_solutions_are_optimal"""
    (A, B, c, Q, R, Qf, xl, xu, ul, uu), x0 = lr.recipe(n, m, N, 2)
    rho = tr.default_rho(Q, R)
    for b in range(2):
        r = lr.admm_levels_ltv(A, B, c, Q, R, Qf, N, xl, xu, ul, uu, x0[b], rho=rho, eps_abs=lr.EPS, eps_rel=lr.EPS, max_iter=lr.MAX_ITER)
        assert r.status == "optimal"
        xs, us, _ = lr.solve_reference_ltv(A, B, c, Q, R, Qf, N, xl, xu, ul, uu, x0[b])
        dev = np.max(np.abs(r.u - us))
        print(f"({n},{m},{N}) instance {b}: {r.iters} iterations, deviation of u from SciPy {dev:.2e}")
        assert dev <= 2e-3


def test_offset_makes_the_problem_infeasible():
    """x+ = x + u + c with |u| <= 0.1, |x| <= 1 from x0 = (0.5, 0): c = (1.5, 0) leaves the box at the first step whatever u does, and the
    certificate -- whose free response carries the offsets -- says so at a check; c = 0 is solved"""
    for offset, want in ((True, "infeasible"), (False, "optimal")):
        (A, B, c, Q, R, Qf, xl, xu, ul, uu), x0 = lr.infeasible_data(offset)
        r = lr.admm_levels_ltv(A, B, c, Q, R, Qf, 3, xl, xu, ul, uu, x0, rho=2.0)
        assert r.status == want, (offset, r.status, r.iters)
        if offset:
            assert r.iters % mo.CHECK_EVERY == 0 and r.iters <= 64, r.iters


def test_cycle_guard_is_needed_with_offsets():
    """instance 0 of the (12, 4, 7) recipe: without the guard two adjacent levels ask for each other at every check until the cap; with
    it the third reversal is refused, the level locked and the solve ends optimal"""
    (A, B, c, Q, R, Qf, xl, xu, ul, uu), x0 = lr.recipe(12, 4, 7, 1)
    kw = dict(rho=tr.default_rho(Q, R), eps_abs=lr.EPS, eps_rel=lr.EPS)
    free = lr.admm_levels_ltv(A, B, c, Q, R, Qf, 7, xl, xu, ul, uu, x0[0], max_iter=4000, guard=False, **kw)
    assert free.status == "user_limit" and len(free.moves) > 100, (free.status, len(free.moves))
    held = lr.admm_levels_ltv(A, B, c, Q, R, Qf, 7, xl, xu, ul, uu, x0[0], max_iter=lr.MAX_ITER, **kw)
    assert held.status == "optimal" and held.locked, (held.status, held.locked, held.iters)


@pytest.mark.parametrize("name", lr.ALL)
def test_gpu_cases_are_decisive(name):
    """every input of tests/test_mpc_ltv_gpu.py stays clear of every rounding-sensitive decision (the thresholds of
    tests/test_mpc_levels_oracle.py): no level decision within 1e-4 of a half-integer, no termination test within 1e-6 of its
    threshold, none at the cap within 1e-6 of the 10x test"""
    c = lr.build(name)
    cap = [step["kw"]["max_iter"] for step in c.steps]
    statuses = set()
    for s, row in enumerate(lr.reference(name)):
        for b, r in enumerate(row):
            statuses.add(r.status)
            at = (name, s, b, r.status, r.iters)
            assert r.level_margin >= 1e-4 and r.stop_margin >= 1e-6, (at, r.level_margin, r.stop_margin)
            if r.iters == cap[s]:
                assert r.near_margin >= 1e-6, (at, r.near_margin)
    if name.startswith("shape") or name == "infeasible":
        assert statuses == {"optimal", "infeasible"}, statuses
    else:
        assert statuses == {"optimal"}, statuses


def test_chain_case_covers_what_it_claims():
    """the chain's warm and shifted solves do start from the stored state, and the update changes the solution"""
    ref = lr.reference("chain")
    assert all(r.status == "optimal" for row in ref for r in row)
    cold = lr.reference_steps(lr.build("chain"), lr.case_rho(mpcUtils, lr.build("chain")),
                              solve=lambda *a, warm=None, shift=False, **kw: lr.admm_levels_ltv(*a, **kw))
    assert sum(r.iters for r in ref[1]) < sum(r.iters for r in cold[1])     # the warm refinement starts from the loose solve
    assert any(r.iters != q.iters for r, q in zip(ref[2], cold[2]))         # the shifted start is a different start
    assert any(np.max(np.abs(a.u - b.u)) > 1e-4 for a, b in zip(ref[2], ref[3]))


# ---- host-side checks of the constructor -------------------------------------------------------------------------------------------------

def _ctor(n=2, m=1, N=3, P=()):
    A = np.broadcast_to(0.5 * np.eye(n), P + (N, n, n)).copy()
    B = np.ones(P + (N, n, m))
    return dict(A=A, B=B, Q=np.eye(n), R=np.eye(m), N=N, x_lb=-np.ones(n), x_ub=np.ones(n), u_lb=-np.ones(m), u_ub=np.ones(m))


def test_constructor_is_host_only_and_refuses_bad_problems():
    prob = mpcUtils.ltvMpc(**_ctor())
    assert prob.P == () and (prob.n, prob.m) == (2, 1) and prob.c.shape == (3, 2) and not prob.c.any()
    assert mpcUtils.ltvMpc(**_ctor(P=(4,))).P == (4,)
    with pytest.raises(ValueError, match=r"stages, expected N = 3"):
        mpcUtils.ltvMpc(**dict(_ctor(), A=np.zeros((4, 2, 2))))
    with pytest.raises(ValueError, match=r"expected N = 3"):
        mpcUtils.ltvMpc(**_ctor(), c=np.zeros((2, 2)))
    with pytest.raises(ValueError, match="do not broadcast"):
        mpcUtils.ltvMpc(**dict(_ctor(P=(4,)), B=np.ones((3, 3, 2, 1))))
    with pytest.raises(ValueError, match=r"n <= 12"):
        mpcUtils.ltvMpc(**_ctor(n=13))
    with pytest.raises(ValueError, match=r"m <= 4"):
        mpcUtils.ltvMpc(**_ctor(m=5))
    with pytest.raises(ValueError, match=r"N <= 75"):
        mpcUtils.ltvMpc(**_ctor(N=76))
    mpcUtils.ltvMpc(**_ctor(N=75))
    with pytest.raises(ValueError, match="not positive semidefinite"):
        mpcUtils.ltvMpc(**dict(_ctor(), Q=np.diag([1.0, -0.1])))
    with pytest.raises(ValueError, match="shapes"):
        mpcUtils.ltvMpc(**dict(_ctor(), Q=np.eye(3)))
    with pytest.raises(NotImplementedError):
        prob.simulate(np.zeros(2), 5)
    with pytest.raises(ValueError, match=r"update: A has shape"):
        prob.update(A=np.zeros((2, 2)))


def test_embedding_pads_every_stage():
    """(3, 2) runs in the (4, 2) kernels: A_k, B_k get zero blocks, c_k a zero, the weights a unit diagonal, no bound on the padding"""
    rng = np.random.default_rng(0)
    d = _ctor(n=3, m=2, N=4, P=(2,))
    d["A"] = rng.standard_normal((2, 4, 3, 3))
    c = rng.standard_normal((4, 3))
    prob = mpcUtils.ltvMpc(**d, c=c)
    assert (prob.n, prob.m, prob._n_user, prob._m_user) == (4, 2, 3, 2)
    assert prob.A.shape == (2, 4, 4, 4) and np.array_equal(prob.A[..., :3, :3], d["A"]) and not prob.A[..., 3, :].any() and not prob.A[..., :, 3].any()
    assert prob.B.shape == (2, 4, 4, 2) and not prob.B[..., 3, :].any()
    assert prob.c.shape == (2, 4, 4) and np.array_equal(prob.c[..., :3], np.broadcast_to(c, (2, 4, 3))) and not prob.c[..., 3].any()
    assert prob.Q.shape == (2, 4, 4) and np.all(prob.Q[..., 3, 3] == 1.0) and np.all(np.isinf(prob.x_ub[..., 3]))


def test_from_expansion_forms_the_offset_in_absolute_coordinates():
    """x+ ~ f + f_x (x - xbar) + f_u (u - ubar): A = f_x, B = f_u, c = f - f_x xbar - f_u ubar, N the number of stages"""
    from zopt_amd.pytrees import AffineDynamics, Trajectory
    rng = np.random.default_rng(2)
    P, N, n, m = (3,), 5, 4, 2
    f, f_x, f_u = rng.standard_normal(P + (N, n)), rng.standard_normal(P + (N, n, n)), rng.standard_normal(P + (N, n, m))
    xbar, ubar = rng.standard_normal(P + (N + 1, n)), rng.standard_normal(P + (N, m))
    prob = mpcUtils.ltvMpc.fromExpansion(AffineDynamics(f, f_x, f_u), Trajectory(xbar, ubar), np.eye(n), np.eye(m), -np.ones(n), np.ones(n),
                                         -np.ones(m), np.ones(m))
    assert prob.N == N and prob.P == P and np.array_equal(prob.A, f_x) and np.array_equal(prob.B, f_u)
    want = np.stack([[f[p, k] - f_x[p, k] @ xbar[p, k] - f_u[p, k] @ ubar[p, k] for k in range(N)] for p in range(3)])
    assert np.max(np.abs(prob.c - want)) <= 1e-14
    # the expansion reproduces itself at the expansion point
    assert np.max(np.abs(np.einsum("pkij,pkj->pki", prob.A, xbar[:, :-1]) + np.einsum("pkij,pkj->pki", prob.B, ubar) + prob.c - f)) <= 1e-13


def test_c_abi_refuses_bad_arguments_without_a_gpu():
    from zopt_amd import _lib
    lib, d = _lib.lib(), 0x1000
    assert lib.zm_mpc_setup_ltv_f64(None, None, None, None, None, None, None, 4, 7, 10, 12, 4, None, None, None, None, None) == _lib.ZM_EINVAL
    assert b"zm_mpc_setup_ltv_f64" in lib.zm_last_error()
    assert lib.zm_mpc_setup_ltv_f64(d, d, None, d, d, d, d, 4, 7, 10, 13, 4, d, d, d, d, None) == _lib.ZM_EUNSUPPORTED
    assert lib.zm_mpc_setup_ltv_f64(None, None, None, None, None, None, None, 0, 7, 10, 12, 4, None, None, None, None, None) == _lib.ZM_OK
    solve = lambda N, n, m, D=d, alpha=1.6: lib.zm_mpc_solve_ltv_f64(d, d, d, d, d, d, d, d, d, D, 7, 3, 5.0, alpha, d, d, d, d, d, None, None, d, d,
                                                                      1, 1e-5, 1e-5, 1e-4, 100, 0, d, d, d, d, d, d, 8, N, n, m, None)
    assert solve(10, 12, 4, D=None) == _lib.ZM_EINVAL and b"zm_mpc_solve_ltv_f64" in lib.zm_last_error()
    assert solve(10, 12, 4, alpha=2.5) == _lib.ZM_EINVAL
    assert solve(76, 12, 4) == _lib.ZM_EUNSUPPORTED and b"N <= 75" in lib.zm_last_error()
    assert solve(10, 24, 8) == _lib.ZM_EUNSUPPORTED and b"16-lanes" in lib.zm_last_error()
    assert solve(10, 5, 3) == _lib.ZM_EUNSUPPORTED
