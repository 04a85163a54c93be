"""CPU checks for mpcUtils.ltvMpc with stage_varying= (per-stage weights and boxes): the NumPy restatement of the kernels
(tests/mpc_ltv_stage_ref.py: admm_levels_ltv_stage) against the restatement it extends and against an independent SciPy solve, the
decisiveness and the non-vacuity of every input of tests/test_mpc_ltv_stage_gpu.py, the gate, and the host-side checks of the constructor,
of realTimeIteration and of the two C entry points.  No GPU."""
import numpy as np
import pytest

from oracle import mpc_oracle as mo
from tests import mpc_ltv_ref as lr
from tests import mpc_ltv_stage_ref as sr
from tests import mpc_tracking_ref as tr
from tests.test_mpc_ltv import _same
from zopt_amd import mpcUtils


@pytest.mark.parametrize("n,m,N", [(4, 2, 4), (12, 4, 7), (2, 1, 5)])
def test_constant_rows_are_the_restatement_it_extends(n, m, N):
    """constant rows: admm_levels_ltv_stage is admm_levels_ltv on the recipe's stage-varying dynamics with offsets -- status, iterations,
    level moves, and x, u, y, lam to 1e-12; cold (loose), then a warm and a shifted solve each fed its own previous state.  Instance 1
    runs with a reference (the linear term by stage is the linear term).  (Both are adapters of oracle.mpc_oracle.admm_levels_stage now:
    this holds `stage_form` and `linear_term_stage` to the one set of weights and bounds.)"""
    (A, B, c, Q, R, Qf, xl, xu, ul, uu), x0 = lr.recipe(n, m, N, 2)
    st = sr.stage_form(Q, R, Qf, N, xl, xu, ul, uu)
    old = lambda x, **kw: lr.admm_levels_ltv(A, B, c, Q, R, Qf, N, xl, xu, ul, uu, x, **kw)
    new = lambda x, **kw: sr.admm_levels_ltv_stage(A, B, c, *st[:2], N, *st[2:], x, **kw)
    kw = dict(rho=tr.default_rho(Q, R), eps_abs=1e-6, eps_rel=1e-6, max_iter=30000)
    kw0 = dict(kw, eps_abs=1e-3, eps_rel=1e-3)
    r0, g0 = old(x0[0], **kw0), new(x0[0], **kw0)
    _same(g0, r0)
    r1, g1 = old(x0[0], warm=(r0.y, r0.lam, r0.level), **kw), new(x0[0], warm=(g0.y, g0.lam, g0.level), **kw)
    assert r1.status == "optimal"
    _same(g1, r1)
    r2 = old(r1.x[1], warm=(r1.y, r1.lam, r1.level), shift=True, **kw)
    g2 = new(g1.x[1], warm=(g1.y, g1.lam, g1.level), shift=True, **kw)
    _same(g2, r2)
    _, _, xRef, uRef = tr.random_case(n, m, N, seed=41, nb=1)
    g_old, g_new = tr.linear_term(Q, R, Qf, N, xRef[0], uRef[0]), sr.linear_term_stage(*st[:2], N, xRef[0], uRef[0])
    assert all(np.array_equal(a, b) for a, b in zip(g_old, g_new))
    _same(new(x0[1], g=g_new, **kw), old(x0[1], g=g_old, **kw))


def test_x0_is_tested_against_row_0_alone():
    (A, B, c, Q, R, Qf, xl, xu, ul, uu), x0 = lr.recipe(2, 1, 3, 1)
    Qs, Rs, xl, xu, ul, uu = sr.stage_form(Q, R, Qf, 3, xl, xu, ul, uu)
    xl[0], xu[0] = x0[0] + 0.1, x0[0] + 0.2                                 # outside row 0, inside every later row
    r = sr.admm_levels_ltv_stage(A, B, c, Qs, Rs, 3, xl, xu, ul, uu, x0[0])
    assert r.status == "infeasible" and r.iters == 0
    xl[0], xu[0] = x0[0] - 0.1, x0[0] + 0.1
    xl[1:], xu[1:] = -np.inf, np.inf
    assert sr.admm_levels_ltv_stage(A, B, c, Qs, Rs, 3, xl, xu, ul, uu, x0[0]).status == "optimal"


@pytest.mark.parametrize("name", [n for n in sr.ALL if sr.build(n).kind])
def test_stage_varying_solutions_agree_with_an_independent_solve(name):
    """the restatement's solution of the stage-varying cases is the QP's (condensed SciPy solve with per-stage weights and bounds), to the
    2e-3 in u of tests/test_mpc_ltv.py::test_solutions_agree_with_an_independent_solve"""
    for b in sr.scipy_instances(name):
        r = sr.reference(name)[0][b]
        assert r.status == "optimal"
        dev = np.max(np.abs(r.u - sr.scipy_solution(name, b)[1]))
        print(f"{name} instance {b}: {r.iters} iterations, deviation of u from SciPy {dev:.2e}")
        assert dev <= 2e-3


@pytest.mark.parametrize("name", sr.ALL)
def test_gpu_cases_are_decisive(name):
    """every input of tests/test_mpc_ltv_stage_gpu.py stays clear of every rounding-sensitive decision, by the margins of
    tests/test_mpc_ltv.py: no level decision within 1e-4 of a half-integer, no termination test within 1e-6 of its threshold, none at
    the cap within 1e-6 of the 10x test"""
    c = sr.build(name)
    assert c.N in sr.HORIZONS and len(c.x0) in sr.BATCHES + (2,)   # (2: the gate and its opened twin)
    cap = [step["kw"]["max_iter"] for step in c.steps]
    statuses = []
    for s, row in enumerate(sr.reference(name)):
        for b, r in enumerate(row):
            statuses.append(r.status)
            at = (name, s, b, r.status, r.iters)
            assert r.level_margin >= 1e-4 and r.stop_margin >= 1e-6, (at, r.level_margin, r.stop_margin)
            if r.iters == cap[s]:
                assert r.near_margin >= 1e-6, (at, r.near_margin)
    if name == "gate":
        assert statuses == ["infeasible", "optimal"]
    elif name == "x0_outside_row0":
        assert statuses == ["optimal"] * 3 + ["infeasible"] + ["optimal"]
    else:
        assert set(statuses) == {"optimal"}, statuses


ACTIVE = 1e-5   # a bound is active where the solution (solved to 1e-6 relative to iterates of size ~1) sits within this of it


@pytest.mark.parametrize("name", [n for n in sr.ALL if sr.build(n).kind in ("box", "both")])
def test_box_cases_need_their_stage_boxes(name):
    """the reference solution has an active bound at a stage where that bound differs from its envelope over the stages, and its u
    differs by more than 1e-4 from the solution with every bound replaced by that envelope"""
    c, r = sr.build(name), sr.reference(name)[0][0]
    _, _, _, _, _, xl, xu, ul, uu = c.inst[0]
    exl, exu, eul, euu = sr.envelope(xl, xu, ul, uu)
    near = [np.where((bd != env) & np.isfinite(bd), np.abs(v - bd), np.inf).min()
            for v, bd, env in ((r.x[1:], xl[1:], exl[1:]), (r.x[1:], xu[1:], exu[1:]), (r.u, ul, eul), (r.u, uu, euu))]
    dev = np.max(np.abs(r.u - sr.variant_solution(name, "envelope")[1]))
    print(f"{name}: nearest stage-specific bound {min(near):.2e}, u moves by {dev:.2e} when the boxes become their envelope")
    assert min(near) <= ACTIVE and dev > 1e-4


@pytest.mark.parametrize("name", [n for n in sr.ALL if sr.build(n).kind in ("weight", "both")])
def test_weight_cases_need_their_stage_weights(name):
    """u differs by more than 1e-4 from the solution with stage-mean weights"""
    dev = np.max(np.abs(sr.reference(name)[0][0].u - sr.variant_solution(name, "mean")[1]))
    print(f"{name}: u moves by {dev:.2e} when the weights become their mean over the stages")
    assert dev > 1e-4
    if name == "waypoint_weights":
        assert sum(1 for Qk in sr.build(name).inst[0][3] if not Qk.any()) >= 4    # Q_k = 0 at most stages


def test_a_gate_the_dynamics_cannot_reach_is_infeasible():
    """x+ = x + u with |u| <= 0.1 from 0: x_2[0] <= 0.2, so the gate 0.5 <= x_2[0] <= 0.6 cannot be reached and the certificate says so
    at a check; opened to -1 <= x_2[0] <= 0.6 the same data is solved"""
    for closed, want in ((True, "infeasible"), (False, "optimal")):
        d, x0 = sr.gate_data(closed)
        r = sr.admm_levels_ltv_stage(*d[:5], 3, *d[5:], x0, rho=2.0)
        assert r.status == want, (closed, r.status, r.iters)
        if closed:
            assert r.iters % mo.CHECK_EVERY == 0 and 0 < r.iters <= 64, r.iters


# ---- host-side checks of the constructor -------------------------------------------------------------------------------------------------

def _ctor(n=2, m=1, N=3, P=(), sv=sr.ALL_SIX):
    """constant rows, every name in `sv` with its stage axis"""
    rows = lambda X, r, name: np.broadcast_to(X, (r,) + X.shape).copy() if name in sv else X
    A = np.broadcast_to(0.5 * np.eye(n), P + (N, n, n)).copy()
    return dict(A=A, B=np.ones(P + (N, n, m)), Q=rows(np.eye(n), N + 1, "Q"), R=rows(2.0 * np.eye(m), N, "R"), N=N,
                x_lb=rows(-np.ones(n), N + 1, "x_lb"), x_ub=rows(np.ones(n), N + 1, "x_ub"), u_lb=rows(-np.ones(m), N, "u_lb"),
                u_ub=rows(np.ones(m), N, "u_ub"), stage_varying=sv)


def test_constructor_takes_stage_axes_and_refuses_bad_ones():
    prob = mpcUtils.ltvMpc(**_ctor())
    assert prob.stage_varying == frozenset(sr.ALL_SIX) and isinstance(prob.stage_varying, frozenset) and prob.P == ()
    assert prob.Q.shape == (4, 2, 2) and prob.R.shape == (3, 1, 1) and prob.x_lb.shape == prob.x_ub.shape == (4, 2)
    assert prob.u_lb.shape == prob.u_ub.shape == (3, 1)
    some = mpcUtils.ltvMpc(**_ctor(P=(4,), sv=("x_ub", "R")))
    assert some.P == (4,) and some.Q.shape == (4, 2, 2) and some.x_ub.shape == (4, 4, 2) and some.x_lb.shape == (4, 2)
    assert some.R.shape == (4, 3, 1, 1) and some.stage_varying == {"x_ub", "R"}
    plain = mpcUtils.ltvMpc(**{k: v for k, v in _ctor(sv=()).items() if k != "stage_varying"})
    assert plain.stage_varying == frozenset() and plain.Q.shape == (2, 2)
    with pytest.raises(ValueError, match=r"Qf must be None"):
        mpcUtils.ltvMpc(**_ctor(), Qf=np.eye(2))
    mpcUtils.ltvMpc(**_ctor(sv=("R",)), Qf=3.0 * np.eye(2))
    with pytest.raises(ValueError, match=r"stage_varying names \['Qf'\]"):
        mpcUtils.ltvMpc(**_ctor(sv=("Q", "Qf")))
    with pytest.raises(ValueError, match=r"Q of shape \(3, 2, 2\) has 3 stages, expected N = 3 \+ 1"):
        mpcUtils.ltvMpc(**dict(_ctor(), Q=np.tile(np.eye(2), (3, 1, 1))))
    with pytest.raises(ValueError, match=r"u_lb of shape \(4, 1\) has 4 stages, expected N = 3"):
        mpcUtils.ltvMpc(**dict(_ctor(), u_lb=-np.ones((4, 1))))
    with pytest.raises(ValueError, match="shapes"):
        mpcUtils.ltvMpc(**dict(_ctor(), x_ub=np.ones(2)))
    Q = np.tile(np.eye(2), (4, 1, 1))
    Q[2] = np.diag([1.0, -0.1])
    with pytest.raises(ValueError, match=r"Q at stage 2 is not positive semidefinite"):
        mpcUtils.ltvMpc(**dict(_ctor(), Q=Q))
    with pytest.raises(ValueError, match=r"Q\[1\] at stage 2 is not positive semidefinite"):
        mpcUtils.ltvMpc(**dict(_ctor(P=(3,)), Q=np.stack([np.tile(np.eye(2), (4, 1, 1)), Q, Q])))
    Q[2], Q[0] = np.eye(2), np.diag([1.0, -0.1])                            # (row 0 is unused, and checked all the same)
    with pytest.raises(ValueError, match=r"Q at stage 0 is not positive semidefinite"):
        mpcUtils.ltvMpc(**dict(_ctor(), Q=Q))
    with pytest.raises(ValueError, match=r"update: x_lb has shape"):
        prob.update(x_lb=-np.ones(2))
    with pytest.raises(ValueError, match=r"stage_varying="):
        plain.update(x_lb=-np.ones(2))
    with pytest.raises(NotImplementedError):
        prob.simulate(np.zeros(2), 5)


def test_embedding_pads_every_stage():
    """(3, 2) runs in the (4, 2) kernels: at every stage the extra weight is 1 and the extra state has no bound"""
    prob = mpcUtils.ltvMpc(**_ctor(n=3, m=2, N=4, P=(2,)))
    assert (prob.n, prob.m, prob._n_user, prob._m_user) == (4, 2, 3, 2)
    assert prob.Q.shape == (2, 5, 4, 4) and np.all(prob.Q[..., 3, 3] == 1.0) and not prob.Q[..., 3, :3].any() and not prob.Q[..., :3, 3].any()
    assert np.array_equal(prob.Q[..., :3, :3], np.broadcast_to(np.eye(3), (2, 5, 3, 3)))
    assert prob.R.shape == (2, 4, 2, 2) and prob.x_lb.shape == (2, 5, 4)
    assert np.all(prob.x_lb[..., 3] == -np.inf) and np.all(prob.x_ub[..., 3] == np.inf) and np.all(prob.x_ub[..., :3] == 1.0)
    wide = mpcUtils.ltvMpc(**_ctor(n=10, m=3, N=2))
    assert (wide.n, wide.m) == (12, 4) and np.all(wide.R[..., 3, 3] == 1.0) and np.all(wide.u_ub[..., 3] == np.inf)
    assert np.all(wide.u_lb[..., 3] == -np.inf) and wide.u_lb.shape == (2, 4)


def test_the_stage_form_packs_the_boxes_in_the_stacked_layout():
    """Qs[k] weights x_{k+1} (row N - 1 terminal), lo / hi row k = [x_lb[k+1] ; u_lb[k]], and row 0 of the state box apart"""
    rng = np.random.default_rng(4)
    n, m, N = 3, 2, 4
    d = _ctor(n=n, m=m, N=N, P=(2,))
    d["x_lb"], d["u_lb"] = -1.0 - rng.uniform(0, 1, (2, N + 1, n)), -1.0 - rng.uniform(0, 1, (N, m))
    d["x_ub"], d["u_ub"] = 1.0 + rng.uniform(0, 1, (N + 1, n)), 1.0 + rng.uniform(0, 1, (2, N, m))
    d["Q"] = np.stack([(k + 1.0) * np.eye(n) for k in range(N + 1)])
    d["x_ub"][2, 1] = np.inf
    f = mpcUtils.ltvMpc(**d)._stage_form()
    assert f["Qs"].shape == (2, N, 4, 4) and f["Rs"].shape == (2, N, 2, 2) and f["lo"].shape == f["hi"].shape == (2, N, 6)
    assert f["x_lb0"].shape == f["x_ub0"].shape == (2, 4)
    for k in range(N):
        assert np.array_equal(f["Qs"][:, k, :n, :n], np.broadcast_to((k + 2.0) * np.eye(n), (2, n, n)))
        assert np.array_equal(f["lo"][:, k, :n], d["x_lb"][:, k + 1]) and np.all(f["lo"][:, k, n] == -np.inf)
        assert np.array_equal(f["lo"][:, k, 4:], np.broadcast_to(d["u_lb"][k], (2, m)))
        assert np.array_equal(f["hi"][:, k, :n], np.broadcast_to(d["x_ub"][k + 1], (2, n))) and np.all(f["hi"][:, k, n] == np.inf)
        assert np.array_equal(f["hi"][:, k, 4:], d["u_ub"][:, k])
    assert np.array_equal(f["x_lb0"][:, :n], d["x_lb"][:, 0]) and np.array_equal(f["x_ub0"][:, :n], np.broadcast_to(d["x_ub"][0], (2, n)))
    # without a stage axis on Q the terminal row is Qf, the others Q
    g = mpcUtils.ltvMpc(**_ctor(n=n, m=m, N=N, sv=("x_lb",)), Qf=3.0 * np.eye(n))._stage_form()
    assert np.all(g["Qs"][:N - 1, 0, 0] == 1.0) and g["Qs"][N - 1, 0, 0] == 3.0 and np.all(g["Rs"][:, 0, 0] == 2.0)


def test_default_penalty_is_the_median_over_the_stages():
    """_penalty(Q_{k+1}, R_k) per stage, then the median: on constant rows exactly the value today's constructor gives, per problem"""
    rng = np.random.default_rng(8)
    n, m, N, P = 4, 2, 6, (3,)
    Mq, Mr = rng.standard_normal(P + (n, n)), rng.standard_normal(P + (m, m))
    Q, R = Mq @ np.swapaxes(Mq, -1, -2) + np.eye(n), Mr @ np.swapaxes(Mr, -1, -2) + np.eye(m)
    base = {k: v for k, v in _ctor(n=n, m=m, N=N, P=P, sv=()).items() if k != "stage_varying"}
    plain = mpcUtils.ltvMpc(**dict(base, Q=Q, R=R))
    staged = mpcUtils.ltvMpc(**dict(base, Q=np.repeat(Q[:, None], N + 1, axis=1), R=np.repeat(R[:, None], N, axis=1)), stage_varying=("Q", "R"))
    assert staged.rho.shape == P and np.array_equal(staged.rho, plain.rho) and np.array_equal(plain.rho, mpcUtils._penalty(Q, R, P))
    assert np.array_equal(mpcUtils.ltvMpc(**dict(base, Q=Q, R=np.repeat(R[:, None], N, axis=1)), stage_varying=("R",)).rho, plain.rho)
    # stage weights: the median of the per-stage values, Q's row 0 left out
    scale = np.array([100.0, 1.0, 2.0, 3.0, 4.0, 5.0, 50.0])
    Qk = scale[:, None, None] * Q[0]
    one = mpcUtils.ltvMpc(**dict({k: v for k, v in _ctor(n=n, m=m, N=N, sv=()).items() if k != "stage_varying"}, Q=Qk, R=R[0]),
                          stage_varying=("Q",))
    per = [mpcUtils._penalty(Qk[k + 1], R[0], ()) for k in range(N)]
    assert one.rho == np.median(per) and one.rho != mpcUtils._penalty(Qk[0], R[0], ())


def test_from_expansion_passes_stage_varying_through():
    from zopt_amd.pytrees import AffineDynamics, Trajectory
    rng = np.random.default_rng(2)
    N, n, m = 5, 4, 2
    f, f_x, f_u = rng.standard_normal((N, n)), rng.standard_normal((N, n, n)), rng.standard_normal((N, n, m))
    traj = Trajectory(rng.standard_normal((N + 1, n)), rng.standard_normal((N, m)))
    xu = np.tile(np.ones(n), (N + 1, 1))
    prob = mpcUtils.ltvMpc.fromExpansion(AffineDynamics(f, f_x, f_u), traj, np.eye(n), np.eye(m), -np.ones(n), xu, -np.ones(m), np.ones(m),
                                         stage_varying=("x_ub",))
    assert prob.stage_varying == {"x_ub"} and prob.x_ub.shape == (N + 1, n) and prob.N == N


def test_real_time_iteration_refuses_before_anything_touches_the_gpu():
    """the refusal comes first: not even the arguments are looked at"""
    prob = mpcUtils.ltvMpc(**_ctor())
    with pytest.raises(NotImplementedError, match=r"realTimeIteration.*relinearize.*update.*solve.*modelStep"):
        prob.realTimeIteration(None, None, 0)
    assert prob._dev is None


def test_c_abi_refuses_bad_arguments_without_a_gpu():
    from zopt_amd import _lib
    lib, d = _lib.lib(), 0x1000
    setup = lambda P=4, n=12, m=4, N=10, L=7, Qs=d, ABt=d: lib.zm_mpc_setup_ltv_stage_f64(d, d, None, Qs, d, d, P, L, N, n, m, d, d, d, ABt, None)
    assert setup(Qs=None) == _lib.ZM_EINVAL and b"zm_mpc_setup_ltv_stage_f64: null pointer" in lib.zm_last_error()
    assert setup(ABt=None) == _lib.ZM_EINVAL
    assert setup(N=0) == _lib.ZM_EINVAL and b"zm_mpc_setup_ltv_stage_f64: bad size" in lib.zm_last_error()
    assert setup(L=0) == _lib.ZM_EINVAL and setup(P=-1) == _lib.ZM_EINVAL
    assert setup(n=13) == _lib.ZM_EUNSUPPORTED and b"n <= 12, m <= 4" in lib.zm_last_error()
    assert setup(m=5) == _lib.ZM_EUNSUPPORTED
    assert lib.zm_mpc_setup_ltv_stage_f64(None, None, None, None, None, None, 0, 7, 10, 12, 4, None, None, None, None, None) == _lib.ZM_OK

    def solve(N=10, n=12, m=4, alpha=1.6, batch=8, P=1, n_levels=7, **null):
        p = lambda k: None if k in null else d
        return lib.zm_mpc_solve_ltv_stage_f64(d, d, p("c"), p("ABt"), p("Qs"), p("Rs"), d, d, p("D"), n_levels, 3, 5.0, alpha, p("x_lb0"),
                                              p("x_ub0"), p("lo"), p("hi"), d, None, None, p("rho_p"), p("problem"), P, 1e-5, 1e-5, 1e-4,
                                              100, 0, d, d, d, d, d, d, batch, N, n, m, None)
    for k in ("c", "ABt", "Qs", "Rs", "D", "x_lb0", "x_ub0", "lo", "hi", "rho_p", "problem"):
        assert solve(**{k: None}) == _lib.ZM_EINVAL, k
        assert b"zm_mpc_solve_ltv_stage_f64: null pointer" in lib.zm_last_error(), k
    assert solve(alpha=2.5) == _lib.ZM_EINVAL and b"alpha" in lib.zm_last_error()
    assert solve(N=0) == _lib.ZM_EINVAL and solve(batch=-1) == _lib.ZM_EINVAL and solve(P=0) == _lib.ZM_EINVAL
    assert solve(n_levels=0) == _lib.ZM_EINVAL and b"bad penalty levels" in lib.zm_last_error()
    assert solve(N=76) == _lib.ZM_EUNSUPPORTED and b"zm_mpc_solve_ltv_stage_f64: N=76" in lib.zm_last_error() and b"N <= 75" in lib.zm_last_error()
    assert solve(n=24, m=8) == _lib.ZM_EUNSUPPORTED and b"16-lanes" in lib.zm_last_error()
    assert solve(n=5, m=3) == _lib.ZM_EUNSUPPORTED
    assert solve(batch=0, Qs=None) == _lib.ZM_OK
