"""CPU checks for mpcUtils.ltvMpc with soft box constraints: the NumPy restatement of zm_mpc_solve_ltv_soft_f64
(tests/mpc_ltv_soft_ref.py: admm_levels_ltv_soft) against the restatement it extends, against known answers and against an independent
slack-variable SciPy solve; the decisiveness and the non-vacuity of every input of tests/test_mpc_ltv_soft_gpu.py; and the host-side
checks of the constructor, of update, of realTimeIteration and of the C entry point.  No GPU."""
import numpy as np
import pytest

from tests import mpc_ltv_ref as lr
from tests import mpc_ltv_soft_ref as so
from tests import mpc_ltv_stage_ref as sr
from tests import mpc_tracking_ref as tr
from zopt_amd import mpcUtils

INF = np.inf


def _equal(a, b):
    """== on everything a solve returns and stores"""
    assert a.status == b.status and a.iters == b.iters and a.moves == b.moves and a.level == b.level and a.locked == b.locked
    for k in ("x", "u", "y", "lam"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k


@pytest.mark.parametrize("n,m,N", [(4, 2, 4), (12, 4, 7), (2, 1, 5), (2, 2, 2), (4, 1, 3)])
def test_all_hard_weights_are_the_restatement_it_extends(n, m, N):
    """every l1 = +inf: admm_levels_ltv_soft returns exactly what admm_levels_ltv_stage returns -- x, u, y, lam, iterations, status with
    == -- cold (loose), then a warm and a shifted solve each fed its own previous state, and an instance with a reference.  (The guard is
    on in both: the recipe has offsets.)  Both are adapters of oracle.mpc_oracle.admm_levels_stage now: this holds l1 = None to l1 = +inf.
    (test_the_proximal_map_is_the_clip_on_a_hard_component_bit_for_bit holds its `prox` to the clip.)"""
    (A, B, c, Q, R, Qf, xl, xu, ul, uu), x0 = lr.recipe(n, m, N, 2)
    st = sr.stage_form(Q, R, Qf, N, xl, xu, ul, uu)
    hard = np.full(n + m, INF)
    old = lambda x, **kw: sr.admm_levels_ltv_stage(A, B, c, *st[:2], N, *st[2:], x, **kw)
    new = lambda x, **kw: so.admm_levels_ltv_soft(A, B, c, *st[:2], N, *st[2:], x, hard, **kw)
    kw = dict(rho=tr.default_rho(Q, R), eps_abs=1e-6, eps_rel=1e-6, max_iter=30000)
    kw0 = dict(kw, eps_abs=1e-3, eps_rel=1e-3)
    r0, g0 = old(x0[0], **kw0), new(x0[0], **kw0)
    _equal(g0, r0)
    r1, g1 = old(x0[0], warm=(r0.y, r0.lam, r0.level), **kw), new(x0[0], warm=(g0.y, g0.lam, g0.level), **kw)
    assert r1.status == "optimal"
    _equal(g1, r1)
    r2 = old(r1.x[1], warm=(r1.y, r1.lam, r1.level), shift=True, **kw)
    g2 = new(g1.x[1], warm=(g1.y, g1.lam, g1.level), shift=True, **kw)
    _equal(g2, r2)
    _, _, xRef, uRef = tr.random_case(n, m, N, seed=41, nb=1)
    g = sr.linear_term_stage(*st[:2], N, xRef[0], uRef[0])
    _equal(new(x0[1], g=g, **kw), old(x0[1], g=g, **kw))
    _equal(new(x0[1], n_levels=1, **kw), old(x0[1], n_levels=1, **kw))


def test_the_proximal_map_is_the_clip_on_a_hard_component_bit_for_bit():
    """t = +inf: e = -inf and y is the bound itself, the sign of a zero bound included; inside the box y = v"""
    v = np.array([-2.0, -0.0, 0.0, 0.5, 2.0, -3.0, 3.0])
    lo, hi = np.array([-1.0, -0.0, 0.0, 0.0, -0.0, -INF, -INF]), np.array([1.0, 1.0, 1.0, 1.0, -0.0, -0.0, INF])
    y = so.prox(v, lo, hi, INF, 1.0)
    want = np.clip(v, lo, hi)
    assert np.array_equal(y, want) and np.array_equal(np.signbit(y), np.signbit(want))
    assert np.signbit(so.prox(np.array([1.0]), np.array([-1.0]), np.array([-0.0]), INF, 1.0))[0]
    # a finite threshold: beyond it the excess is scaled, within it y is the bound
    assert so.prox(np.array([2.0]), -1.0, 1.0, 0.25, 0.5)[0] == 1.0 + 0.5 * 0.75
    assert so.prox(np.array([-1.2]), -1.0, 1.0, 0.25, 0.5)[0] == -1.0 and so.prox(np.array([-3.0]), -1.0, 1.0, 0.25, 1.0)[0] == -2.75


@pytest.mark.parametrize("weights,want", so.SCALAR)
def test_the_scalar_problem_has_its_known_answers(weights, want):
    """x+ = x + u, Q = R = 1, N = 1, x0 = 1, x_1 <= 0:  l1 = 1 -> 1/4;  l1 = 3 (above the multiplier 2) -> the hard 0;  l2 = 1 -> 1/3"""
    d, x0 = so.scalar_data()
    r = so.admm_levels_ltv_soft(*d[:5], 1, *d[5:], x0, np.array([weights[0], INF]), np.array([weights[1], 0.0]), **lr._kw())
    assert r.status == "optimal" and abs(r.x[1, 0] - want) <= 1e-5, (r.status, r.x[1, 0], want)
    xs, us, _ = so.solve_reference_ltv_soft(*d[:5], 1, *d[5:], x0, np.array([weights[0], INF]), np.array([weights[1], 0.0]))
    assert abs(xs[1, 0] - want) <= 1e-5                   # (the slack QP has them too)


@pytest.mark.parametrize("name", ["terminal_box", "moving_boxes"])
def test_an_l1_above_the_multipliers_gives_the_hard_solution(name):
    """the exact penalty: with l1 = 5 on every component (the issue's value, above every multiplier of these cases) u is the hard case's to
    1e-4"""
    c, hard = sr.build(name), sr.reference(name)[0][0]
    A, B, ck, Qs, Rs, xl, xu, ul, uu = c.inst[0]
    n, m = B.shape[-2:]
    rho = float(sr.case_rho(mpcUtils, c)[0])
    r = so.admm_levels_ltv_soft(A, B, ck, Qs, Rs, c.N, xl, xu, ul, uu, c.x0[0], np.full(n + m, 5.0), rho=rho, **lr._kw())
    dev = np.max(np.abs(r.u - hard.u))
    print(f"{name}: l1 = 5 everywhere, {r.iters} iterations, deviation of u from the hard solution {dev:.2e}")
    assert r.status == hard.status == "optimal" and dev <= 1e-4


def test_the_closed_gate_is_infeasible_when_hard_and_solved_when_soft():
    d, x0 = sr.gate_data(True)
    hard = so.admm_levels_ltv_soft(*d[:5], 3, *d[5:], x0, np.full(4, INF), rho=2.0, **lr._kw())
    assert hard.status == "infeasible"
    one = so.admm_levels_ltv_soft(*d[:5], 3, *d[5:], x0, np.array([2.0, INF, INF, INF]), rho=2.0, **lr._kw())
    both = so.admm_levels_ltv_soft(*d[:5], 3, *d[5:], x0, np.array([0.5, 0.5, INF, INF]), np.array([0.5, 0.5, 0.0, 0.0]), rho=2.0, **lr._kw())
    print(f"closed gate: hard {hard.iters} iterations; l1 = 2 on state 0: {one.iters}; l1 = l2 = 0.5 on both states: {both.iters}")
    assert one.status == "optimal" and both.status == "optimal"
    assert one.x[2, 0] < 0.5 - 1e-4                         # (the gate is paid for, not reached)


def test_x0_outside_row_0_is_solved_in_a_soft_component_and_refused_in_a_hard_one():
    (A, B, c, Q, R, Qf, xl, xu, ul, uu), x0 = lr.recipe(2, 1, 3, 1)
    Qs, Rs, xl, xu, ul, uu = sr.stage_form(Q, R, Qf, 3, xl, xu, ul, uu)
    xl[0, 0], xu[0, 0] = x0[0, 0] + 0.1, x0[0, 0] + 0.2          # state 0 of x0 is outside row 0
    solve = lambda l1: so.admm_levels_ltv_soft(A, B, c, Qs, Rs, 3, xl, xu, ul, uu, x0[0], np.array(l1))
    r = solve([1.0, INF, INF])
    assert r.status == "optimal" and r.iters > 0
    r = solve([INF, 1.0, INF])
    assert r.status == "infeasible" and r.iters == 0


@pytest.mark.parametrize("name", [n for n in so.CASES if so.build(n).inst[0][1].shape[-2] <= 4])
def test_soft_solutions_agree_with_the_slack_qp(name):
    """the restatement's solution is the QP's (one slack per soft stage component), to the suite's 2e-3 in u"""
    c = so.build(name)
    for b in so.scipy_instances(name):
        r = so.reference(name)[0][b]
        if r.status == "infeasible":                        # (the hard gate; the instance refused at x0)
            assert name in ("soft_gate", "soft_x0_outside")
            continue
        assert r.status == "optimal"
        dev = np.max(np.abs(r.u - so.scipy_solution(name, b)[1]))
        print(f"{name} instance {b}: {r.iters} iterations, deviation of u from the slack QP {dev:.2e}")
        assert dev <= 2e-3
    if name == "soft_gate":
        assert np.max(np.abs(so.reference(name)[0][1].u - so.scipy_solution(name, 1)[1])) <= 2e-3


@pytest.mark.parametrize("name", so.ALL)
def test_gpu_cases_are_decisive(name):
    """every input of tests/test_mpc_ltv_soft_gpu.py stays clear of every rounding-sensitive decision, by the suite's margins: no level
    decision within 1e-4 of a half-integer, no termination test within 1e-6 of its threshold, none at the cap within 1e-6 of the 10x
    test"""
    c = so.build(name)
    assert c.N in so.HORIZONS and len(c.x0) in so.BATCHES + (2,)   # (2: the gate and its soft twin)
    cap = [step["kw"]["max_iter"] for step in c.steps]
    statuses = []
    for s, row in enumerate(so.reference(name)):
        for b, r in enumerate(row):
            statuses.append(r.status)
            at = (name, s, b, r.status, r.iters)
            assert r.level_margin >= 1e-4 and r.stop_margin >= 1e-6, (at, r.level_margin, r.stop_margin)
            if r.iters == cap[s]:
                assert r.near_margin >= 1e-6, (at, r.near_margin)
    if name == "soft_gate":
        assert statuses == ["infeasible", "optimal"]
    elif name == "soft_x0_outside":
        assert statuses == ["optimal", "infeasible", "optimal", "optimal", "optimal"]
        assert so.reference(name)[0][1].iters == 0
    else:
        assert set(statuses) == {"optimal"}, statuses


def test_the_sequence_moves_the_penalty_and_warm_starts_from_the_moved_level():
    """soft_terminal_sequence: the cold solve moves the level, so the warm and the shifted solve begin with thresholds t, a formed from a
    penalty other than rho0; the fixed-penalty twin runs one level"""
    ref = so.reference("soft_terminal_sequence")
    assert sum(len(r.moves) for r in ref[0]) >= 1
    assert all(r.level != 3 for r in ref[0]) and all(r.iters > 0 for row in ref[1:] for r in row)
    assert all(r.level == 0 and not r.moves for r in so.reference("soft_terminal_fixed")[0])


@pytest.mark.parametrize("name", so.CASES)
def test_soft_cases_need_their_weights(name):
    """the witness instance's solution violates a bound of a soft component by more than 1e-4, differs by more than 1e-4 in u from the
    all-hard solution where there is one, and by more than 1e-4 in u from the solution with the soft components' bounds removed"""
    c = so.build(name)
    b = c.witness
    p = so.problem_of(c, b)
    r = so.reference(name)[0][b]
    soft = np.isfinite(c.soft[p][0])
    viol = np.max(so.violation(r.x, r.u, *c.inst[p][5:])[:, soft])
    hard, free = so.variant_solution(name, "hard", b), so.variant_solution(name, "free", b)
    dev_free = np.max(np.abs(r.u - free.u))
    dev_hard = np.max(np.abs(r.u - hard.u)) if hard.status == "optimal" else None
    print(f"{name} instance {b}: largest violation of a soft bound {viol:.2e}; u moves by "
          f"{'-- (' + hard.status + ')' if dev_hard is None else format(dev_hard, '.2e')} against all hard, by {dev_free:.2e} against no bounds")
    assert r.status == "optimal" and free.status == "optimal"
    assert viol > 1e-4 and dev_free > 1e-4 and (dev_hard is None or dev_hard > 1e-4)
    if name in ("soft_gate", "soft_x0_outside"):
        assert hard.status == "infeasible"


def test_the_cases_cover_what_the_issue_lists():
    shapes = {name: (so.build(name).inst[0][1].shape[-2:], so.build(name).N, len(so.build(name).x0)) for name in so.ALL}
    assert shapes["soft_gate"] == ((2, 2), 3, 2) and shapes["soft_x0_outside"] == ((2, 2), 2, 5)
    assert shapes["soft_terminal"] == ((2, 1), 5, 9) and shapes["soft_quadratic"] == ((4, 2), 7, 5)
    assert shapes["soft_mixed"] == ((8, 4), 4, 1) and shapes["soft_tracking"] == ((12, 4), 7, 5)
    assert shapes["soft_embedded"] == ((3, 2), 3, 9) and shapes["soft_per_problem"] == ((4, 1), 5, 5)
    l1, l2 = so.build("soft_quadratic").soft[0]
    assert np.all(l1[np.isfinite(l1)] == 0.0) and np.all(l2[np.isfinite(l1)] > 0.0)
    l1, l2 = so.build("soft_mixed").soft[0]
    d = so.build("soft_mixed").inst[0]
    assert np.any(np.isfinite(l1[:8])) and np.any(l2[:8] > 0) and np.any(np.isfinite(l1[8:])) and np.any(np.isinf(d[5][1:])) and np.any(np.isinf(d[8]))
    per = so.build("soft_per_problem").soft
    assert np.all(np.isinf(per[2][0])) and len({tuple(w[0]) + tuple(w[1]) for w in per}) == 5
    assert so.build("soft_tracking").xRef is not None and np.max(np.abs(so.build("soft_tracking").xRef)) > 0.6
    assert so.build("soft_terminal_fixed").steps[0]["kw"]["n_levels"] == 1 and len(so.build("soft_terminal_sequence").steps) == 3


# ---- host-side checks ------------------------------------------------------------------------------------------------------------------------

def _ctor(n=2, m=1, N=3, P=(), **more):
    A = np.broadcast_to(0.5 * np.eye(n), P + (N, n, n)).copy()
    return dict(dict(A=A, B=np.ones(P + (N, n, m)), Q=np.eye(n), R=2.0 * np.eye(m), N=N, x_lb=-np.ones(n), x_ub=np.ones(n), u_lb=-np.ones(m),
                     u_ub=np.ones(m)), **more)


def test_constructor_takes_the_weights_and_refuses_bad_ones():
    plain = mpcUtils.ltvMpc(**_ctor())
    assert plain._soft is None and not plain._stage_entry and not hasattr(plain, "soft_l1")
    prob = mpcUtils.ltvMpc(**_ctor(x_soft_l1=[1.0, INF]))
    assert prob._stage_entry and prob.stage_varying == frozenset() and prob.Q.shape == (2, 2)
    assert np.array_equal(prob.soft_l1, [1.0, INF, INF]) and np.array_equal(prob.soft_l2, [0.0, 0.0, 0.0])
    assert np.array_equal(prob.rho, plain.rho)
    f = prob._stage_form()                                  # (the stage form of one set of weights and bounds: constant rows)
    assert f["lo"].shape == (3, 3) and np.array_equal(f["lo"], -np.ones((3, 3))) and f["Qs"].shape == (3, 2, 2)
    per = mpcUtils.ltvMpc(**_ctor(P=(4,), x_soft_l1=np.array([0.0, 2.0]), x_soft_l2=np.arange(8.0).reshape(4, 2), u_soft_l1=[[3.0]] * 4))
    assert per.soft_l1.shape == per.soft_l2.shape == (4, 3) and np.array_equal(per.soft_l1[2], [0.0, 2.0, 3.0])
    assert np.array_equal(per.soft_l2[:, :2], np.arange(8.0).reshape(4, 2)) and not per.soft_l2[:, 2].any()
    staged = mpcUtils.ltvMpc(**_ctor(x_ub=np.ones((4, 2)), stage_varying=("x_ub",), u_soft_l1=[0.5], u_soft_l2=[0.1]))
    assert staged.stage_varying == {"x_ub"} and np.array_equal(staged.soft_l1, [INF, INF, 0.5])
    for bad, match in ((dict(x_soft_l1=[-1.0, 1.0]), "negative or NaN"), (dict(u_soft_l1=[np.nan]), "negative or NaN"),
                       (dict(x_soft_l2=[-0.5, 0.0], x_soft_l1=[1.0, 1.0]), "negative or NaN"),
                       (dict(x_soft_l1=[1.0, 1.0], x_soft_l2=[INF, 0.0]), "non-finite"),
                       (dict(x_soft_l2=[1.0, 0.0]), r"l2 > 0 on a component whose l1 is \+inf"),
                       (dict(x_soft_l1=[1.0, INF], x_soft_l2=[0.0, 1.0]), r"l2 > 0 on a component whose l1 is \+inf"),
                       (dict(x_soft_l1=[1.0]), r"x_soft_l1 has shape \(1,\), expected \(\.\.\., 2\)"),
                       (dict(u_soft_l1=[1.0, 1.0]), r"u_soft_l1 has shape \(2,\), expected \(\.\.\., 1\)"),
                       (dict(x_soft_l1=np.ones((3, 2))), r"broadcast to the problem shape \(\)"),
                       (dict(x_soft_l1=1.0), "x_soft_l1 has shape")):
        with pytest.raises(ValueError, match=match):
            mpcUtils.ltvMpc(**_ctor(**bad))


def test_embedding_pads_the_weights_hard():
    """(3, 2) runs in the (4, 2) kernels: the padded state carries l1 = +inf, l2 = 0"""
    prob = mpcUtils.ltvMpc(**_ctor(n=3, m=2, N=4, P=(2,), x_soft_l1=[0.5, 1.0, 2.0], x_soft_l2=[1.0, 2.0, 3.0], u_soft_l1=[0.1, 0.2],
                                   u_soft_l2=[4.0, 5.0]))
    assert (prob.n, prob.m, prob._n_user, prob._m_user) == (4, 2, 3, 2) and prob.soft_l1.shape == prob.soft_l2.shape == (2, 6)
    assert np.array_equal(prob.soft_l1[1], [0.5, 1.0, 2.0, INF, 0.1, 0.2]) and np.array_equal(prob.soft_l2[0], [1.0, 2.0, 3.0, 0.0, 4.0, 5.0])
    wide = mpcUtils.ltvMpc(**_ctor(n=10, m=3, N=2, x_soft_l1=np.ones(10), u_soft_l1=np.zeros(3), u_soft_l2=np.ones(3)))
    assert (wide.n, wide.m) == (12, 4) and np.all(wide.soft_l1[10:12] == INF) and wide.soft_l1[15] == INF
    assert not wide.soft_l2[10:12].any() and wide.soft_l2[15] == 0.0 and np.all(wide.soft_l2[12:15] == 1.0)


def test_update_takes_new_weights_on_a_soft_object_only():
    prob = mpcUtils.ltvMpc(**_ctor(x_soft_l1=[1.0, INF]))
    prob.update(x_soft_l1=[INF, 2.0], u_soft_l1=[0.0], u_soft_l2=[3.0])          # (host only: nothing is on the device yet)
    assert np.array_equal(prob.soft_l1, [INF, 2.0, 0.0]) and np.array_equal(prob.soft_l2, [0.0, 0.0, 3.0]) and prob._dev is None
    prob.update(x_soft_l1=[INF, INF], u_soft_l1=[INF], u_soft_l2=[0.0])           # (all hard is a soft object still)
    assert np.all(prob.soft_l1 == INF) and prob._soft is not None and prob._stage_entry
    with pytest.raises(ValueError, match="negative or NaN"):
        prob.update(x_soft_l1=[-1.0, 0.0])
    with pytest.raises(ValueError, match=r"l2 > 0 on a component whose l1 is \+inf"):
        prob.update(x_soft_l2=[1.0, 0.0])                                         # (checked with the l1 that stays)
    with pytest.raises(ValueError, match=r"update: x_soft_l1 has shape"):
        prob.update(x_soft_l1=[1.0])
    assert np.all(prob.soft_l1 == INF) and not prob.soft_l2.any()                 # (a refused update changes nothing)
    plain = mpcUtils.ltvMpc(**_ctor())
    with pytest.raises(ValueError, match=r"update: new x_soft_l1 need an object built with soft weights"):
        plain.update(x_soft_l1=[1.0, 1.0])
    with pytest.raises(ValueError, match=r"stage_varying="):
        prob.update(x_lb=-np.ones(2))                                             # (bounds still need their stage axis named)


def test_from_expansion_passes_the_weights_through():
    from zopt_amd.pytrees import AffineDynamics, Trajectory
    rng = np.random.default_rng(2)
    N, n, m = 5, 4, 2
    f, f_x, f_u = rng.standard_normal((N, n)), rng.standard_normal((N, n, n)), rng.standard_normal((N, n, m))
    traj = Trajectory(rng.standard_normal((N + 1, n)), rng.standard_normal((N, m)))
    prob = mpcUtils.ltvMpc.fromExpansion(AffineDynamics(f, f_x, f_u), traj, np.eye(n), np.eye(m), -np.ones(n), np.ones(n), -np.ones(m),
                                         np.ones(m), x_soft_l1=[1.0, INF, INF, 0.0], x_soft_l2=[0.0, 0.0, 0.0, 2.0])
    assert np.array_equal(prob.soft_l1, [1.0, INF, INF, 0.0, INF, INF]) and prob.soft_l2[3] == 2.0 and prob.N == N


def test_real_time_iteration_refuses_a_soft_object_before_anything_touches_the_gpu():
    prob = mpcUtils.ltvMpc(**_ctor(x_soft_l1=[1.0, INF]))
    with pytest.raises(NotImplementedError, match=r"realTimeIteration.*soft.*relinearize.*solve.*modelStep"):
        prob.realTimeIteration(None, None, 0)
    assert prob._dev is None


def test_c_abi_refuses_bad_arguments_without_a_gpu():
    from zopt_amd import _lib
    lib, d = _lib.lib(), 0x1000

    def solve(N=10, n=12, m=4, alpha=1.6, batch=8, P=1, n_levels=7, **null):
        p = lambda k: None if k in null else d
        return lib.zm_mpc_solve_ltv_soft_f64(d, d, p("c"), p("ABt"), p("Qs"), p("Rs"), d, d, p("D"), n_levels, 3, 5.0, alpha, p("x_lb0"),
                                             p("x_ub0"), p("lo"), p("hi"), p("soft_l1"), p("soft_l2"), d, None, None, p("rho_p"),
                                             p("problem"), P, 1e-5, 1e-5, 1e-4, 100, 0, d, d, d, d, d, d, batch, N, n, m, None)
    for k in ("c", "ABt", "Qs", "Rs", "D", "x_lb0", "x_ub0", "lo", "hi", "soft_l1", "rho_p", "problem"):
        assert solve(**{k: None}) == _lib.ZM_EINVAL, k
        assert b"zm_mpc_solve_ltv_soft_f64: null pointer" in lib.zm_last_error(), k
    assert solve(alpha=2.5) == _lib.ZM_EINVAL and b"alpha" in lib.zm_last_error()
    assert solve(N=0) == _lib.ZM_EINVAL and solve(batch=-1) == _lib.ZM_EINVAL and solve(P=0) == _lib.ZM_EINVAL
    assert solve(n_levels=0) == _lib.ZM_EINVAL and b"bad penalty levels" in lib.zm_last_error()
    assert solve(N=76) == _lib.ZM_EUNSUPPORTED and b"zm_mpc_solve_ltv_soft_f64: N=76" in lib.zm_last_error() and b"N <= 75" in lib.zm_last_error()
    assert solve(n=24, m=8) == _lib.ZM_EUNSUPPORTED and b"16-lanes" in lib.zm_last_error()
    assert solve(n=5, m=3) == _lib.ZM_EUNSUPPORTED
    assert solve(soft_l2=None, N=76) == _lib.ZM_EUNSUPPORTED          # (a NULL soft_l2 is zeros: the call gets as far as the shape check)
    assert solve(batch=0, soft_l1=None) == _lib.ZM_OK
