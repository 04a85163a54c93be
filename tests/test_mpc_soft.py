"""CPU checks for mpcUtils.lqrMpc with soft box constraints (`lqrMpc.soften`; zm_mpc_solve_soft_f64, zm_mpc_closed_loop_soft_f64): the host
side of `soften` (checks, merging, embedding, per-problem broadcasting, the refusals before the device), the C entries' refusals, and -- for
every input of tests/test_mpc_soft_gpu.py -- that its restatement (tests/mpc_soft_ref.py over oracle.mpc_oracle.admm_levels_stage) stays
clear of every rounding-sensitive decision, needs its weights, and agrees with the slack QP where that is small.  No GPU."""
import numpy as np
import pytest

from oracle import mpc_oracle as mo
from tests import mpc_soft_ref as sf
from tests import mpc_tracking_ref as tr
from tests.mpc_iterates_cases import _random
from tests.mpc_ltv_soft_ref import SCALAR, _weights
from zopt_amd import mpcUtils

INF = np.inf


def _ctor(n=2, m=1, N=3, P=(), **more):
    A = np.broadcast_to(0.5 * np.eye(n), P + (n, n)).copy()
    return dict(dict(A=A, B=np.ones(P + (n, m)), Q=np.eye(n), R=2.0 * np.eye(m), N=N, x_lb=-np.ones(n), x_ub=np.ones(n), u_lb=-np.ones(m),
                     u_ub=np.ones(m)), **more)


# ---- soften: the host side -------------------------------------------------------------------------------------------------------------

def test_soften_takes_the_weights_returns_self_and_merges_repeated_calls():
    plain = mpcUtils.lqrMpc(**_ctor())
    assert plain._soft is None and not hasattr(plain, "soft_l1")
    prob = mpcUtils.lqrMpc(**_ctor())
    tables = prob._tables
    assert prob.soften(x_soft_l1=[1.0, INF]) is prob
    assert np.array_equal(prob.soft_l1, [1.0, INF, INF]) and np.array_equal(prob.soft_l2, [0.0, 0.0, 0.0])
    assert prob.rho == plain.rho and prob._dev is None and prob._tables is tables          # (nothing touched a device, the tables stay)
    prob.soften(u_soft_l1=[0.0], u_soft_l2=[3.0])                                          # (a second call replaces only what it names)
    assert np.array_equal(prob.soft_l1, [1.0, INF, 0.0]) and np.array_equal(prob.soft_l2, [0.0, 0.0, 3.0])
    prob.soften(x_soft_l1=[2.0, 0.5], x_soft_l2=[0.0, 1.0])
    assert np.array_equal(prob.soft_l1, [2.0, 0.5, 0.0]) and np.array_equal(prob.soft_l2, [0.0, 1.0, 3.0]) and prob._tables is tables
    prob.soften(x_soft_l1=[INF, INF], x_soft_l2=[0.0, 0.0], u_soft_l1=[INF], u_soft_l2=[0.0])    # (all hard is a softened object still)
    assert np.all(prob.soft_l1 == INF) and prob._soft is not None
    assert mpcUtils.lqrMpc(**_ctor()).soften()._soft is not None and np.all(mpcUtils.lqrMpc(**_ctor()).soften().soft_l1 == INF)


def test_soften_refuses_bad_weights_with_ltvmpc_s_messages_and_changes_nothing():
    prob = mpcUtils.lqrMpc(**_ctor()).soften(x_soft_l1=[1.0, INF])
    for bad, match in ((dict(x_soft_l1=[-1.0, 1.0]), "negative or NaN"), (dict(u_soft_l1=[np.nan]), "negative or NaN"),
                       (dict(x_soft_l2=[-0.5, 0.0]), "negative or NaN"),
                       (dict(x_soft_l1=[1.0, 1.0], x_soft_l2=[INF, 0.0]), "non-finite"),
                       (dict(x_soft_l2=[0.0, 1.0]), r"l2 > 0 on a component whose l1 is \+inf"),       # (checked with the l1 that stays)
                       (dict(x_soft_l1=[1.0]), r"lqrMpc\.soften: x_soft_l1 has shape \(1,\), expected \(\.\.\., 2\)"),
                       (dict(u_soft_l1=[1.0, 1.0]), r"u_soft_l1 has shape \(2,\), expected \(\.\.\., 1\)"),
                       (dict(x_soft_l1=np.ones((3, 2))), r"broadcast to the problem shape \(\)"),     # (no per-problem data: (n,) only)
                       (dict(x_soft_l1=1.0), "x_soft_l1 has shape")):
        with pytest.raises(ValueError, match=match):
            prob.soften(**bad)
        assert np.array_equal(prob.soft_l1, [1.0, INF, INF]) and not prob.soft_l2.any(), bad


def test_embedding_pads_the_weights_hard():
    """(3, 2) runs in the (4, 2) kernels, (10, 3) in (12, 4): the padded components carry l1 = +inf, l2 = 0"""
    prob = mpcUtils.lqrMpc(**_ctor(n=3, m=2, N=4)).soften(x_soft_l1=[0.5, 1.0, 2.0], x_soft_l2=[1.0, 2.0, 3.0], u_soft_l1=[0.1, 0.2],
                                                           u_soft_l2=[4.0, 5.0])
    assert (prob.n, prob.m, prob._n_user, prob._m_user) == (4, 2, 3, 2)
    assert np.array_equal(prob.soft_l1, [0.5, 1.0, 2.0, INF, 0.1, 0.2]) and np.array_equal(prob.soft_l2, [1.0, 2.0, 3.0, 0.0, 4.0, 5.0])
    wide = mpcUtils.lqrMpc(**_ctor(n=10, m=3, N=2)).soften(x_soft_l1=np.ones(10), u_soft_l1=np.zeros(3), u_soft_l2=np.ones(3))
    assert (wide.n, wide.m) == (12, 4) and np.all(wide.soft_l1[10:12] == INF) and wide.soft_l1[15] == INF
    assert not wide.soft_l2[10:12].any() and wide.soft_l2[15] == 0.0 and np.all(wide.soft_l2[12:15] == 1.0)


def test_per_problem_weights_broadcast_to_the_problem_shape():
    per = mpcUtils.lqrMpc(**_ctor(P=(4,))).soften(x_soft_l1=np.array([0.0, 2.0]), x_soft_l2=np.arange(8.0).reshape(4, 2),
                                                 u_soft_l1=[[3.0]] * 4)
    assert per.P == (4,) and per.soft_l1.shape == per.soft_l2.shape == (4, 3) and np.array_equal(per.soft_l1[2], [0.0, 2.0, 3.0])
    assert np.array_equal(per.soft_l2[:, :2], np.arange(8.0).reshape(4, 2)) and not per.soft_l2[:, 2].any()
    grid = mpcUtils.lqrMpc(**_ctor(P=(2, 3))).soften(x_soft_l1=np.ones((3, 2)))
    assert grid.soft_l1.shape == (2, 3, 3) and np.all(grid.soft_l1[..., :2] == 1.0) and np.all(grid.soft_l1[..., 2] == INF)
    with pytest.raises(ValueError, match=r"broadcast to the problem shape \(4,\)"):
        per.soften(x_soft_l1=np.ones((3, 2)))


def test_soften_refuses_what_the_16_lane_kernels_do_not_take_before_the_device():
    big = mpcUtils.lqrMpc(**_ctor(n=13, m=2, N=3))                 # (runs in the (24, 8) kernels)
    assert (big.n, big.m) == (24, 8)
    with pytest.raises(ValueError, match=r"lqrMpc\.soften: \(n=13, m=2\).*\(24, 8\).*16-lanes-per-instance"):
        big.soften(x_soft_l1=np.ones(13))
    long = mpcUtils.lqrMpc(**_ctor(N=76))
    with pytest.raises(ValueError, match=r"lqrMpc\.soften: N=76.*N <= 75"):
        long.soften(x_soft_l1=[1.0, 1.0])
    assert big._soft is None and long._soft is None and big._dev is None and long._dev is None
    assert mpcUtils.lqrMpc(**_ctor(N=75)).soften(x_soft_l1=[1.0, 1.0])._soft is not None


def test_ltvmpc_soften_raises_and_names_the_constructor_arguments_and_update():
    A = np.broadcast_to(0.5 * np.eye(2), (3, 2, 2)).copy()
    prob = mpcUtils.ltvMpc(A, np.ones((3, 2, 1)), np.eye(2), np.eye(1), 3, -np.ones(2), np.ones(2), -np.ones(1), np.ones(1))
    with pytest.raises(TypeError, match=r"ltvMpc\.soften.*constructor.*x_soft_l1.*update"):
        prob.soften(x_soft_l1=[1.0, 1.0])
    assert prob._soft is None


# ---- the C entries ------------------------------------------------------------------------------------------------------------------------

def test_c_abi_refuses_bad_arguments_without_a_gpu():
    """both entries on dummy pointers that are never followed: every call below is refused before a launch (or has batch 0)"""
    from zopt_amd import _lib
    lib, d = _lib.lib(), 0x1000
    assert len(_lib.SYMBOLS["zm_mpc_solve_soft_f64"][1]) == len(_lib.SYMBOLS["zm_mpc_solve_tracking_f64"][1]) + 2
    assert len(_lib.SYMBOLS["zm_mpc_closed_loop_soft_f64"][1]) == len(_lib.SYMBOLS["zm_mpc_closed_loop_f64"][1]) + 2

    def solve(N=10, n=12, m=4, alpha=1.6, batch=8, P=1, n_levels=7, rho=0.1, ref=None, **null):
        p = lambda k: None if k in null else d
        return lib.zm_mpc_solve_soft_f64(p("A"), p("B"), p("Q"), p("R"), p("Qf"), p("K"), p("Minv"), n_levels, 3, 5.0, alpha, p("x_lb"),
                                         p("x_ub"), p("u_lb"), p("u_ub"), p("soft_l1"), p("soft_l2"), p("x0"), ref, None, rho, None, None,
                                         P, 1e-5, 1e-5, 1e-4, 100, 0, p("ws"), p("xTraj"), p("uTraj"), p("status"), d, d, batch, N, n, m,
                                         None)

    def run(N=10, n=12, m=4, alpha=1.6, batch=8, steps=4, rho=0.1, ref=None, **null):
        p = lambda k: None if k in null else d
        return lib.zm_mpc_closed_loop_soft_f64(p("A"), p("B"), p("Q"), p("R"), p("Qf"), p("K"), p("Minv"), 7, 3, 5.0, alpha, p("x_lb"),
                                               p("x_ub"), p("u_lb"), p("u_ub"), p("soft_l1"), p("soft_l2"), p("x0"), ref, None,
                                               steps + N, steps + N - 1, rho, None, None, 1, 1e-5, 1e-5, 1e-4, 100, 2, steps, 1e-6, None,
                                               p("ws"), p("states"), p("inputs"), p("status"), p("iters"), None, None, batch, N, n, m, None)

    for call, name, ptrs in ((solve, b"zm_mpc_solve_soft_f64", ("A", "B", "K", "Minv", "x_lb", "x_ub", "u_lb", "u_ub", "soft_l1", "x0", "ws",
                                                                "xTraj", "uTraj", "status")),
                             (run, b"zm_mpc_closed_loop_soft_f64", ("A", "B", "K", "Minv", "x_lb", "x_ub", "u_lb", "u_ub", "soft_l1", "x0", "ws",
                                                                    "states", "inputs", "status", "iters"))):
        for k in ptrs:
            assert call(**{k: None}) == _lib.ZM_EINVAL, (name, k)
            assert name + b": null pointer" in lib.zm_last_error(), (name, k)
        # the weights are read for a reference only: without one a NULL Q passes the pointer check and the call gets as far as the shape
        # check; with one it is required.  (N = 76: every call of this test returns before a launch -- the pointers are never followed.)
        assert call(Q=None, N=76) == _lib.ZM_EUNSUPPORTED and name + b": N=76" in lib.zm_last_error()
        assert call(Q=None, ref=d, N=76) == _lib.ZM_EINVAL and name + b": null pointer" in lib.zm_last_error()
        assert call(alpha=2.5) == _lib.ZM_EINVAL and b"alpha" in lib.zm_last_error()
        assert call(N=0) == _lib.ZM_EINVAL and call(batch=-1) == _lib.ZM_EINVAL and call(rho=0.0) == _lib.ZM_EINVAL
        assert call(N=76) == _lib.ZM_EUNSUPPORTED and name + b": N=76" in lib.zm_last_error() and b"N <= 75" in lib.zm_last_error()
        assert call(n=24, m=8) == _lib.ZM_EUNSUPPORTED and b"16-lanes" in lib.zm_last_error()
        assert call(n=5, m=3) == _lib.ZM_EUNSUPPORTED
        assert call(soft_l2=None, N=76) == _lib.ZM_EUNSUPPORTED       # (a NULL soft_l2 is zeros: the call gets as far as the shape check)
        assert call(soft_l1=None, N=76) == _lib.ZM_EINVAL             # (the pointers come first)
        assert call(batch=0, soft_l1=None) == _lib.ZM_OK
    assert solve(n_levels=0) == _lib.ZM_EINVAL and b"bad penalty levels" in lib.zm_last_error()
    assert run(steps=0) == _lib.ZM_EINVAL and b"steps must be at least 1" in lib.zm_last_error()


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------

def _equal(a, b):
    """== on everything a solve returns and stores"""
    assert a.status == b.status and a.iters == b.iters and a.moves == b.moves and a.level == b.level and a.locked == b.locked
    for k in ("x", "u", "y", "lam"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k


@pytest.mark.parametrize("n,m,N", [(1, 1, 3), (2, 1, 5), (4, 2, 4), (12, 4, 7)])
def test_all_hard_weights_are_admm_levels_bit_for_bit(n, m, N):
    """the parity shapes of tests/test_mpc_soft_gpu.py: the restatement with every l1 = +inf returns exactly what admm_levels returns --
    cold (loose), warm, shifted, with a reference, at the fixed penalty"""
    data, x0 = _random(n, m, N, 1000 * n + 10 * m + N, 2)
    A, B, Q, R, Qf, xl, xu, ul, uu = data
    rho = tr.default_rho(Q, R)
    hard = _weights(n, m)
    old = lambda x, **kw: mo.admm_levels(A, B, Q, R, Qf, N, xl, xu, ul, uu, x, rho=rho, **kw)
    new = lambda x, **kw: sf.restate(data, *hard, x, rho, N=N, **kw)
    kw = dict(eps_abs=1e-6, eps_rel=1e-6, max_iter=30000)
    kw0 = dict(kw, eps_abs=1e-3, eps_rel=1e-3)
    r0, g0 = old(x0[0], **kw0), new(x0[0], **kw0)
    _equal(g0, r0)
    r1, g1 = old(x0[0], warm=(r0.y, r0.lam, r0.level), **kw), new(x0[0], warm=(g0.y, g0.lam, g0.level), **kw)
    assert r1.status == "optimal"
    _equal(g1, r1)
    _equal(new(g1.x[1], warm=(g1.y, g1.lam, g1.level), shift=True, **kw), old(r1.x[1], warm=(r1.y, r1.lam, r1.level), shift=True, **kw))
    _, _, xRef, uRef = tr.random_case(n, m, N, seed=41, nb=1)
    g = tr.linear_term(Q, R, Qf, N, xRef[0], uRef[0])
    _equal(new(x0[1], g=g, **kw), old(x0[1], g=g, **kw))
    _equal(new(x0[1], n_levels=1, **kw), old(x0[1], n_levels=1, **kw))


@pytest.mark.parametrize("b", range(3))
def test_the_scalar_case_has_its_known_answers(b):
    """x+ = x + u, Q = R = 1, N = 1, x0 = 1, x_1 <= 0:  l1 = 1 -> 1/4;  l1 = 3 (above the multiplier 2) -> the hard 0;  l2 = 1 -> 1/3"""
    r = sf.reference("scalar")[0][b]
    assert r.status == "optimal" and abs(r.x[1, 0] - SCALAR[b][1]) <= 1e-5, (r.status, r.x[1, 0], SCALAR[b])
    assert sf.hard_twin("scalar")[b].status == "infeasible"            # (x0 = 1 is outside x <= 0)


@pytest.mark.parametrize("name", sf.CASES)
def test_gpu_cases_are_decisive(name):
    """every (step, instance) of every case stays clear of every rounding-sensitive decision, by the suite's margins
    (tests/test_mpc_levels_oracle.py): no level decision within 1e-4 of a half-integer, no termination test within 1e-6 of its
    threshold, none at the cap within 1e-6 of the 10x test"""
    c = sf.build(name)
    for s, row in enumerate(sf.reference(name)):
        cap = c.steps[s]["kw"]["max_iter"]
        for b, r in enumerate(row):
            at = (name, s, b, r.status, r.iters)
            assert r.level_margin >= 1e-4 and r.stop_margin >= 1e-6, (at, r.level_margin, r.stop_margin)
            if r.iters == cap:
                assert r.near_margin >= 1e-6, (at, r.near_margin)


@pytest.mark.parametrize("name", sf.CASES)
def test_soft_cases_need_their_weights(name):
    """the witness instance is "optimal", violates a bound of a soft component by more than 1e-4, and its all-hard twin differs in status
    or by more than 1e-4 in u"""
    c = sf.build(name)
    b = c.witness
    r, hard = sf.reference(name)[0][b], sf.hard_twin(name)[b]
    n = c.inst[b][1].shape[0]
    A, B, Q, R, Qf, xl, xu, ul, uu = c.inst[b]
    soft = np.isfinite(c.soft[b][0])
    viol = np.max(mo.violation(r.x, r.u, *mo.stage_form(Q, R, Qf, c.N, xl, xu, ul, uu)[2:])[:, soft])
    viol = max(viol, np.max(np.maximum(0.0, np.maximum(r.x[0] - xu, xl - r.x[0]))[soft[:n]]))           # (or starts outside it)
    print(f"{name} instance {b}: {r.iters} iterations, largest violation of a soft bound {viol:.2e}; all hard: {hard.status}"
          + (f", u moves by {np.max(np.abs(r.u - hard.u)):.2e}" if hard.status == "optimal" else ""))
    assert r.status == "optimal" and viol > 1e-4
    assert hard.status != "optimal" or np.max(np.abs(r.u - hard.u)) > 1e-4


def test_the_cases_cover_what_they_claim():
    shape = lambda name: (sf.build(name).inst[0][1].shape, sf.build(name).N, len(sf.build(name).x0))
    assert shape("scalar") == ((1, 1), 1, 3) and shape("x0_outside") == ((2, 2), 2, 5) and shape("quadratic") == ((4, 2), 7, 5)
    assert shape("full_tile") == ((12, 4), 7, 5) and shape("embedded") == ((3, 2), 3, 9) and shape("per_problem") == ((4, 1), 5, 6)
    # x0_outside: state 0 soft, starts inside, on and outside; instance 3 outside in the hard state: refused at once, the others solved
    c, ref = sf.build("x0_outside"), sf.reference("x0_outside")[0]
    assert abs(c.x0[0, 0]) < 1.0 and c.x0[1, 0] == 1.0 and c.x0[2, 0] > 1.0 and c.x0[4, 0] < -1.0 and c.x0[3, 1] > c.inst[0][6][1]
    assert [r.status for r in ref] == ["optimal", "optimal", "optimal", "infeasible", "optimal"] and ref[3].iters == 0
    assert [r.status for r in sf.hard_twin("x0_outside")] == ["optimal", "optimal", "infeasible", "infeasible", "infeasible"]
    l1, l2 = sf.build("quadratic").soft[0]
    assert np.all(l1[np.isfinite(l1)] == 0.0) and np.all(l2[np.isfinite(l1)] > 0.0) and np.isfinite(l1[0]) and np.isfinite(l1[5])
    c = sf.build("full_tile")
    assert c.xRef is not None and np.max(np.abs(c.xRef)) > 2.9 and np.sum(np.isfinite(c.soft[0][0])) == 3
    l1, _ = sf.build("embedded").soft[0]
    assert np.isfinite(l1[1]) and np.isfinite(l1[3]) and np.sum(np.isfinite(l1)) == 2
    # per_problem: hard problems, soft ones with their own weights, a hard one whose certificate the soft neighbours leave alone
    c, ref = sf.build("per_problem"), sf.reference("per_problem")
    assert [bool(np.any(np.isfinite(w[0]))) for w in c.soft] == [False, True, False, True, True, False]
    assert len({tuple(w[0]) + tuple(w[1]) for w in c.soft}) == 4
    assert [r.status for r in ref[0]] == ["optimal", "optimal", "infeasible", "optimal", "optimal", "optimal"]
    twin = sf.hard_twin("per_problem")
    assert ref[0][2].iters == twin[2].iters > 0 and not ref[0][2].locked          # (a certificate, not the x0 test; no guard)
    for b in (0, 5):                                                               # (the all-hard problems are their twins exactly)
        _equal(ref[0][b], twin[b])
    assert c.steps[1]["kw"]["n_levels"] == 1 and all(not r.moves for r in ref[1])
    # sequence: a level move in the cold solve, a warm start from a moved level, a shifted start, one run at the fixed penalty
    c, ref = sf.build("sequence"), sf.reference("sequence")
    assert [s["warm"] for s in c.steps] == [False, True, "shift", False] and c.steps[3]["kw"]["n_levels"] == 1
    assert all(r.status == "optimal" for row in ref for r in row)
    assert sum(len(r.moves) for r in ref[0]) >= 1 and any(r.level != 3 for r in ref[0])
    assert all(r.iters > 0 for row in ref[1:] for r in row) and all(r.level == 0 and not r.moves for r in ref[3])


@pytest.mark.parametrize("name,b", [(name, b) for name, bs in sf.SCIPY.items() for b in bs])
def test_small_soft_cases_agree_with_the_slack_qp(name, b):
    """the restatement's solution is the QP's (one slack per soft stage component), to the 2e-3 in u of tests/test_mpc_ltv_soft.py"""
    r = sf.reference(name)[0][b]
    assert r.status == "optimal"
    dev = np.max(np.abs(r.u - sf.scipy_solution(name, b)[1]))
    print(f"{name} instance {b}: {r.iters} iterations, deviation of u from the slack QP {dev:.2e}")
    assert dev <= 2e-3


# ---- the closed loop ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,m,N", sf.LOOP_SHAPES)
def test_the_gust_puts_instances_outside_a_soft_bound_and_the_hard_twin_cannot_follow(n, m, N):
    """the inputs of the closed-loop tests, by the restated loop: every gusted instance is outside the soft bound after the gust step and
    back inside at the end, "optimal" at every step; its all-hard twin is "infeasible" at the step after the gust without the clip, and
    with the clip its recorded state is not the plant's"""
    data, soft, x0, w = sf.loop_case(n, m, N, 5)
    xu = data[6][0]
    run = sf.restated_loop(data, soft, x0, w, sf.STEPS, N)
    gusted = [b for b in range(5) if w[b, sf.GUST_STEP, 0] != 0.0]
    assert gusted == [0, 2, 4] and np.all(run.status == "optimal")
    hard_clip = sf.restated_loop(data, _weights(n, m), x0, w, sf.STEPS, N)
    hard_none = sf.restated_loop(data, _weights(n, m), x0, w, sf.STEPS, N, clip_tol=None)
    for b in gusted:
        plant = run.px[b, sf.GUST_STEP, 1] + w[b, sf.GUST_STEP]
        assert np.array_equal(run.xTraj[b, sf.GUST_STEP + 1], plant) and plant[0] > xu + 0.4            # (never moved: the plant's state)
        assert np.all(np.abs(run.xTraj[b, -1]) <= data[6])                                                # (and flown back)
        assert hard_none.status[b, sf.GUST_STEP + 1] == "infeasible"
        assert hard_clip.xTraj[b, sf.GUST_STEP + 1, 0] == xu - 1e-6 < hard_clip.px[b, sf.GUST_STEP, 1, 0] + w[b, sf.GUST_STEP, 0]
    for b in set(range(5)) - set(gusted):                                                                 # (the others never leave)
        assert np.all(np.abs(run.xTraj[b, :, 0]) < xu)
    print(f"({n}, {m}, {N}): state 0 of the gusted instances {np.round(run.xTraj[gusted][:, :, 0], 3).tolist()}")
