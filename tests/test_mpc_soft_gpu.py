"""GPU tests of mpcUtils.lqrMpc with soft box constraints (`lqrMpc.soften`): zm_mpc_solve_soft_f64 (mpc_solve_wave_soft_kernel) and
zm_mpc_closed_loop_soft_f64 (mpc_closed_loop_wave_soft_kernel; with references the queue of launches and mpc_advance_soft_kernel).
All-hard weights must reproduce the plain object bit for bit, in `solve` and in `simulate`; every soft case is held to the NumPy
restatement of the whole solve (tests/mpc_soft_ref.py over oracle.mpc_oracle.admm_levels_stage) by the rule of
tests/mpc_iterates_cases.py; `simulate` of a softened object is held, bit for bit, to the loop it documents written over `solve`.
tests/test_mpc_soft.py checks, without a GPU, that these inputs stay clear of every rounding-sensitive decision, that their weights
matter and that the gusts do what the closed-loop tests need."""
import numpy as np
import pytest

from tests import mpc_closed_loop_cases as cl
from tests import mpc_iterates_cases as ic
from tests import mpc_soft_ref as sf
from tests import mpc_tracking_ref as tr
from tests.mpc_ltv_soft_ref import SCALAR, _weights

pytestmark = pytest.mark.gpu

INF = np.inf


@pytest.fixture(scope="module")
def mpc():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from zopt_amd import mpcUtils
    return mpcUtils


def _solve(prob, x0, nb, N, **kw):
    u, traj, status = prob.solve(x0, **kw)
    y, lam, level, ok = ic.read_state(prob, nb, N)
    return dict(u=np.asarray(u), x=np.asarray(traj.xTraj), uT=np.asarray(traj.uTraj), status=np.asarray(status, dtype=str),
                iters=prob.last_iterations.copy(), resid=prob.last_residuals.copy(), y=y.copy(), lam=lam.copy(), level=level.copy(),
                ok=ok.copy())


def _identical(a, b, at):
    for k in a:
        assert np.array_equal(a[k], b[k]), (at, k)


def _hard(prob, n, m):
    return prob.soften(x_soft_l1=np.full(n, INF), u_soft_l1=np.full(m, INF))


# ---- all-hard weights: the plain object, bit for bit -----------------------------------------------------------------------------------

PARITY = [(1, 1, 3), (2, 1, 5), (4, 2, 4), (12, 4, 7)]


@pytest.mark.parametrize("n,m,N", PARITY)
def test_all_hard_weights_are_the_plain_solve_bit_for_bit(mpc, n, m, N):
    """batch 5 (an idle group; instance 3 starts outside its box): == on u, trajectory, status, iteration count, residuals and the stored
    warm-start state (y, lam, level, ok flag) -- cold, warm and "shift", with and without xRef"""
    data, x0 = ic._random(n, m, N, 1000 * n + 10 * m + N, 5, bad=3)
    plain, hard = cl.problem(mpc, data, N), _hard(cl.problem(mpc, data, N), n, m)
    assert hard._soft is not None and plain._soft is None
    _, _, xRef, _ = tr.random_case(n, m, N, seed=41, nb=5)
    seen = set()
    for refs in (False, True):
        kw = dict(max_iter=600, **(dict(xRef=xRef) if refs else {}))
        cold = [_solve(p, x0, 5, N, warm_start=False, eps_abs=1e-3, eps_rel=1e-3, **kw) for p in (plain, hard)]
        _identical(*cold, (n, m, N, refs, "cold"))
        warm = [_solve(p, x0, 5, N, warm_start=True, eps_abs=1e-6, eps_rel=1e-6, **kw) for p in (plain, hard)]
        _identical(*warm, (n, m, N, refs, "warm"))
        x1 = warm[0]["x"][..., 1, :]
        shift = [_solve(p, x1, 5, N, warm_start="shift", eps_abs=1e-6, eps_rel=1e-6, **kw) for p in (plain, hard)]
        _identical(*shift, (n, m, N, refs, "shift"))
        seen |= set(warm[0]["status"]) | set(shift[0]["status"])
        assert cold[0]["status"][3] == "infeasible" and cold[0]["iters"][3] == 0
    assert "optimal" in seen, seen


def test_all_hard_weights_are_the_per_problem_solve_bit_for_bit(mpc):
    """P = (3,) with batch 6 (x0 (2, 3, n)): one wave holds instances of three problems"""
    from tests.test_mpc_batched import _family
    n, m, N = 4, 2, 4
    ctor = _family((3,), n, m, seed=5)
    A, B, Q, R, xl, xu, ul, uu = ctor
    x0 = 0.5 * xu * np.random.default_rng(6).uniform(-1, 1, (2, 3, n))
    plain = mpc.lqrMpc(A, B, Q, R, N, xl, xu, ul, uu)
    hard = _hard(mpc.lqrMpc(A, B, Q, R, N, xl, xu, ul, uu), n, m)
    assert hard.soft_l1.shape == (3, n + m)
    xRef = 1.5 * xu[None, :, None, :] * np.sin(np.arange(N + 1)[None, None, :, None] + np.arange(6).reshape(2, 3, 1, 1))
    for refs in (False, True):
        kw = dict(max_iter=600, **(dict(xRef=xRef) if refs else {}))
        cold = [_solve(p, x0, 6, N, warm_start=False, eps_abs=1e-3, eps_rel=1e-3, **kw) for p in (plain, hard)]
        _identical(*cold, (refs, "cold"))
        warm = [_solve(p, x0, 6, N, warm_start=True, eps_abs=1e-6, eps_rel=1e-6, **kw) for p in (plain, hard)]
        _identical(*warm, (refs, "warm"))
        shift = [_solve(p, warm[0]["x"][..., 1, :].reshape(2, 3, n), 6, N, warm_start="shift", eps_abs=1e-6, eps_rel=1e-6, **kw)
                 for p in (plain, hard)]
        _identical(*shift, (refs, "shift"))
        assert "optimal" in set(warm[0]["status"].ravel())


@pytest.mark.parametrize("n,m,N", PARITY)
def test_all_hard_weights_are_the_plain_run_bit_for_bit(mpc, n, m, N):
    """simulate, 4 steps with a disturbance, clip_tol default and None, regulator (one launch) and with xRef (the queue of launches)"""
    data, x0 = ic._random(n, m, N, 1000 * n + 10 * m + N, 5)
    plain, hard = cl.problem(mpc, data, N), _hard(cl.problem(mpc, data, N), n, m)
    rng = np.random.default_rng(n + N)
    w = 0.3 * rng.standard_normal((5, 4, n))
    xRef = 2.0 * np.sin(0.5 * np.arange(4 + N)[None, :, None] + rng.uniform(0, 6, (5, 1, n)))
    for clip in (1e-6, None):
        for refs in (False, True):
            kw = dict(disturbance=w, clip_tol=clip, return_predictions=True, **(dict(xRef=xRef) if refs else {}))
            a, b = (cl.as_arrays(p.simulate(x0, 4, **kw)) for p in (plain, hard))
            for k in ("xTraj", "uTraj", "iterations", "px", "pu"):
                assert np.array_equal(getattr(a, k), getattr(b, k)), (n, m, N, clip, refs, k)
            assert np.array_equal(a.status.astype(str), b.status.astype(str)), (n, m, N, clip, refs)
            assert "optimal" in set(a.status.astype(str).ravel())


# ---- every case follows the restatement ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sf.CASES)
def test_soft_cases_follow_the_restatement(mpc, name):
    """same status, iteration count and final level; x, u, y, lam and the residuals within TOL"""
    worst = sf.compare(name, sf.run_kernel(mpc, name))
    print(f"{name}: largest deviation {worst:.2e} of its bound")


def test_the_scalar_answers_hold_on_the_device(mpc):
    c = sf.build("scalar")
    _, traj, status = sf.make_problem(mpc, c).solve(c.x0, eps_abs=1e-7, eps_rel=1e-7)
    x1 = np.asarray(traj.xTraj)[:, 1, 0]
    assert list(status) == ["optimal"] * 3 and np.max(np.abs(x1 - [w for _, w in SCALAR])) <= 1e-5, (status, x1)
    _, _, status = sf.make_problem(mpc, c, soft=False).solve(c.x0)
    assert list(status) == ["infeasible"] * 3


@pytest.mark.parametrize("name", list(sf.SCIPY))
def test_small_soft_cases_agree_with_the_slack_qp_on_the_device(mpc, name):
    """u of the device solve against the slack QP, to the 2e-3 of tests/test_mpc_ltv_soft_gpu.py"""
    c = sf.build(name)
    _, traj, status = sf.make_problem(mpc, c).solve(c.x0, **sf._solve_options(c.steps[0]))
    for b in sf.SCIPY[name]:
        assert status[b] == "optimal"
        assert np.max(np.abs(np.asarray(traj.uTraj)[b] - sf.scipy_solution(name, b)[1])) <= 2e-3, (name, b)


# ---- simulate equals the documented loop over solve ----------------------------------------------------------------------------------------

def soft_loop(prob, x0, steps, disturbance, clip_tol=1e-6, warm_start="shift", xRef=None, **opts):
    """the loop `simulate` documents for a softened object, over prob.solve on host arrays: the clip moves the hard state components only.
    Fields as tests/mpc_closed_loop_cases.py: loop."""
    N, n = prob.N, prob._n_user
    lb, ub = prob.x_lb[..., :n], prob.x_ub[..., :n]
    hard = ~np.isfinite(prob.soft_l1[..., :n])
    clip = (lambda v: v) if clip_tol is None else (lambda v: np.where(hard, np.clip(v, lb + clip_tol, ub - clip_tol), v))
    x = np.array(x0, dtype=np.float64)
    out = {k: [] for k in ("xTraj", "uTraj", "status", "iterations", "px", "pu")}
    for s in range(steps):
        x = clip(x)
        out["xTraj"].append(x)
        window = {} if xRef is None else dict(xRef=xRef[..., s:s + N + 1, :])
        u, traj, status = prob.solve(x, warm_start=(False if s == 0 else warm_start), **window, **opts)
        out["uTraj"].append(np.asarray(u))
        out["status"].append(np.asarray(status, dtype=str))
        out["iterations"].append(np.asarray(prob.last_iterations).copy())
        out["px"].append(np.asarray(traj.xTraj))
        out["pu"].append(np.asarray(traj.uTraj))
        x = out["px"][-1][..., 1, :] + disturbance[..., s, :]
    out["xTraj"].append(clip(x))
    axis = {"xTraj": -2, "uTraj": -2, "status": -1, "iterations": -1, "px": -3, "pu": -3}
    return {k: np.stack(v, axis=axis[k]) for k, v in out.items()}


def _same_run(run, ref, at):
    got = cl.as_arrays(run)
    for k in ("xTraj", "uTraj", "iterations") + (("px", "pu") if got.px is not None else ()):
        assert np.array_equal(getattr(got, k), ref[k]), (at, k)
    assert np.array_equal(got.status.astype(str), ref["status"]), at
    return got


@pytest.mark.parametrize("nb", [1, 5])
@pytest.mark.parametrize("n,m,N", sf.LOOP_SHAPES)
def test_simulate_is_the_documented_loop_bit_for_bit(mpc, n, m, N, nb):
    """6 steps, a gust at step 2 that puts state 0 of every second instance outside its soft bound; warm_start "shift", True and False;
    clip_tol default and None; with predictions; and the gust outcome: the softened run is "optimal" at every step, its recorded state is
    the plant's, it returns inside the box; the hard run of the same inputs is not "optimal" after the gust, or records another state"""
    data, soft, x0, w = sf.loop_case(n, m, N, nb)
    kw_soft = sf.soften_kw(n, soft)
    xu = data[6][0]
    for warm in ("shift", True, False):
        for clip in (1e-6, None):
            one, two = cl.problem(mpc, data, N).soften(**kw_soft), cl.problem(mpc, data, N).soften(**kw_soft)
            ref = soft_loop(two, x0, sf.STEPS, w, clip_tol=clip, warm_start=warm)
            run = one.simulate(x0, sf.STEPS, disturbance=w, clip_tol=clip, warm_start=warm, return_predictions=True)
            got = _same_run(run, ref, (n, m, N, nb, warm, clip))
            if warm == "shift" and clip is not None:
                default = ref
            # a soft component is never clipped: the plant's state exactly; the hard ones are clipped as before
            plant = got.px[..., :, 1, :] + w
            assert np.array_equal(got.xTraj[..., 1:, 0], plant[..., 0])
            if clip is not None:
                assert np.array_equal(got.xTraj[..., 1:, 1:], np.clip(plant[..., 1:], data[5][1:] + clip, data[6][1:] - clip))
            assert np.all(got.status.astype(str) == "optimal")
            assert np.all(got.xTraj[::2, sf.GUST_STEP + 1, 0] > xu + 0.4) and np.all(np.abs(got.xTraj[:, -1, 0]) <= xu)
            # the hard run of the same inputs
            hard = cl.as_arrays(cl.problem(mpc, data, N).simulate(x0, sf.STEPS, disturbance=w, clip_tol=clip, warm_start=warm,
                                                                 return_predictions=True))
            after = sf.GUST_STEP + 1
            if clip is None:
                assert np.all(hard.status[::2, after].astype(str) == "infeasible")
            else:
                assert np.all(hard.xTraj[::2, after, 0] == xu - clip) and np.all(hard.px[::2, after - 1, 1, 0] + w[::2, after - 1, 0] > xu)
    # without predictions (every step's rollout in one scratch): the same run
    bare = cl.as_arrays(cl.problem(mpc, data, N).soften(**kw_soft).simulate(x0, sf.STEPS, disturbance=w))
    assert bare.px is None and np.array_equal(bare.xTraj, default["xTraj"]) and np.array_equal(bare.uTraj, default["uTraj"])
    assert np.array_equal(bare.iterations, default["iterations"])


@pytest.mark.parametrize("n,m,N", sf.LOOP_SHAPES)
def test_simulate_with_a_reference_is_the_documented_loop_bit_for_bit(mpc, n, m, N):
    """xRef: the queue of launches (the soft solve kernel with a reference term, mpc_advance_soft_kernel between the steps)"""
    data, soft, x0, w = sf.loop_case(n, m, N, 5)
    kw_soft = sf.soften_kw(n, soft)
    rng = np.random.default_rng(3 * n + N)
    xRef = 2.0 * np.sin(0.5 * np.arange(sf.STEPS + N)[None, :, None] + rng.uniform(0, 6, (5, 1, n)))
    for clip in (1e-6, None):
        one, two = cl.problem(mpc, data, N).soften(**kw_soft), cl.problem(mpc, data, N).soften(**kw_soft)
        ref = soft_loop(two, x0, sf.STEPS, w, clip_tol=clip, xRef=xRef)
        got = _same_run(one.simulate(x0, sf.STEPS, disturbance=w, clip_tol=clip, xRef=xRef, return_predictions=True), ref, (n, m, N, clip))
        assert np.array_equal(got.xTraj[..., 1:, 0], (got.px[..., :, 1, :] + w)[..., 0])
        assert np.any(np.abs(got.xTraj[..., 0]) > data[6][0])           # (the reference of amplitude 2 and the gust take state 0 outside 1.2)


def test_simulate_with_per_problem_weights_is_the_documented_loop_bit_for_bit(mpc):
    """P = (3,): state 0 soft in problems 0 and 2 with their own weights, hard in problem 1 -- whose state is clipped where theirs is not"""
    n, m, N = 4, 2, 5
    data, _, x0, w = sf.loop_case(n, m, N, 3)
    A, B, Q, R, Qf, xl, xu, ul, uu = data
    l1 = np.full((3, n), INF)
    l1[0, 0], l1[2, 0] = 20.0, 5.0
    l2 = np.zeros((3, n))
    l2[2, 0] = 2.0
    w = w.copy()
    w[1, sf.GUST_STEP, 0] = w[0, sf.GUST_STEP, 0]                        # (the hard problem's instance is gusted as well)
    make = lambda: mpc.lqrMpc(np.stack([A] * 3), B, Q, R, N, xl, xu, ul, uu, Qf=Qf).soften(x_soft_l1=l1, x_soft_l2=l2)
    ref = soft_loop(make(), x0, sf.STEPS, w)
    got = _same_run(make().simulate(x0, sf.STEPS, disturbance=w, return_predictions=True), ref, "per-problem weights")
    after = sf.GUST_STEP + 1
    assert got.xTraj[0, after, 0] > xu[0] + 0.4 and got.xTraj[2, after, 0] > xu[0] + 0.4 and got.xTraj[1, after, 0] == xu[0] - 1e-6


# ---- new weights, and what simulate leaves behind ------------------------------------------------------------------------------------------

def test_new_weights_between_two_solves_launch_no_setup(mpc):
    """soften with new weights keeps `_tables` (the same object, the same entries) and the workspace: the second solve equals a fresh
    object's warm-started solve with those weights.  (The quadratic case: its solution moves by more than 2e-3 in u with these weights.)"""
    c = sf.build("quadratic")
    second = sf.soften_kw(4, _weights(4, 2, x1={0: 0.0}, x2={0: 0.3}, u1={1: 0.0}, u2={1: 0.1}))
    kw = dict(eps_abs=1e-6, eps_rel=1e-6, max_iter=30000)
    a = sf.make_problem(mpc, c)
    ra0 = _solve(a, c.x0, 5, c.N, warm_start=False, **kw)
    tables, entries, ws = a._tables, dict(a._tables), a._ws[1]
    assert a.soften(**second) is a
    ra1 = _solve(a, c.x0, 5, c.N, warm_start=True, **kw)
    assert a._tables is tables and list(a._tables) == list(entries) and all(a._tables[k] is v for k, v in entries.items())
    assert a._ws[1] is ws
    b = sf.make_problem(mpc, c)
    _identical(ra0, _solve(b, c.x0, 5, c.N, warm_start=False, **kw), "first solve")
    fresh = sf.make_problem(mpc, c, soft=False).soften(**second)
    fresh._ws = b._ws                                                   # (a fresh object with those weights, started from that state)
    _identical(ra1, _solve(fresh, c.x0, 5, c.N, warm_start=True, **kw), "second solve")
    assert set(ra1["status"]) == {"optimal"} and np.all(np.max(np.abs(ra1["uT"] - ra0["uT"]), axis=(1, 2)) > 1e-3)      # (the new weights matter)
    cold = _solve(sf.make_problem(mpc, c, soft=False).soften(**second), c.x0, 5, c.N, warm_start=False, **kw)
    assert np.all(ra1["iters"] < cold["iters"])                         # (and it was a warm start)


def test_simulate_leaves_the_solve_state_alone(mpc):
    n, m, N = 4, 2, 5
    data, soft, x0, w = sf.loop_case(n, m, N, 5)
    kw = dict(eps_abs=1e-6, eps_rel=1e-6)
    a, b = (cl.problem(mpc, data, N).soften(**sf.soften_kw(n, soft)) for _ in range(2))
    first = [_solve(p, x0, 5, N, warm_start=False, **kw) for p in (a, b)]
    _identical(*first, "first solve")
    its, res, ws = a.last_iterations.copy(), a.last_residuals.copy(), a._ws[1]
    a.simulate(x0, sf.STEPS, disturbance=w)
    assert a._ws[1] is ws and np.array_equal(a.last_iterations, its) and np.array_equal(a.last_residuals, res)
    x1 = first[0]["x"][..., 1, :]
    _identical(_solve(a, x1, 5, N, warm_start="shift", **kw), _solve(b, x1, 5, N, warm_start="shift", **kw), "the solve after the run")
