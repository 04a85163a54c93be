"""GPU tests of lqrMpc.simulate (zm_mpc_closed_loop_f64): the receding-horizon loop as one call -- the fused kernel with the step loop
inside (mpc_wave.hip: mpc_closed_loop_wave_kernel) for regulator runs at the 16-lane shapes, the host loop of launches (mpc.hip) for
tracking runs, (24, 8), horizons beyond LDS and the forced lane path.

The yardstick is the Python loop over `solve` on a second lqrMpc object of the same data (tests/mpc_closed_loop_cases.py: loop, hold):
same statuses, same iteration counts, states / inputs / predictions within 1e-9 max(1, max |loop's value|), for every instance and step."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import mpc_closed_loop_cases as cc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = dict(eps_abs=1e-6, eps_rel=1e-6)


@pytest.fixture(scope="module")
def mpc():
    import torch
    assert torch.cuda.is_available()
    from zopt_amd import mpcUtils
    return mpcUtils


def _both(prob, prob2, x0, steps, what, **kw):
    """simulate on `prob` (with predictions) against the loop on `prob2`"""
    ref = cc.loop(prob2, x0, steps, **kw)
    got = cc.as_arrays(prob.simulate(x0, steps, return_predictions=True, **kw))
    cc.hold(got, ref, what)
    return got, ref


# 1. shapes ------------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 2), (2, 1, 3), (2, 1, 4), (4, 2, 5), (8, 4, 3), (12, 4, 7), (3, 2, 5), (9, 4, 7)]


@pytest.mark.parametrize("nb", [1, 4, 5])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: ",".join(map(str, s)))
def test_shapes_batches_and_step_counts(mpc, shape, nb):
    """N on both sides of the three-stage unroll, NS + MC below and at 16, two embedded shapes; batch 5 leaves three idle groups in the last
    wave; 1, 2 and 6 steps (the loop of 6 steps is the yardstick of all three: its first steps are the shorter loops'), with and without
    the predictions (the run without them rolls every step out into one scratch)"""
    n, m, N = shape
    prob, prob2, x0, _ = cc.random_pair(mpc, n, m, N, nb)
    ref = cc.loop(prob2, x0, 6, **EPS)
    for steps in (1, 2, 6):
        for pred in (True, False):
            got = cc.as_arrays(prob.simulate(x0, steps, return_predictions=pred, **EPS))
            assert (got.px is not None) == pred
            cc.hold(got, ref, f"{shape} batch {nb} steps {steps} predictions {pred}", steps=steps)


# 2. options -----------------------------------------------------------------------------------------------------------------------
OPTIONS = [dict(warm_start=False), dict(warm_start=True), dict(warm_start="shift"), dict(adaptive_rho=False), dict(adaptive_rho=True, alpha=1.0),
           dict(alpha=1.6, rho=0.7), dict(adaptive_rho=False, alpha=1.0, rho=2.5, warm_start=True)]


@pytest.mark.parametrize("opts", OPTIONS, ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()))
@pytest.mark.parametrize("shape", [(4, 2, 5), (12, 4, 7)], ids=lambda s: ",".join(map(str, s)))
def test_options(mpc, shape, opts):
    n, m, N = shape
    prob, prob2, x0, _ = cc.random_pair(mpc, n, m, N, 5)
    _both(prob, prob2, x0, 6, f"{shape} {opts}", **EPS, **opts)


# 3. mixed statuses inside one wave ------------------------------------------------------------------------------------------------
def _mixed(mpc, shape):
    """four instances of one wave: at the origin, deep in saturation (near the corner of the state box), two ordinary ones; instance 2 is
    pushed out of its state box by the disturbance of step 2 and put back inside by that of step 3 (which cancels the successor state the
    yardstick's own step 3 leaves -- read from a first pass of the loop -- and adds half the start)"""
    n, m, N = shape
    prob, prob2, x0, data = cc.random_pair(mpc, n, m, N, 4)
    x0[0] = 0.0
    x0[1] = 3.5 * np.sign(x0[1])
    w = np.zeros((4, 6, n))
    w[2, 2, 0] = 6.0      # the state box is |x| <= 4
    first = cc.loop(cc.problem(mpc, data, N), x0, 4, disturbance=w[:, :4], clip_tol=None, **EPS)
    w[2, 3] = 0.5 * x0[2] - first.px[2, 3, 1]
    return prob, prob2, x0, w


@pytest.mark.parametrize("shape", [(4, 2, 5), (12, 4, 7)], ids=lambda s: ",".join(map(str, s)))
def test_an_instance_leaves_its_box_and_restarts_cold_beside_warm_neighbours(mpc, shape):
    """clip_tol=None: the pushed instance's step 3 is "infeasible" (its state is outside the box), the run goes on from the rollout the
    solve leaves, and its step 4 starts cold (the stored `ok` flag) while its wave neighbours start warm"""
    prob, prob2, x0, w = _mixed(mpc, shape)
    got, ref = _both(prob, prob2, x0, 6, f"{shape} pushed out", disturbance=w, clip_tol=None, **EPS)
    st = ref.status.astype(str)
    assert st[2, 3] == "infeasible" and ref.iterations[2, 3] == 0, st.tolist()
    assert np.max(np.abs(ref.xTraj[2, 3])) > 4.0
    assert set(st[2, :3].tolist()) == {"optimal"} and st[2, 4] == "optimal", st.tolist()
    assert set(st[[0, 3]].ravel().tolist()) == {"optimal"}, st.tolist()
    assert ref.iterations[0].max() <= 1 < ref.iterations[1].max()      # very different difficulty in one wave


@pytest.mark.parametrize("shape", [(4, 2, 5), (12, 4, 7)], ids=lambda s: ",".join(map(str, s)))
def test_iteration_cap_inside_the_run(mpc, shape):
    """max_iter=16: some steps end "user_limit" / "optimal_inaccurate", and the step after such a one starts cold"""
    prob, prob2, x0, w = _mixed(mpc, shape)
    got, ref = _both(prob, prob2, x0, 6, f"{shape} max_iter=16", disturbance=w, max_iter=16, **EPS)
    st = set(ref.status.astype(str).ravel().tolist())
    assert "optimal" in st and st & {"user_limit", "optimal_inaccurate"}, st


# 4. disturbance and clip ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(4, 2, 5), (12, 4, 7)], ids=lambda s: ",".join(map(str, s)))
def test_disturbance_and_clip(mpc, shape):
    """a seeded disturbance large enough to hit the clip, bounds with +-inf components"""
    n, m, N = shape
    from tests.mpc_iterates_cases import _random
    data, x0 = _random(n, m, N, 77, 5)
    A, B, Q, R, Qf, xl, xu, ul, uu = data
    xl, xu = xl.copy(), xu.copy()
    xu[0], xl[n - 1] = np.inf, -np.inf
    xl[: n // 2], xu[: n // 2] = np.maximum(xl[: n // 2], -1.2), np.minimum(xu[: n // 2], 1.2)
    data = (A, B, Q, R, Qf, xl, xu, ul, uu)
    prob, prob2 = cc.problem(mpc, data, N), cc.problem(mpc, data, N)
    w = 0.8 * np.random.default_rng(5).standard_normal((5, 6, n))
    tol = 1e-6
    got, ref = _both(prob, prob2, x0, 6, f"{shape} disturbance + clip", disturbance=w, clip_tol=tol, **EPS)
    assert np.array_equal(got.xTraj[:, :6], got.px[:, :, 0]), "the state a step is solved from is row 0 of its prediction"
    assert np.all(got.xTraj >= xl + tol) and np.all(got.xTraj <= xu - tol)
    assert np.any(got.xTraj[..., : n // 2] == 1.2 - tol) or np.any(got.xTraj[..., : n // 2] == -1.2 + tol), "the clip never acted"


# 5. per-problem data --------------------------------------------------------------------------------------------------------------
def test_per_problem_data(mpc):
    """P = (3,), x0 (2, 3, n), per-problem rho, a disturbance (3, S, n) that broadcasts over the leading 2"""
    from tests.test_mpc_batched import _family
    n, m, N, S = 4, 2, 6, 5
    A, B, Q, R, xl, xu, ul, uu = _family((3,), n, m, seed=42)
    mk = lambda: mpc.lqrMpc(A, B, Q, R, N, xl, xu, ul, uu)
    prob, prob2 = mk(), mk()
    assert prob.P == (3,)
    rng = np.random.default_rng(43)
    x0 = 0.8 * xu * rng.uniform(-1, 1, (2, 3, n))
    w = 0.05 * xu[:, None, :] * rng.standard_normal((3, S, n))
    rho = np.array([0.5, 1.0, 3.0]) * prob.rho
    got, ref = _both(prob, prob2, x0, S, "per-problem", disturbance=w, rho=rho, eps_abs=1e-5, eps_rel=1e-5, max_iter=3000)
    assert got.xTraj.shape == (2, 3, S + 1, n) and got.status.shape == (2, 3, S) and got.px.shape == (2, 3, S, N + 1, n)


# 6. tracking: the host loop ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["both", "uRef", "xRef", "zero"])
@pytest.mark.parametrize("shape", [(4, 2, 5), (12, 4, 7)], ids=lambda s: ",".join(map(str, s)))
def test_tracking_moves_the_reference_window(mpc, shape, which):
    """ramp references of S + N (S + N - 1) rows against the loop that passes the moved windows; a zero reference is the regulator run"""
    n, m, N = shape
    S, nb = 5, 5
    prob, prob2, x0, data = cc.random_pair(mpc, n, m, N, nb)
    rng = np.random.default_rng(9)
    t = np.arange(S + N)
    xRef = 0.05 * t[None, :, None] * rng.uniform(-1, 1, (nb, 1, n))       # up to 0.55: inside the state box
    uRef = 0.01 * t[None, :S + N - 1, None] * rng.uniform(-1, 1, (1, 1, m))  # (broadcasts over the batch)
    refs = {"both": dict(xRef=xRef, uRef=uRef), "uRef": dict(uRef=uRef), "xRef": dict(xRef=xRef),
            "zero": dict(xRef=np.zeros((S + N, n)))}[which]
    got, ref = _both(prob, prob2, x0, S, f"{shape} tracking {which}", **refs, **EPS)
    if which == "zero":
        plain = cc.as_arrays(cc.problem(mpc, data, N).simulate(x0, S, return_predictions=True, **EPS))
        cc.hold(got, plain, f"{shape} zero reference against the regulator run")
    else:
        reg = cc.loop(prob2, x0, 1, **EPS)
        assert np.max(np.abs(reg.uTraj - ref.uTraj[:, :1])) > 1e-6, "the reference changes nothing: the test shows nothing"


# 7. the host loop for the other shapes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(13, 2, 6), (24, 8, 4), (4, 2, 80)], ids=lambda s: ",".join(map(str, s)))
def test_host_loop_for_shapes_beyond_the_wave_kernels(mpc, shape):
    """n > 12 / m > 4 (the lane-per-instance kernel, embedded or not) and a horizon that does not fit LDS"""
    n, m, N = shape
    prob, prob2, x0, _ = cc.random_pair(mpc, n, m, N, 4)
    w = 0.02 * np.random.default_rng(3).standard_normal((4, 3, n))
    _both(prob, prob2, x0, 3, f"{shape} host loop", disturbance=w, eps_abs=1e-5, eps_rel=1e-5)


def test_forced_lane_path_in_a_child_process(tmp_path):
    """(12, 4, 5) and (2, 1, 3) under ZOPT_AMD_MPC_PATH=lane (read once per process): simulate and the yardstick loop both run in the child"""
    out_file = str(tmp_path / "lane.npz")
    env = dict(os.environ, ZOPT_AMD_MPC_PATH="lane")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mpc_closed_loop_lane_child.py"), out_file], env=env,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "MPC-CLOSED-LOOP-LANE-OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    z = np.load(out_file)
    from types import SimpleNamespace
    fields = ("xTraj", "uTraj", "status", "iterations", "px", "pu")
    for shape in ((12, 4, 5), (2, 1, 3)):
        got = SimpleNamespace(**{k: z[f"{shape}|got|{k}"] for k in fields})
        ref = SimpleNamespace(**{k: z[f"{shape}|ref|{k}"] for k in fields})
        cc.hold(got, ref, f"{shape} forced lane path")


# 8. no side effects -----------------------------------------------------------------------------------------------------------------
def test_simulate_leaves_the_solve_state_alone(mpc):
    import torch
    prob, prob2, x0, _ = cc.random_pair(mpc, 4, 2, 5, 5)
    x1 = 0.9 * x0
    a = prob.solve(x0, **EPS)
    its = prob.last_iterations.copy()
    res = prob.last_residuals.copy()
    run = prob.simulate(1.1 * x0, 4, **EPS)
    assert np.array_equal(prob.last_iterations, its) and np.array_equal(prob.last_residuals, res)
    b = prob.solve(x1, warm_start=True, **EPS)
    prob2.solve(x0, **EPS)
    b2 = prob2.solve(x1, warm_start=True, **EPS)
    assert np.array_equal(b[1].xTraj, b2[1].xTraj) and np.array_equal(b[1].uTraj, b2[1].uTraj)
    assert np.array_equal(np.asarray(b[2], dtype=str), np.asarray(b2[2], dtype=str))
    assert np.array_equal(prob.last_iterations, prob2.last_iterations)
    assert min(prob.last_iterations.max(), its.max()) > 1 and not np.array_equal(prob.last_iterations, its)   # the warm start did act
    # array families: NumPy in, NumPy out; device tensor in, device tensors out (status stays an object array of strings)
    assert all(isinstance(v, np.ndarray) for v in (run.xTraj, run.uTraj, run.status, run.iterations)) and run.predictions is None
    assert run.iterations.dtype == np.int32 and run.status.dtype == object
    trun = prob.simulate(torch.as_tensor(1.1 * x0, device="cuda"), 4, return_predictions=True, **EPS)
    for v in (trun.xTraj, trun.uTraj, trun.iterations, trun.predictions.xTraj, trun.predictions.uTraj):
        assert isinstance(v, torch.Tensor) and v.is_cuda
    assert trun.iterations.dtype == torch.int32 and isinstance(trun.status, np.ndarray)
    assert np.array_equal(trun.xTraj.cpu().numpy(), run.xTraj) and np.array_equal(trun.status.astype(str), run.status.astype(str))


def test_one_step_is_one_solve(mpc):
    prob, prob2, x0, _ = cc.random_pair(mpc, 12, 4, 7, 5)
    run = prob.simulate(x0, 1, clip_tol=None, return_predictions=True, **EPS)
    u, traj, status = prob2.solve(x0, warm_start=False, **EPS)
    assert np.array_equal(run.status[:, 0].astype(str), np.asarray(status, dtype=str))
    assert np.array_equal(run.iterations[:, 0], prob2.last_iterations)
    tol = cc.TOL * max(1.0, np.max(np.abs(traj.xTraj)))
    assert np.max(np.abs(run.predictions.xTraj[:, 0] - traj.xTraj)) <= tol and np.max(np.abs(run.predictions.uTraj[:, 0] - traj.uTraj)) <= tol
    assert np.max(np.abs(run.uTraj[:, 0] - u)) <= tol and np.max(np.abs(run.xTraj[:, 1] - traj.xTraj[:, 1])) <= tol
    assert np.array_equal(run.xTraj[:, 0], x0)
    # a single instance: no batch axis anywhere
    one = prob.simulate(x0[0], 3, return_predictions=True, **EPS)
    assert one.xTraj.shape == (4, 12) and one.uTraj.shape == (3, 4) and one.status.shape == (3,) and one.iterations.shape == (3,)
    assert one.predictions.xTraj.shape == (3, 8, 12)      # the array io.mpc_trajectory_array describes, per step
