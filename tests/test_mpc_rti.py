"""CPU checks for ltvMpc.realTimeIteration / relinearize / fromModel and mpcUtils.modelStep: the NumPy restatement of the loop
(tests/mpc_rti_ref.py: run) against an independent SciPy solve and against the time-invariant restatement, the decisiveness of every input
that tests/test_mpc_rti_gpu.py compares with it, and the host-side argument checks.  No GPU."""
import numpy as np
import pytest

from tests import mpc_ltv_ref as lr
from tests import mpc_rti_ref as rr
from tests import mpc_tracking_ref as tr
from zopt_amd import models, mpcUtils, pytrees


# 1. the restatement ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(rr.CASES))
def test_one_step_is_the_qp_of_its_linearisation(name):
    """step 0 of instance 0: the ADMM's solution is that of the QP with the same A_k, B_k, c_k and reference window (condensed, SciPy
    trust-constr), to the tolerance of tests/test_mpc_ltv.py::test_solutions_agree_with_an_independent_solve"""
    c = rr.CASES[name]()
    Q, R, Qf, xl, xu, ul, uu = c.data
    r = rr.reference(name)[0]
    assert r.status[0] == "optimal"
    A, B, ck, f = rr.expansion(c.step, c.plan[0][0], c.plan[1][0])
    assert np.max(np.abs(np.real(np.stack([c.step(x, u) for x, u in zip(c.plan[0][0][:-1], c.plan[1][0])])) - f)) == 0.0
    xs, us, _ = lr.solve_reference_ltv(A, B, ck, Q, R, Qf, c.N, xl, xu, ul, uu, r.states[0], xRef=c.xRef[0, :c.N + 1], uRef=c.uRef[0, :c.N])
    dev = np.max(np.abs(r.pu[0] - us))
    print(f"{name}: {r.iters[0]} iterations, deviation of u from SciPy {dev:.2e}")
    assert dev <= 2e-3
    assert np.array_equal(r.inputs[0], r.pu[0][0]) and np.array_equal(r.states[0], r.px[0][0])
    assert np.array_equal(r.states[1], np.clip(np.real(c.step(r.states[0], r.inputs[0])), xl + 1e-6, xu - 1e-6))


def test_a_linear_model_is_the_time_invariant_loop():
    """LinearModel: c_k is at rounding level and the run's states are those of a loop of the time-invariant tracking restatement
    (tests/mpc_tracking_ref.py: admm) to 1e-9.  One penalty level and cold starts on both sides: neither then has a cycle guard to differ
    in (admm_levels_ltv would switch it on for the rounding-level c)."""
    n, m, N, S = 4, 2, 5, 4
    (A, B, Q, R, Qf, xl, xu, ul, uu), x0, xRef, uRef = tr.random_case(n, m, N, seed=41, nb=1)
    t = np.arange(S + N)
    xRef = 0.05 * t[:, None] * np.linspace(-1, 1, n)[None, :]
    uRef = 0.01 * t[:S + N - 1, None] * np.ones((1, m))
    rho = tr.default_rho(Q, R)
    plan = (np.tile(x0[0], (N + 1, 1)) * np.linspace(1.0, 0.5, N + 1)[:, None], 0.05 * np.ones((N, m)))
    kw = dict(eps_abs=1e-7, eps_rel=1e-7, max_iter=30000, alpha=1.6)
    cs = []

    def solve(Ak, Bk, ck, *a, **k):
        cs.append(np.max(np.abs(ck)))
        return lr.admm_levels_ltv(Ak, Bk, ck, *a, **k)
    got = rr.run(rr.linear_step(A, B), (Q, R, Qf, xl, xu, ul, uu), N, x0[0], plan, S, xRef=xRef, uRef=uRef, warm=False, rho=rho,
                 n_levels=1, solve=solve, **kw)
    assert max(cs) <= 16 * np.finfo(float).eps * (1.0 + np.max(np.abs(plan[0]))) * max(1.0, np.max(np.abs(A)), np.max(np.abs(B)))
    x = x0[0]
    for s in range(S):
        x = np.clip(x, xl + 1e-6, xu - 1e-6)
        assert np.max(np.abs(got.states[s] - x)) <= 1e-9
        xs, us, status, it = tr.admm(A, B, Q, R, Qf, N, xl, xu, ul, uu, x, xRef[s:s + N + 1], uRef[s:s + N], rho=rho, **kw)
        assert status == got.status[s] == "optimal" and it == got.iters[s]
        x = A @ x + B @ us[0]
    assert np.max(np.abs(got.states[S] - np.clip(x, xl + 1e-6, xu - 1e-6))) <= 1e-9


# 2. decision margins ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(rr.CASES))
def test_gpu_cases_are_decisive(name):
    """every input tests/test_mpc_rti_gpu.py compares with the restatement: the expansion perturbed by 1e-12 relative (far more than the
    closed forms and the complex step differ by) leaves every status, iteration count and final penalty level of every step as it is"""
    ref, per = rr.reference(name), rr.reference(name, 1e-12)
    for b, (r, p) in enumerate(zip(ref, per)):
        assert r.status == p.status and r.iters == p.iters and r.level == p.level, (name, b, r.status, p.status, r.iters, p.iters)
        assert all(q.moves == w.moves and q.locked == w.locked for q, w in zip(r.results, p.results)), (name, b)
        assert np.max(np.abs(r.states - p.states)) <= 1e-9
    assert {s for r in ref for s in r.status} == {"optimal"}
    assert any(q.moves for r in ref for q in r.results), "the penalty never moved: the levels are not exercised"


# 3. host-side argument checks ----------------------------------------------------------------------------------------------------------
def _problem(nb=3, N=4):
    model = models.QuadcopterEuler(0.1)
    A, B = np.tile(np.eye(12), (nb, N, 1, 1)), np.zeros((nb, N, 12, 4))
    xu, uu = np.full(12, 4.0), np.full(4, 20.0)
    return model, mpcUtils.ltvMpc(A, B, np.eye(12), np.eye(4), N, -xu, xu, -uu, uu)


@pytest.fixture()
def no_gpu(monkeypatch):
    """anything that reaches for the GPU fails the test: the errors below are raised by host code alone"""
    from zopt_amd import _arrays

    def boom(*a, **k):
        raise AssertionError("the GPU was touched before the argument check")
    monkeypatch.setattr(_arrays, "require_gpu", boom)
    monkeypatch.setattr(_arrays, "to_device", boom)


def test_argument_errors_come_from_the_host(no_gpu):
    model, prob = _problem()
    nb, N, S = 3, 4, 2
    x0 = np.zeros((nb, 12))
    good = pytrees.Trajectory(np.zeros((nb, N + 1, 12)), np.zeros((nb, N, 4)))
    rti = prob.realTimeIteration
    with pytest.raises(ValueError, match="steps must be at least 1"):
        rti(model, x0, 0)
    with pytest.raises(ValueError, match=r"x0 has shape \(3, 11\)"):
        rti(model, np.zeros((nb, 11)), S)
    with pytest.raises(ValueError, match=r"plan has xTraj of shape \(3, 4, 12\)"):
        rti(model, x0, S, plan=pytrees.Trajectory(np.zeros((nb, N, 12)), np.zeros((nb, N, 4))))
    with pytest.raises(ValueError, match=r"plan has xTraj of shape .* uTraj of shape \(3, 4, 3\)"):
        rti(model, x0, S, plan=pytrees.Trajectory(np.zeros((nb, N + 1, 12)), np.zeros((nb, N, 3))))
    with pytest.raises(ValueError, match=r"xRef has shape \(3, 5, 12\), expected \(\.\.\., 6, 12\) for steps = 2, N = 4"):
        rti(model, x0, S, xRef=np.zeros((nb, 5, 12)))
    with pytest.raises(ValueError, match=r"uRef has shape \(5, 3\)"):
        rti(model, x0, S, uRef=np.zeros((5, 3)))
    with pytest.raises(ValueError, match=r"disturbance has shape \(3, 3, 12\)"):
        rti(model, x0, S, disturbance=np.zeros((nb, 3, 12)))
    with pytest.raises(ValueError, match="not a Trajectory"):
        rti(model, x0, S, xRef=good)
    with pytest.raises(ValueError, match=r"do not broadcast to the problem shape \(3,\)"):
        rti(model, np.zeros((2, 12)), S)
    with pytest.raises(ValueError, match=r"do not broadcast to the problem shape \(3,\)"):
        rti(model, np.zeros((5, 3, 12)), S)          # (more instances than problems: every instance is its own problem)
    with pytest.raises(ValueError, match=r"the plant has \(n=8, m=4\), the problem \(n=12, m=4\)"):
        rti(model, x0, S, plant=models.QuadcopterRigidBody(dt=0.1))
    with pytest.raises(ValueError, match=r"the model has \(n=8, m=4\), the problem \(n=12, m=4\)"):
        rti(models.QuadcopterRigidBody(dt=0.1), x0, S)
    with pytest.raises(ValueError, match="needs a step dt > 0"):
        rti(models.QuadcopterEuler(0.0), x0, S)
    with pytest.raises(ValueError, match="clip_tol must be non-negative"):
        rti(model, x0, S, clip_tol=-1.0)
    with pytest.raises(TypeError, match="unknown solver options"):
        rti(model, x0, S, no_such_option=1)
    with pytest.raises(ValueError, match="registered model"):
        rti(lambda x, u: x, x0, S)
    with pytest.raises(ValueError, match=r"relinearize: plan has xTraj of shape \(3, 4, 12\)"):
        prob.relinearize(model, pytrees.Trajectory(np.zeros((nb, N, 12)), np.zeros((nb, N, 4))))
    with pytest.raises(ValueError, match=r"broadcast to the problem shape \(3,\)"):
        prob.relinearize(model, pytrees.Trajectory(np.zeros((2, N + 1, 12)), np.zeros((2, N, 4))))
    with pytest.raises(ValueError, match=r"relinearize: the model has \(n=8, m=4\)"):
        prob.relinearize(models.QuadcopterRigidBody(dt=0.1), good)


def test_models_outside_the_kernels_are_refused_on_the_host(no_gpu):
    big = models.LinearModel(np.eye(13), np.ones((13, 2)))
    wide = models.LinearModel(np.eye(4), np.ones((4, 5)))
    plan = pytrees.Trajectory(np.zeros((4, 13)), np.zeros((3, 2)))
    one = np.ones(13)
    for model in (big, wide):
        with pytest.raises(ValueError, match=r"outside the kernels for stage-varying dynamics \(n <= 12, m <= 4\)"):
            mpcUtils.ltvMpc.fromModel(model, plan, np.eye(13), np.eye(2), -one, one, -one[:2], one[:2])
        with pytest.raises(ValueError, match=r"outside the kernels"):
            mpcUtils.modelStep(model, np.zeros(model.n), np.zeros(model.m))
        with pytest.raises(ValueError, match=r"outside the kernels"):
            _problem()[1].realTimeIteration(model, np.zeros((3, 12)), 2)
    quad = models.QuadcopterEuler(0.1)
    with pytest.raises(ValueError, match=r"fromModel: plan has xTraj of shape \(5, 12\) and uTraj of shape \(5, 4\)"):
        mpcUtils.ltvMpc.fromModel(quad, pytrees.Trajectory(np.zeros((5, 12)), np.zeros((5, 4))), np.eye(12), np.eye(4), -1, 1, -1, 1)
    with pytest.raises(ValueError, match=r"modelStep: x of shape \(2, 12\), u of shape \(3, 4\) do not broadcast"):
        mpcUtils.modelStep(quad, np.zeros((2, 12)), np.zeros((3, 4)))
    with pytest.raises(ValueError, match=r"modelStep: x has shape \(11,\)"):
        mpcUtils.modelStep(quad, np.zeros(11), np.zeros(4))


def test_simulate_still_refuses_and_names_the_new_call():
    with pytest.raises(NotImplementedError, match="realTimeIteration"):
        _problem()[1].simulate(np.zeros((3, 12)), 2)
