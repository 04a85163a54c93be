"""GPU tests of real-time-iteration MPC with ltvMpc: relinearize / fromModel (zm_mpc_relinearize_f64), mpcUtils.modelStep
(zm_model_step_f64) and realTimeIteration (zm_mpc_rti_f64), the whole loop as one call.

Yardsticks: the oracle's complex-step expansion for A_k, B_k and the float64 formula for c_k; the Python loop of public calls
(`loop` below: relinearize, solve, modelStep, shift) for the one call, BIT FOR BIT; the NumPy restatement of that loop
(tests/mpc_rti_ref.py) on the inputs whose decisions tests/test_mpc_rti.py has checked."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import zopt_oracle as zo
from tests import mpc_iterates_cases as mc
from tests import mpc_ltv_ref as lr
from tests import mpc_rti_ref as rr

pytestmark = pytest.mark.gpu

DEMO = dict(eps_abs=1e-4, eps_rel=1e-4, max_iter=4000)


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available()
    from zopt_amd import _lib, models, mpcUtils, pytrees
    return SimpleNamespace(torch=torch, lib=_lib, models=models, mpc=mpcUtils, pytrees=pytrees)


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------
def _linear_case(n, m, N, nb, S, seed):
    """a random stable LinearModel with the boxes of tests/mpc_ltv_ref.py: recipe, plans that are not trajectories of it, ramps to track"""
    from tests.test_mpc_gpu import _random_problem
    rng = np.random.default_rng(seed)
    A, B, Q, R, Qf = _random_problem(rng, n, m, N)
    xu, uu = np.full(n, 4.0), np.full(m, 0.15)
    x0 = rng.uniform(-1.0, 1.0, (nb, n))
    plan = (rng.uniform(-1.0, 1.0, (nb, N + 1, n)), 0.1 * rng.standard_normal((nb, N, m)))
    t = np.arange(S + N)
    xRef = 0.05 * t[None, :, None] * rng.uniform(-1, 1, (nb, 1, n))
    uRef = 0.01 * t[None, :S + N - 1, None] * rng.uniform(-1, 1, (nb, 1, m))
    return SimpleNamespace(kind="linear", AB=(A, B), step=rr.linear_step(A, B), N=N, S=S, nb=nb, x0=x0, plan=plan, xRef=xRef, uRef=uRef,
                           data=(Q, R, Qf, -xu, xu, -uu, uu))


def _case(name):
    if name == "quad":
        return rr.quad_case(5, 7, 4)
    if name == "rigid_body":
        return rr.rigid_body_case(4, 5, 3)
    if name == "embedded":
        return _linear_case(3, 2, 3, 5, 3, seed=21)
    if name == "linear12":
        return _linear_case(12, 4, 3, 5, 3, seed=22)
    if name == "N75":   # the longest horizon whose iterates fit LDS; the plan holds the start (the random plans drift far over 75 stages)
        c = rr.quad_case(75, 1, 2)
        du = 0.05 * np.random.default_rng(2).standard_normal(c.plan[1].shape)
        return SimpleNamespace(**{**vars(c), "plan": (np.repeat(c.x0[:, None, :], 76, axis=1), rr.QUAD_UTRIM + du)})
    raise KeyError(name)


def _model(g, c, wind=None):
    if c.kind == "quad":
        return g.models.QuadcopterEuler(c.dt, wind_ned=wind or (0.0, 0.0, 0.0))
    if c.kind == "rb":
        return g.models.QuadcopterRigidBody(dt=c.dt)
    return g.models.LinearModel(*c.AB)


def _problem(g, c, model):
    Q, R, Qf, xl, xu, ul, uu = c.data
    return g.mpc.ltvMpc.fromModel(model, g.pytrees.Trajectory(*c.plan), Q, R, xl, xu, ul, uu, Qf=Qf)


def loop(g, prob, model, x0, steps, plan, plant=None, disturbance=None, clip_tol=1e-6, xRef=None, uRef=None, each=None, **opts):
    """the loop of public calls that realTimeIteration replaces (its docstring), on NumPy arrays; each(s): called after step s's solve"""
    N = prob.N
    W = opts.pop("warm_start", "shift")
    xl, xu = prob.x_lb[..., :prob._n_user], prob.x_ub[..., :prob._n_user]
    clip = (lambda v: v) if clip_tol is None else (lambda v: np.minimum(np.maximum(v, xl + clip_tol), xu - clip_tol))
    x = np.array(x0, dtype=np.float64)
    out = SimpleNamespace(xTraj=[], uTraj=[], status=[], iterations=[], px=[], pu=[])
    for s in range(steps):
        x = clip(x)
        out.xTraj.append(x)
        prob.relinearize(model, plan)
        ref = {}
        if xRef is not None:
            ref["xRef"] = xRef[:, s:s + N + 1]
        if uRef is not None:
            ref["uRef"] = uRef[:, s:s + N]
        u, traj, status = prob.solve(x, warm_start=(False if s == 0 else W), **ref, **opts)
        out.uTraj.append(u)
        out.status.append(np.asarray(status, dtype=str))
        out.iterations.append(prob.last_iterations.copy())
        out.px.append(traj.xTraj)
        out.pu.append(traj.uTraj)
        if each is not None:
            each(s)
        x = g.mpc.modelStep(plant or model, x, u)
        if disturbance is not None:
            x = x + disturbance[:, s]
        plan = g.pytrees.Trajectory(np.concatenate([traj.xTraj[:, 1:], traj.xTraj[:, -1:]], axis=1),
                                    np.concatenate([traj.uTraj[:, 1:], traj.uTraj[:, -1:]], axis=1))
    out.xTraj.append(clip(x))
    for k in ("xTraj", "uTraj", "status", "iterations", "px", "pu"):
        setattr(out, k, np.stack(getattr(out, k), axis=1))
    return out


def _arrays(run):
    return SimpleNamespace(xTraj=np.asarray(run.xTraj), uTraj=np.asarray(run.uTraj), status=np.asarray(run.status, dtype=str),
                           iterations=np.asarray(run.iterations), px=np.asarray(run.predictions.xTraj), pu=np.asarray(run.predictions.uTraj))


def _same_bits(got, ref, what):
    for k in ("status", "iterations", "xTraj", "uTraj", "px", "pu"):
        a, b = getattr(got, k), getattr(ref, k)
        assert a.shape == b.shape, (what, k, a.shape, b.shape)
        assert np.array_equal(a, b), (what, k, np.argwhere(a != b)[:4].tolist())


# 1. relinearise -------------------------------------------------------------------------------------------------------------------------
RELIN = ["quad", "rigid_body", "embedded", "linear12"]


def _expected(c):
    out = [zo.affine_dynamics_from_trajectory(c.step, zo.Trajectory(c.plan[0][b], c.plan[1][b])) for b in range(c.nb)]
    return tuple(np.stack([np.asarray(o[i]) for o in out]) for i in range(3))


@pytest.mark.parametrize("name", RELIN)
def test_relinearize_writes_the_expansion_into_the_problem_arrays(gpu, name):
    """zm_mpc_relinearize_f64 into arrays filled with a sentinel: A_k, B_k against the oracle's complex-step expansion to the
    1e-12 max(1, |ref|) of tests/test_quad_derivs.py; c_k against f - f_x xbar - f_u ubar in float64 NumPy on the kernel's own f_x, f_u and
    the step function's f, row-wise within k eps (|f| + |f_x||xbar| + |f_u||ubar|), k = n + m + 2 (the n + m terms of the sum, the
    rounding of f and of the reference's own sum); everything outside the leading blocks keeps the sentinel's bits"""
    torch = gpu.torch
    c = _case(name)
    nb, N = c.nb, c.N
    n, m = c.plan[0].shape[-1], c.plan[1].shape[-1]
    ns, mc_ = (4, 2) if name == "embedded" else (n, m)
    model = _model(gpu, c)
    dev = dict(dtype=torch.float64, device="cuda")
    xP, uP = torch.as_tensor(c.plan[0], **dev).contiguous(), torch.as_tensor(c.plan[1], **dev).contiguous()
    sentinel = -7.25e100
    A, B, ck = (torch.full(s, sentinel, **dev) for s in ((nb, N, ns, ns), (nb, N, ns, mc_), (nb, N, ns)))
    cs = model.c_struct()
    rc = gpu.lib.lib().zm_mpc_relinearize_f64(ctypes.addressof(cs), xP.data_ptr(), uP.data_ptr(), A.data_ptr(), B.data_ptr(), ck.data_ptr(),
                                              nb, N, n, m, ns, mc_, None)
    assert rc == 0, gpu.lib.lib().zm_last_error()
    torch.cuda.synchronize()
    A, B, ck = A.cpu().numpy(), B.cpu().numpy(), ck.cpu().numpy()
    f, f_x, f_u = _expected(c)
    for got, ref in ((A[..., :n, :n], f_x), (B[..., :n, :m], f_u)):
        assert np.max(np.abs(got - ref)) <= 1e-12 * max(1.0, np.max(np.abs(ref)))
    pad = np.ones(A.shape, bool), np.ones(B.shape, bool), np.ones(ck.shape, bool)
    pad[0][..., :n, :n], pad[1][..., :n, :m], pad[2][..., :n] = False, False, False
    for X, p in zip((A, B, ck), pad):
        assert np.all(X[p].view(np.int64) == np.float64(sentinel).view(np.int64))
    fs = gpu.mpc.modelStep(model, c.plan[0][:, :-1], c.plan[1])
    assert np.max(np.abs(fs - f)) <= 1e-13 * max(1.0, np.max(np.abs(f)))
    xb, ub = c.plan[0][:, :-1], c.plan[1]
    want = fs - np.einsum("bkij,bkj->bki", A[..., :n, :n], xb) - np.einsum("bkij,bkj->bki", B[..., :n, :m], ub)
    bound = (n + m + 2) * np.finfo(float).eps * (np.abs(fs) + np.einsum("bkij,bkj->bki", np.abs(A[..., :n, :n]), np.abs(xb))
                                                 + np.einsum("bkij,bkj->bki", np.abs(B[..., :n, :m]), np.abs(ub)))
    dev_c = np.abs(ck[..., :n] - want)
    worst = np.max(dev_c[bound > 0] / bound[bound > 0])
    print(f"{name}: c_k deviates by at most {worst:.3f} of its bound")
    assert np.all(dev_c <= bound)            # (a row whose every term is zero has the bound 0 and must be exactly zero)
    if c.kind == "linear":
        assert np.max(np.abs(ck[..., :n])) <= np.max(bound)


@pytest.mark.parametrize("name", RELIN)
def test_relinearize_is_update_with_the_same_arrays(gpu, name):
    """after relinearize, solve gives the bits that update(A=f_x, B=f_u, c=c) gives with the device arrays read back and handed in; the
    host attributes stay as they were; fromModel is the constructor on the same expansion"""
    c = _case(name)
    model = _model(gpu, c)
    prob, prob2 = _problem(gpu, c, model), _problem(gpu, c, model)
    n, m = prob._n_user, prob._m_user
    f, f_x, f_u = _expected(c)
    assert prob.P == (c.nb,) and prob.N == c.N
    assert np.max(np.abs(prob.A[..., :n, :n] - f_x)) <= 1e-12 * max(1.0, np.max(np.abs(f_x)))
    rng = np.random.default_rng(1)
    plan = gpu.pytrees.Trajectory(c.plan[0] + 0.05 * rng.standard_normal(c.plan[0].shape), c.plan[1] + 0.02 * rng.standard_normal(c.plan[1].shape))
    hostA = prob.A.copy()
    a = prob.solve(c.x0, xRef=c.xRef[:, :c.N + 1], uRef=c.uRef[:, :c.N], **DEMO)
    prob.relinearize(model, plan)
    assert np.array_equal(prob.A, hostA)
    d = prob._device_data()
    A, B, ck = (d[k].cpu().numpy() for k in ("A", "B", "c"))
    moved = np.max(np.abs(A - prob2._device_data()["A"].cpu().numpy()))
    if c.kind == "linear":   # (a linear model's A_k, B_k are the model's wherever it is expanded; only the rounding-level c_k moves)
        assert moved <= 1e-12 * max(1.0, np.max(np.abs(A)))
    else:
        assert moved > 1e-4, "the new plan changes nothing: the test shows nothing"
    prob2.solve(c.x0, xRef=c.xRef[:, :c.N + 1], uRef=c.uRef[:, :c.N], **DEMO)
    prob2.update(A=A[..., :n, :n], B=B[..., :n, :m], c=ck[..., :n])
    for p in (prob, prob2):
        p.res = p.solve(c.x0, xRef=c.xRef[:, :c.N + 1], uRef=c.uRef[:, :c.N], warm_start=True, **DEMO)
    assert np.array_equal(prob.res[1].xTraj, prob2.res[1].xTraj) and np.array_equal(prob.res[1].uTraj, prob2.res[1].uTraj)
    assert np.array_equal(np.asarray(prob.res[2], dtype=str), np.asarray(prob2.res[2], dtype=str))
    assert np.array_equal(prob.last_iterations, prob2.last_iterations) and np.array_equal(prob.last_residuals, prob2.last_residuals)
    assert c.kind == "linear" or not np.array_equal(a[1].uTraj, prob.res[1].uTraj)
    # a device plan is read in place and gives the same bits
    torch = gpu.torch
    prob.relinearize(model, gpu.pytrees.Trajectory(torch.as_tensor(plan.xTraj, device="cuda"), torch.as_tensor(plan.uTraj, device="cuda")))
    assert np.array_equal(prob._device_data()["A"].cpu().numpy(), A) and np.array_equal(prob._device_data()["c"].cpu().numpy(), ck)


# 2. the one call is the loop of public calls, bit for bit -------------------------------------------------------------------------------
def _dist(c, S, scale, seed=4):
    return scale * np.random.default_rng(seed).standard_normal((c.nb, S, c.plan[0].shape[-1]))


def _cap_disturbance(c, S):
    w = np.zeros((c.nb, S, 12))
    w[2, 0, 0:3], w[2, 0, 6] = 0.5, 0.2
    return w


BITS = {
    "quad-shift-adaptive": ("quad", dict(warm_start="shift")),
    "quad-warm": ("quad", dict(warm_start=True)),
    "quad-fixed-penalty": ("quad", dict(adaptive_rho=False)),
    "quad-wind-disturbance": ("quad", dict(wind=(3.0, 1.0, 0.0), disturbance=lambda c, S: _dist(c, S, 0.02))),
    "quad-no-clip": ("quad", dict(clip_tol=None, disturbance=lambda c, S: _dist(c, S, 0.1))),
    "quad-no-plan-no-xref": ("quad", dict(plan=None, xRef=None)),
    "rigid-body": ("rigid_body", {}),
    "embedded-3-2": ("embedded", dict(eps_abs=1e-6, eps_rel=1e-6)),
    "N75": ("N75", {}),
    "iteration-cap": ("quad", dict(eps_abs=1e-6, eps_rel=1e-6, max_iter=30, disturbance=_cap_disturbance)),
}


@pytest.mark.parametrize("key", list(BITS))
def test_one_call_is_the_loop_of_public_calls_bit_for_bit(gpu, key):
    """xTraj, uTraj, status, iterations and the predictions of every step; afterwards the warm-start state, last_iterations,
    last_residuals, the device dynamics, and a further warm solve on both objects"""
    name, kw = BITS[key]
    kw = dict(kw)
    c = _case(name)
    S = c.S
    model = _model(gpu, c)
    wind = kw.pop("wind", None)
    plant = _model(gpu, c, wind) if wind else None
    prob, prob2 = _problem(gpu, c, model), _problem(gpu, c, model)
    dist = kw.pop("disturbance", None)
    dist = None if dist is None else dist(c, S)
    refs = dict(xRef=kw.pop("xRef", c.xRef), uRef=c.uRef)
    clip_tol = kw.pop("clip_tol", 1e-6)
    no_plan = "plan" in kw and kw.pop("plan") is None
    opts = {**DEMO, **kw}
    plan = gpu.pytrees.Trajectory(*c.plan)
    if no_plan:   # the documented default: the clipped x0 at every stage, the first N rows of uRef as inputs
        x0c = c.x0 if clip_tol is None else np.minimum(np.maximum(c.x0, c.data[3] + clip_tol), c.data[4] - clip_tol)
        held = gpu.pytrees.Trajectory(np.repeat(x0c[:, None, :], c.N + 1, axis=1), c.uRef[:, :c.N].copy())
    ref = loop(gpu, prob2, model, c.x0, S, held if no_plan else plan, plant=plant, disturbance=dist, clip_tol=clip_tol, **refs, **opts)
    run = prob.realTimeIteration(model, c.x0, S, plan=None if no_plan else plan, plant=plant, disturbance=dist, clip_tol=clip_tol,
                                 return_predictions=True, **refs, **opts)
    got = _arrays(run)
    _same_bits(got, ref, key)
    st = ref.status
    print(f"{key}: iterations {ref.iterations.min()}..{ref.iterations.max()}, statuses {sorted(set(st.ravel().tolist()))}")
    if key == "iteration-cap":     # instance 2 is pushed at step 0: its step 1 hits the cap, and the step after it starts cold
        assert st[2, 1] in ("user_limit", "optimal_inaccurate") and "optimal" in set(st[:, 2:].ravel().tolist()), st.tolist()
        assert set(st[:, 0].tolist()) == {"optimal"}, st.tolist()
    elif key == "quad-no-clip":    # a state pushed out of its box is "infeasible" where it is solved from; the run goes on from its rollout
        assert set(st.ravel().tolist()) == {"optimal", "infeasible"}, st.tolist()
        assert np.any(np.abs(ref.xTraj[..., :8]) > c.data[4][:8]), "nothing ever left the box: clip_tol=None shows nothing"
    elif key != "N75":
        assert set(st.ravel().tolist()) == {"optimal"}, st.tolist()
    assert ref.iterations.max() > 1 and np.any(ref.uTraj[:, 0] != ref.uTraj[:, -1])
    # the objects afterwards
    for a, b in zip(mc.read_state(prob, c.nb, c.N), mc.read_state(prob2, c.nb, c.N)):
        assert np.array_equal(a, b)
    assert np.array_equal(prob.last_iterations, prob2.last_iterations) and np.array_equal(prob.last_residuals, prob2.last_residuals)
    assert np.array_equal(prob.last_iterations, got.iterations[:, -1])
    for k in ("A", "B", "c"):
        assert np.array_equal(prob._device_data()[k].cpu().numpy(), prob2._device_data()[k].cpu().numpy()), k
        assert np.array_equal(getattr(prob, k), getattr(prob2, k))
    x1 = got.xTraj[:, -1]
    last = dict(xRef=None if refs["xRef"] is None else refs["xRef"][:, S - 1:S + c.N], uRef=c.uRef[:, S - 1:S - 1 + c.N])
    res = [p.solve(x1, **{**last, **opts, "warm_start": True}) for p in (prob, prob2)]
    assert np.array_equal(res[0][1].xTraj, res[1][1].xTraj) and np.array_equal(res[0][1].uTraj, res[1][1].uTraj)
    assert np.array_equal(prob.last_iterations, prob2.last_iterations)
    # without the predictions: the same run
    again = _problem(gpu, c, model).realTimeIteration(model, c.x0, S, plan=None if no_plan else plan, plant=plant, disturbance=dist,
                                                      clip_tol=clip_tol, **refs, **opts)
    assert again.predictions is None
    assert np.array_equal(again.xTraj, got.xTraj) and np.array_equal(again.uTraj, got.uTraj) and np.array_equal(again.iterations, got.iterations)


# 3. against the NumPy restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(rr.CASES))
def test_against_the_numpy_restatement(gpu, name):
    """tight tolerance, shifted warm starts, adaptive penalty: every step's status, iteration count and final level; states, inputs and
    predictions to mc.TOL max(1, |ref|), the rule of tests/mpc_ltv_ref.py: compare"""
    c = rr.CASES[name]()
    ref = rr.reference(name)
    model = _model(gpu, c)
    prob, prob2 = _problem(gpu, c, model), _problem(gpu, c, model)
    plan = gpu.pytrees.Trajectory(*c.plan)
    run = _arrays(prob.realTimeIteration(model, c.x0, c.S, plan=plan, return_predictions=True, xRef=c.xRef, uRef=c.uRef, **rr.OPTS))
    levels = []
    loop(gpu, prob2, model, c.x0, c.S, plan, xRef=c.xRef, uRef=c.uRef, each=lambda s: levels.append(mc.read_state(prob2, c.nb, c.N)[2]), **rr.OPTS)
    levels = np.stack(levels, axis=1)
    assert np.array_equal(mc.read_state(prob, c.nb, c.N)[2], levels[:, -1])
    worst = 0.0
    for b, r in enumerate(ref):
        at = f"{name} instance {b}"
        assert run.status[b].tolist() == r.status, (at, run.status[b].tolist(), r.status, run.iterations[b].tolist(), r.iters)
        assert run.iterations[b].tolist() == r.iters, (at, run.iterations[b].tolist(), r.iters)
        assert levels[b].tolist() == r.level, (at, levels[b].tolist(), r.level)
        for got, want in ((run.xTraj[b], r.states), (run.uTraj[b], r.inputs), (run.px[b], r.px), (run.pu[b], r.pu)):
            dev = np.max(np.abs(got - want)) / (mc.TOL * max(1.0, np.max(np.abs(want))))
            worst = max(worst, dev)
            assert dev <= 1.0, (at, dev)
    print(f"{name}: largest deviation {worst:.3g} of the bound")


# 4. the C ABI refuses before it launches ---------------------------------------------------------------------------------------------------
def test_abi_refusals(gpu):
    lib = gpu.lib.lib()
    cs = gpu.models.QuadcopterEuler(0.1).c_struct()
    md, d = ctypes.addressof(cs), 0x1000      # (d: a pointer that is never dereferenced: every call below returns before a launch)

    def call(model=md, out=d, steps=2, xref=d, xrows=6, urows=5, batch=1, N=4, nu=12, mu=4, ns=12, mc_=4):
        return lib.zm_mpc_rti_f64(model, None, d, d, d, d, d, d, d, d, d, d, d, d, d, 7, 3, 5.0, 1.6, d, d, d, d, d, xref, d, xrows, urows, d, d,
                                  1e-4, 1e-4, 1e-4, 100, 2, steps, 1e-6, None, d, out, d, d, d, None, None, None, batch, N, nu, mu, ns, mc_, None)
    EINVAL, EUNSUP = gpu.lib.ZM_EINVAL, gpu.lib.ZM_EUNSUPPORTED
    assert call(batch=0) == 0
    assert call(out=None) == EINVAL and b"null pointer" in lib.zm_last_error()
    assert call(steps=0) == EINVAL and b"steps must be at least 1" in lib.zm_last_error()
    assert call(xrows=5) == EINVAL and b"steps + N rows" in lib.zm_last_error()
    assert call(urows=6) == EINVAL and b"steps + N rows" in lib.zm_last_error()
    assert call(ns=24, mc_=8) == EUNSUP and b"(n=24, m=8)" in lib.zm_last_error()
    assert call(N=76, xrows=78, urows=77) == EUNSUP and b"N=76" in lib.zm_last_error()
    assert call(model=None) == EINVAL and b"null model" in lib.zm_last_error()
    assert call(nu=8) == EINVAL and b"the model has (n=12, m=4)" in lib.zm_last_error()
    assert lib.zm_mpc_relinearize_f64(md, d, d, d, d, None, 1, 4, 12, 4, 12, 4, None) == EINVAL
    assert lib.zm_mpc_relinearize_f64(md, d, d, d, d, d, 1, 4, 12, 4, 24, 8, None) == EUNSUP
    assert lib.zm_mpc_relinearize_f64(md, d, d, d, d, d, 0, 4, 12, 4, 12, 4, None) == 0
    assert lib.zm_model_step_f64(md, d, d, None, 1, None) == EINVAL and lib.zm_model_step_f64(md, None, None, None, 0, None) == 0


def test_abi_refusals_behind_the_map_read_back(gpu):
    """The refusals that need a device, with the full message: the entries copy the instance -> problem map to the host before they
    launch anything, so the map is real device memory and every other pointer a dummy (tests/test_mpc_refusals.py: the argument sets,
    batch 4, N = 3, shape (2, 1); its rows end before the copy).  Nothing is launched."""
    from tests.test_mpc_refusals import BAT, CL, D, LTV, RTI, TRK, _args
    lib = gpu.lib.lib()
    EINVAL, EUNSUP = gpu.lib.ZM_EINVAL, gpu.lib.ZM_EUNSUPPORTED
    dmap = lambda *v: gpu.torch.tensor(v, dtype=gpu.torch.int32, device="cuda")
    past, swapped, fine = dmap(0, 1, 2, 1), dmap(0, 1, 3, 2), dmap(0, 1, 1, 0)
    for entry, over, rc, msg in (
            (BAT, dict(problem=past), EINVAL, "instance 2 maps to problem 2 outside [0, 2)"),
            (BAT, dict(problem=dmap(0, -1, 2, 1)), EINVAL, "instance 1 maps to problem -1 outside [0, 2)"),
            (TRK, dict(problem=past, rho_p=D, P=2), EINVAL, "instance 2 maps to problem 2 outside [0, 2)"),
            (LTV, dict(problem=past, P=2), EINVAL, "instance 2 maps to problem 2 outside [0, 2)"),
            (CL, dict(problem=past, rho_p=D, P=2), EINVAL, "instance 2 maps to problem 2 outside [0, 2)"),
            (RTI, dict(problem=swapped), EINVAL, "instance 2 maps to problem 3; every instance is its own problem here"),
            # (the shape is looked up after the map is read, the horizon of zm_mpc_solve_ltv_f64 before)
            (BAT, dict(problem=fine, n=3, m=3), EUNSUP, "(n=3, m=3) not among the compiled shapes"),
            (BAT, dict(problem=past, n=3, m=3), EINVAL, "instance 2 maps to problem 2 outside [0, 2)"),
            (LTV, dict(problem=past, P=2, N=76), EUNSUP, "N=76 beyond the horizons whose iterates fit LDS (N <= 75)")):
        args = _args(entry, {k: v.data_ptr() if hasattr(v, "data_ptr") else v for k, v in over.items()})
        assert getattr(lib, entry)(*args) == rc, (entry, over)
        assert lib.zm_last_error().decode() == f"{entry}: {msg}"


# 5. streams -----------------------------------------------------------------------------------------------------------------------------
def test_a_side_stream_gives_the_same_bits(gpu):
    torch = gpu.torch
    c = _case("quad")
    model = _model(gpu, c)
    plan = gpu.pytrees.Trajectory(*c.plan)
    kw = dict(plan=plan, return_predictions=True, xRef=c.xRef, uRef=c.uRef, **DEMO)
    ref = _arrays(_problem(gpu, c, model).realTimeIteration(model, c.x0, c.S, **kw))
    prob = _problem(gpu, c, model)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        run = prob.realTimeIteration(model, c.x0, c.S, **kw)
    side.synchronize()
    _same_bits(_arrays(run), ref, "side stream")
