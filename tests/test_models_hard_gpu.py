"""Every evaluator of the registered quadcopter models on the device against the long-double reference of tests/model_hp_ref.py, on
its hard point families: many-turn angles, quadrant boundaries, gimbal lock, badly scaled states, large winds, zeros.

Evaluators: zm_linearize_dynamics_f64 (12-state closed forms, still air and wind, dt = 0 and dt != 0; the 8-state model on dual numbers
with body wind; the listed form with an id list that skips trajectories), zm_quadratic_dynamics_f64 on hyper-dual numbers for both
models, zm_quadratic_dynamics_pairs_list_f64 (the packed pairs; every undeclared pair exactly zero), zm_mpc_relinearize_f64 (A_k,
B_k, c_k), zm_model_step_f64, short rollouts (fast one-lane and four-lane kernels, the generic kernel, the wind model) and one long
spinning rollout.  The packed Jacobian image and the one-lane / 16-lane expansion kernels of the solvers have no entry point of
their own: tests/test_expand_forms_hard_gpu.py runs them on the same families through one iteration of the solvers, and
tests/test_models_hard.py holds their formulas to the families on the host.

Shapes: batch x horizon of (1, 1), (3, 1), (1, 17), (67, 1) -- 1, 3, 17 and 67 points, none of which fills a 16-lane group times
four or a wave; the 88 points of a family are dealt over them, so every point runs through every evaluator.

Metric: the error of output row i (the derivatives of xDot_i, or its value) over max(1, largest |reference entry| of the row); for
values and c_k over the row's largest |term|.  Bound: per family and output, 100 x the fp64 oracle's own worst error in that
metric on the same points (complex-step Jacobians, autograd second derivatives, oracle rollouts), floor 100 x 2^-52 = 2.2e-14;
computed at test time on the CPU, never from a kernel.  With wind the oracle has no second derivatives: the bound is the one
measured on the still-air evaluation of the same points.  Rollouts: per trajectory and per prefix of steps (RolloutCase).
A NaN or inf is allowed only where the reference itself is not finite in fp64.

Oracle errors -> bounds in force, 12-state model (the 8-state model's are of the same order: model_hp_ref.bounds_table("rigid")):

    family           dt    values             Jacobians          c_k                second derivatives
    nominal          0     3.9e-16 -> 3.9e-14   5.0e-16 -> 5.0e-14   1.7e-15 -> 1.7e-13   5.0e-16 -> 5.0e-14
    nominal          0.1   3.1e-16 -> 3.1e-14   4.3e-16 -> 4.3e-14   4.7e-16 -> 4.7e-14   5.5e-16 -> 5.5e-14
    many_turns       0     5.2e-16 -> 5.2e-14   6.7e-16 -> 6.7e-14   5.1e-15 -> 5.1e-13   5.6e-16 -> 5.6e-14
    many_turns       0.1   3.5e-16 -> 3.5e-14   3.6e-16 -> 3.6e-14   7.9e-16 -> 7.9e-14   5.8e-16 -> 5.8e-14
    quadrants        0     3.8e-16 -> 3.8e-14   5.4e-16 -> 5.4e-14   1.3e-15 -> 1.3e-13   4.8e-16 -> 4.8e-14
    quadrants        0.1   4.1e-16 -> 4.1e-14   5.9e-16 -> 5.9e-14   8.1e-16 -> 8.1e-14   4.4e-16 -> 4.4e-14
    gimbal           0     4.3e-16 -> 4.3e-14   3.4e-15 -> 3.4e-13   3.4e-15 -> 3.4e-13   2.5e-15 -> 2.5e-13
    gimbal           0.1   4.2e-16 -> 4.2e-14   3.4e-15 -> 3.4e-13   3.6e-15 -> 3.6e-13   2.4e-15 -> 2.4e-13
    scaled           0     3.7e-16 -> 3.7e-14   7.4e-16 -> 7.4e-14   7.7e-16 -> 7.7e-14   5.7e-16 -> 5.7e-14
    scaled           0.1   4.1e-16 -> 4.1e-14   4.8e-16 -> 4.8e-14   8.8e-16 -> 8.8e-14   6.2e-16 -> 6.2e-14
    zeros            0     2.4e-16 -> 2.4e-14   2.4e-16 -> 2.4e-14   2.9e-16 -> 2.9e-14   3.4e-16 -> 3.4e-14
    zeros            0.1   2.4e-16 -> 2.4e-14   1.5e-16 -> 2.2e-14   2.8e-16 -> 2.8e-14   2.1e-16 -> 2.2e-14
    nominal+wind     0     5.8e-16 -> 5.8e-14   5.0e-16 -> 5.0e-14   1.7e-15 -> 1.7e-13   (still air) 5.0e-14
    nominal+wind     0.1   3.0e-16 -> 3.0e-14   4.3e-16 -> 4.3e-14   5.2e-16 -> 5.2e-14   (still air) 5.5e-14
    many_turns+wind  0     1.2e-15 -> 1.2e-13   2.2e-15 -> 2.2e-13   5.1e-15 -> 5.1e-13   (still air) 5.6e-14
    many_turns+wind  0.1   6.7e-16 -> 6.7e-14   8.9e-16 -> 8.9e-14   3.0e-15 -> 3.0e-13   (still air) 5.8e-14
    gimbal+wind      0     7.5e-16 -> 7.5e-14   3.4e-15 -> 3.4e-13   3.4e-15 -> 3.4e-13   (still air) 2.5e-13
    gimbal+wind      0.1   8.3e-16 -> 8.3e-14   3.4e-15 -> 3.4e-13   3.6e-15 -> 3.6e-13   (still air) 2.4e-13

    rollouts (dt = 0.1, N = 7; oracle error over the determined (trajectory, prefix) pairs): nominal 1.2e-15, many_turns 4.5e-10 (an
    angle of 6e5 rad moves by ulps of 1e-10), quadrants 2.9e-8 (81 of 119 determined), gimbal 7.8e-5 (89 of 119), scaled 1.6e-5
    (117 of 119), zeros 3.5e-16; long spinning rollout: oracle 2.2e-14 -> bound 2.2e-12.
(model_hp_ref.bounds_table() prints the table.)"""
import ctypes

import numpy as np
import pytest

from tests import model_hp_ref as hp

pytestmark = pytest.mark.gpu
CASE_IDS = [hp.case_id(c) for c in hp.CASES]
SHAPES = [(1, 1), (3, 1), (1, 17), (67, 1)]                   # (batch, horizon): 1 + 3 + 17 + 67 = the 88 points of a family
DTS = [0.0, 0.1]


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available()
    from zopt_amd import _lib, ilqrUtils, models, mpcUtils, pytrees

    class G:
        pass
    g = G()
    g.torch, g.lib, g.models, g.mpc, g.ilqr, g.pt = torch, _lib, models, mpcUtils, ilqrUtils, pytrees
    return g


def _model(gpu, c):
    if c.kind == "inertial":
        return gpu.models.QuadcopterEuler(c.dt, wind_ned=c.w)
    return gpu.models.QuadcopterRigidBody(c.dt, wind_body=c.w)


def _deal(c):
    """the case's points dealt over SHAPES: (batch, horizon, slice of the points, xTraj (b, N + 1, n), uTraj (b, N, 4)); the state
    after the last step is not an expansion point (a copy of the last one)"""
    off = 0
    for b, N in SHAPES:
        sl = slice(off, off + b * N)
        off += b * N
        x = c.x[sl].reshape(b, N, c.n)
        yield b, N, sl, np.concatenate([x, x[:, -1:]], axis=1), c.u[sl].reshape(b, N, 4)
    assert off == hp.NPOINTS


def _dev(gpu, a, dtype=None):
    return gpu.torch.as_tensor(np.ascontiguousarray(a), device="cuda") if dtype is None else \
        gpu.torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device="cuda")


def _nan(gpu, *shape):
    return gpu.torch.full(shape, float("nan"), dtype=gpu.torch.float64, device="cuda")


def _linearize(gpu, model, xT, uT, lst=None):
    b, N, n = xT.shape[0], uT.shape[1], xT.shape[2]
    md = model.c_struct()
    dx, du = _dev(gpu, xT), _dev(gpu, uT)
    f, fx, fu = _nan(gpu, b, N, n), _nan(gpu, b, N, n, n), _nan(gpu, b, N, n, 4)
    lib = gpu.lib.lib()
    if lst is None:
        rc = lib.zm_linearize_dynamics_f64(ctypes.addressof(md), dx.data_ptr(), du.data_ptr(), None, f.data_ptr(), fx.data_ptr(),
                                           fu.data_ptr(), b, N, None)
    else:
        dl = _dev(gpu, lst, np.int32)
        rc = lib.zm_linearize_dynamics_list_f64(ctypes.addressof(md), dx.data_ptr(), du.data_ptr(), dl.data_ptr(), len(lst), None,
                                                f.data_ptr(), fx.data_ptr(), fu.data_ptr(), b, N, None)
    gpu.lib.check(rc, "linearize")
    gpu.torch.cuda.synchronize()
    return f.cpu().numpy(), np.concatenate([fx.cpu().numpy(), fu.cpu().numpy()], axis=-1)


def _check_expansion(c, sl, f, F, what):
    f, F = f.reshape(-1, c.n), F.reshape(-1, c.n, c.n + 4)
    assert hp.finite_where_reference_is(f, c.f[sl]) and hp.finite_where_reference_is(F, c.F[sl]), what
    ef = hp.row_error(f[:, :, None], c.f[sl][:, :, None], c.fscale[sl])
    eF = hp.row_error(F, c.F[sl])
    print(f"{what}: values {ef:.2e} (bound {c.b_f:.2e})  Jacobians {eF:.2e} (bound {c.b_F:.2e})")
    assert ef <= c.b_f and eF <= c.b_F, what


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kind", ["inertial", "rigid"])
@pytest.mark.parametrize("case", hp.CASES, ids=CASE_IDS)
def test_linearize_dynamics(gpu, case, kind, dt):
    """zm_linearize_dynamics_f64: the 12-state closed forms (still air / wind) and the 8-state model on dual numbers (body wind)"""
    c = hp.expansion_case(kind, case[0], case[1], dt)
    for b, N, sl, xT, uT in _deal(c):
        f, F = _linearize(gpu, _model(gpu, c), xT, uT)
        _check_expansion(c, sl, f, F, f"{kind} {hp.case_id(case)} dt={dt} ({b}, {N})")


@pytest.mark.parametrize("kind", ["inertial", "rigid"])
@pytest.mark.parametrize("case", hp.CASES, ids=CASE_IDS)
def test_linearize_dynamics_listed(gpu, case, kind):
    """the _list form: 20 trajectories of one step, 17 listed in a shuffled order, 3 skipped -- their rows keep the sentinel"""
    c = hp.expansion_case(kind, case[0], case[1], 0.1)
    sl = slice(4, 21)
    lst = np.array([7, 0, 18, 2, 16, 5, 1, 12, 9, 10, 17, 4, 13, 6, 14, 15, 8])      # not 3, 11, 19
    xT, uT = np.zeros((20, 2, c.n)), np.tile(hp.U_TRIM, (20, 1, 1))
    xT[lst, 0], xT[lst, 1], uT[lst, 0] = c.x[sl], c.x[sl], c.u[sl]
    f, F = _linearize(gpu, _model(gpu, c), xT, uT, lst)
    _check_expansion(c, sl, f[lst], F[lst], f"{kind} {hp.case_id(case)} listed")
    assert np.all(np.isnan(f[[3, 11, 19]])) and np.all(np.isnan(F[[3, 11, 19]]))


def _quadratic(gpu, model, xT, uT):
    b, N, n = xT.shape[0], uT.shape[1], xT.shape[2]
    md = model.c_struct()
    dx, du = _dev(gpu, xT), _dev(gpu, uT)
    fxx, fux, fuu = _nan(gpu, b, N, n, n, n), _nan(gpu, b, N, n, 4, n), _nan(gpu, b, N, n, 4, 4)
    gpu.lib.check(gpu.lib.lib().zm_quadratic_dynamics_f64(ctypes.addressof(md), dx.data_ptr(), du.data_ptr(), None, fxx.data_ptr(),
                                                          fux.data_ptr(), fuu.data_ptr(), b, N, None), "quadratic")
    gpu.torch.cuda.synchronize()
    H = np.zeros((b * N, n, n + 4, n + 4))
    H[:, :, :n, :n] = fxx.cpu().numpy().reshape(-1, n, n, n)
    H[:, :, n:, :n] = fux.cpu().numpy().reshape(-1, n, 4, n)
    H[:, :, :n, n:] = np.swapaxes(H[:, :, n:, :n], -1, -2)
    H[:, :, n:, n:] = fuu.cpu().numpy().reshape(-1, n, 4, 4)
    return H


def _declared_mask():
    m = np.zeros((16, 16), bool)
    for ab in hp.PAIR_TABLE:
        m[ab >> 4, ab & 15] = m[ab & 15, ab >> 4] = True
    return m


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kind", ["inertial", "rigid"])
@pytest.mark.parametrize("case", hp.CASES, ids=CASE_IDS)
def test_quadratic_dynamics_full_tensors(gpu, case, kind, dt):
    """zm_quadratic_dynamics_f64 on hyper-dual numbers, both models; for the 12-state model every entry of an undeclared pair is
    exactly zero (a NaN from an evaluation at gimbal lock must not leak into them either)"""
    c = hp.expansion_case(kind, case[0], case[1], dt)
    for b, N, sl, xT, uT in _deal(c):
        H = _quadratic(gpu, _model(gpu, c), xT, uT)
        what = f"{kind} {hp.case_id(case)} dt={dt} ({b}, {N})"
        assert hp.finite_where_reference_is(H, c.H[sl]), what
        err = hp.row_error(H, c.H[sl])
        print(f"{what}: second derivatives {err:.2e} (bound {c.b_H:.2e})")
        assert err <= c.b_H, what
        if kind == "inertial":
            assert np.all(H[:, :, ~_declared_mask()] == 0.0), what


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", hp.CASES, ids=CASE_IDS)
def test_quadratic_dynamics_packed_pairs(gpu, case, dt):
    """zm_quadratic_dynamics_pairs_list_f64 (the closed forms, 28 declared pairs x 12 rows per point), whole batches and a list that
    skips trajectories; rows are scaled by the whole row of the reference tensor, as for the full tensors"""
    c = hp.expansion_case("inertial", case[0], case[1], dt)
    md = _model(gpu, c).c_struct()
    lib = gpu.lib.lib()
    pairs, npairs = (ctypes.c_int32 * 64)(), ctypes.c_int32(0)
    gpu.lib.check(lib.zm_model_hessian_pairs(ctypes.addressof(md), ctypes.addressof(pairs), ctypes.addressof(npairs)), "pairs")
    assert npairs.value == 28 and [pairs[2 * q] * 16 + pairs[2 * q + 1] for q in range(28)] == list(hp.PAIR_TABLE)

    def run(xT, uT, lst):
        b, N = xT.shape[0], uT.shape[1]
        dx, du, H = _dev(gpu, xT), _dev(gpu, uT), _nan(gpu, b, N, 28, 12)
        dl = None if lst is None else _dev(gpu, lst, np.int32)
        gpu.lib.check(lib.zm_quadratic_dynamics_pairs_list_f64(ctypes.addressof(md), dx.data_ptr(), du.data_ptr(),
                                                               None if dl is None else dl.data_ptr(), 0 if lst is None else len(lst),
                                                               None, H.data_ptr(), b, N, None), "packed pairs")
        gpu.torch.cuda.synchronize()
        return H.cpu().numpy()

    def check(H, sl, what):
        got = np.swapaxes(H.reshape(-1, 28, 12), 1, 2)
        ref = np.stack([c.H[sl][:, :, ab >> 4, ab & 15] for ab in hp.PAIR_TABLE], axis=2)
        scale = np.max(np.abs(c.H[sl].reshape(len(ref), 12, -1)), axis=2)
        assert hp.finite_where_reference_is(got, ref), what
        err = hp.row_error(got, ref, np.where(np.isfinite(scale), scale, 0))
        print(f"{what}: packed pairs {err:.2e} (bound {c.b_H:.2e})")
        assert err <= c.b_H, what

    for b, N, sl, xT, uT in _deal(c):
        check(run(xT, uT, None), sl, f"{hp.case_id(case)} dt={dt} ({b}, {N})")
    sl = slice(4, 21)
    lst = np.array([7, 0, 18, 2, 16, 5, 1, 12, 9, 10, 17, 4, 13, 6, 14, 15, 8])
    xT, uT = np.zeros((20, 2, 12)), np.tile(hp.U_TRIM, (20, 1, 1))
    xT[lst, 0], xT[lst, 1], uT[lst, 0] = c.x[sl], c.x[sl], c.u[sl]
    H = run(xT, uT, lst)
    check(H[lst], sl, f"{hp.case_id(case)} dt={dt} listed")
    assert np.all(np.isnan(H[[3, 11, 19]]))


@pytest.mark.parametrize("kind", ["inertial", "rigid"])
@pytest.mark.parametrize("case", hp.CASES, ids=CASE_IDS)
def test_relinearize_and_model_step(gpu, case, kind):
    """zm_mpc_relinearize_f64: A_k = f_x, B_k = f_u, c_k = f - f_x xbar - f_u ubar (it cancels at large states: scaled by its largest
    term); zm_model_step_f64 (mpcUtils.modelStep): the value alone"""
    c = hp.expansion_case(kind, case[0], case[1], 0.1)
    model, n = _model(gpu, c), c.n
    md = model.c_struct()
    for b, N, sl, xT, uT in _deal(c):
        dx, du = _dev(gpu, xT), _dev(gpu, uT)
        A, B, ck = _nan(gpu, b, N, n, n), _nan(gpu, b, N, n, 4), _nan(gpu, b, N, n)
        gpu.lib.check(gpu.lib.lib().zm_mpc_relinearize_f64(ctypes.addressof(md), dx.data_ptr(), du.data_ptr(), A.data_ptr(), B.data_ptr(),
                                                           ck.data_ptr(), b, N, n, 4, n, 4, None), "relinearize")
        gpu.torch.cuda.synchronize()
        F = np.concatenate([A.cpu().numpy(), B.cpu().numpy()], axis=-1).reshape(-1, n, n + 4)
        ck = ck.cpu().numpy().reshape(-1, n)
        what = f"{kind} {hp.case_id(case)} ({b}, {N})"
        assert hp.finite_where_reference_is(F, c.F[sl]) and hp.finite_where_reference_is(ck, c.c[sl]), what
        eF, ec = hp.row_error(F, c.F[sl]), hp.row_error(ck[:, :, None], c.c[sl][:, :, None], c.cscale[sl])
        xn = gpu.mpc.modelStep(model, c.x[sl], c.u[sl])
        assert hp.finite_where_reference_is(xn, c.f[sl]), what
        ef = hp.row_error(xn[:, :, None], c.f[sl][:, :, None], c.fscale[sl])
        print(f"{what}: A, B {eF:.2e} (bound {c.b_F:.2e})  c {ec:.2e} (bound {c.b_c:.2e})  step {ef:.2e} (bound {c.b_f:.2e})")
        assert eF <= c.b_F and ec <= c.b_c and ef <= c.b_f, what


def _rollout_abi(gpu, model, problem, n_alpha):
    """zm_rollout_linesearch_f64 with a cost: one step size (ROLLOUT_ALPHA) or the 16 of the line search; (xTraj, uTraj, idx)"""
    torch = gpu.torch
    x0, l, L, xp, up = problem
    b, N = l.shape[:2]
    rng = np.random.default_rng(3)
    if n_alpha == 16:     # diagonal weights: the winners are re-rolled by the four-lane kernel
        cost = gpu.models.QuadraticCost(np.diag(rng.uniform(0.5, 2.0, 12)), np.diag(rng.uniform(0.5, 2.0, 4)), np.diag(rng.uniform(5, 20, 12)))
        al = 0.5 ** np.arange(16)
    else:
        M = rng.standard_normal((12, 12))
        cost = gpu.models.QuadraticCost(M @ M.T / 12 + np.eye(12), np.eye(4), 10 * np.eye(12))
        al = np.array([hp.ROLLOUT_ALPHA])
    md, cs = model.c_struct(), cost.c_struct()
    dev = [_dev(gpu, X) for X in (x0, l, L, xp, up)]
    dal = _dev(gpu, al)
    xT, uT, J = _nan(gpu, b, N + 1, 12), _nan(gpu, b, N, 4), _nan(gpu, b)
    idx = torch.full((b,), -1, dtype=torch.int32, device="cuda")
    gpu.lib.check(gpu.lib.lib().zm_rollout_linesearch_f64(
        ctypes.addressof(md), ctypes.addressof(cs), *[t.data_ptr() for t in dev], dal.data_ptr(), n_alpha, None, xT.data_ptr(), uT.data_ptr(),
        J.data_ptr(), idx.data_ptr() if n_alpha == 16 else None, b, N, None), "rollout")
    torch.cuda.synchronize()
    return xT.cpu().numpy(), uT.cpu().numpy(), idx.cpu().numpy()


@pytest.mark.parametrize("N", [1, 2, 3, 7])
@pytest.mark.parametrize("fam", hp.FAMILIES)
def test_short_rollouts_from_hard_initial_states(gpu, fam, N):
    """trajectoryRollout from the first 17 points of the family (dt = 0.1): the generic lane-per-trajectory kernel (no cost), the fast
    kernel with one step size (one lane per rollout) and the 16-step-size line search with diagonal weights (winners other than
    alpha_0 re-rolled on four lanes; the reference is rolled out with each trajectory's winning step size -- the step size the
    kernel REPORTED: whether it is the right one, and whether J belongs to it, is held by tests/test_linesearch_hard_gpu.py)"""
    rc = hp.rollout_case(fam, N)
    assert rc.determined[:, 0].all()                   # every initial state is compared on its first step at least
    x0, l, L, xp, up = rc.problem
    model = gpu.models.QuadcopterEuler(hp.ROLLOUT_DT)
    traj = gpu.ilqr.trajectoryRollout(x0, model, gpu.pt.AffinePolicy(l, L), gpu.pt.Trajectory(xp, up), alpha=hp.ROLLOUT_ALPHA)
    for what, (xT, uT) in (("generic", (traj.xTraj, traj.uTraj)), ("fast, one lane", _rollout_abi(gpu, model, rc.problem, 1)[:2])):
        worst, finite = rc.worst(xT, uT)
        print(f"{fam} N={N} {what}: worst error / bound {worst:.3f}; {rc.summary()}")
        assert finite and worst <= 1.0, what
    xT, uT, idx = _rollout_abi(gpu, model, rc.problem, 16)
    assert np.all((idx >= 0) & (idx < 16)) and np.any(idx != 0)      # some winners are not alpha_0: the four-lane kernel re-rolled them
    rc16 = hp.RolloutCase(fam, N, alpha=0.5 ** idx)
    assert rc16.determined[:, 0].all()
    worst, finite = rc16.worst(xT, uT)
    print(f"{fam} N={N} line search (winners {sorted(set(idx.tolist()))}): worst error / bound {worst:.3f}; {rc16.summary()}")
    assert finite and worst <= 1.0


@pytest.mark.parametrize("N", [1, 2, 3, 7])
@pytest.mark.parametrize("fam", list(hp.WINDS))
def test_short_rollouts_with_wind(gpu, fam, N):
    rc = hp.rollout_case(fam, N, True)
    assert rc.determined[:, 0].all()
    x0, l, L, xp, up = rc.problem
    model = gpu.models.QuadcopterEuler(hp.ROLLOUT_DT, wind_ned=hp.WINDS[fam])
    traj = gpu.ilqr.trajectoryRollout(x0, model, gpu.pt.AffinePolicy(l, L), gpu.pt.Trajectory(xp, up), alpha=hp.ROLLOUT_ALPHA)
    worst, finite = rc.worst(traj.xTraj, traj.uTraj)
    print(f"{fam}+wind N={N}: worst error / bound {worst:.3f}; {rc.summary()}")
    assert finite and worst <= 1.0


def test_long_spinning_rollout(gpu):
    """N = 200, dt = 0.1, r = 50 rad/s held by mz = 0.05 r: psi passes 1e3 rad (model_hp_ref.spinning_problem), on the generic and
    the fast kernel, against the Euler recursion in long double; the bound is 100 x the oracle rollout's error against the same"""
    problem = x0, l, L, xp, up = hp.spinning_problem()
    xl, ul = hp.rollout(x0.astype(hp.LD), l, L, xp, up, 1.0, hp.euler_step_ld((0, 0, 0), 0.1))
    xo, _ = hp.rollout(x0, l, L, xp, up, 1.0, hp.euler_step_oracle((0, 0, 0), 0.1))
    assert float(xl[0, -1, 8]) > 1e3 and 0.1 < float(np.abs(xl[0, -1, :2]).max()) < 10.0
    e = hp.traj_error(xo, xl)
    model = gpu.models.QuadcopterEuler(0.1)
    traj = gpu.ilqr.trajectoryRollout(x0, model, gpu.pt.AffinePolicy(l, L), gpu.pt.Trajectory(xp, up), alpha=hp.ROLLOUT_ALPHA)
    xf, _, _ = _rollout_abi(gpu, model, problem, 1)
    for what, xT in (("generic", traj.xTraj), ("fast", xf)):
        err = hp.traj_error(xT, xl)
        print(f"spinning, {what}: {err:.2e} (oracle {e:.2e}, bound {hp.bound(e):.2e})")
        assert np.all(np.isfinite(xT)) and err <= hp.bound(e), what
