"""GPU checks of models.TracedModel: the interpreter's kernels (zopt_amd/csrc/traced.hip) behind modelStep, trajectoryRollout,
forwardPass2, the expansions and the fused iLQR / DDP solves.

Shapes: the smallest at which the kernels can go wrong -- models (1, 1), pendulum (2, 1), cart-pole (4, 1), car (4, 2), the traced
quadcopter (12, 4) and the 64-slot tape; batches 1, 3, 67, 130 (a partial 16-lane group, a partial wave, more than one workgroup);
horizons 1, 2, 7.

The value path is held bit for bit to the host build of the same interpreter (tests/tape_shim.cpp).  sqrt is held bit for bit too:
the (1, 1) model takes a square root, and the device's fp64 sqrt is correctly rounded.
"""
import functools

import numpy as np
import pytest

from oracle import zopt_oracle as zo
from tests import model_hp_ref as hp
from tests import tape_ref as R

pytestmark = pytest.mark.gpu
LD = np.longdouble
BATCHES = (1, 3, 67, 130)


@pytest.fixture(scope="module")
def mods():
    import torch
    assert torch.cuda.is_available()
    from zopt_amd import ilqrUtils, models, mpcUtils, pytrees
    return ilqrUtils, models, mpcUtils, pytrees


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return R.build(tmp_path_factory.mktemp("tape_shim"))


def _rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300)


@functools.lru_cache(maxsize=None)
def _model(name):
    from zopt_amd import models
    f, n, m = {"scalar11": (R.scalar11, 1, 1), "pendulum": (R.pendulum, 2, 1), "cartpole": (R.cartpole, 4, 1), "car": (R.car, 4, 2),
               "quadcopter": (zo.quad_euler_step(0.1), 12, 4), "wide64": (R.wide_live(62), 1, 1)}[name]
    return models.TracedModel(f, n, m)


MODELS = ("scalar11", "pendulum", "cartpole", "car", "quadcopter", "wide64")


def _points(n, m, b, specials=True):
    rng = np.random.default_rng([11, n, m, b])
    x, u = rng.standard_normal((b, n)) * 2.0, rng.standard_normal((b, m))
    x[b // 2:] += 2 * np.pi * rng.integers(-1000, 1001, (b - b // 2, n))          # many-turn angles
    if specials:
        for k, v in enumerate((np.nan, np.inf, -np.inf)):
            if k < b:
                x[k, k % n] = v
    return x, u


# ---- value path, bit for bit ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", BATCHES)
@pytest.mark.parametrize("name", MODELS)
def test_model_step_and_one_step_rollout_bit_for_bit(mods, host, name, b):
    ilqr, models, mpc, pt = mods
    md = _model(name)
    n, m = md.n, md.m
    x, u = _points(n, m, b)
    got = mpc.modelStep(md, x, u)
    want = R.host_step(host, md.tape, x, u)
    assert np.array_equal(got, want, equal_nan=True)
    assert np.isnan(want).any()
    # trajectoryRollout with a zero policy about a zero trajectory: u_0 = l_0; finite states (the policy multiplies L = 0 into x)
    for T in (1, 2):
        xf, uf = _points(n, m, b, specials=False)
        pol = pt.AffinePolicy(np.repeat(uf[:, None, :], T, 1), np.zeros((b, T, m, n)))
        traj = ilqr.trajectoryRollout(xf, md, pol, pt.Trajectory(np.zeros((b, T + 1, n)), np.zeros((b, T, m))), 1.0)
        assert np.array_equal(traj.xTraj[:, 0], xf)
        for k in range(T):
            assert np.array_equal(traj.xTraj[:, k + 1], R.host_step(host, md.tape, traj.xTraj[:, k], traj.uTraj[:, k]), equal_nan=True)
        assert np.array_equal(traj.uTraj[:, 0], uf + 0.0)


@pytest.mark.parametrize("b", BATCHES)
def test_parameters_shared_and_per_trajectory_bit_for_bit(mods, host, b):
    ilqr, models, mpc, pt = mods
    lengths = np.linspace(0.4, 2.5, b)[:, None]
    x, u = _points(2, 1, b)
    per = models.TracedModel(R.pendulum_p, 2, 1, params=lengths)
    assert np.array_equal(mpc.modelStep(per, x, u), R.host_step(host, per.tape, x, u, lengths), equal_nan=True)
    shared = models.TracedModel(R.pendulum_p, 2, 1, params=np.array([0.7]))             # one row, read with stride 0
    assert np.array_equal(mpc.modelStep(shared, x, u), R.host_step(host, shared.tape, x, u, np.array([[0.7]])), equal_nan=True)
    if b > 3:
        assert not np.array_equal(mpc.modelStep(per, x, u)[3:], mpc.modelStep(shared, x, u)[3:])


# ---- rollouts with gains and the 16-way line search -----------------------------------------------------------------------------------
def _cost_ld(Q, R_, Qf, xs, us):
    Q, R_, Qf = (np.asarray(M, dtype=LD) for M in (Q, R_, Qf))
    with np.errstate(all="ignore"):
        c = np.einsum("bki,ij,bkj->b", xs[:, :-1], Q, xs[:, :-1]) + np.einsum("bki,ij,bkj->b", us, R_, us)
        return c + np.einsum("bi,ij,bj->b", xs[:, -1], Qf, xs[:, -1])


@pytest.mark.parametrize("fam", ["nominal", "many_turns", "scaled"])
def test_rollouts_with_gains_and_line_search(mods, fam):
    """T = 7 on model_hp_ref's rollout problems through the traced quadcopter: trajectoryRollout at alpha = 0.5 by the per-prefix rule
    of RolloutCase; forwardPass2's 16 step sizes against long-double rollouts and costs -- the chosen index equals the reference's
    wherever the reference's two best costs differ by more than DETERMINED (relative to the best), and the winner's trajectory obeys
    the same rule at its step size."""
    ilqr, models, mpc, pt = mods
    md = _model("quadcopter")
    N = 7
    case = hp.rollout_case(fam, N)
    x0, l, L, xp, up = case.problem
    traj = ilqr.trajectoryRollout(x0, md, pt.AffinePolicy(l, L), pt.Trajectory(xp, up), hp.ROLLOUT_ALPHA)
    worst, finite = case.worst(traj.xTraj, traj.uTraj)
    print(f"{fam}: rollout worst error / bound {worst:.2e} ({case.summary()})")
    assert finite and worst <= 1.0
    w = np.linspace(0.5, 2.0, 12)
    w[6:9] = 0.0                                         # no weight on the angles: many turns would drown the step sizes' differences
    Q, R_, Qf = np.diag(w), 0.3 * np.eye(4), np.diag(4.0 * (w > 0))
    cost = models.QuadraticCost(Q, R_, Qf)
    lbig = 30.0 * l                                      # so that the step sizes differ in cost
    trj, J = ilqr.forwardPass2(x0, md, cost, pt.AffinePolicy(lbig, L), pt.Trajectory(xp, up))
    alphas = 0.5 ** np.arange(16)
    step_ld = hp.euler_step_ld((0.0, 0.0, 0.0), hp.ROLLOUT_DT)
    Jr = np.stack([_cost_ld(Q, R_, Qf, *hp.fp64_range(*hp.rollout(x0.astype(LD), lbig * a, L, xp, up, 1.0, step_ld))) for a in alphas], 1)
    # the step size forwardPass2 took, read off its first input: u_0 = alpha l_0 + L_0 (x_0 - xPrev_0) + uPrev_0
    u00 = trj.uTraj[:, 0, 0] - up[:, 0, 0] - np.einsum("bj,bj->b", L[:, 0, 0], x0 - xp[:, 0])
    got_idx = np.argmin(np.abs(alphas[None, :] * lbig[:, 0, 0, None] - u00[:, None]), axis=1)
    checked = 0
    for i in range(len(x0)):
        if not np.all(np.isfinite(Jr[i].astype(np.float64))):
            continue
        order = np.argsort(Jr[i], kind="stable")
        if Jr[i, order[1]] - Jr[i, order[0]] > hp.DETERMINED * abs(Jr[i, order[0]]):
            assert got_idx[i] == order[0], (fam, i, got_idx[i], order[:3])
            checked += 1
    print(f"{fam}: {checked} of {len(x0)} step-size choices determined and equal to the reference's")
    assert checked >= 1 or fam == "scaled"              # (velocities ~1e3: costs ~1e6, the step sizes' differences are below DETERMINED)
    # the winner's trajectory by the same per-prefix rule at the step size taken
    ls = lbig * alphas[got_idx][:, None, None]
    xr, ur = hp.fp64_range(*hp.rollout(x0.astype(LD), ls, L, xp, up, 1.0, step_ld))
    xo, uo = hp.rollout(x0, ls, L, xp, up, 1.0, hp.euler_step_oracle((0.0, 0.0, 0.0), hp.ROLLOUT_DT))
    e = hp.prefix_errors(xo, uo, xr, ur)
    det = np.minimum.accumulate((e <= hp.DETERMINED) & np.all(np.isfinite(xr[:, 1:].astype(np.float64)), axis=2), axis=1)
    det &= np.all(np.isfinite(Jr.astype(np.float64)), axis=1)[:, None]      # (a NaN cost wins: no reference step size there)
    ratio = np.where(det, hp.prefix_errors(trj.xTraj, trj.uTraj, xr, ur) / np.maximum(hp.FLOOR, 100.0 * e), 0.0)
    print(f"{fam}: winner's rollout worst error / bound {ratio.max():.2e} on {int(det.sum())}/{det.size} determined prefixes")
    assert ratio.max() <= 1.0


def test_line_search_nan_wins_and_first_index_wins_ties(mods):
    ilqr, models, mpc, pt = mods
    md = models.TracedModel(lambda x, u: np.array([0.5 * x[0] + np.sqrt(u[0] - 0.3)]), 1, 1)
    b, N = 3, 2
    x0 = np.array([[1.0], [2.0], [3.0]])
    l = np.ones((b, N, 1))                               # u = alpha: alpha <= 0.25 takes the root of a negative number
    pol, prev = pt.AffinePolicy(l, np.zeros((b, N, 1, 1))), pt.Trajectory(np.zeros((b, N + 1, 1)), np.zeros((b, N, 1)))
    traj, J = ilqr.forwardPass2(x0, md, models.QuadraticCost(np.eye(1), np.eye(1), np.eye(1)), pol, prev)
    assert np.all(np.isnan(J)) and np.array_equal(traj.uTraj[:, 0, 0], np.full(b, 0.25))       # the first NaN cost: index 2
    tie = models.TracedModel(lambda x, u: np.array([0.5 * x[0] + 0.0 * u[0]]), 1, 1)
    traj, J = ilqr.forwardPass2(x0, tie, models.QuadraticCost(np.eye(1), np.zeros((1, 1)), np.eye(1)), pol, prev)
    assert np.array_equal(traj.uTraj[:, 0, 0], np.ones(b))                                      # all 16 costs equal: index 0


# ---- expansions -------------------------------------------------------------------------------------------------------------------
def test_expansions_match_the_registered_quadcopter(mods):
    """the comparison tests/test_generic_gpu.py makes for the torch path, at its tolerance 1e-12; T = 1, 2, 7 and batches with a
    partial group / wave"""
    ilqr, models, mpc, pt = mods
    rng = np.random.default_rng(3)
    tm, reg = _model("quadcopter"), models.QuadcopterEuler(0.1)
    for b, N in ((1, 1), (3, 2), (67, 7), (130, 1)):
        xT = 0.3 * rng.standard_normal((b, N + 1, 12))
        uT = models.QuadcopterEuler.uTrim + 0.3 * rng.standard_normal((b, N, 4))
        traj = pt.Trajectory(xT, uT)
        a, q = pt.QuadraticDynamics.from_trajectory(tm, traj), pt.QuadraticDynamics.from_trajectory(reg, traj)
        for fa, fb in zip(tuple.__iter__(a), tuple.__iter__(q)):
            assert fa.shape == fb.shape and np.max(np.abs(fa - fb)) <= 1e-12
        a1, q1 = pt.AffineDynamics.from_trajectory(tm, traj), pt.AffineDynamics.from_trajectory(reg, traj)
        for fa, fb in zip(tuple.__iter__(a1), tuple.__iter__(q1)):
            assert np.max(np.abs(fa - fb)) <= 1e-12


@pytest.mark.parametrize("case", [("nominal", False), ("many_turns", False), ("gimbal", False), ("scaled", False), ("gimbal", True)],
                         ids=hp.case_id)
def test_expansions_on_the_hard_families(mods, case):
    """per output row against the long-double / sympy reference, bound(oracle_error) of model_hp_ref"""
    ilqr, models, mpc, pt = mods
    fam, windy = case
    c = hp.expansion_case("inertial", fam, windy, 0.1)
    w = np.array(c.w, dtype=np.float64)
    md = models.TracedModel(lambda x, u: x + 0.1 * zo.quad_inertialDynamics(x, u, wind_ned=w), 12, 4)
    q = pt.QuadraticDynamics.from_function(md, c.x, c.u)
    F = np.concatenate([q.f_x, q.f_u], -1)
    H = np.zeros((len(c.x), 12, 16, 16))
    H[:, :, :12, :12], H[:, :, 12:, :12], H[:, :, 12:, 12:] = q.f_xx, q.f_ux, q.f_uu
    H[:, :, :12, 12:] = np.swapaxes(q.f_ux, -1, -2)
    e_f, e_F, e_H = hp.row_error(q.f, c.f, c.fscale), hp.row_error(F, c.F), hp.row_error(H, c.H)
    print(f"{hp.case_id(case)}: values {e_f:.1e} ({c.b_f:.1e})  Jacobians {e_F:.1e} ({c.b_F:.1e})  second {e_H:.1e} ({c.b_H:.1e})")
    assert hp.finite_where_reference_is(q.f, c.f) and hp.finite_where_reference_is(F, c.F) and hp.finite_where_reference_is(H, c.H)
    assert e_f <= c.b_f and e_F <= c.b_F and e_H <= c.b_H


@pytest.mark.parametrize("name", ["car", "cartpole", "scalar11", "wide64"])
def test_expansions_of_control_nonlinear_models(mods, name):
    """first derivatives against long-double dual numbers on the tape, second against sympy derivatives of the same expression in long
    double (rows: 100 x 2^-52 of the row's largest entry, model_hp_ref's floor); f_ux, f_uu nonzero exactly where sympy's are.  The
    64-slot tape's Hyper slot file is the private-scratch one, the others' is in LDS."""
    ilqr, models, mpc, pt = mods
    md = _model(name)
    n, m = md.n, md.m
    f = md.f
    for b, N in ((3, 1), (67, 2), (5, 7)):
        rng = np.random.default_rng([5, n, b])
        xT, uT = rng.standard_normal((b, N + 1, n)), 0.4 * rng.standard_normal((b, N, m))
        q = pt.QuadraticDynamics.from_trajectory(md, pt.Trajectory(xT, uT))
        x, u = xT[:, :-1].reshape(-1, n), uT.reshape(-1, m)
        fl, Jl = R.jacobian(md.tape, x, u)
        F = np.concatenate([q.f_x, q.f_u], -1).reshape(-1, n, n + m)
        assert hp.row_error(F, Jl) <= hp.FLOOR and hp.row_error(q.f.reshape(-1, n), fl) <= hp.FLOOR
        Hs = R.sympy_hessian(f, n, m, x, u)
        H = np.zeros((len(x), n, n + m, n + m))
        H[:, :, :n, :n], H[:, :, n:, :n] = q.f_xx.reshape(-1, n, n, n), q.f_ux.reshape(-1, n, m, n)
        H[:, :, n:, n:], H[:, :, :n, n:] = q.f_uu.reshape(-1, n, m, m), np.swapaxes(q.f_ux.reshape(-1, n, m, n), -1, -2)
        assert hp.row_error(H, Hs) <= hp.FLOOR
        assert np.array_equal(H[:, :, n:, :] != 0, Hs[:, :, n:, :] != 0)
        if name == "car":
            assert np.any(q.f_ux != 0) and np.any(q.f_uu != 0)
        if name == "cartpole":
            assert np.any(q.f_ux != 0)


# ---- solves -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ddp", [False, True])
def test_quadcopter_solves_match_the_oracle_loop(mods, ddp):
    """tests/test_generic_gpu.py's three quadcopter problems (N = 25), same weights and tolerances, through the traced model"""
    ilqr, models, mpc, pt = mods
    N = 25
    Q, R_, Qf = np.eye(12), (0.2 if ddp else 1.0) * np.eye(4), 10 * np.eye(12)
    cost = models.QuadraticCost(Q, R_, Qf)
    x0 = np.zeros((3, 12))
    x0[:, 9:12] = [[0, 5, 0], [1, -2, 3], [-4, 1, 2]]
    ug = np.tile(models.QuadcopterEuler.uTrim, (3, N, 1))
    solve = ilqr.differentialDynamicProgramming if ddp else ilqr.iterativeLqr
    traj, L, J, conv = solve(_model("quadcopter"), cost, cost, x0, ug)
    fn = zo.quad_euler_step(0.1)
    for i in range(3):
        if ddp:
            rt, rL, rJ, rc = zo.differentialDynamicProgramming(fn, zo.quad_euler_step_torch(0.1), Q, R_, Qf, x0[i], ug[i])
        else:
            rt, rL, rJ, rc = zo.iterativeLqr(fn, Q, R_, Qf, x0[i], ug[i])
        assert bool(conv[i]) == rc and abs(J[i] - rJ) <= 1e-7 * abs(rJ)
        assert _rel(traj.xTraj[i], rt.xTraj) <= 1e-6 and _rel(traj.uTraj[i], rt.uTraj) <= 1e-6 and _rel(L[i], rL) <= 1e-5


def test_identity_kat(mods):
    """reference tests/test_ilqrUtils.py:167-196 (A = B = Q = R = I, N = 3, x0 = (2, 1)) written as lambda x, u: x + u"""
    ilqr, models, mpc, pt = mods
    I = np.eye(2)
    x0 = np.array([2.0, 1.0])
    md, cost = models.TracedModel(lambda x, u: x + u, 2, 2), models.QuadraticCost(I, I, I)
    assert md.tape.mask == 0
    for solver, ddp in ((ilqr.iterativeLqr, False), (ilqr.differentialDynamicProgramming, True)):
        traj, L, J, conv = solver(md, cost, cost, x0, np.zeros((3, 2)))
        assert conv is True and isinstance(J, float)
        if ddp:
            rt, rL, rJ, rc = zo.differentialDynamicProgramming(lambda x, u: x + u, lambda x, u: x + u, I, I, I, x0, np.zeros((3, 2)))
        else:
            rt, rL, rJ, rc = zo.iterativeLqr(lambda x, u: x + u, I, I, I, x0, np.zeros((3, 2)))
        assert rc and _rel(traj.uTraj, rt.uTraj) <= 1e-9 and _rel(L, rL) <= 1e-9 and J == pytest.approx(rJ, rel=1e-10)


def _pendulum_any(x, u):
    """the README's pendulum, one callable for NumPy recording scalars and torch tensors"""
    import torch
    sin = torch.sin if isinstance(x, torch.Tensor) else np.sin
    th, om = x[0], x[1]
    a, b = th + 0.05 * om, om + 0.05 * (u[0] - 9.81 * sin(th))
    return torch.stack([a, b]) if isinstance(x, torch.Tensor) else np.array([a, b])


@pytest.mark.parametrize("ddp", [False, True])
def test_pendulum_matches_the_generic_torch_path(mods, ddp):
    ilqr, models, mpc, pt = mods
    N = 7
    cost = models.QuadraticCost(np.diag([10.0, 1.0]), 0.1 * np.eye(1), np.diag([100.0, 10.0]))
    x0 = np.array([[0.5, 0.0], [-1.0, 0.3], [2.5, -1.0]])
    ug = np.zeros((3, N, 1))
    solve = ilqr.differentialDynamicProgramming if ddp else ilqr.iterativeLqr
    a = solve(models.TracedModel(_pendulum_any, 2, 1), cost, cost, x0, ug)
    g = solve(_pendulum_any, cost.runningCost, cost.terminalCost, x0, ug)
    for i in range(3):
        assert bool(a[3][i]) == bool(g[3][i]) and abs(a[2][i] - g[2][i]) <= 1e-7 * abs(g[2][i])
        assert _rel(a[0].xTraj[i], g[0].xTraj[i]) <= 1e-6 and _rel(a[0].uTraj[i], g[0].uTraj[i]) <= 1e-6 and _rel(a[1][i], g[1][i]) <= 1e-5


# ---- batch behaviour ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ddp", [False, True])
def test_batch_of_67_with_parameters_equals_the_single_solves_bit_for_bit(mods, ddp):
    """every instance of a batch with per-trajectory parameters equals its single-problem solve bit for bit: a trajectory's results
    depend on nothing but its own data, and one that has converged is not touched again while the others go on"""
    ilqr, models, mpc, pt = mods
    b, N = 67, 7
    rng = np.random.default_rng(67)
    lengths = rng.uniform(0.5, 2.0, (b, 1))
    x0 = np.stack([rng.uniform(-1.5, 1.5, b), rng.uniform(-1, 1, b)], 1)
    ug = np.zeros((b, N, 1))
    cost = models.QuadraticCost(np.diag([10.0, 1.0]), 0.1 * np.eye(1), np.diag([100.0, 10.0]))
    solve = ilqr.differentialDynamicProgramming if ddp else ilqr.iterativeLqr
    traj, L, J, conv = solve(models.TracedModel(R.pendulum_p, 2, 1, params=lengths), cost, cost, x0, ug, maxIter=30)
    assert conv.any()
    for i in range(b):
        ti, Li, Ji, ci = solve(models.TracedModel(R.pendulum_p, 2, 1, params=lengths[i]), cost, cost, x0[i], ug[i], maxIter=30)
        assert np.array_equal(ti.xTraj, traj.xTraj[i]) and np.array_equal(ti.uTraj, traj.uTraj[i]) and np.array_equal(Li, L[i])
        assert Ji == J[i] and ci == bool(conv[i])
