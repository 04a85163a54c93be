"""GPU checks of models.TracedCost: the kernels of zopt_amd/csrc/traced_cost.hip behind forwardPass2, cost(traj), the cost expansions
and the fused iLQR / DDP solves with a recorded cost (zm_traced_cost_*).

Shapes: the smallest at which the kernels can go wrong -- models (1, 1), pendulum (2, 1), car (4, 2), quadcopter (12, 4), registered and
traced; batches 1, 3, 67, 130 (a partial 16-lane group, a partial wave, more than one workgroup); horizons 1, 2, 7.

The value path is held bit for bit to the host build of the same interpreter (tests/tape_cost_shim.cpp, tests/tape_shim.cpp).
Derivative bound: tests/test_traced_cost.py's (the larger of model_hp_ref.FLOOR and 100 x the fp64 NumPy evaluation's own error).
"""
import ctypes
import functools
import warnings

import numpy as np
import pytest

from oracle import zopt_oracle as zo
from tests import model_hp_ref as hp
from tests import tape_ref as R
from tests import traced_cost_cases as C
from tests import traced_cost_ref as TR
from tests.test_traced_cost import case_quadratic_dynamics, wide_cost

pytestmark = pytest.mark.gpu
LD = np.longdouble
BATCHES = (1, 3, 67, 130)
ALPHAS = 0.5 ** np.arange(16)


@pytest.fixture(scope="module")
def mods():
    import torch
    assert torch.cuda.is_available()
    from zopt_amd import _lib, ilqrUtils, models, pytrees
    return ilqrUtils, models, pytrees, _lib


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("tape_cost_shim")
    return TR.build(d), R.build(d)


def _rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300)


def scalar_running(x, u):
    return np.sqrt(x[0] * x[0] + 1.0) + 0.5 * u[0] * u[0]


def scalar_terminal(x):
    return 3.0 * x[0] * x[0]


@functools.lru_cache(maxsize=None)
def _setup(name):
    """name -> (device model, NumPy step or None for a registered model, TracedModel twin or None, cost callables, n, m, n_params)"""
    from zopt_amd import models
    if name == "scalar11":
        md = models.TracedModel(R.scalar11, 1, 1)
        return md, md, scalar_running, scalar_terminal, 1, 1, 0
    if name == "linear21":              # a registered LinearModel under the pendulum's cost
        A, B = np.array([[1.0, 0.05], [-0.4, 0.98]]), np.array([[0.0], [0.05]])
        return models.LinearModel(A, B), None, C.pendulum_running, C.pendulum_terminal, 2, 1, 0
    if name == "pendulum":
        md = models.TracedModel(C.pendulum_any, 2, 1)
        return md, md, C.pendulum_running, C.pendulum_terminal, 2, 1, 0
    if name == "car":
        md = models.TracedModel(C.car_any, 4, 2)
        return md, md, C.car_running, C.car_terminal, 4, 2, 4
    if name == "quad_registered":
        return models.QuadcopterEuler(0.1), None, C.quad_running, C.quad_terminal, 12, 4, 0
    md = models.TracedModel(zo.quad_euler_step(0.1), 12, 4)
    return md, md, C.quad_running, C.quad_terminal, 12, 4, 0


SETUPS = ("scalar11", "linear21", "pendulum", "car", "quad_registered", "quad_traced")


def _problem(n, m, b, T, seed=0, specials=True, scale=1.0):
    rng = np.random.default_rng([21, n, m, b, T, seed])
    x0 = scale * rng.standard_normal((b, n))
    l, L = 0.5 * rng.standard_normal((b, T, m)), 0.1 * rng.standard_normal((b, T, m, n))
    xp, up = 0.3 * rng.standard_normal((b, T + 1, n)), 0.2 * rng.standard_normal((b, T, m))
    if m == 4:
        up[:, :, 0] += 9.807
    if specials:
        for k, v in enumerate((np.nan, np.inf, -np.inf)):
            if k + 1 < b:
                x0[k + 1, k % n] = v
    return x0, l, L, xp, up


def _params(npar, b):
    if not npar:
        return None
    rng = np.random.default_rng([4, b])
    p = rng.uniform(-3, 3, (b, npar))
    p[b // 2:] += 1e6                                    # goals 1e6 from the origin
    return p


# ---- line search: the value path, bit for bit -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", BATCHES)
@pytest.mark.parametrize("name", SETUPS)
def test_forward_pass_cost_and_steps_bit_for_bit(mods, host, name, b):
    """forwardPass2 and cost(traj): J of the returned trajectory equals the host interpreter's per-step costs summed in step order plus
    the terminal cost; x_{k+1} equals the host step of (x_k, u_k) for traced models; NaN and +-inf states included"""
    ilqr, models, pt, _ = mods
    hcost, hstep = host
    md, twin, run, term, n, m, npar = _setup(name)
    p = _params(npar, b)
    cost = models.TracedCost(run, term, n, m, params=p)
    for T in (1, 2, 7):
        x0, l, L, xp, up = _problem(n, m, b, T)
        traj, J = ilqr.forwardPass2(x0, md, cost, pt.AffinePolicy(l, L), pt.Trajectory(xp, up))
        want = TR.host_cost_of_trajectory(hcost, cost, traj.xTraj, traj.uTraj, p)
        assert np.array_equal(J, want, equal_nan=True), (name, b, T)
        assert np.array_equal(cost(traj), want, equal_nan=True)
        with np.errstate(all="ignore"):
            ck = cost(traj, 0)
        assert np.array_equal(ck, TR.host_value(hcost, cost.running_tape, traj.xTraj[:, 0], traj.uTraj[:, 0], p), equal_nan=True)
        assert np.array_equal(traj.xTraj[:, 0], x0, equal_nan=True)
        if twin is not None:
            for k in range(T):
                assert np.array_equal(traj.xTraj[:, k + 1], R.host_step(hstep, twin.tape, traj.xTraj[:, k], traj.uTraj[:, k]), equal_nan=True)
        if b > 3:
            assert np.isnan(want[1]) and np.isfinite(want[4:]).mean() > 0.9
        # the step size taken is one of the 16: u_0 = alpha l_0 + L_0 (x_0 - xPrev_0) + uPrev_0
        fin = np.isfinite(x0).all(1)
        u0 = ALPHAS[None, :, None] * l[fin, None, 0] + (np.einsum("bij,bj->bi", L[fin, 0], x0[fin] - xp[fin, 0]) + up[fin, 0])[:, None]
        assert np.all(np.min(np.max(np.abs(u0 - traj.uTraj[fin, None, 0]), axis=2), axis=1) <= 1e-12)


@pytest.mark.parametrize("name", ["pendulum", "car", "quad_registered"])
def test_chosen_step_against_long_double(mods, name):
    """T = 7, batch 17: the 16 costs in long double (rollouts of the tape / of model_hp_ref's quadcopter, the cost tapes on long
    double); the chosen index equals the reference's wherever its two best costs differ by more than DETERMINED, and the winner's
    trajectory obeys the per-prefix rule of tests/test_traced_model_gpu.py::test_rollouts_with_gains_and_line_search"""
    ilqr, models, pt, _ = mods
    md, twin, run, term, n, m, npar = _setup(name)
    b, T = 17, 7
    p = None if not npar else np.random.default_rng(8).uniform(-3, 3, (b, npar))
    cost = models.TracedCost(run, term, n, m, params=p)
    x0, l, L, xp, up = _problem(n, m, b, T, seed=1, specials=False)
    l = 4.0 * l                                          # so that the step sizes differ in cost
    if twin is None:
        step_ld, step_64 = hp.euler_step_ld((0.0, 0.0, 0.0), 0.1), hp.euler_step_oracle((0.0, 0.0, 0.0), 0.1)
    else:
        step_ld = lambda x, u: R.evaluate(twin.tape, x, u, num=R.Real(LD))              # noqa: E731
        step_64 = lambda x, u: R.evaluate(twin.tape, x, u)                               # noqa: E731
    trj, J = ilqr.forwardPass2(x0, md, cost, pt.AffinePolicy(l, L), pt.Trajectory(xp, up))

    def cost_ld(xs, us):
        J = np.zeros(b, dtype=LD)
        for k in range(T):
            J = J + TR.tape_value_ld(cost.running_tape, xs[:, k], us[:, k], p)
        return J + TR.tape_value_ld(cost.terminal_tape, xs[:, T], None, p)
    Jr = np.stack([cost_ld(*hp.rollout(x0.astype(LD), l * a, L, xp, up, 1.0, step_ld)) for a in ALPHAS], 1)
    u00 = trj.uTraj[:, 0, 0] - up[:, 0, 0] - np.einsum("bj,bj->b", L[:, 0, 0], x0 - xp[:, 0])
    got_idx = np.argmin(np.abs(ALPHAS[None, :] * l[:, 0, 0, None] - u00[:, None]), axis=1)
    checked = 0
    for i in range(b):
        order = np.argsort(Jr[i], kind="stable")
        if Jr[i, order[1]] - Jr[i, order[0]] > hp.DETERMINED * abs(Jr[i, order[0]]):
            assert got_idx[i] == order[0], (name, i, got_idx[i], order[:3])
            assert abs(J[i] - float(Jr[i, order[0]])) <= 1e-10 * abs(float(Jr[i, order[0]]))
            checked += 1
    print(f"{name}: {checked} of {b} step-size choices determined and equal to the reference's; indices {sorted(set(got_idx.tolist()))}")
    assert checked >= 1
    ls = l * ALPHAS[got_idx][:, None, None]
    xr, ur = hp.rollout(x0.astype(LD), ls, L, xp, up, 1.0, step_ld)
    xo, uo = hp.rollout(x0, ls, L, xp, up, 1.0, step_64)
    e = hp.prefix_errors(xo, uo, xr, ur)
    det = np.minimum.accumulate(e <= hp.DETERMINED, axis=1)
    ratio = np.where(det, hp.prefix_errors(trj.xTraj, trj.uTraj, xr, ur) / np.maximum(hp.FLOOR, 100.0 * e), 0.0)
    print(f"{name}: winner's rollout worst error / bound {ratio.max():.2e} on {int(det.sum())}/{det.size} determined prefixes")
    assert ratio.max() <= 1.0 and det.sum() >= 1


def test_line_search_nan_wins_and_first_index_wins_ties(mods):
    ilqr, models, pt, _ = mods
    b, N = 3, 2
    x0 = np.array([[1.0], [2.0], [3.0]])
    l = np.ones((b, N, 1))                               # u = alpha: alpha <= 0.25 takes the root of a negative number
    pol, prev = pt.AffinePolicy(l, np.zeros((b, N, 1, 1))), pt.Trajectory(np.zeros((b, N + 1, 1)), np.zeros((b, N, 1)))
    root = models.TracedCost(lambda x, u: np.sqrt(u[0] - 0.3), lambda x: x[0] * x[0], 1, 1)
    for md in (models.LinearModel(np.array([[0.5]]), np.array([[1.0]])), models.TracedModel(lambda x, u: np.array([0.5 * x[0] + u[0]]), 1, 1)):
        traj, J = ilqr.forwardPass2(x0, md, root, pol, prev)
        assert np.all(np.isnan(J)) and np.array_equal(traj.uTraj[:, 0, 0], np.full(b, 0.25))       # the first NaN cost: index 2
    blind = models.TracedCost(lambda x, u: x[0] * x[0], lambda x: x[0] * x[0], 1, 1)               # ignores u, on models that ignore u
    for md in (models.LinearModel(np.array([[0.5]]), np.array([[0.0]])), models.TracedModel(lambda x, u: np.array([0.5 * x[0] + 0.0 * u[0]]), 1, 1)):
        traj, J = ilqr.forwardPass2(x0, md, blind, pol, prev)
        assert np.array_equal(traj.uTraj[:, 0, 0], np.ones(b)) and np.all(np.isfinite(J))          # all 16 costs equal: index 0


def _raw_linesearch(_lib, md_struct, cs, x0, l, L, xp, up, ids=None, act=None, n_alpha=16, fill=None):
    import torch
    dev = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device="cuda")          # noqa: E731
    b, T, m = l.shape
    n = x0.shape[1]
    dx0, dl, dL, dxp, dup, dal = (dev(a) for a in (x0, l, L, xp, up, ALPHAS))
    mk = lambda *s: torch.full(s, float("nan") if fill is None else fill, dtype=torch.float64, device="cuda")   # noqa: E731
    xT, uT, J, idx = mk(b, T + 1, n), mk(b, T, m), mk(b), torch.full((b,), -7, dtype=torch.int32, device="cuda")
    dids = None if ids is None else dev(ids, torch.int32)
    dact = None if act is None else dev(act, torch.int32)
    p = lambda t: None if t is None else t.data_ptr()                                                              # noqa: E731
    rc = _lib.lib().zm_traced_cost_linesearch_list_f64(ctypes.addressof(md_struct), ctypes.addressof(cs), p(dx0), p(dl), p(dL), p(dxp),
                                                       p(dup), p(dal), n_alpha, p(dids), 0 if ids is None else len(ids), p(dact), p(xT),
                                                       p(uT), p(J), p(idx), b, T, None)
    assert rc == 0, _lib.lib().zm_last_error()
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in (xT, uT, J, idx)]


def _raw_expand(_lib, cs, n, m, xT, uT, ids=None, act=None):
    import torch
    dev = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device="cuda")          # noqa: E731
    b, T = uT.shape[:2]
    mk = lambda *s: torch.full(s, 7.5, dtype=torch.float64, device="cuda")                                        # noqa: E731
    outs = [mk(b, T), mk(b, T, n), mk(b, T, m), mk(b, T, n, n), mk(b, T, m, n), mk(b, T, m, m), mk(b), mk(b, n), mk(b, n, n)]
    dx, du = dev(xT), dev(uT)
    dids = None if ids is None else dev(ids, torch.int32)
    dact = None if act is None else dev(act, torch.int32)
    p = lambda t: None if t is None else t.data_ptr()                                                              # noqa: E731
    rc = _lib.lib().zm_traced_cost_expand_list_f64(ctypes.addressof(cs), p(dx), p(du), p(dids), 0 if ids is None else len(ids), p(dact),
                                                   *[p(o) for o in outs], b, T, None)
    assert rc == 0, _lib.lib().zm_last_error()
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


@pytest.mark.parametrize("name", ["car", "quad_registered"])
def test_list_form_touches_only_listed_active_trajectories(mods, name):
    """an id list with gaps and an `active` mask: listed, active trajectories get bit for bit what the dense call writes (parameters
    are read by trajectory id, not by slot), every other row is left untouched -- line search and expansion"""
    ilqr, models, pt, _lib = mods
    md, twin, run, term, n, m, npar = _setup(name)
    b, T = 9, 5
    p = _params(npar, b)
    cost = models.TracedCost(run, term, n, m, params=p)
    cs, ms = cost.tcost_struct((b,)), models.model_struct(md, (b,))
    prob = _problem(n, m, b, T, seed=2, specials=False)
    dense = _raw_linesearch(_lib, ms, cs, *prob)
    ids, act = [7, 2, 5, 0], np.ones(b, dtype=np.int32)
    act[5] = 0
    part = _raw_linesearch(_lib, ms, cs, *prob, ids=ids, act=act)
    dex = _raw_expand(_lib, cs, n, m, dense[0], dense[1])
    pex = _raw_expand(_lib, cs, n, m, dense[0], dense[1], ids=ids, act=act)
    for i in range(b):
        on = i in (7, 2, 0)
        for a, d in zip(part, dense):
            assert np.array_equal(a[i], d[i]) if on else (np.all(np.isnan(a[i])) or np.all(a[i] == -7)), (name, i)
        for a, d in zip(pex, dex):
            assert np.array_equal(a[i], d[i]) if on else np.all(a[i] == 7.5), (name, i)
    one = _raw_linesearch(_lib, ms, cs, *prob, n_alpha=1)          # n_alpha = 1: alpha = 1, index 0
    u0 = prob[1][:, 0] + (np.einsum("bij,bj->bi", prob[2][:, 0], prob[0] - prob[3][:, 0]) + prob[4][:, 0])
    assert np.all(one[3] == 0) and np.max(np.abs(one[1][:, 0] - u0)) <= 1e-13


# ---- expansion ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["scalar11", "pendulum", "car", "quad_registered", "wide62"])
def test_expansion_values_bit_for_bit_and_derivatives_at_the_bound(mods, host, name):
    """c, v bit for bit to the host build; gradients and Hessians per row against the long-double / sympy references; zeros exactly
    where sympy's derivative is identically zero; T = 1, 2, 7; the <= 32-slot costs run the Hyper slot file in LDS, the 62-live-slot
    cost in private scratch"""
    ilqr, models, pt, _ = mods
    hcost, _ = host
    if name == "wide62":
        run, term, n, m, npar = wide_cost(62), (lambda x: np.sin(x[0])), 1, 1, 0
    else:
        _, _, run, term, n, m, npar = _setup(name)
    for b, T in ((3, 1), (67, 2), (130, 1), (5, 7)):
        rng = np.random.default_rng([6, n, b])
        p = None if not npar else rng.uniform(-3, 3, (b, npar))
        cost = models.TracedCost(run, term, n, m, params=p)
        assert (cost.running_tape.n_slots > 32) == (name == "wide62")
        xT, uT = rng.standard_normal((b, T + 1, n)), 0.4 * rng.standard_normal((b, T, m))
        xT[b // 2:] += 2 * np.pi * rng.integers(-1000, 1001, (b - b // 2, 1, n))          # many-turn angles
        traj = pt.Trajectory(xT, uT)
        q = pt.QuadraticCostFunction.from_trajectory(cost, traj)
        V = pt.QuadraticValueFunction.fromTerminalCostFunction(cost, xT[:, -1])
        x, u = xT[:, :-1].reshape(-1, n), uT.reshape(-1, m)
        pp = None if p is None else np.repeat(p, T, 0)
        assert np.array_equal(q.c.reshape(-1), TR.host_value(hcost, cost.running_tape, x, u, pp))
        assert np.array_equal(V.v, TR.host_value(hcost, cost.terminal_tape, xT[:, -1], None, p))
        K = n + m

        def grad(tape, xx, uu, _p):
            return np.concatenate([q.c_x, q.c_u], -1).reshape(-1, K) if uu is not None else np.concatenate([V.v_x, np.zeros((b, m))], -1)

        def hess(tape, xx, uu, _p):
            H = np.zeros((len(xx), K, K))
            if uu is not None:
                H[:, :n, :n], H[:, n:, :n], H[:, n:, n:] = q.c_xx.reshape(-1, n, n), q.c_ux.reshape(-1, m, n), q.c_uu.reshape(-1, m, m)
                H[:, :n, n:] = np.swapaxes(q.c_ux.reshape(-1, m, n), -1, -2)
            else:
                H[:, :n, :n] = V.v_xx
            return H

        class _Case:
            pass
        case = _Case()
        case.n, case.m, case.running, case.terminal = n, m, run, term

        # the running points along the trajectory, the terminal points at its end
        res_r = _derivative_errors_at(case, cost, grad, hess, x, u, pp, True)
        res_t = _derivative_errors_at(case, cost, grad, hess, xT[:, -1], None, p, False)
        for (eg, bg, eH, bH), which in ((res_r, "running"), (res_t, "terminal")):
            print(f"{name} b={b} T={T} {which}: gradient {eg:.1e} (bound {bg:.1e})  Hessian {eH:.1e} (bound {bH:.1e})")
            assert eg <= bg and eH <= bH


def _derivative_errors_at(case, cost, grad, hess, x, u, p, running):
    """tests/test_traced_cost.py's comparison for one of the two tapes at its own points"""
    tape, fn = (cost.running_tape, case.running) if running else (cost.terminal_tape, case.terminal)
    _, g_ld = TR.tape_gradient_ld(tape, x, u, p)
    _, g_64 = TR.tape_gradient_ld(tape, x, u, p, dtype=np.float64)
    sym = TR.SymbolicSecond(fn, case.n, case.m, 0 if p is None else p.shape[1], running)
    H_ld, H_64 = sym(x, u, p)[:, 0], sym(x, u, p, dtype=np.float64)[:, 0]
    g, H = grad(tape, x, u, p), hess(tape, x, u, p)
    bg, bH = hp.bound(hp.row_error(g_64[:, None, :], g_ld[:, None, :])), hp.bound(hp.row_error(H_64, H_ld))
    assert hp.finite_where_reference_is(g, g_ld) and hp.finite_where_reference_is(H, H_ld)
    S = sym.pattern()[0]
    assert not H[:, ~S].any(), "zeros exactly where sympy's derivative is identically zero"
    assert len(x) < 16 or np.all((H != 0).any(0) == S)
    return hp.row_error(g[:, None, :], g_ld[:, None, :]), bg, hp.row_error(H, H_ld), bH


# ---- a quadratic cost written as a function equals QuadraticCost ------------------------------------------------------------------------
def _solve(ilqr, model, cost, x0, ug, ddp=False, **kw):
    """-> (xTraj, uTraj, L, J, converged, J_trace, alpha_trace) through the trace entry point"""
    fn = ilqr.differentialDynamicProgramming if ddp else ilqr.iterativeLqr
    ilqr._TRACE = []
    try:
        traj, L, J, conv = fn(model, cost, cost, x0, ug, **kw)
        rec = dict(ilqr._TRACE)
    finally:
        ilqr._TRACE = None
    return traj.xTraj, traj.uTraj, L, J, conv, rec["J_trace"], rec["alpha_trace"]


def _quadratic_pair(models, which):
    if which == "quadcopter":
        n, m = 12, 4
        q, r, qf = np.linspace(0.5, 2.0, n), np.array([0.3, 0.5, 0.7, 0.9]), np.linspace(5.0, 12.0, n)
        model = models.QuadcopterEuler(0.1)
        rng = np.random.default_rng(3)
        x0 = np.zeros((5, n))
        x0[:, 9:12] = rng.uniform(-3, 3, (5, 3))
        x0[:, 0:3] = rng.uniform(-1, 1, (5, 3))
        ug = np.tile(models.QuadcopterEuler.uTrim, (5, 7, 1))
    else:
        n, m = 4, 2
        q, r, qf = np.array([1.0, 2.0, 0.5, 0.3]), np.array([0.4, 0.2]), np.array([20.0, 10.0, 1.0, 3.0])
        model = models.TracedModel(C.car_any, 4, 2)
        rng = np.random.default_rng(4)
        x0 = np.concatenate([rng.uniform(-2, 2, (5, 3)), rng.uniform(0.5, 2.0, (5, 1))], 1)
        ug = np.zeros((5, 7, 2))
    run = lambda x, u: sum(q[i] * x[i] * x[i] for i in range(n)) + sum(r[j] * u[j] * u[j] for j in range(m))      # noqa: E731
    term = lambda x: sum(qf[i] * x[i] * x[i] for i in range(n))                                                       # noqa: E731
    return model, models.QuadraticCost(np.diag(q), np.diag(r), np.diag(qf)), models.TracedCost(run, term, n, m), x0, ug


@pytest.mark.parametrize("which", ["quadcopter", "car"])
def test_quadratic_cost_written_as_a_function_equals_QuadraticCost(mods, which):
    """forwardPass2: same index, J to 1e-10, trajectories to 1e-9 (the line-search tolerances of tests/test_ilqr_tracking_gpu.py);
    solves, iLQR and DDP, by the agreement rule of that file: leading iterations equal in step index and cost to 1e-9, and where the
    iterates stay together to the end: `converged` equal, J to 1e-7, inputs to 1e-6, L to 1e-5"""
    ilqr, models, pt, _ = mods
    model, qc, tc, x0, ug = _quadratic_pair(models, which)
    n, m = tc.n, tc.m
    b, T = ug.shape[:2]
    _, l, L, xp, up = _problem(n, m, b, T, seed=5, specials=False)
    pol, prev = pt.AffinePolicy(2.0 * l, L), pt.Trajectory(xp, up)
    ta, Ja = ilqr.forwardPass2(x0, model, tc, pol, prev)
    tq, Jq = ilqr.forwardPass2(x0, model, qc, pol, prev)
    assert np.all(np.abs(Ja - Jq) <= 1e-10 * np.abs(Jq)) and _rel(ta.xTraj, tq.xTraj) <= 1e-9 and _rel(ta.uTraj, tq.uTraj) <= 1e-9
    index = lambda t: np.argmin(np.abs(ALPHAS[None, :] * 2.0 * l[:, 0, 0, None] -                                    # noqa: E731
                                       (t.uTraj[:, 0, 0] - up[:, 0, 0] - np.einsum("bj,bj->b", L[:, 0, 0], x0 - xp[:, 0]))[:, None]), axis=1)
    assert np.array_equal(index(ta), index(tq))
    for ddp in (False, True):
        a = _solve(ilqr, model, tc, x0, ug, ddp, maxIter=12, tol=1e-3)
        q = _solve(ilqr, model, qc, x0, ug, ddp, maxIter=12, tol=1e-3)
        report = []
        for i in range(b):
            its = int(np.sum(q[6][:, i] >= 0))
            trace = [(q[5][k, i], int(q[6][k, i]), None) for k in range(its)]
            agree = TR.agreement(a[5][:, i], a[6][:, i], trace)
            report.append((i, agree, its))
            assert agree >= min(2, its), (which, ddp, report)
            if agree == its and np.sum(a[6][:, i] >= 0) == its:
                assert bool(a[4][i]) == bool(q[4][i]) and abs(a[3][i] - q[3][i]) <= 1e-7 * abs(q[3][i]), (which, ddp, i)
                assert _rel(a[1][i], q[1][i]) <= 1e-6 and _rel(a[2][i], q[2][i]) <= 1e-5, (which, ddp, i)
        print(f"{which} {'ddp' if ddp else 'ilqr'}: (trajectory, iterations in agreement, QuadraticCost's iterations)", report)
        assert any(ag == its for _, ag, its in report)


# ---- the non-quadratic cases ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ddp", [False, True], ids=["ilqr", "ddp"])
@pytest.mark.parametrize("name", ["pendulum", "car", "quadcopter", "quadcopter_registered"])
def test_non_quadratic_cases_follow_the_restatement(mods, name, ddp):
    """every start of tests/traced_cost_cases.py against the NumPy restatement, iterate by iterate: cost to 1e-9 relative and step
    index exactly in every iteration (test_traced_cost.py::test_solve_cases_are_decided holds the starts to a determined line search,
    so nothing is excluded), then `converged` equal, J to 1e-7, inputs to 1e-6, L to 1e-5"""
    ilqr, models, pt, _ = mods
    case = C.by_name(name.split("_")[0])
    model = case.model(models, traced=not name.endswith("registered"))
    cost = case.cost(models)
    xT, uT, L, J, conv, Jtr, atr = _solve(ilqr, model, cost, case.x0, case.uGuess, ddp, maxIter=case.maxIter, tol=case.tol)
    rc, qd = TR.RefCost(cost), case_quadratic_dynamics(case)
    for i in range(len(case.x0)):
        tr = []
        p = None if case.params is None else case.params[i]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            rt, rL, rJ, rconv, its = TR.solve(case.step, rc, case.x0[i], case.uGuess[i], p, case.maxIter, case.tol, ddp, qd, tr)
        agree = TR.agreement(Jtr[:, i], atr[:, i], tr)
        print(f"{name} {'ddp' if ddp else 'ilqr'} start {i}: {agree} of {its} iterations in agreement, indices {[t[1] for t in tr]}")
        assert agree == its, (name, ddp, i, [(t[0], t[1]) for t in tr], Jtr[:its, i], atr[:its, i])
        assert bool(conv[i]) == rconv and abs(J[i] - rJ) <= 1e-7 * abs(rJ)
        assert _rel(uT[i], rt.uTraj) <= 1e-6 and _rel(xT[i], rt.xTraj) <= 1e-6 and _rel(L[i], rL) <= 1e-5


@pytest.mark.parametrize("ddp", [False, True], ids=["ilqr", "ddp"])
@pytest.mark.parametrize("name", ["pendulum", "car"])
def test_non_quadratic_cases_match_the_generic_torch_path(mods, name, ddp):
    """the same callables as torch callables on the generic path (a closure per start over its parameter row); tolerances of
    tests/test_traced_model_gpu.py::test_pendulum_matches_the_generic_torch_path"""
    import torch
    ilqr, models, pt, _ = mods
    case = C.by_name(name)
    solve = ilqr.differentialDynamicProgramming if ddp else ilqr.iterativeLqr
    cost = case.cost(models)
    a = solve(case.model(models), cost.runningCost, cost.terminalCost, case.x0, case.uGuess, maxIter=case.maxIter, tol=case.tol)
    for i in range(len(case.x0)):
        if case.params is None:
            run, term = case.running, case.terminal
        else:
            pi = torch.as_tensor(case.params[i], dtype=torch.float64, device="cuda")
            run, term = (lambda x, u, pi=pi: case.running(x, u, pi)), (lambda x, pi=pi: case.terminal(x, pi))
        g = solve(case.step, run, term, case.x0[i], case.uGuess[i], maxIter=case.maxIter, tol=case.tol)
        assert bool(a[3][i]) == bool(g[3]) and abs(a[2][i] - g[2]) <= 1e-7 * abs(g[2]), (name, ddp, i)
        assert _rel(a[0].xTraj[i], g[0].xTraj) <= 1e-6 and _rel(a[0].uTraj[i], g[0].uTraj) <= 1e-6 and _rel(a[1][i], g[1]) <= 1e-5


# ---- batch behaviour ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ddp", [False, True], ids=["ilqr", "ddp"])
def test_batch_of_67_with_parameters_equals_the_single_solves_bit_for_bit(mods, ddp):
    """per-trajectory cost parameters on a traced model that has per-trajectory parameters too: every instance of the batch equals
    its single-problem solve bit for bit, and one that has converged is not touched again while the others go on"""
    ilqr, models, pt, _ = mods
    b, N = 67, 7
    rng = np.random.default_rng(67)
    lengths = rng.uniform(0.5, 2.0, (b, 1))
    goal = np.stack([rng.uniform(-0.5, 0.5, b), rng.uniform(2.0, 12.0, b)], 1)          # (goal angle, weight)
    x0 = np.stack([rng.uniform(-1.5, 1.5, b), rng.uniform(-1, 1, b)], 1)
    ug = np.zeros((b, N, 1))
    run = lambda x, u, p: p[1] * (1.0 - np.cos(x[0] - p[0])) + 0.5 * x[1] * x[1] + 0.1 * u[0] * u[0]      # noqa: E731
    term = lambda x, p: 10.0 * p[1] * (1.0 - np.cos(x[0] - p[0])) + 10.0 * x[1] * x[1]                    # noqa: E731
    solve = ilqr.differentialDynamicProgramming if ddp else ilqr.iterativeLqr
    cost = models.TracedCost(run, term, 2, 1, params=goal)
    traj, L, J, conv = solve(models.TracedModel(R.pendulum_p, 2, 1, params=lengths), cost, cost, x0, ug, maxIter=30)
    assert conv.any()
    for i in range(b):
        ci = models.TracedCost(run, term, 2, 1, params=goal[i])
        ti, Li, Ji, cvi = solve(models.TracedModel(R.pendulum_p, 2, 1, params=lengths[i]), ci, ci, x0[i], ug[i], maxIter=30)
        assert np.array_equal(ti.xTraj, traj.xTraj[i]) and np.array_equal(ti.uTraj, traj.uTraj[i]) and np.array_equal(Li, L[i]), i
        assert Ji == J[i] and cvi == bool(conv[i])


# ---- reference KAT --------------------------------------------------------------------------------------------------------------------
def test_identity_kat(mods):
    """reference tests/test_ilqrUtils.py:167-196 (A = B = Q = R = I, N = 3, x0 = (2, 1)) written as three lambdas"""
    ilqr, models, pt, _ = mods
    I = np.eye(2)
    x0 = np.array([2.0, 1.0])
    cost = models.TracedCost(lambda x, u: x @ x + u @ u, lambda x: x @ x, 2, 2)
    for md in (models.TracedModel(lambda x, u: x + u, 2, 2), models.LinearModel(I, I)):
        for solver, ddp in ((ilqr.iterativeLqr, False), (ilqr.differentialDynamicProgramming, True)):
            traj, L, J, conv = solver(md, cost.runningCost, cost.terminalCost, x0, np.zeros((3, 2)))
            assert conv is True and isinstance(J, float)
            if ddp:
                rt, rL, rJ, rc = zo.differentialDynamicProgramming(lambda x, u: x + u, lambda x, u: x + u, I, I, I, x0, np.zeros((3, 2)))
            else:
                rt, rL, rJ, rc = zo.iterativeLqr(lambda x, u: x + u, I, I, I, x0, np.zeros((3, 2)))
            assert rc and _rel(traj.uTraj, rt.uTraj) <= 1e-9 and _rel(L, rL) <= 1e-9 and J == pytest.approx(rJ, rel=1e-10)
