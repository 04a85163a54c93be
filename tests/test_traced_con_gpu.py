"""GPU tests of models.TracedConstraint (zm_tracedcon_t; zopt_amd/csrc/traced_con.hip): device values of g against the host build of
the interpreter, the penalty line search, the penalty expansion and the multiplier update against NumPy and long double, and the
augmented-Lagrangian solve against the restatement (tests/traced_con_ref.py) iterate by iterate through the trace entry.

Cases: tests/traced_con_cases.py (their hygiene is asserted on the CPU by tests/test_traced_con.py, so no comparison is skipped here).
Shapes are the smallest that reach the kernels' seams: n + m = 3 (idle lanes of a 16-lane group) and 16 (lane 15 included), T = 1,
5 x 12 points (no multiple of the 4 points of a wave), n_con in {1, 2, 8}, a terminal-only constraint, rows that depend on u, permuted
id lists and masks with holes."""
import ctypes

import numpy as np
import pytest

from oracle import zopt_oracle as zo
from tests import tape_ref as R
from tests import traced_con_cases as C
from tests import traced_con_ref as CR
from tests import ilqr_tracking_ref as tref

pytestmark = pytest.mark.gpu
LD = np.longdouble
ULP = 2.0 ** -52


@pytest.fixture(scope="module")
def mods():
    import torch
    assert torch.cuda.is_available()
    from zopt_amd import _lib, ilqrUtils, models, pytrees
    return ilqrUtils, models, pytrees, _lib


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return CR.build(tmp_path_factory.mktemp("tape_con_shim"))


def _dev(a, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype or torch.float64).cuda()


def _cost(models, c):
    if c.goals is None:
        return models.QuadraticCost(c.Q, c.R, c.Qf)
    return models.TrackingCost(c.Q, c.R, c.Qf, xRef=c.goals[:, None, :], uRef=c.ug[:, :1, :])


def _prow(c, b):
    return None if c.params is None else c.params[b]


def _trajectories(c):
    """(xTraj (b, T + 1, n), uTraj (b, T, m)): the restatement's solutions, then pushed off them by a seeded perturbation of the inputs
    so that rows of either sign occur"""
    rng = np.random.default_rng([7, c.n, c.T])
    B = c.x0.shape[0]
    xs, us = [], []
    for b in range(B):
        u = C.restatement(c.name, b)["traj"].uTraj + 0.3 * rng.standard_normal((c.T, c.m)) * (1.0 if c.n < 12 else 0.02)
        t = zo.trajectoryRollout(c.x0[b], c.dyn, zo.AffinePolicy(u, np.zeros((c.T, c.m, c.n))), zo.Trajectory(np.zeros((c.T + 1, c.n)), np.zeros((c.T, c.m))))
        xs.append(t.xTraj), us.append(t.uTraj)
    return np.stack(xs), np.stack(us)


def _multipliers(c, seed, scale=1e4):
    """lam (b, T, nc), lamT (b, nct), mu (b): a third of the multipliers zero, the others 10^U(-2, log scale); mu 10^linspace(0, 4)"""
    rng = np.random.default_rng([seed, c.n, c.T])
    B = c.x0.shape[0]

    def draw(shape):
        v = 10.0 ** rng.uniform(-2, np.log10(scale), shape)
        v[rng.random(shape) < 1 / 3] = 0.0
        return v
    mu = rng.permutation(10.0 ** np.linspace(0, 4, B)) if B > 1 else np.array([30.0])
    return draw((B, c.T, c.n_con)), draw((B, c.n_con_terminal)), mu


# ------------------------------------------------------------------------------------------------------------------------- 1  values
@pytest.mark.parametrize("name", C.NAMES)
def test_device_values_are_the_host_build_bit_for_bit(mods, shim, name):
    c = C.by_name(name)
    con = C.constraint(name)
    x, u = _trajectories(c)
    g, gT = con.values(x, u)
    assert g.shape == (len(x), c.T, c.n_con) and gT.shape == (len(x), c.n_con_terminal)
    for b in range(len(x)):
        if c.n_con:
            h = CR.host_value(shim, con.stage_tape, x[b, :-1], u[b], _prow(c, b))
            assert np.array_equal(g[b], h), (name, b, np.max(np.abs(g[b] - h)))
        if c.n_con_terminal:
            h = CR.host_value(shim, con.terminal_tape, x[b, -1:], None, _prow(c, b))
            assert np.array_equal(gT[b], h[0]), (name, b)


# --------------------------------------------------------------------------------------------------------------------- 2  line search
def _linesearch_problem(c, seed):
    """a policy about the restatement's solution: l a seeded step, L a seeded gain"""
    rng = np.random.default_rng([seed, c.n, c.T, 3])
    x, u = _trajectories(c)
    B = len(x)
    sc = 1.0 if c.n < 12 else 0.02
    l = 0.2 * sc * rng.standard_normal((B, c.T, c.m))
    L = 0.05 * rng.standard_normal((B, c.T, c.m, c.n))
    return x, u, l, L


def _linesearch_reference(c, con, b, x, u, l, L, lam, lamT, mu):
    rc = CR.RefCon(con)
    xr, ur = C.references(c, b)
    return CR.forward_pass(c.x0[b], c.dyn, c.Q, c.R, c.Qf, xr, ur, zo.AffinePolicy(l[b], L[b]), zo.Trajectory(x[b], u[b]), rc, _prow(c, b),
                           (lam[b], lamT[b], mu[b]))


def _magnitude(c, con, b, traj, lam, lamT, mu):
    """the sum of the absolute values of the terms of J and of J_AL along a trajectory: the yardstick of the 1e-12"""
    xr, ur = C.references(c, b)
    S = 0.0
    for k in range(c.T):
        S += abs(tref.running_cost(c.Q, c.R, xr, ur, k)(traj.xTraj[k], traj.uTraj[k]))
    S += abs(tref.terminal_cost(c.Qf, xr)(traj.xTraj[-1]))
    g, gT = CR.RefCon(con).rows(traj, _prow(c, b))
    SP = float(np.sum((CR.pos(lam[b] + mu[b] * g) ** 2 + lam[b] ** 2) / (2 * mu[b])) + np.sum((CR.pos(lamT[b] + mu[b] * gT) ** 2 + lamT[b] ** 2) / (2 * mu[b])))
    return S, S + SP


def _call_linesearch(mods, c, con, x, u, l, L, lam, lamT, mu, alphas, list_=None, active=None, fill=None):
    import torch
    ilqr, models, _, _lib = mods
    B = len(x)
    lead = (B,)
    d = dict(x0=_dev(c.x0), l=_dev(l), L=_dev(L), xp=_dev(x), up=_dev(u), al=_dev(alphas), lam=_dev(lam), lamT=_dev(lamT), mu=_dev(mu))
    cs = con.con_struct(lead, d["lam"], d["lamT"], d["mu"])
    md = models.model_struct(con.model, lead)
    cost = _cost(models, c)
    ks = cost.track_struct(lead, c.T) if c.goals is not None else cost.c_struct()
    val = np.nan if fill is None else fill
    xT = torch.full((B, c.T + 1, c.n), val, dtype=torch.float64, device="cuda")
    uT = torch.full((B, c.T, c.m), val, dtype=torch.float64, device="cuda")
    J = torch.full((B,), val, dtype=torch.float64, device="cuda")
    Jc = torch.full((B,), val, dtype=torch.float64, device="cuda")
    idx = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    dl = None if list_ is None else _dev(list_, torch.int32)
    da = None if active is None else _dev(active, torch.int32)
    pk = ctypes.addressof(ks)
    rc = _lib.lib().zm_traced_con_linesearch_list_f64(
        ctypes.addressof(md), None if c.goals is not None else pk, pk if c.goals is not None else None, ctypes.addressof(cs),
        d["x0"].data_ptr(), d["l"].data_ptr(), d["L"].data_ptr(), d["xp"].data_ptr(), d["up"].data_ptr(), d["al"].data_ptr(), len(alphas),
        None if dl is None else dl.data_ptr(), 0 if list_ is None else len(list_), None if da is None else da.data_ptr(), xT.data_ptr(),
        uT.data_ptr(), J.data_ptr(), Jc.data_ptr(), idx.data_ptr(), B, c.T, None)
    _lib.check(rc, "linesearch")
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (xT, uT, J, Jc, idx))


@pytest.mark.parametrize("name", ["lin21_T9", "lin21_T1", "lin21_terminal", "car", "car8", "pendulum", "quadcopter"])
def test_penalty_line_search_against_the_restatement(mods, name):
    """NA = 16 over a permuted list with a masked hole, and NA = 1 at the winning step size: the index exact, J_AL and J to 1e-12 of
    the magnitude of their terms, the winner's rows to 1e-12, the rows of trajectories not listed or not active untouched"""
    c = C.by_name(name)
    con = C.constraint(name)
    x, u, l, L = _linesearch_problem(c, 11)
    lam, lamT, mu = _multipliers(c, 5)
    B = len(x)
    order = np.random.default_rng(3).permutation(B)
    listed = order if B == 1 else order[:-1]                    # one trajectory is not listed
    active = np.ones(B, dtype=np.int32)
    if B > 2:
        active[listed[1]] = 0                                       # a hole in the mask
    xT, uT, J, Jc, idx = _call_linesearch(mods, c, con, x, u, l, L, lam, lamT, mu, zo.LINESEARCH_ALPHAS, list_=listed.astype(np.int32),
                                          active=active, fill=-3.25)
    ran = [b for b in listed if active[b]]
    for b in range(B):
        if b not in ran:
            assert np.all(xT[b] == -3.25) and np.all(uT[b] == -3.25) and J[b] == -3.25 and Jc[b] == -3.25 and idx[b] == -7, (name, b)
    single = {}
    for b in ran:
        t, Jr, Jcr, ir, Js = _linesearch_reference(c, con, b, x, u, l, L, lam, lamT, mu)
        srt = np.sort(Js)
        assert srt[1] - srt[0] >= 1e-9 * abs(srt[0]), (name, b, "the test's own problem has no determined winner")
        S, SAL = _magnitude(c, con, b, t, lam, lamT, mu)
        print(f"{name}[{b}]: idx {idx[b]} ({ir}), |J_AL - ref| / S = {abs(J[b] - Jr) / SAL:.2e}, |J - ref| / S = {abs(Jc[b] - Jcr) / S:.2e}")
        assert idx[b] == ir, (name, b, idx[b], ir)
        assert abs(J[b] - Jr) <= 1e-12 * SAL and abs(Jc[b] - Jcr) <= 1e-12 * S, (name, b)
        sx = np.maximum(1.0, np.max(np.abs(t.xTraj)))
        assert np.max(np.abs(xT[b] - t.xTraj)) <= 1e-12 * sx and np.max(np.abs(uT[b] - t.uTraj)) <= 1e-12 * max(1.0, np.max(np.abs(t.uTraj)))
        assert np.array_equal(xT[b, 0], c.x0[b])
        single[b] = (J[b], Jc[b], xT[b], uT[b])
    # NA = 1: every trajectory at its own winner's step size is not one launch; run the launch at alphas[i] for each i that won
    for i in sorted({int(idx[b]) for b in ran}):
        x1, u1, J1, Jc1, i1 = _call_linesearch(mods, c, con, x, u, l, L, lam, lamT, mu, zo.LINESEARCH_ALPHAS[i:i + 1])
        for b in ran:
            if int(idx[b]) == i:
                assert J1[b] == single[b][0] and Jc1[b] == single[b][1] and i1[b] == 0, (name, b)
                assert np.array_equal(x1[b], single[b][2]) and np.array_equal(u1[b], single[b][3])


def test_a_nan_rollout_wins_the_line_search(mods):
    """jnp.argmin: a NaN cost beats every number, the first index among equals -- here every step size of trajectory 1 is NaN"""
    c = C.by_name("car")
    con = C.constraint("car")
    x, u, l, L = _linesearch_problem(c, 11)
    lam, lamT, mu = _multipliers(c, 5)
    l[1, 3, 0] = np.nan
    xT, uT, J, Jc, idx = _call_linesearch(mods, c, con, x, u, l, L, lam, lamT, mu, zo.LINESEARCH_ALPHAS)
    assert np.isnan(J[1]) and idx[1] == 0 and np.all(np.isfinite(np.delete(J, 1)))
    assert np.all(np.isfinite(xT[1, :4])) and np.isnan(uT[1, 3, 0])


# ----------------------------------------------------------------------------------------------------------------------- 3  expansion
def _expand(mods, c, con, x, u, lam, lamT, mu, shared, pre, list_=None, active=None):
    """zm_traced_con_expand_list_f64; shared = (sc_xx, sc_ux, sc_uu, sv_xx); pre = (c_x, c_u, v_x) before the call; the per-point
    Hessians start as NaN"""
    import torch
    _, models, _, _lib = mods
    B = len(x)
    d = dict(lam=_dev(lam), lamT=_dev(lamT), mu=_dev(mu))
    cs = con.con_struct((B,), d["lam"], d["lamT"], d["mu"])
    dx, du = _dev(x), _dev(u)
    sh = [_dev(s) for s in shared]
    g = [_dev(p) for p in pre]
    n, m, T = c.n, c.m, c.T
    H = [torch.full(s, float("nan"), dtype=torch.float64, device="cuda") for s in ((B, T, n, n), (B, T, m, n), (B, T, m, m), (B, n, n))]
    dl = None if list_ is None else _dev(list_, torch.int32)
    da = None if active is None else _dev(active, torch.int32)
    rc = _lib.lib().zm_traced_con_expand_list_f64(
        ctypes.addressof(cs), dx.data_ptr(), du.data_ptr(), None if dl is None else dl.data_ptr(), 0 if list_ is None else len(list_),
        None if da is None else da.data_ptr(), *[s.data_ptr() for s in sh], *[t.data_ptr() for t in g], *[t.data_ptr() for t in H], B, T,
        None)
    _lib.check(rc, "expand")
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in g], [t.cpu().numpy() for t in H]


def _row_bound(ref_ld, ref64):
    """per row (last axis): the larger of 100 ulp of the row's largest entry and 100 x the fp64 restatement's own error"""
    big = np.max(np.abs(ref_ld), axis=-1, keepdims=True).astype(np.float64)
    e64 = np.max(np.abs(ref64.astype(LD) - ref_ld), axis=-1, keepdims=True).astype(np.float64)
    return np.maximum(100 * ULP * big, 100 * e64)


@pytest.mark.parametrize("name", ["lin21_T1", "lin21_terminal", "car", "car8", "pendulum", "quadcopter"])
def test_penalty_expansion_against_long_double_dual_numbers(mods, name):
    """zero shared Hessians and zero gradients before the call: the outputs are the addends themselves -- G^T pos(s) and
    mu G^T diag(s > 0) G per row against long-double dual numbers on the tape, bound 100 x the fp64 restatement's own error; then
    with seeded shared Hessians and gradients: exactly (shared + addend) and (before + addend); rows of trajectories that are not
    listed or not active keep what they held"""
    c = C.by_name(name)
    con = C.constraint(name)
    rc = CR.RefCon(con)
    x, u = _trajectories(c)
    lam, lamT, mu = _multipliers(c, 9)
    B, n, m, T = len(x), c.n, c.m, c.T
    K = n + m
    zero_sh = (np.zeros((n, n)), np.zeros((m, n)), np.zeros((m, m)), np.zeros((n, n)))
    zero_pre = (np.zeros((B, T, n)), np.zeros((B, T, m)), np.zeros((B, n)))
    (gx, gu, gv), (Hxx, Hux, Huu, Hv) = _expand(mods, c, con, x, u, lam, lamT, mu, zero_sh, zero_pre)
    worst = 0.0
    for b in range(B):
        traj = zo.Trajectory(x[b], u[b])
        p = _prow(c, b)
        refs = []
        for dt in (LD, np.float64):
            G, GT = rc.jacobians(traj, p, dt)
            if dt is LD:       # g in long double on the tape as well
                pp = None if p is None else np.asarray(p, dtype=LD)
                g = R.evaluate(con.stage_tape, x[b, :-1].astype(LD), u[b].astype(LD), pp, R.Real(LD)) if c.n_con else np.zeros((T, 0), dtype=LD)
                gT = (R.evaluate(con.terminal_tape, x[b, -1:].astype(LD), np.zeros((1, m), dtype=LD), pp, R.Real(LD))[0] if c.n_con_terminal
                      else np.zeros(0, dtype=LD))
                s = np.concatenate([(lam[b] + mu[b] * g).ravel(), (lamT[b] + mu[b] * gT).ravel()]).astype(np.float64)
                size = np.concatenate([(lam[b] + mu[b] * np.abs(g)).ravel(), (lamT[b] + mu[b] * np.abs(gT)).ravel()]).astype(np.float64)
                assert np.all(np.abs(s) >= 1e-9 * np.maximum(size, 1e-300)), (name, b, "a row on the edge of activity: reseed")
            else:
                g, gT = rc.rows(traj, p)
            refs.append(CR.addends(g.astype(dt), G, lam[b].astype(dt), dt(mu[b])) + CR.addends(gT.astype(dt), GT, lamT[b].astype(dt), dt(mu[b])))
        (grad, H, gradT, HT), (grad64, H64, gradT64, HT64) = refs
        dev_grad = np.concatenate([gx[b], gu[b]], axis=-1)                                    # (T, K)
        dev_H = np.zeros((T, K, K))
        dev_H[:, :n, :n], dev_H[:, n:, :n], dev_H[:, n:, n:] = Hxx[b], Hux[b], Huu[b]
        dev_H[:, :n, n:] = np.swapaxes(Hux[b], -1, -2)                                        # (the block the kernel does not store)
        checks = [(dev_grad, grad, grad64), (dev_H, H, H64), (gv[b], gradT, gradT64), (Hv[b], HT, HT64)]
        for dv, ld, f64 in checks:
            if ld.size == 0:
                continue
            bound = _row_bound(ld, f64)
            err = np.abs(dv.astype(LD) - ld).astype(np.float64)
            assert np.all(err <= bound), (name, b, float(np.max(err / np.maximum(bound, 1e-300))))
            worst = max(worst, float(np.max(np.where(bound > 0, err / np.maximum(bound, 1e-300), 0.0))))
        assert np.array_equal(Hxx[b], np.swapaxes(Hxx[b], -1, -2)) or np.max(np.abs(Hxx[b] - np.swapaxes(Hxx[b], -1, -2))) <= 4 * ULP * np.max(np.abs(Hxx[b]))
    print(f"{name}: worst error / bound {worst:.3f}")
    # seeded shared Hessians and gradients, a permuted list with a trajectory left out and a hole in the mask
    rng = np.random.default_rng(2)
    shared = tuple(rng.standard_normal(s.shape) for s in zero_sh)
    pre = tuple(rng.standard_normal(s.shape) for s in zero_pre)
    order = rng.permutation(B)
    listed = order if B == 1 else order[:-1]
    active = np.ones(B, dtype=np.int32)
    if B > 2:
        active[listed[0]] = 0
    (gx2, gu2, gv2), (Hxx2, Hux2, Huu2, Hv2) = _expand(mods, c, con, x, u, lam, lamT, mu, shared, pre, listed.astype(np.int32), active)
    for b in range(B):
        if b in listed and active[b]:
            assert np.array_equal(gx2[b], pre[0][b] + gx[b]) and np.array_equal(gu2[b], pre[1][b] + gu[b]) and np.array_equal(gv2[b], pre[2][b] + gv[b])
            assert np.array_equal(Hxx2[b], shared[0] + Hxx[b]) and np.array_equal(Hux2[b], shared[1] + Hux[b])
            assert np.array_equal(Huu2[b], shared[2] + Huu[b]) and np.array_equal(Hv2[b], shared[3] + Hv[b])
        else:
            assert np.array_equal(gx2[b], pre[0][b]) and np.array_equal(gu2[b], pre[1][b]) and np.array_equal(gv2[b], pre[2][b])
            assert np.all(np.isnan(Hxx2[b])) and np.all(np.isnan(Hux2[b])) and np.all(np.isnan(Huu2[b])) and np.all(np.isnan(Hv2[b]))


# --------------------------------------------------------------------------------------------------------------- 4  multiplier update
@pytest.mark.parametrize("name", ["lin21_T1", "car", "car8", "quadcopter", "lin21_terminal"])
@pytest.mark.parametrize("update", [1, 0])
def test_multiplier_update_exactly_against_numpy_on_the_devices_own_g(mods, name, update):
    """violation, lam, mu, the masks and the counters exactly; a finished trajectory's rows are untouched; a NaN trajectory is never
    done"""
    import torch
    _, models, _, _lib = mods
    c = C.by_name(name)
    con = C.constraint(name)
    x, u = _trajectories(c)
    B0 = len(x)
    reps = 2 if B0 > 1 else 4                       # a batch of at least 4: done earlier, done now, not done, NaN
    x, u = np.tile(x, (reps, 1, 1))[:max(4, B0)], np.tile(u, (reps, 1, 1))[:max(4, B0)]
    B = len(x)
    x[B - 1, c.T if c.n_con == 0 else min(1, c.T - 1), 9 if c.n == 12 else 0] = np.nan      # a position: every case's rows read it
    params = None if c.params is None else np.tile(c.params, (reps, 1))[:B]
    con = models.TracedConstraint(c.model(), c.g, c.n_con, c.terminal, c.n_con_terminal, params=params, **c.kw) if params is not None else con
    g, gT = con.values(x, u)
    rng = np.random.default_rng([4, B, c.T])
    lam, lamT = rng.uniform(0, 2, (B, c.T, c.n_con)) * (rng.random((B, c.T, c.n_con)) < 0.7), rng.uniform(0, 2, (B, c.n_con_terminal))
    mu = 10.0 ** rng.uniform(0, 7.9, B)
    mu[0] = 5e7                                      # growth takes it past mu_max
    active = np.ones(B, dtype=np.int32)
    active[1] = 0                                    # done earlier
    conv = np.ones(B, dtype=np.int32)
    conv[2] = 0                                      # its inner solve did not converge: not done whatever the violation
    viol_np = np.array([np.nan if (np.isnan(g[b]).any() or np.isnan(gT[b]).any()) else max(0.0, np.max(np.concatenate([g[b].ravel(), gT[b].ravel()])))
                        for b in range(B)])
    ctol = float(np.nanmedian(viol_np[viol_np > 0])) if np.any(viol_np > 0) else 1e-4       # some below, some above
    d = dict(lam=_dev(lam), lamT=_dev(lamT), mu=_dev(mu), x=_dev(x), u=_dev(u), act=_dev(active, torch.int32), conv=_dev(conv, torch.int32))
    viol = torch.full((B,), -1.0, dtype=torch.float64, device="cuda")
    count = torch.full((B,), 3, dtype=torch.int32, device="cuda")
    rem = torch.zeros(1, dtype=torch.int32, device="cuda")
    cs = con.con_struct((B,), d["lam"], d["lamT"], d["mu"])
    rc = _lib.lib().zm_traced_con_multiplier_update_f64(ctypes.addressof(cs), d["x"].data_ptr(), d["u"].data_ptr(), d["act"].data_ptr(),
                                                        d["conv"].data_ptr(), viol.data_ptr(), count.data_ptr(), rem.data_ptr(), ctol, 10.0,
                                                        1e8, update, B, c.T, None)
    _lib.check(rc, "update")
    torch.cuda.synchronize()
    o = {k: v.cpu().numpy() for k, v in d.items()}
    viol, count, rem = viol.cpu().numpy(), count.cpu().numpy(), int(rem.cpu().numpy()[0])
    left = 0
    for b in range(B):
        if not active[b]:
            assert viol[b] == -1.0 and count[b] == 3 and o["act"][b] == 0 and o["conv"][b] == 1 and o["mu"][b] == mu[b]
            assert np.array_equal(o["lam"][b], lam[b]) and np.array_equal(o["lamT"][b], lamT[b])
            continue
        assert (np.isnan(viol[b]) and np.isnan(viol_np[b])) or viol[b] == viol_np[b], (name, b, viol[b], viol_np[b])
        done = bool(conv[b]) and bool(viol_np[b] <= ctol)
        assert count[b] == 4 and o["conv"][b] == int(done) and o["act"][b] == int(not done), (name, b)
        left += int(not done)
        if done or not update:
            assert o["mu"][b] == mu[b] and np.array_equal(o["lam"][b], lam[b]) and np.array_equal(o["lamT"][b], lamT[b])
        else:
            assert o["mu"][b] == min(mu[b] * 10.0, 1e8)
            with np.errstate(invalid="ignore"):
                assert np.array_equal(o["lam"][b], CR.pos(lam[b] + mu[b] * g[b])) and np.array_equal(o["lamT"][b], CR.pos(lamT[b] + mu[b] * gT[b]))
    assert rem == left
    assert o["act"][B - 1] == 1 and o["conv"][B - 1] == 0 and np.isnan(viol[B - 1])          # the NaN trajectory is never done
    assert o["mu"][0] == (1e8 if update and o["act"][0] else mu[0])


# -------------------------------------------------------------------------------------------------------------------------- 5  solves
def _solve(mods, c, con, info=True):
    ilqr, models, _, _ = mods
    cost = _cost(models, c)
    ilqr._TRACE = []
    try:
        out = ilqr.constrainedIterativeLqr(con, cost, cost, c.x0, c.ug, maxIter=c.maxIter, tol=c.tol)
        rec = dict(ilqr._TRACE)
    finally:
        ilqr._TRACE = None
    return out, rec


@pytest.mark.parametrize("name", C.NAMES)
def test_solves_follow_the_restatement(mods, name):
    """iterate by iterate through the trace entry: converged, the outer count, every inner count and every step index equal; the J_AL
    trace, J, the violation and mu to 1e-9; the multipliers to 1e-8 of their largest"""
    c = C.by_name(name)
    con = C.constraint(name)
    (traj, L, J, conv, info), rec = _solve(mods, c, con)
    B = c.x0.shape[0]
    assert info.lam.shape == (B, c.T, c.n_con) and info.lam_terminal.shape == (B, c.n_con_terminal)
    assert np.all(info.violation[conv] <= con.ctol)
    for b in range(B):
        r = C.restatement(name, b)
        vs = max([1.0] + [abs(o["violation"]) for o in r["trace"] if np.isfinite(o["violation"])])
        assert bool(conv[b]) == r["converged"] and int(info.outerIterations[b]) == r["outer"], (name, b, conv[b], info.outerIterations[b], r["outer"])
        assert list(info.innerIterations[b][: r["outer"]]) == r["inner"], (name, b, info.innerIterations[b], r["inner"])
        for j, o in enumerate(r["trace"]):
            assert abs(rec["mu_trace"][j, b] - o["mu"]) <= 1e-9 * o["mu"]
            assert abs(rec["violation_trace"][j, b] - o["violation"]) <= 1e-9 * vs, (name, b, j, rec["violation_trace"][j, b], o["violation"])
            for it, rit in enumerate(o["inner"]):
                Jd, ad = rec["J_trace"][j, it, b], rec["alpha_trace"][j, it, b]
                assert ad == rit["idx"], (name, b, j, it, ad, rit["idx"])
                assert abs(Jd - rit["J"]) <= 1e-9 * abs(rit["J"]), (name, b, j, it, Jd, rit["J"])
        assert abs(J[b] - r["J"]) <= 1e-9 * abs(r["J"]) and abs(info.mu[b] - r["mu"]) <= 1e-9 * r["mu"]
        assert abs(info.violation[b] - r["violation"]) <= 1e-9 * vs
        for dv, q in ((info.lam[b], r["lam"]), (info.lam_terminal[b], r["lam_terminal"])):
            if q.size:
                assert np.max(np.abs(dv - q)) <= 1e-8 * max(np.max(np.abs(q)), 1.0), (name, b)
        assert np.max(np.abs(traj.uTraj[b] - r["traj"].uTraj)) <= 1e-6 * max(1.0, np.max(np.abs(r["traj"].uTraj))), (name, b)
    print(f"{name}: outer {info.outerIterations.tolist()} converged {conv.tolist()} violation {info.violation.tolist()}")


def test_the_returned_violation_is_that_of_the_values_entry_and_iterativeLqr_returns_four(mods):
    c = C.by_name("car")
    con = C.constraint("car")
    ilqr, models, _, _ = mods
    cost = _cost(models, c)
    traj, L, J, conv, info = ilqr.constrainedIterativeLqr(con, cost, cost, c.x0, c.ug, maxIter=c.maxIter, tol=c.tol)
    g, gT = con.values(traj.xTraj, traj.uTraj)
    assert np.array_equal(info.violation, np.maximum(0.0, g.max(axis=(1, 2))))
    assert np.all(info.lam[2] == 0.0) and info.outerIterations[2] == 1 and np.all(info.innerIterations[2, 1:] == 0)   # never active
    assert not conv[3] and info.violation[3] > con.ctol and info.outerIterations[3] == con.outer                      # starts inside
    out4 = ilqr.iterativeLqr(con, cost, cost, c.x0, c.ug, maxIter=c.maxIter, tol=c.tol)
    assert len(out4) == 4 and np.array_equal(out4[0].uTraj, traj.uTraj) and np.array_equal(out4[2], J)
    # the plain cost of the returned trajectory
    Jq = np.array([tref.trajectory_cost(c.Q, c.R, c.Qf, np.zeros((c.T + 1, c.n)), np.zeros((c.T, c.m)), zo.Trajectory(traj.xTraj[b], traj.uTraj[b]))
                   for b in range(len(J))])
    assert np.max(np.abs(J - Jq) / np.abs(Jq)) <= 1e-12


def test_rollouts_unwrap_a_traced_constraint(mods):
    ilqr, models, pytrees, _ = mods
    c = C.by_name("car")
    con = C.constraint("car")
    x, u = _trajectories(c)
    pol = pytrees.AffinePolicy(np.zeros_like(u), np.zeros((len(u), c.T, c.m, c.n)))
    prev = pytrees.Trajectory(x, u)
    a = ilqr.trajectoryRollout(c.x0, con, pol, prev)
    b = ilqr.trajectoryRollout(c.x0, con.model, pol, prev)
    assert np.array_equal(a.xTraj, b.xTraj) and np.array_equal(a.uTraj, b.uTraj)
    from zopt_amd import simulator
    s = simulator.simulateTrackingController(con, c.x0, np.zeros((len(u), c.T, c.m, c.n)), prev)
    assert np.array_equal(s.xTraj, b.xTraj)
