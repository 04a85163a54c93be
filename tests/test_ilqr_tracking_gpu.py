"""GPU tests of the tracking cost (models.TrackingCost, zm_trackcost_t) through the fused iLQR / DDP path: the line-search kernels
(rollout.hip, rollout_fast.hip), the expansion kernels (linearize.hip) and the solve (ilqr_solve.hip), against the QuadraticCost
calls (zero reference: bit for bit), against the NumPy restatement (tests/ilqr_tracking_ref.py) and against each other.

Shapes are the smallest that reach the kernels' seams: T in {1, 2, 3, 4, 5, 7} (the fast kernel prefetches three steps ahead in four
rotating register sets), batches of 5 and 9 (a partial four-trajectory wave, an idle group), the (12, 4) fast path and the generic
kernel, diagonal and full weights, the three reference layouts, an id list with gaps and an `active` mask."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import zopt_oracle as zo
from tests import ilqr_tracking_child as child
from tests import ilqr_tracking_ref as tref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TS = (1, 2, 3, 4, 5, 7)


def _rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300)


@pytest.fixture(scope="module")
def mods():
    import torch
    assert torch.cuda.is_available()
    from zopt_amd import _lib, ilqrUtils, models, pytrees
    return ilqrUtils, models, pytrees, _lib


def _model(models, name):
    """-> (registered model, the oracle's callable, n, m)"""
    rng = np.random.default_rng(5)
    if name == "quad":
        return models.QuadcopterEuler(0.1), zo.quad_euler_step(0.1), 12, 4
    if name == "rb":
        return models.QuadcopterRigidBody(0.1), (lambda x, u: x + 0.1 * zo.quad_rigidBodyDynamics(x, u)), 8, 4
    n, m = (12, 4) if name == "lin12" else (3, 2)
    A, B = np.eye(n) + 0.05 * rng.standard_normal((n, n)), 0.3 * rng.standard_normal((n, m))
    return models.LinearModel(A, B), (lambda x, u: A @ x + B @ u), n, m


def _weights(n, m, diag):
    rng = np.random.default_rng(n + 7 * diag)
    if diag:
        return np.diag(rng.uniform(0.5, 2, n)), np.diag(rng.uniform(0.5, 2, m)), np.diag(rng.uniform(5, 20, n))
    return (np.eye(n) + 0.1 * rng.standard_normal((n, n)), np.eye(m) + 0.1 * rng.standard_normal((m, m)),
            10 * np.eye(n) + 0.1 * rng.standard_normal((n, n)))          # nonsymmetric on purpose


def _point(rng, name, B, T, n, m):
    """a policy, a previous trajectory and start states that keep a rollout of T steps tame"""
    u0 = np.array([9.807, 0, 0, 0]) if name in ("quad", "rb") else np.zeros(m)
    x0 = 0.3 * rng.standard_normal((B, n))
    l, L = 0.05 * rng.standard_normal((B, T, m)), 0.02 * rng.standard_normal((B, T, m, n))
    xp, up = 0.1 * rng.standard_normal((B, T + 1, n)), u0 + 0.05 * rng.standard_normal((B, T, m))
    return x0, l, L, xp, up


def _reference(rng, layout, B, T, n, m):
    """the three layouts: one goal for all, a goal per trajectory (step axis of length 1: stride 0), a full per-step reference"""
    if layout == "shared":
        return rng.standard_normal(n), 0.3 * rng.standard_normal(m)
    if layout == "goal":
        return rng.standard_normal((B, 1, n)), 0.3 * rng.standard_normal((B, 1, m))
    return rng.standard_normal((B, T + 1, n)), 0.3 * rng.standard_normal((B, T, m))


def _dev(a, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda") if dtype is None else torch.as_tensor(a, dtype=dtype, device="cuda")


def _linesearch(_lib, model, cost, x0, l, L, xp, up, ids=None, act=None, n_alpha=16):
    """the array-level line search on a QuadraticCost or a TrackingCost; untouched rows keep the fill value 7"""
    import torch
    from zopt_amd import models
    lib = _lib.lib()
    B, T, m, n = L.shape
    tracking = isinstance(cost, models.TrackingCost)
    md, cs = model.c_struct(), (cost.track_struct((B,), T) if tracking else cost.c_struct())
    d = [_dev(a) for a in (x0, l, L, xp, up, 0.5 ** np.arange(n_alpha))]
    xT, uT, J = (torch.full(s, 7.0, dtype=torch.float64, device="cuda") for s in ((B, T + 1, n), (B, T, m), (B,)))
    idx = torch.full((B,), 77, dtype=torch.int32, device="cuda")
    p = lambda t: None if t is None else t.data_ptr()
    dact = None if act is None else _dev(act, torch.int32)
    head = (ctypes.addressof(md), ctypes.addressof(cs)) + tuple(p(t) for t in d) + (n_alpha,)
    tail = (p(xT), p(uT), p(J), p(idx), B, T, None)
    if ids is None:
        fn = lib.zm_rollout_linesearch_tracking_f64 if tracking else lib.zm_rollout_linesearch_f64
        rc = fn(*head, p(dact), *tail)
    else:
        dids = _dev(ids, torch.int32)
        fn = lib.zm_rollout_linesearch_tracking_list_f64 if tracking else lib.zm_rollout_linesearch_list_f64
        rc = fn(*head, p(dids), len(ids), p(dact), *tail)
    assert rc == 0, lib.zm_last_error()
    torch.cuda.synchronize()
    return xT.cpu().numpy(), uT.cpu().numpy(), J.cpu().numpy(), idx.cpu().numpy()


def _expansion(_lib, cost, xT, uT, ids=None, act=None):
    """the array-level cost expansion -> (c, c_x, c_u, v, v_x, c_xx, c_ux, c_uu, v_xx); untouched rows keep 7"""
    import torch
    from zopt_amd import models
    lib = _lib.lib()
    B, T, m = uT.shape
    n = xT.shape[-1]
    tracking = isinstance(cost, models.TrackingCost)
    cs = cost.track_struct((B,), T) if tracking else cost.c_struct()
    dx, du = _dev(xT), _dev(uT)
    outs = [torch.full(s, 7.0, dtype=torch.float64, device="cuda") for s in ((B, T), (B, T, n), (B, T, m), (B,), (B, n), (n, n), (m, n),
                                                                             (m, m), (n, n))]
    p = lambda t: None if t is None else t.data_ptr()
    dact = None if act is None else _dev(act, torch.int32)
    if ids is None:
        fn = lib.zm_quadratize_cost_tracking_f64 if tracking else lib.zm_quadratize_cost_f64
        rc = fn(ctypes.addressof(cs), n, m, p(dx), p(du), p(dact), *[p(o) for o in outs], B, T, None)
    else:
        dids = _dev(ids, torch.int32)
        fn = lib.zm_quadratize_cost_tracking_list_f64 if tracking else lib.zm_quadratize_cost_list_f64
        rc = fn(ctypes.addressof(cs), n, m, p(dx), p(du), p(dids), len(ids), p(dact), *[p(o) for o in outs], B, T, None)
    assert rc == 0, lib.zm_last_error()
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


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


# ------------------------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("diag", [1, 0], ids=["diagonal", "full"])
@pytest.mark.parametrize("name", ["quad", "lin12", "rb", "lin3"])
def test_zero_reference_gives_the_QuadraticCost_results_bit_for_bit(mods, name, diag):
    """zero arrays in every layout, and None: line search, expansion, iterativeLqr and differentialDynamicProgramming return what the
    QuadraticCost calls return on the same inputs -- array_equal on every output, the J / step-index trace included"""
    ilqr, models, _, _lib = mods
    model, _, n, m = _model(models, name)
    Q, R, Qf = _weights(n, m, diag)
    qc = models.QuadraticCost(Q, R, Qf)
    rng = np.random.default_rng(11)
    for T, B in zip(TS, (5, 9, 5, 9, 5, 9)):
        zeros = [models.TrackingCost(Q, R, Qf), models.TrackingCost(Q, R, Qf, np.zeros(n), np.zeros(m)),
                 models.TrackingCost(Q, R, Qf, np.zeros((B, 1, n)), None), models.TrackingCost(Q, R, Qf, None, np.zeros((B, T, m))),
                 models.TrackingCost(Q, R, Qf, np.zeros((B, T + 1, n)), np.zeros((B, T, m)))]
        pt = _point(rng, name, B, T, n, m)
        ref_ls = _linesearch(_lib, model, qc, *pt)
        ref_one = _linesearch(_lib, model, qc, *pt, n_alpha=1)
        xT, uT = ref_ls[0], ref_ls[1]
        ref_ex = _expansion(_lib, qc, xT, uT)
        for tc in zeros:
            for a, b in zip(_linesearch(_lib, model, tc, *pt), ref_ls):
                assert np.array_equal(a, b), (T, B)
            for a, b in zip(_linesearch(_lib, model, tc, *pt, n_alpha=1), ref_one):
                assert np.array_equal(a, b), (T, B)
            for a, b in zip(_expansion(_lib, tc, xT, uT), ref_ex):
                assert np.array_equal(a, b), (T, B)
    if name == "rb":
        return                                                     # (the rigid body is here for the generic kernels; the solves below take the other three)
    T, B = 7, 5
    x0 = 0.3 * rng.standard_normal((B, n))
    ug = np.tile(np.array([9.807, 0, 0, 0]) if name == "quad" else np.zeros(m), (B, T, 1))
    for ddp in (False, True):
        ref = _solve(ilqr, model, qc, x0, ug, ddp, maxIter=5, tol=1e-6)
        for tc in (models.TrackingCost(Q, R, Qf), models.TrackingCost(Q, R, Qf, np.zeros((B, 1, n)), np.zeros(m)),
                   models.TrackingCost(Q, R, Qf, np.zeros((B, T + 1, n)), np.zeros((B, T, m)))):
            for a, b in zip(_solve(ilqr, model, tc, x0, ug, ddp, maxIter=5, tol=1e-6), ref):
                assert np.array_equal(a, b, equal_nan=True), (ddp,)


# ------------------------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("diag", [1, 0], ids=["diagonal", "full"])
@pytest.mark.parametrize("name", ["quad", "lin12", "rb", "lin3"])
def test_line_search_and_expansion_against_the_restatement(mods, name, diag):
    """nonzero references: the winner's index exactly; J at 1e-10 and the trajectory at 1e-9 (tests/test_rollout_gpu.py's bounds for
    the QuadraticCost line search), c, c_x, c_u, v, v_x at 1e-13 (tests/test_ilqr_solve_gpu.py's for the QuadraticCost expansion)"""
    _, models, _, _lib = mods
    model, step, n, m = _model(models, name)
    Q, R, Qf = _weights(n, m, diag)
    rng = np.random.default_rng(12 + diag)
    for T, B, layout in zip(TS, (5, 9, 5, 9, 5, 9), ("shared", "goal", "full", "full", "goal", "full")):
        xRef, uRef = _reference(rng, layout, B, T, n, m)
        tc = models.TrackingCost(Q, R, Qf, xRef, uRef)
        x0, l, L, xp, up = _point(rng, name, B, T, n, m)
        xT, uT, J, idx = _linesearch(_lib, model, tc, x0, l, L, xp, up)
        c, c_x, c_u, v, v_x, c_xx, c_ux, c_uu, v_xx = _expansion(_lib, tc, xT, uT)
        assert np.array_equal(c_xx, Q + Q.T) and np.array_equal(c_uu, R + R.T) and np.array_equal(v_xx, Qf + Qf.T) and not c_ux.any()
        for b in range(B):
            xr, ur = tref.full_reference(xRef, uRef, T, n, m, b)
            rt, rJ, ridx, rJs = tref.forward_pass(x0[b], step, Q, R, Qf, xr, ur, zo.AffinePolicy(l[b], L[b]), zo.Trajectory(xp[b], up[b]))
            assert idx[b] == ridx, (T, B, layout, b, rJs)
            assert abs(J[b] - rJ) <= 1e-10 * abs(rJ), (T, B, layout, b)
            assert _rel(xT[b], rt.xTraj) <= 1e-9 and _rel(uT[b], rt.uTraj) <= 1e-9
            ex = tref.cost_expansion(Q, R, xr, ur, zo.Trajectory(xT[b], uT[b]))
            vf = tref.terminal_expansion(Qf, xr, xT[b, -1])
            assert _rel(c[b], ex.c) <= 1e-13 and _rel(c_x[b], ex.c_x) <= 1e-13 and _rel(c_u[b], ex.c_u) <= 1e-13, (T, B, layout, b)
            assert abs(v[b] - vf.v) <= 1e-13 * abs(vf.v) and _rel(v_x[b], vf.v_x) <= 1e-13, (T, B, layout, b)


# ------------------------------------------------------------------------------------------------------------------------------- 3
def _agreement(J_gpu, a_gpu, trace, rtol=1e-9):
    """the rule of tests/test_ilqr_solve_gpu.py: leading iterations in which the kernel's cost after the acceptance step (to `rtol`,
    NaN == NaN) and its winning step-size index (exactly) agree with the restatement's"""
    k = 0
    for (Jo, idx, _), Jg, ag in zip(trace, J_gpu, a_gpu):
        same_J = (np.isnan(Jo) and np.isnan(Jg)) or (Jo == Jg) or (np.isfinite(Jo) and np.isfinite(Jg) and abs(Jo - Jg) <= rtol * abs(Jo))
        if not (same_J and int(ag) == idx):
            break
        k += 1
    return k


def _solve_case(models, case):
    rng = np.random.default_rng(31)
    if case == "quad_goals":            # per-trajectory goals on the quadcopter, uRef = uTrim
        model, step, n, m = _model(models, "quad")
        T, B = 7, 5
        Q, R, Qf = np.eye(n), 0.5 * np.eye(m), 10 * np.eye(n)
        x0 = np.zeros((B, n))
        x0[:, 9:12] = rng.uniform(-3, 3, (B, 3))
        goal = np.zeros((B, 1, n))
        goal[:, 0, 9:12] = rng.uniform(-2, 2, (B, 3))
        return model, step, (Q, R, Qf), goal, models.QuadcopterEuler.uTrim, x0, np.tile(models.QuadcopterEuler.uTrim, (B, T, 1)), dict(maxIter=8, tol=1e-3)
    if case == "lin3_ramp":             # a ramp reference on the (3, 2) linear model, full weights.  One iteration: it solves an LQ problem, and
        # a second one would search among 16 costs that are equal to rounding -- its argmin is noise in any implementation
        model, step, n, m = _model(models, "lin3")
        T, B = 7, 5
        Q, R, Qf = _weights(n, m, 0)
        ramp = np.linspace(0, 1, T + 1)[None, :, None] * rng.standard_normal((B, 1, n))
        return model, step, (Q, R, Qf), ramp, 0.2 * rng.standard_normal((B, T, m)), rng.standard_normal((B, n)), np.zeros((B, T, m)), dict(maxIter=1, tol=1e-9)
    # a start that does not converge within maxIter: large attitude and rates, a far goal, a tolerance it cannot reach
    model, step, n, m = _model(models, "quad")
    T, B = 7, 5
    Q, R, Qf = np.eye(n), 0.5 * np.eye(m), 10 * np.eye(n)
    x0 = np.zeros((B, n))
    x0[:, 3:9] = rng.uniform(-1.0, 1.0, (B, 6))
    x0[:, 9:12] = rng.uniform(-8, 8, (B, 3))
    goal = np.zeros((B, 1, n))
    goal[:, 0, 9:12] = rng.uniform(-8, 8, (B, 3))
    return model, step, (Q, R, Qf), goal, models.QuadcopterEuler.uTrim, x0, np.tile(models.QuadcopterEuler.uTrim, (B, T, 1)), dict(maxIter=10, tol=1e-13)


@pytest.mark.parametrize("case", ["quad_goals", "lin3_ramp", "non_converging"])
def test_solves_follow_the_restatement_iteration_by_iteration(mods, case):
    """zm_ilqr_solve_tracking_trace_f64 against the restatement: the cost to 1e-9 relative and the step index exactly for as many
    iterations as the two agree, and that count at least what the same check reaches for the QuadraticCost twin of the case (the same
    problem with a zero reference, kernel against oracle.zopt_oracle.iterativeLqr) -- measured here, per trajectory."""
    import warnings
    ilqr, models, _, _ = mods
    model, step, (Q, R, Qf), xRef, uRef, x0, ug, kw = _solve_case(models, case)
    B, T, m = ug.shape
    n = x0.shape[-1]
    xT, uT, L, J, conv, Jtr, atr = _solve(ilqr, model, models.TrackingCost(Q, R, Qf, xRef, uRef), x0, ug, **kw)
    _, _, _, Jq, convq, Jtrq, atrq = _solve(ilqr, model, models.QuadraticCost(Q, R, Qf), x0, ug, **kw)
    report = []
    for b in range(B):
        xr, ur = tref.full_reference(xRef, uRef, T, n, m, b)
        tr, trq = [], []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            rt, rL, rJ, rc, its = tref.iterativeLqr(step, Q, R, Qf, xr, ur, x0[b], ug[b], return_iters=True, trace=tr, **kw)
            _, _, _, rcq, itsq = zo.iterativeLqr(step, Q, R, Qf, x0[b], ug[b], return_iters=True, trace=trq, **kw)
        agree, twin = _agreement(Jtr[:, b], atr[:, b], tr), _agreement(Jtrq[:, b], atrq[:, b], trq)
        report.append((b, agree, its, twin, itsq))
        assert agree >= 1 and agree >= min(twin, its), (case, report)
        if agree == its:                                        # together to the end: the same answer
            assert bool(conv[b]) == rc and abs(J[b] - rJ) <= 1e-7 * abs(rJ), (case, b)
            assert _rel(uT[b], rt.uTraj) <= 1e-6 and _rel(L[b], rL) <= 1e-5, (case, b)
        if case == "non_converging":
            assert not conv[b] and not rc and its == kw["maxIter"]
    print(f"tracking solve {case}: (trajectory, iterations in agreement, restatement iterations, twin's agreement, twin's iterations)", report)


# ------------------------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("name", ["quad", "lin3"])
def test_list_form_against_dense_form(mods, name):
    """an id list with gaps and an `active` mask: listed, active trajectories get bit for bit what the dense call writes (the
    reference is read by trajectory id, not by slot), every other row is left untouched"""
    _, models, _, _lib = mods
    model, _, n, m = _model(models, name)
    rng = np.random.default_rng(41)
    B, T = 9, 5
    Q, R, Qf = _weights(n, m, 0)
    tc = models.TrackingCost(Q, R, Qf, *_reference(rng, "full", B, T, n, m))
    pt = _point(rng, name, B, T, n, m)
    dense = _linesearch(_lib, model, tc, *pt)
    ids, act = [7, 2, 5, 0], np.ones(B, dtype=np.int32)
    act[5] = 0
    part = _linesearch(_lib, model, tc, *pt, ids=ids, act=act)
    dex = _expansion(_lib, tc, dense[0], dense[1])
    pex = _expansion(_lib, tc, dense[0], dense[1], ids=ids, act=act)
    for b in range(B):
        for a, d in list(zip(part, dense)) + list(zip(pex[:5], dex[:5])):
            if b in (7, 2, 0):
                assert np.array_equal(a[b], d[b]), b
            else:
                assert np.all(a[b] == (77 if a.dtype == np.int32 else 7.0)), b
    masked = _linesearch(_lib, model, tc, *pt, act=act)
    assert np.array_equal(masked[2][act == 1], dense[2][act == 1]) and masked[2][5] == 7.0


def test_a_batch_member_solved_alone(mods):
    ilqr, models, _, _ = mods
    for name, (mk_model, mk_cost, x0, ug, ddp) in child.cases().items():
        model, cost = mk_model(), mk_cost()
        full = _solve(ilqr, model, cost, x0, ug, bool(ddp), maxIter=6, tol=1e-9)
        for b in (0, 3):
            xr = cost.xRef if cost.xRef.ndim == 1 else cost.xRef[b:b + 1]
            ur = cost.uRef if (cost.uRef is None or cost.uRef.ndim == 1) else cost.uRef[b:b + 1]
            alone = _solve(ilqr, model, models.TrackingCost(cost.Q, cost.R, cost.Qf, xr, ur), x0[b:b + 1], ug[b:b + 1], bool(ddp),
                           maxIter=6, tol=1e-9)
            for a, f in zip(alone[:5], full[:5]):
                assert np.array_equal(a[0], f[b], equal_nan=True), (name, b)
            its = alone[5].shape[0]
            assert np.array_equal(alone[5][:, 0], full[5][:its, b], equal_nan=True), (name, b)


@pytest.mark.parametrize("env", [{"ZOPT_AMD_ILQR_TAIL": "0"}, {"ZOPT_AMD_EXPAND": "group"}], ids=["two-pass", "16-lane-expansion"])
def test_kernel_forms_against_each_other(mods, env, tmp_path):
    """The default solve of a small batch runs the line search in its all-store form and the quadcopter's expansion one lane per
    point; ZOPT_AMD_ILQR_TAIL=0 keeps the two-pass form, ZOPT_AMD_EXPAND=group the 16-lane expansion (switches of the -DZM_LAB build,
    read once per process: hence a child process).  Bit for bit the same solves, traces included."""
    ilqr = mods[0]
    lab = dict(os.environ, ZOPT_AMD_LIB=os.path.join(ROOT, "zopt_amd", "csrc", "libzopt_amd_lab.so"), **env)
    out = tmp_path / "forms.npz"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ilqr_tracking_child.py"), str(out)], env=lab, capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0 and "TRACKING-CHILD-OK" in p.stdout, (p.stdout[-500:], p.stderr[-1500:])
    other = np.load(out)
    here = {}
    for name, case in child.cases().items():
        here.update(child.run(name, case))
    assert sorted(other.files) == sorted(here)
    for key in here:
        assert np.array_equal(other[key], here[key], equal_nan=True), key


# ------------------------------------------------------------------------------------------------------------------------------- 5
def test_constant_goal_against_the_generic_path(mods):
    """a constant goal on a small problem: the fused path with a TrackingCost against the generic path with torch callables closing
    over the same goal -- at tests/test_generic_gpu.py's bounds for its fused-against-generic comparison (J 1e-7, trajectory 1e-6,
    gains 1e-5, each there against the common oracle loop)"""
    import torch
    ilqr, models, _, _ = mods
    rng = np.random.default_rng(51)
    n, m, T, B = 3, 2, 6, 4
    A, Bm = np.eye(n) + 0.05 * rng.standard_normal((n, n)), 0.3 * rng.standard_normal((n, m))
    Q, R, Qf = np.eye(n), 0.5 * np.eye(m), 5 * np.eye(n)
    goal, uh = rng.standard_normal(n), 0.2 * rng.standard_normal(m)
    x0, ug = rng.standard_normal((B, n)), np.zeros((B, T, m))
    fused = ilqr.iterativeLqr(models.LinearModel(A, Bm), *(models.TrackingCost(Q, R, Qf, goal, uh),) * 2, x0, ug)
    tA, tB, tQ, tR, tQf, tg, tu = (torch.as_tensor(a, device="cuda") for a in (A, Bm, Q, R, Qf, goal, uh))
    gen = ilqr.iterativeLqr(lambda x, u: tA @ x + tB @ u, lambda x, u: (x - tg) @ tQ @ (x - tg) + (u - tu) @ tR @ (u - tu),
                            lambda x: (x - tg) @ tQf @ (x - tg), x0, ug)
    assert np.array_equal(fused[3], gen[3]) and fused[3].all()
    assert np.max(np.abs(fused[2] - gen[2]) / np.abs(gen[2])) <= 1e-7
    assert _rel(fused[0].xTraj, gen[0].xTraj) <= 1e-6 and _rel(fused[0].uTraj, gen[0].uTraj) <= 1e-6 and _rel(fused[1], gen[1]) <= 1e-5
    J0 = [tref.trajectory_cost(Q, R, Qf, *tref.full_reference(goal, uh, T, n, m), zo.trajectoryRollout(
        x0[b], lambda x, u: A @ x + Bm @ u, zo.AffinePolicy(ug[b], np.zeros((T, m, n))), zo.Trajectory(np.zeros((T + 1, n)), np.zeros((T, m)))))
        for b in range(B)]
    assert np.all(fused[2] < np.array(J0))                      # it steered towards the goal, not towards the origin


# ------------------------------------------------------------------------------------------------------------------------------- 6
def test_ddp_with_a_goal(mods):
    """differentialDynamicProgramming with per-trajectory goals: J never increases along the iterations, the returned J is the
    restatement's cost of the returned trajectory, and the cost expansion at it (pytrees, i.e. the tracking kernels) is the
    restatement's -- with a gradient that has become small where the solve converged (stationarity)"""
    ilqr, models, pytrees, _ = mods
    model, step, (Q, R, Qf), goal, uRef, x0, ug, _ = _solve_case(models, "quad_goals")
    B, T, m = ug.shape
    n = 12
    tc = models.TrackingCost(Q, R, Qf, goal, uRef)
    xT, uT, L, J, conv, Jtr, atr = _solve(ilqr, model, tc, x0, ug, ddp=True, maxIter=50, tol=1e-6)
    assert conv.all()
    first = np.array([tref.trajectory_cost(Q, R, Qf, *tref.full_reference(goal, uRef, T, n, m, b), zo.trajectoryRollout(
        x0[b], step, zo.AffinePolicy(ug[b], np.zeros((T, m, n))), zo.Trajectory(np.zeros((T + 1, n)), np.zeros((T, m))))) for b in range(B)])
    hist = np.vstack([first[None], Jtr])
    assert np.all(np.diff(hist, axis=0) <= 1e-12 * np.abs(hist[:-1]))
    qc = pytrees.QuadraticCostFunction.from_trajectory(tc, pytrees.Trajectory(xT, uT))
    vf = pytrees.QuadraticValueFunction.fromTerminalCostFunction(tc, xT[:, -1])
    Jc = tc(pytrees.Trajectory(xT, uT))                            # cost(traj) and cost(traj, k): CostFunction.__call__ on the tracking kernels
    assert Jc.shape == J.shape and np.max(np.abs(Jc - J) / np.abs(J)) <= 1e-10
    assert np.array_equal(tc(pytrees.Trajectory(xT, uT), 2), qc.c[:, 2])
    for b in range(B):
        xr, ur = tref.full_reference(goal, uRef, T, n, m, b)
        assert abs(J[b] - tref.trajectory_cost(Q, R, Qf, xr, ur, zo.Trajectory(xT[b], uT[b]))) <= 1e-10 * abs(J[b])
        ex = tref.cost_expansion(Q, R, xr, ur, zo.Trajectory(xT[b], uT[b]))
        tv = tref.terminal_expansion(Qf, xr, xT[b, -1])
        assert _rel(qc.c_x[b], ex.c_x) <= 1e-13 and _rel(qc.c_u[b], ex.c_u) <= 1e-13 and _rel(qc.c[b], ex.c) <= 1e-13
        assert _rel(vf.v_x[b], tv.v_x) <= 1e-13 and abs(vf.v[b] - tv.v) <= 1e-13 * abs(tv.v)
        # stationarity: one more backward pass at the returned trajectory proposes (almost) no change of the controls
        dyn = zo.affine_dynamics_from_trajectory(step, zo.Trajectory(xT[b], uT[b]))
        pol = zo.backwardPass_ilqr(dyn, zo.conditionQuadraticCost(ex), zo.conditionValueFunction(tv))
        assert np.max(np.abs(pol.l)) <= 1e-2 * max(1.0, np.max(np.abs(uT[b] - uRef)))
