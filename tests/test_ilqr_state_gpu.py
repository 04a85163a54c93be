"""GPU tests of the state box (models.StateBox, zm_statebox_t): the penalty line search (rollout.hip), the penalty expansion and the
multiplier update (state_box.hip), the sweep with the diagonal addend (ilqr_backward.hip) and the augmented-Lagrangian solve
(ilqr_solve.hip), against NumPy, against the existing entries they must reduce to, and against the restatement
(tests/ilqr_state_ref.py) outer iteration by outer iteration.

Shapes are the smallest that reach the kernels' seams: (n, m) in {(2, 1), (4, 1), (5, 2), (8, 4), (12, 4)} (KS = 1, 2, 3 and ragged
tiles), T in {1, 2, 3, 4, 5, 8} (every exit of the sweep's two-step prefetch loop; at T = 1 only the terminal row is constrained),
batches of 5 with a permuted id list and a mask with holes, shared and per-trajectory bounds, infinite sides and lb == ub."""
import ctypes

import numpy as np
import pytest

from oracle import zopt_oracle as zo
from tests import hp_reference as hp
from tests import ilqr_box_cases as bcases
from tests import ilqr_box_ref as br
from tests import ilqr_state_cases as cases
from tests import ilqr_state_ref as sref
from tests import ilqr_tracking_ref as tref
from tests import linesearch_hp_ref as lhp
from tests.test_ilqr_box_gpu import _box, _box_linesearch, _box_sweep, _p, _pattern
from tests.test_ilqr_tracking_gpu import _dev, _linesearch, _rel

pytestmark = pytest.mark.gpu
INF = np.inf
SHAPES = ((2, 1), (4, 1), (5, 2), (8, 4), (12, 4))
TS = (1, 2, 3, 4, 5, 8)
ULP = 2.0 ** -52


@pytest.fixture(scope="module")
def mods():
    import torch
    assert torch.cuda.is_available()
    from zopt_amd import _lib, ilqrUtils, models, pytrees
    return ilqrUtils, models, pytrees, _lib


def _bounds(rng, B, n, per_traj):
    """walls about the origin with an infinite lower side on component 0, an infinite upper side on the last and lb == ub on
    component 1 (where there is one)"""
    shp = (B, n) if per_traj else (n,)
    lb, ub = -rng.uniform(0.1, 0.6, shp), rng.uniform(0.1, 0.6, shp)
    lb[..., 0] = -INF
    ub[..., -1] = INF
    if n > 2:
        ub[..., 1] = lb[..., 1]
    return lb, ub


def _statebox(models, lb, ub, lam_lb, lam_ub, mu, n):
    d = [_dev(np.asarray(a, dtype=np.float64)) for a in (lb, ub, lam_lb, lam_ub, mu)]
    return models.zm_statebox_t(d[0].data_ptr(), d[1].data_ptr(), 0 if np.ndim(lb) == 1 else n, d[2].data_ptr(), d[3].data_ptr(),
                                d[4].data_ptr()), d


# ------------------------------------------------------------------------------------------------ 1  expansion add-on, multiplier update
@pytest.mark.parametrize("n", [2, 5, 12])
@pytest.mark.parametrize("per_traj", [False, True])
def test_penalty_expansion_and_multiplier_update_against_numpy(mods, n, per_traj):
    """g, h and the updated multipliers to 4 ulp of the largest term of each entry; the active pattern, the done flags and the masks
    exactly; rows of unlisted / masked / done trajectories and row 0 bitwise untouched.  T = 1 (terminal row only) and T = 3."""
    import torch
    _, models, _, _lib = mods
    lib = _lib.lib()
    B = 5
    for T in (1, 3):
        rng = np.random.default_rng(10 * n + T + per_traj)
        lb, ub = _bounds(rng, B, n, per_traj)
        x = rng.standard_normal((B, T + 1, n))
        lbb, ubb = np.broadcast_to(lb, (B, n))[:, None], np.broadcast_to(ub, (B, n))[:, None]
        x[0, 1, -1], x[4, 1, -1] = lbb[0, 0, -1] - 0.5, lbb[4, 0, -1] - 0.25             # 0 and 4 violate a wall
        x[3, 1:] = np.clip(x[3, 1:], np.where(np.isfinite(lbb[2]), lbb[2], -9), np.where(np.isfinite(ubb[2]), ubb[2], 9))   # feasible for 2
        mu = 10.0 ** rng.uniform(0, 8, B)
        lam_lb, lam_ub = (np.where(rng.random((B, T + 1, n)) < 0.5, 0.0, 10.0 ** rng.uniform(-2, 8, (B, T + 1, n))) for _ in range(2))
        lam_lb[:, 0], lam_ub[:, 0] = 0.0, 0.0
        su, sl = sref.slacks(x, lbb, ubb, lam_lb, lam_ub, mu[:, None, None])
        g = sref.pos(su) - sref.pos(sl)
        h = mu[:, None, None] * ((su > 0).astype(float) + (sl > 0).astype(float))
        g[:, 0], h[:, 0] = 0.0, 0.0
        with np.errstate(invalid="ignore"):
            big = np.maximum(np.abs(lam_ub), np.abs(np.where(np.isfinite(ubb), mu[:, None, None] * (x - ubb), 0)))
            big = np.maximum(big, np.maximum(np.abs(lam_lb), np.abs(np.where(np.isfinite(lbb), mu[:, None, None] * (lbb - x), 0))))
        # (s = lam + mu (x - ub): two roundings of terms as large as `big`, one more in the difference of the two sides)
        ids, act = np.array([4, 0, 2, 3], dtype=np.int32), np.array([1, 1, 1, 0, 1], dtype=np.int32)       # 1: unlisted, 3: masked
        touched = np.array([True, False, True, False, True])
        ss, keep = _statebox(models, lb, ub, lam_lb, lam_ub, mu, n)
        c_x0, v_x0 = rng.standard_normal((B, T, n)), rng.standard_normal((B, n))
        dcx, dvx, dx = _dev(c_x0), _dev(v_x0), _dev(x)
        dh = torch.full((B, T + 1, n), 7.0, dtype=torch.float64, device="cuda")
        dids, dact = _dev(ids), _dev(act)
        rc = lib.zm_state_penalty_expand_list_f64(ctypes.addressof(ss), _p(dx), _p(dids), 4, _p(dact), _p(dcx), _p(dvx), _p(dh), B, T, n, None)
        assert rc == 0, lib.zm_last_error()
        torch.cuda.synchronize()
        cx, vx, hh = dcx.cpu().numpy(), dvx.cpu().numpy(), dh.cpu().numpy()
        assert np.array_equal(cx[~touched], c_x0[~touched]) and np.array_equal(vx[~touched], v_x0[~touched]) and np.all(hh[~touched] == 7.0)
        assert np.array_equal(cx[:, 0], c_x0[:, 0]) if T > 1 else True
        assert np.array_equal(hh[touched], h[touched])                      # mu * {0, 1, 2}: exact, and the pattern s > 0 with it
        gd = np.concatenate([cx[:, 1:] - c_x0[:, 1:], (vx - v_x0)[:, None]], axis=1)
        tol = 4 * ULP * np.maximum(big[:, 1:], np.abs(np.concatenate([c_x0[:, 1:], v_x0[:, None]], axis=1)))
        assert np.all(np.abs(gd - g[:, 1:])[touched] <= tol[touched] + 4 * ULP * np.abs(g[:, 1:])[touched])
        # the multiplier update: 0 active and converged with a violation, 2 active and converged and feasible (3's states, clipped),
        # 1 not active (done before), 3 -> its states moved to 2; 4 active, not converged
        x2 = x.copy()
        x2[2] = x[3]
        dx2 = _dev(x2)
        active, conv = _dev(np.array([1, 0, 1, 0, 1], dtype=np.int32)), _dev(np.array([1, 1, 1, 1, 0], dtype=np.int32))
        viol = torch.full((B,), 7.0, dtype=torch.float64, device="cuda")
        oc, rem = torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
        rc = lib.zm_state_multiplier_update_f64(ctypes.addressof(ss), _p(dx2), _p(active), _p(conv), _p(viol), _p(oc), _p(rem), 1e-4, 10.0,
                                                1e8, 1, B, T, n, None)
        assert rc == 0, lib.zm_last_error()
        torch.cuda.synchronize()
        v_ref = np.array([sref.violation(x2[b], np.broadcast_to(lb, (B, n))[b], np.broadcast_to(ub, (B, n))[b]) for b in range(B)])
        assert v_ref[2] == 0.0 and v_ref[0] > 1e-4 and v_ref[4] > 1e-4
        vd = viol.cpu().numpy()
        assert np.array_equal(vd[[0, 2, 4]], v_ref[[0, 2, 4]]) and vd[1] == 7.0 and vd[3] == 7.0        # a max of exact differences
        assert active.cpu().tolist() == [1, 0, 0, 0, 1] and conv.cpu().tolist() == [0, 1, 1, 1, 0]
        assert oc.cpu().tolist() == [1, 0, 1, 0, 1] and int(rem.cpu()[0]) == 2
        nlu, nll, nmu = keep[3].cpu().numpy(), keep[2].cpu().numpy(), keep[4].cpu().numpy()
        su2, sl2 = sref.slacks(x2, lbb, ubb, lam_lb, lam_ub, mu[:, None, None])
        for b in range(B):
            if b in (0, 4):
                assert np.array_equal(nlu[b, 0], lam_ub[b, 0]) and np.array_equal(nll[b, 0], lam_lb[b, 0])
                assert np.all(np.abs(nlu[b, 1:] - sref.pos(su2[b, 1:])) <= 4 * ULP * big[b, 1:]) and np.array_equal(nlu[b, 1:] > 0, su2[b, 1:] > 0)
                assert np.all(np.abs(nll[b, 1:] - sref.pos(sl2[b, 1:])) <= 4 * ULP * big[b, 1:]) and np.array_equal(nll[b, 1:] > 0, sl2[b, 1:] > 0)
                assert nmu[b] == min(mu[b] * 10.0, 1e8)
            else:
                assert np.array_equal(nlu[b], lam_ub[b]) and np.array_equal(nll[b], lam_lb[b]) and nmu[b] == mu[b]


def test_multiplier_update_nan_state_is_never_done(mods):
    import torch
    _, models, _, _lib = mods
    B, T, n = 2, 3, 4
    x = np.zeros((B, T + 1, n))
    x[1, 2, 1] = np.nan
    ss, keep = _statebox(models, -np.ones(n), np.ones(n), np.zeros((B, T + 1, n)), np.zeros((B, T + 1, n)), np.ones(B), n)
    active, conv = _dev(np.ones(B, dtype=np.int32)), _dev(np.ones(B, dtype=np.int32))
    viol = torch.zeros(B, dtype=torch.float64, device="cuda")
    dx = _dev(x)
    assert _lib.lib().zm_state_multiplier_update_f64(ctypes.addressof(ss), _p(dx), _p(active), _p(conv), _p(viol), None, None, 1e-4, 10.0,
                                                     1e8, 1, B, T, n, None) == 0
    torch.cuda.synchronize()
    v = viol.cpu().numpy()
    assert v[0] == 0.0 and np.isnan(v[1]) and conv.cpu().tolist() == [1, 0] and active.cpu().tolist() == [0, 1]


# ------------------------------------------------------------------------------------------------------------------------- 2  the sweep
def _state_sweep(_lib, models, dyn, cost, Vf, h, u=None, lb=None, ub=None, ids=None, act=None, shared=False):
    """zm_ilqr_backward_state[_list]_f64 -> (l, L); untouched rows keep the fill value 7"""
    import torch
    lib = _lib.lib()
    B, T, n, m = np.asarray(dyn[2]).shape
    ops = [dyn[1], dyn[2], cost[1], cost[2], cost[3], cost[4], cost[5], Vf[1], Vf[2], h]
    if shared:
        ops[4:7] = [np.asarray(cost[i])[0, 0] for i in (3, 4, 5)]
        ops[8] = np.asarray(Vf[2])[0]
    d = [_dev(np.asarray(a, dtype=np.float64)) for a in ops]
    du = None if u is None else _dev(np.asarray(u, dtype=np.float64))
    bs, keep = (None, None) if u is None else _box(models, lb, ub, m)
    l = torch.full((B, T, m), 7.0, dtype=torch.float64, device="cuda")
    L = torch.full((B, T, m, n), 7.0, dtype=torch.float64, device="cuda")
    dids = None if ids is None else _dev(np.asarray(ids), torch.int32)
    dact = None if act is None else _dev(act, torch.int32)
    rc = lib.zm_ilqr_backward_state_list_f64(*[_p(t) for t in d], _p(du), None if bs is None else ctypes.addressof(bs), _p(dids),
                                             0 if ids is None else len(ids), _p(dact), 1 if shared else 0, _p(l), _p(L), None, B, T, n, m, None)
    assert rc == 0, lib.zm_last_error()
    torch.cuda.synchronize()
    return l.cpu().numpy(), L.cpu().numpy()


def _sweep_problem(n, m, T, B, seed):
    """a tame sweep problem with a diagonal addend whose entries run from 0 to 1e8 (a third of them exactly 0)"""
    rng = np.random.default_rng(seed)
    f_x = np.eye(n) + 0.2 * rng.standard_normal((B, T, n, n))
    f_u = 0.5 * rng.standard_normal((B, T, n, m))
    M = rng.standard_normal((B, T, n + m, n + m))
    H = M @ np.swapaxes(M, -1, -2) / (n + m) + np.eye(n + m)
    Mf = rng.standard_normal((B, n, n))
    dyn = (None, f_x, f_u)
    cost = (None, rng.standard_normal((B, T, n)), rng.standard_normal((B, T, m)), H[..., :n, :n].copy(), H[..., n:, :n].copy(), H[..., n:, n:].copy())
    Vf = (None, rng.standard_normal((B, n)), Mf @ np.swapaxes(Mf, -1, -2) / n + np.eye(n))
    h = np.where(rng.random((B, T + 1, n)) < 1 / 3, 0.0, 10.0 ** rng.uniform(-3, 8, (B, T + 1, n)))
    h[:, 0] = 0.0
    return dyn, cost, Vf, h


def _materialised(cost, Vf, h):
    T = cost[3].shape[1]
    c_xx = cost[3] + np.stack([np.stack([np.diag(hk) for hk in hb[:T]]) for hb in h])
    v_xx = Vf[2] + np.stack([np.diag(hb[T]) for hb in h])
    return cost[:3] + (c_xx,) + cost[4:], Vf[:2] + (v_xx,)


@pytest.mark.parametrize("shape", SHAPES)
def test_state_sweep_with_the_box_gives_the_bits_of_the_box_sweep_on_the_materialised_hessians(mods, shape):
    """the box + penalty kernel against zm_ilqr_backward_box_f64 with per-step Hessians c_xx + diag h_k (shared_hessian = 0) and the
    terminal v_xx + diag h_T: the same register kernel body, the addend formed before anything is accumulated onto it -- equal bits,
    at every T of the prefetch loop's exits; with a permuted list and a mask with holes only the listed, active rows are written"""
    _, models, _, _lib = mods
    n, m = shape
    B = 5
    clamped = 0
    for T in TS:
        dyn, cost, Vf, h = _sweep_problem(n, m, T, B, 100 * n + T)
        rng = np.random.default_rng(T)
        u = 0.05 * rng.standard_normal((B, T, m))
        lb, ub = -rng.uniform(0.05, 0.2, (B, m)), rng.uniform(0.05, 0.2, (B, m))
        costm, Vfm = _materialised(cost, Vf, h)
        ref_l, ref_L, _ = _box_sweep(_lib, models, dyn, costm, Vfm, u, lb, ub)
        l, L = _state_sweep(_lib, models, dyn, cost, Vf, h, u, lb, ub)
        assert np.array_equal(l, ref_l) and np.array_equal(L, ref_L), (shape, T)
        clamped += int(np.count_nonzero(_pattern(L)))
        ids, act = [3, 0, 4, 1], np.array([1, 0, 1, 1, 1], dtype=np.int32)            # 2 unlisted, 1 masked
        pl, pL = _state_sweep(_lib, models, dyn, cost, Vf, h, u, lb, ub, ids=ids, act=act)
        for b in range(B):
            assert (np.array_equal(pl[b], l[b]) and np.array_equal(pL[b], L[b])) if b in (3, 0, 4) else (np.all(pl[b] == 7.0) and np.all(pL[b] == 7.0))
    assert clamped > 0, "no clamped input at any horizon: the cases do not reach the box step"


@pytest.mark.parametrize("shape", SHAPES)
def test_state_sweep_with_a_zero_addend_and_shared_hessians_gives_the_bits_of_the_box_sweep(mods, shape):
    """h = 0 on the solver's layout (one shared Hessian set): the bits of zm_ilqr_backward_box_f64"""
    _, models, _, _lib = mods
    n, m = shape
    for T in (1, 4, 5):
        dyn, cost, Vf, h = _sweep_problem(n, m, T, 5, 7 * n + T)
        u, lb, ub = np.zeros((5, T, m)), np.full(m, -0.3), np.full(m, 0.4)
        ref_l, ref_L, _ = _box_sweep(_lib, models, dyn, cost, Vf, u, lb, ub, shared=True)
        l, L = _state_sweep(_lib, models, dyn, cost, Vf, np.zeros_like(h), u, lb, ub, shared=True)
        assert np.array_equal(l, ref_l) and np.array_equal(L, ref_L), (shape, T)


@pytest.mark.parametrize("shape", SHAPES)
def test_state_sweep_without_a_box_against_the_long_double_sweep(mods, shape):
    """the penalty kernel without a box against hp.ilqr_backward_ld on the materialised Hessians, under hp.sweep_bounds (100 x the fp64
    oracle's own error on the same inputs; the plain family's part is the oracle's error on the same problem with h = 0), and against
    the existing per-step-Hessian call (zm_ilqr_backward_list_f64, shared_hessian = 0) under the same bound"""
    import torch
    _, models, _, _lib = mods
    lib = _lib.lib()
    n, m = shape
    B = 5
    report = []
    for T in TS:
        dyn, cost, Vf, h = _sweep_problem(n, m, T, B, 100 * n + T)
        costm, Vfm = _materialised(cost, Vf, h)
        ref = hp.ilqr_backward_ld(dyn, costm, Vfm)
        plain = hp.ilqr_backward_ld(dyn, cost, Vf)
        bound = {}
        o = zo.backwardPass_ilqr(zo.AffineDynamics(None, dyn[1], dyn[2]), zo.QuadraticCostFunction(np.zeros((B, T)), *costm[1:]),
                                 zo.QuadraticValueFunction(np.zeros(B), Vfm[1], Vfm[2]))
        o0 = zo.backwardPass_ilqr(zo.AffineDynamics(None, dyn[1], dyn[2]), zo.QuadraticCostFunction(np.zeros((B, T)), *cost[1:]),
                                  zo.QuadraticValueFunction(np.zeros(B), Vf[1], Vf[2]))
        for key in ("l", "L"):
            bound[key] = hp.sweep_bounds(hp.sweep_metric(getattr(o, key), ref[key]), hp.sweep_metric(getattr(o0, key), plain[key]))
        l, L = _state_sweep(_lib, models, dyn, cost, Vf, h)
        d = [_dev(np.asarray(a)) for a in (dyn[1], dyn[2], costm[1], costm[2], costm[3], costm[4], costm[5], Vfm[1], Vfm[2])]
        pl, pL = torch.empty((B, T, m), dtype=torch.float64, device="cuda"), torch.empty((B, T, m, n), dtype=torch.float64, device="cuda")
        assert lib.zm_ilqr_backward_list_f64(*[_p(t) for t in d], None, 0, None, 0, _p(pl), _p(pL), B, T, n, m, None) == 0
        torch.cuda.synchronize()
        el, eL = float(hp.sweep_metric(l, ref["l"]).max()), float(hp.sweep_metric(L, ref["L"]).max())
        report.append((T, el, bound["l"], eL, bound["L"]))
        assert el <= bound["l"] and eL <= bound["L"], (shape, report[-1])
        assert hp.sweep_metric(pl.cpu().numpy(), ref["l"]).max() <= bound["l"] and hp.sweep_metric(pL.cpu().numpy(), ref["L"]).max() <= bound["L"]
    print(f"state sweep {shape}: (T, error of l, bound, error of L, bound)", report)


# ------------------------------------------------------------------------------------------------------------------- 3  the line search
def _state_linesearch(_lib, models, model, cost, sbox, x0, l, L, xp, up, box=None, ids=None, act=None, n_alpha=16, alphas=None):
    """zm_rollout_linesearch_state[_list]_f64 -> (xTraj, uTraj, J_AL, J_cost, idx); untouched rows keep the fill value 7"""
    import torch
    lib = _lib.lib()
    B, T, m, n = L.shape
    tracking = isinstance(cost, models.TrackingCost)
    md = model.c_struct()
    cs = cost.track_struct((B,), T) if tracking else cost.c_struct()
    pcs = ctypes.addressof(cs)
    bs, keepb = (None, None) if box is None else _box(models, box[0], box[1], m)
    ss, keeps = _statebox(models, *sbox, n)
    if alphas is not None:
        n_alpha = len(alphas)
    d = [_dev(a) for a in (x0, l, L, xp, up, 0.5 ** np.arange(n_alpha) if alphas is None else np.asarray(alphas, dtype=np.float64))]
    xT, uT, J, Jc = (torch.full(s, 7.0, dtype=torch.float64, device="cuda") for s in ((B, T + 1, n), (B, T, m), (B,), (B,)))
    idx = torch.full((B,), 77, dtype=torch.int32, device="cuda")
    dact = None if act is None else _dev(act, torch.int32)
    head = (ctypes.addressof(md), None if tracking else pcs, pcs if tracking else None, None if bs is None else ctypes.addressof(bs),
            ctypes.addressof(ss)) + tuple(_p(t) for t in d) + (n_alpha,)
    tail = (_p(xT), _p(uT), _p(J), _p(Jc), _p(idx), B, T, None)
    if ids is None:
        rc = lib.zm_rollout_linesearch_state_f64(*head, _p(dact), *tail)
    else:
        dids = _dev(np.asarray(ids), torch.int32)
        rc = lib.zm_rollout_linesearch_state_list_f64(*head, _p(dids), len(ids), _p(dact), *tail)
    assert rc == 0, lib.zm_last_error()
    torch.cuda.synchronize()
    return xT.cpu().numpy(), uT.cpu().numpy(), J.cpu().numpy(), Jc.cpu().numpy(), idx.cpu().numpy()


def _ls_problem(models, n, m, T, B, seed):
    rng = np.random.default_rng(seed)
    A, Bm = np.eye(n) + 0.05 * rng.standard_normal((n, n)), 0.3 * rng.standard_normal((n, m))
    x0 = 0.5 * rng.standard_normal((B, n))
    l, L = 0.3 * rng.standard_normal((B, T, m)), 0.05 * rng.standard_normal((B, T, m, n))
    xp, up = 0.1 * rng.standard_normal((B, T + 1, n)), 0.1 * rng.standard_normal((B, T, m))
    Q, R, Qf = np.eye(n) + 0.1 * rng.standard_normal((n, n)), np.eye(m) + 0.1 * rng.standard_normal((m, m)), 5 * np.eye(n)
    return models.LinearModel(A, Bm), (lambda x, u: A @ x + Bm @ u), (Q, R, Qf), x0, l, L, xp, up


@pytest.mark.parametrize("shape", [(2, 1), (5, 2), (8, 4), (12, 4)])
def test_penalty_line_search_with_infinite_bounds_gives_the_bits_of_its_siblings(mods, shape):
    """infinite state bounds and zero multipliers: P is exactly 0.0 -- J_AL, J_cost, the winner's rows and the index are the bits of
    zm_rollout_linesearch_box_f64 (with an input box) and of the tracking entry (without one); at (12, 4) those entries run the fast
    kernel, which accumulates in another order and has no penalty form: there the index, and J and the winner's rows to 1e-12"""
    _, models, _, _lib = mods
    n, m = shape
    B = 5
    for T in (1, 4):
        model, step, (Q, R, Qf), x0, l, L, xp, up = _ls_problem(models, n, m, T, B, 31 * n + T)
        rng = np.random.default_rng(T)
        sbox = (np.full(n, -INF), np.full(n, INF), np.zeros((B, T + 1, n)), np.zeros((B, T + 1, n)), 10.0 ** rng.uniform(0, 8, B))
        for cost in (models.QuadraticCost(Q, R, Qf), models.TrackingCost(Q, R, Qf, rng.standard_normal((B, 1, n)), 0.3 * rng.standard_normal((B, 1, m)))):
            ub = rng.uniform(0.05, 0.3, (B, m))
            ref = _box_linesearch(_lib, models, model, cost, -ub, ub, x0, l, L, xp, up)
            out = _state_linesearch(_lib, models, model, cost, sbox, x0, l, L, xp, up, box=(-ub, ub))
            assert np.array_equal(out[3], out[2])
            if shape == (12, 4):
                assert np.array_equal(out[4], ref[3]) and _rel(out[2], ref[2]) <= 1e-12 and _rel(out[0], ref[0]) <= 1e-12, (shape, T)
            else:
                assert all(np.array_equal(a, b) for a, b in zip((out[0], out[1], out[2], out[4]), ref)), (shape, T)
            ref = _linesearch(_lib, model, cost if isinstance(cost, models.TrackingCost) else models.TrackingCost(Q, R, Qf, None, None), x0, l, L, xp, up)
            out = _state_linesearch(_lib, models, model, cost, sbox, x0, l, L, xp, up)
            if shape == (12, 4):
                assert np.array_equal(out[4], ref[3]) and _rel(out[2], ref[2]) <= 1e-12 and _rel(out[0], ref[0]) <= 1e-12, (shape, T)
            else:
                assert all(np.array_equal(a, b) for a, b in zip((out[0], out[1], out[2], out[4]), ref)) and np.array_equal(out[3], out[2]), (shape, T)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("boxed", [False, True])
def test_penalty_line_search_against_the_restatement(mods, shape, boxed):
    """the 16 costs' minimum, J_cost, the chosen index and the winner's rows against the NumPy restatement (clipped rollouts of
    tests/ilqr_box_ref.py, tests/ilqr_state_ref.penalty) at moderate multipliers: J to 1e-12 relative to the sum of the magnitudes of
    its terms, the index exactly where the restatement's best two costs are 1e-9 apart; a list in permuted order and a mask with holes
    leave the other rows untouched; a trajectory with a NaN x0 wins its own argmin (index 0, NaN costs) next to undisturbed neighbours"""
    _, models, _, _lib = mods
    n, m = shape
    B = 5
    for T in (1, 3, 8):
        model, step, (Q, R, Qf), x0, l, L, xp, up = _ls_problem(models, n, m, T, B, 17 * n + T + boxed)
        rng = np.random.default_rng(T + 5)
        lb, ub = _bounds(rng, B, n, per_traj=bool(T & 1))
        mu = 10.0 ** rng.uniform(0, 3, B)
        lam_lb, lam_ub = (np.where(rng.random((B, T + 1, n)) < 0.5, 0.0, 10.0 ** rng.uniform(-2, 1, (B, T + 1, n))) for _ in range(2))
        lam_lb[:, 0], lam_ub[:, 0] = 0.0, 0.0
        ulb, uub = (-np.full(m, 0.2), np.full(m, 0.25)) if boxed else (np.full(m, -INF), np.full(m, INF))
        cost = models.QuadraticCost(Q, R, Qf)
        x0n = x0.copy()
        x0n[2, 0] = np.nan
        out = _state_linesearch(_lib, models, model, cost, (lb, ub, lam_lb, lam_ub, mu), x0n, l, L, xp, up, box=(ulb, uub) if boxed else None)
        assert out[4][2] == 0 and np.isnan(out[2][2]) and np.isnan(out[3][2])
        xr, ur = np.zeros((T + 1, n)), np.zeros((T, m))
        for b in (0, 1, 3, 4):
            pen = (np.broadcast_to(lb, (B, n))[b], np.broadcast_to(ub, (B, n))[b], lam_lb[b], lam_ub[b], mu[b])
            trj, J, Jc, idx, Js = sref._forward_pass(x0[b], step, Q, R, Qf, xr, ur, zo.AffinePolicy(l[b], L[b]), zo.Trajectory(xp[b], up[b]),
                                                     ulb if boxed else None, uub if boxed else None, pen)
            mag = abs(Jc) + sum(abs(t) for t in (pen[4] * np.max(np.abs(trj.xTraj)) ** 2, np.max(pen[2]) ** 2 / pen[4], np.max(pen[3]) ** 2 / pen[4])) * (T * n)
            srt = np.sort(Js)
            if srt[1] - srt[0] >= 1e-9 * abs(srt[0]):
                assert out[4][b] == idx, (shape, T, b)
                assert abs(out[2][b] - J) <= 1e-12 * mag and abs(out[3][b] - Jc) <= 1e-12 * mag, (shape, T, b, out[2][b], J)
                assert _rel(out[0][b], trj.xTraj) <= 1e-12 and _rel(out[1][b], trj.uTraj) <= 1e-12
        part = _state_linesearch(_lib, models, model, cost, (lb, ub, lam_lb, lam_ub, mu), x0n, l, L, xp, up, box=(ulb, uub) if boxed else None,
                                 ids=[4, 1, 0, 2], act=np.array([1, 0, 1, 1, 1], dtype=np.int32))
        for b in range(B):
            for a, d in zip(part, out):
                assert (np.array_equal(a[b], d[b], equal_nan=True) if b in (4, 0, 2) else np.all(a[b] == (77 if a.dtype == np.int32 else 7.0))), (shape, T, b)


LS_HARD = (("linear", "index_j", 5, 2, 6, 5, None, None, 0), ("linear", "unstable", 12, 4, 8, 5, None, None, 0),
           ("linear", "scaled", 8, 4, 5, 5, None, None, 0), ("linear", "index_j", 4, 1, 3, 5, None, "goal", 0),
           ("quad", "nominal", 3, True), ("quad", "many_turns", 7, False))


@pytest.mark.parametrize("key", LS_HARD, ids=[lhp.key_id(k) for k in LS_HARD])
@pytest.mark.parametrize("boxed", [False, True])
def test_penalty_line_search_against_the_long_double_reference(mods, key, boxed):
    """the hard families of tests/linesearch_hp_ref.py -- linear stable (index_j), unstable and badly scaled, a tracking cost about
    goals 1e6 from the origin, the quadcopter's nominal and many-turns points -- with multipliers and mu up to 1e8 and bounds a few
    units from the states, 1e6 away or infinite (per trajectory), without and with an input box, under that file's `check` rule
    (tests/ilqr_state_ref.check_linesearch): the chosen index inside the candidate set and equal to the argmin where it is determined,
    J_AL and J_cost at that index, the returned rows, the returned trajectory's own J_AL, and the 16 costs of single-step-size calls,
    each within 100 x the fp64 restatement's own worst error on the trajectory (floor 100 x 2^-52) of the long-double values"""
    _, models, _, _lib = mods
    p = lhp.problem(*key)
    pen = sref.linesearch_penalty(p, 1)
    box = None
    if boxed:
        # (linear: the 10 % and 90 % quantiles of the previous inputs per component, so that rollouts clip wherever the inputs lie)
        box = ((np.quantile(p.uPrev, 0.1, axis=(0, 1)), np.quantile(p.uPrev, 0.9, axis=(0, 1))) if p.kind == "linear" else
               (np.array([9.0, -0.5, -0.5, -0.5]), np.array([10.5, 0.5, 0.5, 0.5])))
    ref = sref.PenaltyReference(p, pen, box)
    model = models.QuadcopterEuler(p.dt) if p.kind == "quad" else models.LinearModel(p.A, p.B)
    cost = models.TrackingCost(p.Q, p.R, p.Qf, p.xRef, p.uRef) if p.tracking else models.QuadraticCost(p.Q, p.R, p.Qf)
    xT, uT, J, Jc, idx = _state_linesearch(_lib, models, model, cost, pen, p.x0, p.l, p.L, p.xPrev, p.uPrev, box=box, alphas=p.alphas)
    J16 = np.stack([_state_linesearch(_lib, models, model, cost, pen, p.x0, p.l, p.L, p.xPrev, p.uPrev, box=box, alphas=[a])[2] for a in p.alphas])
    assert np.max(pen[4]) > 1e6 and max(np.max(pen[2]), np.max(pen[3])) > 1e7
    if boxed:
        assert np.all(uT >= box[0]) and np.all(uT <= box[1]) and np.any((uT == box[0]) | (uT == box[1]))
    sref.check_linesearch(ref, xT, uT, J, Jc, idx, J16, what=f"penalty line search {lhp.key_id(key)} boxed={boxed}")


@pytest.mark.parametrize("family", cases.SWEEP_FAMILIES)
def test_box_penalty_sweep_against_the_long_double_box_sweep(mods, family):
    """the box + penalty kernel on the box tests' hard families and shapes (tests/ilqr_box_cases.py: plain, unstable, cheap control,
    inputs on their bounds) with an addend h of entries 0 .. 1e8, against tests/ilqr_box_ref.box_backward(ld=True) on the Hessians
    c_xx + diag h_k, v_xx + diag h_T under hp.sweep_bounds (100 x the fp64 restatement's own error on the case and on the plain
    family); the clamped sets exactly -- every step of every case keeps the strict-complementarity margin of tests/ilqr_box_cases.py,
    asserted on the CPU; and the existing per-step-Hessian call on the materialised Hessians under the same bounds"""
    _, models, _, _lib = mods
    report = []
    for shape in cases.SWEEP_SHAPES:
        c = cases.sweep_case(family, *shape)
        bl, bL = cases.sweep_bounds(family, *shape)
        dyn, cost, Vf, u, lb, ub = c["args"]
        l, L = _state_sweep(_lib, models, dyn, cost, Vf, c["h"], u, lb, ub)
        el, eL = float(hp.sweep_metric(l, c["ref"]["l"]).max()), float(hp.sweep_metric(L, c["ref"]["L"]).max())
        report.append((shape, el, bl, eL, bL))
        assert np.array_equal(_pattern(L), c["ref"]["clamped"]), (family, shape)
        assert el <= bl and eL <= bL, (family, report[-1])
        ml, mL, cap = _box_sweep(_lib, models, dyn, c["mat"][0], c["mat"][1], u, lb, ub)
        assert hp.sweep_metric(ml, c["ref"]["l"]).max() <= bl and hp.sweep_metric(mL, c["ref"]["L"]).max() <= bL and not cap.any()
    print(f"box + penalty sweep {family}: (shape, error of l, bound, error of L, bound)", report)


@pytest.mark.parametrize("shape", SHAPES)
def test_state_sweep_without_a_box_and_a_zero_addend_gives_the_bits_of_the_plain_register_sweep(mods, shape):
    """h = 0 without a box: the bits of zm_ilqr_backward_list_f64 on its register path -- the path it takes at these shapes by
    itself, and at (8, 4) and (12, 4), where aligned operands go to the ring kernel, for an f_x that starts 8 bytes off a 16-byte
    boundary (the ring kernel refuses it)"""
    import torch
    _, models, _, _lib = mods
    lib = _lib.lib()
    n, m = shape
    B = 5
    for T in TS:
        dyn, cost, Vf, h = _sweep_problem(n, m, T, B, 100 * n + T)
        for shared in (False, True):
            ops = [dyn[1], dyn[2], cost[1], cost[2], cost[3], cost[4], cost[5], Vf[1], Vf[2]]
            if shared:
                ops[4:7] = [np.asarray(cost[i])[0, 0] for i in (3, 4, 5)]
                ops[7 + 1] = np.asarray(Vf[2])[0]
            d = [_dev(np.asarray(a, dtype=np.float64)) for a in ops]
            buf = torch.zeros(d[0].numel() + 3, dtype=torch.float64, device="cuda")
            off = 1 if buf.data_ptr() % 16 == 0 else 2          # an address that is 8 modulo 16
            fx = buf[off:off + d[0].numel()].view(d[0].shape)
            fx.copy_(d[0])
            assert fx.data_ptr() % 16 == 8
            d[0] = fx
            dh = torch.zeros((B, T + 1, n), dtype=torch.float64, device="cuda")
            outs = []
            for pen in (False, True):
                l = torch.full((B, T, m), 7.0, dtype=torch.float64, device="cuda")
                L = torch.full((B, T, m, n), 7.0, dtype=torch.float64, device="cuda")
                if pen:
                    rc = lib.zm_ilqr_backward_state_list_f64(*[_p(t) for t in d], _p(dh), None, None, None, 0, None, 1 if shared else 0, _p(l), _p(L),
                                                             None, B, T, n, m, None)
                else:
                    rc = lib.zm_ilqr_backward_list_f64(*[_p(t) for t in d], None, 0, None, 1 if shared else 0, _p(l), _p(L), B, T, n, m, None)
                assert rc == 0, lib.zm_last_error()
                torch.cuda.synchronize()
                outs.append((l.cpu().numpy(), L.cpu().numpy()))
            assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]), (shape, T, shared)


# -------------------------------------------------------------------------------------------------------------------------- 4  solves
def _solve(ilqr, models, p, boxed, x0s, kw, sb_kw=None, lb=None, ub=None):
    """constrainedIterativeLqr on a QP case with the start states x0s (B, n) -> (result tuple, trace dict)"""
    model = models.LinearModel(p["A"], p["B"])
    if boxed:
        model = models.InputBox(model, p["u_lb"], p["u_ub"])
    sb = models.StateBox(model, p["x_lb"] if lb is None else lb, p["x_ub"] if ub is None else ub, **(sb_kw or {}))
    cost = models.QuadraticCost(p["Q"], p["R"], p["Qf"])
    ilqr._TRACE = []
    try:
        out = ilqr.constrainedIterativeLqr(sb, cost, cost, x0s, np.zeros((len(x0s), p["T"], p["B"].shape[1])), **kw)
        rec = dict(ilqr._TRACE)
    finally:
        ilqr._TRACE = None
    return out, rec


SCALES = (1.0, 0.6, 0.0)       # the case's x0, a milder start, and the origin (never touches a bound: done after one outer iteration)


@pytest.mark.parametrize("name,boxed", cases.SOLVE_CASES)
def test_state_solves_follow_the_restatement(mods, name, boxed):
    """the device solve against tests/ilqr_state_ref.py on a batch of three starts of a convex case (default settings): converged, the
    outer count, every inner count, and every step index where the restatement's best two of the 16 costs are 1e-9 apart (elsewhere --
    the confirming iteration of a linear-quadratic inner solve, whose step is zero and whose 16 costs coincide -- the device's choice
    must cost the same to 1e-9); J_AL trace, J, violation, mu to 1e-9 relative (the violation to 1e-9 of the bound's magnitude), the
    multipliers to 1e-8 of their largest; every stored input inside the box"""
    ilqr, models, _, _ = mods
    p = cases.qp_problem(name)
    x0s = np.stack([s * p["x0"] for s in SCALES])
    kw = dict(maxIter=cases.LOOSE["maxIter"], tol=cases.LOOSE["tol"])
    sb_kw = dict(outer=cases.LOOSE["outer"], ctol=cases.LOOSE["ctol"])
    (traj, L, J, conv, info), rec = _solve(ilqr, models, p, boxed, x0s, kw, sb_kw)
    if boxed:
        assert np.all(traj.uTraj >= p["u_lb"]) and np.all(traj.uTraj <= p["u_ub"]) and not rec["qp_capped"].any()
    assert np.all(info.violation[conv] <= cases.LOOSE["ctol"])
    walls = np.concatenate([p["x_lb"], p["x_ub"]])
    wall = np.max(np.abs(walls[np.isfinite(walls)]))
    for b, s in enumerate(SCALES):
        tr = []
        r = sref.constrainedIterativeLqr(lambda x, u: p["A"] @ x + p["B"] @ u, p["Q"], p["R"], p["Qf"], x0s[b], np.zeros((p["T"], p["B"].shape[1])),
                                         p["x_lb"], p["x_ub"], u_lb=p["u_lb"] if boxed else None, u_ub=p["u_ub"] if boxed else None, trace=tr,
                                         **cases.LOOSE)
        assert bool(conv[b]) == r["converged"] and int(info.outerIterations[b]) == r["outer"], (name, b)
        assert list(info.innerIterations[b][: r["outer"]]) == r["inner"], (name, b, info.innerIterations[b], r["inner"])
        for j, o in enumerate(tr):
            assert abs(rec["mu_trace"][j, b] - o["mu"]) <= 1e-9 * o["mu"]
            assert abs(rec["violation_trace"][j, b] - o["violation"]) <= 1e-9 * wall, (name, b, j)
            for it, rit in enumerate(o["inner"]):
                Jd, ad = rec["J_trace"][j, it, b], rec["alpha_trace"][j, it, b]
                srt = np.sort(rit["Js"])
                if srt[1] - srt[0] >= 1e-9 * abs(srt[0]):
                    assert ad == rit["idx"], (name, b, j, it)
                else:
                    assert abs(rit["Js"][ad] - srt[0]) <= 1e-9 * abs(srt[0]), (name, b, j, it)
                assert abs(Jd - rit["J"]) <= 1e-9 * abs(rit["J"]), (name, b, j, it, Jd, rit["J"])
        assert abs(J[b] - r["J"]) <= 1e-9 * abs(r["J"]) + 1e-300 and abs(info.mu[b] - r["mu"]) <= 1e-9 * r["mu"]
        assert abs(info.violation[b] - r["violation"]) <= 1e-9 * wall
        for d, q in ((info.lam_lb[b], r["lam_lb"]), (info.lam_ub[b], r["lam_ub"])):
            assert np.max(np.abs(d - q)) <= 1e-8 * max(np.max(np.abs(q)), 1.0), (name, b)
            assert np.all(d[0] == 0.0)
        assert _rel(traj.uTraj[b], r["traj"].uTraj) <= 1e-7 or np.max(np.abs(r["traj"].uTraj)) == 0.0
    assert int(info.outerIterations[2]) == 1 and info.violation[2] == 0.0         # the start at the origin never touches a bound


def test_frozen_rows_and_sync_independence(mods, monkeypatch):
    """a mixed batch: the rows of the trajectories that finish early are bit for bit those of a run cut off at that outer iteration
    (nothing of a done trajectory is touched again), and the results do not depend on ZOPT_AMD_ILQR_SYNC in {1, 4}"""
    ilqr, models, _, _ = mods
    p = cases.qp_problem("dint")
    x0s = np.stack([s * p["x0"] for s in (1.0, 0.0, 0.3, 1.2, 0.1)])
    kw = dict(maxIter=100, tol=1e-3)
    monkeypatch.setenv("ZOPT_AMD_ILQR_SYNC", "4")
    (traj, L, J, conv, info), rec = _solve(ilqr, models, p, True, x0s, kw)
    outs = np.asarray(info.outerIterations)
    assert outs.min() == 1 and outs.max() >= 3 and len(set(outs.tolist())) >= 2, outs
    monkeypatch.setenv("ZOPT_AMD_ILQR_SYNC", "1")
    (traj1, L1, J1, conv1, info1), rec1 = _solve(ilqr, models, p, True, x0s, kw)
    for a, b in ((traj.xTraj, traj1.xTraj), (traj.uTraj, traj1.uTraj), (L, L1), (J, J1), (conv, conv1), (info.violation, info1.violation),
                 (info.mu, info1.mu), (info.lam_ub, info1.lam_ub), (info.lam_lb, info1.lam_lb), (info.outerIterations, info1.outerIterations),
                 (info.innerIterations, info1.innerIterations)):
        assert np.array_equal(a, b)
    for cut in sorted(set(outs.tolist()))[:-1]:
        (trajc, Lc, Jc, convc, infoc), _ = _solve(ilqr, models, p, True, x0s, kw, dict(outer=int(cut)))
        for b in np.nonzero(outs == cut)[0]:
            assert conv[b] and convc[b]
            for a, c in ((traj.xTraj, trajc.xTraj), (traj.uTraj, trajc.uTraj), (L, Lc), (J, Jc), (info.violation, infoc.violation),
                         (info.mu, infoc.mu), (info.lam_ub, infoc.lam_ub), (info.lam_lb, infoc.lam_lb)):
                assert np.array_equal(a[b], c[b]), (cut, b)


def test_one_trajectory_exhausts_outer(mods):
    """a wall no input can hold (the velocity pinned to 0.5 from a start at rest) is never feasible: that trajectory runs every outer
    iteration and is not converged, its mu reaches growth ** (outer - 1); its neighbour finishes as it does alone"""
    ilqr, models, _, _ = mods
    p = cases.qp_problem("dint")
    x0s = np.stack([p["x0"], 0.3 * p["x0"]])
    lb, ub = np.array([[-INF, 0.5], [-INF, -INF]]), np.array([[INF, 0.5], [INF, 0.7]])
    (traj, L, J, conv, info), _ = _solve(ilqr, models, p, False, x0s, dict(maxIter=50, tol=1e-3), dict(outer=4), lb=lb, ub=ub)
    assert not conv[0] and conv[1] and int(info.outerIterations[0]) == 4 and info.mu[0] == 1e3 and info.violation[0] > 1e-4
    (_, _, J1, conv1, info1), _ = _solve(ilqr, models, p, False, x0s[1:], dict(maxIter=50, tol=1e-3), dict(outer=4), lb=lb[1:], ub=ub[1:])
    assert np.array_equal(J1[0], J[1]) and np.array_equal(info1.lam_ub[0], info.lam_ub[1]) and int(info1.outerIterations[0]) == int(info.outerIterations[1])


def test_infinite_state_bounds_reproduce_the_box_solve_bit_for_bit(mods):
    """all state bounds infinite inside an InputBox: one outer iteration whose inner solve is zm_ilqr_solve_box_f64's loop on kernels
    that add an exact 0.0 -- the same bits (trajectory, gains, cost, flags, trace); without an InputBox the plain solve is followed
    iterate by iterate (it runs the ring sweep: same step indices, costs to 1e-9), and so is the box solve at (12, 4), whose line
    search is the fast kernel (it has no penalty form)"""
    ilqr, models, _, _ = mods
    for name in ("dint", "unstable5", "stable12"):
        p = cases.qp_problem(name)
        n, m = p["B"].shape
        x0s = np.stack([s * p["x0"] for s in (1.0, -0.5, 0.2, 0.0, 2.0)])
        ug = np.zeros((5, p["T"], m))
        cost = models.QuadraticCost(p["Q"], p["R"], p["Qf"])
        for boxed in (True, False):
            inner = models.LinearModel(p["A"], p["B"])
            inner = models.InputBox(inner, p["u_lb"], p["u_ub"]) if boxed else inner
            ilqr._TRACE = []
            try:
                ref = ilqr.iterativeLqr(inner, cost, cost, x0s, ug)
                rref = dict(ilqr._TRACE)
                ilqr._TRACE = []
                out = ilqr.iterativeLqr(models.StateBox(inner, np.full(n, -INF), np.full(n, INF)), cost, cost, x0s, ug)
                rout = dict(ilqr._TRACE)
            finally:
                ilqr._TRACE = None
            its = rref["iterations"]
            assert rout["iterations"] == 1
            if boxed and n < 12:
                assert np.array_equal(rout["alpha_trace"][0, :its], rref["alpha_trace"]), (name, boxed)
                assert np.array_equal(rout["J_trace"][0, :its], rref["J_trace"])
                for a, b in zip((out[0].xTraj, out[0].uTraj, out[1], out[2], out[3]), (ref[0].xTraj, ref[0].uTraj, ref[1], ref[2], ref[3])):
                    assert np.array_equal(a, b), (name, boxed)
            else:
                # (the step index only where it is decided: the confirming iteration of a linear-quadratic solve has 16 equal costs)
                assert _rel(out[2], ref[2]) <= 1e-9 and _rel(out[0].uTraj, ref[0].uTraj) <= 1e-7 and np.array_equal(out[3], ref[3]), (name, boxed)
                assert np.array_equal(rout["alpha_trace"][0, 0], rref["alpha_trace"][0]) and _rel(rout["J_trace"][0, 0], rref["J_trace"][0]) <= 1e-9


def test_reentry_rollout_reproduces_the_stored_states(mods):
    """the re-entry of an inner solve from (uTraj, L = 0) rolls out the stored states bit for bit: a solve whose inner loops may not
    iterate (maxIter = 0) returns, after three outer iterations, the trajectory of a plain rollout of uGuess"""
    ilqr, models, pytrees, _ = mods
    p = cases.qp_problem("unstable5")
    n, m = p["B"].shape
    rng = np.random.default_rng(3)
    x0s, ug = rng.standard_normal((5, n)), rng.standard_normal((5, p["T"], m))
    model = models.InputBox(models.LinearModel(p["A"], p["B"]), p["u_lb"], p["u_ub"])
    cost = models.QuadraticCost(p["Q"], p["R"], p["Qf"])
    traj, L, J, conv, info = ilqr.constrainedIterativeLqr(models.StateBox(model, p["x_lb"], p["x_ub"], outer=3), cost, cost, x0s, ug, maxIter=0)
    roll = ilqr.trajectoryRollout(x0s, model, pytrees.AffinePolicy(ug, np.zeros((5, p["T"], m, n))),
                                  pytrees.Trajectory(np.zeros((5, p["T"] + 1, n)), np.zeros((5, p["T"], m))))
    assert np.array_equal(traj.xTraj, roll.xTraj) and np.array_equal(traj.uTraj, roll.uTraj) and not conv.any()
    assert np.all(info.outerIterations == 3) and np.all(info.innerIterations == 0) and np.all(L == 0.0)


# ------------------------------------------------------------------------------------------------------------------ 5  public surface
def test_quadcopters_under_a_ceiling_and_a_speed_cap_through_the_public_calls(mods):
    """QuadcopterEuler (T = 20) with a TrackingCost about a goal per trajectory, an altitude bound, a speed cap and thrust limits:
    NumPy and torch inputs give the same bits, no leading axis and a 2-D leading shape work, every returned input is inside the input
    box, violation <= ctol wherever converged, and iterativeLqr returns the first four results of constrainedIterativeLqr"""
    import torch
    ilqr, models, _, _ = mods
    T, n, m = 20, 12, 4
    rng = np.random.default_rng(0)
    hover = np.asarray(models.QuadcopterEuler.uTrim, dtype=np.float64)
    goals = np.zeros((2, 3, 1, n))
    goals[..., 9:12] = rng.uniform(-2, 2, (2, 3, 1, 3))       # positions are states 9..11 (z down)
    cost = models.TrackingCost(np.eye(n), np.eye(m), 10 * np.eye(n), goals, hover)
    x_lb, x_ub = np.full(n, -INF), np.full(n, INF)
    x_lb[11], x_ub[11] = -1.0, 1.0               # a ceiling and a floor a metre from the start
    x_lb[0:3], x_ub[0:3] = -0.8, 0.8             # a cap on the body velocities
    u_lb, u_ub = hover - np.array([2.0, 0.05, 0.05, 0.05]), hover + np.array([2.0, 0.05, 0.05, 0.05])
    sb = models.StateBox(models.InputBox(models.QuadcopterEuler(0.1), u_lb, u_ub), x_lb, x_ub)
    x0, ug = np.zeros((2, 3, n)), np.tile(hover, (2, 3, T, 1))
    traj, L, J, conv, info = ilqr.constrainedIterativeLqr(sb, cost, cost, x0, ug)
    assert traj.xTraj.shape == (2, 3, T + 1, n) and info.lam_ub.shape == (2, 3, T + 1, n) and info.innerIterations.shape == (2, 3, 10)
    assert np.all(traj.uTraj >= u_lb) and np.all(traj.uTraj <= u_ub)
    assert conv.any() and np.all(info.violation[conv] <= 1e-4)
    assert np.any(info.lam_ub > 0) or np.any(info.lam_lb > 0), "no bound was ever active: the case does not test the penalty"
    four = ilqr.iterativeLqr(sb, cost, cost, x0, ug)
    assert len(four) == 4 and np.array_equal(four[0].xTraj, traj.xTraj) and np.array_equal(four[2], J) and np.array_equal(four[3], conv)
    tt = ilqr.constrainedIterativeLqr(sb, cost, cost, torch.as_tensor(x0, device="cuda"), torch.as_tensor(ug, device="cuda"))
    assert torch.is_tensor(tt[4].violation) and np.array_equal(tt[0].uTraj.cpu().numpy(), traj.uTraj) and np.array_equal(tt[4].mu.cpu().numpy(), info.mu)
    one = ilqr.constrainedIterativeLqr(models.StateBox(models.InputBox(models.QuadcopterEuler(0.1), u_lb, u_ub), x_lb, x_ub),
                                       *(2 * (models.TrackingCost(np.eye(n), np.eye(m), 10 * np.eye(n), goals[1, 2], hover),)), x0[1, 2], ug[1, 2])
    assert isinstance(one[2], float) and isinstance(one[3], bool) and np.array_equal(one[0].xTraj, traj.xTraj[1, 2])
    assert np.array_equal(one[4].lam_ub, info.lam_ub[1, 2]) and one[4].innerIterations.shape == (10,)


@pytest.mark.parametrize("boxed", [False, True])
def test_quadcopter_state_solves_follow_the_restatement(mods, boxed):
    """QuadcopterEuler (T = 20) with a TrackingCost about hover and a goal per trajectory, an altitude floor and a speed cap, without
    and inside an InputBox (tests/ilqr_state_cases.quad_case; the CPU file asserts its hygiene by the rule as written: every
    iteration's best two costs 1e-9 apart): converged, the outer count, every inner count and every step index equal; the J_AL
    trace, J, violation and mu to 1e-9 relative, the multipliers to 1e-8 of their largest"""
    ilqr, models, _, _ = mods
    c = cases.quad_case()
    kw = cases.QUAD_KW
    model = models.QuadcopterEuler(cases.QUAD_DT)
    if boxed:
        model = models.InputBox(model, c["u_lb"], c["u_ub"])
    sb = models.StateBox(model, c["x_lb"], c["x_ub"], mu0=kw["mu0"], ctol=kw["ctol"], outer=kw["outer"])
    cost = models.TrackingCost(c["Q"], c["R"], c["Qf"], c["goals"], cases.QUAD_UTRIM)
    ilqr._TRACE = []
    try:
        traj, L, J, conv, info = ilqr.constrainedIterativeLqr(sb, cost, cost, c["x0"], c["ug"], maxIter=kw["maxIter"], tol=kw["tol"])
        rec = dict(ilqr._TRACE)
    finally:
        ilqr._TRACE = None
    if boxed:
        assert np.all(traj.uTraj >= c["u_lb"]) and np.all(traj.uTraj <= c["u_ub"]) and not rec["qp_capped"].any()
    worst = {"J_AL": 0.0, "J": 0.0, "violation": 0.0, "lam": 0.0}
    for b in range(cases.QUAD_B):
        r = cases.quad_restatement(boxed, b)
        print(f"quadcopter boxed={boxed} trajectory {b}: device outer {int(info.outerIterations[b])} inner {info.innerIterations[b][:r['outer']].tolist()} "
              f"restatement outer {r['outer']} inner {r['inner']}")
        assert bool(conv[b]) == r["converged"] and int(info.outerIterations[b]) == r["outer"], b
        assert list(info.innerIterations[b][: r["outer"]]) == r["inner"], b
        for j, o in enumerate(r["trace"]):
            assert abs(rec["mu_trace"][j, b] - o["mu"]) <= 1e-9 * o["mu"]
            worst["violation"] = max(worst["violation"], abs(rec["violation_trace"][j, b] - o["violation"]))
            for it, rit in enumerate(o["inner"]):
                assert rec["alpha_trace"][j, it, b] == rit["idx"], (b, j, it)
                worst["J_AL"] = max(worst["J_AL"], abs(rec["J_trace"][j, it, b] - rit["J"]) / abs(rit["J"]))
        worst["J"] = max(worst["J"], abs(J[b] - r["J"]) / abs(r["J"]))
        for d, q in ((info.lam_lb[b], r["lam_lb"]), (info.lam_ub[b], r["lam_ub"])):
            worst["lam"] = max(worst["lam"], float(np.max(np.abs(d - q)) / max(np.max(np.abs(q)), 1.0)))
        assert abs(info.mu[b] - r["mu"]) <= 1e-9 * r["mu"]
    print(f"quadcopter boxed={boxed}: worst relative differences", worst)
    assert worst["J_AL"] <= 1e-9 and worst["J"] <= 1e-9 and worst["violation"] <= 1e-9 and worst["lam"] <= 1e-8, worst


def test_mixed_batch_frozen_rows(mods):
    """one batch in which trajectory 1 never touches a bound (done after the first outer iteration), trajectories 0 and 2 finish
    after a few, and trajectory 3 -- its velocity pinned to 0.5 from a start at rest, which no input can hold -- exhausts `outer`, so
    that the others finish while it runs on to the last outer iteration, where nothing is updated: the rows of every trajectory that
    finishes early are bit for bit those of a run cut off at that outer iteration, the exhausting one is not converged and its mu is
    growth ** (outer - 1)"""
    ilqr, models, _, _ = mods
    p = cases.qp_problem("dint")
    x0s = np.stack([s * p["x0"] for s in (1.0, 0.0, 0.6, 1.0)])
    lb = np.array([[-INF, -INF], [-INF, -INF], [-INF, -INF], [-INF, 0.5]])
    ub = np.array([[INF, 0.7], [INF, 0.7], [INF, 0.7], [INF, 0.5]])
    kw = dict(maxIter=100, tol=1e-3)
    outer = 7
    (traj, L, J, conv, info), _ = _solve(ilqr, models, p, True, x0s, kw, dict(outer=outer), lb=lb, ub=ub)
    outs = np.asarray(info.outerIterations)
    assert outs[1] == 1 and 2 <= outs[0] < outer and 2 <= outs[2] < outer and outs[3] == outer, outs
    assert conv.tolist() == [True, True, True, False] and info.mu[3] == 10.0 ** (outer - 1) and info.violation[3] > 1e-4
    assert np.all(info.violation[:3] <= 1e-4)
    for cut in sorted(set(outs[:3].tolist())):
        (trajc, Lc, Jc, convc, infoc), _ = _solve(ilqr, models, p, True, x0s, kw, dict(outer=int(cut)), lb=lb, ub=ub)
        for b in np.nonzero(outs == cut)[0]:
            assert convc[b]
            for a, c in ((traj.xTraj, trajc.xTraj), (traj.uTraj, trajc.uTraj), (L, Lc), (J, Jc), (info.violation, infoc.violation),
                         (info.mu, infoc.mu), (info.lam_ub, infoc.lam_ub), (info.lam_lb, infoc.lam_lb), (info.innerIterations[:, :cut], infoc.innerIterations)):
                assert np.array_equal(a[b], c[b]), (cut, b)


def test_rollouts_unwrap_a_state_box(mods):
    """trajectoryRollout and the simulator take a StateBox for its dynamics: the bits of the rollout through the InputBox inside it
    (the inputs clipped), and of the bare model's without one"""
    ilqr, models, pytrees, _ = mods
    from zopt_amd import simulator
    p = cases.qp_problem("unstable5")
    n, m = p["B"].shape
    rng = np.random.default_rng(8)
    x0s, l, L = rng.standard_normal((5, n)), rng.standard_normal((5, p["T"], m)), 0.1 * rng.standard_normal((5, p["T"], m, n))
    prev = pytrees.Trajectory(0.1 * rng.standard_normal((5, p["T"] + 1, n)), 0.1 * rng.standard_normal((5, p["T"], m)))
    bare = models.LinearModel(p["A"], p["B"])
    for inner in (bare, models.InputBox(bare, p["u_lb"], p["u_ub"])):
        sb = models.StateBox(inner, p["x_lb"], p["x_ub"])
        a, b = ilqr.trajectoryRollout(x0s, sb, pytrees.AffinePolicy(l, L), prev, 0.5), ilqr.trajectoryRollout(x0s, inner, pytrees.AffinePolicy(l, L), prev, 0.5)
        assert np.array_equal(a.xTraj, b.xTraj) and np.array_equal(a.uTraj, b.uTraj)
        if inner is not bare:
            assert np.any((a.uTraj == p["u_lb"]) | (a.uTraj == p["u_ub"]))
        sa, sbb = simulator.simulateTrackingController(sb, x0s, L, prev), simulator.simulateTrackingController(inner, x0s, L, prev)
        assert np.array_equal(sa.xTraj, sbb.xTraj) and np.array_equal(sa.uTraj, sbb.uTraj)
