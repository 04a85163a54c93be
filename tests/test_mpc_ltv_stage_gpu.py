"""GPU tests of mpcUtils.ltvMpc with stage_varying=: per-stage weights and boxes through zm_mpc_setup_ltv_stage_f64 and
zm_mpc_solve_ltv_stage_f64.  Constant rows must reproduce the plain ltvMpc bit for bit (the same sums, the same tables); every
stage-varying case is held to the NumPy restatement of the whole solve (tests/mpc_ltv_stage_ref.py: admm_levels_ltv_stage) by the rule
of tests/test_mpc_ltv_gpu.py.  tests/test_mpc_ltv_stage.py checks, without a GPU, that these inputs stay clear of every
rounding-sensitive decision and that their stage data matters.  Horizons 2, 3, 4, 5, 7 (below the prefetch depth, its depth, both tail
branches of the three-stage loops, 3 * 2 + 1), batches 1, 5 (idle groups) and 9, eps 1e-6."""
import numpy as np
import pytest

from tests import mpc_iterates_cases as ic
from tests import mpc_ltv_ref as lr
from tests import mpc_ltv_stage_ref as sr
from tests import mpc_tracking_ref as tr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mpc():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from zopt_amd import mpcUtils
    return mpcUtils


# ---- constant rows: the plain ltvMpc, bit for bit ------------------------------------------------------------------------------------------

# every compiled shape with n + m <= 16, then three embedded ones; each with one of the horizons and one of the batches
PARITY = [(12, 4, 7, 5), (8, 4, 5, 9), (4, 2, 4, 5), (4, 1, 3, 1), (2, 2, 2, 9), (2, 1, 7, 1), (1, 1, 5, 5),
          (3, 1, 4, 9), (3, 2, 3, 5), (10, 3, 2, 1)]


def _state(prob, nb, N):
    y, lam, level, ok = ic.read_state(prob, nb, N)
    return dict(y=y.copy(), lam=lam.copy(), level=level.copy(), ok=ok.copy())


def _solve(prob, x0, nb, N, **kw):
    u, traj, status = prob.solve(x0, **kw)
    return dict(u=np.asarray(u), x=np.asarray(traj.xTraj), uT=np.asarray(traj.uTraj), status=np.asarray(status, dtype=str),
                iters=prob.last_iterations.copy(), resid=prob.last_residuals.copy(), **_state(prob, nb, N))


def _identical(a, b, at):
    for k in a:
        assert np.array_equal(a[k], b[k]), (at, k)


@pytest.mark.parametrize("n,m,N,nb", PARITY)
def test_constant_rows_are_the_plain_solve_bit_for_bit(mpc, n, m, N, nb):
    """a stage-varying object whose rows are all the same against a plain ltvMpc on the same data: == on status, iteration count, u,
    trajectory, residuals and the stored warm-start state (y, lam, level, ok flag), and on the tables -- cold, warm and "shift", alpha 1.0
    and 1.6, adaptive and fixed penalty, with and without references"""
    import torch
    (A, B, c, Q, R, Qf, xl, xu, ul, uu), x0 = lr.recipe(n, m, N, nb, bad=3 if nb > 3 else None)
    Qs, Rs, sxl, sxu, sul, suu = sr.stage_form(Q, R, Qf, N, xl, xu, ul, uu)
    plain = mpc.ltvMpc(A, B, Q, R, N, xl, xu, ul, uu, Qf=Qf, c=c)
    staged = mpc.ltvMpc(A, B, np.concatenate([Qs[:1], Qs]), Rs, N, sxl, sxu, sul, suu, c=c, stage_varying=sr.ALL_SIX)
    assert (staged.n, staged.m) == (plain.n, plain.m)
    _, _, xRef, uRef = tr.random_case(n, m, N, seed=41, nb=nb)
    seen = set()
    for alpha in (1.0, 1.6):
        for adaptive in (True, False):
            for refs in (False, True):
                kw = dict(rho=plain.rho, alpha=alpha, adaptive_rho=adaptive, max_iter=600, **(dict(xRef=xRef, uRef=uRef) if refs else {}))
                at = (n, m, N, nb, alpha, adaptive, refs)
                cold = [_solve(p, x0, nb, N, warm_start=False, eps_abs=1e-3, eps_rel=1e-3, **kw) for p in (plain, staged)]
                _identical(*cold, at + ("cold",))
                for tp, ts in zip(plain._tables[(plain.rho.tobytes(), adaptive)], staged._tables[(plain.rho.tobytes(), adaptive)]):
                    if torch.is_tensor(tp):
                        assert torch.equal(tp, ts), at
                warm = [_solve(p, x0, nb, N, warm_start=True, eps_abs=1e-6, eps_rel=1e-6, **kw) for p in (plain, staged)]
                _identical(*warm, at + ("warm",))
                x1 = warm[0]["x"][..., 1, :]
                shift = [_solve(p, x1, nb, N, warm_start="shift", eps_abs=1e-6, eps_rel=1e-6, **kw) for p in (plain, staged)]
                _identical(*shift, at + ("shift",))
                seen |= set(warm[0]["status"]) | set(shift[0]["status"])
                if nb > 3:
                    assert cold[0]["status"][3] == "infeasible" and cold[0]["iters"][3] == 0
    assert "optimal" in seen, seen


# ---- stage-varying data: the restatement, iterate by iterate ------------------------------------------------------------------------------

def _hold(mpc, name, prob=None):
    c, ref = sr.build(name), sr.reference(name)
    got = sr.run_steps(prob or sr.make_problem(mpc, c), c, ref)
    worst = sr.compare(name, ref, got)
    print(f"{name}: largest deviation {worst:.2e} of its bound")
    return got


@pytest.mark.parametrize("name", sr.ALL)
def test_stage_varying_cases_follow_the_restatement(mpc, name):
    """moving boxes, a tight terminal box, +-inf at some stages, stage weights with Q_k = 0 at most stages, weights and boxes together under
    references, the gate, x0 outside row 0, per-problem stage data, instances sharing a problem: same status, iteration count, final
    level and ok flag; x, u, y, lam and the residuals to 1e-9 max(1, |reference|)"""
    got = _hold(mpc, name)[0]
    if name == "gate":
        assert list(got["status"]) == ["infeasible", "optimal"] and got["iters"][0] % 8 == 0 and got["iters"][0] > 0
    if name == "x0_outside_row0":
        assert got["status"][3] == "infeasible" and got["iters"][3] == 0
    if name == "both_tracking":
        c = sr.build(name)
        assert got["x"].shape[-1] == 3 and got["u"].shape[-1] == 2 and (c.inst[0][0].shape[-1], c.inst[0][1].shape[-1]) == (3, 2)


def test_a_subset_of_names_is_the_same_problem(mpc):
    """only the names whose rows differ carry a stage axis; the rest goes in as one set: the same solve, bit for bit"""
    c = sr.build("terminal_box")
    A, B, ck, Qs, Rs, xl, xu, ul, uu = c.inst[0]
    some = mpc.ltvMpc(A, B, Qs[0], Rs[0], c.N, xl, xu, ul[0], uu[0], Qf=Qs[-1], c=ck, stage_varying=("x_lb", "x_ub"))
    full = sr.make_problem(mpc, c)
    kw = dict(rho=full.rho, **c.steps[0]["kw"])
    _identical(_solve(some, c.x0, 9, c.N, **kw), _solve(full, c.x0, 9, c.N, **kw), "terminal_box")


@pytest.mark.parametrize("name", sr.SCIPY_GPU)
def test_final_solutions_are_the_qp_solutions(mpc, name):
    """the kernels' u against the condensed SciPy solve, at the 2e-3 of the CPU test"""
    c = sr.build(name)
    prob = sr.make_problem(mpc, c)
    extra = {} if c.rho is None else dict(rho=c.rho)
    _, traj, status = prob.solve(c.x0[:2], **extra, **c.steps[0]["kw"])
    for b in sr.scipy_instances(name):
        dev = np.max(np.abs(np.asarray(traj.uTraj)[b] - sr.scipy_solution(name, b)[1]))
        print(f"{name} instance {b}: deviation of u from SciPy {dev:.2e}")
        assert status[b] == "optimal" and dev <= 2e-3


# ---- update ----------------------------------------------------------------------------------------------------------------------------------

def _moved(c, p=0):
    """the case's boxes one stage further on (the last row repeated), its weights scaled by stage: the next window of a moving corridor"""
    _, _, _, Qs, Rs, xl, xu, ul, uu = c.inst[p]
    nxt = lambda X: np.concatenate([X[1:], X[-1:]])
    keep0 = lambda X: np.concatenate([X[:1], nxt(X[1:])])       # (row 0 is the test on x0: the start has not moved)
    s = 1.0 + 0.1 * np.arange(c.N)
    Qn = np.concatenate([Qs[:1], Qs]) * np.concatenate([[1.0], s])[:, None, None]
    return dict(Q=Qn, R=Rs * s[::-1, None, None], x_lb=keep0(xl) - 0.01, x_ub=keep0(xu) + 0.01, u_lb=nxt(ul) - 0.01, u_ub=nxt(uu) + 0.01)


def _fresh(mpc, c, new):
    if c.shared:
        A, B, ck = c.inst[0][:3]
    else:
        A, B, ck = (np.stack([d[i] for d in c.inst]) for i in range(3))
    return mpc.ltvMpc(A, B, new["Q"], new["R"], c.N, new["x_lb"], new["x_ub"], new["u_lb"], new["u_ub"], c=ck, stage_varying=sr.ALL_SIX)


def _new_data(c):
    if c.shared:
        return _moved(c)
    per = [_moved(c, p) for p in range(len(c.inst))]
    return {k: np.stack([d[k] for d in per]) for k in per[0]}


@pytest.mark.parametrize("name,device", [("moving_boxes", False), ("per_problem", False), ("both_tracking", True)])
def test_update_of_bounds_keeps_the_tables_and_of_weights_rebuilds_them(mpc, name, device):
    """new bounds leave the table tensors where they are (same data_ptr, no setup launch) and a cold solve then equals a fresh object's bit
    for bit; new Q, R drop the tables, and a cold solve equals a fresh object's; the warm-start workspace survives both.  device: the new
    data goes in as device tensors.  (both_tracking is embedded: the padding stays what the constructor made it.)"""
    import torch
    c = sr.build(name)
    nb, N = len(c.x0), c.N
    prob = sr.make_problem(mpc, c)
    refs = {} if c.xRef is None else dict(xRef=c.xRef, uRef=c.uRef)
    kw = dict(rho=prob.rho, warm_start=False, **refs, **c.steps[0]["kw"])
    _solve(prob, c.x0, nb, N, **kw)
    new = _new_data(c)
    give = (lambda v: torch.as_tensor(v, device="cuda")) if device else (lambda v: v)
    bounds = {k: new[k] for k in ("x_lb", "x_ub", "u_lb", "u_ub")}
    tabs, ws = dict(prob._tables), prob._ws
    ptrs = [t.data_ptr() for t in next(iter(tabs.values())) if torch.is_tensor(t)]
    prob.update(**{k: give(v) for k, v in bounds.items()})
    assert prob._ws is ws and list(prob._tables) == list(tabs)
    assert [t.data_ptr() for t in next(iter(prob._tables.values())) if torch.is_tensor(t)] == ptrs
    got = _solve(prob, c.x0, nb, N, **kw)
    want = _solve(_fresh(mpc, c, dict(new, Q=_user(prob, "Q"), R=_user(prob, "R"))), c.x0, nb, N, **kw)
    _identical(got, want, (name, "bounds"))
    assert not np.array_equal(got["u"], _solve(sr.make_problem(mpc, c), c.x0, nb, N, **kw)["u"])     # (the new boxes do matter)
    ws = prob._ws
    prob.update(Q=give(new["Q"]), R=give(new["R"]))
    assert prob._tables == {} and prob._ws is ws
    got = _solve(prob, c.x0, nb, N, **kw)
    assert len(prob._tables) == 1
    _identical(got, _solve(_fresh(mpc, c, new), c.x0, nb, N, **kw), (name, "weights"))
    assert not np.array_equal(got["u"], want["u"])                                                   # (so do the new weights)


def _user(prob, name):
    """the object's weight `name` without the padding of an embedded shape"""
    w = prob._n_user if name == "Q" else prob._m_user
    return getattr(prob, name)[..., :w, :w]
