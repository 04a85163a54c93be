"""GPU tests of mpcUtils.ltvMpc with soft box constraints: zm_mpc_solve_ltv_soft_f64 (mpc_solve_wave_ltv_soft_kernel).  All-hard weights
must reproduce zm_mpc_solve_ltv_stage_f64 bit for bit; every soft case is held to the NumPy restatement of the whole solve
(tests/mpc_ltv_soft_ref.py: admm_levels_ltv_soft) by the rule of tests/test_mpc_ltv_gpu.py.  tests/test_mpc_ltv_soft.py checks, without
a GPU, that these inputs stay clear of every rounding-sensitive decision and that their weights matter.  Horizons 2, 3, 4, 5, 7, batches
1, 5 (idle groups) and 9, eps 1e-6."""
import numpy as np
import pytest

from tests import mpc_iterates_cases as ic
from tests import mpc_ltv_ref as lr
from tests import mpc_ltv_soft_ref as so
from tests import mpc_ltv_stage_ref as sr
from tests import mpc_tracking_ref as tr

pytestmark = pytest.mark.gpu

INF = np.inf


@pytest.fixture(scope="module")
def mpc():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from zopt_amd import mpcUtils
    return mpcUtils


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


# ---- all-hard weights: the stage entry, bit for bit ------------------------------------------------------------------------------------

# every compiled shape with n + m <= 16, then an embedded one; each with one of the horizons and one of the batches
PARITY = [(12, 4, 7, 5), (8, 4, 5, 9), (4, 2, 4, 5), (4, 1, 3, 1), (2, 2, 2, 9), (2, 1, 7, 1), (1, 1, 5, 5), (3, 2, 3, 5)]


@pytest.mark.parametrize("n,m,N,nb", PARITY)
def test_all_hard_weights_are_the_stage_solve_bit_for_bit(mpc, n, m, N, nb):
    """an object with every l1 = +inf (built without stage_varying=: it materialises the stage form itself) through the soft entry
    against a stage-varying object with constant rows through zm_mpc_solve_ltv_stage_f64: == on status, iteration count, u, trajectory,
    residuals and the stored warm-start state (y, lam, level, ok flag) -- cold, warm and "shift", alpha 1.0 and 1.6, adaptive and fixed
    penalty, with and without references"""
    (A, B, c, Q, R, Qf, xl, xu, ul, uu), x0 = lr.recipe(n, m, N, nb, bad=3 if nb > 3 else None)
    Qs, Rs, sxl, sxu, sul, suu = sr.stage_form(Q, R, Qf, N, xl, xu, ul, uu)
    staged = mpc.ltvMpc(A, B, np.concatenate([Qs[:1], Qs]), Rs, N, sxl, sxu, sul, suu, c=c, stage_varying=sr.ALL_SIX)
    hard = mpc.ltvMpc(A, B, Q, R, N, xl, xu, ul, uu, Qf=Qf, c=c, x_soft_l1=np.full(n, INF), u_soft_l2=np.zeros(m))
    assert (staged.n, staged.m) == (hard.n, hard.m) and hard._soft is not None and staged._soft is None
    _, _, xRef, uRef = tr.random_case(n, m, N, seed=41, nb=nb)
    seen = set()
    for alpha in (1.0, 1.6):
        for adaptive in (True, False):
            for refs in (False, True):
                kw = dict(rho=staged.rho, alpha=alpha, adaptive_rho=adaptive, max_iter=600, **(dict(xRef=xRef, uRef=uRef) if refs else {}))
                at = (n, m, N, nb, alpha, adaptive, refs)
                cold = [_solve(p, x0, nb, N, warm_start=False, eps_abs=1e-3, eps_rel=1e-3, **kw) for p in (staged, hard)]
                _identical(*cold, at + ("cold",))
                warm = [_solve(p, x0, nb, N, warm_start=True, eps_abs=1e-6, eps_rel=1e-6, **kw) for p in (staged, hard)]
                _identical(*warm, at + ("warm",))
                x1 = warm[0]["x"][..., 1, :]
                shift = [_solve(p, x1, nb, N, warm_start="shift", eps_abs=1e-6, eps_rel=1e-6, **kw) for p in (staged, hard)]
                _identical(*shift, at + ("shift",))
                seen |= set(warm[0]["status"]) | set(shift[0]["status"])
                if nb > 3:
                    assert cold[0]["status"][3] == "infeasible" and cold[0]["iters"][3] == 0
    assert "optimal" in seen, seen


# ---- soft cases: the restatement, iterate by iterate -------------------------------------------------------------------------------------

def _hold(mpc, name):
    c, ref = so.build(name), so.reference(name)
    got = so.run_steps(so.make_problem(mpc, c), c, ref)
    worst = so.compare(name, ref, got)
    print(f"{name}: largest deviation {worst:.2e} of its bound")
    return got


@pytest.mark.parametrize("name", so.ALL)
def test_soft_cases_follow_the_restatement(mpc, name):
    """the closed gate next to its soft twin, x0 outside row 0 in a soft and in a hard component, a terminal set under a small l1, a purely
    quadratic penalty on moving boxes, l1 and l2 with a soft input and +-inf bounds, references outside soft boxes, an embedded shape,
    weights per problem, a cold / warm / shifted sequence across a level move, one penalty level: same status, iteration count, final
    level and ok flag; x, u, y, lam and the residuals to 1e-9 max(1, |reference|)"""
    got = _hold(mpc, name)
    if name == "soft_gate":        # (a soft neighbour in the wave does not disturb the hard instance's certificate)
        assert list(got[0]["status"]) == ["infeasible", "optimal"] and got[0]["iters"][0] % 8 == 0 and got[0]["iters"][0] > 0
    if name == "soft_x0_outside":
        assert list(got[0]["status"]) == ["optimal", "infeasible", "optimal", "optimal", "optimal"] and got[0]["iters"][1] == 0
    if name == "soft_embedded":
        assert got[0]["x"].shape[-1] == 3 and got[0]["u"].shape[-1] == 2
    if name == "soft_terminal_sequence":
        assert len(got) == 3 and np.all(got[0]["level"] != 3) and np.all(got[2]["status"] == "optimal")
    if name == "soft_terminal_fixed":
        assert np.all(got[0]["level"] == 0)


@pytest.mark.parametrize("name", so.SCIPY_GPU)
def test_final_solutions_are_the_slack_qp_solutions(mpc, name):
    """the kernel's u against the slack-variable SciPy solve, at the 2e-3 of the CPU test"""
    c = so.build(name)
    prob = so.make_problem(mpc, c)
    _, traj, status = prob.solve(c.x0[:2], **c.steps[0]["kw"])
    for b in so.scipy_instances(name):
        dev = np.max(np.abs(np.asarray(traj.uTraj)[b] - so.scipy_solution(name, b)[1]))
        print(f"{name} instance {b}: deviation of u from the slack QP {dev:.2e}")
        assert status[b] == "optimal" and dev <= 2e-3


# ---- update ----------------------------------------------------------------------------------------------------------------------------------

def _other(soft):
    """other weights on the same components, and one more soft component"""
    out = []
    for l1, l2 in soft:
        fin = np.isfinite(l1)
        n1, n2 = np.where(fin, 2.0 * l1 + 0.01, INF), np.where(fin, l2 + 0.25, 0.0)
        hard = np.flatnonzero(~fin)
        if len(hard):
            n1[hard[-1]], n2[hard[-1]] = 0.03, 0.5
        out.append((n1, n2))
    return out


@pytest.mark.parametrize("name,device", [("soft_terminal", False), ("soft_per_problem", True), ("soft_embedded", False)])
def test_update_of_the_weights_keeps_the_tables(mpc, name, device):
    """new weights leave the table tensors where they are (the same objects, the same data_ptr: no setup launch) and the workspace in
    place; a cold solve then equals a freshly built object's bit for bit and differs from the old weights'; an update to all-inf weights
    gives the hard solve, that of the stage entry.  device: the new weights go in as device tensors."""
    import torch
    c = so.build(name)
    nb, N = len(c.x0), c.N
    prob = so.make_problem(mpc, c)
    refs = {} if c.xRef is None else dict(xRef=c.xRef, uRef=c.uRef)
    kw = dict(rho=prob.rho, warm_start=False, **refs, **c.steps[0]["kw"])
    before = _solve(prob, c.x0, nb, N, **kw)
    new = _other(c.soft)
    n = c.inst[0][1].shape[-2]
    stack = lambda i, part: (new[0][i][part] if c.shared else np.stack([w[i][part] for w in new]))
    give = (lambda v: torch.as_tensor(v, device="cuda")) if device else (lambda v: v)
    xs, us = slice(0, n), slice(n, None)
    tabs, ws = dict(prob._tables), prob._ws
    held = [t for t in next(iter(tabs.values())) if torch.is_tensor(t)]
    ptrs = [t.data_ptr() for t in held]
    prob.update(x_soft_l1=give(stack(0, xs)), x_soft_l2=give(stack(1, xs)), u_soft_l1=give(stack(0, us)), u_soft_l2=give(stack(1, us)))
    assert prob._ws is ws and list(prob._tables) == list(tabs)
    now = [t for t in next(iter(prob._tables.values())) if torch.is_tensor(t)]
    assert all(a is b for a, b in zip(now, held)) and [t.data_ptr() for t in now] == ptrs
    got = _solve(prob, c.x0, nb, N, **kw)
    _identical(got, _solve(so.make_problem(mpc, c, soft=new), c.x0, nb, N, **kw), (name, "new weights"))
    assert not np.array_equal(got["u"], before["u"])                                                 # (the new weights do matter)
    width = (n, len(new[0][0]) - n)
    lead = () if c.shared else (len(c.inst),)
    ws = prob._ws
    prob.update(x_soft_l1=np.full(lead + width[:1], INF), x_soft_l2=np.zeros(lead + width[:1]), u_soft_l2=np.zeros(lead + width[1:]),
                u_soft_l1=np.full(lead + width[1:], INF))
    assert list(prob._tables) == list(tabs) and prob._ws is ws
    hard = _solve(prob, c.x0, nb, N, **kw)
    _identical(hard, _solve(sr.make_problem(mpc, c), c.x0, nb, N, **kw), (name, "all hard"))
    assert not np.array_equal(hard["u"], got["u"])
