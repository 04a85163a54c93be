"""Cases, restatement adapter and comparison for mpcUtils.lqrMpc with soft box constraints (`lqrMpc.soften`: zm_mpc_solve_soft_f64,
zm_mpc_closed_loop_soft_f64); a helper module, not collected as a test.

The restatement is oracle.mpc_oracle.admm_levels_stage on constant rows -- A_k = A, B_k = B, c = None, mo.stage_form(Q, R, Qf, N, ...) --
with the weights l1, l2 (n + m,) of the instance's problem in the stacked layout [x ; u]: `restate`.  Every case is a batch of instances
and a chain of solves on ONE softened lqrMpc object; `reference(name)` restates every instance of every solve (fed its own previous final
state in a chain, never the kernel's), `run_kernel` runs the kernels on the same inputs and `compare` holds them to the references by the
rule of tests/mpc_iterates_cases.py: compare.  tests/test_mpc_soft.py checks without a GPU that every reference stays clear of every
rounding-sensitive decision and that the cases cover what they claim.

The closed-loop inputs (`loop_case`) come with `restated_loop`, the loop `lqrMpc.simulate` documents written over the restatement."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

from oracle import mpc_oracle as mo
from tests import mpc_tracking_ref as tr
from tests.mpc_iterates_cases import CHAIN, COLD, TOL, _kw, _random, read_state
from tests.mpc_ltv_soft_ref import SCALAR, _weights

INF = np.inf


def restate(data, l1, l2, x0, rho, g=None, warm=None, shift=False, **kw):
    """one instance: admm_levels_stage on the constant rows of lqrMpc's data (A, B, Q, R, Qf, x_lb, x_ub, u_lb, u_ub)"""
    A, B, Q, R, Qf, xl, xu, ul, uu = data
    N = kw.pop("N")
    return mo.admm_levels_stage(np.tile(A, (N, 1, 1)), np.tile(B, (N, 1, 1)), None, *mo.stage_args(Q, R, Qf, N, xl, xu, ul, uu), x0, l1, l2,
                                rho=rho, g=g, warm=warm, shift=shift, **kw)


def soften_kw(n, soft):
    """the four keywords of `soften` from per-problem stacked (l1, l2) rows: one problem (n + m,), or a list of them (P, n + m)"""
    l1, l2 = (np.asarray(v) for v in (zip(*soft) if isinstance(soft, list) else soft))
    l1, l2 = np.array(l1), np.array(l2)
    return dict(x_soft_l1=l1[..., :n], x_soft_l2=l2[..., :n], u_soft_l1=l1[..., n:], u_soft_l2=l2[..., n:])


def _case(data, N, x0, steps, soft, **more):
    """shared data: every instance solves the one problem with the weights `soft` = (l1, l2)"""
    A, B, Q, R, Qf, xl, xu, ul, uu = data
    c = SimpleNamespace(ctor=(A, B, Q, R, N, xl, xu, ul, uu), Qf=Qf, N=N, x0=x0, inst=[data] * len(x0), soft=[soft] * len(x0),
                        soften=soften_kw(B.shape[0], soft), steps=steps, xRef=None, uRef=None, witness=0)
    c.__dict__.update(more)
    return c


def _scalar():
    """so.scalar_data in lqrMpc's data: x+ = x + u, Q = R = Qf = 1, N = 1, x0 = 1 outside x <= 0 -- three problems, one per (l1, l2)"""
    one = np.ones((3, 1, 1))
    xl, xu, ul, uu = np.full((3, 1), -INF), np.zeros((3, 1)), np.full((3, 1), -INF), np.full((3, 1), INF)
    soft = [_weights(1, 1, x1={0: w[0]}, x2={0: w[1]}) for w, _ in SCALAR]
    inst = [(one[i], one[i], one[i], one[i], one[i], xl[i], xu[i], ul[i], uu[i]) for i in range(3)]
    return SimpleNamespace(ctor=(one, one, one, one, 1, xl, xu, ul, uu), Qf=None, N=1, x0=np.ones((3, 1)), inst=inst, soft=soft,
                           soften=soften_kw(1, soft), steps=COLD(1e-7), xRef=None, uRef=None, witness=0)


def _per_problem():
    """(4, 1), N = 5, six problems, one instance each (a batch shape must broadcast with the problem shape, so batch 6 is P = (6,)): one wave
    holds instances of four problems, the second wave two and two idle groups.  Problems 0 and 5 are all hard; 1, 3, 4 soft with their own
    weights; problem 2 is hard and truly infeasible (x+ = 2 x + B u with a small input box leaves its state box: a certificate, not the x0
    test).  Each is the random stable problem of tests/mpc_iterates_cases.py with a seed of its own.  The second step of the case runs the fixed penalty."""
    n, m, N = 4, 1, 5
    parts = [_random(n, m, N, 4150 + i, 1) for i in range(6)]
    A, B, Q, R, Qf, xl, xu, ul, uu = (np.stack([d[k] for d, _ in parts]) for k in range(9))
    x0 = np.concatenate([x for _, x in parts])
    A[2], B[2] = 2.0 * np.eye(n), 0.1 * np.ones((n, m))
    x0[2] = 0.9 * xu[2]
    for i, k, start in ((1, 0, 0.45), (3, 1, -0.4), (4, 2, 0.5)):       # the soft components: a box of half-width 0.3, a start outside it
        x0[i] *= 0.3                                                    # (small starts: with one input within 0.15 a larger one drives
        xl[i, k], xu[i, k], x0[i, k] = -0.3, 0.3, start                 # a HARD component out of its box, which no weight can mend)
    soft = [_weights(n, m), _weights(n, m, x1={0: 6.0}), _weights(n, m), _weights(n, m, x1={1: 2.0, 3: 1.0}, x2={1: 4.0}, u1={0: 0.5}),
            _weights(n, m, x1={2: 0.0}, x2={2: 30.0}), _weights(n, m)]
    inst = [(A[i], B[i], Q[i], R[i], Qf[i], xl[i], xu[i], ul[i], uu[i]) for i in range(6)]
    steps = COLD(1e-5, max_iter=3000) + [dict(kw=_kw(1e-5, max_iter=3000, n_levels=1), warm=False, x0="given")]
    return SimpleNamespace(ctor=(A, B, Q, R, N, xl, xu, ul, uu), Qf=Qf, N=N, x0=x0, inst=inst, soft=soft, soften=soften_kw(n, soft),
                           steps=steps, xRef=None, uRef=None, witness=1)


@functools.lru_cache(maxsize=None)
def build(name):
    """(a seed that fails a condition of tests/test_mpc_soft.py is replaced here, never skipped)"""
    if name == "scalar":
        return _scalar()
    if name == "x0_outside":      # (2, 2), N = 2, batch 5: state 0 soft with a box of half-width 1, starts inside (0), on (1) and outside
        (A, B, Q, R, Qf, xl, xu, ul, uu), x0 = _random(2, 2, 2, 2022, 5)      # (2, 4) it; instance 3 starts outside in the hard state 1:
        xl, xu = xl.copy(), xu.copy()                                         # refused, and its neighbours in the wave are solved
        xl[0], xu[0] = -1.0, 1.0
        x0[:, 0] = [0.3, 1.0, 1.5, 0.2, -1.7]
        x0[3, 1] = 5.0
        return _case((A, B, Q, R, Qf, xl, xu, ul, uu), 2, x0, COLD(1e-6), _weights(2, 2, x1={0: 3.0}), witness=2)
    if name == "quadratic":       # (4, 2), N = 7, batch 5: l1 = 0, l2 > 0 on state 0 (starts up to 0.6 outside) and on input 1 (box 0.15)
        data, x0 = _random(4, 2, 7, 4027, 5)
        x0[:, 0] = [4.6, 3.9, -4.3, 4.2, 1.0]
        return _case(data, 7, x0, COLD(1e-6), _weights(4, 2, x1={0: 0.0}, x2={0: 3.0}, u1={1: 0.0}, u2={1: 1.5}))
    if name == "full_tile":       # (12, 4), N = 7, batch 5: no lane outside a role; references of amplitude 3 under soft boxes of
        n, m, N = 12, 4, 7        # half-width 0.6 on states 0..2 -- the tracking term and the soft term together
        (A, B, Q, R, Qf, xl, xu, ul, uu), x0 = _random(n, m, N, 12047, 5)
        xl, xu = xl.copy(), xu.copy()
        xl[:3], xu[:3] = -0.6, 0.6
        rng = np.random.default_rng(21)
        k = np.arange(N + 1)
        xRef = 3.0 * np.sin(0.7 * k[None, :, None] + rng.uniform(0, 6, (5, 1, n)))
        return _case((A, B, Q, R, Qf, xl, xu, ul, uu), N, x0, COLD(1e-6), _weights(n, m, x1={0: 1.0, 1: 0.5, 2: 2.0}, x2={1: 1.0}),
                     xRef=xRef, uRef=np.zeros((5, N, m)))
    if name == "embedded":        # (3, 2) in the (4, 2) kernels, N = 3, batch 9: state 1 and input 0 soft; the padded state is hard
        data, x0 = _random(3, 2, 3, 3023, 9)
        x0[:, 1] = np.linspace(3.6, 4.8, 9)
        return _case(data, 3, x0, COLD(1e-6), _weights(3, 2, x1={1: 0.5}, u1={0: 0.2}, u2={0: 0.3}), witness=8)
    if name == "per_problem":
        return _per_problem()
    if name == "sequence":        # (4, 2), N = 5, batch 5: cold at a loose tolerance, warm, shifted from x_1, then cold at the fixed penalty;
        data, x0 = _random(4, 2, 5, 3, 5)         # every start 0.5 outside the box in the soft state 0
        x0[:, 0] = 4.5
        steps = CHAIN(1e-3, 1e-6) + [dict(kw=_kw(1e-6, n_levels=1), warm=False, x0="given")]
        return _case(data, 5, x0, steps, _weights(4, 2, x1={0: 20.0}))
    raise KeyError(name)


CASES = ["scalar", "x0_outside", "quadratic", "full_tile", "embedded", "per_problem", "sequence"]
SCIPY = {"scalar": (0, 1, 2), "x0_outside": (0, 2), "embedded": (0, 8)}     # the small cases and the instances whose slack QP is solved


def make_problem(mpcUtils, c, soft=True):
    """the lqrMpc object of a case (host side only: no GPU is touched before the first solve), softened with the case's weights"""
    prob = mpcUtils.lqrMpc(*c.ctor) if c.Qf is None else mpcUtils.lqrMpc(*c.ctor, Qf=c.Qf)
    return prob.soften(**c.soften) if soft else prob


def _options(step):
    """a step's options for the restatement (n_levels as it spells the fixed penalty)"""
    return dict(step["kw"])


def _solve_options(step):
    """... and for `solve`, which spells it adaptive_rho=False"""
    kw = dict(step["kw"])
    if kw.pop("n_levels", None) == 1:
        kw["adaptive_rho"] = False
    return kw


def reference_steps(c, soft=None):
    """[step][instance] -> admm_levels_stage result of the case with the weights `soft` per instance (default: the case's); `x0` of the
    step is kept on each result"""
    from zopt_amd import mpcUtils
    soft = c.soft if soft is None else soft
    rho = np.broadcast_to(make_problem(mpcUtils, c, soft=False).rho, (len(c.x0),))
    out = []
    for s, step in enumerate(c.steps):
        row = []
        for b, data in enumerate(c.inst):
            prev = out[-1][b] if s else None
            x0 = prev.x[1] if step["x0"] == "x1" else c.x0[b]
            warm = (prev.y, prev.lam, prev.level) if (step["warm"] and prev.status == "optimal") else None
            g = None if c.xRef is None else tr.linear_term(data[2], data[3], data[4], c.N, c.xRef[b], c.uRef[b])
            r = restate(data, *soft[b], x0, float(rho[b]), g=g, warm=warm, shift=step["warm"] == "shift", N=c.N, **_options(step))
            r.x0 = x0
            row.append(r)
        out.append(row)
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    return reference_steps(build(name))


@functools.lru_cache(maxsize=None)
def hard_twin(name):
    """the first step of the case with every component hard"""
    c = build(name)
    n, m = c.inst[0][1].shape
    twin = SimpleNamespace(**{**c.__dict__, "steps": c.steps[:1]})
    return reference_steps(twin, [_weights(n, m)] * len(c.x0))[0]


@functools.lru_cache(maxsize=None)
def scipy_solution(name, b):
    """(x, u) of the slack QP of instance b (references included)"""
    c = build(name)
    A, B, Q, R, Qf, xl, xu, ul, uu = c.inst[b]
    N = c.N
    ref = {} if c.xRef is None else dict(xRef=c.xRef[b], uRef=c.uRef[b])
    x, u, _ = mo.solve_reference_stage(np.tile(A, (N, 1, 1)), np.tile(B, (N, 1, 1)), None, *mo.stage_args(Q, R, Qf, N, xl, xu, ul, uu),
                                       c.x0[b], *c.soft[b], **ref)
    return x, u


def run_kernel(mpcUtils, name):
    """every solve of the case on one softened lqrMpc object -> [step] dict of arrays"""
    c, ref = build(name), reference(name)
    prob = make_problem(mpcUtils, c)
    nb = len(c.x0)
    got = []
    for s, step in enumerate(c.steps):
        x0 = np.stack([r.x0 for r in ref[s]])
        extra = {} if c.xRef is None else dict(xRef=c.xRef, uRef=c.uRef)
        _, traj, status = prob.solve(x0, warm_start=step["warm"], **extra, **_solve_options(step))
        y, lam, level, ok = read_state(prob, nb, c.N)
        got.append(dict(x=np.asarray(traj.xTraj), u=np.asarray(traj.uTraj), status=np.asarray(status, dtype=str),
                        iters=prob.last_iterations.copy(), resid=prob.last_residuals.copy(), y=y, lam=lam, ok=ok, level=level))
    return got


def compare(name, got):
    """tests/mpc_iterates_cases.py: compare, on this module's cases -- every instance of every solve has its reference's status, iteration
    count and final level, and x, u, y, lam and the residuals within TOL of it; returns the largest deviation relative to its bound"""
    c, ref = build(name), reference(name)
    worst = 0.0
    for s, (row, g) in enumerate(zip(ref, got)):
        fixed = c.steps[s]["kw"].get("n_levels") == 1
        for b, r in enumerate(row):
            at = f"{name} step {s} instance {b}"
            assert g["status"][b] == r.status, (at, g["status"][b], r.status, int(g["iters"][b]), r.iters)
            assert int(g["iters"][b]) == r.iters, (at, int(g["iters"][b]), r.iters)
            scale = TOL * max(1.0, np.max(np.abs(r.x)), np.max(np.abs(r.u)))
            dev = {"x": np.max(np.abs(g["x"][b] - r.x)) / scale, "u": np.max(np.abs(g["u"][b] - r.u)) / scale,
                   "rp": abs(g["resid"][b, 0] - r.rp) / (2 * scale), "rd": abs(g["resid"][b, 1] - r.rd) / (2 * scale * r.rho_final),
                   "y": np.max(np.abs(g["y"][b] - r.y)) / (TOL * max(1.0, np.max(np.abs(r.y)))),
                   "lam": np.max(np.abs(g["lam"][b] - r.lam)) / (TOL * max(1.0, np.max(np.abs(r.lam))))}
            assert max(dev.values()) <= 1.0, (at, dev)
            assert g["ok"][b] == (1.0 if r.status == "optimal" else 0.0), at
            assert g["level"][b] == (0 if fixed else r.level), (at, g["level"][b], r.level)     # (one table: its level is 0)
            worst = max(worst, max(dev.values()))
    return worst


# ---- closed loop -------------------------------------------------------------------------------------------------------------------------

STEPS, GUST_STEP = 6, 2
LOOP_SHAPES = [(4, 2, 5), (12, 4, 7)]


@functools.lru_cache(maxsize=None)
def loop_case(n, m, N, nb):
    """The random stable problem with a box of half-width 1.2 on state 0, which is soft (l1 = 20: above the multipliers, so the run keeps
    to the box while it can); `nb` starts inside; a gust at step GUST_STEP that puts state 0 of every second instance (the first included)
    0.5 outside its upper bound, wherever the run then is: w = (1.7 - the undisturbed successor) from the restated loop, and small noise in
    every component at every step (so that no clip is a no-op by accident).  Returns (data, (l1, l2), x0, w (nb, STEPS, n))."""
    (A, B, Q, R, Qf, xl, xu, ul, uu), x0 = _random(n, m, N, 1000 * n + 10 * m + N, nb)
    xl, xu = xl.copy(), xu.copy()
    xl[0], xu[0] = -1.2, 1.2
    data = (A, B, Q, R, Qf, xl, xu, ul, uu)
    soft = _weights(n, m, x1={0: 20.0})
    rng = np.random.default_rng(7 * n + N)
    w = 0.01 * rng.standard_normal((nb, STEPS, n))
    w[:, GUST_STEP:] = 0.0
    calm = restated_loop(data, soft, x0, w, GUST_STEP + 1, N)
    for b in range(0, nb, 2):
        w[b, GUST_STEP, 0] = 1.7 - calm.px[b, GUST_STEP, 1, 0]
    return data, soft, x0, w


def restated_loop(data, soft, x0, w, steps, N, clip_tol=1e-6, warm="shift", eps=1e-5, max_iter=10000):
    """the loop `lqrMpc.simulate` documents, written over the restatement, instance by instance: the clip moves the hard state components
    only.  Fields as tests/mpc_closed_loop_cases.py: loop, batch-leading."""
    A, B, Q, R, Qf, xl, xu, ul, uu = data
    n = B.shape[0]
    l1, l2 = soft
    hard = ~np.isfinite(l1[:n])
    rho = tr.default_rho(Q, R)
    clip = (lambda v: v) if clip_tol is None else (lambda v: np.where(hard, np.clip(v, xl + clip_tol, xu - clip_tol), v))
    out = SimpleNamespace(xTraj=[], uTraj=[], status=[], iterations=[], px=[], pu=[])
    for b in range(len(x0)):
        x, prev = np.array(x0[b]), None
        xs, us, st, its, px, pu = [], [], [], [], [], []
        for s in range(steps):
            x = clip(x)
            xs.append(x)
            start = (prev.y, prev.lam, prev.level) if (prev is not None and warm and prev.status == "optimal") else None
            prev = restate(data, l1, l2, x, rho, warm=start, shift=warm == "shift", N=N, eps_abs=eps, eps_rel=eps,
                           max_iter=max_iter)
            us.append(prev.u[0])
            st.append(prev.status)
            its.append(prev.iters)
            px.append(prev.x)
            pu.append(prev.u)
            x = prev.x[1] + w[b, s]
        xs.append(clip(x))
        for k, v in zip(("xTraj", "uTraj", "status", "iterations", "px", "pu"), (xs, us, st, its, px, pu)):
            getattr(out, k).append(np.stack(v))
    for k in ("xTraj", "uTraj", "status", "iterations", "px", "pu"):
        setattr(out, k, np.stack(getattr(out, k)))
    return out

