"""Inputs, references and comparison of tests/test_mpc_iterates_gpu.py; a helper module, not collected as a test.

Every case is a batch of lqrMpc instances and a chain of solves on ONE lqrMpc object.  `reference(name)` restates every instance of every
solve with oracle.mpc_oracle.admm_levels (fed its own previous final state in a chain, never the kernel's); tests/test_mpc_levels_oracle.py
checks, without a GPU, that each of these references stays clear of every rounding-sensitive decision and that the cases cover what they
claim; tests/test_mpc_iterates_gpu.py runs the kernels on the same inputs and holds them to the references with `compare`."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

from oracle import mpc_oracle as mo
from tests import mpc_tracking_ref as tr

TOL = 1e-9   # the suite's iterate tolerance (tests/test_mpc_gpu.py, tests/test_mpc_tracking_gpu.py): 1e-9 max(1, max |reference|)


def _random(n, m, N, seed, nb, bad=None):
    """the random stable problem of tests/test_mpc_gpu.py, state box 4, input box 0.15; instance `bad` starts outside its box"""
    from tests.test_mpc_gpu import _random_problem
    rng = np.random.default_rng(seed)
    A, B, Q, R, Qf = _random_problem(rng, n, m, N)
    x_ub, u_ub = np.full(n, 4.0), np.full(m, 0.15)
    x0 = rng.uniform(-1.0, 1.0, (nb, n))
    if bad is not None:
        x0[bad, 0] = 5.0
    return (A, B, Q, R, Qf, -x_ub, x_ub, -u_ub, u_ub), x0


def _quad_x0(nb, seed, spread=10.0, rate=0.03):
    """the starts of tests/test_mpc_gpu.py: small rates and attitudes (deviation `rate`), positions up to `spread` m from the origin"""
    x_ub = tr.quad_data(2)[6]
    rng = np.random.default_rng(seed)
    x0 = np.clip(rate * rng.standard_normal((nb, 12)), -x_ub + 1e-6, x_ub - 1e-6)
    x0[:, 9:12] = rng.uniform(-spread, spread, (nb, 3))
    return x0


def _shared(data, N, x0, steps, **more):
    A, B, Q, R, Qf, xl, xu, ul, uu = data
    c = SimpleNamespace(ctor=(A, B, Q, R, N, xl, xu, ul, uu), Qf=Qf, N=N, x0=x0, inst=[data] * len(x0), steps=steps, xRef=None,
                        uRef=None, n_levels=7)
    c.__dict__.update(more)
    return c


def _per_problem(n, m, N, seed, x_scale, steps, track=False):
    from tests.test_mpc_batched import _family
    A, B, Q, R, xl, xu, ul, uu = _family((5,), n, m, seed=seed)
    rng = np.random.default_rng(seed + 1)
    x0 = x_scale * xu * rng.uniform(-1, 1, (5, n))
    c = SimpleNamespace(ctor=(A, B, Q, R, N, xl, xu, ul, uu), Qf=None, N=N, x0=x0, steps=steps, xRef=None, uRef=None, n_levels=7,
                        inst=[(A[i], B[i], Q[i], R[i], Q[i], xl[i], xu[i], ul[i], uu[i]) for i in range(5)])
    if track:   # references that leave each problem's own box
        t = np.arange(N + 1)
        c.xRef = 1.5 * xu[:, None, :] * np.sin(2 * np.pi * t[None, :, None] / N + rng.uniform(0, 2 * np.pi, (5, 1, n)))
        c.uRef = 2.0 * uu[:, None, :] * (t[None, :N, None] / N) * np.sign(rng.standard_normal((5, 1, m)))
    return c


def _kw(eps, max_iter=30000, **more):
    return dict(eps_abs=eps, eps_rel=eps, max_iter=max_iter, **more)


COLD = lambda eps, **kw: [dict(kw=_kw(eps, **kw), warm=False, x0="given")]
# a solve, a warm refinement of it, a shifted solve from the second state of the refined plan
CHAIN = lambda e0, e1, **kw: [dict(kw=_kw(e0, **kw), warm=False, x0="given"), dict(kw=_kw(e1, **kw), warm=True, x0="given"),
                              dict(kw=_kw(e1, **kw), warm="shift", x0="x1")]

# (n, m, N) of the compiled 16-lane shapes: every shape at two horizons of different N mod 3, N = 1 and N = 2 at (12, 4)
SHAPES = [(1, 1, 2), (1, 1, 3), (2, 1, 4), (2, 1, 5), (2, 2, 1), (2, 2, 3), (4, 1, 5), (4, 1, 7), (4, 2, 2), (4, 2, 4), (8, 4, 3), (8, 4, 7),
          (12, 4, 1), (12, 4, 2), (12, 4, 7)]
EMBEDDED = [(3, 2, 5), (5, 3, 4), (9, 4, 7)]
LANE = [(13, 2, 6), (16, 5, 5), (24, 8, 4), (4, 2, 80)]
LANE_CHILD = [(12, 4, 10), (2, 1, 3)]
CAPS = [5, 16, 30]


def _seed(n, m, N):
    """(a seed that fails a condition of tests/test_mpc_levels_oracle.py is replaced here, never skipped; none has so far)"""
    return 1000 * n + 10 * m + N


@functools.lru_cache(maxsize=None)
def build(name):
    kind, *arg = name.split(":")
    shape = tuple(int(v) for v in arg[0].split(",")) if arg else None
    if kind == "shape":       # batch 7: two waves, the second with an idle group; the middle instance starts outside its box
        n, m, N = shape
        data, x0 = _random(n, m, N, _seed(n, m, N), 7, bad=3)
        return _shared(data, N, x0, COLD(1e-6))
    if kind == "embedded":
        n, m, N = shape
        data, x0 = _random(n, m, N, _seed(n, m, N), 5)
        return _shared(data, N, x0, COLD(1e-6))
    if kind == "quad":
        return _shared(tr.quad_data(30), 30, _quad_x0(5, 1), COLD(1e-4))
    if kind == "cap":
        return _shared(tr.quad_data(30), 30, _quad_x0(5, 4, spread=3.0), COLD(1e-3, max_iter=shape[0]))
    if kind == "caprandom":   # the quadcopter's weights are all I, so its K_k is the same at every level: a random problem, where it is not
        n, m, N, cap = shape
        data, x0 = _random(n, m, N, _seed(n, m, N), 5)
        return _shared(data, N, x0, COLD(1e-6, max_iter=cap))
    if kind == "perproblem":
        n, m, N = shape
        return _per_problem(n, m, N, 10 * n + m, 0.9 if n == 4 else 0.3, COLD(1e-5, max_iter=3000))
    if kind == "infeasible":  # tests/test_mpc_gpu.py: test_infeasible_instances (b), x1 = 2 x0 + u with |u| <= 0.1 leaves |x| <= 1
        I, one = np.eye(2), np.ones(2)
        return _shared((2 * I, I, I, I, I, -one, one, -0.1 * one, 0.1 * one), 3, np.array([[0.9, 0.9], [0.09, -0.09], [0.01, -0.01]]), COLD(1e-5))
    if kind == "warm":        # the first call's cap holds the slowest instance back from "optimal": its slot starts the second call cold
        N, cap = shape
        steps = CHAIN(1e-3, 1e-5)
        steps[0]["kw"]["max_iter"] = cap
        seed, rate = {10: (5, 0.08), 30: (4, 0.03)}[N]     # (N = 10: larger rates, or no bound is active on so short a horizon)
        return _shared(tr.quad_data(N), N, _quad_x0(5, seed, spread=5.0, rate=rate), steps)
    if kind == "track":
        n, m, N = shape
        data, x0, xRef, uRef = tr.random_case(n, m, N, seed=41, nb=8)
        return _shared(data, N, x0, COLD(1e-6), xRef=xRef, uRef=uRef)
    if kind == "trackquad":
        x0, xRef, uRef = tr.quad_reference(25, nb=3, seed=0)
        return _shared(tr.quad_data(25), 25, x0, COLD(1e-5), xRef=xRef, uRef=uRef)
    if kind == "trackperproblem":
        return _per_problem(4, 2, 8, 5, 0.3, COLD(1e-5, max_iter=3000), track=True)
    if kind in ("lane", "lanechild"):   # the lane-per-instance kernel runs the level-`level0` penalty whatever adaptive_rho says
        n, m, N = shape
        data, x0 = _random(n, m, N, _seed(n, m, N), 4)
        c = _shared(data, N, x0, CHAIN(1e-4, 1e-6))
        c.n_levels, c.lane = 1, True
        return c
    if kind == "unstable":    # an open-loop-unstable plant (problems.hard_mpc: lti_unstable, spectral radius 1.3), inputs within 0.5, no state
        n, m, N = shape       # box; x0 = 1.2 randn is small enough to be feasible and large enough for active input bounds
        from tests import problems
        A, B, _, Qs, Rs, _ = (X[0] for X in problems.hard_mpc("lti_unstable", n, m, N))
        inf, u_ub = np.full(n, np.inf), np.full(m, 0.5)
        x0 = 1.2 * np.random.default_rng(100 * n + N).standard_normal((5, n))
        return _shared((A[0], B[0], Qs[0], Rs[0], Qs[N - 1], -inf, inf, -u_ub, u_ub), N, x0, COLD(1e-6))
    raise KeyError(name)


# the tests of tests/test_mpc_iterates_gpu.py: their cases and the statuses they claim to cover
GROUPS = {
    "shapes": ([f"shape:{n},{m},{N}" for n, m, N in SHAPES], {"optimal", "infeasible"}),
    "quadcopter": (["quad"], {"optimal"}),
    "embedded": ([f"embedded:{n},{m},{N}" for n, m, N in EMBEDDED], {"optimal"}),
    "per_problem": (["perproblem:4,2,6", "perproblem:12,4,10"], {"optimal", "infeasible"}),
    "infeasible": (["infeasible"], {"optimal", "infeasible"}),
    "cap": ([f"cap:{c}" for c in CAPS] + ["caprandom:8,4,7,16"], {"optimal", "optimal_inaccurate", "user_limit"}),
    "warm": (["warm:10,20", "warm:30,120"], {"optimal", "optimal_inaccurate", "user_limit"}),
    "tracking": (["track:4,1,8", "trackquad", "trackperproblem"], {"optimal"}),
    "lane": ([f"lane:{n},{m},{N}" for n, m, N in LANE], {"optimal"}),
    "lane_child": ([f"lanechild:{n},{m},{N}" for n, m, N in LANE_CHILD], {"optimal"}),
    "unstable": (["unstable:12,4,40"], {"optimal"}),
}
ALL = [name for names, _ in GROUPS.values() for name in names]


def make_problem(mpcUtils, c):
    """the lqrMpc object of a case (host side only: no GPU is touched before the first solve)"""
    return mpcUtils.lqrMpc(*c.ctor) if c.Qf is None else mpcUtils.lqrMpc(*c.ctor, Qf=c.Qf)


@functools.lru_cache(maxsize=None)
def reference(name):
    """[step][instance] -> admm_levels result; `x0` of the step is kept on each result"""
    from zopt_amd import mpcUtils
    c = build(name)
    rho = np.broadcast_to(make_problem(mpcUtils, c).rho, (len(c.x0),))
    out = []
    for s, step in enumerate(c.steps):
        row = []
        for b, (A, B, Q, R, Qf, xl, xu, ul, uu) in enumerate(c.inst):
            prev = out[-1][b] if s else None
            x0 = prev.x[1] if step["x0"] == "x1" else c.x0[b]
            warm = (prev.y, prev.lam, prev.level) if (step["warm"] and prev.status == "optimal") else None
            g = None if c.xRef is None else tr.linear_term(Q, R, Qf, c.N, c.xRef[b], c.uRef[b])
            r = mo.admm_levels(A, B, Q, R, Qf, c.N, xl, xu, ul, uu, x0, rho=float(rho[b]), n_levels=c.n_levels, g=g, warm=warm,
                               shift=step["warm"] == "shift", **step["kw"])
            r.x0 = x0
            row.append(r)
        out.append(row)
    return out


def read_state(prob, nb, N, lane=False):
    """(y (nb, N, n+m), lam (nb, N, n+m), level (nb,), ok (nb,)) of the last solve, read back from its workspace: the state a warm start
    reads.  16-lane kernels (mpc_solve_wave_body.h): per instance [y (N, W) | lam (N, W) | kf (N, MC), ok flag, level | unused], W the
    compiled n + m; the lane kernel (mpc_solve_lane_body.h) keeps y[k][i][inst], lam[k][i][inst], the ok flags after kf, and no level.
    Padded components of an embedded shape are dropped."""
    ws = prob._ws[1].cpu().numpy()
    W, MC = prob.n + prob.m, prob.m
    cols = list(range(prob._n_user)) + list(range(prob.n, prob.n + prob._m_user))
    if lane:
        y = ws[:N * W * nb].reshape(N, W, nb).transpose(2, 0, 1)
        lam = ws[N * W * nb:2 * N * W * nb].reshape(N, W, nb).transpose(2, 0, 1)
        ok = ws[2 * N * W * nb + N * MC * nb:][:nb]
        return y[:, :, cols], lam[:, :, cols], None, ok
    blk = ws[:4 * N * W * nb].reshape(nb, 4 * N * W)
    y, lam = blk[:, :N * W].reshape(nb, N, W), blk[:, N * W:2 * N * W].reshape(nb, N, W)
    flag = 2 * N * W + N * MC
    return y[:, :, cols], lam[:, :, cols], blk[:, flag + 1].astype(int), blk[:, flag]


def run_kernel(mpcUtils, name):
    """every solve of the case on one lqrMpc object -> [step] dict of arrays"""
    c, ref = build(name), reference(name)
    prob = make_problem(mpcUtils, c)
    nb = len(c.x0)
    got = []
    for s, step in enumerate(c.steps):
        x0 = np.stack([r.x0 for r in ref[s]])
        extra = {} if c.xRef is None else dict(xRef=c.xRef, uRef=c.uRef)
        _, traj, status = prob.solve(x0, warm_start=step["warm"], **extra, **step["kw"])
        y, lam, level, ok = read_state(prob, nb, c.N, lane=getattr(c, "lane", False))
        got.append(dict(x=np.asarray(traj.xTraj), u=np.asarray(traj.uTraj), status=np.asarray(status, dtype=str),
                        iters=prob.last_iterations.copy(), resid=prob.last_residuals.copy(), y=y, lam=lam, ok=ok,
                        level=np.zeros(nb, dtype=int) if level is None else level))
    return got


def compare(name, got):
    """hold every instance of every solve to its reference; returns the largest iterate deviation relative to its bound (<= 1)"""
    c, ref = build(name), reference(name)
    worst = 0.0
    for s, (row, g) in enumerate(zip(ref, got)):
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
            if c.n_levels > 1:
                assert g["level"][b] == r.level, (at, g["level"][b], r.level)
            worst = max(worst, max(dev.values()))
    return worst
