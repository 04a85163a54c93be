"""CPU checkers and cases for mpcUtils.ltvMpc with soft box constraints (x_soft_l1, x_soft_l2, u_soft_l1, u_soft_l2: a penalty
l1 d + l2 d^2 on the distance d of a component of [x_{k+1} ; u_k] from its box, per problem and component, constant over the stages;
l1 = +inf is a hard component); a helper module, not collected as a test.

  * `admm_levels_ltv_soft`     -- the NumPy restatement of zm_mpc_solve_ltv_soft_f64: the one body of every family itself,
                                  oracle.mpc_oracle.admm_levels_stage, whose data this entry takes in full (x0 test, proximal map `prox`,
                                  support term and guard rule of a soft component: see there).
  * `solve_reference_ltv_soft` -- oracle.mpc_oracle.solve_reference_stage: the condensed SciPy trust-constr solve with one slack e >= 0
                                  per soft (stage, component) that has a finite bound: lo - e <= w <= hi + e, cost + l1 e + l2 e^2.
  * the named cases of tests/test_mpc_ltv_soft.py and tests/test_mpc_ltv_soft_gpu.py, built from the recipes of
    tests/mpc_ltv_stage_ref.py and run through its case glue, with its `run_steps` and comparison rule.

An instance's data is that of tests/mpc_ltv_stage_ref.py followed by the weights l1, l2, each (n + m,) in the stacked layout [x ; u].
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

from oracle.mpc_oracle import admm_levels_stage as admm_levels_ltv_soft  # noqa: F401  (l1 is its 12th argument, l2 its 13th)
from oracle.mpc_oracle import prox, violation  # noqa: F401
from oracle.mpc_oracle import solve_reference_stage as solve_reference_ltv_soft  # noqa: F401
from tests import mpc_ltv_ref as lr
from tests import mpc_ltv_stage_ref as sr

INF = np.inf


# ---- the scalar problem with known answers -------------------------------------------------------------------------------------------------

def scalar_data():
    """x+ = x + u, Q = R = 1, N = 1, x0 = 1, x_1 <= 0: minimise x_1^2 + u^2 + l1 max(0, x_1) + l2 max(0, x_1)^2.  Hard: x_1 = 0 with
    multiplier 2, so any l1 > 2 is exact; l1 = 1: x_1 = 1/4; l1 = 0, l2 = 1: x_1 = 1/3."""
    one = np.ones((1, 1, 1))
    d = [one, one, np.zeros((1, 1)), one, one, np.full((2, 1), -INF), np.array([[INF], [0.0]]), np.full((1, 1), -INF), np.full((1, 1), INF)]
    return d, np.ones(1)


SCALAR = [((1.0, 0.0), 0.25), ((3.0, 0.0), 0.0), ((0.0, 1.0), 1.0 / 3.0)]     # ((l1, l2) on the state, x_1)


# ---- cases -------------------------------------------------------------------------------------------------------------------------------
# As in tests/mpc_ltv_stage_ref.py, with `soft`: per problem (l1, l2), each (n + m,) in the stacked layout.  `witness`: the instance the
# non-vacuity conditions of tests/test_mpc_ltv_soft.py are checked on.

EPS, MAX_ITER = sr.EPS, sr.MAX_ITER
HORIZONS, BATCHES = sr.HORIZONS, sr.BATCHES
problem_of = sr.problem_of


def _weights(n, m, x1=None, x2=None, u1=None, u2=None):
    """(l1, l2) from {component: weight} maps; a component in none is hard"""
    l1, l2 = np.full(n + m, INF), np.zeros(n + m)
    for src, dst, at in ((x1, l1, 0), (x2, l2, 0), (u1, l1, n), (u2, l2, n)):
        for i, w in (src or {}).items():
            dst[at + i] = w
    assert not np.any((l2 > 0) & np.isinf(l1))
    return l1, l2


def _case(inst, soft, x0, N, shared, witness=0, **more):
    c = sr._case(inst, x0, N, shared, None, **more)
    c.soft, c.witness = soft, witness
    return c


def _sequence():
    """a cold solve at a loose tolerance, a warm one from it, a shifted one from x_1"""
    return [dict(kw=lr._kw(eps=1e-3), warm=False, x0="given"), dict(kw=lr._kw(), warm=True, x0="same"),
            dict(kw=lr._kw(), warm="shift", x0="x1")]


@functools.lru_cache(maxsize=None)
def build(name):
    if name == "soft_gate":          # P = (2,): the closed gate of tests/mpc_ltv_stage_ref.py, hard, and its twin with l1 = 2 on state 0
        (d, x0) = sr.gate_data(True)
        return _case([d, [v.copy() for v in d]], [_weights(2, 2), _weights(2, 2, x1={0: 2.0})], np.stack([x0, x0]), 3, False, witness=1,
                     rho=2.0)
    if name == "soft_x0_outside":    # (2, 2), N = 2, batch 5: state 0 soft with a box of half-width 1 about the first start at every row,
        n, m, N = 2, 2, 2            # state 1 hard; instance 3 starts outside in state 0 (solved), instance 1 outside in state 1 (refused)
        d, x0 = sr._base(n, m, N, 5, spread=0.2)
        d[5][:, 0], d[6][:, 0] = x0[0, 0] - 1.0, x0[0, 0] + 1.0
        d[5][0, 1], d[6][0, 1] = x0[0, 1] - 1.0, x0[0, 1] + 1.0
        x0 = x0.copy()
        x0[3, 0] += 1.5
        x0[1, 1] += 1.5
        return _case([d], [_weights(n, m, x1={0: 0.3})], x0, N, True, witness=3)
    if name in ("soft_terminal", "soft_terminal_sequence", "soft_terminal_fixed"):
        n, m, N = 2, 1, 5            # (2, 1), N = 5, batch 9: the terminal set of terminal_box under an l1 too small to reach it
        d, x0 = sr._base(n, m, N, 9, u_box=1.5)
        x, u = sr._plan(d, x0[0], N)
        d[5][N], d[6][N] = x[N] + 0.1, x[N] + 0.2
        more = {}
        if name == "soft_terminal_sequence":
            more["steps"] = _sequence()
        if name == "soft_terminal_fixed":
            more["steps"] = [dict(kw=lr._kw(n_levels=1), warm=False, x0="given")]
        return _case([d], [_weights(n, m, x1={0: 0.05, 1: 0.08})], x0, N, True, **more)
    if name == "soft_quadratic":     # (4, 2), N = 7, batch 5: the corridor and gate of moving_boxes with l1 = 0, l2 > 0 on state 0 and on
        n, m, N = 4, 2, 7            # input 1, whose box opens along the horizon
        c = sr.build("moving_boxes")
        d = [v.copy() for v in c.inst[0]]
        return _case([d], [_weights(n, m, x1={0: 0.0}, x2={0: 3.0}, u1={1: 0.0}, u2={1: 1.5})], c.x0, N, True)
    if name == "soft_mixed":         # (8, 4), N = 4, batch 1: infinite_stages (+-inf at some stages) with l1 and l2 on the states its boxes
        n, m, N = 8, 4, 4            # cut at, and a soft input whose bound cuts into the plan
        c = sr.build("infinite_stages")
        d = [v.copy() for v in c.inst[0]]
        _, u = sr._plan(sr._base(n, m, N, 1)[0], c.x0[0], N)
        d[8][1, 1] = u[1, 1] - 0.05
        soft = _weights(n, m, x1={0: 0.05, 1: 0.2, 3: 0.0, 4: 0.02}, x2={1: 0.5, 3: 2.0}, u1={1: 0.01})
        return _case([d], [soft], c.x0, N, True)
    if name == "soft_tracking":      # (12, 4), N = 7, batch 5: references of amplitude 3 under soft boxes of half-width 0.6 on states 0..2
        n, m, N = 12, 4, 7
        d, x0 = sr._base(n, m, N, 5, spread=0.3)
        d[5][1:, :3], d[6][1:, :3] = -0.6, 0.6
        rng = np.random.default_rng(21)
        k = np.arange(N + 1)
        xRef = 3.0 * np.sin(0.7 * k[None, :, None] + rng.uniform(0, 6, (5, 1, n)))
        uRef = np.zeros((5, N, m))
        return _case([d], [_weights(n, m, x1={0: 1.0, 1: 0.5, 2: 2.0}, x2={1: 1.0})], x0, N, True, xRef=xRef, uRef=uRef)
    if name == "soft_embedded":      # (3, 2) embedded in (4, 2), N = 3, batch 9: both_tracking with state 1 (a shrinking box) and input 0 soft
        c = sr.build("both_tracking")
        d = [v.copy() for v in c.inst[0]]
        return _case([d], [_weights(3, 2, x1={1: 0.5}, u1={0: 0.2}, u2={0: 0.3})], c.x0, c.N, True, xRef=c.xRef, uRef=c.uRef)
    if name == "soft_per_problem":   # (4, 1), N = 5, P = (5,): per_problem with its own weights per problem (mostly quadratic: the bound
                                     # of problem 0 cuts in by 0.05, which an l1 either ignores or enforces); problem 2 is all hard
        c = sr.build("per_problem")
        inst = [[v.copy() for v in d] for d in c.inst]
        soft = []
        for i in range(5):
            soft.append(_weights(4, 1) if i == 2 else
                        _weights(4, 1, x1={i % 4: 0.5 * (i % 2)}, x2={i % 4: 40.0 + 10.0 * i}, u1={0: 0.05} if i >= 3 else None))
        return _case(inst, soft, c.x0, c.N, False)
    raise KeyError(name)


CASES = ["soft_gate", "soft_x0_outside", "soft_terminal", "soft_quadratic", "soft_mixed", "soft_tracking", "soft_embedded",
         "soft_per_problem"]
ALL = CASES + ["soft_terminal_sequence", "soft_terminal_fixed"]
SCIPY_GPU = ["soft_terminal", "soft_quadratic"]


def scipy_instances(name):
    """the instances whose slack QP the tests solve: the first two -- of soft_quadratic the first alone (trust-constr needs a quarter of
    a minute per instance there: 14 inputs and 14 slacks under 40 rows)"""
    return (0,) if name == "soft_quadratic" else (0, 1)[:len(build(name).x0)]


def make_problem(mpcUtils, c, soft=None):
    """the ltvMpc object of a case (host side only); soft: other weights per problem than the case's"""
    return sr.make_problem(mpcUtils, c, soft=c.soft if soft is None else soft)


case_rho, reference_steps = sr.case_rho, sr.reference_steps     # (the case's own weights are their default)


@functools.lru_cache(maxsize=None)
def reference(name):
    return sr.reference_case(build(name))


@functools.lru_cache(maxsize=None)
def scipy_solution(name, b=0):
    """(x, u) of the slack QP of instance b"""
    return sr.scipy_case(build(name), b)


@functools.lru_cache(maxsize=None)
def variant_solution(name, variant, b=0):
    """the restatement's result for instance b with every component hard ("hard": its status may be "infeasible"), or with the bounds of
    the soft components removed ("free"): what a case's solution must differ from for its weights to matter"""
    return sr.variant_case(build(name), variant, b, max_iter=3000)


def run_steps(prob, c, ref):
    """tests/mpc_ltv_stage_ref.py: run_steps; a step whose options fix the penalty (n_levels = 1, the restatement's spelling) goes to
    `solve` as adaptive_rho=False"""
    def kw(step):
        k = dict(step["kw"])
        if k.pop("n_levels", None) == 1:
            k["adaptive_rho"] = False
        return k
    twin = SimpleNamespace(**{**c.__dict__, "steps": [dict(step, kw=kw(step)) for step in c.steps]})
    return sr.run_steps(prob, twin, ref)


compare = sr.compare
