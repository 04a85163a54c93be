"""The cases of the hard-family sweep tests (tests/test_sweeps_hard_gpu.py and the CPU property tests of tests/test_hp_reference.py),
computed once per process: inputs from tests/problems.py, the long-double reference of tests/hp_reference.py, the fp64 oracle's own
error against it (`hp_reference.sweep_metric`, maximum over trajectories and steps; L of `badly_scaled` measured as L D so that every
column counts), and the bounds that follow from those errors."""
import functools

import numpy as np

from oracle import zopt_oracle as zo
from tests import problems
from tests.hp_reference import (affine_lqr_ld, ddp_bounds, ddp_reference_and_sensitivity, ilqr_backward_ld, sweep_bounds, sweep_metric)


def _scaled(name, n, L):
    return L * problems.sweep_scaling(n) if name == "badly_scaled" else L


def policy_errors(name, n, out_l, out_L, ref):
    """(error of l, error of L) of a policy against the case's reference, each (batch, T), in the tests' metric."""
    return sweep_metric(out_l, ref["l"]), sweep_metric(_scaled(name, n, np.asarray(out_L)), _scaled(name, n, ref["L"]))


@functools.lru_cache(maxsize=None)
def ilqr_case(name, n, m, T, shared=False, batch=2):
    dyn, cost, Vf = problems.hard_sweep(name, n, m, T, batch, shared)
    ref = ilqr_backward_ld(dyn, cost, Vf)
    o = zo.backwardPass_ilqr(zo.AffineDynamics(*dyn), zo.QuadraticCostFunction(*cost), zo.QuadraticValueFunction(*Vf))
    el, eL = policy_errors(name, n, o.l, o.L, ref)
    return {"args": (dyn, cost, Vf), "ref": ref, "e_l": float(el.max()), "e_L": float(eL.max())}


@functools.lru_cache(maxsize=None)
def affine_case(name, n, m, T, batch=2):
    args = problems.hard_affine(name, n, m, T, batch)
    ref = affine_lqr_ld(*args[:8], T)
    L, l = zo.bilinearAffineLqr(*args, T)
    el, eL = policy_errors(name, n, l, L, ref)
    return {"args": args, "ref": ref, "e_l": float(el.max()), "e_L": float(eL.max())}


@functools.lru_cache(maxsize=None)
def ddp_case(name, n, m, T, batch=2):
    dyn, cost, Vf, planted = problems.hard_ddp(name, n, m, T, batch)
    ref, (s_l, s_L) = ddp_reference_and_sensitivity(dyn, cost, Vf)
    o = zo.backwardPass_ddp(zo.QuadraticDynamics(*dyn), zo.QuadraticCostFunction(*cost), zo.QuadraticValueFunction(*Vf))
    el, eL = policy_errors(name, n, o.l, o.L, ref)
    return {"args": (dyn, cost, Vf), "ref": ref, "planted": planted, "e_l": float(el.max()), "e_L": float(eL.max()), "s_l": s_l, "s_L": s_L}


def case_bounds(case_fn, name, n, m, T, **kw):
    """(bound on l, bound on L) of a hard-family case: `sweep_bounds` from the oracle's error on the case and on the plain family at
    the same shape and horizon; for `ddp_case` widened to `ddp_bounds` by the case's sensitivity to the projection's resolution."""
    c, p = case_fn(name, n, m, T, **kw), case_fn("plain", n, m, T, **kw)
    if case_fn is ddp_case:
        return ddp_bounds(c["e_l"], p["e_l"], c["s_l"]), ddp_bounds(c["e_L"], p["e_L"], c["s_L"])
    return sweep_bounds(c["e_l"], p["e_l"]), sweep_bounds(c["e_L"], p["e_L"])
