"""The cases of the box DDP tests (tests/test_ddp_box.py on the CPU, tests/test_ddp_box_gpu.py on the device), computed once per
process: inputs, the long-double reference of tests/ddp_box_ref.py, the fp64 restatement's own error against it, the reruns with
perturbed projections, and the bounds that follow (`hp_reference.ddp_bounds`).  The CPU file asserts every case's strict-complementarity
margin and the stability of its clamped sets under the projection's resolution, so the GPU file may compare clamped sets exactly."""
import functools

import numpy as np

from oracle import zopt_oracle as zo
from tests import ddp_box_ref as dr
from tests import hp_reference as hp
from tests import ilqr_box_cases as ibc
from tests import ilqr_tracking_ref as tref
from tests import problems

MARGIN = ibc.MARGIN     # the smallest strict-complementarity margin a case may have
SET_REL = 2e-10         # perturbation of every projected matrix under which the clamped sets must not change: 10 x the projection's
                        # documented resolution (2e-11 of max|P|, ns16.h)
SENS_REL = 2e-11        # the perturbation whose effect on l, L enters the bounds (hp.ddp_reference_and_sensitivity's)
SENS_SEEDS = 3
# the smallest relative distance between the best two of the 16 line-search costs at which a solve case may compare winning indices:
# 10 x the 1e-9 to which the accepted costs are compared, so two candidates that agree with the restatement to that cannot swap
COST_GAP = 1e-8

# (n, m, T, batch, a box per trajectory): every KS of the kernel, a ragged shape, T = 1, both bound layouts
SWEEP_SHAPES = ((3, 2, 1, 3, False), (3, 2, 5, 5, True), (5, 3, 4, 3, True), (8, 4, 5, 3, False), (12, 4, 3, 5, True), (12, 4, 6, 3, False))
SWEEP_FAMILIES = ("plain", "strongly_indefinite", "control_affine_8", "packed_pairs", "onbound")


def family_shapes(family):
    return tuple(s for s in SWEEP_SHAPES if family != "packed_pairs" or s[:2] == (12, 4))


def _sweep_inputs(family, n, m, T, batch, per_traj):
    """problems.hard_ddp's model of the family (`onbound`: of `plain`) with the box and the inputs of ilqr_box_cases._sweep_inputs at
    tight = 1 (half-widths uniform in 0.3 .. 0.8, the last upper bound +inf, u = clip(0.3 randn); `onbound`: u_k on a bound)"""
    dyn, cost, Vf, _ = problems.hard_ddp("plain" if family == "onbound" else family, n, m, T, batch)
    u, lb, ub = ibc._sweep_inputs("onbound" if family == "onbound" else "plain", n, m, T, batch, per_traj, seed=17 * n + T + batch)[3:]
    return dyn, cost, Vf, u, lb, ub


@functools.lru_cache(maxsize=None)
def sweep_case(family, n, m, T, batch, per_traj):
    """dict(args = (dyn, cost, Vf, uTraj, lb, ub), ref = the long-double box DDP sweep (l, L, clamped, margin), e_l, e_L = the fp64
    restatement's error (hp.sweep_metric, maximum), same64 = its clamped sets equal the reference's, stable = so do those of the
    rerun perturbed by SET_REL, s_l, s_L = the largest change of l, L over SENS_SEEDS reruns perturbed by SENS_REL)"""
    args = _sweep_inputs(family, n, m, T, batch, per_traj)
    ref, reruns = dr.ddp_box_backward_with_reruns(*args, rels=[SET_REL] + [SENS_REL] * SENS_SEEDS)
    o = dr.ddp_box_backward(*args)
    s_l, s_L = (max(float(hp.sweep_metric(r[name], ref[name]).max()) for r in reruns[1:]) for name in ("l", "L"))
    return {"args": args, "ref": ref, "e_l": float(hp.sweep_metric(o["l"], ref["l"]).max()),
            "e_L": float(hp.sweep_metric(o["L"], ref["L"]).max()), "same64": bool(np.array_equal(o["clamped"], ref["clamped"])),
            "stable": all(bool(np.array_equal(r["clamped"], ref["clamped"])) for r in reruns), "s_l": s_l, "s_L": s_L, "o64": o}


def sweep_bounds(family, n, m, T, batch, per_traj):
    """(bound on l, bound on L): hp.ddp_bounds from the restatement's error on the case and on the plain family at the same shape and
    the case's sensitivity to the projection's resolution"""
    c, p = sweep_case(family, n, m, T, batch, per_traj), sweep_case("plain", n, m, T, batch, per_traj)
    return hp.ddp_bounds(c["e_l"], p["e_l"], c["s_l"]), hp.ddp_bounds(c["e_L"], p["e_L"], c["s_L"])


@functools.lru_cache(maxsize=None)
def unbounded_case(family, n, m, T, batch):
    """the family without a box: hp.ddp_backward_hp's reference with its sensitivity, the oracle's error against it and the bounds
    the unboxed kernel is held to (tests/hard_cases.py's rule)"""
    dyn, cost, Vf, _ = problems.hard_ddp(family, n, m, T, batch)
    ref, (s_l, s_L) = hp.ddp_reference_and_sensitivity(dyn, cost, Vf)
    o = zo.backwardPass_ddp(zo.QuadraticDynamics(*dyn), zo.QuadraticCostFunction(*cost), zo.QuadraticValueFunction(*Vf))
    e_l, e_L = float(hp.sweep_metric(o.l, ref["l"]).max()), float(hp.sweep_metric(o.L, ref["L"]).max())
    return {"args": (dyn, cost, Vf), "ref": ref, "o64": o, "e_l": e_l, "e_L": e_L, "s_l": s_l, "s_L": s_L}


def unbounded_bounds(family, n, m, T, batch):
    c, p = unbounded_case(family, n, m, T, batch), unbounded_case("plain", n, m, T, batch)
    return hp.ddp_bounds(c["e_l"], p["e_l"], c["s_l"]), hp.ddp_bounds(c["e_L"], p["e_L"], c["s_L"])


def pair_rows(f_xx):
    """H[b, t, p, i] = f_xx[b, t, i, a_p, b_p] over the quadcopter's declared pairs: what the pairs entries take"""
    return np.ascontiguousarray(np.stack([f_xx[:, :, :, a, b] for a, b in problems.QUAD_HESSIAN_PAIRS], axis=2))


# ------------------------------------------------------------------------------------------------------------------------ solves
# rb: the rigid-body model (n = 8, no declared Hessian pairs: the full-tensor branch of the solve).  Its DDP policy saturates every input
# of a trajectory, so several of the 16 clipped rollouts coincide and their costs tie exactly in some line searches: the winning index
# is compared only in the iterations whose two best costs are COST_GAP apart (`index_comparable`); a tie leaves the accepted cost,
# which every iteration compares, the same whichever index wins.
SOLVE_CASES = ("quad_hover", "quad_origin", "rb")


def solve_case(name):
    """ilqr_box_cases.solve_case's dict plus `torch` = the model's step in torch.  quad_hover: its TrackingCost case; quad_origin: the
    same model, start states and bounds with a QuadraticCost about the origin; rb: its rigid-body case (QuadraticCost)."""
    c = dict(ibc.solve_case("rb" if name == "rb" else "quad_hover"))
    if name == "quad_origin":
        c.update(xRef=None, uRef=None)
    c["torch"] = dr.rigid_body_step_torch(c["model"][1]) if name == "rb" else zo.quad_euler_step_torch(c["model"][1])
    return c


def index_comparable(Js):
    return cost_gap(Js) >= COST_GAP


@functools.lru_cache(maxsize=None)
def solve_reference(name):
    """the restatement's solve of every trajectory of the case: list of dict(traj, L, J, converged, its, trace)"""
    import warnings
    c = solve_case(name)
    B, T, m = c["ug"].shape
    n = c["x0"].shape[-1]
    out = []
    for b in range(B):
        xr, ur = tref.full_reference(c["xRef"], c["uRef"], T, n, m, b)
        tr = []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            traj, L, J, conv, its = dr.differentialDynamicProgramming_box(c["step"], c["torch"], c["Q"], c["R"], c["Qf"], c["x0"][b], c["ug"][b],
                                                                          c["lb"], c["ub"], xr, ur, return_iters=True, trace=tr, **c["kw"])
        out.append(dict(traj=traj, L=L, J=J, converged=conv, its=its, trace=tr))
    return out


def cost_gap(Js):
    """relative distance between the best two of the line search's finite costs"""
    s = np.sort(np.asarray(Js)[np.isfinite(Js)])
    return float((s[1] - s[0]) / abs(s[0])) if s.size > 1 else float("inf")
