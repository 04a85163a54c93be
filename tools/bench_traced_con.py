#!/usr/bin/env python3
"""What recorded constraints cost and what they buy (models.TracedConstraint, zopt_amd/csrc/traced_con.hip).  The variants of a
comparison are alternated in one process so that clock and thermal drift hit them alike; medians with min / max over the repetitions,
one JSON line per measurement (also appended to --out).  The helpers are tools/bench_traced_model.py's.

  (a) the price of interpretation: 8192 quadcopters, T = 100, a TrackingCost about hover with a goal per vehicle, a floor per vehicle
      and a 3 m/s cap on the body velocities (the problem (d) of tools/bench_ilqr_state.py) as a StateBox and as the same 7 rows written
      as g(x, u, p) (stage rows and terminal rows; every start is strictly inside, so the row sets coincide), at the same `outer`;
      the outer and inner iteration counts of the two are compared;
  (b) what hardness costs: the same fleet with a sphere per vehicle between start and goal, as a TracedConstraint (hard: done means
      outside to ctol) and as the soft keep-out penalty w / (d^2 + eps) of tools/bench_traced_cost.py written into a TracedCost;
  (c) the untouched solves -- plain, input box, state box -- through this tree's library and through the parent commit's, loaded
      next to it (the library ZOPT_AMD_PARENT_LIB names; left out without it), parent / own / parent.

    python tools/bench_traced_con.py [--out profiles/traced_con_bench.txt]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_traced_con.py --only a --reps 1 --con-only     # per-kernel totals
"""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_traced_model as M          # noqa: E402

emit, stats, alternate = M.emit, M.stats, M.alternate
VCAP = 3.0


def box_rows(x, u, p):
    """p = [floor]: z (state 11, pointing down) at most the floor, |body velocities| at most 3 m/s"""
    return np.array([x[11] - p[0], x[0] - VCAP, -VCAP - x[0], x[1] - VCAP, -VCAP - x[1], x[2] - VCAP, -VCAP - x[2]])


def sphere_row(x, u, p):
    """p = [centre (3), radius]"""
    d0, d1, d2 = x[9] - p[0], x[10] - p[1], x[11] - p[2]
    return np.array([p[3] * p[3] - (d0 * d0 + d1 * d1 + d2 * d2)])


def soft_running(x, u, p):
    """p = [goal (3), obstacle (3)]: the TrackingCost's terms about the goal and hover, plus the smooth keep-out penalty"""
    c = sum(x[i] * x[i] for i in range(9)) + sum((x[9 + i] - p[i]) * (x[9 + i] - p[i]) for i in range(3))
    c = c + (u[0] - 9.807) * (u[0] - 9.807) + u[1] * u[1] + u[2] * u[2] + u[3] * u[3]
    d0, d1, d2 = x[9] - p[3], x[10] - p[4], x[11] - p[5]
    return c + 4.0 / (d0 * d0 + d1 * d1 + d2 * d2 + 0.5)


def soft_terminal(x, p):
    return 10.0 * (sum(x[i] * x[i] for i in range(9)) + sum((x[9 + i] - p[i]) * (x[9 + i] - p[i]) for i in range(3)))


def fleet(B, T, torch, models):
    rng = np.random.default_rng(2)
    dev = dict(dtype=torch.float64, device="cuda")
    x0 = np.zeros((B, 12))
    x0[:, 9:12] = rng.uniform(-10, 10, (B, 3))
    goal = np.zeros((B, 12))
    goal[:, 9:12] = rng.uniform(-10, 10, (B, 3))
    uTrim = np.asarray(models.QuadcopterEuler.uTrim, dtype=np.float64)
    tg = torch.as_tensor(goal, **dev)
    cost = models.TrackingCost(np.eye(12), np.eye(4), 10 * np.eye(12), tg[:, None, :], uTrim)
    return x0, goal, torch.as_tensor(x0, **dev), torch.as_tensor(np.tile(uTrim, (B, T, 1)), **dev), cost


def counts(info, conv, torch):
    fin = torch.isfinite(info.violation)
    return dict(converged_frac=float(conv.double().mean().item()), outer_iterations_mean=float(info.outerIterations.double().mean().item()),
                inner_iterations_total_mean=float(info.innerIterations.sum(-1).double().mean().item()),
                largest_violation_where_done=float(info.violation[conv].max().item()) if bool(conv.any()) else None,
                largest_violation_finite=float(info.violation[fin].max().item()))


def part_a(args, torch, ilqr, models):
    B, T = args.batch, args.T
    x0, goal, tx0, tug, cost = fleet(B, T, torch, models)
    model = models.QuadcopterEuler(0.1)
    floor = np.maximum(x0[:, 11], goal[:, 11]) + 0.2
    inf = np.full(12, np.inf)
    x_lb, x_ub = np.tile(-inf, (B, 1)), np.tile(inf, (B, 1))
    x_ub[:, 11] = floor
    x_lb[:, 0:3], x_ub[:, 0:3] = -VCAP, VCAP
    kw = dict(outer=args.outer)
    sb = models.StateBox(model, x_lb, x_ub, **kw)
    tc = models.TracedConstraint(model, box_rows, 7, lambda x, p: box_rows(x, None, p), 7, params=floor[:, None], **kw)
    t = tc.stage_tape
    emit(part="a", what="stage tape of the box written as g", instructions=len(t.code), constants=len(t.consts), slots=t.n_slots, rows=len(t.outputs))
    variants = {"TracedConstraint, box written as g": lambda: ilqr.constrainedIterativeLqr(tc, cost, cost, tx0, tug)}
    if not args.con_only:
        variants = {"StateBox": lambda: ilqr.constrainedIterativeLqr(sb, cost, cost, tx0, tug), **variants}
    times, res = alternate(variants, args.reps, torch.cuda.synchronize)
    for k in times:
        emit(part="a", workload=f"constrainedIterativeLqr quadcopter n=12 m=4 T={T} batch={B} fp64, floor per vehicle, |uvw| <= 3, outer={args.outer}",
             variant=k, **counts(res[k][4], res[k][3], torch), **stats(times[k]))
    if not args.con_only:
        a, b = res["StateBox"], res["TracedConstraint, box written as g"]
        fin = torch.isfinite(a[2]) & torch.isfinite(b[2])
        emit(part="a", traced_over_statebox=float(np.median(times["TracedConstraint, box written as g"]) / np.median(times["StateBox"])),
             same_outer_counts_frac=float((a[4].outerIterations == b[4].outerIterations).double().mean().item()),
             same_inner_counts_frac=float((a[4].innerIterations == b[4].innerIterations).all(-1).double().mean().item()),
             same_done_frac=float((a[3] == b[3]).double().mean().item()),
             median_rel_J_difference=float(((a[2][fin] - b[2][fin]).abs() / a[2][fin].abs()).median().item()))


def part_b(args, torch, ilqr, models):
    B, T = args.batch, args.T
    x0, goal, tx0, tug, cost = fleet(B, T, torch, models)
    rng = np.random.default_rng(6)
    model = models.QuadcopterEuler(0.1)
    centre = 0.5 * (x0[:, 9:12] + goal[:, 9:12]) + rng.uniform(-0.3, 0.3, (B, 3))
    radius = rng.uniform(0.5, 1.0, (B, 1))
    hard = models.TracedConstraint(model, sphere_row, 1, params=np.concatenate([centre, radius], 1), outer=args.outer)
    soft = models.TracedCost(soft_running, soft_terminal, 12, 4, params=np.concatenate([goal[:, 9:12], centre], 1))
    variants = {"TracedConstraint, sphere per vehicle (hard)": lambda: ilqr.constrainedIterativeLqr(hard, cost, cost, tx0, tug),
                "TracedCost, keep-out penalty 4 / (d^2 + 0.5) (soft)": lambda: ilqr.iterativeLqr(model, soft, soft, tx0, tug)}
    times, res = alternate(variants, args.reps, torch.cuda.synchronize)
    for k in times:
        traj, conv = res[k][0], res[k][3]
        d = (traj.xTraj[:, :, 9:12] - torch.as_tensor(centre, dtype=torch.float64, device="cuda")[:, None, :]).norm(dim=-1).min(dim=1).values
        clear = d - torch.as_tensor(radius[:, 0], dtype=torch.float64, device="cuda")
        fin = torch.isfinite(clear)
        row = dict(part="b", workload=f"iLQR quadcopter n=12 m=4 T={T} batch={B} fp64, goal and sphere per vehicle", variant=k,
                   converged_frac=float(conv.double().mean().item()), inside_the_sphere_frac=float((clear[fin] < 0).double().mean().item()),
                   inside_the_sphere_frac_where_converged=float((clear[fin & conv] < 0).double().mean().item()) if bool((fin & conv).any()) else None,
                   deepest_penetration_where_converged_m=float((-clear[fin & conv]).clamp(min=0).max().item()) if bool((fin & conv).any()) else None,
                   **stats(times[k]))
        if len(res[k]) == 5:
            row.update(counts(res[k][4], conv, torch))
        emit(**row)
    ks = list(variants)
    emit(part="b", hard_over_soft=float(np.median(times[ks[0]]) / np.median(times[ks[1]])))


def _load(path, _lib):
    """a library with the signatures of the entries it has (the parent commit's lacks the new ones)"""
    handle = ctypes.CDLL(path)
    for name, (res, argt) in _lib.SYMBOLS.items():
        fn = getattr(handle, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, argt
    return handle


def part_c(args, torch, ilqr, models, _lib):
    path = os.environ.get("ZOPT_AMD_PARENT_LIB")
    if not path or not os.path.exists(path):
        emit(part="c", skipped="ZOPT_AMD_PARENT_LIB names no library")
        return
    own, parent = _lib.lib(), _load(path, _lib)
    B, T = args.batch, args.T
    x0, goal, tx0, tug, cost = fleet(B, T, torch, models)
    model = models.QuadcopterEuler(0.1)
    uTrim = np.asarray(models.QuadcopterEuler.uTrim, dtype=np.float64)
    lim = np.array([2.0, 0.05, 0.05, 0.05])
    inf = np.full(12, np.inf)
    subjects = {"plain": (ilqr.iterativeLqr, model), "input box": (ilqr.iterativeLqr, models.InputBox(model, uTrim - lim, uTrim + lim)),
                "state box, infinite bounds, outer = 1": (ilqr.iterativeLqr, models.StateBox(model, -inf, inf, outer=1))}

    def run(handle, fn, dyn):
        _lib._lib = handle                                      # every call of the drivers goes through _lib.lib()
        try:
            return fn(dyn, cost, cost, tx0, tug)
        finally:
            _lib._lib = own
    bits = lambda t: t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t      # noqa: E731  (NaN rows compare as bits)
    for name, (fn, dyn) in subjects.items():
        variants = {"parent a": lambda: run(parent, fn, dyn), "own": lambda: run(own, fn, dyn), "parent b": lambda: run(parent, fn, dyn)}
        times, res = alternate(variants, args.reps_c, torch.cuda.synchronize)
        med = {k: float(np.median(v)) for k, v in times.items()}
        pm = 0.5 * (med["parent a"] + med["parent b"])
        same = all(torch.equal(bits(a), bits(b)) for a, b in ((res["own"][0].xTraj, res["parent a"][0].xTraj), (res["own"][0].uTraj, res["parent a"][0].uTraj),
                                                             (res["own"][1], res["parent a"][1]), (res["own"][2], res["parent a"][2])))
        emit(part="c", workload=f"iterativeLqr quadcopter n=12 m=4 T={T} batch={B} fp64, TrackingCost about hover: {name}", reps=args.reps_c,
             own_ms_median=med["own"], parent_a_ms_median=med["parent a"], parent_b_ms_median=med["parent b"],
             parent_spread_ms=abs(med["parent a"] - med["parent b"]), own_over_parent_median=med["own"] / pm, own_bits_equal_parent=bool(same))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--reps-c", type=int, default=7)
    ap.add_argument("--outer", type=int, default=3, help="outer iterations of every augmented-Lagrangian variant")
    ap.add_argument("--only", default="abc")
    ap.add_argument("--con-only", action="store_true", help="(a) without the StateBox variant (for a kernel trace)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    M.OUT = args.out
    import torch
    from zopt_amd import _lib, ilqrUtils, models
    if args.out and os.path.exists(args.out):
        os.remove(args.out)
    emit(tool="tools/bench_traced_con.py", device=torch.cuda.get_device_name(0), args={k: v for k, v in vars(args).items() if k != "out"})
    if "a" in args.only:
        part_a(args, torch, ilqrUtils, models)
    if "b" in args.only:
        part_b(args, torch, ilqrUtils, models)
    if "c" in args.only:
        part_c(args, torch, ilqrUtils, models, _lib)


if __name__ == "__main__":
    main()
