#!/usr/bin/env python3
"""Secondary benchmark: what the proximal map of soft box constraints costs next to the clip.  tools/bench_mpc_ltv_stage.py's problem
(`batch` quadcopter instances, N = 30, each linearised about its own trajectory) solved by
    stage : ltvMpc with stage_varying= all six, constant rows          (zm_mpc_solve_ltv_stage_f64)
    hard  : the same data with every soft weight l1 = +inf              (zm_mpc_solve_ltv_soft_f64: the same iterations, bit for bit)
    soft  : l1 = 1 on the eight bounded states                          (zm_mpc_solve_ltv_soft_f64: its own iterations)
alternated in one process; all three share zm_mpc_setup_ltv_stage_f64, which is not timed.  `stage` and `hard` run the same iterations
(checked: the iteration counts and u are equal), so their times compare kernel against kernel; `soft` solves another problem and is
reported per iteration of its own count.  Medians with min / max over --reps: the time per ADMM iteration at eps 1e-4 and per cold solve at
eps 1e-2 (host clock around a device synchronise, the solve time over the slowest instance's iteration count: a launch ends with its last
instance)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--N", type=int, default=30)
    ap.add_argument("--max-iter", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch
    from zopt_amd import models, mpcUtils, pytrees
    Bn, N, dt = args.batch, args.N, 0.1
    model = models.QuadcopterEuler(dt)
    uTrim = np.asarray(models.QuadcopterEuler.uTrim, dtype=np.float64)
    rng = np.random.default_rng(1)
    x_ub = np.array([1, 1, 1, 0.3, 0.3, 0.1, 0.5, 0.5, np.inf, np.inf, np.inf, np.inf])
    u_ub = np.array([3.0, 3, 3, 3])
    dev0 = np.clip(0.03 * rng.standard_normal((Bn, 12)), -x_ub + 1e-6, x_ub - 1e-6)
    dev0[:, 9:12] = rng.uniform(-10, 10, (Bn, 3))
    dev0[:, 8] = 0.0
    trim = np.zeros((Bn, 12))
    trim[:, 8] = rng.uniform(-np.pi, np.pi, Bn)
    sync = torch.cuda.synchronize

    lin = pytrees.AffineDynamics.from_function(model, trim, np.tile(uTrim, (Bn, 1)))
    A = np.asarray(lin.f_x)
    xbar = np.zeros((Bn, N + 1, 12))
    xbar[:, 0] = dev0
    for k in range(N):
        xbar[:, k + 1] = np.einsum("bij,bj->bi", A, xbar[:, k])
    xbar += trim[:, None, :]
    traj = pytrees.Trajectory(torch.as_tensor(xbar, device="cuda"), torch.as_tensor(np.tile(uTrim, (Bn, N, 1)), device="cuda"))
    dyn = pytrees.AffineDynamics.from_trajectory(model, traj)
    rows = lambda v, r: np.broadcast_to(v, (r,) + np.shape(v)).copy()
    six = (rows(np.eye(12), N + 1), rows(np.eye(4), N), rows(-x_ub, N + 1), rows(x_ub, N + 1), rows(uTrim - u_ub, N), rows(uTrim + u_ub, N))
    build = lambda **soft: mpcUtils.ltvMpc.fromExpansion(dyn, traj, *six, stage_varying=("Q", "R", "x_lb", "x_ub", "u_lb", "u_ub"), **soft)
    stage, hard = build(), build(x_soft_l1=np.full(12, np.inf))
    soft = build(x_soft_l1=np.where(np.isfinite(x_ub), 1.0, np.inf))
    legs = {"stage (zm_mpc_solve_ltv_stage_f64)": stage, "hard (zm_mpc_solve_ltv_soft_f64, l1 = inf)": hard,
            "soft (zm_mpc_solve_ltv_soft_f64, l1 = 1 on 8 states)": soft}
    k_stage, k_hard, k_soft = legs

    def alternated(f, reps):
        """{leg: sorted times in ms} of f(prob), the legs alternated; the first round warms the shapes up and is dropped"""
        times = {k: [] for k in legs}
        for r in range(reps + 1):
            for name, prob in legs.items():
                sync()
                t0 = time.perf_counter()
                f(prob)
                sync()
                if r:
                    times[name].append((time.perf_counter() - t0) * 1e3)
        return {k: np.sort(v) for k, v in times.items()}

    x0 = torch.as_tensor(dev0 + trim, device="cuda")
    ref = dict(xRef=torch.as_tensor(np.tile(trim[:, None, :], (1, N + 1, 1)), device="cuda"),
               uRef=torch.as_tensor(np.tile(uTrim, (Bn, N, 1)), device="cuda"))
    for eps, what in ((1e-4, "ms_per_admm_iteration"), (1e-2, "solve_ms")):
        kw = dict(eps_abs=eps, eps_rel=eps, max_iter=args.max_iter, warm_start=False)
        seen = {}

        def solve(prob):
            u, _, status = prob.solve(x0, **ref, **kw)
            seen[id(prob)] = (prob.last_iterations.copy(), float(np.mean(status == "optimal")), u)
        ts = alternated(solve, args.reps)
        assert np.array_equal(seen[id(stage)][0], seen[id(hard)][0]) and torch.equal(seen[id(stage)][2], seen[id(hard)][2]), \
            "all-hard weights must run the stage solve's iterations"
        med = {}
        for name, prob in legs.items():
            its, ok, _ = seen[id(prob)]
            per = 1.0 / max(int(its.max()), 1) if what == "ms_per_admm_iteration" else 1.0
            med[name] = float(np.median(ts[name])) * per
            print(json.dumps({"timed": name, "workload": f"quadcopter n=12 m=4 N={N}, {Bn} instances, eps={eps:g}, cold", "reps": args.reps,
                              "iters_mean": float(its.mean()), "iters_max": int(its.max()), "optimal_frac": ok,
                              what + "_median": med[name], what + "_min": float(ts[name][0]) * per, what + "_max": float(ts[name][-1]) * per}))
        print(json.dumps({"eps": eps, what + "_ratio_hard_over_stage": med[k_hard] / med[k_stage],
                          what + "_ratio_soft_over_stage": med[k_soft] / med[k_stage]}))


if __name__ == "__main__":
    main()
