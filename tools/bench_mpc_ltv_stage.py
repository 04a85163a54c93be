#!/usr/bin/env python3
"""Secondary benchmark: what the stage's box in the forward prefetch set and the stage's weights in the setup cost.  tools/bench_mpc_ltv.py's
stage-varying problem (`batch` quadcopter instances, N = 30, each linearised about its own trajectory) solved by
    plain : ltvMpc, one set of weights and bounds per problem          (zm_mpc_setup_ltv_f64,       zm_mpc_solve_ltv_f64)
    stage : the same data as constant rows with stage_varying= all six  (zm_mpc_setup_ltv_stage_f64, zm_mpc_solve_ltv_stage_f64)
alternated in one process.  Constant rows compile the same sums, so both legs run the same iterations (checked: the iteration counts and
u are equal) and the times compare kernel against kernel.  Reported as medians with min / max over --reps: the time per ADMM iteration at
eps 1e-4 and per cold solve at eps 1e-2 (host clock around a device synchronise, the solve time over the slowest instance's iteration
count: a launch ends with its last instance), and the two setup launches (tables of batch x 7 levels)."""
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
    plain = mpcUtils.ltvMpc.fromExpansion(dyn, traj, np.eye(12), np.eye(4), -x_ub, x_ub, uTrim - u_ub, uTrim + u_ub)
    stage = mpcUtils.ltvMpc.fromExpansion(dyn, traj, rows(np.eye(12), N + 1), rows(np.eye(4), N), rows(-x_ub, N + 1), rows(x_ub, N + 1),
                                          rows(uTrim - u_ub, N), rows(uTrim + u_ub, N),
                                          stage_varying=("Q", "R", "x_lb", "x_ub", "u_lb", "u_ub"))
    rho = np.array(np.broadcast_to(plain.rho, plain.P))
    assert np.array_equal(rho, np.broadcast_to(stage.rho, stage.P))
    legs = {"plain (zm_mpc_*_ltv_f64)": plain, "stage (zm_mpc_*_ltv_stage_f64)": stage}

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

    def setup(prob):
        prob._tables = {}
        prob._device_problem_batched(rho, True)
    ts = alternated(setup, args.reps)
    for name in legs:
        print(json.dumps({"timed": "setup, " + name, "workload": f"quadcopter n=12 m=4 N={N}, {Bn} problems x 7 penalty levels",
                          "reps": args.reps, "setup_ms_median": float(np.median(ts[name])), "setup_ms_min": float(ts[name][0]),
                          "setup_ms_max": float(ts[name][-1])}))
    a, b = (float(np.median(ts[k])) for k in legs)
    print(json.dumps({"setup_ms_ratio_stage_over_plain": b / a}))

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
        (its, ok, u), (its_s, _, u_s) = seen[id(plain)], seen[id(stage)]
        assert np.array_equal(its, its_s) and torch.equal(u, u_s), "constant rows must run the plain solve's iterations"
        per = 1.0 / max(int(its.max()), 1) if what == "ms_per_admm_iteration" else 1.0
        for name in legs:
            print(json.dumps({"timed": name, "workload": f"quadcopter n=12 m=4 N={N}, {Bn} instances, eps={eps:g}, cold", "reps": args.reps,
                              "iters_mean": float(its.mean()), "iters_max": int(its.max()), "optimal_frac": ok,
                              what + "_median": float(np.median(ts[name])) * per, what + "_min": float(ts[name][0]) * per,
                              what + "_max": float(ts[name][-1]) * per}))
        a, b = (float(np.median(ts[k])) for k in legs)
        print(json.dumps({"eps": eps, what + "_ratio_stage_over_plain": b / a}))


if __name__ == "__main__":
    main()
