#!/usr/bin/env python3
"""Secondary benchmark: ltvMpc (stage-varying dynamics, zm_mpc_setup_ltv_f64 / zm_mpc_solve_ltv_f64) on `batch` quadcopter instances,
N = 30, each linearised about ITS OWN trajectory, next to the yardstick it is built on: the per-problem tracking solve of lqrMpc
(zm_mpc_solve_tracking_f64) with `batch` distinct trim linearisations, in the same run.

Instance i hovers-to-be at yaw psi_i (every yaw is a trim); its start is the start of tools/bench_mpc.py about that trim.
    yardstick: lqrMpc in deviation coordinates with A_i, B_i the linearisation at trim i, tracking the zero reference (arrays, so that the
               tracking kernels run: the same per-problem, linear-term form the stage-varying kernel always takes)
    ltvMpc   : absolute coordinates; the nominal trajectory is the free response of instance i's linear model from its start (a
               non-equilibrium trajectory: the vehicle moves), expanded on the device by AffineDynamics.from_trajectory; the cost is about
               trim (xRef = trim state, uRef = uTrim); inputs within 3 of trim.
Reported per tolerance: the cold solve (median of --reps after a warm-up of the same shape, host clock around a device synchronise), the
time per ADMM iteration (solve time over the slowest instance's iteration count: a launch ends with its last instance) of both, and
their ratio; once: the expansion and the setup launch of the stage-varying problem (tables of batch x 7 levels) next to the setup launch
of the yardstick."""
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
    ap.add_argument("--eps", type=float, nargs="+", default=[1e-2, 1e-4])
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

    def timed(f, reps):
        ts = []
        for r in range(reps + 1):   # (the first call warms the shape up and is dropped)
            sync()
            t0 = time.perf_counter()
            out = f()
            sync()
            if r:
                ts.append((time.perf_counter() - t0) * 1e3)
        return out, float(np.median(ts)), float(np.min(ts)), float(np.max(ts))

    # the yardstick: one trim linearisation per instance
    lin = pytrees.AffineDynamics.from_function(model, trim, np.tile(uTrim, (Bn, 1)))
    A, B = np.asarray(lin.f_x), np.asarray(lin.f_u)
    lti = mpcUtils.lqrMpc(A, B, np.eye(12), np.eye(4), N, -x_ub, x_ub, -u_ub, u_ub)
    # the stage-varying problem: the free response of each instance's linear model, expanded about on the device
    xbar = np.zeros((Bn, N + 1, 12))
    xbar[:, 0] = dev0
    for k in range(N):
        xbar[:, k + 1] = np.einsum("bij,bj->bi", A, xbar[:, k])
    xbar += trim[:, None, :]
    traj = pytrees.Trajectory(torch.as_tensor(xbar, device="cuda"), torch.as_tensor(np.tile(uTrim, (Bn, N, 1)), device="cuda"))
    dyn, t_exp, _, _ = timed(lambda: pytrees.AffineDynamics.from_trajectory(model, traj), 5)
    ltv = mpcUtils.ltvMpc.fromExpansion(dyn, traj, np.eye(12), np.eye(4), -x_ub, x_ub, uTrim - u_ub, uTrim + u_ub)
    rho_v, rho_i = np.array(np.broadcast_to(ltv.rho, ltv.P)), np.array(np.broadcast_to(lti.rho, lti.P))

    def setup(prob, rho):
        prob._tables = {}
        return prob._device_problem_batched(rho, True)
    _, t_set_v, lo_v, hi_v = timed(lambda: setup(ltv, rho_v), 10)
    _, t_set_i, lo_i, hi_i = timed(lambda: setup(lti, rho_i), 10)
    print(json.dumps({"workload": f"quadcopter n=12 m=4 N={N}, {Bn} problems x 7 penalty levels", "expansion_ms": t_exp,
                      "setup_ltv_ms_median": t_set_v, "setup_ltv_ms_min": lo_v, "setup_ltv_ms_max": hi_v,
                      "setup_per_problem_ms_median": t_set_i, "setup_per_problem_ms_min": lo_i, "setup_per_problem_ms_max": hi_i}))

    x0_i = torch.as_tensor(dev0, device="cuda")
    x0_v = torch.as_tensor(dev0 + trim, device="cuda")
    ref_i = dict(xRef=torch.zeros((Bn, N + 1, 12), dtype=torch.float64, device="cuda"),
                 uRef=torch.zeros((Bn, N, 4), dtype=torch.float64, device="cuda"))
    ref_v = dict(xRef=torch.as_tensor(np.tile(trim[:, None, :], (1, N + 1, 1)), device="cuda"),
                 uRef=torch.as_tensor(np.tile(uTrim, (Bn, N, 1)), device="cuda"))
    legs = {"per-problem tracking (lqrMpc)": (lti, x0_i, ref_i), "stage-varying (ltvMpc)": (ltv, x0_v, ref_v)}
    for eps in args.eps:
        kw = dict(eps_abs=eps, eps_rel=eps, max_iter=args.max_iter, warm_start=False)
        times = {k: [] for k in legs}
        stats = {}
        for r in range(args.reps + 1):            # the two alternated; the first round warms the shapes up and is dropped
            for name, (prob, x0, ref) in legs.items():
                sync()
                t0 = time.perf_counter()
                _, _, status = prob.solve(x0, **ref, **kw)
                sync()
                if r:
                    times[name].append((time.perf_counter() - t0) * 1e3)
                stats[name] = (prob.last_iterations.copy(), float(np.mean(status == "optimal")))
        per_it = {}
        for name in legs:
            ts, (its, ok) = np.sort(times[name]), stats[name]
            med = float(np.median(ts))
            per_it[name] = med / max(int(its.max()), 1)
            print(json.dumps({"timed": name, "workload": f"quadcopter n=12 m=4 N={N}, {Bn} instances, eps={eps:g}", "reps": args.reps,
                              "solve_ms_median": med, "solve_ms_min": float(ts[0]), "solve_ms_max": float(ts[-1]),
                              "iters_mean": float(its.mean()), "iters_max": int(its.max()), "optimal_frac": ok,
                              "ms_per_admm_iteration": per_it[name]}))
        a, b = (per_it[k] for k in legs)
        print(json.dumps({"eps": eps, "ms_per_admm_iteration_ratio_ltv_over_per_problem_tracking": b / a}))


if __name__ == "__main__":
    main()
