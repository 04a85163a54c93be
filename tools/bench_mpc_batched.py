#!/usr/bin/env python3
"""Secondary benchmark: lqrMpc with per-problem data.  A family of P distinct QuadcopterEuler(0.1) linearisations (attitudes and
velocities spread around hover; the demo's Q = R = I and bounds, N = 30), one initial state per problem (x0[9:12] ~ U(-10, 10)^3 and
small velocities / angles, as tools/bench_mpc.py), solved

  * batched: one setup launch (P problems x 7 penalty levels) + one solve launch, at P in --sizes;
  * shared:  the same x0 on ONE problem (hover), today's path -- the yardstick a batched solve is held to;
  * loop:    P = --loop-problems single-problem objects, each built, set up and solved on its own (what the feature replaces).

Prints one JSON line per measurement: wall times (setup = device upload + table launch, solve = the solve call incl. its result
copies), ADMM iterations and the status mix."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

X_UB = np.array([1, 1, 1, 0.3, 0.3, 0.1, 0.5, 0.5, np.inf, np.inf, np.inf, np.inf])
U_UB = np.array([3.0, 3, 3, 3])


def family(P, seed=0):
    from zopt_amd import models, pytrees
    rng = np.random.default_rng(seed)
    X = np.zeros((P, 12))
    X[:, 3:6] = rng.uniform(-0.15, 0.15, (P, 3))
    X[:, 6:12] = rng.uniform(-0.5, 0.5, (P, 6))
    U = np.broadcast_to(models.QuadcopterEuler.uTrim, (P, 4)).copy()
    lin = pytrees.AffineDynamics.from_function(models.QuadcopterEuler(0.1), X, U)
    x0 = np.clip(0.03 * rng.standard_normal((P, 12)), -X_UB + 1e-6, X_UB - 1e-6)
    x0[:, 9:12] = rng.uniform(-10, 10, (P, 3))
    return np.asarray(lin.f_x), np.asarray(lin.f_u), x0


def mix(status):
    v, c = np.unique(np.asarray(status).astype(str), return_counts=True)
    return {str(a): int(b) for a, b in zip(v, c)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1, 1024, 8192])
    ap.add_argument("--N", type=int, default=30)
    ap.add_argument("--eps", type=float, nargs="+", default=[1e-2, 1e-4])
    ap.add_argument("--max-iter", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loop-problems", type=int, default=32)
    args = ap.parse_args()
    import torch
    from zopt_amd import models, mpcUtils, pytrees
    sync = torch.cuda.synchronize
    Q, R = np.eye(12), np.eye(4)
    hover = pytrees.AffineDynamics.from_function(models.QuadcopterEuler(0.1), np.zeros(12), models.QuadcopterEuler.uTrim)
    shared = mpcUtils.lqrMpc(np.asarray(hover.f_x), np.asarray(hover.f_u), Q, R, args.N, -X_UB, X_UB, -U_UB, U_UB)
    # warm-up: library, kernels, allocator
    A, B, x0 = family(8, seed=99)
    mpcUtils.lqrMpc(A, B, Q, R, args.N, -X_UB, X_UB, -U_UB, U_UB).solve(x0, eps_abs=1e-2, eps_rel=1e-2)
    shared.solve(x0, eps_abs=1e-2, eps_rel=1e-2)
    sync()
    for P in args.sizes:
        A, B, x0 = family(P, seed=P)
        tx0 = torch.as_tensor(x0, device="cuda")
        t0 = time.perf_counter()
        prob = mpcUtils.lqrMpc(A, B, Q, R, args.N, -X_UB, X_UB, -U_UB, U_UB)
        t1 = time.perf_counter()
        prob._device_problem_batched(prob.rho, True)
        sync()
        t2 = time.perf_counter()
        for eps in args.eps:
            kw = dict(eps_abs=eps, eps_rel=eps, max_iter=args.max_iter, warm_start=False)
            for name, obj in (("batched", prob), ("shared hover problem", shared)):
                ts = []
                for _ in range(args.reps):
                    sync()
                    s0 = time.perf_counter()
                    u, traj, status = obj.solve(tx0, **kw)
                    sync()
                    ts.append(time.perf_counter() - s0)
                its = obj.last_iterations
                line = {"workload": f"lqrMpc {name}: {P} problems x 1 state, n=12 m=4 N={args.N}, eps={eps:g}",
                        "solve_ms": float(np.median(ts)) * 1e3, "solve_ms_min": float(np.min(ts)) * 1e3,
                        "iters_mean": float(its.mean()), "iters_max": int(its.max()), "status": mix(status)}
                if name == "batched":
                    line.update(construct_ms=(t1 - t0) * 1e3, setup_ms=(t2 - t1) * 1e3, table_mb=P * 7 * args.N * 4 * 16 * 8 / 1e6)
                print(json.dumps(line), flush=True)
    # the loop the feature replaces: one object per problem, each set up and solved alone
    P = args.loop_problems
    A, B, x0 = family(P, seed=P)
    for eps in args.eps:
        sync()
        t0 = time.perf_counter()
        its = []
        for i in range(P):
            one = mpcUtils.lqrMpc(A[i], B[i], Q, R, args.N, -X_UB, X_UB, -U_UB, U_UB)
            one.solve(x0[i], eps_abs=eps, eps_rel=eps, max_iter=args.max_iter, warm_start=False)
            its.append(int(one.last_iterations))
        sync()
        t = time.perf_counter() - t0
        print(json.dumps({"workload": f"lqrMpc loop of single-problem objects: {P} problems, n=12 m=4 N={args.N}, eps={eps:g}",
                          "total_ms": t * 1e3, "ms_per_problem": t * 1e3 / P, "iters_mean": float(np.mean(its))}), flush=True)


if __name__ == "__main__":
    main()
