#!/usr/bin/env python3
"""Secondary benchmark: real-time-iteration nonlinear MPC as one call (ltvMpc.realTimeIteration) against the Python loop of public calls
it replaces -- clip, relinearize, solve (step 0 cold, then warm_start="shift"), modelStep, shift of the plan.

Workload: `--batch` quadcopters (models.QuadcopterEuler, dt = 0.1, the weights and bounds of demos/lqrMpc.py in absolute coordinates) that
follow a position ramp from hover, as tools/examples/mpc_ltv.py; N = 30, 50 MPC steps, the demo tolerance eps = 1e-2.  Measured with the
adaptive penalty on (7 tabulated levels: the setup launch of every step factors 7 x batch problems) and off (1 level).
Both contenders run in one process, alternated, after one warm-up run each; a host clock around work that ends in torch.cuda.synchronize().
Prints one JSON line per variant: ms per MPC step (median, min, max over --reps) for both, their ratio, and whether the two runs agree bit
for bit.  `--profile-one-call K`: no timing; after a warm-up, K one-call runs of the first variant and nothing else (the run to put under
`rocprofv3 --kernel-trace --stats -- python tools/bench_mpc_rti.py --profile-one-call 1` for the per-kernel split)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

X_UB = np.array([1, 1, 1, 0.3, 0.3, 0.1, 0.5, 0.5, np.inf, np.inf, np.inf, np.inf])
U_UB = np.array([3.0, 3, 3, 3])
DT = 0.1
CLIP = 1e-6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--N", type=int, default=30)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--adaptive", nargs="+", type=int, default=[1, 0], help="1: adaptive penalty (7 levels), 0: one level")
    ap.add_argument("--profile-one-call", type=int, default=0)
    args = ap.parse_args()
    import torch
    from zopt_amd import models, mpcUtils, pytrees
    N, S, nb = args.N, args.steps, args.batch
    model = models.QuadcopterEuler(DT)
    uTrim = np.asarray(models.QuadcopterEuler.uTrim, dtype=np.float64)
    dev = dict(dtype=torch.float64, device="cuda")
    lo, hi = torch.as_tensor(-X_UB + CLIP, **dev), torch.as_tensor(X_UB - CLIP, **dev)

    rng = np.random.default_rng(0)                                        # the ramp of tools/examples/mpc_ltv.py
    d = rng.standard_normal((nb, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    vel, p0 = d * rng.uniform(0.2, 0.6, (nb, 1)), 2.5 * d
    xRef = np.zeros((nb, S + N, 12))
    xRef[:, :, 9:12] = p0[:, None, :] + vel[:, None, :] * (DT * np.arange(S + N))[None, :, None]
    xRef[:, :, 0:3] = vel[:, None, :]
    xRef = torch.as_tensor(xRef, **dev)
    uRef = torch.as_tensor(np.tile(uTrim, (nb, S + N - 1, 1)), **dev)
    x0 = torch.zeros((nb, 12), **dev)
    hover = lambda: pytrees.Trajectory(torch.zeros((nb, N + 1, 12), **dev), uRef[:, :N].clone())
    mk = lambda: mpcUtils.ltvMpc.fromModel(model, hover(), np.eye(12), np.eye(4), -X_UB, X_UB, uTrim - U_UB, uTrim + U_UB)

    for adaptive in args.adaptive:
        kw = dict(eps_abs=1e-2, eps_rel=1e-2, max_iter=4000, adaptive_rho=bool(adaptive))

        def py_loop(prob):
            x, plan = x0, hover()
            xs, status, its = [], [], []
            for s in range(S):
                x = torch.minimum(torch.maximum(x, lo), hi)
                xs.append(x)
                prob.relinearize(model, plan)
                u, traj, st = prob.solve(x, xRef=xRef[:, s:s + N + 1], uRef=uRef[:, s:s + N], warm_start=(False if s == 0 else "shift"), **kw)
                status.append(st)
                its.append(prob.last_iterations)
                x = mpcUtils.modelStep(model, x, u)
                plan = pytrees.Trajectory(torch.cat([traj.xTraj[:, 1:], traj.xTraj[:, -1:]], dim=1),
                                          torch.cat([traj.uTraj[:, 1:], traj.uTraj[:, -1:]], dim=1))
            xs.append(torch.minimum(torch.maximum(x, lo), hi))
            return torch.stack(xs, dim=1), np.stack(status, axis=1), np.stack(its, axis=1)

        def one_call(prob):
            run = prob.realTimeIteration(model, x0, S, plan=hover(), clip_tol=CLIP, warm_start="shift", xRef=xRef, uRef=uRef, **kw)
            return run.xTraj, run.status, run.iterations.cpu().numpy()

        if args.profile_one_call:
            prob = mk()
            for _ in range(1 + args.profile_one_call):
                one_call(prob)
            torch.cuda.synchronize()
            return
        contenders = {"loop": (py_loop, mk()), "one_call": (one_call, mk())}    # one object each: neither sees the other's warm start
        times = {k: [] for k in contenders}
        out = {}
        for r in range(args.reps + 1):                                    # (the first round warms both up and is dropped)
            for k, (fn, prob) in contenders.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out[k] = fn(prob)
                torch.cuda.synchronize()
                if r:
                    times[k].append((time.perf_counter() - t0) * 1e3 / S)
        (xl, sl, il), (xf, sf, i_f) = out["loop"], out["one_call"]
        line = {"workload": f"real-time iteration, quadcopter: {S} MPC steps x {nb} instances, n=12 m=4 N={N}, eps=1e-2, warm_start=shift, "
                            f"adaptive_rho={bool(adaptive)} ({7 if adaptive else 1} penalty levels)", "reps": args.reps}
        for k, ts in times.items():
            line.update({f"{k}_ms_per_step_median": float(np.median(ts)), f"{k}_ms_per_step_min": float(np.min(ts)),
                         f"{k}_ms_per_step_max": float(np.max(ts))})
        line["loop_over_one_call"] = line["loop_ms_per_step_median"] / line["one_call_ms_per_step_median"]
        line["same_bits"] = bool(torch.equal(xl, xf))
        line["same_statuses"] = bool(np.array_equal(sl.astype(str), sf.astype(str)))
        line["same_iterations"] = bool(np.array_equal(il, i_f))
        v, c = np.unique(sf.astype(str), return_counts=True)
        line["status"] = {str(a): int(b) for a, b in zip(v, c)}
        line["iters_mean"] = float(i_f.mean())
        line["iters_max_per_step_mean"] = float(i_f.max(axis=0).mean())
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
