#!/usr/bin/env python3
"""Secondary benchmark: the receding-horizon run as one call (lqrMpc.simulate) against the Python loop over lqrMpc.solve with the same
semantics -- clip, solve (step 0 cold, then warm_start="shift"), x <- xTraj[1], every instance kept in the run whatever its status (no
parking of dead instances, unlike the loop of tools/bench_mpc.py).

Workload: the one the README quotes -- `--batch` quadcopter instances linearised at hover (demos/lqrMpc.py:11-32: dt = 0.1, Q = R = I, the
demo's bounds), N = 30, 50 MPC steps, eps 1e-2, the x0 of tools/bench_mpc.py (same seed) -- and next to it
  * per-problem: `--batch` distinct linearisations, as tools/bench_mpc_batched.py builds them (one state per problem);
  * tracking:    the hover problem following a position ramp (every instance from where it stands), which goes by the host loop of launches.
Both contenders run in one process, alternated, after one warm-up run each; a host clock around work that ends in torch.cuda.synchronize().
Prints one JSON line per family: ms per MPC step (median, min, max over --reps) for both, their ratio, and whether the two runs agree in
every status and iteration count (and how far apart their states are)."""
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
    ap.add_argument("--families", nargs="+", default=["shared", "per_problem", "tracking"])
    args = ap.parse_args()
    import torch
    from tools.bench_mpc_batched import family
    from zopt_amd import models, mpcUtils, pytrees
    N, S, nb = args.N, args.steps, args.batch
    kw = dict(solver="OSQP", eps_abs=1e-2, eps_rel=1e-2, eps_prim_inf=1e-3, max_iter=4000)      # the options of tools/bench_mpc.py's loop
    lo = torch.as_tensor(-X_UB + CLIP, device="cuda")
    hi = torch.as_tensor(X_UB - CLIP, device="cuda")

    def py_loop(prob, tx0, refs):
        x = tx0
        xs, status, its = [], [], []
        for s in range(S):
            x = torch.minimum(torch.maximum(x, lo), hi)
            xs.append(x)
            win = {k: v[:, s:s + N + (k == "xRef")] for k, v in refs.items()}
            _, traj, st = prob.solve(x, warm_start=(False if s == 0 else "shift"), **win, **kw)
            status.append(st)
            its.append(prob.last_iterations)
            x = traj.xTraj[:, 1]
        xs.append(torch.minimum(torch.maximum(x, lo), hi))
        return torch.stack(xs, dim=1), np.stack(status, axis=1), np.stack(its, axis=1)

    def fused(prob, tx0, refs):
        run = prob.simulate(tx0, S, clip_tol=CLIP, warm_start="shift", **refs, **kw)
        return run.xTraj, run.status, run.iterations.cpu().numpy()

    hover = pytrees.AffineDynamics.from_function(models.QuadcopterEuler(DT), np.zeros(12), models.QuadcopterEuler.uTrim)
    A0, B0 = np.asarray(hover.f_x), np.asarray(hover.f_u)
    rng = np.random.default_rng(1)                                       # tools/bench_mpc.py: the same draws in the same order
    x0 = np.clip(0.03 * rng.standard_normal((nb, 12)), -X_UB + 1e-6, X_UB - 1e-6)
    x0[:, 9:12] = rng.uniform(-10, 10, (nb, 3))
    for name in args.families:
        refs = {}
        if name == "per_problem":
            A, B, xs0 = family(nb, seed=nb)
            mk = lambda: mpcUtils.lqrMpc(A, B, np.eye(12), np.eye(4), N, -X_UB, X_UB, -U_UB, U_UB)
        else:
            xs0 = x0
            mk = lambda: mpcUtils.lqrMpc(A0, B0, np.eye(12), np.eye(4), N, -X_UB, X_UB, -U_UB, U_UB)
            if name == "tracking":                                       # the ramp of tools/bench_mpc.py --track, S + N rows long
                vel = np.random.default_rng(2).uniform(-0.5, 0.5, (nb, 3))
                xRef = np.zeros((nb, S + N, 12))
                xRef[:, :, 9:12] = xs0[:, None, 9:12] + vel[:, None, :] * (DT * np.arange(S + N))[None, :, None]
                xRef[:, :, 0:3] = vel[:, None, :]
                refs = {"xRef": torch.as_tensor(xRef, device="cuda")}
        tx0 = torch.as_tensor(xs0, device="cuda")
        contenders = {"loop": (py_loop, mk()), "simulate": (fused, mk())}    # one object each: neither sees the other's warm start
        times = {k: [] for k in contenders}
        out = {}
        for r in range(args.reps + 1):                                   # (the first round warms both up and is dropped)
            for k, (fn, prob) in contenders.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out[k] = fn(prob, tx0, refs)
                torch.cuda.synchronize()
                if r:
                    times[k].append((time.perf_counter() - t0) * 1e3 / S)
        (xl, sl, il), (xf, sf, i_f) = out["loop"], out["simulate"]
        line = {"workload": f"closed loop, {name}: {S} MPC steps x {nb} instances, n=12 m=4 N={N}, eps=1e-2, warm_start=shift", "reps": args.reps}
        for k, ts in times.items():
            line.update({f"{k}_ms_per_step_median": float(np.median(ts)), f"{k}_ms_per_step_min": float(np.min(ts)),
                         f"{k}_ms_per_step_max": float(np.max(ts))})
        line["loop_over_simulate"] = line["loop_ms_per_step_median"] / line["simulate_ms_per_step_median"]
        line["same_statuses"] = bool(np.array_equal(sl.astype(str), sf.astype(str)))
        line["same_iterations"] = bool(np.array_equal(il, i_f))
        line["max_state_difference"] = float((xl - xf).abs().max().item())
        v, c = np.unique(sf.astype(str), return_counts=True)
        line["status"] = {str(a): int(b) for a, b in zip(v, c)}
        line["iters_mean"] = float(i_f.mean())
        line["iters_max_per_step_mean"] = float(i_f.max(axis=0).mean())
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
