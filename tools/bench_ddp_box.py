#!/usr/bin/env python3
"""What an input box costs the fused DDP solve: 8192 quadcopters, T = 100, a TrackingCost about hover (demo weights, a goal per
trajectory, uRef = uTrim), solved four ways, alternated in one process so that clock and thermal drift hit all alike:
  * plain DDP: differentialDynamicProgramming(model, ...) -- the ring sweep on packed Jacobians and sparse second derivatives, the
    four-lane / all-store line search;
  * box DDP, infinite bounds: differentialDynamicProgramming(InputBox(model, -inf, inf), ...) -- the same problem, so the ratio is
    the cost of the register sweep with its box-QP, full Jacobians, pair rows and the one-lane two-pass line search over the plain
    path's forms;
  * box DDP, limits: thrust within uTrim +- 2, moments within +- 0.05 (tools/examples/ddp_box.py's limits; another problem, other
    iterates, reported for its own sake);
  * box iLQR, limits: iterativeLqr on the same bounded problem -- what the second-order terms cost and buy under the same box.
Medians with min / max over the repetitions and the share of starts that converge; one JSON line per solve and one for the ratios."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    import torch
    from zopt_amd import ilqrUtils, models
    rng = np.random.default_rng(2)
    B, T = args.batch, args.T
    uTrim = np.asarray(models.QuadcopterEuler.uTrim, dtype=np.float64)
    dev = dict(dtype=torch.float64, device="cuda")
    x0 = np.zeros((B, 12))
    x0[:, 9:12] = rng.uniform(-10, 10, (B, 3))
    tx0 = torch.as_tensor(x0, **dev)
    tug = torch.as_tensor(np.tile(uTrim, (B, T, 1)), **dev)
    goal = torch.zeros((B, 12), **dev)
    goal[:, 9:12] = torch.as_tensor(rng.uniform(-10, 10, (B, 3)), **dev)
    cost = models.TrackingCost(np.eye(12), np.eye(4), 10 * np.eye(12), goal[:, None, :], uTrim)
    model = models.QuadcopterEuler(0.1)
    lim = np.array([2.0, 0.05, 0.05, 0.05])
    limited = models.InputBox(model, uTrim - lim, uTrim + lim)
    ddp, ilqr = ilqrUtils.differentialDynamicProgramming, ilqrUtils.iterativeLqr
    variants = {"plain DDP": (ddp, model), "box DDP, infinite bounds": (ddp, models.InputBox(model, -np.inf, np.inf)),
                "box DDP, thrust uTrim +- 2, moments +- 0.05": (ddp, limited),
                "box iLQR, thrust uTrim +- 2, moments +- 0.05": (ilqr, limited)}
    res = {}
    for solve, v in variants.values():                          # warm-up at the timed shape: every kernel form of every variant once
        solve(v, cost, cost, tx0, tug)
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.reps):                                  # alternated
        for k, (solve, v) in variants.items():
            t0 = time.perf_counter()
            res[k] = solve(v, cost, cost, tx0, tug)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
    lo, hi = torch.as_tensor(uTrim - lim, **dev), torch.as_tensor(uTrim + lim, **dev)
    for k in variants:
        traj, _, J, conv = res[k]
        u = traj.uTraj[torch.isfinite(J)]
        viol = float(torch.clamp(torch.maximum(lo - u, u - hi), min=0).max().item())
        print(json.dumps({"workload": f"quadcopter n=12 m=4 T={T} batch={B} fp64, TrackingCost about hover", "variant": k,
                          "reps": args.reps, "solve_ms_median": float(np.median(times[k])), "solve_ms_min": min(times[k]),
                          "solve_ms_max": max(times[k]), "converged_frac": float(conv.double().mean().item()),
                          "J_mean_finite": float(J[torch.isfinite(J)].mean().item()), "largest_violation_of_the_limits": viol}))
    med = {k: float(np.median(t)) for k, t in times.items()}
    p, b = res["plain DDP"], res["box DDP, infinite bounds"]
    fin = torch.isfinite(p[2]) & torch.isfinite(b[2])
    print(json.dumps({"infinite_bounds_over_plain_ddp_median": med["box DDP, infinite bounds"] / med["plain DDP"],
                      "ddp_limits_over_plain_ddp_median": med["box DDP, thrust uTrim +- 2, moments +- 0.05"] / med["plain DDP"],
                      "ddp_limits_over_ilqr_limits_median": med["box DDP, thrust uTrim +- 2, moments +- 0.05"] /
                      med["box iLQR, thrust uTrim +- 2, moments +- 0.05"],
                      "infinite_bounds_J_rel_diff_max": float(((p[2][fin] - b[2][fin]).abs() / p[2][fin].abs()).max().item()),
                      "infinite_bounds_same_converged": bool(torch.equal(p[3], b[3]))}))


if __name__ == "__main__":
    main()
