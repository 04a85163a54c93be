#!/usr/bin/env python3
"""What a state box costs the fused iLQR solve: 8192 quadcopters, T = 100, a TrackingCost about hover (demo weights, a goal per
trajectory, uRef = uTrim), alternated in one process so that clock and thermal drift hit all alike:
  (a) box, infinite bounds: iterativeLqr(InputBox(model, -inf, inf), ...) -- the input box's kernels, the baseline;
  (b) state box around it, every bound infinite: the same iterates on the penalty forms (one-lane two-pass line search with the
      penalty, the penalty expansion, the sweep with the diagonal addend), so (b) / (a) is the price of those forms;
  (c) state box without an input box, every bound infinite, against the plain solve (ring sweep on packed Jacobians, four-lane /
      all-store line search);
  (b1), (c1): (b) and (c) with outer = 1 -- one inner solve, the iteration counts of (a) and of the plain solve: a trajectory whose
      inner solve does not converge (4 % here, NaN ones among them) is not done, so (b) and (c) run it through all 10 outer
      iterations of 100 iLQR iterations each, which is what their ratios mostly measure;
  (d) a floor per trajectory 0.2 m under the lower of its start and its goal (z points down) and a 3 m/s cap on the body velocities:
      another problem, reported for its own sake -- time, outer and inner iteration counts, the share done, the largest violation.
Medians with min / max over the repetitions; one JSON line per variant and one for the ratios."""
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
    inf = np.full(12, np.inf)
    x_lb, x_ub = np.tile(-inf, (B, 1)), np.tile(inf, (B, 1))
    x_ub[:, 11] = np.maximum(x0[:, 11], goal[:, 11].cpu().numpy()) + 0.2      # z points down: no sinking below the lower of start and goal
    x_lb[:, 0:3], x_ub[:, 0:3] = -3.0, 3.0                       # body velocities
    box_inf = models.InputBox(model, -np.inf, np.inf)
    variants = {"(a) box, infinite bounds": box_inf,
                "(b) state box in an input box, infinite bounds": models.StateBox(box_inf, -inf, inf),
                "plain": model,
                "(c) state box, infinite bounds": models.StateBox(model, -inf, inf),
                "(b1) as (b), outer = 1": models.StateBox(box_inf, -inf, inf, outer=1),
                "(c1) as (c), outer = 1": models.StateBox(model, -inf, inf, outer=1),
                "(d) floor per trajectory, |uvw| <= 3": models.StateBox(model, x_lb, x_ub)}

    def run(v):
        if isinstance(v, models.StateBox):
            return ilqrUtils.constrainedIterativeLqr(v, cost, cost, tx0, tug)
        return ilqrUtils.iterativeLqr(v, cost, cost, tx0, tug)
    res = {}
    for v in variants.values():                                 # warm-up at the timed shape: every kernel form of every variant once
        run(v)
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.reps):                                  # alternated
        for k, v in variants.items():
            t0 = time.perf_counter()
            res[k] = run(v)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
    for k in variants:
        traj, _, J, conv = res[k][:4]
        row = {"workload": f"iterativeLqr quadcopter n=12 m=4 T={T} batch={B} fp64, TrackingCost about hover", "variant": k,
               "reps": args.reps, "solve_ms_median": float(np.median(times[k])), "solve_ms_min": min(times[k]),
               "solve_ms_max": max(times[k]), "converged_frac": float(conv.double().mean().item()),
               "J_mean_finite": float(J[torch.isfinite(J)].mean().item())}
        if len(res[k]) == 5:
            info = res[k][4]
            fin = torch.isfinite(info.violation)
            row.update({"outer_iterations_max": int(info.outerIterations.max().item()),
                        "outer_iterations_mean": float(info.outerIterations.double().mean().item()),
                        "inner_iterations_total_max": int(info.innerIterations.sum(-1).max().item()),
                        "inner_iterations_total_mean": float(info.innerIterations.sum(-1).double().mean().item()),
                        "largest_violation_where_done": float(info.violation[conv].max().item()) if bool(conv.any()) else None,
                        "largest_violation_finite": float(info.violation[fin].max().item()),
                        "share_with_an_active_bound": float(((info.lam_ub > 0).flatten(1).any(1) | (info.lam_lb > 0).flatten(1).any(1)).double().mean().item())})
        print(json.dumps(row))
    med = lambda k: float(np.median(times[k]))                   # noqa: E731
    a, b, p, c = (res[k] for k in list(variants)[:4])
    fin = torch.isfinite(a[2]) & torch.isfinite(b[2])
    finc = torch.isfinite(p[2]) & torch.isfinite(c[2])
    print(json.dumps({"b_over_a_median": med(list(variants)[1]) / med(list(variants)[0]),
                      "c_over_plain_median": med(list(variants)[3]) / med("plain"),
                      "b1_over_a_median": med(list(variants)[4]) / med(list(variants)[0]),
                      "c1_over_plain_median": med(list(variants)[5]) / med("plain"),
                      "b_vs_a_J_rel_diff_max": float(((a[2][fin] - b[2][fin]).abs() / a[2][fin].abs()).max().item()),
                      "b_vs_a_same_converged": bool(torch.equal(a[3], b[3])),
                      "c_vs_plain_J_rel_diff_max": float(((p[2][finc] - c[2][finc]).abs() / p[2][finc].abs()).max().item()),
                      "c_vs_plain_same_converged": bool(torch.equal(p[3], c[3]))}))


if __name__ == "__main__":
    main()
