#!/usr/bin/env python3
"""What a tracking cost costs the fused iLQR solve: BASELINE configs[3] (8192 quadcopters, T = 100, demo weights, x0[9:12] ~ U(-10, 10)^3,
uGuess = uTrim, seed 2 -- tools/bench_ilqr.py's workload) solved with models.QuadraticCost and with models.TrackingCost on a ZERO
reference (the same iterates bit for bit, hence the same work: only the kernels differ), alternated in one process so that clock and
thermal drift hit both alike; then the TrackingCost solve with a goal per trajectory and uRef = uTrim (another problem: other
iterates, reported for its own sake).  Medians with min / max over the repetitions; one JSON line per variant and one for the ratio."""
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
    x0 = np.zeros((B, 12))
    x0[:, 9:12] = rng.uniform(-10, 10, (B, 3))
    Q, R, Qf = np.eye(12), np.eye(4), 10 * np.eye(12)
    model = models.QuadcopterEuler(0.1)
    dev = dict(dtype=torch.float64, device="cuda")
    tx0 = torch.as_tensor(x0, **dev)
    tug = torch.as_tensor(np.tile(models.QuadcopterEuler.uTrim, (B, T, 1)), **dev)
    goal = torch.zeros((B, 12), **dev)
    goal[:, 9:12] = torch.as_tensor(rng.uniform(-10, 10, (B, 3)), **dev)
    costs = {"QuadraticCost": models.QuadraticCost(Q, R, Qf),
             "TrackingCost, zero reference": models.TrackingCost(Q, R, Qf, torch.zeros((B, 1, 12), **dev), torch.zeros(4, **dev)),
             "TrackingCost, goal per trajectory, uRef = uTrim": models.TrackingCost(Q, R, Qf, goal[:, None, :], models.QuadcopterEuler.uTrim)}
    res = {}
    for c in costs.values():                                   # warm-up at the timed shape: every kernel form of every variant once
        ilqrUtils.iterativeLqr(model, c, c, tx0, tug)
    torch.cuda.synchronize()
    times = {k: [] for k in costs}
    for _ in range(args.reps):                                 # alternated
        for k, c in costs.items():
            t0 = time.perf_counter()
            res[k] = ilqrUtils.iterativeLqr(model, c, c, tx0, tug)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
    q_, z_ = res["QuadraticCost"], res["TrackingCost, zero reference"]
    same = all(bool(((a == b) | (a.isnan() & b.isnan())).all())          # (the starts that never converge end in NaN: NaN == NaN here)
               for a, b in ((q_[0].xTraj, z_[0].xTraj), (q_[0].uTraj, z_[0].uTraj), (q_[1], z_[1]), (q_[2], z_[2]))) and torch.equal(q_[3], z_[3])
    for k in costs:
        J, conv = res[k][2], res[k][3]
        print(json.dumps({"workload": f"iterativeLqr quadcopter n=12 m=4 T={T} batch={B} fp64", "cost": k, "reps": args.reps,
                          "solve_ms_median": float(np.median(times[k])), "solve_ms_min": min(times[k]), "solve_ms_max": max(times[k]),
                          "converged_frac": float(conv.double().mean().item()),
                          "J_mean_finite": float(J[torch.isfinite(J)].mean().item())}))
    q, z = np.median(times["QuadraticCost"]), np.median(times["TrackingCost, zero reference"])
    print(json.dumps({"zero_reference_over_QuadraticCost_median": float(z / q), "same_iterates_bit_for_bit": bool(same)}))


if __name__ == "__main__":
    main()
