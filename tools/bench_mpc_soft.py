#!/usr/bin/env python3
"""Secondary benchmark: what soft box constraints cost on lqrMpc (`soften`; zm_mpc_solve_soft_f64, zm_mpc_closed_loop_soft_f64).
Workload: `--batch` quadcopters linearised at hover (demos/lqrMpc.py:11-32: dt = 0.1, Q = R = I, the demo's bounds), N = 30, the x0 of
tools/bench_mpc.py (same seed).  The legs of each part are alternated in one process after a warm-up round; a host clock around work that
ends in torch.cuda.synchronize(); medians with min / max over --reps.

(a) solve, cold, at eps 1e-4 (reported per ADMM iteration: the solve time over the slowest instance's count) and at eps 1e-2 (per solve):
      plain : the object as built                                   (zm_mpc_solve_relaxed_f64)
      hard  : softened with every l1 = +inf                         (zm_mpc_solve_soft_f64: the same iterations -- the tool asserts equal
                                                                     iteration counts and equal u)
      soft  : l1 = --l1 on the eight bounded states                 (zm_mpc_solve_soft_f64: its own iterations, per iteration of its count)
(b) simulate over --steps MPC steps at eps 1e-2 with a gust at step --gust-step: 0.6 m/s added to the velocity of every vehicle along its
    direction of flight, which pushes those flying at the velocity bound through it:
      hard   : the plain object, clip_tol = 1e-6 (the clip puts the state back into the box: the run it returns is not the plant's)
      soft   : the softened object, one call
      loop   : the softened object, the loop `simulate` documents written by hand over `solve` -- the reference for "one call is faster"
    ms per MPC step, vehicle-steps not "optimal", vehicle-steps the clip moved by more than 0.05 (hard) and, for soft, how far the run
    leaves the box, the first and the last step at which a vehicle is more than 0.05 outside, and whether it agrees with the loop in every
    status and iteration count."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

X_UB = np.array([1, 1, 1, 0.3, 0.3, 0.1, 0.5, 0.5, np.inf, np.inf, np.inf, np.inf])
U_UB = np.array([3.0, 3, 3, 3])
DT, CLIP, MOVED = 0.1, 1e-6, 0.05


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--N", type=int, default=30)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--gust-step", type=int, default=10)
    ap.add_argument("--l1", type=float, default=100.0)
    ap.add_argument("--max-iter", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    import torch
    from zopt_amd import models, mpcUtils, pytrees
    nb, N, S = args.batch, args.N, args.steps
    hover = pytrees.AffineDynamics.from_function(models.QuadcopterEuler(DT), np.zeros(12), models.QuadcopterEuler.uTrim)
    A, B = np.asarray(hover.f_x), np.asarray(hover.f_u)
    mk = lambda: mpcUtils.lqrMpc(A, B, np.eye(12), np.eye(4), N, -X_UB, X_UB, -U_UB, U_UB)
    l1 = np.where(np.isfinite(X_UB), args.l1, np.inf)
    rng = np.random.default_rng(1)                                       # tools/bench_mpc.py: the same draws in the same order
    x0 = np.clip(0.03 * rng.standard_normal((nb, 12)), -X_UB + 1e-6, X_UB - 1e-6)
    x0[:, 9:12] = rng.uniform(-10, 10, (nb, 3))
    tx0 = torch.as_tensor(x0, device="cuda")
    sync = torch.cuda.synchronize

    def alternated(legs, reps, scale=1.0):
        """{leg: sorted times in ms} of its function, the legs alternated; the first round warms up and is dropped"""
        times = {k: [] for k in legs}
        for r in range(reps + 1):
            for name, f in legs.items():
                sync()
                t0 = time.perf_counter()
                f()
                sync()
                if r:
                    times[name].append((time.perf_counter() - t0) * 1e3 * scale)
        return {k: np.sort(v) for k, v in times.items()}

    # ---- (a) solve
    probs = {"plain (zm_mpc_solve_relaxed_f64)": mk(), "hard (zm_mpc_solve_soft_f64, l1 = inf)": mk().soften(x_soft_l1=np.full(12, np.inf)),
             f"soft (zm_mpc_solve_soft_f64, l1 = {args.l1:g} on 8 states)": mk().soften(x_soft_l1=l1)}
    k_plain, k_hard, k_soft = probs
    for eps, what in ((1e-4, "ms_per_admm_iteration"), (1e-2, "solve_ms")):
        kw = dict(eps_abs=eps, eps_rel=eps, max_iter=args.max_iter, warm_start=False)
        seen = {}

        def solve(name):
            u, _, status = probs[name].solve(tx0, **kw)
            seen[name] = (probs[name].last_iterations.copy(), float(np.mean(status == "optimal")), u)
        ts = alternated({k: (lambda k=k: solve(k)) for k in probs}, args.reps)
        assert np.array_equal(seen[k_plain][0], seen[k_hard][0]) and torch.equal(seen[k_plain][2], seen[k_hard][2]), \
            "all-hard weights must run the plain solve's iterations"
        med = {}
        for name in probs:
            its, ok, _ = seen[name]
            per = 1.0 / max(int(its.max()), 1) if what == "ms_per_admm_iteration" else 1.0
            med[name] = float(np.median(ts[name])) * per
            print(json.dumps({"timed": name, "workload": f"quadcopter n=12 m=4 N={N}, {nb} instances, eps={eps:g}, cold", "reps": args.reps,
                              "iters_mean": float(its.mean()), "iters_max": int(its.max()), "optimal_frac": ok,
                              what + "_median": med[name], what + "_min": float(ts[name][0]) * per, what + "_max": float(ts[name][-1]) * per}),
                  flush=True)
        print(json.dumps({"eps": eps, what + "_ratio_hard_over_plain": med[k_hard] / med[k_plain],
                          what + "_ratio_soft_over_plain": med[k_soft] / med[k_plain]}), flush=True)

    # ---- (b) simulate with a gust
    kw = dict(eps_abs=1e-2, eps_rel=1e-2, eps_prim_inf=1e-3, max_iter=4000)      # the options of tools/bench_mpc_closed_loop.py
    w = np.zeros((nb, S, 12))
    w[:, args.gust_step, 0:3] = -0.6 * np.sign(x0[:, 9:12])                      # (every vehicle flies towards the origin)
    tw = torch.as_tensor(w, device="cuda")
    hard, soft, looped = mk(), mk().soften(x_soft_l1=l1), mk().soften(x_soft_l1=l1)
    out = {}

    def run(name, prob):
        r = prob.simulate(tx0, S, disturbance=tw, clip_tol=CLIP, warm_start="shift", return_predictions=(name == "hard"), **kw)
        out[name] = (r.xTraj, r.status, r.iterations.cpu().numpy(), r.predictions)

    def loop():   # (every bounded state is soft and the others have no bound: the documented loop clips nothing)
        x, xs, status, its = tx0, [], [], []
        for s in range(S):
            xs.append(x)
            _, traj, st = looped.solve(x, warm_start=(False if s == 0 else "shift"), **kw)
            status.append(st)
            its.append(looped.last_iterations)
            x = traj.xTraj[:, 1] + tw[:, s]
        xs.append(x)
        out["loop"] = (torch.stack(xs, dim=1), np.stack(status, axis=1), np.stack(its, axis=1), None)
    ts = alternated({"hard": lambda: run("hard", hard), "soft": lambda: run("soft", soft), "loop": loop}, args.reps, 1.0 / S)
    line = {"workload": f"closed loop with a gust at step {args.gust_step}: {S} MPC steps x {nb} instances, n=12 m=4 N={N}, eps=1e-2, "
                        f"warm_start=shift", "reps": args.reps}
    for k, t in ts.items():
        line.update({f"{k}_ms_per_step_median": float(np.median(t)), f"{k}_ms_per_step_min": float(t[0]), f"{k}_ms_per_step_max": float(t[-1])})
        line[f"{k}_vehicle_steps_not_optimal"] = int(np.sum(out[k][1].astype(str) != "optimal"))
    line["loop_over_soft"] = line["loop_ms_per_step_median"] / line["soft_ms_per_step_median"]
    line["soft_over_hard"] = line["soft_ms_per_step_median"] / line["hard_ms_per_step_median"]
    xh, _, _, pred = out["hard"]
    plant = pred.xTraj[:, :, 1] + tw                                              # what the plant did, before the clip
    # (a solve at eps 1e-2 leaves its successor state up to ~1e-2 outside: only moves beyond MOVED count as the clip's, or as outside)
    line["hard_vehicle_steps_moved_by_the_clip"] = int(torch.sum(torch.any((plant - xh[:, 1:]).abs() > MOVED, dim=-1)).item())
    xs_, ss, its_s, _ = out["soft"]
    xl_, sl, its_l, _ = out["loop"]
    ub = torch.as_tensor(np.where(np.isfinite(X_UB), X_UB, 1e300), device="cuda")
    excess = torch.clamp(xs_.abs() - ub, min=0.0).amax(dim=(0, 2)).cpu().numpy()  # per step: how far the worst vehicle is outside its box
    outside = np.flatnonzero(excess > MOVED)
    line.update({"soft_largest_excursion": float(excess.max()), "soft_first_step_outside": int(outside[0]) if outside.size else None,
                 "soft_last_step_outside": int(outside[-1]) if outside.size else None,
                 "soft_same_statuses_as_loop": bool(np.array_equal(ss.astype(str), sl.astype(str))),
                 "soft_same_iterations_as_loop": bool(np.array_equal(its_s, its_l)),
                 "soft_max_state_difference_from_loop": float((xs_ - xl_).abs().max().item()),
                 "soft_iters_mean": float(its_s.mean())})
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
