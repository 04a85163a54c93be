#!/usr/bin/env python3
"""What a recorded cost costs and what it buys (models.TracedCost, zopt_amd/csrc/traced_cost.hip).  One process per library, the
variants of a comparison alternated inside it so that clock and thermal drift hit them alike; medians with min / max over the
repetitions, one JSON line per measurement (also appended to --out).  The helpers are tools/bench_traced_model.py's.

  (a) the price of a recorded cost: 8192 quadcopters, T = 100, the QuadraticCost problem of tools/bench_ilqr.py, iLQR and DDP, through
      the built-in cost, the same cost recorded (registered quadcopter) and the recorded cost on the traced quadcopter.  The recorded
      form runs per-point Hessians, conditions them in every iteration, full Jacobians, the register sweeps and the one-lane two-pass
      line search;
  (b) the gain over the torch path: the car to a goal per vehicle past a smooth keep-out penalty (tools/examples/ilqr_traced_cost.py's
      cost), T = 100, at most --max-iter iterations, at --torch-batch through the fused path and through zopt_amd/generic.py with the
      same callables in torch (the generic path has no per-trajectory parameters: one goal and one obstacle there, the same on the fused
      side), and the full batch with per-vehicle parameters through the fused path;
  (c) the line search's slot file in LDS and in private scratch once two or three tapes share it (a child process on the -DZM_LAB
      library, ZOPT_AMD_TRACED_SLOTS flipped between calls): the 16-way line search alone and the whole car solve.

    python tools/bench_traced_cost.py [--out profiles/traced_cost_bench.txt]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_traced_cost.py --only a --reps 1        # per-kernel totals of (a)
"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_traced_model as M          # noqa: E402

emit, stats, alternate, event_ms = M.emit, M.stats, M.alternate, M.event_ms


def _fn(x, name):
    import torch
    return getattr(torch if isinstance(x, torch.Tensor) else np, name)


def car_running(x, u, p):
    """p = [goal x, goal y, obstacle x, obstacle y]: distance to the goal, effort, and a smooth keep-out penalty around the obstacle"""
    dx, dy, ox, oy = x[0] - p[0], x[1] - p[1], x[0] - p[2], x[1] - p[3]
    return 0.5 * (dx * dx + dy * dy) + 0.05 * x[3] * x[3] + 0.2 * u[0] * u[0] + 0.1 * u[1] * u[1] + 4.0 / (ox * ox + oy * oy + 0.5)


def car_terminal(x, p):
    dx, dy = x[0] - p[0], x[1] - p[1]
    return 20.0 * (dx * dx + dy * dy) + 2.0 * x[3] * x[3]


def quad_costs(R):
    run = lambda x, u: sum(x[i] * x[i] for i in range(12)) + R * sum(u[j] * u[j] for j in range(4))          # noqa: E731
    term = lambda x: 10.0 * sum(x[i] * x[i] for i in range(12))                                                # noqa: E731
    return run, term


def part_a(args, torch, ilqr, models, zo):
    B, T = args.batch, args.T
    x0, ug = M.quad_problem(B, T, torch, models)
    traced, reg = models.TracedModel(zo.quad_euler_step(0.1), 12, 4), models.QuadcopterEuler(0.1)
    for name, solve, R in (("iLQR", ilqr.iterativeLqr, 1.0), ("DDP", ilqr.differentialDynamicProgramming, 0.2)):
        cost = models.QuadraticCost(np.eye(12), R * np.eye(4), 10 * np.eye(12))
        rec = models.TracedCost(*quad_costs(R), 12, 4)
        t = rec.running_tape
        emit(part="a", what=f"running tape of the recorded quadratic cost ({name})", instructions=len(t.code), constants=len(t.consts),
             slots=t.n_slots, mask=hex(t.mask))
        variants = {"QuadraticCost, registered quadcopter": lambda: solve(reg, cost, cost, x0, ug),
                    "TracedCost, registered quadcopter": lambda: solve(reg, rec, rec, x0, ug)}
        if not args.skip_traced_model:
            variants["TracedCost, traced quadcopter"] = lambda: solve(traced, rec, rec, x0, ug)
        times, res = alternate(variants, args.reps, torch.cuda.synchronize)
        for k in times:
            emit(part="a", workload=f"{name} quadcopter n=12 m=4 T={T} batch={B} fp64", variant=k,
                 converged_frac=float(res[k][3].double().mean().item()), **stats(times[k]))
        base = np.median(times["QuadraticCost, registered quadcopter"])
        Jb = res["QuadraticCost, registered quadcopter"][2]
        for k in times:
            if k.startswith("TracedCost"):
                Ja = res[k][2]
                fin = torch.isfinite(Ja) & torch.isfinite(Jb)
                emit(part="a", workload=name, variant=k, over_QuadraticCost=float(np.median(times[k]) / base),
                     max_rel_J_difference=float(((Ja[fin] - Jb[fin]).abs() / Jb[fin].abs()).max().item()))


def car_problem(B, T, torch, shared):
    rng = np.random.default_rng(5)
    dev = dict(dtype=torch.float64, device="cuda")
    x0 = np.concatenate([np.zeros((B, 2)), rng.uniform(-3, 3, (B, 1)), rng.uniform(0.5, 3.0, (B, 1))], 1)
    goal = rng.uniform(-3, 3, (B, 2))
    p = np.concatenate([goal, 0.5 * goal + rng.uniform(-0.3, 0.3, (B, 2))], 1)
    if shared:
        p = np.tile(p[:1], (B, 1))
    return torch.as_tensor(x0, **dev), torch.zeros((B, T, 2), **dev), p


def part_b(args, torch, ilqr, models):
    T, Bt = args.T, args.torch_batch
    traced = models.TracedModel(M.car_any, 4, 2)
    for solver, solve in (("iLQR", ilqr.iterativeLqr), ("DDP", ilqr.differentialDynamicProgramming)):
        kw = dict(maxIter=args.max_iter)
        x0, ug, p = car_problem(args.batch, T, torch, shared=False)
        cost = models.TracedCost(car_running, car_terminal, 4, 2, params=p)
        times, res = alternate({"fused": lambda: solve(traced, cost, cost, x0, ug, **kw)}, args.reps, torch.cuda.synchronize)
        emit(part="b", workload=f"{solver} car with keep-out penalty n=4 m=2 T={T} batch={args.batch}, goal and obstacle per vehicle",
             path="TracedModel + TracedCost", converged_frac=float(res["fused"][3].double().mean().item()), **stats(times["fused"]))
        xs, us, ps = car_problem(Bt, T, torch, shared=True)
        one = models.TracedCost(car_running, car_terminal, 4, 2, params=ps[0])
        pt = torch.as_tensor(ps[0], dtype=torch.float64, device="cuda")
        run_t, term_t = (lambda x, u: car_running(x, u, pt)), (lambda x: car_terminal(x, pt))
        times, res = alternate({"TracedModel + TracedCost": lambda: solve(traced, one, one, xs, us, **kw),
                                "torch callables (generic.py)": lambda: solve(M.car_any, run_t, term_t, xs, us, **kw)},
                               args.torch_reps, torch.cuda.synchronize)
        for k in times:
            emit(part="b", workload=f"{solver} car with keep-out penalty n=4 m=2 T={T} batch={Bt}, one goal and obstacle", path=k,
                 converged_frac=float(res[k][3].double().mean().item()), **stats(times[k]))
        Ja, Jb = res["TracedModel + TracedCost"][2], res["torch callables (generic.py)"][2]
        emit(part="b", workload=f"{solver} car batch={Bt}",
             torch_over_fused=float(np.median(times["torch callables (generic.py)"]) / np.median(times["TracedModel + TracedCost"])),
             median_rel_J_difference=float(((Ja - Jb).abs() / Jb.abs()).median().item()))


def part_c_child(args, torch, ilqr, models, pt, zo):
    """the slot file of the traced-cost line search in LDS and in scratch, alternated (the -DZM_LAB library)"""
    B, T = args.batch, args.T
    x0, l, L, xp, up = M.linesearch_problem(B, T, torch, models)
    rec = models.TracedCost(*quad_costs(1.0), 12, 4)
    pol, prev = pt.AffinePolicy(l, L), pt.Trajectory(xp, up)
    for label, md in (("registered quadcopter", models.QuadcopterEuler(0.1)), ("traced quadcopter", models.TracedModel(zo.quad_euler_step(0.1), 12, 4))):
        times, ref = {"lds": [], "scratch": []}, {}
        for r in range(args.reps + 1):
            for k in ("lds", "scratch"):
                os.environ["ZOPT_AMD_TRACED_SLOTS"] = k
                ms = event_ms(torch, lambda: ilqr.forwardPass2(x0, md, rec, pol, prev), 1)
                ref[k] = ilqr.forwardPass2(x0, md, rec, pol, prev)[1]
                if r:
                    times[k] += ms
        a, b = ref["lds"], ref["scratch"]
        assert bool(((a == b) | (a.isnan() & b.isnan())).all())          # the same costs bit for bit
        for k in times:
            emit(part="c", kernel=f"traced_cost_rollout_kernel<16>, {label}, slot file in {k}", workload=f"forwardPass2 T={T} batch={B}",
                 note="device events around the call (uploads excluded: device tensors in)", **stats(times[k]))
        emit(part="c", kernel=f"16-way line search, {label}", scratch_over_lds=float(np.median(times["scratch"]) / np.median(times["lds"])))
    x0c, ugc, p = car_problem(B, T, torch, shared=False)
    cost, car = models.TracedCost(car_running, car_terminal, 4, 2, params=p), models.TracedModel(M.car_any, 4, 2)

    def solve_with(k):
        os.environ["ZOPT_AMD_TRACED_SLOTS"] = k
        return ilqr.iterativeLqr(car, cost, cost, x0c, ugc, maxIter=args.max_iter)
    times, res = alternate({k: (lambda k=k: solve_with(k)) for k in ("lds", "scratch")}, args.reps, torch.cuda.synchronize)
    assert bool((res["lds"][2] == res["scratch"][2]).all())
    for k in times:
        emit(part="c", what=f"whole iLQR solve, car with keep-out penalty, T={T} batch={B}, line search's slot file in {k}", **stats(times[k]))
    emit(part="c", what="whole iLQR solve", scratch_over_lds=float(np.median(times["scratch"]) / np.median(times["lds"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--torch-batch", type=int, default=256)
    ap.add_argument("--torch-reps", type=int, default=2)
    ap.add_argument("--max-iter", type=int, default=50)
    ap.add_argument("--only", default="abc")
    ap.add_argument("--skip-traced-model", action="store_true", help="(a) without the traced quadcopter (its solves take seconds each)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--slots-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    M.OUT = args.out
    import torch
    from oracle import zopt_oracle as zo          # (the oracle's quadcopter callable is a subject of (a); the product never imports it)
    from zopt_amd import _lib, ilqrUtils, models, pytrees
    if args.slots_child:
        return part_c_child(args, torch, ilqrUtils, models, pytrees, zo)
    if args.out and os.path.exists(args.out):
        os.remove(args.out)
    emit(tool="tools/bench_traced_cost.py", device=torch.cuda.get_device_name(0),
         args={k: v for k, v in vars(args).items() if k not in ("out", "slots_child")})
    if "a" in args.only:
        part_a(args, torch, ilqrUtils, models, zo)
    if "b" in args.only:
        part_b(args, torch, ilqrUtils, models)
    if "c" in args.only:
        torch.cuda.synchronize()
        env = dict(os.environ, ZOPT_AMD_LIB=_lib.LAB_LIB_PATH)
        cmd = [sys.executable, os.path.abspath(__file__), "--slots-child", "--batch", str(args.batch), "--T", str(args.T), "--reps", str(args.reps),
               "--max-iter", str(args.max_iter)]
        subprocess.run(cmd + (["--out", args.out] if args.out else []), env=env, check=True)


if __name__ == "__main__":
    main()
