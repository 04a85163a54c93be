#!/usr/bin/env python3
"""What a traced model costs and what it buys (models.TracedModel, zopt_amd/csrc/traced.hip).  One process per library, the variants
of a comparison alternated inside it so that clock and thermal drift hit them alike; medians with min / max over the repetitions, one
JSON line per measurement (also appended to --out).

  (a) the price of interpretation: 8192 quadcopters, T = 100 (tools/bench_ilqr.py's workload) through the traced oracle callable and
      through the registered QuadcopterEuler, iLQR and DDP -- the same problems, the same iterates up to rounding;
  (b) the gain over the torch path: cart-pole and car through TracedModel at 8192 and at --torch-batch, and the same callables in torch
      through zopt_amd/generic.py at --torch-batch;
  (c) per kernel, by device events around the array-level calls: the 16-way line search with its slot file in LDS and in private
      scratch (a child process on the -DZM_LAB library, ZOPT_AMD_TRACED_SLOTS flipped between calls), and the first- and second-order
      expansions against the registered quadcopter's.

    python tools/bench_traced_model.py [--out profiles/traced_model_bench.txt]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_traced_model.py --only a --reps 1        # per-kernel totals of (a)
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = None


def emit(**row):
    line = json.dumps(row)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as fh:
            fh.write(line + "\n")


def stats(ms):
    return {"ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms)), "reps": len(ms)}


def alternate(variants, reps, sync):
    """variants: {name: thunk}; every thunk once as warm-up, then `reps` rounds in turn -> ({name: [ms]}, {name: last result})"""
    res = {k: f() for k, f in variants.items()}
    sync()
    times = {k: [] for k in variants}
    for _ in range(reps):
        for k, f in variants.items():
            t0 = time.perf_counter()
            res[k] = f()
            sync()
            times[k].append((time.perf_counter() - t0) * 1e3)
    return times, res


def cartpole_any(x, u, dt=0.02, mc=1.0, mp=0.1, length=0.5, g=9.81):
    """cart-pole, one callable for NumPy recording scalars and torch tensors"""
    import torch
    tt = isinstance(x, torch.Tensor)
    sin, cos = (torch.sin, torch.cos) if tt else (np.sin, np.cos)
    pos, th, v, om = x[0], x[1], x[2], x[3]
    s, c = sin(th), cos(th)
    den = mc + mp * s * s
    acc = (u[0] + mp * s * (length * om * om + g * c)) / den
    alpha = (-u[0] * c - mp * length * om * om * c * s - (mc + mp) * g * s) / (length * den)
    out = [pos + dt * v, th + dt * om, v + dt * acc, om + dt * alpha]
    return torch.stack(out) if tt else np.array(out)


def car_any(x, u, dt=0.1, wheelbase=2.5):
    import torch
    tt = isinstance(x, torch.Tensor)
    sin, cos, tan = (torch.sin, torch.cos, torch.tan) if tt else (np.sin, np.cos, np.tan)
    px, py, th, v = x[0], x[1], x[2], x[3]
    out = [px + dt * v * cos(th), py + dt * v * sin(th), th + dt * v * tan(u[0]) / wheelbase, v + dt * u[1]]
    return torch.stack(out) if tt else np.array(out)


def quad_problem(B, T, torch, models):
    rng = np.random.default_rng(2)
    x0 = np.zeros((B, 12))
    x0[:, 9:12] = rng.uniform(-10, 10, (B, 3))
    dev = dict(dtype=torch.float64, device="cuda")
    return torch.as_tensor(x0, **dev), torch.as_tensor(np.tile(models.QuadcopterEuler.uTrim, (B, T, 1)), **dev)


def part_a(args, torch, ilqr, models, zo):
    B, T = args.batch, args.T
    x0, ug = quad_problem(B, T, torch, models)
    traced, reg = models.TracedModel(zo.quad_euler_step(0.1), 12, 4), models.QuadcopterEuler(0.1)
    t = traced.tape
    emit(part="a", what="tape of the traced quadcopter", instructions=len(t.code), constants=len(t.consts), slots=t.n_slots, mask=hex(t.mask))
    for name, solve, R in (("iLQR", ilqr.iterativeLqr, 1.0), ("DDP", ilqr.differentialDynamicProgramming, 0.2)):
        cost = models.QuadraticCost(np.eye(12), R * np.eye(4), 10 * np.eye(12))
        times, res = alternate({"registered QuadcopterEuler": lambda: solve(reg, cost, cost, x0, ug),
                                "TracedModel(quad_euler_step)": lambda: solve(traced, cost, cost, x0, ug)}, args.reps, torch.cuda.synchronize)
        for k in times:
            emit(part="a", workload=f"{name} quadcopter n=12 m=4 T={T} batch={B} fp64", model=k,
                 converged_frac=float(res[k][3].double().mean().item()), **stats(times[k]))
        a, b = (np.median(times[k]) for k in ("TracedModel(quad_euler_step)", "registered QuadcopterEuler"))
        Ja, Jb = res["TracedModel(quad_euler_step)"][2], res["registered QuadcopterEuler"][2]
        fin = torch.isfinite(Ja) & torch.isfinite(Jb)
        emit(part="a", workload=name, traced_over_registered=float(a / b),
             max_rel_J_difference=float(((Ja[fin] - Jb[fin]).abs() / Jb[fin].abs()).max().item()))


def part_b(args, torch, ilqr, models):
    T, Bt = args.T, args.torch_batch
    for name, f, n, m, Q, R, Qf, scale in (("cart-pole", cartpole_any, 4, 1, np.diag([1.0, 10.0, 0.1, 0.1]), 0.01 * np.eye(1), 10 * np.eye(4), 0.3),
                                           ("car", car_any, 4, 2, np.diag([1.0, 1.0, 0.1, 0.1]), 0.1 * np.eye(2), 10 * np.eye(4), 1.0)):
        cost = models.QuadraticCost(Q, R, Qf)
        traced = models.TracedModel(f, n, m)
        rng = np.random.default_rng(5)
        dev = dict(dtype=torch.float64, device="cuda")
        x0 = torch.as_tensor(scale * rng.standard_normal((args.batch, n)), **dev)
        ug = torch.zeros((args.batch, T, m), **dev)
        for solver, solve in (("iLQR", ilqr.iterativeLqr), ("DDP", ilqr.differentialDynamicProgramming)):
            kw = dict(maxIter=args.max_iter)
            times, res = alternate({"traced": lambda: solve(traced, cost, cost, x0, ug, **kw)}, args.reps, torch.cuda.synchronize)
            emit(part="b", workload=f"{solver} {name} n={n} m={m} T={T} batch={args.batch}", path="TracedModel",
                 converged_frac=float(res["traced"][3].double().mean().item()), **stats(times["traced"]))
            xs, us = x0[:Bt].contiguous(), ug[:Bt].contiguous()
            times, res = alternate({"TracedModel": lambda: solve(traced, cost, cost, xs, us, **kw),
                                    "torch callable (generic.py)": lambda: solve(f, cost.runningCost, cost.terminalCost, xs, us, **kw)},
                                   args.torch_reps, torch.cuda.synchronize)
            for k in times:
                emit(part="b", workload=f"{solver} {name} n={n} m={m} T={T} batch={Bt}", path=k,
                     converged_frac=float(res[k][3].double().mean().item()), **stats(times[k]))
            emit(part="b", workload=f"{solver} {name} batch={Bt}",
                 torch_over_traced=float(np.median(times["torch callable (generic.py)"]) / np.median(times["TracedModel"])))


def event_ms(torch, f, reps):
    f()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def linesearch_problem(B, T, torch, models):
    rng = np.random.default_rng(9)
    dev = dict(dtype=torch.float64, device="cuda")
    x0, ug = quad_problem(B, T, torch, models)
    l = torch.as_tensor(0.1 * rng.standard_normal((B, T, 4)), **dev)
    L = torch.as_tensor(0.01 * rng.standard_normal((B, T, 4, 12)), **dev)
    xp = torch.zeros((B, T + 1, 12), **dev)
    xp[:] = x0[:, None, :]
    return x0, l, L, xp, ug


def part_c_child(args, torch, ilqr, models, pt, zo):
    """the 16-way line search of the traced quadcopter, slot file in LDS and in scratch, alternated (the -DZM_LAB library)"""
    B, T = args.batch, args.T
    x0, l, L, xp, up = linesearch_problem(B, T, torch, models)
    traced = models.TracedModel(zo.quad_euler_step(0.1), 12, 4)
    cost = models.QuadraticCost(np.eye(12), np.eye(4), 10 * np.eye(12))
    pol, prev = pt.AffinePolicy(l, L), pt.Trajectory(xp, up)
    times = {"lds": [], "scratch": []}
    ref = {}
    for r in range(args.reps + 1):
        for k in ("lds", "scratch"):
            os.environ["ZOPT_AMD_TRACED_SLOTS"] = k
            ms = event_ms(torch, lambda: ilqr.forwardPass2(x0, traced, cost, pol, prev), 1)
            ref[k] = ilqr.forwardPass2(x0, traced, cost, pol, prev)[1]
            if r:
                times[k] += ms
    a, b = ref["lds"], ref["scratch"]
    assert bool(((a == b) | (a.isnan() & b.isnan())).all())          # the same costs bit for bit (a diverged rollout: NaN both ways)
    for k in times:
        emit(part="c", kernel=f"traced_rollout_kernel<16>, slot file in {k}", workload=f"forwardPass2 traced quadcopter T={T} batch={B}",
             note="device events around the call (uploads excluded: device tensors in)", **stats(times[k]))
    emit(part="c", scratch_over_lds=float(np.median(times["scratch"]) / np.median(times["lds"])))


def part_c(args, torch, ilqr, models, pt, zo):
    B, T = args.batch, args.T
    x0, l, L, xp, up = linesearch_problem(B, T, torch, models)
    traced, reg = models.TracedModel(zo.quad_euler_step(0.1), 12, 4), models.QuadcopterEuler(0.1)
    cost = models.QuadraticCost(np.eye(12), np.eye(4), 10 * np.eye(12))
    pol, prev = pt.AffinePolicy(l, L), pt.Trajectory(xp, up)
    for k, md in (("registered quadcopter (four-lane fast kernel)", reg), ("traced quadcopter (product: LDS slot file)", traced)):
        emit(part="c", kernel="16-way line search", model=k, workload=f"forwardPass2 T={T} batch={B}",
             **stats(event_ms(torch, lambda: ilqr.forwardPass2(x0, md, cost, pol, prev), args.reps)))
    Be = args.expand_batch
    traj = pt.Trajectory(xp[:Be].contiguous(), up[:Be].contiguous())
    for k, md in (("registered quadcopter (closed forms)", reg), ("traced quadcopter (tape on Dual / Hyper)", traced)):
        emit(part="c", kernel="first-order expansion", model=k, workload=f"AffineDynamics.from_trajectory T={T} batch={Be}",
             note="includes the output allocations", **stats(event_ms(torch, lambda: pt.AffineDynamics.from_trajectory(md, traj), args.reps)))
        emit(part="c", kernel="first- and second-order expansion, full tensors", model=k,
             workload=f"QuadraticDynamics.from_trajectory T={T} batch={Be}", note="includes the output allocations",
             **stats(event_ms(torch, lambda: pt.QuadraticDynamics.from_trajectory(md, traj), args.reps)))


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch-batch", type=int, default=256)
    ap.add_argument("--torch-reps", type=int, default=2)
    ap.add_argument("--expand-batch", type=int, default=1024)
    ap.add_argument("--max-iter", type=int, default=50)
    ap.add_argument("--only", default="abc")
    ap.add_argument("--out", default=None)
    ap.add_argument("--slots-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    OUT = args.out
    import torch
    from oracle import zopt_oracle as zo          # (the oracle's quadcopter callable is the subject of (a); the product never imports it)
    from zopt_amd import _lib, ilqrUtils, models, pytrees
    if args.slots_child:
        return part_c_child(args, torch, ilqrUtils, models, pytrees, zo)
    if OUT and os.path.exists(OUT):
        os.remove(OUT)
    emit(tool="tools/bench_traced_model.py", device=torch.cuda.get_device_name(0), args={k: v for k, v in vars(args).items() if k not in ("out", "slots_child")})
    if "a" in args.only:
        part_a(args, torch, ilqrUtils, models, zo)
    if "b" in args.only:
        part_b(args, torch, ilqrUtils, models)
    if "c" in args.only:
        part_c(args, torch, ilqrUtils, models, pytrees, zo)
        torch.cuda.synchronize()
        env = dict(os.environ, ZOPT_AMD_LIB=_lib.LAB_LIB_PATH)
        cmd = [sys.executable, os.path.abspath(__file__), "--slots-child", "--batch", str(args.batch), "--T", str(args.T), "--reps", str(args.reps)]
        subprocess.run(cmd + (["--out", OUT] if OUT else []), env=env, check=True)


if __name__ == "__main__":
    main()
