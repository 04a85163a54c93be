#!/usr/bin/env python3
"""What stage-varying input bounds cost the fused box solves, and what carrying them costs the constant form: the workload of
tools/bench_ilqr_box.py (8192 quadcopters, T = 100, a TrackingCost about hover with a goal per trajectory, thrust within uTrim +- 2,
moments within +- 0.05), iLQR and DDP, solved by
  * the parent commit's library, twice (`parent a`, `parent b`: two runs of the same code -- their difference is the spread the
    constant form is held to).  It is the library ZOPT_AMD_LIB names; without ZOPT_AMD_LIB the two runs are left out;
  * this tree's library with InputBox(model, lb, ub) (`constant`);
  * this tree's library with the same bounds as (T, m) rows, InputBox(..., stage_varying=True) (`stage`): the same problem and, bit
    for bit, the same iterates, so the ratio is the cost of the stage kernels alone.
All in one process, alternated, so that clock and thermal drift hit all alike.  A struct with the trailing step_stride is passed to
both libraries; the parent reads its first three fields.

    ZOPT_AMD_LIB=/path/to/parent/libzopt_amd.so python tools/bench_ilqr_box_stage.py --reps 7
    rocprofv3 --kernel-trace --stats ... -- python tools/bench_ilqr_box_stage.py --reps 3 --own-only     # the per-kernel split
--full-weights puts one off-diagonal pair into Q: the fast line search then runs its general-weights instantiation (the one that
spills), the rest of the solve is unchanged in kind.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _load(path):
    from zopt_amd import _lib
    handle = ctypes.CDLL(path)
    for name, (res, args) in _lib.SYMBOLS.items():
        fn = getattr(handle, name)
        fn.restype = res
        fn.argtypes = args
    return handle


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--own-only", action="store_true", help="this tree's library alone (for a kernel trace)")
    ap.add_argument("--full-weights", action="store_true", help="Q with an off-diagonal pair: the general-weights line search")
    args = ap.parse_args()
    import torch
    from zopt_amd import _lib, ilqrUtils, models
    own_path = os.path.join(_lib.CSRC, "libzopt_amd.so")
    parent = None
    if os.environ.get("ZOPT_AMD_LIB") and not args.own_only:
        parent = _lib.lib()                                     # the library ZOPT_AMD_LIB names
        own = _load(own_path)
    else:
        own = _lib.lib()
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
    Q = np.eye(12)
    if args.full_weights:
        Q[0, 1] = Q[1, 0] = 1e-3
    cost = models.TrackingCost(Q, np.eye(4), 10 * np.eye(12), goal[:, None, :], uTrim)
    model = models.QuadcopterEuler(0.1)
    lim = np.array([2.0, 0.05, 0.05, 0.05])
    const = models.InputBox(model, uTrim - lim, uTrim + lim)
    stage = models.InputBox(model, np.tile(uTrim - lim, (T, 1)), np.tile(uTrim + lim, (T, 1)), stage_varying=True)
    variants = {"constant": (own, const), "stage": (own, stage)}
    if parent is not None:
        variants = {"parent a": (parent, const), "constant": (own, const), "stage": (own, stage), "parent b": (parent, const)}

    def solve(handle, box, ddp):
        _lib._lib = handle                                      # every call of the drivers goes through _lib.lib()
        fn = ilqrUtils.differentialDynamicProgramming if ddp else ilqrUtils.iterativeLqr
        out = fn(box, cost, cost, tx0, tug)
        torch.cuda.synchronize()
        return out

    for ddp in (False, True):
        res = {}
        for h, box in variants.values():                        # warm-up at the timed shape
            solve(h, box, ddp)
        times = {k: [] for k in variants}
        for _ in range(args.reps):                              # alternated
            for k, (h, box) in variants.items():
                t0 = time.perf_counter()
                res[k] = solve(h, box, ddp)
                times[k].append((time.perf_counter() - t0) * 1e3)
        name = "differentialDynamicProgramming" if ddp else "iterativeLqr"
        for k in variants:
            traj, _, J, conv = res[k]
            print(json.dumps({"workload": f"{name} quadcopter n=12 m=4 T={T} batch={B} fp64, TrackingCost about hover, thrust uTrim +- 2, "
                                          "moments +- 0.05" + (", Q with an off-diagonal pair" if args.full_weights else ""), "variant": k, "reps": args.reps, "solve_ms_median": float(np.median(times[k])),
                              "solve_ms_min": min(times[k]), "solve_ms_max": max(times[k]),
                              "converged_frac": float(conv.double().mean().item()), "J_mean_finite": float(J[torch.isfinite(J)].mean().item())}))
        med = {k: float(np.median(v)) for k, v in times.items()}
        bits = lambda t: t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t      # noqa: E731  (NaN rows compare as bits)
        same = lambda a, b: all(torch.equal(bits(x), bits(y)) for x, y in ((res[a][0].xTraj, res[b][0].xTraj), (res[a][0].uTraj, res[b][0].uTraj),      # noqa: E731
                                                                (res[a][1], res[b][1]), (res[a][3], res[b][3])))
        line = {"solver": name, "stage_over_constant_median": med["stage"] / med["constant"], "stage_bits_equal_constant": same("stage", "constant")}
        if parent is not None:
            pm = 0.5 * (med["parent a"] + med["parent b"])
            line.update(parent_spread_ms=abs(med["parent a"] - med["parent b"]), constant_minus_parent_ms=med["constant"] - pm,
                        constant_over_parent_median=med["constant"] / pm, constant_bits_equal_parent=same("constant", "parent a"))
        print(json.dumps(line))


if __name__ == "__main__":
    main()
