#!/usr/bin/env python3
"""Host-layer identity of the iLQR / DDP drivers between two trees (GPU needed): runs a fixed set of small cases from fixed seeds
through whichever `zopt_amd` is first on the path and writes every output to one .npz; two such files are then compared array by
array, bit for bit (NaN positions included, dtypes too).

    PYTHONPATH=<parent tree> python tools/ilqr_host_identity.py --out parent.npz
    PYTHONPATH=.             python tools/ilqr_host_identity.py --out branch.npz
    python tools/ilqr_host_identity.py --compare parent.npz branch.npz
    ... --out x.npz --fallback                                     # the same cases on the product's fallback kernels
    ZOPT_AMD_LIB=<another build of the library> ... --out x.npz    # two builds of the kernels under one host layer
    PYTHONPATH=<tree> python tools/ilqr_host_identity.py --time     # 200 back-to-back calls of the small linear solve per family: us per call
"""
import argparse
import json
import os
import sys
import time

import numpy as np


def _spd(rng, lead, k):
    M = rng.standard_normal(lead + (k, k))
    return M @ np.swapaxes(M, -1, -2) / k + np.eye(k)


def linear_case(rng, n=3, m=2, T=6, B=5):
    """n=3, m=2, T=6, batch 5 unless given: a stable-ish linear model, costs about the origin and about a reference"""
    from zopt_amd import models
    A = np.eye(n) + 0.1 * rng.standard_normal((n, n))
    Bm = rng.standard_normal((n, m))
    model = models.LinearModel(A, Bm)
    Q, R, Qf = _spd(rng, (), n), _spd(rng, (), m), 5 * _spd(rng, (), n)
    costs = {"quad": models.QuadraticCost(Q, R, Qf),
             "track": models.TrackingCost(Q, R, Qf, 0.3 * rng.standard_normal((B, T + 1, n)), 0.1 * rng.standard_normal(m))}
    x0 = rng.standard_normal((B, n))
    ug = 0.1 * rng.standard_normal((B, T, m))
    ibox = lambda mdl: models.InputBox(mdl, -0.4, 0.5)                           # noqa: E731
    sbox = lambda mdl: models.StateBox(mdl, -0.8 * np.ones(n), 0.9 * np.ones(n), outer=4)   # noqa: E731
    wrappers = {"none": model, "ibox": ibox(model), "sbox": sbox(model), "sbox_ibox": sbox(ibox(model))}
    return costs, wrappers, x0, ug


def quad_case(rng):
    """quadcopter (12, 4), T=8, batch 3"""
    from zopt_amd import models
    T, B = 8, 3
    model = models.QuadcopterEuler(0.1)
    uTrim = np.asarray(models.QuadcopterEuler.uTrim, dtype=np.float64)
    cost = models.QuadraticCost(np.eye(12), np.eye(4), 10 * np.eye(12))
    x0 = np.zeros((B, 12))
    x0[:, 9:12] = rng.uniform(-2, 2, (B, 3))
    ug = np.tile(uTrim, (B, T, 1)) + 0.05 * rng.standard_normal((B, T, 4))
    return cost, {"none": model, "ibox": models.InputBox(model, uTrim - [3, 0.2, 0.2, 0.2], uTrim + [3, 0.2, 0.2, 0.2])}, x0, ug


def sweep_operands(rng, lead, N, n, m):
    from zopt_amd.pytrees import QuadraticCostFunction, QuadraticDynamics, QuadraticValueFunction
    s = lead + (N,)
    dyn = QuadraticDynamics(rng.standard_normal(s + (n,)), np.eye(n) + 0.1 * rng.standard_normal(s + (n, n)), rng.standard_normal(s + (n, m)),
                            0.05 * rng.standard_normal(s + (n, n, n)), 0.05 * rng.standard_normal(s + (n, m, n)),
                            0.05 * rng.standard_normal(s + (n, m, m)))
    cost = QuadraticCostFunction(rng.standard_normal(s), rng.standard_normal(s + (n,)), rng.standard_normal(s + (m,)), _spd(rng, s, n),
                                 0.1 * rng.standard_normal(s + (m, n)), _spd(rng, s, m))
    Vf = QuadraticValueFunction(rng.standard_normal(lead), rng.standard_normal(lead + (n,)), _spd(rng, lead, n))
    return dyn, cost, Vf, 0.2 * rng.standard_normal(s + (m,))


def _np(x):
    if x is None:
        return np.zeros(0)
    if hasattr(x, "detach"):
        return x.detach().cpu().numpy()
    return np.asarray(x)


def _put(out, key, value):
    """flatten nested tuples of arrays under `key`"""
    if isinstance(value, tuple):
        for i, v in enumerate(tuple.__iter__(value)):
            _put(out, f"{key}.{i}", v)
    else:
        out[key] = _np(value)


def run_cases():
    import torch
    from zopt_amd import ilqrUtils, models
    from zopt_amd.pytrees import AffineDynamics, AffinePolicy, Trajectory
    out = {}

    def solve(key, fn, *args):
        for trace in (False, True):
            ilqrUtils._TRACE = [] if trace else None
            try:
                _put(out, f"{key}.trace{int(trace)}", fn(*args))
                for j, (name, val) in enumerate(ilqrUtils._TRACE or []):
                    out[f"{key}.trace1.T{j}.{name}"] = np.asarray(val)
            finally:
                ilqrUtils._TRACE = None

    rng = np.random.default_rng(11)
    costs, wrappers, x0, ug = linear_case(rng)
    for ck, cost in costs.items():
        for wk, w in wrappers.items():
            solve(f"linear.{ck}.{wk}.iterativeLqr", ilqrUtils.iterativeLqr, w, cost, cost, x0, ug, 20, 1e-6)
            if isinstance(w, models.StateBox):
                solve(f"linear.{ck}.{wk}.constrained", ilqrUtils.constrainedIterativeLqr, w, cost, cost, x0, ug, 20, 1e-6)
    # one empty batch
    solve("linear.empty.iterativeLqr", ilqrUtils.iterativeLqr, wrappers["none"], costs["quad"], costs["quad"], x0[:0], ug[:0])
    solve("linear.empty.constrained", ilqrUtils.constrainedIterativeLqr, wrappers["sbox"], costs["quad"], costs["quad"], x0[:0], ug[:0])
    # rollouts
    lin = wrappers["none"]
    n, m, T, B = lin.n, lin.m, ug.shape[1], ug.shape[0]
    pol = AffinePolicy(0.1 * rng.standard_normal((B, T, m)), 0.1 * rng.standard_normal((B, T, m, n)))
    prev = Trajectory(0.2 * rng.standard_normal((B, T + 1, n)), 0.2 * rng.standard_normal((B, T, m)))
    for wk, w, ck in (("none", lin, "quad"), ("ibox", wrappers["ibox"], "quad"), ("none", lin, "track")):
        _put(out, f"rollout.{wk}.{ck}.forwardPass2", ilqrUtils.forwardPass2(x0, w, costs[ck], pol, prev))
        _put(out, f"rollout.{wk}.{ck}.trajectoryRollout", ilqrUtils.trajectoryRollout(x0, w, pol, prev, 0.5))

    qcost, qwrap, qx0, qug = quad_case(rng)
    for wk, w in qwrap.items():
        solve(f"quad.{wk}.iterativeLqr", ilqrUtils.iterativeLqr, w, qcost, qcost, qx0, qug, 10, 1e-4)
        solve(f"quad.{wk}.ddp", ilqrUtils.differentialDynamicProgramming, w, qcost, qcost, qx0, qug, 10, 1e-4)

    # sweeps and steps, NumPy fp64 in and torch fp32 in
    for shape, (lead, N, n, m) in {"linear": ((5,), 6, 3, 2), "quad": ((3,), 8, 12, 4)}.items():
        dyn, cost, Vf, uT = sweep_operands(rng, lead, N, n, m)
        f32 = lambda t: type(t)(*[torch.as_tensor(np.asarray(a), dtype=torch.float32, device="cuda") for a in tuple.__iter__(t)])   # noqa: E731
        for fam, conv in (("np64", lambda t: t), ("torch32", f32)):
            d, c, v = conv(dyn), conv(cost), conv(Vf)
            u = uT if fam == "np64" else torch.as_tensor(uT, dtype=torch.float32, device="cuda")
            aff = AffineDynamics(*list(tuple.__iter__(d))[:3])
            key = f"sweep.{shape}.{fam}"
            _put(out, f"{key}.backwardPass_ilqr", ilqrUtils.backwardPass_ilqr(aff, c, v))
            _put(out, f"{key}.backwardPass_ilqr_box", ilqrUtils.backwardPass_ilqr_box(aff, c, v, u, -0.3, 0.4))
            _put(out, f"{key}.backwardPass_ddp", ilqrUtils.backwardPass_ddp(d, c, v))
            _put(out, f"{key}.backwardPass_ddp_box", ilqrUtils.backwardPass_ddp_box(d, c, v, u, -0.3, 0.4))
            step = lambda t: type(t)(*[a[:, 0] for a in tuple.__iter__(t)])   # noqa: E731  (one time step, batch axis kept)
            _put(out, f"{key}.riccatiStep_ilqr", ilqrUtils.riccatiStep_ilqr(step(aff), step(c), v))
            _put(out, f"{key}.riccatiStep_ddp", ilqrUtils.riccatiStep_ddp(step(d), step(c), v))
    kernel_cases(out, rng)
    return out


def kernel_cases(out, rng):
    """Every instantiation of the sweep, line-search and expansion kernels (ilqr_backward.hip, rollout*.hip, linearize.hip, traced.hip)
    at least once.  With --fallback the (12, 4) cases run the register-prefetch sweep and the generic line search instead of the
    LDS-ring sweep and the fast line search."""
    from zopt_amd import ilqrUtils, lqrUtils, models
    from zopt_amd.pytrees import AffineDynamics, AffinePolicy, QuadraticCostFunction, Trajectory
    # sweeps: K-steps 1, 2, 3; T = 1..5 are the five ways through the prefetch loop's tail
    for n, m in ((3, 2), (6, 3), (12, 4)):
        for T in (1, 2, 3, 4, 5):
            dyn, cost, Vf, uT = sweep_operands(rng, (3,), T, n, m)
            aff = AffineDynamics(*list(tuple.__iter__(dyn))[:3])
            key = f"kernels.sweep.n{n}m{m}T{T}"
            _put(out, f"{key}.ilqr", ilqrUtils.backwardPass_ilqr(aff, cost, Vf))
            _put(out, f"{key}.affine", lqrUtils.bilinearAffineLqr(dyn.f_x, dyn.f_u, dyn.f, cost.c_xx, cost.c_uu, cost.c_ux, cost.c_x, cost.c_u,
                                                                  cost.c, T))
            _put(out, f"{key}.ilqr_box", ilqrUtils.backwardPass_ilqr_box(aff, cost, Vf, uT, -0.3, 0.4))
            _put(out, f"{key}.ddp", ilqrUtils.backwardPass_ddp(dyn, cost, Vf))
            _put(out, f"{key}.ddp_box", ilqrUtils.backwardPass_ddp_box(dyn, cost, Vf, uT, -0.3, 0.4))
    # the penalty sweeps (with and without the input box) and the penalty line search: state-box solves at K-steps 2 and 3
    for n, m in ((6, 3), (12, 4)):
        costs, wrappers, x0, ug = linear_case(rng, n, m)
        for wk in ("sbox", "sbox_ibox"):
            _put(out, f"kernels.constrained.n{n}m{m}.{wk}", ilqrUtils.constrainedIterativeLqr(wrappers[wk], costs["quad"], costs["quad"], x0, ug, 10, 1e-6))
    # line search: 1, 3 and 16 step sizes (1, 4 and 16 lanes per trajectory), 70 trajectories (no multiple of the 4, 16, 64 per wave),
    # trajectory 7 starts at NaN (every cost NaN: the argmin's NaN branch)
    B, T = 70, 6
    for name, (n, m) in (("lin", (3, 2)), ("lin12", (12, 4)), ("quad", (12, 4)), ("traced", (3, 2))):
        costs, wrappers, _, _ = linear_case(rng, n, m, B=B, T=T)
        if name == "quad":
            wrappers = {"none": models.QuadcopterEuler(0.1)}
            wrappers["ibox"] = models.InputBox(wrappers["none"], -0.4, 0.5)
        if name == "traced":
            Am, Bm = np.eye(n) + 0.1 * rng.standard_normal((n, n)), rng.standard_normal((n, m))
            step = lambda x, u: np.array([sum(Am[i, j] * x[j] for j in range(n)) + sum(Bm[i, j] * u[j] for j in range(m))   # noqa: E731
                                          + 0.01 * np.sin(x[i]) for i in range(n)])
            wrappers = {"none": models.TracedModel(step, n, m)}
            costs = {"quad": costs["quad"]}
        x0 = rng.standard_normal((B, n))
        x0[7] = np.nan
        pol = AffinePolicy(0.1 * rng.standard_normal((B, T, m)), 0.1 * rng.standard_normal((B, T, m, n)))
        prev = Trajectory(0.2 * rng.standard_normal((B, T + 1, n)), 0.2 * rng.standard_normal((B, T, m)))
        for wk in ("none", "ibox"):
            for ck, cost in costs.items():
                if wk in wrappers:
                    for na, alphas in ((1, [0.5]), (3, [1.0, 0.5, 0.25]), (16, ilqrUtils.LINESEARCH_ALPHAS)):
                        _put(out, f"kernels.linesearch.{name}.{wk}.{ck}.na{na}", ilqrUtils._rollout(x0, wrappers[wk], pol, prev, alphas, cost))
    # expansions: a generic model and the quadcopter in still air and wind, with and without a reference; the solves above and below run
    # the fused (cost) forms, the from_trajectory calls the plain ones
    for name, model in (("lin", linear_case(rng)[1]["none"]), ("still", models.QuadcopterEuler(0.1)),
                        ("wind", models.QuadcopterEuler(0.1, (1.0, -0.5, 0.2)))):
        n, m, B, T = model.n, model.m, 3, 5
        traj = Trajectory(0.3 * rng.standard_normal((B, T + 1, n)), 0.3 * rng.standard_normal((B, T, m)))
        Q, R, Qf = _spd(rng, (), n), _spd(rng, (), m), _spd(rng, (), n)
        costs = {"quad": models.QuadraticCost(Q, R, Qf), "diag": models.QuadraticCost(np.diag(np.diag(Q)), np.diag(np.diag(R)), np.diag(np.diag(Qf))),
                 "track": models.TrackingCost(Q, R, Qf, 0.3 * rng.standard_normal((B, T + 1, n)), 0.1 * rng.standard_normal(m))}
        _put(out, f"kernels.expand.{name}.affine", AffineDynamics.from_trajectory(model, traj))
        for ck, cost in costs.items():
            _put(out, f"kernels.expand.{name}.{ck}.cost", QuadraticCostFunction.from_trajectory(cost, traj))
            if name != "lin":
                x0 = np.zeros((B, 12))
                x0[:, 9:12] = rng.uniform(-1, 1, (B, 3))
                ug = np.tile(np.asarray(models.QuadcopterEuler.uTrim, dtype=np.float64), (B, T, 1)) + 0.05 * rng.standard_normal((B, T, 4))
                _put(out, f"kernels.expand.{name}.{ck}.iterativeLqr", ilqrUtils.iterativeLqr(model, cost, cost, x0, ug, 4, 1e-4))
                _put(out, f"kernels.expand.{name}.{ck}.ddp", ilqrUtils.differentialDynamicProgramming(model, cost, cost, x0, ug, 4, 1e-4))


def compare(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    bad = 0
    for k in sorted(set(a.files) | set(b.files)):
        if k not in a.files or k not in b.files:
            verdict = "MISSING in " + (a_path if k not in a.files else b_path)
        else:
            x, y = a[k], b[k]
            same = x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y, equal_nan=x.dtype.kind == "f") and \
                (x.dtype.kind != "f" or np.array_equal(np.isnan(x), np.isnan(y)))
            verdict = "equal" if same else f"DIFFERENT ({x.dtype}{x.shape} vs {y.dtype}{y.shape})"
        bad += verdict != "equal"
        print(f"{verdict:9s} {k}" + (f"  {a[k].dtype}{a[k].shape} nan={int(np.isnan(a[k]).sum()) if a[k].dtype.kind == 'f' else 0}" if verdict == "equal" else ""))
    print(f"{len(set(a.files) | set(b.files))} arrays compared, {bad} not equal")
    return 1 if bad else 0


def time_loop(calls):
    """`calls` back-to-back calls of the small linear solve per family, NumPy in and out (the host-bound case): us per call"""
    from zopt_amd import ilqrUtils, models
    rng = np.random.default_rng(11)
    costs, wrappers, x0, ug = linear_case(rng)
    fams = {"plain": ("quad", "none"), "tracking": ("track", "none"), "box": ("quad", "ibox"), "state": ("quad", "sbox")}
    row = {}
    for fam, (ck, wk) in fams.items():
        w, cost = wrappers[wk], costs[ck]
        fn = ilqrUtils.constrainedIterativeLqr if isinstance(w, models.StateBox) else ilqrUtils.iterativeLqr
        for _ in range(20):
            fn(w, cost, cost, x0, ug, 20, 1e-6)
        t0 = time.perf_counter()
        for _ in range(calls):
            fn(w, cost, cost, x0, ug, 20, 1e-6)
        row[fam] = (time.perf_counter() - t0) / calls * 1e6
    print(json.dumps({"host_loop_us_per_call": row, "calls": calls}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="run the cases and write every output to this .npz")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"), help="compare two such files")
    ap.add_argument("--time", action="store_true", help="the host-bound loop: us per call of the small linear solve, per family")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--fallback", action="store_true", help="run the cases on the product's fallback kernels (ZOPT_AMD_ILQR_PATH=reg, "
                                                            "ZOPT_AMD_ROLLOUT_PATH=generic): the (12, 4) shapes then reach the register-prefetch "
                                                            "sweep and the generic line search")
    args = ap.parse_args()
    if args.fallback:   # read once per process by the library
        os.environ.update(ZOPT_AMD_ILQR_PATH="reg", ZOPT_AMD_ROLLOUT_PATH="generic")
    if args.compare:
        return compare(*args.compare)
    if args.time:
        return time_loop(args.calls)
    if not args.out:
        ap.error("one of --out, --compare, --time")
    import zopt_amd
    out = run_cases()
    np.savez(args.out, **out)
    print(f"{len(out)} arrays from {zopt_amd.__file__} -> {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
