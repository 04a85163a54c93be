#!/usr/bin/env python3
"""Host-layer identity of the LQR family between two trees (GPU needed): runs a fixed set of tiny cases from fixed seeds through whichever
`zopt_amd` is first on the path -- every function of lqrUtils and simulateProportionalFeedback, at shapes that reach every dispatch
branch behind them -- and writes every output to one .npz; two such files are then compared array by array, bit for bit (NaN positions
included, dtypes and shapes too) by tools/ilqr_host_identity.py's `compare`.

    PYTHONPATH=<parent tree> python tools/lqr_host_identity.py --out parent.npz
    PYTHONPATH=.             python tools/lqr_host_identity.py --out branch.npz
    python tools/lqr_host_identity.py --compare parent.npz branch.npz
    PYTHONPATH=<tree> python tools/lqr_host_identity.py --time     # 200 back-to-back NumPy calls of four entries: us per call
"""
import argparse
import json
import sys
import time

import numpy as np

from ilqr_host_identity import _put, compare

B3 = (3,)


def _spd(rng, lead, k):
    M = rng.standard_normal(lead + (k, k))
    return M @ np.swapaxes(M, -1, -2) / k + np.eye(k)


def sweep_operands(rng, lead, T, n, m):
    """time-varying (A, B, Q, R) of a finite-horizon problem"""
    s = lead + (T,)
    return (np.eye(n) + 0.1 * rng.standard_normal(s + (n, n)), rng.standard_normal(s + (n, m)), _spd(rng, s, n), _spd(rng, s, m))


def affine_operands(rng, lead, T, n, m):
    """(A, B, d, Q, R, H, q, r, q0) of bilinearAffineLqr"""
    s = lead + (T,)
    A, B, Q, R = sweep_operands(rng, lead, T, n, m)
    return (A, B, 0.1 * rng.standard_normal(s + (n,)), Q, R, 0.1 * rng.standard_normal(s + (m, n)), rng.standard_normal(s + (n,)),
            rng.standard_normal(s + (m,)), rng.standard_normal(s))


def design(rng, lead, n, m, radius=0.8):
    """(A, B, Q, R) of an infinite-horizon design; A scaled to the spectral radius `radius` (discrete: the value iteration converges
    in a few hundred steps; continuous: any A has a stabilising solution with these B)"""
    A = rng.standard_normal(lead + (n, n))
    A *= radius / np.max(np.abs(np.linalg.eigvals(A)), axis=-1)[..., None, None]
    return A, rng.standard_normal(lead + (n, m)), _spd(rng, lead, n), _spd(rng, lead, m)


def run_cases():
    import torch
    from zopt_amd import lqrUtils as lqr
    from zopt_amd import models, simulator
    out = {}
    rng = np.random.default_rng(23)
    dev = lambda a, dt=None: torch.as_tensor(a, dtype=dt, device="cuda")   # noqa: E731

    # ---- discreteFiniteHorizonLqr, fp64: the register kernels at run-time KS = 1, 2, 3 and the compile-time (4, 1), the ring shapes,
    # the tile kernels up to (64, 16) exact; every horizon of the tail peel and of the ring's phases
    for n, m in ((4, 1), (3, 2), (7, 3), (11, 4), (8, 4), (12, 4), (13, 3), (24, 8), (40, 5), (50, 7), (64, 16)):
        for T in (1, 2, 3, 7):
            ops = sweep_operands(rng, B3, T, n, m)
            _put(out, f"dfh.f64.{n}x{m}.T{T}", lqr.discreteFiniteHorizonLqr(*ops, T))
    for n, m in ((12, 4), (24, 8)):
        ops = sweep_operands(rng, (2, 3), 3, n, m)
        _put(out, f"dfh.f64.{n}x{m}.lead23", lqr.discreteFiniteHorizonLqr(*ops, 3))
        _put(out, f"dfh.f64.{n}x{m}.empty", lqr.discreteFiniteHorizonLqr(*[a[:0] for a in ops], 3))
        _put(out, f"dfh.f64.{n}x{m}.carry", lqr.discreteFiniteHorizonLqr(*sweep_operands(rng, B3, 7, n, m), 5))
    _put(out, "dfh.f64.4x1.carry", lqr.discreteFiniteHorizonLqr(*sweep_operands(rng, B3, 7, 4, 1), 5))
    # (12, 4) as torch views that start one double into a flat buffer: not 16-byte aligned, so the register kernel serves them
    views = []
    for a in sweep_operands(rng, B3, 7, 12, 4):
        flat = torch.zeros(a.size + 1, dtype=torch.float64, device="cuda")
        flat[1:] = dev(a).reshape(-1)
        views.append(flat[1:].view(a.shape))
    assert all(v.data_ptr() % 16 == 8 and v.is_contiguous() for v in views)
    _put(out, "dfh.f64.12x4.unaligned", lqr.discreteFiniteHorizonLqr(*views, 7))

    # ---- fp32, NumPy and torch: fp32 storage on the ring, fp64 with one rounding at (5, 2), the fp32 tiles
    for n, m in ((12, 4), (8, 4), (5, 2), (20, 5), (64, 16)):
        ops = [a.astype(np.float32) for a in sweep_operands(rng, B3, 7, n, m)]
        _put(out, f"dfh.f32.np.{n}x{m}", lqr.discreteFiniteHorizonLqr(*ops, 7))
        _put(out, f"dfh.f32.torch.{n}x{m}", lqr.discreteFiniteHorizonLqr(*[dev(a) for a in ops], 7))
        _put(out, f"dfh.f32.np.{n}x{m}.carry", lqr.discreteFiniteHorizonLqr(*ops, 5))
    _put(out, "dfh.f32.np.empty", lqr.discreteFiniteHorizonLqr(*[a[:0].astype(np.float32) for a in sweep_operands(rng, B3, 3, 8, 4)], 3))

    # ---- bilinearAffineLqr
    for n, m in ((5, 2), (8, 4), (12, 4), (20, 5)):
        _put(out, f"affine.{n}x{m}", lqr.bilinearAffineLqr(*affine_operands(rng, B3, 7, n, m), 7))
    ops = affine_operands(rng, (2, 3), 7, 8, 4)
    _put(out, "affine.8x4.lead23.carry", lqr.bilinearAffineLqr(*ops, 5))
    _put(out, "affine.8x4.empty", lqr.bilinearAffineLqr(*[a[:0] for a in ops], 5))
    _put(out, "affine.8x4.f32", lqr.bilinearAffineLqr(*[a.astype(np.float32) for a in ops], 7))
    _put(out, "affine.8x4.f32.torch", lqr.bilinearAffineLqr(*[dev(a, torch.float32) for a in ops], 7))

    # ---- discreteInfiniteHorizonLqr
    for n, m in ((4, 2), (7, 3), (12, 4), (16, 4), (40, 8)):
        ops = design(rng, B3, n, m)
        _put(out, f"dare.{n}x{m}", lqr.discreteInfiniteHorizonLqr(*ops))
        _put(out, f"dare.{n}x{m}.value", lqr.discreteInfiniteHorizonLqr(*ops, return_value=True))
    ops = design(rng, (2, 3), 4, 2)
    _put(out, "dare.4x2.lead23.capped", lqr.discreteInfiniteHorizonLqr(*ops, maxIter=5, return_value=True))
    _put(out, "dare.4x2.empty", lqr.discreteInfiniteHorizonLqr(*[a[:0] for a in ops], return_value=True))
    _put(out, "dare.4x2.f32", lqr.discreteInfiniteHorizonLqr(*[a.astype(np.float32) for a in ops], tol=1e-9, return_value=True))

    # ---- infiniteHorizonLqr, infiniteHorizonIntegralLqr
    for n, m in ((4, 2), (16, 16)):
        ops = design(rng, B3, n, m, radius=1.0)
        _put(out, f"care.{n}x{m}", lqr.infiniteHorizonLqr(*ops))
        _put(out, f"care.{n}x{m}.value", lqr.infiniteHorizonLqr(*ops, return_value=True))
    ops = design(rng, (2, 3), 4, 2, radius=1.0)
    _put(out, "care.4x2.lead23", lqr.infiniteHorizonLqr(*ops, return_value=True))
    _put(out, "care.4x2.empty", lqr.infiniteHorizonLqr(*[a[:0] for a in ops], return_value=True))
    _put(out, "care.4x2.f32.torch", lqr.infiniteHorizonLqr(*[dev(a, torch.float32) for a in ops], return_value=True))
    A, B, Q, R = design(rng, B3, 13, 3, radius=1.0)    # as many inputs as integral states: the integrators are stabilisable
    _put(out, "care.integral.13+3", lqr.infiniteHorizonIntegralLqr(A, B, Q, R, _spd(rng, B3, 3), rng.standard_normal(B3 + (3, 13))))
    A, B, Q, R = design(rng, B3, 4, 2, radius=1.0)
    _put(out, "care.integral.1d", lqr.infiniteHorizonIntegralLqr(A, B, Q, R, _spd(rng, B3, 1), rng.standard_normal(B3 + (4,))))

    # ---- finiteHorizonLqr: constant coefficients, time-varying ones with refinement, an explicit n_samples
    A, B, Q, R = design(rng, B3, 4, 2, radius=1.0)
    A1 = 0.3 * rng.standard_normal((4, 4))
    Ri, Qf = np.linalg.inv(R), _spd(rng, B3, 4)
    const = (lambda t: A, lambda t: B, lambda t: Q, lambda t: Ri)
    vary = (lambda t: A + np.sin(3.0 * t) * A1, lambda t: B, lambda t: (1.0 + 0.5 * t) * Q, lambda t: Ri)
    for key, coef, kw in (("const", const, dict(N=5)), ("vary", vary, dict(N=5, max_refinements=2)), ("samples", vary, dict(N=4, n_samples=9))):
        K = lqr.finiteHorizonLqr(*coef, Qf, 1.5, **kw)
        _put(out, f"fh.{key}", (K.t, K.V, K.info, np.asarray(K.n_samples), np.asarray(K.coef_change), K(0.0), K(0.4), K(1.5)))

    # ---- simulateProportionalFeedback with a constant and with a time-indexed gain
    n, m, T = 4, 2, 6
    Am, Bm = np.eye(n) + 0.1 * rng.standard_normal((n, n)), rng.standard_normal((n, m))
    model = models.LinearModel(Am, Bm)
    x0, xTrim, uTrim = rng.standard_normal(B3 + (n,)), 0.1 * rng.standard_normal(n), 0.1 * rng.standard_normal(m)
    tile = lambda M: np.broadcast_to(M, B3 + M.shape).copy()   # noqa: E731
    Kc = lqr.discreteInfiniteHorizonLqr(tile(Am), tile(Bm), _spd(rng, B3, n), _spd(rng, B3, m))
    _put(out, "sim.constant", simulator.simulateProportionalFeedback(model, x0, Kc, xTrim, uTrim, N=T))
    tileT = lambda M: np.broadcast_to(M, B3 + (T,) + M.shape).copy()   # noqa: E731
    Kt = lqr.discreteFiniteHorizonLqr(tileT(Am), tileT(Bm), _spd(rng, B3 + (T,), n), _spd(rng, B3 + (T,), m), T)
    _put(out, "sim.indexed", simulator.simulateProportionalFeedback(model, x0, Kt, xTrim, uTrim))
    _put(out, "sim.indexed.N4", simulator.simulateProportionalFeedback(model, x0, Kt, xTrim, uTrim, N=4))
    return out


def time_loop(calls):
    """`calls` back-to-back NumPy-in / NumPy-out calls of four entries at batch 5 (the host-bound case): us per call"""
    from zopt_amd import lqrUtils as lqr
    rng = np.random.default_rng(23)
    lead = (5,)
    dfh = sweep_operands(rng, lead, 7, 12, 4)
    aff = affine_operands(rng, lead, 7, 8, 4)
    des = design(rng, lead, 4, 2)
    fams = {"discreteFiniteHorizonLqr": lambda: lqr.discreteFiniteHorizonLqr(*dfh, 7),
            "bilinearAffineLqr": lambda: lqr.bilinearAffineLqr(*aff, 7),
            "discreteInfiniteHorizonLqr": lambda: lqr.discreteInfiniteHorizonLqr(*des),
            "infiniteHorizonLqr": lambda: lqr.infiniteHorizonLqr(*des)}
    row = {}
    for fam, fn in fams.items():
        for _ in range(20):
            fn()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        row[fam] = (time.perf_counter() - t0) / calls * 1e6
    print(json.dumps({"host_loop_us_per_call": row, "calls": calls}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="run the cases and write every output to this .npz")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"), help="compare two such files")
    ap.add_argument("--time", action="store_true", help="the host-bound loop: us per call of four entries at batch 5")
    ap.add_argument("--calls", type=int, default=200)
    args = ap.parse_args()
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
