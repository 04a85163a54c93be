"""Host build of zopt_amd/csrc/trig.h (tests/trig_shim.cpp), the argument set on which it is tested, and the multi-precision
reference -- shared by tests/test_sincos.py (CPU: the error contract against mpmath) and tests/test_sincos_gpu.py (GPU: every
consumer's device bits equal the host build's bits on the same arguments).

The contract (the header's own ulp figure plus its own neglected third term of pi/2), k = rint(2x/pi), |x| <= 1e6:

    |error| <= 1.4 ulp(result) + (|k| + 1) * 1.6e-33
"""
import ctypes
import functools
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "zopt_amd", "csrc")
MP_BITS = 400                       # working precision of the reference: ~290 bits below the 1.6e-33 term being measured
ULP_FACTOR, K_TERM = 1.4, 1.6e-33   # the contract


def build(outdir, header_dir=HEADER_DIR):
    """Compile tests/trig_shim.cpp against `header_dir`/trig.h (the tree's; a scratch copy for mutation checks) into `outdir`;
    returns the loaded library.  -ffp-contract=off: every FMA of the header is explicit, as its pragma demands of clang."""
    outdir = str(outdir)
    os.makedirs(os.path.join(outdir, "stub", "hip"), exist_ok=True)
    open(os.path.join(outdir, "stub", "hip", "hip_runtime.h"), "w").close()      # what the header includes; nothing of it is used
    so = os.path.join(outdir, "trig_shim.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", header_dir,
                    "-I", os.path.join(outdir, "stub"), "-o", so, os.path.join(ROOT, "tests", "trig_shim.cpp")], check=True)
    lib = ctypes.CDLL(so)
    dp = ctypes.POINTER(ctypes.c_double)
    lib.sc.argtypes = [dp, dp, dp, ctypes.c_long]
    lib.sc.restype = None
    lib.quad_step.argtypes = [dp, dp, ctypes.c_double, dp, ctypes.c_long]
    lib.quad_step.restype = None
    return lib


def sincos(lib, x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    s, c = np.empty_like(x), np.empty_like(x)
    dp = ctypes.POINTER(ctypes.c_double)
    lib.sc(x.ctypes.data_as(dp), s.ctypes.data_as(dp), c.ctypes.data_as(dp), x.size)
    return s, c


def quad_step(lib, x, u, dt):
    """x + dt inertialDynamics(x, u) in still air, rounded as the fast rollout kernels round it: x (P, 12), u (P, 4) -> (P, 12)"""
    x, u = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(u, dtype=np.float64)
    out = np.empty_like(x)
    dp = ctypes.POINTER(ctypes.c_double)
    lib.quad_step(x.ctypes.data_as(dp), u.ctypes.data_as(dp), float(dt), out.ctypes.data_as(dp), x.shape[0])
    return out


def _neighbours(x):
    x = np.asarray(x, dtype=np.float64)
    return np.concatenate([np.nextafter(x, -np.inf), x, np.nextafter(x, np.inf)])


@functools.lru_cache(maxsize=None)
def arguments():
    """{family: fp64 arguments}, seeded.  All finite, |x| <= 1e6: the domain of the contract."""
    import mpmath as mp
    rng = np.random.default_rng(20240611)
    fam = {}
    for name, a in (("uniform7", 7.0), ("uniform100", 100.0), ("uniform1e6", 1e6)):
        fam[name] = rng.uniform(-a, a, 4000)
    with mp.workprec(MP_BITS):
        hp = mp.pi / 2
        near = np.arange(-64, 65)
        far = rng.integers(-636000, 636001, 4000)
        # fl(k pi/2) and its two neighbours: the zeros of sin (k even) and cos (k odd), where the reduction's last bits are the result
        fam["zeros_small_k"] = _neighbours([float(int(k) * hp) for k in near])
        fam["zeros_large_k"] = _neighbours([float(int(k) * hp) for k in far])
        # (k + 1/2) pi/2: x * 2/pi sits on a rounding tie of rint, k goes either way, |r| = pi/4 is the edge of the kernels' interval
        fam["ties"] = _neighbours([float((int(k) + mp.mpf(1) / 2) * hp) for k in np.concatenate([near, far[:300]])])
    tiny = np.array([5e-324, 1e-320, 2.2250738585072014e-308, 2.2250738585072009e-308, 1e-300, 1e-160, 1.5e-154, 1e-100, 1e-30,
                     2.0 ** -27, 2.0 ** -26, 1e-8, 1e-5])
    fam["tiny"] = np.concatenate([tiny, -tiny, [0.0, -0.0]])
    edge = np.array([1e6, np.nextafter(1e6, 0.0), 999999.9, 999999.5, 999998.0, 636619.0 * (np.pi / 2), 999999.0])
    fam["under_1e6"] = np.concatenate([edge, -edge])
    for v in fam.values():
        assert np.all(np.isfinite(v)) and np.all(np.abs(v) <= 1e6)
    return fam


def all_arguments():
    return np.concatenate(list(arguments().values()))


SPECIALS = np.array([np.inf, -np.inf, np.nan])      # documented: NaN out


def contract_ratio(x, s, c):
    """max(|s - sin x|, |c - cos x|) / (1.4 ulp(result) + (|k| + 1) 1.6e-33) per argument, in MP_BITS-bit arithmetic; also the error
    in ulp of the exact result alone (to show where the ulp bound fails).  ulp(y): the spacing of fp64 at |y| (2^-1074 below the
    normal range).  k as the function itself forms it: rint of the fp64 product x * fl(2/pi)."""
    import mpmath as mp
    k = np.abs(np.rint(np.asarray(x) * 6.36619772367581382433e-01))
    ratio, ulps = np.empty(len(x)), np.empty(len(x))
    with mp.workprec(MP_BITS):
        tiniest = mp.ldexp(mp.mpf(1), -1074)
        for i, (xi, si, ci) in enumerate(zip(x.tolist(), s.tolist(), c.tolist())):
            r, u = mp.mpf(0), mp.mpf(0)
            for got, ref in ((si, mp.sin(mp.mpf(xi))), (ci, mp.cos(mp.mpf(xi)))):
                err = abs(mp.mpf(got) - ref)
                ulp = tiniest if ref == 0 else mp.ldexp(mp.mpf(1), max(mp.frexp(ref)[1] - 1, -1022) - 52)
                r = max(r, err / (ULP_FACTOR * ulp + (k[i] + 1) * mp.mpf(K_TERM)))
                u = max(u, err / ulp)
            ratio[i], ulps[i] = float(r), float(u)
    return ratio, ulps
