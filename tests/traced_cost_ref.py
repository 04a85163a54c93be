"""References for models.TracedCost: the host build of the cost interpreter (tests/tape_cost_shim.cpp around
zopt_amd/csrc/tape_cost.h), long-double / sympy expansions of a cost callable, and a NumPy restatement of the iLQR and DDP loops for cost
callables built from the oracle's pieces (zo.forwardPass2, zo.conditionQuadraticCost, zo.conditionValueFunction, zo.backwardPass_ilqr /
_ddp, zo.affine_dynamics_from_trajectory).  The cost expansions of the restatement come from the tape on long-double dual numbers
(tests/tape_ref.py) and from sympy derivatives of the expression the callable builds, evaluated in long double.
"""
import ctypes
import os
import subprocess

import numpy as np

from oracle import zopt_oracle as zo
from tests import tape_ref as R
from zopt_amd import tape as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble


# ---- host build of the interpreter ------------------------------------------------------------------------------------------------
def build(outdir):
    """Compile tests/tape_cost_shim.cpp against the tree's headers, as tests/tape_ref.py builds its shim; returns the loaded library."""
    outdir = str(outdir)
    os.makedirs(os.path.join(outdir, "stub", "hip"), exist_ok=True)
    open(os.path.join(outdir, "stub", "hip", "hip_runtime.h"), "w").close()
    so = os.path.join(outdir, "tape_cost_shim.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", R.HEADER_DIR,
                    "-I", os.path.join(outdir, "stub"), "-o", so, os.path.join(ROOT, "tests", "tape_cost_shim.cpp")], check=True)
    lib = ctypes.CDLL(so)
    vp, dp, ci = ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.c_int
    # (blob, n_instr, n_const, n_slots, n, m, np, controls, x, u, p, p_stride, P, out)
    for fn in (lib.cost_value, lib.cost_gradient, lib.cost_hessian):
        fn.argtypes = [vp, ci, ci, ci, ci, ci, ci, ci, dp, dp, vp, ctypes.c_long, ctypes.c_long, dp]
        fn.restype = None
    return lib


def _host(fn, tape, controls, x, u, p, width):
    x = np.ascontiguousarray(np.atleast_2d(x), dtype=np.float64)
    P = x.shape[0]
    u = np.zeros((P, tape.m)) if u is None else np.ascontiguousarray(np.atleast_2d(u), dtype=np.float64)
    blob = np.ascontiguousarray(T.blob(tape))
    stride, pp = 0, None
    if tape.n_params:
        pp = np.ascontiguousarray(np.atleast_2d(p), dtype=np.float64)
        stride = tape.n_params if pp.shape[0] == P and P > 1 else 0
    out = np.empty((P,) + width)
    dp = ctypes.POINTER(ctypes.c_double)
    fn(blob.ctypes.data, len(tape.code), len(tape.consts), tape.n_slots, tape.n, tape.m, tape.n_params, 1 if controls else 0,
       x.ctypes.data_as(dp), u.ctypes.data_as(dp), None if pp is None else pp.ctypes.data, stride, P, out.ctypes.data_as(dp))
    return out


def host_value(lib, tape, x, u=None, p=None):
    """c (P) by the host build on double; u = None: a terminal tape"""
    return _host(lib.cost_value, tape, u is not None, x, u, p, ())


def host_gradient(lib, tape, x, u=None, p=None):
    """[c_x | c_u] (P, n + m) by the host build on Dual"""
    return _host(lib.cost_gradient, tape, u is not None, x, u, p, (tape.n + tape.m,))


def host_hessian(lib, tape, x, u=None, p=None):
    """(P, n + m, n + m) by the host build on Hyper"""
    return _host(lib.cost_hessian, tape, u is not None, x, u, p, (tape.n + tape.m, tape.n + tape.m))


def host_cost_of_trajectory(lib, cost, xTraj, uTraj, p=None):
    """J (b) of trajectories (b, N + 1, n), (b, N, m): the host interpreter's per-step costs summed in step order from 0.0, then the
    terminal cost -- the line search's arithmetic"""
    b, N = uTraj.shape[:2]
    J = np.zeros(b)
    with np.errstate(all="ignore"):
        for k in range(N):
            J = J + host_value(lib, cost.running_tape, xTraj[:, k], uTraj[:, k], p)
        return J + host_value(lib, cost.terminal_tape, xTraj[:, N], None, p)


# ---- long-double / sympy expansions of a scalar callable ------------------------------------------------------------------------------
def tape_value_ld(tape, x, u=None, p=None, dtype=LD):
    x = np.atleast_2d(np.asarray(x, dtype=dtype))
    u = np.zeros((len(x), tape.m), dtype=dtype) if u is None else np.atleast_2d(np.asarray(u, dtype=dtype))
    return R.evaluate(tape, x, u, None if p is None else np.asarray(p, dtype=dtype), R.Real(dtype))[:, 0]


def tape_gradient_ld(tape, x, u=None, p=None, dtype=LD):
    """(c (P), [c_x | c_u] (P, n + m)) of a cost tape by dual numbers of `dtype`"""
    x = np.atleast_2d(np.asarray(x, dtype=dtype))
    u = np.zeros((len(x), tape.m), dtype=dtype) if u is None else np.atleast_2d(np.asarray(u, dtype=dtype))
    f, J = R.jacobian(tape, x, u, None if p is None else np.asarray(p, dtype=dtype), dtype)
    return f[:, 0], J[:, 0, :]


class SymbolicSecond:
    """Second derivatives of the expression a NumPy callable builds, by sympy, lambdified once and evaluated in long double.  The
    callable is f(x, u[, p]) (controls) or f(x[, p]) and returns `n_out` values (a scalar counts as one)."""

    def __init__(self, f, n, m, n_params=0, controls=True):
        import sympy
        self.n, self.m, self.np, self.controls = n, m, n_params, controls
        z = sympy.symbols(f"z0:{n + m}", real=True)
        q = sympy.symbols(f"q0:{max(n_params, 1)}", real=True)
        box = lambda a: np.array([R._Sym(v) for v in a] + [None], dtype=object)[:-1]          # noqa: E731
        args = ((box(z[:n]), box(z[n:])) if controls else (box(z[:n]),)) + ((box(q[:n_params]),) if n_params else ())
        out = np.asarray(f(*args), dtype=object).reshape(-1)
        self.exprs = [o.e if isinstance(o, R._Sym) else sympy.sympify(float(o)) for o in out]
        self.syms = tuple(z) + tuple(q[:n_params])
        K = n + m
        self.entries = []
        for i, e in enumerate(self.exprs):
            for a in range(K):
                for b in range(a, K):
                    d = sympy.diff(e, z[a], z[b])
                    if d != 0:
                        self.entries.append((i, a, b, sympy.lambdify(self.syms, d, modules="numpy")))

    def pattern(self):
        """(n_out, K, K) bool: the entries whose derivative is not identically zero"""
        K = self.n + self.m
        S = np.zeros((len(self.exprs), K, K), dtype=bool)
        for i, a, b, _ in self.entries:
            S[i, a, b] = S[i, b, a] = True
        return S

    def __call__(self, x, u=None, p=None, dtype=LD):
        """H (P, n_out, K, K) in long double (or `dtype`: the fp64 evaluation of the same derivative expressions)"""
        x = np.atleast_2d(np.asarray(x, dtype=dtype))
        P = len(x)
        u = np.zeros((P, self.m), dtype=dtype) if u is None else np.atleast_2d(np.asarray(u, dtype=dtype))
        cols = [x[:, k] for k in range(self.n)] + [u[:, k] for k in range(self.m)]
        if self.np:
            pp = np.broadcast_to(np.atleast_2d(np.asarray(p, dtype=dtype)), (P, self.np))
            cols += [pp[:, k] for k in range(self.np)]
        K = self.n + self.m
        H = np.zeros((P, len(self.exprs), K, K), dtype=dtype)
        with np.errstate(all="ignore"):
            for i, a, b, fn in self.entries:
                H[:, i, a, b] = H[:, i, b, a] = fn(*cols)
        return H


class RefCost:
    """A recorded cost for the restatement: the callables, their tapes (dual numbers) and their sympy second derivatives.
    `cost`: a zopt_amd.models.TracedCost."""

    def __init__(self, cost):
        self.cost, self.n, self.m, self.np = cost, cost.n, cost.m, cost.n_params
        self.h_run = SymbolicSecond(cost._running, cost.n, cost.m, cost.n_params, True)
        self.h_term = SymbolicSecond(cost._terminal, cost.n, cost.m, cost.n_params, False)

    def running(self, p=None):
        return (lambda x, u: self.cost._running(x, u, p)) if self.np else self.cost._running

    def terminal(self, p=None):
        return (lambda x: self.cost._terminal(x, p)) if self.np else self.cost._terminal

    def expand(self, traj, p=None):
        """(QuadraticCostFunction along traj, QuadraticValueFunction at its last state) in fp64, from the long-double references"""
        n, m = self.n, self.m
        xT, uT = (np.asarray(t, dtype=np.float64) for t in traj)
        c, g = tape_gradient_ld(self.cost.running_tape, xT[:-1], uT, p)
        H = self.h_run(xT[:-1], uT, p)[:, 0]
        v, gv = tape_gradient_ld(self.cost.terminal_tape, xT[-1:], None, p)
        Hv = self.h_term(xT[-1:], None, p)[0, 0]
        f = lambda a: np.asarray(a, dtype=np.float64)                                          # noqa: E731
        qc = zo.QuadraticCostFunction(f(c), f(g[:, :n]), f(g[:, n:]), f(H[:, :n, :n]), f(H[:, n:, :n]), f(H[:, n:, n:]))
        return qc, zo.QuadraticValueFunction(f(v[0]), f(gv[0, :n]), f(Hv[:n, :n]))


def solve(dynFun, ref_cost, x0, uGuess, p=None, maxIter=100, tol=1e-3, ddp=False, quadratic_dynamics=None, trace=None, projected=None):
    """The loop of reference ilqrUtils.py:290-327 (ddp: :360-397) for one trajectory with cost callables.  dynFun(x, u): NumPy, analytic
    (complex-step Jacobians); quadratic_dynamics(traj) -> zo.QuadraticDynamics for ddp; p: the cost's parameter row.  trace (a list)
    receives per iteration (J_new, winning step index, the 16 costs); projected (a list) receives per iteration whether a PD projection
    changed a cost or terminal Hessian by more than 1e-9 of its scale.  Returns (Trajectory, L, J, converged, iterations)."""
    x0 = np.asarray(x0, dtype=np.float64)
    uGuess = np.asarray(uGuess, dtype=np.float64)
    n = x0.shape[0]
    N, m = uGuess.shape
    rc, tc = ref_cost.running(p), ref_cost.terminal(p)
    policy = zo.AffinePolicy(uGuess, np.zeros((N, m, n)))
    traj = zo.trajectoryRollout(x0, dynFun, policy, zo.Trajectory(np.zeros((N + 1, n)), np.zeros((N, m))))
    J = zo.trajectoryCost(rc, tc, traj)
    converged, it = False, 0
    while (not converged) and it < maxIter:
        dyn = quadratic_dynamics(traj) if ddp else zo.affine_dynamics_from_trajectory(dynFun, traj)
        raw, rawV = ref_cost.expand(traj, p)
        cost, Vf = zo.conditionQuadraticCost(raw), zo.conditionValueFunction(rawV)
        if projected is not None:
            moved = lambda a, b: np.max(np.abs(a - b)) > 1e-9 * max(1.0, np.max(np.abs(a)))   # noqa: E731
            projected.append(bool(moved(raw.c_xx, cost.c_xx) or moved(raw.c_uu, cost.c_uu) or moved(raw.c_ux, cost.c_ux) or
                                  moved(rawV.v_xx, Vf.v_xx)))
        policy = (zo.backwardPass_ddp if ddp else zo.backwardPass_ilqr)(dyn, cost, Vf)
        traj_new, J_new, idx, Js = zo.forwardPass2(x0, dynFun, rc, tc, policy, traj, return_index=True)
        if trace is not None:
            trace.append((J_new, idx, Js))
        converged = bool(abs(J - J_new) <= tol)
        traj, J = traj_new, J_new
        it += 1
    return traj, policy.L, J, converged, it


def symbolic_quadratic_dynamics(f, n, m):
    """quadratic_dynamics(traj) for `solve` from sympy second derivatives of the dynamics callable f(x, u) (fp64 values, complex-step
    Jacobians)"""
    second = SymbolicSecond(f, n, m)

    def expand(traj):
        a = zo.affine_dynamics_from_trajectory(f, traj)
        xT, uT = traj
        H = np.asarray(second(xT[:-1], uT), dtype=np.float64)
        return zo.QuadraticDynamics(a.f, a.f_x, a.f_u, H[:, :, :n, :n], H[:, :, n:, :n], H[:, :, n:, n:])
    return expand


def agreement(J_gpu, a_gpu, trace, rtol=1e-9):
    """the rule of tests/test_ilqr_tracking_gpu.py: leading iterations in which the kernel's cost after the acceptance step (to `rtol`,
    NaN == NaN) and its winning step-size index (exactly) agree with the restatement's"""
    k = 0
    for (Jo, idx, _), Jg, ag in zip(trace, J_gpu, a_gpu):
        same_J = (np.isnan(Jo) and np.isnan(Jg)) or (Jo == Jg) or (np.isfinite(Jo) and np.isfinite(Jg) and abs(Jo - Jg) <= rtol * abs(Jo))
        if not (same_J and int(ag) == idx):
            break
        k += 1
    return k
