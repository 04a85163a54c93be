"""References for models.TracedConstraint: the host build of the constraint interpreter (tests/tape_con_shim.cpp around
zopt_amd/csrc/tape_con.h) and a NumPy restatement of the augmented-Lagrangian iLQR on recorded constraints, built from the pieces of
tests/ilqr_state_ref.py (pos, the outer loop's rule), tests/ilqr_tracking_ref.py (cost, expansions) and the oracle (rollouts,
conditioning, backward pass), as tests/ilqr_state_ref.py is.

Rows: g(x_k, u_k, p) for k = 0..N-1 (n_con values each; stage 0 included) and terminal(x_N, p) (n_con_terminal values).  With
pos(s) = s > 0 ? s : 0 (a NaN gives 0):
    s_i = lam_i + mu g_i,   psi_i = (pos(s_i)^2 - lam_i^2) / (2 mu)
    J_AL = J_cost + P,  P = sum of psi_i in an accumulator of its own: k ascending, i ascending, the terminal rows last, added once
    expansion: c_x[k] += G_x^T pos(s), c_u[k] += G_u^T pos(s), v_x += G_T^T pos(s_T); the conditioned [c_xx c_ux^T; c_ux c_uu][k] +=
               mu G^T diag(s > 0) G, the conditioned v_xx += the same of the terminal rows (Gauss-Newton: no second derivatives of g)
    outer loop: inner iLQR on J_AL from the stored inputs with policy (u, L = 0); viol = max(0, max g) over every row, NaN if any g is;
                done = inner converged and viol <= ctol; else, if another outer iteration follows, lam <- pos(s), mu <- min(mu growth, mu_max)
One trajectory per call, as the oracle.  g is the callable itself on float64 arrays; G comes from the tape on float64 dual numbers
(tests/tape_ref.py), or on long double with `ld_jacobian` (the expansion test's reference).
"""
import ctypes
import os
import subprocess

import numpy as np

from oracle import zopt_oracle as zo
from tests import ilqr_state_ref as sref
from tests import ilqr_tracking_ref as tref
from tests import tape_ref as R
from zopt_amd import tape as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
pos = sref.pos


# ---- host build of the interpreter ------------------------------------------------------------------------------------------------
def build(outdir):
    """Compile tests/tape_con_shim.cpp against the tree's headers, as tests/traced_cost_ref.py builds its shim; returns the library."""
    outdir = str(outdir)
    os.makedirs(os.path.join(outdir, "stub", "hip"), exist_ok=True)
    open(os.path.join(outdir, "stub", "hip", "hip_runtime.h"), "w").close()
    so = os.path.join(outdir, "tape_con_shim.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", R.HEADER_DIR,
                    "-I", os.path.join(outdir, "stub"), "-o", so, os.path.join(ROOT, "tests", "tape_con_shim.cpp")], check=True)
    lib = ctypes.CDLL(so)
    vp, dp, ci = ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.c_int
    # (blob, n_instr, n_const, n_slots, n, m, np, nc, controls, x, u, p, p_stride, P, out)
    for fn in (lib.con_value, lib.con_jacobian):
        fn.argtypes = [vp, ci, ci, ci, ci, ci, ci, ci, ci, dp, dp, vp, ctypes.c_long, ctypes.c_long, dp]
        fn.restype = None
    lib.con_psi.argtypes = [dp, dp, dp, ctypes.c_long, dp]
    lib.con_psi.restype = None
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
    fn(blob.ctypes.data, len(tape.code), len(tape.consts), tape.n_slots, tape.n, tape.m, tape.n_params, len(tape.outputs),
       1 if controls else 0, x.ctypes.data_as(dp), u.ctypes.data_as(dp), None if pp is None else pp.ctypes.data, stride, P,
       out.ctypes.data_as(dp))
    return out


def host_value(lib, tape, x, u=None, p=None):
    """g (P, n_out) by the host build on double; u = None: a terminal tape"""
    return _host(lib.con_value, tape, u is not None, x, u, p, (len(tape.outputs),))


def host_jacobian(lib, tape, x, u=None, p=None):
    """G (P, n_out, n + m) by the host build on Dual"""
    return _host(lib.con_jacobian, tape, u is not None, x, u, p, (len(tape.outputs), tape.n + tape.m))


def host_psi(lib, g, lam, mu):
    """psi, elementwise, by the host build of the kernels' own function"""
    g, lam, mu = (np.ascontiguousarray(np.broadcast_arrays(g, lam, mu)[i], dtype=np.float64) for i in range(3))
    out = np.empty(g.shape)
    dp = ctypes.POINTER(ctypes.c_double)
    lib.con_psi(g.ctypes.data_as(dp), lam.ctypes.data_as(dp), mu.ctypes.data_as(dp), g.size, out.ctypes.data_as(dp))
    return out


# ---- a recorded constraint for the restatement -----------------------------------------------------------------------------------------
class RefCon:
    """The callables of a zopt_amd.models.TracedConstraint and their tapes; p: the parameter row of the trajectory at hand."""

    def __init__(self, con):
        self.con, self.n, self.m, self.nc, self.nct = con, con.n, con.m, con.n_con, con.n_con_terminal

    def g(self, x, u, p=None):
        """(n_con,) float64: the callable itself"""
        if not self.nc:
            return np.zeros(0)
        with np.errstate(all="ignore"):
            return np.asarray(self.con._g(x, u, p) if self.con.n_params else self.con._g(x, u), dtype=np.float64).reshape(-1)

    def gT(self, x, p=None):
        if not self.nct:
            return np.zeros(0)
        with np.errstate(all="ignore"):
            return np.asarray(self.con._terminal(x, p) if self.con.n_params else self.con._terminal(x), dtype=np.float64).reshape(-1)

    def rows(self, traj, p=None):
        """(g (N, n_con), gT (n_con_terminal,)) along a trajectory"""
        xT, uT = traj
        N = uT.shape[0]
        g = np.stack([self.g(xT[k], uT[k], p) for k in range(N)]) if self.nc else np.zeros((N, 0))
        return g, self.gT(xT[N], p)

    def jacobians(self, traj, p=None, dtype=np.float64):
        """(G (N, n_con, n + m), GT (n_con_terminal, n)) by dual numbers of `dtype` on the tapes"""
        xT, uT = (np.asarray(t, dtype=dtype) for t in traj)
        N = uT.shape[0]
        pp = None if p is None else np.asarray(p, dtype=dtype)
        with np.errstate(all="ignore"):
            G = R.jacobian(self.con.stage_tape, xT[:N], uT, pp, dtype)[1] if self.nc else np.zeros((N, 0, self.n + self.m), dtype=dtype)
            GT = (R.jacobian(self.con.terminal_tape, xT[N:], np.zeros((1, self.m), dtype=dtype), pp, dtype)[1][0, :, :self.n]
                  if self.nct else np.zeros((0, self.n), dtype=dtype))
        return G, GT


def penalty(g, gT, lam, lamT, mu):
    """P: the stage rows k ascending, i ascending, then the terminal rows; every operation rounded on its own (the kernels' con_psi)"""
    P = 0.0
    with np.errstate(all="ignore"):
        for k in range(g.shape[0]):
            for i in range(g.shape[1]):
                p = float(pos(lam[k, i] + mu * g[k, i]))
                P = P + (p * p - lam[k, i] * lam[k, i]) / (2.0 * mu)
        for i in range(gT.shape[0]):
            p = float(pos(lamT[i] + mu * gT[i]))
            P = P + (p * p - lamT[i] * lamT[i]) / (2.0 * mu)
    return P


def addends(g, G, lam, mu):
    """(gradient addend (..., K), Hessian addend (..., K, K)) of rows g (..., nc) with Jacobians G (..., nc, K)"""
    with np.errstate(all="ignore"):
        s = lam + mu * g
        a = (s > 0).astype(G.dtype)
    w = pos(s).astype(G.dtype)
    grad = np.einsum("...i,...ij->...j", w, G)
    H = mu * np.einsum("...i,...ij,...ik->...jk", a, G, G)
    return grad, H


def violation(g, gT):
    allg = np.concatenate([g.ravel(), gT.ravel()])
    if np.isnan(allg).any():
        return float("nan")
    return float(max(0.0, np.max(allg))) if allg.size else 0.0


def forward_pass(x0, dynFun, Q, R_, Qf, xr, ur, policy, trajPrev, rc, p, pen):
    """the 16-way search on J_AL -> (traj, J_AL, J_cost, index, the 16 J_AL)"""
    lam, lamT, mu = pen
    Js, Jcs, trajs = [], [], []
    with np.errstate(all="ignore"):
        for alpha in zo.LINESEARCH_ALPHAS:
            t = zo.trajectoryRollout(x0, dynFun, policy, trajPrev, alpha=alpha)
            trajs.append(t)
            Jc = tref.trajectory_cost(Q, R_, Qf, xr, ur, t)
            Jcs.append(Jc)
            Js.append(Jc + penalty(*rc.rows(t, p), lam, lamT, mu))
    idx = int(np.argmin(np.asarray(Js)))
    return trajs[idx], Js[idx], Jcs[idx], idx, np.asarray(Js)


def expansion(dynFun, Q, R_, Qf, xr, ur, traj, rc, p, pen):
    """(AffineDynamics, QuadraticCostFunction, QuadraticValueFunction) of J_AL along traj: the conditioned cost expansion plus the
    penalty's addends"""
    lam, lamT, mu = pen
    n = rc.n
    N = traj.uTraj.shape[0]
    dyn = zo.affine_dynamics_from_trajectory(dynFun, traj)
    cost = zo.conditionQuadraticCost(tref.cost_expansion(Q, R_, xr, ur, traj))
    Vf = zo.conditionValueFunction(tref.terminal_expansion(Qf, xr, traj.xTraj[-1]))
    g, gT = rc.rows(traj, p)
    G, GT = rc.jacobians(traj, p)
    grad, H = addends(g, G, lam, mu)
    gradT, HT = addends(gT, GT, lamT, mu)
    cost = cost._replace(c_x=cost.c_x + grad[:, :n], c_u=cost.c_u + grad[:, n:], c_xx=cost.c_xx + H[:, :n, :n],
                         c_ux=cost.c_ux + H[:, n:, :n], c_uu=cost.c_uu + H[:, n:, n:])
    Vf = Vf._replace(v_x=Vf.v_x + gradT, v_xx=Vf.v_xx + HT)
    return dyn, cost, Vf


def inner_solve(dynFun, Q, R_, Qf, xr, ur, x0, uStart, rc, p, pen, maxIter, tol, trace=None):
    """tests/ilqr_tracking_ref.iterativeLqr on J_AL -> (traj, L, J_AL, J_cost, converged, iterations); `trace` receives per iteration
    dict(J, Jcost, idx, Js, dJ)"""
    n = x0.shape[0]
    N, m = uStart.shape
    lam, lamT, mu = pen
    policy = zo.AffinePolicy(uStart, np.zeros((N, m, n)))
    prev = zo.Trajectory(np.zeros((N + 1, n)), np.zeros((N, m)))
    with np.errstate(all="ignore"):
        traj = zo.trajectoryRollout(x0, dynFun, policy, prev)
        Jc = tref.trajectory_cost(Q, R_, Qf, xr, ur, traj)
    J = Jc + penalty(*rc.rows(traj, p), lam, lamT, mu)
    converged, it = False, 0
    while (not converged) and it < maxIter:
        dyn, cost, Vf = expansion(dynFun, Q, R_, Qf, xr, ur, traj, rc, p, pen)
        policy = zo.backwardPass_ilqr(dyn, cost, Vf)
        traj_new, J_new, Jc_new, idx, Js = forward_pass(x0, dynFun, Q, R_, Qf, xr, ur, policy, traj, rc, p, pen)
        if trace is not None:
            trace.append(dict(J=J_new, Jcost=Jc_new, idx=idx, Js=Js, dJ=abs(J - J_new)))
        converged = bool(abs(J - J_new) <= tol)
        traj, J, Jc = traj_new, J_new, Jc_new
        it += 1
    return traj, policy.L, J, Jc, converged, it


def constrainedIterativeLqr(dynFun, Q, R_, Qf, x0, uGuess, con, p=None, xr=None, ur=None, maxIter=100, tol=1e-3, trace=None):
    """`con`: a zopt_amd.models.TracedConstraint (its callables, tapes and settings mu0, growth, mu_max, outer, ctol); p: its parameter
    row for this trajectory.  -> dict(traj, L, J (plain cost), converged (done), violation, mu, lam, lam_terminal, outer (iterations
    run), inner (list of the inner-iteration counts)).  `trace` receives per outer iteration dict(inner=[per-iteration dicts], violation,
    mu (the one the inner solve ran with), converged (the inner solve's))."""
    import warnings
    Q, R_, Qf = (np.asarray(t, dtype=np.float64) for t in (Q, R_, Qf))
    x0, uGuess = np.asarray(x0, dtype=np.float64), np.asarray(uGuess, dtype=np.float64)
    n = x0.shape[0]
    N, m = uGuess.shape
    rc = RefCon(con)
    xr = np.zeros((N + 1, n)) if xr is None else xr
    ur = np.zeros((N, m)) if ur is None else ur
    lam, lamT, mu = np.zeros((N, rc.nc)), np.zeros(rc.nct), float(con.mu0)
    u, inner, done, ran = uGuess, [], False, 0
    traj = L = Jc = viol = None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for j in range(con.outer):
            itr = [] if trace is not None else None
            traj, L, _, Jc, conv, its = inner_solve(dynFun, Q, R_, Qf, xr, ur, x0, u, rc, p, (lam, lamT, mu), maxIter, tol, itr)
            inner.append(its)
            g, gT = rc.rows(traj, p)
            viol = violation(g, gT)
            if trace is not None:
                trace.append(dict(inner=itr, violation=viol, mu=mu, converged=conv))
            ran = j + 1
            done = bool(conv and viol <= con.ctol)
            if done:
                break
            if j + 1 < con.outer:
                with np.errstate(all="ignore"):
                    lam, lamT = pos(lam + mu * g), pos(lamT + mu * gT)
                mu = min(mu * con.growth, con.mu_max)
            u = traj.uTraj
    return dict(traj=traj, L=L, J=Jc, converged=done, violation=viol, mu=mu, lam=lam, lam_terminal=lamT, outer=ran, inner=inner)


def min_gap(out):
    """the smallest relative gap between the best two of the 16 costs over every iteration of a traced run (the rule of
    tests/test_ilqr_state_gpu.py)"""
    gap = np.inf
    for o in out["trace"]:
        for it in o["inner"]:
            Js = np.sort(it["Js"])
            gap = min(gap, (Js[1] - Js[0]) / max(abs(Js[0]), 1e-300))
    return gap
