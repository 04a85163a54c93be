"""NumPy restatement of the iLQR loop with a tracking cost (support code of tests/test_ilqr_tracking*.py).

    J = sum_{k<T} (x_k - xr_k)'Q(x_k - xr_k) + (u_k - ur_k)'R(u_k - ur_k)  +  (x_T - xr_T)'Qf(x_T - xr_T)            (no 1/2)

The loop is `oracle.zopt_oracle.iterativeLqr` (reference ilqrUtils.py:290-327) composed from the oracle's own pieces --
trajectoryRollout, jacobians (complex step), conditionQuadraticCost, conditionValueFunction, backwardPass_ilqr and the 16-way
argmin with NumPy's NaN rule -- with this file's tracking cost and gradients in place of the oracle's cost about the origin.  One
trajectory per call, as the oracle; xRef (T+1, n) and uRef (T, m) are full per-step arrays (`full_reference` builds them from the
layouts TrackingCost accepts)."""
import numpy as np

from oracle import zopt_oracle as zo


def full_reference(xRef, uRef, T, n, m, b=None):
    """(T+1, n), (T, m) arrays of trajectory `b` from None / (width,) / (..., steps, width) with broadcasting leading and step axes."""
    def one(r, rows, width):
        if r is None:
            return np.zeros((rows, width))
        r = np.asarray(r, dtype=np.float64)
        if r.ndim == 1:
            return np.tile(r, (rows, 1))
        if r.ndim > 2:
            lead = r.reshape((-1,) + r.shape[-2:])
            r = lead[0 if lead.shape[0] == 1 else b]
        return np.broadcast_to(r, (rows, width)).copy()
    return one(xRef, T + 1, n), one(uRef, T, m)


def running_cost(Q, R, xr, ur, k):
    """callable (x, u) -> cost of step k; works on complex arguments (complex-step derivative)"""
    return lambda x, u: (x - xr[k]) @ Q @ (x - xr[k]) + (u - ur[k]) @ R @ (u - ur[k])


def terminal_cost(Qf, xr):
    return lambda x: (x - xr[-1]) @ Qf @ (x - xr[-1])


def trajectory_cost(Q, R, Qf, xr, ur, traj):
    """CostFunction.__call__ (pytrees.py:49-52) with the stage index: the accumulation order of zo.trajectoryCost"""
    xT, uT = traj
    J = 0.0
    for k in range(uT.shape[0]):
        J = J + running_cost(Q, R, xr, ur, k)(xT[k], uT[k])
    return J + terminal_cost(Qf, xr)(xT[-1])


def cost_expansion(Q, R, xr, ur, traj):
    """QuadraticCostFunction.from_trajectory (pytrees.py:109-115) of the tracking cost"""
    xT, uT = traj
    N, n, m = uT.shape[0], xT.shape[1], uT.shape[1]
    ex, eu = xT[:-1] - xr[:-1], uT - ur
    c = np.einsum('ki,ij,kj->k', ex, Q, ex) + np.einsum('ki,ij,kj->k', eu, R, eu)
    return zo.QuadraticCostFunction(c, ex @ (Q + Q.T).T, eu @ (R + R.T).T, np.tile(Q + Q.T, (N, 1, 1)), np.zeros((N, m, n)),
                                    np.tile(R + R.T, (N, 1, 1)))


def terminal_expansion(Qf, xr, xf):
    """QuadraticValueFunction.fromTerminalCostFunction (pytrees.py:72-81) of the tracking cost"""
    e = xf - xr[-1]
    return zo.QuadraticValueFunction(e @ Qf @ e, (Qf + Qf.T) @ e, Qf + Qf.T)


def forward_pass(x0, dynFun, Q, R, Qf, xr, ur, policy, trajPrev):
    """forwardPass2 (ilqrUtils.py:116-150): 16 rollouts, argmin with NaN winning; -> (traj, J, index, the 16 costs)"""
    Js, trajs = [], []
    for alpha in zo.LINESEARCH_ALPHAS:
        t = zo.trajectoryRollout(x0, dynFun, policy, trajPrev, alpha=alpha)
        trajs.append(t)
        Js.append(trajectory_cost(Q, R, Qf, xr, ur, t))
    idx = int(np.argmin(np.asarray(Js)))
    return trajs[idx], Js[idx], idx, np.asarray(Js)


def iterativeLqr(dynFun, Q, R, Qf, xr, ur, x0, uGuess, maxIter=100, tol=1e-3, return_iters=False, trace=None):
    """zo.iterativeLqr with the tracking cost; `trace` receives (J_new, winning index, the 16 costs) per iteration, as there"""
    Q, R, Qf = (np.asarray(t, dtype=np.float64) for t in (Q, R, Qf))
    x0 = np.asarray(x0, dtype=np.float64)
    uGuess = np.asarray(uGuess, dtype=np.float64)
    n = x0.shape[0]
    N, m = uGuess.shape
    policy = zo.AffinePolicy(uGuess, np.zeros((N, m, n)))                                  # :293
    traj_prev = zo.Trajectory(np.zeros((N + 1, n)), np.zeros((N, m)))                       # :294
    traj = zo.trajectoryRollout(x0, dynFun, policy, traj_prev)                              # :297
    J = trajectory_cost(Q, R, Qf, xr, ur, traj)                                             # :298
    converged, it = False, 0
    while (not converged) and it < maxIter:                                                 # :301-303
        dyn = zo.affine_dynamics_from_trajectory(dynFun, traj)                              # :308
        cost = zo.conditionQuadraticCost(cost_expansion(Q, R, xr, ur, traj))                # :309, :312
        Vf = zo.conditionValueFunction(terminal_expansion(Qf, xr, traj.xTraj[-1]))          # :310, :313
        policy = zo.backwardPass_ilqr(dyn, cost, Vf)                                        # :315
        traj_new, J_new, idx, Js = forward_pass(x0, dynFun, Q, R, Qf, xr, ur, policy, traj)  # :316
        if trace is not None:
            trace.append((J_new, idx, Js))
        converged = bool(abs(J - J_new) <= tol)                                             # :318
        traj, J = traj_new, J_new
        it += 1
    out = (traj, policy.L, J, converged)
    return out + (it,) if return_iters else out
