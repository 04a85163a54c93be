"""NumPy restatement of control-limited DDP (input box u_lb <= u <= u_ub on the DDP sweep; Tassa, Mansard, Todorov 2014): support code
of tests/test_ddp_box*.py, built on tests/hp_reference.py's DDP step and tests/ilqr_box_ref.py's box step.

    backward step:  Q_x, Q_u, Q_xx, Q_ux, Q_uu as the iLQR step forms them                                  (hp._sweep_ld)
                    vf_zz = sum_i v_x[i] d2f_i/dz2 stacked [[xx, ux'], [ux, uu]], P = its PD projection at eps = 1e-3
                    Q_xx += P[:n,:n],  Q_ux += P[n:,:n],  Q_uu += P[n:,n:]
                    then ilqr_box_ref.box_tail: the box-QP over lb - u_k <= d <= ub - u_k, L[C,:] = 0, v_x', v_xx'

fp64 (np.linalg.eigh, np.linalg.solve) or long double (hp.psd_project_ld, hp.solve_ld).  The products and the projection run over the
batch at once (a long-double eigensolve per step is what the reference costs); the box step enumerates active sets per trajectory."""
import numpy as np

from oracle import zopt_oracle as zo
from tests import hp_reference as hp
from tests import ilqr_box_ref as br
from tests import ilqr_tracking_ref as tref

LD = np.longdouble
_T = hp._T
_mv = hp._mv


def ddp_box_backward(dyn, cost, Vf, uTraj, lb, ub, ld=False, eps=1e-3, perturb=None):
    """The box DDP backward pass of a batch.  dyn = (f, f_x (B,T,n,n), f_u (B,T,n,m), f_xx (B,T,n,n,n), f_ux (B,T,n,m,n), f_uu
    (B,T,n,m,m)), cost = (c, c_x, c_u, c_xx, c_ux, c_uu), Vf = (v, v_x, v_xx), uTraj (B,T,m), lb / ub (m,) or (B,m).
    perturb = (rel, rng), as hp._sweep_ld takes it: a symmetric random matrix with largest entry rel * max|P| is added to every step's
    projected matrix P; rel may be an array (B,1,1).
    Returns dict(l (B,T,m), L (B,T,m,n), clamped (B,T) bit masks, margin (B,T))."""
    dt = LD if ld else np.float64
    f_x, f_u, f_xx, f_ux, f_uu = (np.asarray(t, dtype=dt) for t in dyn[1:6])
    c_x, c_u, c_xx, c_ux, c_uu = (np.asarray(t, dtype=dt) for t in cost[1:])
    v_x, v_xx = (np.asarray(t, dtype=dt) for t in Vf[1:])
    B, T, n, m = f_u.shape
    u = np.asarray(uTraj, dtype=dt)
    lb, ub = (np.broadcast_to(np.asarray(t, dtype=dt), (B, m)) for t in (lb, ub))
    out = {"l": np.empty((B, T, m), dtype=dt), "L": np.empty((B, T, m, n), dtype=dt), "clamped": np.zeros((B, T), dtype=np.int64),
           "margin": np.empty((B, T))}
    for k in range(T - 1, -1, -1):
        fx, fu = f_x[:, k], f_u[:, k]
        Q_x = c_x[:, k] + _mv(_T(fx), v_x)
        Q_u = c_u[:, k] + _mv(_T(fu), v_x)
        Q_xx = c_xx[:, k] + (_T(fx) @ v_xx) @ fx
        Q_uu = c_uu[:, k] + (_T(fu) @ v_xx) @ fu
        Q_ux = c_ux[:, k] + (_T(fu) @ v_xx) @ fx
        vf = [np.sum(v_x[:, :, None, None] * F[:, k], axis=-3) for F in (f_xx, f_ux, f_uu)]
        Z = np.concatenate([np.concatenate([vf[0], _T(vf[1])], axis=-1), np.concatenate([vf[1], vf[2]], axis=-1)], axis=-2)
        P = hp.psd_project_ld(Z, eps) if ld else zo.ensurePositiveDefinite(Z, eps)
        if perturb is not None:
            rel, rng = perturb
            E = rng.standard_normal(P.shape)
            E = E + _T(E)
            P = P + (E / np.max(np.abs(E), axis=(-1, -2), keepdims=True) * (rel * np.max(np.abs(P), axis=(-1, -2), keepdims=True))).astype(dt)
        Q_xx, Q_ux, Q_uu = Q_xx + P[:, :n, :n], Q_ux + P[:, n:, :n], Q_uu + P[:, n:, n:]
        v_x, v_xx = np.empty_like(v_x), np.empty_like(v_xx)
        for b in range(B):
            v_x[b], v_xx[b], l, L, mask, margin = br.box_tail(Q_x[b], Q_u[b], Q_xx[b], Q_uu[b], Q_ux[b], lb[b] - u[b, k], ub[b] - u[b, k], ld)
            out["l"][b, k], out["L"][b, k], out["clamped"][b, k], out["margin"][b, k] = l, L, mask, margin
    return out


def ddp_box_backward_with_reruns(dyn, cost, Vf, uTraj, lb, ub, rels, seed=12345):
    """The long-double pass and reruns of it with every projected matrix perturbed (hp.ddp_reference_and_sensitivity's scheme: the
    reruns are extra batch entries of one sweep).  rels: the relative sizes, one rerun each.  Returns (ref, [rerun, ...])."""
    B = np.asarray(uTraj).shape[0]
    k = len(rels) + 1
    rep = lambda t: tuple(None if x is None else np.concatenate([np.asarray(x)] * k, axis=0) for x in t)      # noqa: E731
    lbs, ubs = (np.concatenate([np.broadcast_to(np.asarray(t, dtype=np.float64), (B, np.asarray(uTraj).shape[-1]))] * k, axis=0) for t in (lb, ub))
    scale = np.repeat([0.0] + list(rels), B)[:, None, None]
    out = ddp_box_backward(rep(dyn), rep(cost), rep(Vf), np.concatenate([np.asarray(uTraj)] * k, axis=0), lbs, ubs, ld=True,
                           perturb=(scale, np.random.default_rng(seed)))
    cut = lambda i: {name: v[B * i:B * (i + 1)] for name, v in out.items()}      # noqa: E731
    return cut(0), [cut(i) for i in range(1, k)]


def rigid_body_step_torch(dt):
    """torch (CPU, fp64) restatement of x+ = x + dt * zo.quad_rigidBodyDynamics(x, u) without wind (8 states), for the second
    derivatives by autograd, as zo.quad_euler_step_torch is for the 12-state model."""
    import torch

    def f(x, u):
        uvw, pqr = x[0:3], x[3:6]
        phi, theta = x[6], x[7]
        cphi, sphi = torch.cos(phi), torch.sin(phi)
        cth, sth, tth = torch.cos(theta), torch.sin(theta), torch.tan(theta)
        zero = torch.zeros_like(phi)
        flin, fquad, mlin = (torch.tensor(a, dtype=x.dtype) for a in (zo.QUAD_FORCE_LIN, zo.QUAD_FORCE_QUAD, zo.QUAD_MOMENT_LIN))
        force = zo.QUAD_MASS * torch.stack([zero, zero, -u[0]]) + flin * uvw + fquad * uvw ** 2 + \
            zo.QUAD_MASS * zo.QUAD_G * torch.stack([-sth, sphi * cth, cphi * cth])
        uvwDot = (1 / zo.QUAD_MASS) * (-torch.linalg.cross(pqr, uvw) + force)
        pqrDot = u[1:4] + mlin * pqr
        phiDot = pqr[0] + sphi * tth * pqr[1] + cphi * tth * pqr[2]
        thetaDot = cphi * pqr[1] - sphi * pqr[2]
        return x + dt * torch.cat([uvwDot, pqrDot, torch.stack([phiDot, thetaDot])])
    return f


def differentialDynamicProgramming_box(dynFun, f_torch, Q, R, Qf, x0, uGuess, lb, ub, xr=None, ur=None, maxIter=100, tol=1e-3,
                                       return_iters=False, trace=None):
    """tests/ilqr_box_ref.iterativeLqr's loop with the second-order expansion (zo.quadratic_dynamics_from_trajectory of `f_torch`, the
    same map as `dynFun` in torch) and the box DDP backward pass.  `trace` receives (J_new, winning index, the 16 costs, the backward
    pass's clamped masks (T,), its margins (T,)) per iteration."""
    Q, R, Qf = (np.asarray(t, dtype=np.float64) for t in (Q, R, Qf))
    x0, uGuess = np.asarray(x0, dtype=np.float64), np.asarray(uGuess, dtype=np.float64)
    n = x0.shape[0]
    N, m = uGuess.shape
    lb, ub = (np.broadcast_to(np.asarray(t, dtype=np.float64), (m,)) for t in (lb, ub))
    xr = np.zeros((N + 1, n)) if xr is None else xr
    ur = np.zeros((N, m)) if ur is None else ur
    policy = zo.AffinePolicy(uGuess, np.zeros((N, m, n)))
    traj = br.rollout(x0, dynFun, policy, zo.Trajectory(np.zeros((N + 1, n)), np.zeros((N, m))), lb, ub)
    J = tref.trajectory_cost(Q, R, Qf, xr, ur, traj)
    converged, it = False, 0
    while (not converged) and it < maxIter:
        dyn = zo.quadratic_dynamics_from_trajectory(f_torch, traj)
        cost = zo.conditionQuadraticCost(tref.cost_expansion(Q, R, xr, ur, traj))
        Vf = zo.conditionValueFunction(tref.terminal_expansion(Qf, xr, traj.xTraj[-1]))
        one = lambda t: tuple(None if x is None else np.asarray(x)[None] for x in t)      # noqa: E731
        bw = ddp_box_backward(one(dyn), one(cost), one(Vf), traj.uTraj[None], lb, ub)
        policy = zo.AffinePolicy(bw["l"][0], bw["L"][0])
        traj_new, J_new, idx, Js = br.forward_pass(x0, dynFun, Q, R, Qf, xr, ur, policy, traj, lb, ub)
        if trace is not None:
            trace.append((J_new, idx, Js, bw["clamped"][0], bw["margin"][0]))
        converged = bool(abs(J - J_new) <= tol)
        traj, J = traj_new, J_new
        it += 1
    out = (traj, policy.L, J, converged)
    return out + (it,) if return_iters else out
