"""Drop-in for the array-level hot path of ``zopt.ilqrUtils`` on MI355X HIP kernels.

Same function names / arguments / return types as the reference (ilqrUtils.py); arrays may carry extra LEADING
batch axes.  NumPy in -> NumPy out; torch ROCm tensors in -> torch ROCm tensors out.
"""
from __future__ import annotations

import ctypes
import os
from typing import NamedTuple

import numpy as np

from . import _arrays as arr
from . import _lib
from . import models as _models
from ._arrays import batch as _batch, is_fp32 as _is_fp32, shape as _shape
from .pytrees import (AffineDynamics, AffinePolicy, QuadraticCostFunction, QuadraticDynamics,  # noqa: F401
                      QuadraticValueFunction, Trajectory)

try:
    import torch
except Exception:  # pragma: no cover
    torch = None


class _LazyGeneric:
    """zopt_amd.generic (torch.func producers in front of the HIP sweeps for callable models) imports torch unconditionally; it is
    loaded on first use so that `import zopt_amd.ilqrUtils` works on a host without torch, as the other modules do (calls raise)."""
    _mod = None

    @staticmethod
    def is_callable_model(f):
        return callable(f) and not hasattr(f, "c_struct")

    def __getattr__(self, name):
        if _LazyGeneric._mod is None:
            from . import generic
            _LazyGeneric._mod = generic
        return getattr(_LazyGeneric._mod, name)


_generic = _LazyGeneric()


def _fields(t):
    """Fields of a (Named)tuple; the pytrees override __getitem__ (per-time-step slice), so use tuple.__iter__."""
    return list(tuple.__iter__(t)) if isinstance(t, tuple) else list(t)


def _check_shapes(table):
    """`table`: (name, array, expected shape) rows; a row whose shape is None is an operand that is left out (NULL)."""
    for name, X, s in table:
        if s is not None and _shape(X) != s:
            raise ValueError(f"{name} has shape {_shape(X)}, expected {s}")


def _backward_pass(who, entry, dynamics, cost, Vf, ddp=False, boxed=None, cast_back=False, stage_varying=False):
    """The four backwardPass_* functions: shape table, upload, outputs, the call of `entry` and the return.  `boxed`: (uTraj, u_lb, u_ub)
    of the *_box forms (`stage_varying`: the bounds carry a step axis, models.InputBox).  Every sweep computes in fp64; `cast_back` hands an fp32 caller fp32 back -- backwardPass_ilqr does (as the fused
    solves do), backwardPass_ilqr_box, backwardPass_ddp and backwardPass_ddp_box return fp64 whatever came in."""
    dyn = _fields(dynamics)
    f_x, f_u = dyn[1], dyn[2]
    f_xx, f_ux, f_uu = dyn[3:6] if ddp else (None, None, None)
    _, c_x, c_u, c_xx, c_ux, c_uu = _fields(cost)
    _, v_x, v_xx = _fields(Vf)
    shp = _shape(f_u)
    if len(shp) < 3:
        raise ValueError("f_u must have shape (..., N, n, m)")
    lead, (N, n, m) = shp[:-3], shp[-3:]
    if boxed is not None and (n > _models.INPUTBOX_MAX_N or m > _models.INPUTBOX_MAX_M):
        raise ValueError(f"{who}: (n={n}, m={m}) not covered (need n <= 12, m <= 4)")
    # backwardPass_ddp_box alone takes dynamics affine in the controls: f_ux = f_uu = None (identically zero), neither stored nor read
    affine = ddp and boxed is not None and f_ux is None and f_uu is None
    if ddp and boxed is not None and not affine and (f_ux is None or f_uu is None):
        raise ValueError("f_ux and f_uu are None together or not at all")
    step = lead + (N,)
    table = [("f_x", f_x, step + (n, n)), ("f_u", f_u, shp)]   # in the entries' argument order
    if ddp:
        table += [("f_xx", f_xx, step + (n, n, n))]
        table += [("f_ux", None, None), ("f_uu", None, None)] if affine else [("f_ux", f_ux, step + (n, m, n)), ("f_uu", f_uu, step + (n, m, m))]
    table += [("c_x", c_x, step + (n,)), ("c_u", c_u, step + (m,)), ("c_xx", c_xx, step + (n, n)), ("c_ux", c_ux, step + (m, n)),
              ("c_uu", c_uu, step + (m, m)), ("v_x", v_x, lead + (n,)), ("v_xx", v_xx, lead + (n, n))]
    if boxed is not None:
        table += [("uTraj", boxed[0], step + (m,))]
    _check_shapes(table)
    box = _models.InputBox.for_shape(n, m, boxed[1], boxed[2], stage_varying).box_struct(tuple(lead), N) if boxed is not None else None
    dt = torch.float64
    dev = [None if s is None else arr.to_device(X, dt) for _, X, s in table]
    batch = _batch(lead)
    dl = torch.empty(step + (m,), dtype=dt, device=dev[0].device)
    dL = torch.empty(step + (m, n), dtype=dt, device=dev[0].device)
    if ddp and boxed is None and _ddp_large(n, m):
        _ddp_backward_large(dev, dl, dL, batch, N, n, m)
    else:
        ptrs = [None if t is None else t.data_ptr() for t in dev]
        if boxed is not None:         # (..., box*, shared_hessian, l, L, qp_capped, ...)
            ptrs += [ctypes.addressof(box), 0, dl.data_ptr(), dL.data_ptr(), None]
        elif ddp:                     # (..., active, shared_hessian, l, L, ...)
            ptrs += [None, 0, dl.data_ptr(), dL.data_ptr()]
        else:
            ptrs += [dl.data_ptr(), dL.data_ptr()]
        rc = getattr(_lib.lib(), entry)(*ptrs, batch, N, n, m, ctypes.c_void_p(arr.stream_ptr(dev[0])))
        _lib.check(rc, who)
    if cast_back and _is_fp32(f_x):
        dl, dL = dl.to(torch.float32), dL.to(torch.float32)
    return AffinePolicy(arr.result_like(dl, f_x), arr.result_like(dL, f_x))


def backwardPass_ilqr(dynamics, cost, Vf):
    """Backwards pass of the iLQR algorithm (reference ilqrUtils.py:176-181, step :153-173).

    Arguments
    ---------
        dynamics : AffineDynamics(f (..., N, n), f_x (..., N, n, n), f_u (..., N, n, m))   (f is unused, :156)
        cost : QuadraticCostFunction(c (..., N), c_x (..., N, n), c_u (..., N, m), c_xx, c_ux (..., N, m, n), c_uu)
        Vf : QuadraticValueFunction(v (...), v_x (..., n), v_xx (..., n, n)) terminal value function

    Returns
    -------
        AffinePolicy(l (..., N, m), L (..., N, m, n))
    """
    return _backward_pass("backwardPass_ilqr", "zm_ilqr_backward_f64", dynamics, cost, Vf, cast_back=True)


def backwardPass_ilqr_box(dynamics, cost, Vf, uTraj, u_lb, u_ub, stage_varying=False):
    """Backwards pass of control-limited iLQR (Tassa, Mansard, Todorov 2014); an extension, the reference has no counterpart.

    As `backwardPass_ilqr`, with bounds `u_lb <= u <= u_ub` on the inputs: per step `l_k` minimises the step's quadratic model over
    `u_lb - uTraj_k <= l_k <= u_ub - uTraj_k` (a box-constrained QP), the rows of `L_k` of the clamped components are zero and the
    other rows are `-Q_uu[F,F]^-1 Q_ux[F,:]`.

    Arguments
    ---------
        dynamics, cost, Vf : as backwardPass_ilqr
        uTraj : (..., N, m) inputs of the trajectory the expansions were taken along
        u_lb, u_ub : scalars, (m,) or (..., m) with leading axes that broadcast to the batch; entries may be -inf / +inf
        stage_varying : the bounds are (N, m) or (..., N, m) (or a scalar next to such an array): step k uses row k

    Returns
    -------
        AffinePolicy(l (..., N, m), L (..., N, m, n))
    """
    return _backward_pass("backwardPass_ilqr_box", "zm_ilqr_backward_box_f64", dynamics, cost, Vf, boxed=(uTraj, u_lb, u_ub),
                          stage_varying=stage_varying)


def _ddp_large(n, m):
    """Shapes the one-tile DDP kernels (ilqr_backward.hip MODE 2, psd.hip's contracted-dynamics kernel) do not take."""
    return n > 12 or m > 4


def _project_vf_zz(v_x, f_xx, f_ux, f_uu, eps=1e-3):
    """conditionQuadraticDynamics for LARGE shapes (reference ilqrUtils.py:237-251) on flat batches: `vf_.. = einsum('i,ijk', v_x, f_..)`
    (a torch contraction on the GPU), the stacked `[[vf_xx, vf_ux^T],[vf_ux, vf_uu]]` PD-projected by the HIP kernel (zm_psd_project_f64:
    multi-tile matrix-sign iteration beyond 16 x 16), blocks returned.  Arguments (b, n), (b, n, n, n), (b, n, m, n), (b, n, m, m)."""
    n, m = f_ux.shape[-1], f_ux.shape[-2]
    vf_xx = torch.einsum("bi,bijk->bjk", v_x, f_xx)
    vf_ux = torch.einsum("bi,bijk->bjk", v_x, f_ux)
    vf_uu = torch.einsum("bi,bijk->bjk", v_x, f_uu)
    Z = torch.cat([torch.cat([vf_xx, vf_ux.transpose(-1, -2)], dim=-1), torch.cat([vf_ux, vf_uu], dim=-1)], dim=-2).contiguous()
    if Z.shape[0]:
        rc = _lib.lib().zm_psd_project_f64(Z.data_ptr(), Z.shape[0], n + m, float(eps), ctypes.c_void_p(arr.stream_ptr(Z)))
        _lib.check(rc, "conditionQuadraticDynamics")
    return Z[:, :n, :n], Z[:, n:, :n], Z[:, n:, n:]


def _riccati_value_call(f_x, f_u, c, c_x, c_u, c_xx, c_ux, c_uu, v, v_x, v_xx):
    """zm_riccati_value_f64 (iLQR form, one time step) on flat contiguous batches; returns (v', v_x', v_xx', l, L)."""
    b, n, m = f_u.shape
    dt, dev = f_x.dtype, f_x.device
    dl, dL = torch.empty((b, m), dtype=dt, device=dev), torch.empty((b, m, n), dtype=dt, device=dev)
    ov, ovx, ovxx = torch.empty(b, dtype=dt, device=dev), torch.empty((b, n), dtype=dt, device=dev), torch.empty((b, n, n), dtype=dt, device=dev)
    ts = [t.contiguous() for t in (f_x, f_u, c, c_x, c_u, c_xx, c_ux, c_uu, v, v_x, v_xx)]
    rc = _lib.lib().zm_riccati_value_f64(ts[0].data_ptr(), ts[1].data_ptr(), None, None, None, *[t.data_ptr() for t in ts[2:]],
                                         dl.data_ptr(), dL.data_ptr(), ov.data_ptr(), ovx.data_ptr(), ovxx.data_ptr(), b, 1, n, m,
                                         ctypes.c_void_p(arr.stream_ptr(f_x)))
    _lib.check(rc, "riccatiStep")
    return ov, ovx, ovxx, dl, dL


def _ddp_step_large(f_x, f_u, f_xx, f_ux, f_uu, c, c_x, c_u, c_xx, c_ux, c_uu, v, v_x, v_xx):
    """riccatiStep_ddp for large shapes (reference ilqrUtils.py:184-206): the iLQR step (HIP tile sweep, T = 1) with the cost Hessians
    augmented by the PD-projected second-order terms -- Q_xx = c_xx + f_x^T v_xx f_x + vf_xx etc. (:196-198)."""
    vf_xx, vf_ux, vf_uu = _project_vf_zz(v_x, f_xx, f_ux, f_uu)
    return _riccati_value_call(f_x, f_u, c, c_x, c_u, c_xx + vf_xx, c_ux + vf_ux, c_uu + vf_uu, v, v_x, v_xx)


def _ddp_backward_large(dev, dl, dL, batch, N, n, m):
    """backwardPass_ddp beyond the one-tile DDP sweep (n <= 12, m <= 4): the recursion runs step by step from the host, per step a torch
    contraction, the HIP PD projection of the stacked (n+m)^2 matrix and the HIP tile sweep for one step (three launches per time step:
    a coverage path for the shapes the generic-callable drivers take, not a fast one).  `dev`: the uploaded operands in the order of
    zm_ddp_backward_f64; fills dl, dL."""
    if n > 48 or m > 16:
        raise ValueError(f"backwardPass_ddp: (n={n}, m={m}) not covered (need n <= 48, m <= 16)")
    nlead = dl.dim() - 2
    fx, fu, fxx, fux, fuu, cx, cu, cxx, cux, cuu, vx, vxx = (t.reshape((batch,) + tuple(t.shape[nlead:])) for t in dev)
    vv = torch.zeros(batch, dtype=dl.dtype, device=vx.device)
    zc = torch.zeros(batch, dtype=dl.dtype, device=vx.device)
    fl, fL = dl.reshape(batch, N, m), dL.reshape(batch, N, m, n)
    for k in range(N - 1, -1, -1):
        vv, vx, vxx, lk, Lk = _ddp_step_large(fx[:, k], fu[:, k], fxx[:, k].contiguous(), fux[:, k].contiguous(), fuu[:, k].contiguous(),
                                              zc, cx[:, k], cu[:, k], cxx[:, k], cux[:, k], cuu[:, k], vv, vx, vxx)
        fl[:, k], fL[:, k] = lk, Lk


def _riccati_step(dynamics, cost, value, ddp):
    """One backward step with the value function returned (zm_riccati_value_f64, T = 1)."""
    dyn = _fields(dynamics)
    f_x, f_u = dyn[1], dyn[2]
    c, c_x, c_u, c_xx, c_ux, c_uu = _fields(cost)
    v, v_x, v_xx = _fields(value)
    shp = _shape(f_u)
    if len(shp) < 2:
        raise ValueError("f_u must have shape (..., n, m)")
    lead, (n, m) = shp[:-2], shp[-2:]
    table = [("f_x", f_x, lead + (n, n)), ("c", c, lead), ("c_x", c_x, lead + (n,)), ("c_u", c_u, lead + (m,)),
             ("c_xx", c_xx, lead + (n, n)), ("c_ux", c_ux, lead + (m, n)), ("c_uu", c_uu, lead + (m, m)),
             ("v", v, lead), ("v_x", v_x, lead + (n,)), ("v_xx", v_xx, lead + (n, n))]
    if ddp:
        table += [("f_xx", dyn[3], lead + (n, n, n)), ("f_ux", dyn[4], lead + (n, m, n)), ("f_uu", dyn[5], lead + (n, m, m))]
    _check_shapes(table)
    template = f_x
    dt = torch.float64
    df_x, df_u, dc, dc_x, dc_u, dc_xx, dc_ux, dc_uu, dv, dv_x, dv_xx = (arr.to_device(X, dt) for X in (f_x, f_u, c, c_x, c_u, c_xx, c_ux,
                                                                                                       c_uu, v, v_x, v_xx))
    zk = [arr.to_device(X, dt) for X in dyn[3:6]] if ddp else []   # the second derivatives, uploaded once and held until the call is out
    z = [t.data_ptr() for t in zk] if ddp else [None, None, None]
    batch = _batch(lead)
    dev = df_x.device
    if ddp and _ddp_large(n, m):
        fl = lambda t, tail: t.reshape((batch,) + tail)
        ov, ovx, ovxx, dl, dL = _ddp_step_large(fl(df_x, (n, n)), fl(df_u, (n, m)), fl(zk[0], (n, n, n)), fl(zk[1], (n, m, n)),
                                                fl(zk[2], (n, m, m)), fl(dc, ()), fl(dc_x, (n,)), fl(dc_u, (m,)), fl(dc_xx, (n, n)),
                                                fl(dc_ux, (m, n)), fl(dc_uu, (m, m)), fl(dv, ()), fl(dv_x, (n,)), fl(dv_xx, (n, n)))
        outs = [arr.result_like(o.reshape(lead + tuple(o.shape[1:])), template) for o in (ov, ovx, ovxx, dl, dL)]
        if not arr.is_torch(template) and len(lead) == 0:
            outs[0] = float(outs[0])
        return QuadraticValueFunction(*outs[:3]), AffinePolicy(*outs[3:])
    dl = torch.empty(lead + (m,), dtype=dt, device=dev)
    dL = torch.empty(lead + (m, n), dtype=dt, device=dev)
    ov = torch.empty(lead, dtype=dt, device=dev)
    ovx = torch.empty(lead + (n,), dtype=dt, device=dev)
    ovxx = torch.empty(lead + (n, n), dtype=dt, device=dev)
    rc = _lib.lib().zm_riccati_value_f64(df_x.data_ptr(), df_u.data_ptr(), z[0], z[1], z[2], dc.data_ptr(), dc_x.data_ptr(),
                                         dc_u.data_ptr(), dc_xx.data_ptr(), dc_ux.data_ptr(), dc_uu.data_ptr(), dv.data_ptr(),
                                         dv_x.data_ptr(), dv_xx.data_ptr(), dl.data_ptr(), dL.data_ptr(), ov.data_ptr(),
                                         ovx.data_ptr(), ovxx.data_ptr(), batch, 1, n, m, ctypes.c_void_p(arr.stream_ptr(df_x)))
    _lib.check(rc, "riccatiStep")
    outs = [arr.result_like(o, template) for o in (ov, ovx, ovxx, dl, dL)]
    if not arr.is_torch(template) and len(lead) == 0:
        outs[0] = float(outs[0])
    return QuadraticValueFunction(*outs[:3]), AffinePolicy(*outs[3:])


def riccatiStep_ilqr(dynamics, cost, value):
    """One step of the iLQR Riccati recursion (reference ilqrUtils.py:153-173): AffineDynamics (f (n), f_x (n,n), f_u (n,m)),
    QuadraticCostFunction and QuadraticValueFunction of ONE time step (optionally with leading batch axes) ->
    (QuadraticValueFunction(v', v_x', v_xx'), AffinePolicy(l, L))."""
    return _riccati_step(dynamics, cost, value, ddp=False)


def riccatiStep_ddp(dynamics, cost, value):
    """One step of the DDP Riccati recursion (reference ilqrUtils.py:184-206): as riccatiStep_ilqr with QuadraticDynamics
    (f, f_x, f_u, f_xx (n,n,n), f_ux (n,m,n), f_uu (n,m,m)); the second-order terms are PD-projected (:237-251)."""
    return _riccati_step(dynamics, cost, value, ddp=True)


LINESEARCH_ALPHAS = 0.5 ** np.arange(16)   # reference ilqrUtils.py:145
_TRACE = None   # diagnostics: a list; while it is one, the fused drivers run zm_ilqr_solve_trace_f64 and append ("iterations", its),
#                 ("J_trace", (its, batch) costs after every iteration's acceptance), ("alpha_trace", (its, batch) winning step-size indices)
#                 a StateBox solve (zm_ilqr_solve_state_trace_f64): "iterations" counts the outer iterations, J_trace / alpha_trace are
#                 (outer, maxIter, batch) (J_AL; NaN / -1 where nothing ran), plus ("violation_trace", (outer, batch)), ("mu_trace", (outer,
#                 batch)) and ("inner_trace", (outer, batch) iLQR iterations per outer iteration)


class ConstraintInfo(NamedTuple):
    """What `constrainedIterativeLqr` returns besides `iterativeLqr`'s four: per trajectory the largest violation of the state bounds
    over k = 1..N, the final penalty, the multipliers (..., N+1, n) (row 0 zero), the outer iterations it took part in and its iLQR
    iterations in each of them (..., outer)."""
    violation: object
    mu: object
    lam_lb: object
    lam_ub: object
    outerIterations: object
    innerIterations: object


class TracedConstraintInfo(NamedTuple):
    """`ConstraintInfo` of a `models.TracedConstraint` solve: per trajectory the largest pos(g) over the stage rows k = 0..N-1 and the
    terminal row, the final penalty, the multipliers of the stage rows (..., N, n_con) and of the terminal row (..., n_con_terminal),
    the outer iterations it took part in and its iLQR iterations in each of them (..., outer)."""
    violation: object
    mu: object
    lam: object
    lam_terminal: object
    outerIterations: object
    innerIterations: object


def _rollout(x0, dynFun, policy, trajPrev, alphas, costFun):
    """Shared driver of trajectoryRollout / forwardPass2 on the rollout_linesearch kernel."""
    if isinstance(dynFun, _models.TracedConstraint):
        if costFun is not None:
            raise ValueError("forwardPass2 takes no TracedConstraint: its cost would silently omit the constraints' penalty (the line "
                             "search on the augmented-Lagrangian cost runs inside iterativeLqr / constrainedIterativeLqr; an array-level "
                             "form is the follow-up)")
        dynFun = dynFun.model         # the dynamics are unchanged
    if isinstance(dynFun, _models.StateBox):
        if costFun is not None:
            raise ValueError("forwardPass2 takes no StateBox: its cost would silently omit the state box's penalty (the line search on "
                             "the augmented-Lagrangian cost runs inside iterativeLqr / constrainedIterativeLqr)")
        dynFun = dynFun.model         # the dynamics are unchanged; an inner InputBox still clips
    box = dynFun if isinstance(dynFun, _models.InputBox) else None
    if box is not None:
        dynFun = box.model
    traced_cost = _models.traced_cost_of(costFun)
    if traced_cost is not None:       # (before anything touches the device)
        _models.check_traced_cost(traced_cost, dynFun, "forwardPass2", box=box)
    if _generic.is_callable_model(dynFun):
        return _rollout_generic(x0, dynFun, policy, trajPrev, alphas, costFun)
    if not hasattr(dynFun, "c_struct"):
        raise TypeError("dynFun must be a registered device model (zopt_amd.models.LinearModel / QuadcopterEuler) or a torch "
                        "callable f(x, u) -> x+ (generic path, zopt_amd/generic.py)")
    tracking = isinstance(costFun, _models.TrackingCost)
    if tracking:
        _models.refuse_traced(dynFun, "forwardPass2 with a TrackingCost", "the tracking line search on the tape interpreter is the follow-up")
    if costFun is not None and not tracking and traced_cost is None and not hasattr(costFun, "c_struct"):
        raise TypeError("costFun must be a registered zopt_amd.models.QuadraticCost, TrackingCost or TracedCost")
    l, L = _fields(policy)
    xPrev, uPrev = _fields(trajPrev)
    n, m = dynFun.n, dynFun.m
    shp = _shape(L)
    lead, (N, mm, nn) = shp[:-3], shp[-3:]
    if (mm, nn) != (m, n):
        raise ValueError(f"policy.L has shape {shp}, model is (n={n}, m={m})")
    if box is not None:
        box.check_horizon(N)          # (before anything touches the device)
    for name, X, s in (("x0", x0, lead + (n,)), ("policy.l", l, lead + (N, m)), ("xPrev", xPrev, lead + (N + 1, n)),
                       ("uPrev", uPrev, lead + (N, m))):
        if _shape(X) != s:
            raise ValueError(f"{name} has shape {_shape(X)}, expected {s}")
    dt = torch.float64
    dx0, dl, dL, dxp, dup = (arr.to_device(X, dt) for X in (x0, l, L, xPrev, uPrev))
    dal = arr.to_device(np.asarray(alphas, dtype=np.float64), dt)
    batch = _batch(lead)
    xT = torch.empty(lead + (N + 1, n), dtype=dt, device=dx0.device)
    uT = torch.empty(lead + (N, m), dtype=dt, device=dx0.device)
    J = torch.empty(lead, dtype=dt, device=dx0.device) if costFun is not None else None
    md = _models.model_struct(dynFun, lead)
    if traced_cost is not None:       # the line search with the cost tape next to the model step (list == NULL: every trajectory)
        cs = traced_cost.tcost_struct(tuple(lead))
        rc = _lib.lib().zm_traced_cost_linesearch_list_f64(
            ctypes.addressof(md), ctypes.addressof(cs), dx0.data_ptr(), dl.data_ptr(), dL.data_ptr(), dxp.data_ptr(), dup.data_ptr(),
            dal.data_ptr(), int(dal.numel()), None, 0, None, xT.data_ptr(), uT.data_ptr(), J.data_ptr(), None, batch, N,
            ctypes.c_void_p(arr.stream_ptr(dx0)))
        _lib.check(rc, "rollout")
        return Trajectory(arr.result_like(xT, L), arr.result_like(uT, L)), arr.result_like(J, L)
    cs = (costFun.track_struct(lead, N) if tracking else costFun.c_struct()) if costFun is not None else None
    linesearch = _lib.lib().zm_rollout_linesearch_tracking_f64 if tracking else _lib.lib().zm_rollout_linesearch_f64
    pcs = ctypes.addressof(cs) if cs is not None else None
    head = (pcs,)
    if box is not None:               # (model*, cost* | NULL, track* | NULL, box*, ...)
        bs = box.box_struct(tuple(lead), N)
        linesearch, head = _lib.lib().zm_rollout_linesearch_box_f64, (None if tracking else pcs, pcs if tracking else None,
                                                                      ctypes.addressof(bs))
    rc = linesearch(
        ctypes.addressof(md), *head, dx0.data_ptr(), dl.data_ptr(),
        dL.data_ptr(), dxp.data_ptr(), dup.data_ptr(), dal.data_ptr(), int(dal.numel()), None, xT.data_ptr(),
        uT.data_ptr(), J.data_ptr() if J is not None else None, None, batch, N, ctypes.c_void_p(arr.stream_ptr(dx0)))
    _lib.check(rc, "rollout")
    traj = Trajectory(arr.result_like(xT, L), arr.result_like(uT, L))
    return traj, (arr.result_like(J, L) if J is not None else None)


def _torch_costs(runningCost, terminalCost):
    """torch callables (x, u) -> c, (x) -> cf from what the caller passed: torch callables as they are; a registered QuadraticCost (or
    its bound methods) as x'Qx + u'Ru, x'Qf x on device copies of its matrices"""
    if _models.traced_cost_of(runningCost, terminalCost) is not None:
        _models.check_traced_cost(_models.traced_cost_of(runningCost, terminalCost), None, "the generic torch-callable path")
    for c in (runningCost, getattr(runningCost, "__self__", None), terminalCost, getattr(terminalCost, "__self__", None)):
        if isinstance(c, _models.TrackingCost):
            raise TypeError("a TrackingCost cannot run on the generic-callable path: its callables carry no stage index, so a reference "
                            "would be dropped -- register a device model, or close torch callables over a constant goal")
    for c in (runningCost, getattr(runningCost, "__self__", None)):
        if isinstance(c, _models.QuadraticCost):
            Q, R, Qf = (arr.to_device(M, torch.float64) for M in (c.Q, c.R, c.Qf))
            return (lambda x, u: x @ Q @ x + u @ R @ u), (lambda x: x @ Qf @ x)
    if not callable(runningCost) or not callable(terminalCost):
        raise TypeError("runningCost / terminalCost must be torch callables or a registered zopt_amd.models.QuadraticCost")
    return runningCost, terminalCost


def _rollout_generic(x0, dynFun, policy, trajPrev, alphas, costFun):
    """trajectoryRollout / forwardPass2 for a torch callable `dynFun(x, u) -> x+` (zopt_amd/generic.py); `costFun`: None, a
    registered QuadraticCost, or an object with torch callables `.runningCost(x, u)` / `.terminalCost(x)` (CostFunction of the
    reference, pytrees.py:27-38)."""
    if isinstance(costFun, _models.TrackingCost):
        raise TypeError("a TrackingCost needs a registered device model: the generic-callable rollout has no stage index to read the "
                        "reference by")
    l, L = _fields(policy)
    xPrev, uPrev = _fields(trajPrev)
    shp = _shape(L)
    lead, (N, m, n) = shp[:-3], shp[-3:]
    dt = torch.float64
    dx0, dl, dL, dxp, dup = (arr.to_device(X, dt) for X in (x0, l, L, xPrev, uPrev))
    dx0, dl, dL = dx0.reshape(-1, n), dl.reshape(-1, N, m), dL.reshape(-1, N, m, n)
    dxp, dup = dxp.reshape(-1, N + 1, n), dup.reshape(-1, N, m)
    if costFun is None:
        al = arr.to_device(np.asarray(alphas, dtype=np.float64), dt)
        xs, us, _ = _generic.rollout(dx0, dynFun, dl, dL, dxp, dup, al)
        xT, uT, J = xs[:, 0], us[:, 0], None
    else:
        rc, tc = _torch_costs(getattr(costFun, "runningCost", costFun), getattr(costFun, "terminalCost", costFun))
        xT, uT, J = _generic.forward_pass2(dx0, dynFun, rc, tc, dl, dL, dxp, dup)
        J = arr.result_like(J.reshape(lead), L)
    traj = Trajectory(arr.result_like(xT.reshape(lead + (N + 1, n)), L), arr.result_like(uT.reshape(lead + (N, m)), L))
    return traj, J


def trajectoryRollout(x0, dynFun, policy, trajPrev, alpha=1):
    """Rollout a trajectory from the initial state using the provided control policy (reference ilqrUtils.py:33-66):
    `u_k = alpha*l_k + L_k (x_k - xPrev_k) + uPrev_k`, `x_{k+1} = dynFun(x_k, u_k)`; returns Trajectory(xTraj (N+1,n)
    incl. x0, uTraj (N,m)).  `dynFun` is a registered device model."""
    traj, _ = _rollout(x0, dynFun, policy, trajPrev, [float(alpha)], None)
    return traj


def forwardPass2(x0, dynFun, costFun, policy, trajPrev):
    """Simplified iLQR forward pass (reference ilqrUtils.py:116-150): roll out the 16 step sizes 0.5**j and return the
    trajectory of minimum cost and that cost.  `costFun` is a registered QuadraticCost or TrackingCost, or a `models.TracedCost` (a
    recorded cost function: its tape runs next to the model step inside the line-search kernel)."""
    traj, J = _rollout(x0, dynFun, policy, trajPrev, LINESEARCH_ALPHAS, costFun)
    if not arr.is_torch(J) and np.ndim(J) == 0:
        J = float(J)
    return traj, J


def ensurePositiveDefinite(a, eps=1e-3):
    """`w, v = eigh(a); (v * max(w, eps)) @ v.T` (reference ilqrUtils.py:217-219; eigh symmetrises its input).
    `a` is (..., k, k) with k <= 64 (one MFMA tile up to 16, NT x NT tiles beyond: psd_tiled.hip); returns a new array."""
    shp = _shape(a)
    if len(shp) < 2 or shp[-1] != shp[-2]:
        raise ValueError("a must be (..., k, k)")
    k = shp[-1]
    d = arr.to_device(a, torch.float64).clone()
    rc = _lib.lib().zm_psd_project_f64(d.data_ptr(), _batch(shp[:-2]), k, float(eps), ctypes.c_void_p(arr.stream_ptr(d)))
    _lib.check(rc, "ensurePositiveDefinite")
    return arr.result_like(d, a)


def conditionQuadraticCost(quadratic_cost):
    """Ensure quadratic cost is strictly positive definite (reference ilqrUtils.py:222-234): project the stacked
    Hessian [[c_xx, c_ux^T],[c_ux, c_uu]] of every time step and slice it back."""
    c, c_x, c_u, c_xx, c_ux, c_uu = _fields(quadratic_cost)
    shp = _shape(c_ux)
    m, n = shp[-2:]
    lead = shp[:-2]
    if _shape(c_xx) != lead + (n, n) or _shape(c_uu) != lead + (m, m):
        raise ValueError("inconsistent cost Hessian shapes")
    dxx, dux, duu = (arr.to_device(X, torch.float64).clone() for X in (c_xx, c_ux, c_uu))
    rc = _lib.lib().zm_condition_cost_f64(dxx.data_ptr(), dux.data_ptr(), duu.data_ptr(), _batch(lead), n, m, 1e-3,
                                          ctypes.c_void_p(arr.stream_ptr(dxx)))
    _lib.check(rc, "conditionQuadraticCost")
    return QuadraticCostFunction(c, c_x, c_u, arr.result_like(dxx, c_xx), arr.result_like(dux, c_ux),
                                 arr.result_like(duu, c_uu))


def conditionValueFunction(Vf):
    """reference ilqrUtils.py:254-257."""
    v, v_x, v_xx = _fields(Vf)
    return QuadraticValueFunction(v, v_x, ensurePositiveDefinite(v_xx))


def conditionQuadraticDynamics(quadratic_dynamics, v_x):
    """Ensure the quadratic terms of the DDP riccati step are positive definite (reference ilqrUtils.py:237-251):
    `vf_.. = einsum('i,ijk', v_x, f_..)`, the stacked `[[vf_xx, vf_ux^T],[vf_ux, vf_uu]]` PD-projected, blocks returned as
    `(vf_xx (..., n, n), vf_ux (..., m, n), vf_uu (..., m, m))`.  One time step or any leading batch / time axes."""
    dyn = _fields(quadratic_dynamics)
    f_xx, f_ux, f_uu = dyn[3], dyn[4], dyn[5]
    shp = _shape(f_ux)
    if len(shp) < 3:
        raise ValueError("f_ux must have shape (..., n, m, n)")
    lead, (n, m, n2) = shp[:-3], shp[-3:]
    if n2 != n or _shape(f_xx) != lead + (n, n, n) or _shape(f_uu) != lead + (n, m, m) or _shape(v_x) != lead + (n,):
        raise ValueError("conditionQuadraticDynamics: inconsistent shapes")
    dt = torch.float64
    dxx, dux, duu, dvx = (arr.to_device(X, dt).contiguous() for X in (f_xx, f_ux, f_uu, v_x))
    count = _batch(lead)
    if n + m > 16:      # beyond the one-tile kernel: torch contraction + the multi-tile HIP projection
        oxx, oux, ouu = _project_vf_zz(dvx.reshape(count, n), dxx.reshape(count, n, n, n), dux.reshape(count, n, m, n),
                                       duu.reshape(count, n, m, m))
        return tuple(arr.result_like(o.reshape(lead + tuple(o.shape[1:])).contiguous(), f_xx) for o in (oxx, oux, ouu))
    oxx = torch.empty(lead + (n, n), dtype=dt, device=dxx.device)
    oux = torch.empty(lead + (m, n), dtype=dt, device=dxx.device)
    ouu = torch.empty(lead + (m, m), dtype=dt, device=dxx.device)
    rc = _lib.lib().zm_condition_dynamics_f64(dxx.data_ptr(), dux.data_ptr(), duu.data_ptr(), dvx.data_ptr(), oxx.data_ptr(),
                                              oux.data_ptr(), ouu.data_ptr(), count, n, m, 1e-3,
                                              ctypes.c_void_p(arr.stream_ptr(dxx)))
    _lib.check(rc, "conditionQuadraticDynamics")
    return tuple(arr.result_like(o, f_xx) for o in (oxx, oux, ouu))


def _registered_cost(runningCost, terminalCost):
    """Accepts a zopt_amd.models.QuadraticCost or TrackingCost handle (for both arguments) or its bound methods."""
    kinds = (_models.QuadraticCost, _models.TrackingCost, _models.TracedCost)
    for c in (runningCost, getattr(runningCost, "__self__", None)):
        if isinstance(c, kinds):
            other = terminalCost if isinstance(terminalCost, kinds) else getattr(terminalCost, "__self__", None)
            if other is not c:
                raise TypeError(f"runningCost and terminalCost must come from the same {type(c).__name__}")
            return c
    raise TypeError("runningCost / terminalCost must be a registered zopt_amd.models.QuadraticCost, TrackingCost or TracedCost (or its "
                    ".runningCost / .terminalCost methods); arbitrary Python callables cannot run inside a HIP kernel")


def backwardPass_ddp(dynamics, cost, Vf):
    """Backwards pass of the DDP algorithm (reference ilqrUtils.py:209-214, step :184-206, :237-251).

    Arguments
    ---------
        dynamics : QuadraticDynamics(f, f_x (..., N, n, n), f_u (..., N, n, m), f_xx (..., N, n, n, n),
                   f_ux (..., N, n, m, n), f_uu (..., N, n, m, m))
        cost : QuadraticCostFunction, Vf : QuadraticValueFunction   (as backwardPass_ilqr)

    Returns
    -------
        AffinePolicy(l (..., N, m), L (..., N, m, n))
    """
    return _backward_pass("backwardPass_ddp", "zm_ddp_backward_f64", dynamics, cost, Vf, ddp=True)


def backwardPass_ddp_box(dynamics, cost, Vf, uTraj, u_lb, u_ub, stage_varying=False):
    """Backwards pass of control-limited DDP (Tassa, Mansard, Todorov 2014) with the second-order dynamics terms; an extension, the
    reference has no counterpart.

    As `backwardPass_ddp` (per step `Q_xx`, `Q_ux`, `Q_uu` receive the blocks of the PD-projected `sum_i v_x[i] d2f_i/dz2`), with
    the bounds of `backwardPass_ilqr_box`: `l_k` minimises the step's quadratic model over `u_lb - uTraj_k <= l_k <= u_ub - uTraj_k`,
    the rows of `L_k` of the clamped components are zero.

    Arguments
    ---------
        dynamics : QuadraticDynamics(f, f_x, f_u, f_xx, f_ux, f_uu) as backwardPass_ddp; f_ux and f_uu may both be None for dynamics
                   affine in the controls (they are identically zero and are neither stored nor read)
        cost, Vf : as backwardPass_ilqr
        uTraj : (..., N, m) inputs of the trajectory the expansions were taken along
        u_lb, u_ub : scalars, (m,) or (..., m) with leading axes that broadcast to the batch; entries may be -inf / +inf

    Returns
    -------
        AffinePolicy(l (..., N, m), L (..., N, m, n))
    """
    return _backward_pass("backwardPass_ddp_box", "zm_ddp_backward_box_f64", dynamics, cost, Vf, ddp=True, boxed=(uTraj, u_lb, u_ub),
                          stage_varying=stage_varying)


def iterativeLqr(dynamics, runningCost, terminalCost, x0, uGuess, maxIter=100, tol=1e-3):
    """Iterative LQR algorithm (reference ilqrUtils.py:260-327), batched and device-resident.

    Arguments
    ---------
        dynamics : registered discrete model `xOut = f(x,u)` (zopt_amd.models.LinearModel / QuadcopterEuler)
        runningCost, terminalCost : a registered zopt_amd.models.QuadraticCost or TrackingCost, or a zopt_amd.models.TracedCost --
                   user-written cost callables, recorded once (the handle, or its two methods); a TracedCost's Hessians are per
                   point, expanded and PD-conditioned in every iteration over the trajectories that have not converged
        x0 : (..., n) initial state(s)
        uGuess : (..., N, m) initial guess for the control trajectory
        maxIter : maximum number of iLQR iterations
        tol : convergence tolerance `abs(J_prev - J) <= tol` (per trajectory)

    Returns
    -------
        traj : Trajectory(xTraj (..., N+1, n), uTraj (..., N, m))
        L : (..., N, m, n) feedback gains: `u[k] = L[k] @ (x[k]-xTraj[k]) + uTraj[k]`
        J : (...) cost
        converged : (...) bool

    Per iteration (ilqrUtils.py:305-322): linearise along the trajectory, expand the cost, PD-condition the cost and
    terminal Hessians (they are trajectory-independent for a quadratic cost: done once, shared), backward pass,
    16-way line-search rollout, `converged = |J - J_new| <= tol`.  Converged trajectories drop out of later iterations
    (the reference under vmap would run every lane to the slowest).
    """
    return _ilqr_or_ddp(dynamics, runningCost, terminalCost, x0, uGuess, maxIter, tol, ddp=False)


def constrainedIterativeLqr(dynamics, runningCost, terminalCost, x0, uGuess, maxIter=100, tol=1e-3):
    """`iterativeLqr` with bounds on the states: `dynamics` is a `models.StateBox` (around a registered model or an `InputBox`), solved
    by an augmented-Lagrangian outer loop around the fused iLQR -- per outer iteration an iLQR solve (at most `maxIter` iterations,
    `|J_AL - J_AL,new| <= tol`) on the cost plus the penalty of the state box, then the multiplier and penalty update; a trajectory is
    done (`converged`) when its inner solve converged and its violation is <= the StateBox's `ctol`, and is not touched again.

    `dynamics` may also be a `models.TracedConstraint` (user-written constraints g(x, u) <= 0, terminal(x) <= 0 around a registered
    model or a `TracedModel`): the same loop on the penalty of the recorded constraints.

    Returns (traj, L, J, converged, info): `J` is the plain cost of the returned trajectory, `info` a `ConstraintInfo` (a
    `TracedConstraintInfo` for a TracedConstraint)."""
    if not isinstance(dynamics, (_models.StateBox, _models.TracedConstraint)):
        raise TypeError("constrainedIterativeLqr: dynamics must be a zopt_amd.models.StateBox or a zopt_amd.models.TracedConstraint")
    return _ilqr_or_ddp(dynamics, runningCost, terminalCost, x0, uGuess, maxIter, tol, ddp=False, info=True)


def differentialDynamicProgramming(dynamics, runningCost, terminalCost, x0, uGuess, maxIter=100, tol=1e-3):
    """Differential dynamic programming algorithm (reference ilqrUtils.py:330-397): `iterativeLqr` with the second-order
    expansion of the dynamics (QuadraticDynamics.from_trajectory, :365) and `backwardPass_ddp` (:373).  Same arguments
    and return values as `iterativeLqr`.  A `models.InputBox` around a quadcopter model is solved as by `iterativeLqr`, on
    `backwardPass_ddp_box`; around a LinearModel it is refused (no second derivatives: `iterativeLqr` is the call)."""
    return _ilqr_or_ddp(dynamics, runningCost, terminalCost, x0, uGuess, maxIter, tol, ddp=True)


def _ilqr_or_ddp_generic(dynamics, runningCost, terminalCost, x0, uGuess, maxIter, tol, ddp):
    """The drivers for a torch callable `dynamics(x, u) -> x+` (and torch callables or a registered QuadraticCost for the costs):
    zopt_amd/generic.py produces the expansions and the line-search rollouts with torch.func on the GPU, the sweeps and the PD
    projections are the HIP kernels."""
    rc, tc = _torch_costs(runningCost, terminalCost)
    shp = _shape(uGuess)
    lead, (N, m) = shp[:-2], shp[-2:]
    n = _shape(x0)[-1]
    if _shape(x0) != lead + (n,):
        raise ValueError(f"x0 {_shape(x0)} / uGuess {shp} do not match")
    dt = torch.float64
    dx0 = arr.to_device(x0, dt).reshape(-1, n).contiguous()
    dug = arr.to_device(uGuess, dt).reshape(-1, N, m).contiguous()
    xT, uT, L, J, cv = _generic.solve(dynamics, rc, tc, dx0, dug, maxIter, tol, ddp)
    tmpl = uGuess
    xo, uo, Lo, Jo = (arr.result_like(o, tmpl) for o in (xT.reshape(lead + (N + 1, n)), uT.reshape(lead + (N, m)),
                                                      L.reshape(lead + (N, m, n)), J.reshape(lead)))
    co = arr.result_like(cv.reshape(lead), tmpl)
    if not arr.is_torch(tmpl) and len(lead) == 0:
        Jo, co = float(Jo), bool(co)
    return Trajectory(xo, uo), Lo, Jo, co


def _ilqr_or_ddp(dynamics, runningCost, terminalCost, x0, uGuess, maxIter, tol, ddp, info=False):
    model = dynamics
    con = model if isinstance(model, _models.TracedConstraint) else None
    if con is not None:               # (before anything touches the device)
        if ddp:
            raise ValueError("differentialDynamicProgramming takes no TracedConstraint: DDP with recorded constraints is the follow-up "
                             "to the augmented-Lagrangian iLQR (use iterativeLqr / constrainedIterativeLqr)")
        if _models.traced_cost_of(runningCost, terminalCost) is not None:
            raise TypeError("iterativeLqr: a TracedConstraint takes a QuadraticCost or a TrackingCost -- a TracedCost next to recorded "
                            "constraints (per-point cost Hessians under the penalty's addend) is the follow-up")
        model = con.model
    sbox = model if isinstance(model, _models.StateBox) else None
    if sbox is not None:
        if ddp:                       # (before anything touches the device)
            raise ValueError("differentialDynamicProgramming takes no StateBox: DDP with state bounds is the follow-up to the "
                             "augmented-Lagrangian iLQR (use iterativeLqr / constrainedIterativeLqr)")
        model = sbox.model
    box = model if isinstance(model, _models.InputBox) else None
    if box is not None:
        if ddp and isinstance(box.model, _models.LinearModel):   # (before anything touches the device)
            raise ValueError("differentialDynamicProgramming takes no InputBox around a LinearModel: a linear model has no second "
                             "derivatives, DDP is iLQR there (use iterativeLqr)")
        model = box.model
    if _models.traced_cost_of(runningCost, terminalCost) is not None:   # (before anything touches the device)
        _models.check_traced_cost(_registered_cost(runningCost, terminalCost), model,
                                  "differentialDynamicProgramming" if ddp else "iterativeLqr", box=box, sbox=sbox)
    if _generic.is_callable_model(model):
        return _ilqr_or_ddp_generic(dynamics, runningCost, terminalCost, x0, uGuess, maxIter, tol, ddp)
    if not hasattr(model, "c_struct"):
        raise TypeError("dynamics must be a registered device model (zopt_amd.models.*) or a torch callable f(x, u) -> x+")
    cost = _registered_cost(runningCost, terminalCost)
    traced_cost = isinstance(cost, _models.TracedCost)
    if isinstance(cost, _models.TrackingCost):                   # (before anything touches the device)
        _models.refuse_traced(model, "iterativeLqr / differentialDynamicProgramming with a TrackingCost",
                              "the tracking line search and expansion on the tape interpreter are the follow-up")
    n, m = model.n, model.m
    shp = _shape(uGuess)
    lead, (N, mm) = shp[:-2], shp[-2:]
    if mm != m or _shape(x0) != lead + (n,):
        raise ValueError(f"x0 {_shape(x0)} / uGuess {shp} do not match the model (n={n}, m={m})")
    if box is not None:
        box.check_horizon(N)          # (before anything touches the device)
    dt = torch.float64
    lib = _lib.lib()
    dx0 = arr.to_device(x0, dt).reshape(-1, n).contiguous()
    dug = arr.to_device(uGuess, dt).reshape(-1, N, m).contiguous()
    dev = dx0.device
    B = dx0.shape[0]
    st = ctypes.c_void_p(arr.stream_ptr(dx0))
    tracking = isinstance(cost, _models.TrackingCost)
    if tracking and (cost.n != n or cost.m != m):
        raise ValueError(f"the TrackingCost is (n={cost.n}, m={cost.m}), the model (n={n}, m={m})")
    md = _models.model_struct(model, lead)
    if (tracking or not traced_cost) and (cost.n != n or cost.m != m) and con is not None:
        raise ValueError(f"the cost is (n={cost.n}, m={cost.m}), the model (n={n}, m={m})")
    cs = cost.tcost_struct(tuple(lead)) if traced_cost else cost.track_struct(tuple(lead), N) if tracking else cost.c_struct()
    i32 = torch.int32
    L = torch.empty((B, N, m, n), dtype=dt, device=dev)
    xT = torch.empty((B, N + 1, n), dtype=dt, device=dev)
    uT = torch.empty((B, N, m), dtype=dt, device=dev)
    J = torch.empty(B, dtype=dt, device=dev)
    converged = torch.zeros(B, dtype=i32, device=dev)
    if sbox is not None:              # what the augmented-Lagrangian loop returns besides (ConstraintInfo)
        lam_lb = torch.empty((B, N + 1, n), dtype=dt, device=dev)
        lam_ub = torch.empty((B, N + 1, n), dtype=dt, device=dev)
        mu = torch.empty(B, dtype=dt, device=dev)
        viol = torch.zeros(B, dtype=dt, device=dev)
        outer_its = torch.zeros(B, dtype=i32, device=dev)
        inner_its = torch.zeros((sbox.outer, B), dtype=i32, device=dev)
    if con is not None:               # likewise (TracedConstraintInfo)
        lam = torch.zeros((B, N, con.n_con), dtype=dt, device=dev)
        lam_t = torch.zeros((B, con.n_con_terminal), dtype=dt, device=dev)
        mu = torch.empty(B, dtype=dt, device=dev)
        viol = torch.zeros(B, dtype=dt, device=dev)
        outer_its = torch.zeros(B, dtype=i32, device=dev)
        inner_its = torch.zeros((con.outer, B), dtype=i32, device=dev)
    al = sbox if sbox is not None else con      # the augmented-Lagrangian wrapper, if any
    if B:
        # The whole loop -- initial rollout (:293-298), per iteration expansions, PD-conditioned Hessians, backward pass, 16-way
        # line search, `converged = |J - J_new| <= tol` (:305-322) over the compacted list of still-active trajectories -- is ONE
        # call into the C ABI: the host side of the iteration runs in C++ (zopt_amd/csrc/ilqr_solve.hip), no Python between the
        # launches.  SYNC: host synchronisation (termination test + rebuild of the id list) every SYNC iterations; the results do
        # not depend on it (an iteration over a converged trajectory touches nothing).
        # One record serves the eight entries (_lib.SOLVE_ARGS names each one's arguments in order).  The plain and the tracking
        # entries take their cost struct as `cost`; the box and state entries take exactly one of `cost` and `track`.
        family = "state_" if sbox is not None else "box_" if box is not None else "tracking_" if tracking else ""
        entry = f"zm_ilqr_solve_{family}{'trace_' if _TRACE is not None else ''}f64"
        if traced_cost:               # a recorded cost: the same loop behind its own entries (`tcost` in place of `cost`)
            entry = f"zm_traced_cost_solve_{'trace_' if _TRACE is not None else ''}f64"
        if con is not None:           # recorded constraints: the state entries' loop behind its own (`con` in place of `sbox`)
            entry = f"zm_traced_con_solve_{'trace_' if _TRACE is not None else ''}f64"
        pmd, pcs = ctypes.addressof(md), ctypes.addressof(cs)
        nws = int(lib.zm_traced_con_solve_workspace_f64(pmd, B, N) if con is not None else
                  lib.zm_ilqr_solve_state_workspace_f64(pmd, B, N) if sbox is not None else
                  lib.zm_traced_cost_solve_workspace_f64(pmd, pcs, B, N, 1 if ddp else 0) if traced_cost else
                  lib.zm_ilqr_solve_workspace_f64(pmd, B, N, 1 if ddp else 0))
        if nws < 0:
            raise ValueError("iterativeLqr: cannot size the workspace for this model")
        ws = torch.empty(nws, dtype=dt, device=dev)
        iwork = torch.empty(2 * B + 2, dtype=i32, device=dev)
        its = ctypes.c_int32(0)
        d = {"model": pmd, "cost": None if tracking and (family in ("state_", "box_") or con is not None) else pcs,
             "track": pcs if tracking else None,
             "tcost": pcs if traced_cost else None,
             "x0": dx0.data_ptr(), "uGuess": dug.data_ptr(), "ddp": 1 if ddp else 0, "max_iter": int(maxIter), "tol": float(tol),
             "sync_every": max(1, int(os.environ.get("ZOPT_AMD_ILQR_SYNC", "4"))), "workspace": ws.data_ptr(),
             "workspace_doubles": nws, "iwork": iwork.data_ptr(), "xTraj": xT.data_ptr(), "uTraj": uT.data_ptr(), "L": L.data_ptr(),
             "J": J.data_ptr(), "converged": converged.data_ptr(), "iterations": ctypes.addressof(its), "batch": B, "T": N, "stream": st}
        if box is not None or sbox is not None:
            bs = box.box_struct(tuple(lead), N) if box is not None else None
            capped = torch.zeros(B, dtype=i32, device=dev)
            d.update(box=ctypes.addressof(bs) if box is not None else None, qp_capped=capped.data_ptr())
        if sbox is not None:
            ss = sbox.statebox_struct(tuple(lead), lam_lb, lam_ub, mu)
            d.update(sbox=ctypes.addressof(ss), mu0=sbox.mu0, growth=sbox.growth, mu_max=sbox.mu_max, outer=sbox.outer, ctol=sbox.ctol,
                     violation=viol.data_ptr(), outer_iterations=outer_its.data_ptr(), inner_iterations=inner_its.data_ptr())
        if con is not None:
            cc = con.con_struct(tuple(lead), lam, lam_t, mu)
            d.update(con=ctypes.addressof(cc), mu0=con.mu0, growth=con.growth, mu_max=con.mu_max, outer=con.outer, ctol=con.ctol,
                     violation=viol.data_ptr(), outer_iterations=outer_its.data_ptr(), inner_iterations=inner_its.data_ptr())
        if _TRACE is not None:        # (outer, maxIter, batch) rows for a state box, (maxIter, batch) otherwise
            outer = al.outer if al is not None else 1
            Jtr = torch.full((outer * max(int(maxIter), 1), B), float("nan"), dtype=dt, device=dev)
            atr = torch.full((outer * max(int(maxIter), 1), B), -1, dtype=i32, device=dev)
            d.update(J_trace=Jtr.data_ptr(), alpha_trace=atr.data_ptr())
            if al is not None:
                vtr = torch.full((outer, B), float("nan"), dtype=dt, device=dev)
                mtr = torch.full((outer, B), float("nan"), dtype=dt, device=dev)
                d.update(violation_trace=vtr.data_ptr(), mu_trace=mtr.data_ptr())
        names = _lib.TRACED_CON_SOLVE_ARGS if con is not None else _lib.TRACED_COST_SOLVE_ARGS if traced_cost else _lib.SOLVE_ARGS
        rc = getattr(lib, entry)(*[d[k] for k in names[entry]])
        _lib.check(rc, "differentialDynamicProgramming" if ddp else "iterativeLqr")
        if _TRACE is not None:
            o = int(its.value)        # iLQR / DDP iterations; outer iterations of a state-box solve
            if al is not None:
                Jtr, atr = Jtr.reshape(outer, -1, B), atr.reshape(outer, -1, B)
            _TRACE.append(("iterations", o))
            _TRACE.append(("J_trace", Jtr[:o].cpu().numpy()))
            _TRACE.append(("alpha_trace", atr[:o].cpu().numpy()))
            if al is not None:
                _TRACE.append(("violation_trace", vtr[:o].cpu().numpy()))
                _TRACE.append(("mu_trace", mtr[:o].cpu().numpy()))
                _TRACE.append(("inner_trace", inner_its[:o].cpu().numpy()))
            if box is not None:
                _TRACE.append(("qp_capped", capped.cpu().numpy()))
    tmpl = uGuess
    fp32_in = _is_fp32(tmpl)
    outs = [xT.reshape(lead + (N + 1, n)), uT.reshape(lead + (N, m)), L.reshape(lead + (N, m, n)), J.reshape(lead)]
    if fp32_in:
        outs = [o.to(torch.float32) for o in outs]
    xo, uo, Lo, Jo = (arr.result_like(o, tmpl) for o in outs)
    co = arr.result_like(converged.bool().reshape(lead), tmpl)
    if not arr.is_torch(tmpl) and len(lead) == 0:
        Jo, co = float(Jo), bool(co)
    if info:
        fl = [viol.reshape(lead), mu.reshape(lead)]
        fl += ([lam.reshape(lead + (N, con.n_con)), lam_t.reshape(lead + (con.n_con_terminal,))] if con is not None else
               [lam_lb.reshape(lead + (N + 1, n)), lam_ub.reshape(lead + (N + 1, n))])
        if fp32_in:
            fl = [o.to(torch.float32) for o in fl]
        res = [arr.result_like(o, tmpl) for o in fl]
        res += [arr.result_like(outer_its.reshape(lead), tmpl),
                arr.result_like(inner_its.transpose(0, 1).contiguous().reshape(lead + (al.outer,)), tmpl)]
        return Trajectory(xo, uo), Lo, Jo, co, (TracedConstraintInfo if con is not None else ConstraintInfo)(*res)
    return Trajectory(xo, uo), Lo, Jo, co
