"""Registered device models and costs (host-side handles for the structs in include/zopt_amd.h).

The reference takes arbitrary Python callables (`dynamics`, `runningCost`, `terminalCost`) and lets JAX trace and
differentiate them (ilqrUtils.py:260-269).  A HIP kernel needs the model in device code, so the fused paths take
one of these handles wherever the reference takes a callable; the handles are also plain callables on NumPy arrays
(same math), so they can be passed to code that expects `f(x, u)`.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _arrays as arr

ZM_MODEL_LINEAR = 1
ZM_MODEL_QUADCOPTER = 2
ZM_MODEL_QUADCOPTER_RB = 3
ZM_MODEL_TRACED = 4


class zm_model_t(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int), ("n", ctypes.c_int), ("m", ctypes.c_int), ("reserved", ctypes.c_int),
                ("dt", ctypes.c_double), ("A", ctypes.c_void_p), ("B", ctypes.c_void_p), ("wind_ned", ctypes.c_double * 3)]


class zm_quadcost_t(ctypes.Structure):
    _fields_ = [("Q", ctypes.c_void_p), ("R", ctypes.c_void_p), ("Qf", ctypes.c_void_p), ("diagonal", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class LinearModel:
    """x+ = A x + B u (time-invariant), e.g. the LQ problem of the reference's iLQR test (tests/test_ilqrUtils.py:167-196)."""

    def __init__(self, A, B):
        self.A = np.ascontiguousarray(np.asarray(A, dtype=np.float64))
        self.B = np.ascontiguousarray(np.asarray(B, dtype=np.float64))
        self.n, self.m = self.B.shape
        if self.A.shape != (self.n, self.n):
            raise ValueError("A must be (n,n) and B (n,m)")
        self._dev = None

    def __call__(self, x, u):
        return self.A @ x + self.B @ u

    def c_struct(self):
        import torch
        if self._dev is None:
            self._dev = (arr.to_device(self.A, torch.float64), arr.to_device(self.B, torch.float64))
        st = zm_model_t(ZM_MODEL_LINEAR, self.n, self.m, 0, 0.0, self._dev[0].data_ptr(), self._dev[1].data_ptr())
        st._owner = self      # the struct holds raw device addresses: keep the arrays behind them alive with it
        return st


class QuadcopterEuler:
    """x+ = x + dt * Quadcopter.inertialDynamics(x, u)  (reference quadcopter.py:116-144; demos/iterativeLqr.py:35)."""
    n, m = 12, 4
    uTrim = np.array([9.807, 0.0, 0.0, 0.0])   # hover: thrust = g (quadcopter.py:15, tests/test_quadcopter.py:55-58)

    def __init__(self, dt: float = 0.1, wind_ned=(0.0, 0.0, 0.0)):
        """dt: Euler step; wind_ned: constant wind in the NED frame (quadcopter.py:117; demos/iterativeLqr.py:48)"""
        self.dt = float(dt)
        self.wind_ned = tuple(float(w) for w in wind_ned)
        if len(self.wind_ned) != 3:
            raise ValueError("wind_ned must have 3 components")

    def c_struct(self):
        return zm_model_t(ZM_MODEL_QUADCOPTER, 12, 4, 0, self.dt, None, None, (ctypes.c_double * 3)(*self.wind_ned))


class zm_traced_model_t(ctypes.Structure):
    """zm_model_t as ZM_MODEL_TRACED reads it: the same 64 bytes, the descriptor in place of A, B, wind_ned and the mask in `reserved`"""
    _fields_ = [("kind", ctypes.c_int), ("n", ctypes.c_int), ("m", ctypes.c_int), ("mask", ctypes.c_int),
                ("dt", ctypes.c_double), ("tape", ctypes.c_void_p), ("params", ctypes.c_void_p), ("param_stride", ctypes.c_int64),
                ("n_instr", ctypes.c_int32), ("n_const", ctypes.c_int32), ("n_slots", ctypes.c_int32), ("n_params", ctypes.c_int32)]


class TracedModel:
    """x+ = f(x, u) or f(x, u, p) for a user-written `f`: the callable is recorded ONCE on NumPy object arrays of recording scalars
    (zopt_amd/tape.py: `+ - * /`, unary minus, `** k`, np.sin / cos / tan / sqrt; no branches on the data) and the recording is
    evaluated by an interpreter inside the rollout, line-search, expansion and plant kernels on double, dual and hyper-dual numbers --
    the part jax.jit / jax.jacobian / jax.hessian play for the reference's callables (ilqrUtils.py:260-269).

    n, m: state and control dimensions (n <= 12, m <= 4).  params: None, (np,) -- one row shared by the batch -- or (..., np) with
    leading axes that broadcast to the batch of the call (as TrackingCost.xRef): per-problem constants, np <= 8; no derivative is
    taken with respect to them.  At most 1024 instructions, 64 live slots (inputs included) and 256 constants: ValueError beyond.

    Accepted wherever a registered model is by `iterativeLqr`, `differentialDynamicProgramming`, `forwardPass2`, `trajectoryRollout`,
    the simulator, `AffineDynamics` / `QuadraticDynamics` `.from_function` / `.from_trajectory` and `mpcUtils.modelStep`, with a
    `QuadraticCost`.  Not yet with a `TrackingCost`, inside an `InputBox` / `StateBox`, or in `ltvMpc.fromModel / relinearize /
    realTimeIteration`: those refuse it.  Called with numeric arrays it evaluates `f`."""

    def __init__(self, f, n, m, params=None):
        from . import tape as _tape
        if not callable(f):
            raise TypeError("TracedModel: f must be a callable f(x, u) or f(x, u, p)")
        self.f, self.n, self.m = f, int(n), int(m)
        self.params = None
        if params is not None:
            self.params = params if arr.is_torch(params) else np.asarray(params, dtype=np.float64)
            if len(self.params.shape) < 1 or self.params.shape[-1] < 1:
                raise ValueError(f"TracedModel: params has shape {tuple(self.params.shape)}, expected (np,) or (..., np)")
        self.n_params = 0 if self.params is None else int(self.params.shape[-1])
        self.tape = _tape.record(f, self.n, self.m, self.n_params)
        self._dev = {}

    def __call__(self, x, u, p=None):
        if self.n_params:
            if p is None:
                p = self.params.detach().cpu().numpy() if arr.is_torch(self.params) else self.params
                if p.ndim != 1:
                    raise ValueError("TracedModel: pass the parameter row p of this point (params has batch axes)")
            return self.f(x, u, p)
        return self.f(x, u)

    def c_struct(self, lead=None):
        """zm_model_t of kind ZM_MODEL_TRACED for a call with batch axes `lead` (None: a model without per-trajectory params)"""
        import torch
        from . import tape as _tape
        t = self.tape
        pdev, stride = None, 0
        if self.n_params and lead is None and not all(int(d) == 1 for d in tuple(self.params.shape)[:-1]):
            raise ValueError("TracedModel: params has batch axes; this call has no batch to match them with")   # (before the device)
        if self.n_params:
            shp = tuple(int(d) for d in self.params.shape)
            if all(d == 1 for d in shp[:-1]):
                key = "shared"
                if key not in self._dev:
                    self._dev[key] = arr.to_device(self.params, torch.float64).reshape(self.n_params).contiguous()
            else:
                key = tuple(int(d) for d in lead)
                if key not in self._dev:
                    full = key + (self.n_params,)
                    if len(shp) > len(full) or any(a != 1 and a != b for a, b in zip(shp[::-1], full[::-1])):
                        raise ValueError(f"TracedModel: leading axes {shp[:-1]} of params do not broadcast to the batch {key}")
                    self._dev[key] = arr.to_device(self.params, torch.float64).expand(full).reshape(-1, self.n_params).contiguous()
                stride = self.n_params
            pdev = self._dev[key]
        if "blob" not in self._dev:
            self._dev["blob"] = arr.to_device(_tape.blob(t).view(np.float64), torch.float64)
        blob = self._dev["blob"]
        st = zm_traced_model_t(ZM_MODEL_TRACED, self.n, self.m, t.mask, 0.0, blob.data_ptr(), None if pdev is None else pdev.data_ptr(),
                               stride, len(t.code), len(t.consts), t.n_slots, self.n_params)
        st._owner = (self, blob, pdev)      # raw device addresses: keep the arrays behind them alive with the struct
        return st


def model_struct(model, lead):
    """c_struct() of a registered model for a call with batch axes `lead` (a TracedModel's per-trajectory params need them)"""
    return model.c_struct(tuple(lead)) if isinstance(model, TracedModel) else model.c_struct()


def refuse_traced_constraint(model, who):
    """A TracedConstraint inside a box, refused before anything touches the device"""
    if isinstance(model, TracedConstraint):
        raise TypeError(f"{who}: a TracedConstraint takes no InputBox / StateBox around it -- clipped inputs and a state box next to "
                        "recorded constraints are the follow-up (write the bounds as rows of g)")


def refuse_traced(model, who, follow_up):
    """The combinations a TracedModel is not built for yet, refused before anything touches the device"""
    if isinstance(model, TracedModel):
        raise TypeError(f"{who}: a TracedModel is not supported here yet -- {follow_up}")


class QuadraticCost:
    """runningCost(x,u) = x'Qx + u'Ru, terminalCost(x) = x'Qf x  (demos/iterativeLqr.py:12-13,37; no 1/2)."""

    def __init__(self, Q, R, Qf=None):
        self.Q = np.ascontiguousarray(np.asarray(Q, dtype=np.float64))
        self.R = np.ascontiguousarray(np.asarray(R, dtype=np.float64))
        self.Qf = self.Q if Qf is None else np.ascontiguousarray(np.asarray(Qf, dtype=np.float64))
        self.n, self.m = self.Q.shape[0], self.R.shape[0]
        if self.Q.shape != (self.n, self.n) or self.R.shape != (self.m, self.m) or self.Qf.shape != (self.n, self.n):
            raise ValueError("QuadraticCost: Q (n,n), R (m,m), Qf (n,n) expected")
        self._dev = None

    def __call__(self, traj, k=None):
        """Cost of a trajectory, J = terminalCost(x_N) + sum_k runningCost(x_k, u_k) -- CostFunction.__call__ of the reference
        (pytrees.py:40-55); with `k`, the running cost at step k only.  Leading batch axes allowed; evaluated on the GPU."""
        from .pytrees import _expand
        c, _, _, _, _, _ = _expand("cost", self, traj[0] if not hasattr(traj, "xTraj") else traj.xTraj,
                                   traj[1] if not hasattr(traj, "uTraj") else traj.uTraj)
        if k is not None:
            return c[..., k]
        xT = traj.xTraj if hasattr(traj, "xTraj") else traj[0]
        v, _, _ = _expand("terminal", self, xT[..., -2:, :], None)
        J = c.sum(-1) + v[..., 0]
        return float(J) if (not hasattr(J, "device") and getattr(J, "ndim", 1) == 0) else J

    def runningCost(self, x, u):
        return x @ self.Q @ x + u @ self.R @ u

    def terminalCost(self, x):
        return x @ self.Qf @ x

    def c_struct(self):
        import torch
        if self._dev is None:
            self._dev = tuple(arr.to_device(X, torch.float64) for X in (self.Q, self.R, self.Qf))
        isdiag = lambda M: not np.any(M - np.diag(np.diagonal(M)))          # exact: also False for NaN off the diagonal
        diag = int(isdiag(self.Q) and isdiag(self.R) and isdiag(self.Qf))
        st = zm_quadcost_t(*[t.data_ptr() for t in self._dev], diag, 0)
        st._owner = self      # the struct holds raw device addresses: keep the arrays behind them alive with it
        return st


class zm_traced_t(ctypes.Structure):
    _fields_ = [("tape", ctypes.c_void_p), ("params", ctypes.c_void_p), ("param_stride", ctypes.c_int64), ("n_instr", ctypes.c_int32),
                ("n_const", ctypes.c_int32), ("n_slots", ctypes.c_int32), ("n_params", ctypes.c_int32)]


class zm_tracedcost_t(ctypes.Structure):
    _fields_ = [("running", zm_traced_t), ("terminal", zm_traced_t), ("n", ctypes.c_int32), ("m", ctypes.c_int32),
                ("running_mask", ctypes.c_uint32), ("terminal_mask", ctypes.c_uint32)]


class TracedCost:
    """runningCost(x, u) / terminalCost(x) for user-written callables (optionally with a parameter row: runningCost(x, u, p),
    terminalCost(x, p)), each returning a scalar: recorded ONCE by the recorder of `TracedModel` (zopt_amd/tape.py: `+ - * /`, unary
    minus, `** k`, np.sin / cos / tan / sqrt, indexing, np.array, np.concatenate, `@`, np.cross; no branches on the data) and evaluated
    by the tape interpreter inside the line-search and expansion kernels on double, dual and hyper-dual numbers -- the part the
    reference's cost callables play (ilqrUtils.py:260-269; demos/iterativeLqr.py:35-36).

    terminalCost=None is the reference's rule (pytrees.py:37): terminalCost(x) = runningCost(x, zeros(m)).  The result of a callable is a
    recorded scalar, a 0-d array or an array of exactly one element (ValueError otherwise).  params: None, (np,) or (..., np) with
    leading axes that broadcast to the batch of the call, as `TracedModel.params`: per-problem constants (a goal or an obstacle centre
    per trajectory), np <= 8, no derivative is taken with respect to them.  Caps per tape: 1024 instructions, 64 live slots (inputs
    included), 256 constants; n <= 12, m <= 4.

    Accepted -- the handle for both cost arguments, or its two bound methods, as a `QuadraticCost` -- with a registered model
    (`LinearModel` at n <= 12 and m <= 4, the quadcopters) or a `TracedModel` by `iterativeLqr`, `differentialDynamicProgramming`,
    `forwardPass2`, `cost(traj)` / `cost(traj, k)`, `QuadraticCostFunction.from_trajectory / from_function` and
    `QuadraticValueFunction.fromTerminalCostFunction`.  Refused (TypeError, before anything touches the device): together with an
    `InputBox` or a `StateBox`, on the generic torch-callable path, and with a model of another (n, m)."""

    def __init__(self, runningCost, terminalCost, n, m, params=None):
        from . import tape as _tape
        if not callable(runningCost) or not (terminalCost is None or callable(terminalCost)):
            raise TypeError("TracedCost: runningCost must be a callable c(x, u) or c(x, u, p), terminalCost a callable v(x) or v(x, p) "
                            "or None")
        self.n, self.m = int(n), int(m)
        self.params = None
        if params is not None:
            self.params = params if arr.is_torch(params) else np.asarray(params, dtype=np.float64)
            if len(self.params.shape) < 1 or self.params.shape[-1] < 1:
                raise ValueError(f"TracedCost: params has shape {tuple(self.params.shape)}, expected (np,) or (..., np)")
        self.n_params = 0 if self.params is None else int(self.params.shape[-1])
        self._running = runningCost
        if terminalCost is None:      # pytrees.py:37
            zeros = np.zeros(self.m)
            terminalCost = (lambda x, p: runningCost(x, zeros, p)) if self.n_params else (lambda x: runningCost(x, zeros))
        self._terminal = terminalCost
        self.running_tape = _tape.record(self._running, self.n, self.m, self.n_params, n_out=1, who="TracedCost")
        self.terminal_tape = _tape.record(self._terminal, self.n, self.m, self.n_params, n_out=1, controls=False, who="TracedCost")
        self._dev = {}

    def _row(self, p):
        if p is None:
            p = self.params.detach().cpu().numpy() if arr.is_torch(self.params) else self.params
            if p.ndim != 1:
                raise ValueError("TracedCost: pass the parameter row p of this point (params has batch axes)")
        return p

    def runningCost(self, x, u, p=None):
        """the callable itself on numeric arrays"""
        return self._running(x, u, self._row(p)) if self.n_params else self._running(x, u)

    def terminalCost(self, x, p=None):
        return self._terminal(x, self._row(p)) if self.n_params else self._terminal(x)

    def __call__(self, traj, k=None):
        """Cost of a trajectory, J = terminalCost(x_N) + sum_k runningCost(x_k, u_k) -- CostFunction.__call__ of the reference
        (pytrees.py:40-55); with `k`, the running cost at step k only.  Leading batch axes allowed; evaluated on the GPU, the sum in
        step order."""
        from .pytrees import _traced_cost_values
        xT = traj.xTraj if hasattr(traj, "xTraj") else traj[0]
        uT = traj.uTraj if hasattr(traj, "uTraj") else traj[1]
        c, v = _traced_cost_values(self, xT, uT)
        if k is not None:
            return c[..., k]
        J = 0.0 + c[..., 0]                           # J = (((0 + c_0) + c_1) + ...) + v: the line search's order
        for i in range(1, c.shape[-1]):
            J = J + c[..., i]
        J = J + v
        return float(J) if (not hasattr(J, "device") and getattr(J, "ndim", 1) == 0) else J

    def tcost_struct(self, lead=None):
        """zm_tracedcost_t for a call with batch axes `lead` (None: a cost without per-trajectory params)"""
        import torch
        from . import tape as _tape
        pdev, stride = None, 0
        if self.n_params:
            shp = tuple(int(d) for d in self.params.shape)
            if all(d == 1 for d in shp[:-1]):
                key = "shared"
                if key not in self._dev:
                    self._dev[key] = arr.to_device(self.params, torch.float64).reshape(self.n_params).contiguous()
            else:
                if lead is None:
                    raise ValueError("TracedCost: params has batch axes; this call has no batch to match them with")
                key = tuple(int(d) for d in lead)
                if key not in self._dev:
                    full = key + (self.n_params,)
                    if len(shp) > len(full) or any(a != 1 and a != b for a, b in zip(shp[::-1], full[::-1])):
                        raise ValueError(f"TracedCost: leading axes {shp[:-1]} of params do not broadcast to the batch {key}")
                    self._dev[key] = arr.to_device(self.params, torch.float64).expand(full).reshape(-1, self.n_params).contiguous()
                stride = self.n_params
            pdev = self._dev[key]
        if "blobs" not in self._dev:
            self._dev["blobs"] = tuple(arr.to_device(_tape.blob(t).view(np.float64), torch.float64)
                                       for t in (self.running_tape, self.terminal_tape))
        blobs = self._dev["blobs"]
        pp = None if pdev is None else pdev.data_ptr()
        tapes = [zm_traced_t(b.data_ptr(), pp, stride, len(t.code), len(t.consts), t.n_slots, self.n_params)
                 for b, t in zip(blobs, (self.running_tape, self.terminal_tape))]
        st = zm_tracedcost_t(tapes[0], tapes[1], self.n, self.m, self.running_tape.mask, self.terminal_tape.mask)
        st._owner = (self, blobs, pdev)      # raw device addresses: keep the arrays behind them alive with the struct
        return st


def traced_cost_of(runningCost, terminalCost=None):
    """The TracedCost behind a cost argument (the handle or one of its bound methods), else None"""
    for c in (runningCost, getattr(runningCost, "__self__", None), terminalCost, getattr(terminalCost, "__self__", None)):
        if isinstance(c, TracedCost):
            return c
    return None


def check_traced_cost(cost, model, who, box=None, sbox=None):
    """What a TracedCost is not built for, refused with a TypeError before anything touches the device"""
    if box is not None or sbox is not None:
        raise TypeError(f"{who}: a TracedCost takes no InputBox / StateBox yet -- the clipped line search, the box-QP sweep and the "
                        "augmented-Lagrangian penalty next to a recorded cost are the follow-up")
    if not hasattr(model, "c_struct"):
        raise TypeError(f"{who}: a TracedCost needs a registered device model or a TracedModel -- its callables are written on NumPy "
                        "arrays, not torch, so the generic torch-callable path cannot differentiate them (write the dynamics as a "
                        "models.TracedModel; a torch restatement of the cost on the generic path is the alternative)")
    if (model.n, model.m) != (cost.n, cost.m):
        raise TypeError(f"{who}: the TracedCost is (n={cost.n}, m={cost.m}), the model (n={model.n}, m={model.m}) -- record the cost for "
                        "the model's shape")
    if model.n > 12 or model.m > 4:
        raise TypeError(f"{who}: a TracedCost covers n <= 12, m <= 4 (the tape interpreter's caps); larger linear models are the follow-up")


class zm_trackcost_t(ctypes.Structure):
    _fields_ = [("Q", ctypes.c_void_p), ("R", ctypes.c_void_p), ("Qf", ctypes.c_void_p), ("diagonal", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("xRef", ctypes.c_void_p), ("uRef", ctypes.c_void_p),
                ("xref_traj_stride", ctypes.c_int64), ("xref_step_stride", ctypes.c_int64),
                ("uref_traj_stride", ctypes.c_int64), ("uref_step_stride", ctypes.c_int64)]


TRACKING_MAX_N, TRACKING_MAX_M = 12, 4     # the fused drivers' shapes (zm::MAXN, zm::MAXM)


class TrackingCost:
    """The quadratic cost about a goal or a reference trajectory (no 1/2, as QuadraticCost):

        J = sum_{k<T} (x_k - xr_k)'Q(x_k - xr_k) + (u_k - ur_k)'R(u_k - ur_k)  +  (x_T - xr_T)'Qf(x_T - xr_T)

    xRef: None (zeros), (n,) -- one goal for every step and trajectory -- or (..., T+1, n) with leading axes that broadcast to the
    batch of the call; the step axis may have length 1 (`goal[:, None, :]`: a goal per trajectory, read with a step stride of 0, not
    materialised per step).  uRef: None, (m,) or (..., T, m), likewise.  NumPy arrays or device tensors; a device tensor that is
    contiguous in its trailing axes is read in place.  The reference's drivers take cost callables (ilqrUtils.py:260-269); this is
    the registered form of `lambda x, u, k: (x - xr[k]) @ Q @ (x - xr[k]) + ...` for the fused drivers, accepted wherever
    QuadraticCost is.  It is deliberately NOT a QuadraticCost: code that knows only that class would drop the reference."""

    def __init__(self, Q, R, Qf=None, xRef=None, uRef=None):
        self._w = QuadraticCost(Q, R, Qf)
        self.Q, self.R, self.Qf, self.n, self.m = self._w.Q, self._w.R, self._w.Qf, self._w.n, self._w.m
        self.xRef = self._checked(xRef, self.n, "xRef")
        self.uRef = self._checked(uRef, self.m, "uRef")

    @staticmethod
    def _checked(r, width, what):
        if r is None:
            return None
        if not arr.is_torch(r):
            r = np.asarray(r, dtype=np.float64)
        shp = tuple(r.shape)
        if len(shp) == 0 or shp[-1] != width or (len(shp) >= 2 and shp[-2] < 1):
            raise ValueError(f"TrackingCost: {what} has shape {shp}, expected ({width},) or (..., steps, {width})")
        return r

    # ---- host side (NumPy; a single trajectory or point) -------------------------------------------------------------------------
    def _row(self, r, k, width):
        if r is None:
            return np.zeros(width)
        r = r.detach().cpu().numpy() if arr.is_torch(r) else r
        if r.ndim == 1:
            return r
        if r.ndim != 2:
            raise ValueError("TrackingCost: the single-point form needs a reference without batch axes")
        return r[0 if r.shape[0] == 1 else k]

    def runningCost(self, x, u, k=0):
        ex, eu = x - self._row(self.xRef, k, self.n), u - self._row(self.uRef, k, self.m)
        return ex @ self.Q @ ex + eu @ self.R @ eu

    def terminalCost(self, x):
        ex = x - self._row(self.xRef, -1, self.n)
        return ex @ self.Qf @ ex

    def __call__(self, traj, k=None):
        """Cost of a trajectory (CostFunction.__call__ of the reference, pytrees.py:40-55); with `k`, the running cost at step k."""
        return QuadraticCost.__call__(self, traj, k)

    # ---- device side -----------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _view(r, lead, rows, width, what, terminal):
        """-> (device tensor or None, trajectory stride, step stride, offset) of a reference for a call with batch axes `lead` and
        `rows` steps.  Only a reference whose leading axes broadcast PARTLY to `lead` is copied (per trajectory, never per step)."""
        import torch
        if r is None:
            return None, 0, 0, 0
        in_place = arr.is_torch(r) and r.is_cuda and r.dtype == torch.float64 and r.stride(-1) == 1 and (
            r.ndim == 1 or r.shape[-2] == 1 or r.stride(-2) in (0, width))
        t = r if in_place else arr.to_device(r, torch.float64)
        if t.ndim == 1:
            return t.contiguous(), 0, 0, 0
        have = int(t.shape[-2])
        if terminal:              # the terminal row of the cost's own horizon
            rows = have
        if have not in (1, rows):
            raise ValueError(f"TrackingCost: {what} has {have} steps, the call needs {rows} (or 1)")
        if have > 1 and t.stride(-2) == 0:
            t, have = t[..., :1, :], 1
        ls = tuple(int(d) for d in t.shape[:-2])
        if len(ls) > len(lead) or any(a != 1 and a != b for a, b in zip(ls[::-1], tuple(lead)[::-1])):
            raise ValueError(f"TrackingCost: leading axes {ls} of {what} do not broadcast to the batch {tuple(lead)}")
        if all(d == 1 for d in ls):
            t, ts = t.reshape(have, width).contiguous(), 0
        elif ls == tuple(lead) and len(ls) == 1 and t.stride(-1) == 1 and (have == 1 or t.stride(-2) == width):
            ts = int(t.stride(0))          # one batch axis: any trajectory stride is read in place
        elif ls == tuple(lead):
            t, ts = t.contiguous(), have * width
        else:
            t, ts = t.expand(tuple(lead) + (have, width)).contiguous(), have * width
        ss = width if have > 1 else 0
        return t, ts, ss, ((have - 1) * ss if terminal else 0)

    def track_struct(self, lead, N, terminal=False):
        """zm_trackcost_t for a call with batch axes `lead` and N steps.  terminal: every row is the reference's LAST one (the terminal
        cost about xr_T evaluated on a short trajectory; uRef is not read)."""
        if self.n > TRACKING_MAX_N or self.m > TRACKING_MAX_M:
            raise ValueError(f"TrackingCost: (n={self.n}, m={self.m}) not covered -- the fused drivers take n <= {TRACKING_MAX_N}, "
                             f"m <= {TRACKING_MAX_M}; the wide rollouts have no tracking form")
        w = self._w.c_struct()
        xr, xts, xss, xoff = self._view(self.xRef, lead, N + 1, self.n, "xRef", terminal)
        ur, uts, uss, _ = (None, 0, 0, 0) if terminal else self._view(self.uRef, lead, N, self.m, "uRef", False)
        st = zm_trackcost_t(w.Q, w.R, w.Qf, w.diagonal, 0, xr.data_ptr() + 8 * xoff if xr is not None else None,
                            ur.data_ptr() if ur is not None else None, xts, 0 if terminal else xss, uts, uss)
        st._owner = (self, w, xr, ur)      # raw device addresses: keep the arrays behind them alive with the struct
        return st


class QuadcopterRigidBody:
    """The 8-state model the reference trims and linearises: `rigidBodyDynamics(state, control, wind_body)`
    (quadcopter.py:70-113), state [u,v,w,p,q,r,phi,theta].  dt = 0: the continuous derivative; dt > 0: one Euler step."""
    n, m = 8, 4

    def __init__(self, dt: float = 0.0, wind_body=(0.0, 0.0, 0.0)):
        self.dt = float(dt)
        self.wind_body = tuple(float(w) for w in wind_body)
        if len(self.wind_body) != 3:
            raise ValueError("wind_body must have 3 components")

    def c_struct(self):
        return zm_model_t(ZM_MODEL_QUADCOPTER_RB, 8, 4, 0, self.dt, None, None, (ctypes.c_double * 3)(*self.wind_body))


class Quadcopter:
    """Mirror of `zopt.quadcopter.Quadcopter` (quadcopter.py:10-201) on the device kernels: same method names and argument order,
    every array may carry leading batch axes (a family of operating points in one call)."""
    g, m, I = 9.807, 2.5, np.eye(3)         # quadcopter.py:15-18 (compiled into the device model)

    def rigidBodyDynamics(self, state, control, wind_body=(0.0, 0.0, 0.0)):
        """xDot (..., 8) of the rigid-body model (quadcopter.py:70-113)."""
        from .pytrees import AffineDynamics
        return AffineDynamics.from_function(QuadcopterRigidBody(0.0, wind_body), state, control).f

    def inertialDynamics(self, state, control, wind_ned=(0.0, 0.0, 0.0)):
        """xDot (..., 12) with position states (quadcopter.py:116-144)."""
        from .pytrees import AffineDynamics
        return AffineDynamics.from_function(QuadcopterEuler(0.0, wind_ned), state, control).f

    def trim(self, uvwTrim, tol=1e-9):
        """Trim at the body velocities uvwTrim (..., 3) (quadcopter.py:146-177) -> (xTrim (..., 8), uTrim (..., 4)).
        Raises RuntimeError("Trim failed") like the reference when an instance does not reach |rigidBodyDynamics| <= 1e-3."""
        import torch
        from . import _arrays as arr
        from . import _lib
        v = arr.to_device(uvwTrim, torch.float64)
        lead = tuple(v.shape[:-1])
        if v.shape[-1] != 3:
            raise ValueError("uvwTrim must have shape (..., 3)")
        v = v.reshape(-1, 3).contiguous()
        b = v.shape[0]
        xT = torch.empty((b, 8), dtype=torch.float64, device=v.device)
        uT = torch.empty((b, 4), dtype=torch.float64, device=v.device)
        res = torch.empty(b, dtype=torch.float64, device=v.device)
        rc = _lib.lib().zm_quadcopter_trim_f64(v.data_ptr(), None, xT.data_ptr(), uT.data_ptr(), res.data_ptr(), None, b, float(tol),
                                               ctypes.c_void_p(arr.stream_ptr(v)))
        _lib.check(rc, "Quadcopter.trim")
        if b and float(res.max()) > 1e-3:
            raise RuntimeError("Trim failed")
        return arr.result_like(xT.reshape(lead + (8,)), uvwTrim), arr.result_like(uT.reshape(lead + (4,)), uvwTrim)

    def linearize(self, x0, u0, dt=0):
        """Linearise the rigid-body dynamics about (x0 (..., 8), u0 (..., 4)) (quadcopter.py:179-201): continuous (A, B) for
        dt = 0, forward-Euler discretised `I + dt A`, `dt B` otherwise."""
        from .pytrees import AffineDynamics
        lin = AffineDynamics.from_function(QuadcopterRigidBody(float(dt)), x0, u0)
        return lin.f_x, lin.f_u


class zm_inputbox_t(ctypes.Structure):
    # (step_stride trails: a struct built from three fields leaves it zero, the constant form)
    _fields_ = [("lb", ctypes.c_void_p), ("ub", ctypes.c_void_p), ("stride", ctypes.c_int64), ("step_stride", ctypes.c_int64)]


INPUTBOX_MAX_N, INPUTBOX_MAX_M = 12, 4     # the fused drivers' shapes (zm::MAXN, zm::MAXM)


class InputBox:
    """A registered model with bounds on its inputs, `u_lb <= u <= u_ub` per component: control-limited iLQR (Tassa, Mansard, Todorov
    2014).  An extension: the reference's iLQR is unconstrained (ilqrUtils.py:260-327).

    u_lb, u_ub: scalars, (m,) or (..., m) with leading axes that broadcast to the batch of the call; an entry of -inf / +inf means no
    bound on that side of that component, `u_lb == u_ub` fixes a component.  `u_lb > u_ub` and NaN are refused.

    stage_varying=True: the bounds change along the horizon.  Each bound is (N, m) or (..., N, m) -- row k is the box of `u_k`, N the
    horizon of every call the box is used in, the leading axes broadcast to the batch -- or a scalar (the other bound then carries the
    step axis).  Rows with `u_lb == u_ub` pin inputs that are committed already (delay compensation), a row of zeros is a cut-off.
    A call with another horizon is a ValueError; a `StateBox` around a stage-varying box is a TypeError (the follow-up).

    Accepted wherever a registered model is by `iterativeLqr`, `differentialDynamicProgramming` (quadcopter models), `forwardPass2`,
    `trajectoryRollout` and the simulator: rollouts clip
    `u_k = clip(alpha l_k + L_k (x_k - xPrev_k) + uPrev_k, u_lb, u_ub)`, the backward pass solves a box-constrained QP per step and
    zeroes the feedback rows of the clamped inputs.  It is deliberately neither callable nor a device model itself: code that knows
    nothing of the box (the expansions, the generic-callable path) refuses it instead of dropping the bounds."""

    def __init__(self, model, u_lb, u_ub, stage_varying=False):
        if isinstance(model, InputBox):
            raise TypeError("InputBox: the model is an InputBox already")
        if isinstance(model, StateBox):
            raise TypeError("InputBox: a StateBox is the outer wrapper -- write StateBox(InputBox(model, u_lb, u_ub), x_lb, x_ub)")
        refuse_traced_constraint(model, "InputBox")
        refuse_traced(model, "InputBox", "the box-QP line search and sweeps on the tape interpreter are the follow-up")
        if not hasattr(model, "c_struct"):
            raise TypeError("InputBox wraps a registered device model (zopt_amd.models.*); the generic-callable path has no box: clip "
                            "inside the torch callable there")
        self.model, self.n, self.m = model, int(model.n), int(model.m)
        if self.n > INPUTBOX_MAX_N or self.m > INPUTBOX_MAX_M:
            raise ValueError(f"InputBox: (n={self.n}, m={self.m}) not covered -- the box kernels take n <= {INPUTBOX_MAX_N}, "
                             f"m <= {INPUTBOX_MAX_M}")
        self._set_bounds(u_lb, u_ub, stage_varying)

    @classmethod
    def for_shape(cls, n, m, u_lb, u_ub, stage_varying=False):
        """the bounds alone, for array-level calls that have no model (ilqrUtils.backwardPass_ilqr_box)"""
        self = cls.__new__(cls)
        self.model, self.n, self.m = None, int(n), int(m)
        self._set_bounds(u_lb, u_ub, stage_varying)
        return self

    def _set_bounds(self, u_lb, u_ub, stage_varying=False):
        host = lambda b: np.asarray(b.detach().cpu().numpy() if arr.is_torch(b) else b, dtype=np.float64)       # noqa: E731
        lb, ub = host(u_lb), host(u_ub)
        self.stage_varying = bool(stage_varying)
        if self.stage_varying:
            return self._set_stage_bounds(lb, ub)
        for name, b in (("u_lb", lb), ("u_ub", ub)):
            if b.ndim and b.shape[-1] != self.m:
                raise ValueError(f"InputBox: {name} has shape {b.shape}, expected a scalar, ({self.m},) or (..., {self.m})")
            if np.isnan(b).any():
                raise ValueError(f"InputBox: {name} holds a NaN")
        try:
            shp = np.broadcast_shapes(lb.shape, ub.shape, (self.m,))
        except ValueError:
            raise ValueError(f"InputBox: u_lb {lb.shape} and u_ub {ub.shape} do not broadcast") from None
        self.u_lb, self.u_ub = np.array(np.broadcast_to(lb, shp)), np.array(np.broadcast_to(ub, shp))
        if (self.u_lb > self.u_ub).any():
            raise ValueError("InputBox: u_lb > u_ub")
        self._dev = {}

    def _set_stage_bounds(self, lb, ub):
        """stage_varying=True: u_lb, u_ub (N, m) or (..., N, m), or a scalar next to such an array"""
        for name, b in (("u_lb", lb), ("u_ub", ub)):
            if b.ndim and (b.ndim < 2 or b.shape[-1] != self.m):
                raise ValueError(f"InputBox: stage-varying {name} has shape {b.shape}, expected a scalar, (N, {self.m}) or (..., N, {self.m})")
            if np.isnan(b).any():
                raise ValueError(f"InputBox: {name} holds a NaN")
        if lb.ndim == 0 and ub.ndim == 0:
            raise ValueError("InputBox: stage-varying bounds need a step axis -- u_lb or u_ub of shape (N, m) or (..., N, m)")
        if lb.ndim and ub.ndim and lb.shape[-2] != ub.shape[-2]:
            raise ValueError(f"InputBox: u_lb has {lb.shape[-2]} steps and u_ub {ub.shape[-2]}")
        try:
            shp = np.broadcast_shapes(lb.shape, ub.shape)
        except ValueError:
            raise ValueError(f"InputBox: u_lb {lb.shape} and u_ub {ub.shape} do not broadcast") from None
        if shp[-2] < 1:
            raise ValueError("InputBox: stage-varying bounds need at least one step")
        self.u_lb, self.u_ub = np.array(np.broadcast_to(lb, shp)), np.array(np.broadcast_to(ub, shp))
        self.steps = int(shp[-2])
        bad = self.u_lb > self.u_ub
        if bad.any():
            raise ValueError(f"InputBox: u_lb > u_ub at step {int(np.argwhere(bad)[0][-2])}")
        self._dev = {}

    def clip(self, u):
        """u clipped into the box (NumPy, host side); stage-varying bounds: u (..., N, m), row k into the box of step k"""
        return np.minimum(np.maximum(u, self.u_lb), self.u_ub)

    def check_horizon(self, T):
        """stage-varying bounds: the call's horizon is the bounds' step axis (checked by the drivers before anything touches the device)"""
        if self.stage_varying and (T is None or int(T) != self.steps):
            raise ValueError(f"InputBox: the stage-varying bounds have {self.steps} steps, the call has a horizon of {T}")

    def box_struct(self, lead, T=None):
        """zm_inputbox_t for a call with batch axes `lead` and horizon `T`: one shared row (stride 0) or a row per trajectory (stride m);
        stage-varying bounds: (T, m) rows, one schedule shared (stride 0) or one per trajectory (stride T m), step_stride m.  The device
        copy is made once per `lead` and kept."""
        import torch
        lead = tuple(int(d) for d in lead)
        self.check_horizon(T)
        if self.stage_varying:
            if lead not in self._dev:
                if self.u_lb.ndim == 2:
                    rows, stride = (self.u_lb, self.u_ub), 0
                else:
                    try:
                        rows = tuple(np.array(np.broadcast_to(b, lead + (self.steps, self.m))) for b in (self.u_lb, self.u_ub))
                    except ValueError:
                        raise ValueError(f"InputBox: leading axes {self.u_lb.shape[:-2]} of the bounds do not broadcast to the batch "
                                         f"{lead}") from None
                    stride = self.steps * self.m
                self._dev[lead] = tuple(arr.to_device(np.ascontiguousarray(b), torch.float64) for b in rows) + (stride,)
            lb, ub, stride = self._dev[lead]
            st = zm_inputbox_t(lb.data_ptr(), ub.data_ptr(), stride, self.m)
            st._owner = (self, lb, ub)
            return st
        if lead not in self._dev:
            if self.u_lb.ndim == 1:
                rows, stride = (self.u_lb, self.u_ub), 0
            else:
                try:
                    rows = tuple(np.array(np.broadcast_to(b, lead + (self.m,))) for b in (self.u_lb, self.u_ub))
                except ValueError:
                    raise ValueError(f"InputBox: leading axes {self.u_lb.shape[:-1]} of the bounds do not broadcast to the batch "
                                     f"{lead}") from None
                stride = self.m
            self._dev[lead] = tuple(arr.to_device(np.ascontiguousarray(b), torch.float64) for b in rows) + (stride,)
        lb, ub, stride = self._dev[lead]
        st = zm_inputbox_t(lb.data_ptr(), ub.data_ptr(), stride)
        st._owner = (self, lb, ub)      # raw device addresses: keep the arrays behind them alive with the struct
        return st


class zm_statebox_t(ctypes.Structure):
    _fields_ = [("lb", ctypes.c_void_p), ("ub", ctypes.c_void_p), ("stride", ctypes.c_int64), ("lam_lb", ctypes.c_void_p),
                ("lam_ub", ctypes.c_void_p), ("mu", ctypes.c_void_p)]


STATEBOX_MAX_N, STATEBOX_MAX_M = 12, 4     # the fused drivers' shapes (zm::MAXN, zm::MAXM)


class StateBox:
    """A registered model (or an `InputBox` around one) with bounds on its states, `x_lb <= x_k <= x_ub` per component for
    k = 1..N (x_0 is given): iLQR with an augmented-Lagrangian outer loop (AL-iLQR).  An extension: the reference's iLQR is
    unconstrained (ilqrUtils.py:260-327).

    x_lb, x_ub: scalars, (n,) or (..., n) with leading axes that broadcast to the batch of the call; an entry of -inf / +inf means no
    bound on that side of that component, `x_lb == x_ub` pins a component.  `x_lb > x_ub` and NaN are refused.
    mu0, growth, mu_max: the penalty starts at mu0 and grows by `growth` per outer iteration up to mu_max; outer: at most that many
    outer iterations; ctol: a trajectory is done when its inner solve converged and its largest violation is <= ctol.

    Accepted by `iterativeLqr` and `constrainedIterativeLqr`.  `trajectoryRollout` and the simulator unwrap it (the dynamics are
    unchanged; an inner InputBox still clips); `forwardPass2` and `differentialDynamicProgramming` refuse it.  An InputBox around a
    StateBox is a TypeError: the state box is the outer wrapper."""

    def __init__(self, model, x_lb, x_ub, mu0=1.0, growth=10.0, mu_max=1e8, outer=10, ctol=1e-4):
        if isinstance(model, StateBox):
            raise TypeError("StateBox: the model is a StateBox already")
        refuse_traced_constraint(model, "StateBox")
        inner = model.model if isinstance(model, InputBox) else model
        if isinstance(model, InputBox) and model.stage_varying:
            raise TypeError("StateBox: a stage-varying InputBox inside a StateBox is the follow-up -- the penalty line search and sweep "
                            "take one input box for the whole horizon")
        refuse_traced(inner, "StateBox", "the augmented-Lagrangian line search on the tape interpreter is the follow-up")
        if not hasattr(inner, "c_struct"):
            raise TypeError("StateBox wraps a registered device model (zopt_amd.models.*) or an InputBox around one; the "
                            "generic-callable path has no state box")
        self.model, self.n, self.m = model, int(inner.n), int(inner.m)
        if self.n > STATEBOX_MAX_N or self.m > STATEBOX_MAX_M:
            raise ValueError(f"StateBox: (n={self.n}, m={self.m}) not covered -- the state-box kernels take n <= {STATEBOX_MAX_N}, "
                             f"m <= {STATEBOX_MAX_M}")
        self.mu0, self.growth, self.mu_max, self.outer, self.ctol = float(mu0), float(growth), float(mu_max), int(outer), float(ctol)
        if not self.mu0 > 0 or not self.growth >= 1 or not self.mu_max >= self.mu0 or self.outer < 1 or not self.ctol >= 0:
            raise ValueError("StateBox: need mu0 > 0, growth >= 1, mu_max >= mu0, outer >= 1, ctol >= 0")
        host = lambda b: np.asarray(b.detach().cpu().numpy() if arr.is_torch(b) else b, dtype=np.float64)       # noqa: E731
        lb, ub = host(x_lb), host(x_ub)
        for name, b in (("x_lb", lb), ("x_ub", ub)):
            if b.ndim and b.shape[-1] != self.n:
                raise ValueError(f"StateBox: {name} has shape {b.shape}, expected a scalar, ({self.n},) or (..., {self.n})")
            if np.isnan(b).any():
                raise ValueError(f"StateBox: {name} holds a NaN")
        try:
            shp = np.broadcast_shapes(lb.shape, ub.shape, (self.n,))
        except ValueError:
            raise ValueError(f"StateBox: x_lb {lb.shape} and x_ub {ub.shape} do not broadcast") from None
        self.x_lb, self.x_ub = np.array(np.broadcast_to(lb, shp)), np.array(np.broadcast_to(ub, shp))
        if (self.x_lb > self.x_ub).any():
            raise ValueError("StateBox: x_lb > x_ub")
        self._dev = {}

    def bounds_rows(self, lead):
        """(x_lb, x_ub, stride) as host arrays for a call with batch axes `lead`: one shared row (stride 0) or a row per trajectory
        (stride n)"""
        lead = tuple(int(d) for d in lead)
        if self.x_lb.ndim == 1:
            return self.x_lb, self.x_ub, 0
        try:
            lb, ub = (np.array(np.broadcast_to(b, lead + (self.n,))).reshape(-1, self.n) for b in (self.x_lb, self.x_ub))
        except ValueError:
            raise ValueError(f"StateBox: leading axes {self.x_lb.shape[:-1]} of the bounds do not broadcast to the batch {lead}") from None
        return lb, ub, self.n

    def statebox_struct(self, lead, lam_lb, lam_ub, mu):
        """zm_statebox_t for a call with batch axes `lead` on the caller's device arrays for the multipliers and the penalty"""
        import torch
        lead = tuple(int(d) for d in lead)
        if lead not in self._dev:
            lb, ub, stride = self.bounds_rows(lead)
            self._dev[lead] = tuple(arr.to_device(np.ascontiguousarray(b), torch.float64) for b in (lb, ub)) + (stride,)
        lb, ub, stride = self._dev[lead]
        st = zm_statebox_t(lb.data_ptr(), ub.data_ptr(), stride, lam_lb.data_ptr(), lam_ub.data_ptr(), mu.data_ptr())
        st._owner = (self, lb, ub, lam_lb, lam_ub, mu)      # raw device addresses: keep the arrays behind them alive with the struct
        return st


class zm_tracedcon_t(ctypes.Structure):
    _fields_ = [("stage", zm_traced_t), ("terminal", zm_traced_t), ("n", ctypes.c_int32), ("m", ctypes.c_int32),
                ("n_con", ctypes.c_int32), ("n_con_terminal", ctypes.c_int32), ("lam", ctypes.c_void_p),
                ("lam_terminal", ctypes.c_void_p), ("mu", ctypes.c_void_p)]


TRACEDCON_MAX = 8     # rows per tape (ZM_TRACEDCON_MAX)


class TracedConstraint:
    """A registered model or a `TracedModel` with user-written inequality constraints: `g(x, u)` or `g(x, u, p)` returns `n_con`
    values, enforced as `g <= 0` at every stage k = 0..N-1 on (x_k, u_k) (stage 0 included: u_0 is free); `terminal(x)` or
    `terminal(x, p)` returns `n_con_terminal` values, enforced on x_N.  At least one of the two is given (`g=None`: n_con = 0).  Both
    are recorded ONCE by the recorder of `TracedModel` (zopt_amd/tape.py: `+ - * /`, unary minus, `** k`, np.sin / cos / tan / sqrt,
    indexing, np.array, np.concatenate, `@`, np.cross; no branches on the data) and evaluated by the tape interpreter inside the
    line-search, expansion and multiplier-update kernels of an augmented-Lagrangian loop around the fused iLQR (AL-iLQR, as `StateBox`):
    penalty sum_i (pos(lam_i + mu g_i)^2 - lam_i^2) / (2 mu), its gradient G^T pos(s) and Gauss-Newton Hessian mu G^T diag(s > 0) G on
    dual numbers (no second derivatives of g).  An extension: the reference's iLQR is unconstrained (ilqrUtils.py:260-327).

    params: None, (np,) or (..., np) with leading axes that broadcast to the batch of the call, as `TracedCost.params`: per-problem
    constants (an obstacle centre and radius per trajectory), np <= 8.  Caps: those of `TracedModel` per tape (n <= 12, m <= 4, 1024
    instructions, 64 live slots, 256 constants), n_con <= 8, n_con_terminal <= 8: ValueError beyond.
    mu0, growth, mu_max, outer, ctol: as `StateBox`.

    Accepted by `iterativeLqr` and `constrainedIterativeLqr` with a `QuadraticCost` or (registered models) a `TrackingCost`.
    `trajectoryRollout` and the simulator unwrap it.  Refused (the follow-up): `differentialDynamicProgramming`, `forwardPass2`, a
    `TracedCost` next to it, an `InputBox` or `StateBox` inside or around it, the generic torch-callable path."""

    def __init__(self, model, g, n_con, terminal=None, n_con_terminal=0, params=None, mu0=1.0, growth=10.0, mu_max=1e8, outer=10,
                 ctol=1e-4):
        from . import tape as _tape
        if isinstance(model, (InputBox, StateBox, TracedConstraint)):
            raise TypeError("TracedConstraint: an InputBox / StateBox / TracedConstraint inside a TracedConstraint is the follow-up -- "
                            "the penalty line search takes no clipped inputs and no second penalty (write the bounds as rows of g)")
        if not hasattr(model, "c_struct"):
            raise TypeError("TracedConstraint wraps a registered device model (zopt_amd.models.*) or a TracedModel; constraints on the "
                            "generic torch-callable path are the follow-up")
        if g is None and terminal is None:
            raise ValueError("TracedConstraint: give g, terminal, or both")
        if not (g is None or callable(g)) or not (terminal is None or callable(terminal)):
            raise TypeError("TracedConstraint: g must be a callable g(x, u) or g(x, u, p), terminal a callable t(x) or t(x, p), or None")
        self.model, self.n, self.m = model, int(model.n), int(model.m)
        self.n_con = 0 if g is None else int(n_con)
        self.n_con_terminal = 0 if terminal is None else int(n_con_terminal)
        if g is not None and not 1 <= self.n_con <= TRACEDCON_MAX:
            raise ValueError(f"TracedConstraint: n_con = {self.n_con}, need 1 <= n_con <= {TRACEDCON_MAX}")
        if terminal is not None and not 1 <= self.n_con_terminal <= TRACEDCON_MAX:
            raise ValueError(f"TracedConstraint: n_con_terminal = {self.n_con_terminal}, need 1 <= n_con_terminal <= {TRACEDCON_MAX}")
        self.mu0, self.growth, self.mu_max, self.outer, self.ctol = float(mu0), float(growth), float(mu_max), int(outer), float(ctol)
        if not self.mu0 > 0 or not self.growth >= 1 or not self.mu_max >= self.mu0 or self.outer < 1 or not self.ctol >= 0:
            raise ValueError("TracedConstraint: need mu0 > 0, growth >= 1, mu_max >= mu0, outer >= 1, ctol >= 0")
        self.params = None
        if params is not None:
            self.params = params if arr.is_torch(params) else np.asarray(params, dtype=np.float64)
            if len(self.params.shape) < 1 or self.params.shape[-1] < 1:
                raise ValueError(f"TracedConstraint: params has shape {tuple(self.params.shape)}, expected (np,) or (..., np)")
        self.n_params = 0 if self.params is None else int(self.params.shape[-1])
        self._g, self._terminal = g, terminal
        self.stage_tape = None if g is None else _tape.record(g, self.n, self.m, self.n_params, n_out=self.n_con, who="TracedConstraint")
        self.terminal_tape = None if terminal is None else _tape.record(terminal, self.n, self.m, self.n_params,
                                                                        n_out=self.n_con_terminal, controls=False,
                                                                        who="TracedConstraint")
        self._dev = {}

    def _row(self, p):
        if p is None:
            p = self.params.detach().cpu().numpy() if arr.is_torch(self.params) else self.params
            if p.ndim != 1:
                raise ValueError("TracedConstraint: pass the parameter row p of this point (params has batch axes)")
        return p

    def g(self, x, u, p=None):
        """the stage callable itself on numeric arrays"""
        return np.asarray(self._g(x, u, self._row(p)) if self.n_params else self._g(x, u), dtype=np.float64).reshape(-1)

    def terminal(self, x, p=None):
        return np.asarray(self._terminal(x, self._row(p)) if self.n_params else self._terminal(x), dtype=np.float64).reshape(-1)

    def con_struct(self, lead, lam=None, lam_terminal=None, mu=None):
        """zm_tracedcon_t for a call with batch axes `lead` on the caller's device arrays for the multipliers and the penalty (None:
        a call that reads none of them)"""
        import torch
        from . import tape as _tape
        pdev, stride = None, 0
        if self.n_params:
            shp = tuple(int(d) for d in self.params.shape)
            if all(d == 1 for d in shp[:-1]):
                key = "shared"
                if key not in self._dev:
                    self._dev[key] = arr.to_device(self.params, torch.float64).reshape(self.n_params).contiguous()
            else:
                key = tuple(int(d) for d in lead)
                if key not in self._dev:
                    full = key + (self.n_params,)
                    if len(shp) > len(full) or any(a != 1 and a != b for a, b in zip(shp[::-1], full[::-1])):
                        raise ValueError(f"TracedConstraint: leading axes {shp[:-1]} of params do not broadcast to the batch {key}")
                    self._dev[key] = arr.to_device(self.params, torch.float64).expand(full).reshape(-1, self.n_params).contiguous()
                stride = self.n_params
            pdev = self._dev[key]
        if "blobs" not in self._dev:
            self._dev["blobs"] = tuple(None if t is None else arr.to_device(_tape.blob(t).view(np.float64), torch.float64)
                                       for t in (self.stage_tape, self.terminal_tape))
        blobs = self._dev["blobs"]
        pp = None if pdev is None else pdev.data_ptr()
        tapes = [zm_traced_t(None, None, 0, 0, 0, 0, 0) if t is None else
                 zm_traced_t(b.data_ptr(), pp, stride, len(t.code), len(t.consts), t.n_slots, self.n_params)
                 for b, t in zip(blobs, (self.stage_tape, self.terminal_tape))]
        ptr = lambda t: None if t is None else t.data_ptr()                                                    # noqa: E731
        st = zm_tracedcon_t(tapes[0], tapes[1], self.n, self.m, self.n_con, self.n_con_terminal, ptr(lam), ptr(lam_terminal), ptr(mu))
        st._owner = (self, blobs, pdev, lam, lam_terminal, mu)      # raw device addresses: keep the arrays behind them alive
        return st

    def values(self, xTraj, uTraj):
        """(g (..., N, n_con), terminal (..., n_con_terminal)) along trajectories xTraj (..., N+1, n), uTraj (..., N, m), evaluated on
        the device by the interpreter (the bits of a host build of it); NumPy in -> NumPy out, torch in -> torch out"""
        import torch
        from . import _lib
        shp = tuple(arr.shape(uTraj))
        lead, (N, m) = shp[:-2], shp[-2:]
        if m != self.m or tuple(arr.shape(xTraj)) != lead + (N + 1, self.n):
            raise ValueError(f"TracedConstraint.values: xTraj {tuple(arr.shape(xTraj))} / uTraj {shp} do not match (n={self.n}, m={self.m})")
        cs = self.con_struct(lead)            # (the parameter rows are checked before anything else touches the device)
        dx, du = (arr.to_device(X, torch.float64).contiguous() for X in (xTraj, uTraj))
        B = arr.batch(lead)
        gs = torch.zeros(lead + (N, self.n_con), dtype=torch.float64, device=dx.device)
        gt = torch.zeros(lead + (self.n_con_terminal,), dtype=torch.float64, device=dx.device)
        rc = _lib.lib().zm_traced_con_values_f64(ctypes.addressof(cs), dx.data_ptr(), du.data_ptr(), gs.data_ptr() if self.n_con else None,
                                                 gt.data_ptr() if self.n_con_terminal else None, B, N,
                                                 ctypes.c_void_p(arr.stream_ptr(dx)))
        _lib.check(rc, "TracedConstraint.values")
        return arr.result_like(gs, uTraj), arr.result_like(gt, uTraj)
