"""Drop-in for the solve path of ``zopt.mpcUtils`` (class ``lqrMpc``) on MI355X HIP kernels.

Same constructor and ``solve`` signature as the reference (mpcUtils.py:14-26, 61-81).  New: ``x0`` may carry leading
batch axes -- every initial state is an independent QP instance solved by one GPU lane; `solve` takes references to track (keywords
xRef, uRef).  The plotting / animation helpers
of the reference module (mpcUtils.py:84-202) are presentation code and not part of this package.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _arrays as arr
from . import _lib
from .pytrees import Trajectory

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

# cvxpy's status strings (mpcUtils.py:74,78).  "optimal_inaccurate" = OSQP's "solved inaccurate": the iteration limit was reached with
# both residuals within 10x their tolerances.  "unbounded" cannot arise for this QP (Q, Qf >= 0, R > 0); an instance that is neither
# solved nor certified infeasible at the limit is "user_limit" (cvxpy's name for OSQP's "maximum iterations reached").
_STATUS = {1: "optimal", 2: "infeasible", 3: "user_limit", 4: "optimal_inaccurate"}


class lqrMpc():

    def __init__(self, A, B, Q, R, N, x_lb, x_ub, u_lb, u_ub, Qf=None):
        """
        Setup an LQR MPC problem (reference mpcUtils.py:14-59)

        Arguments
        ---------
            A : Dynamics matrix; shape = (n,n)
            B : Input matrix; shape = (n,m)
            Q : State cost matrix; shape = (n,n)
            R : Control cost matrix; shape = (m,m)
            N : MPC horizon
            x_lb, x_ub : State lower / upper bound (+-inf allowed)
            u_lb, u_ub : Control lower / upper bound
            Qf : Terminal cost matrix, optional; shape = (n,n).  Defaults to Q

        Extension: every array may carry leading axes (A, Q, Qf (..., n, n), B (..., n, m), R (..., m, m), bounds (..., n) /
        (..., m)); they broadcast to the problem shape `P` and each problem has its own data (gain-scheduled MPC, fleets,
        per-instance boxes).  `rho` then has shape `P` and `solve` runs every problem in one launch.
        """
        if Qf is None:
            Qf = Q
        if _has_leading_axes(A, B, Q, R, Qf, x_lb, x_ub, u_lb, u_ub):
            self._init_batched(A, B, Q, R, N, x_lb, x_ub, u_lb, u_ub, Qf)
            return
        self.P = None
        f64 = lambda X: np.ascontiguousarray(np.asarray(X, dtype=np.float64))
        self.A, self.B, self.Q, self.R, self.Qf = f64(A), f64(B), f64(Q), f64(R), f64(Qf)
        self.n, self.m = self.B.shape
        self.N = int(N)
        self.x_lb, self.x_ub, self.u_lb, self.u_ub = f64(x_lb), f64(x_ub), f64(u_lb), f64(u_ub)
        if self.A.shape != (self.n, self.n) or self.Q.shape != (self.n, self.n) or self.R.shape != (self.m, self.m) \
                or self.x_lb.shape != (self.n,) or self.u_lb.shape != (self.m,) or self.N < 1:
            raise ValueError("inconsistent lqrMpc problem shapes")
        # cvxpy refuses the reference's problem (DCPError at solve time) unless every quad_form weight is positive semidefinite; here the
        # ADMM's Hessians 2Q + rho I would hide a slightly indefinite weight and return the stationary point of a non-convex problem
        for name, W in (("Q", self.Q), ("R", self.R), ("Qf", self.Qf)):
            w = np.linalg.eigvalsh(0.5 * (W + W.T))
            if w[0] < -1e-10 * max(1.0, abs(w[-1])):
                raise ValueError(f"lqrMpc: {name} is not positive semidefinite (smallest eigenvalue {w[0]:.3g}): the problem is not "
                                 f"convex (cvxpy raises DCPError for the reference's quad_form)")
        self._dev = None
        self._tables = {}
        self._ws = None   # ((batch, device, rho), ADMM workspace) of the last solve: warm start
        # one penalty for every instance: the geometric mean of the cost curvatures keeps both blocks of the
        # w-update Hessian (2Q + rho I, 2R + rho I) comparably conditioned
        self.rho = float(np.sqrt(max(np.trace(2 * self.Q) / self.n, 1e-12) * max(np.trace(2 * self.R) / self.m, 1e-12)))
        # The solve kernels are compiled for a few (n, m); any other n <= 24, m <= 8 is embedded in the next one: the extra
        # states follow x+ = 0 from x = 0 with unit weight and no bound, the extra controls act on nothing and cost u^2 --
        # they stay exactly zero and are sliced off the results.
        self._n_user, self._m_user = self.n, self.m
        fit = [(ns, mc) for (ns, mc) in self._COMPILED if ns >= self.n and mc >= self.m]
        if not fit:
            raise ValueError(f"lqrMpc: (n={self.n}, m={self.m}) outside the compiled kernels (n <= 24, m <= 8)")
        ns, mc = min(fit, key=lambda t: (t[0] * t[1], t[0]))
        if (ns, mc) != (self.n, self.m):
            n0, m0 = self.n, self.m
            pad2 = lambda X, r, c, d: np.block([[X, np.zeros((X.shape[0], c - X.shape[1]))],
                                                [np.zeros((r - X.shape[0], X.shape[1])), d * np.eye(r - X.shape[0], c - X.shape[1])]])
            self.A = pad2(self.A, ns, ns, 0.0)
            self.B = pad2(self.B, ns, mc, 0.0)
            self.Q, self.Qf = pad2(self.Q, ns, ns, 1.0), pad2(self.Qf, ns, ns, 1.0)
            self.R = pad2(self.R, mc, mc, 1.0)
            inf = np.inf
            self.x_lb = np.concatenate([self.x_lb, np.full(ns - n0, -inf)])
            self.x_ub = np.concatenate([self.x_ub, np.full(ns - n0, inf)])
            self.u_lb = np.concatenate([self.u_lb, np.full(mc - m0, -inf)])
            self.u_ub = np.concatenate([self.u_ub, np.full(mc - m0, inf)])
            self.n, self.m = ns, mc

    # (24, 8): beyond the 16-index tile of the 16-lanes-per-instance kernel -- the lane-per-instance kernel with a fixed penalty (no
    # tabulated levels): a coverage path, an order of magnitude slower per instance than the (12, 4) kernels
    _COMPILED = ((24, 8), (12, 4), (8, 4), (4, 2), (4, 1), (2, 2), (2, 1), (1, 1))

    N_LEVELS, RHO_STEP = 7, 5.0      # adaptive penalty: rho * 5^(l - 3), l = 0..6  (OSQP changes rho only by factors >= 5)

    def _init_batched(self, A, B, Q, R, N, x_lb, x_ub, u_lb, u_ub, Qf):
        """Per-problem data: the checks, penalty and embedding of the single-problem constructor, applied problem by problem."""
        A, B, Q, R, Qf, x_lb, x_ub, u_lb, u_ub = (_host_f64(X) for X in (A, B, Q, R, Qf, x_lb, x_ub, u_lb, u_ub))
        if B.ndim < 2:
            raise ValueError("inconsistent lqrMpc problem shapes")
        n, m = B.shape[-2:]
        self.N = int(N)
        mats = {"A": (A, (n, n)), "B": (B, (n, m)), "Q": (Q, (n, n)), "R": (R, (m, m)), "Qf": (Qf, (n, n)),
                "x_lb": (x_lb, (n,)), "x_ub": (x_ub, (n,)), "u_lb": (u_lb, (m,)), "u_ub": (u_ub, (m,))}
        if self.N < 1 or any(X.ndim < len(t) or X.shape[X.ndim - len(t):] != t for X, t in mats.values()):
            raise ValueError("inconsistent lqrMpc problem shapes")
        try:
            P = np.broadcast_shapes(*(X.shape[:X.ndim - len(t)] for X, t in mats.values()))
        except ValueError:
            raise ValueError("inconsistent lqrMpc problem shapes: the leading (problem) axes do not broadcast: "
                             + ", ".join(f"{k} {X.shape}" for k, (X, _) in mats.items())) from None
        self.P = tuple(int(d) for d in P)
        # PSD check per problem (see the single-problem constructor); the first offending problem is named by its index in P
        for name, W in (("Q", Q), ("R", R), ("Qf", Qf)):
            w = np.linalg.eigvalsh(0.5 * (W + np.swapaxes(W, -1, -2)))
            bad = np.broadcast_to(w[..., 0] < -1e-10 * np.maximum(1.0, np.abs(w[..., -1])), self.P)
            if bad.any():
                i = tuple(int(v) for v in np.argwhere(bad)[0])
                lo = float(np.broadcast_to(w[..., 0], self.P)[i])
                raise ValueError(f"lqrMpc: {name}[{', '.join(map(str, i))}] is not positive semidefinite (smallest eigenvalue {lo:.3g}): "
                                 f"the problem is not convex (cvxpy raises DCPError for the reference's quad_form)")
        self._dev = None
        self._tables = {}
        self._ws = None
        # the single-problem penalty, problem by problem: the same operations in the same order (a trace is the pairwise sum of the
        # contiguous diagonal, as np.trace's), so rho[i] is bit for bit lqrMpc(A[i], B[i], ...).rho
        tq = np.ascontiguousarray(np.diagonal(2 * Q, axis1=-2, axis2=-1)).sum(axis=-1) / n
        tr = np.ascontiguousarray(np.diagonal(2 * R, axis1=-2, axis2=-1)).sum(axis=-1) / m
        self.rho = np.sqrt(np.broadcast_to(np.maximum(tq, 1e-12) * np.maximum(tr, 1e-12), self.P)).astype(np.float64)
        self._n_user, self._m_user = n, m
        fit = [(ns, mc) for (ns, mc) in self._COMPILED if ns >= n and mc >= m]
        if not fit:
            raise ValueError(f"lqrMpc: (n={n}, m={m}) outside the compiled kernels (n <= 24, m <= 8)")
        ns, mc = min(fit, key=lambda t: (t[0] * t[1], t[0]))
        # every array materialised to P, embedded as the single-problem constructor embeds it (pad2: zero / unit padding blocks)
        inf = np.inf

        def emb(X, r, c, d):
            out = np.zeros(self.P + (r, c))
            out[..., :X.shape[-2], :X.shape[-1]] = X
            for i in range(min(r - X.shape[-2], c - X.shape[-1])):
                out[..., X.shape[-2] + i, X.shape[-1] + i] = d
            return out

        def embv(v, k, fill):
            out = np.full(self.P + (k,), fill)
            out[..., :v.shape[-1]] = v
            return out
        self.A, self.B = emb(A, ns, ns, 0.0), emb(B, ns, mc, 0.0)
        self.Q, self.Qf, self.R = emb(Q, ns, ns, 1.0), emb(Qf, ns, ns, 1.0), emb(R, mc, mc, 1.0)
        self.x_lb, self.x_ub = embv(x_lb, ns, -inf), embv(x_ub, ns, inf)
        self.u_lb, self.u_ub = embv(u_lb, mc, -inf), embv(u_ub, mc, inf)
        self.n, self.m = ns, mc

    def _device_problem_batched(self, rho, adaptive):
        """Device copies of the per-problem data and their tables: ONE setup launch for every (problem, penalty level)."""
        arr.require_gpu()
        Pn = int(np.prod(self.P))
        if self._dev is None:
            self._dev = {k: arr.to_device(getattr(self, k).reshape((Pn,) + getattr(self, k).shape[len(self.P):]), torch.float64)
                         for k in ("A", "B", "Q", "R", "Qf", "x_lb", "x_ub", "u_lb", "u_ub")}
        key = (rho.tobytes(), bool(adaptive))
        if key not in self._tables:
            d = self._dev
            nl = self.N_LEVELS if adaptive else 1
            l0 = nl // 2
            dev = d["A"].device
            # the level penalties of the single-problem setup, float(rho) * RHO_STEP ** (l - l0), as one (P, L) table
            fac = np.array([self.RHO_STEP ** (l - l0) for l in range(nl)])
            rtab = arr.to_device(rho.reshape(Pn, 1) * fac[None, :], torch.float64, dev)
            K = torch.empty((Pn, nl, self.N, self.m, self.n), dtype=torch.float64, device=dev)
            Mi = torch.empty((Pn, nl, self.N, self.m, self.m), dtype=torch.float64, device=dev)
            rc = _lib.lib().zm_mpc_setup_batched_f64(d["A"].data_ptr(), d["B"].data_ptr(), d["Q"].data_ptr(), d["R"].data_ptr(),
                                                     d["Qf"].data_ptr(), rtab.data_ptr(), Pn, nl, self.N, self.n, self.m,
                                                     K.data_ptr(), Mi.data_ptr(), ctypes.c_void_p(arr.stream_ptr(K)))
            _lib.check(rc, "lqrMpc setup")
            self._tables[key] = (K, Mi, nl, l0, arr.to_device(rho.reshape(Pn), torch.float64, dev), rtab)
        return self._dev, self._tables[key]

    def _device_problem(self, rho, adaptive):
        arr.require_gpu()
        if self._dev is None:
            self._dev = {k: arr.to_device(getattr(self, k), torch.float64)
                         for k in ("A", "B", "Q", "R", "Qf", "x_lb", "x_ub", "u_lb", "u_ub")}
        key = (rho, bool(adaptive))
        if key not in self._tables:
            d = self._dev
            nl = self.N_LEVELS if adaptive else 1
            l0 = nl // 2
            K = torch.empty((nl, self.N, self.m, self.n), dtype=torch.float64, device=d["A"].device)
            Mi = torch.empty((nl, self.N, self.m, self.m), dtype=torch.float64, device=d["A"].device)
            for l in range(nl):
                rc = _lib.lib().zm_mpc_setup_f64(d["A"].data_ptr(), d["B"].data_ptr(), d["Q"].data_ptr(), d["R"].data_ptr(),
                                                 d["Qf"].data_ptr(), float(rho) * self.RHO_STEP ** (l - l0), self.N, self.n,
                                                 self.m, K[l].data_ptr(), Mi[l].data_ptr(),
                                                 ctypes.c_void_p(arr.stream_ptr(K)))
                _lib.check(rc, "lqrMpc setup")
            self._tables[key] = (K, Mi, nl, l0)
        return self._dev, self._tables[key]

    def solve(self, x0, **kwargs):
        """
        Solve the MPC step at state x0 (reference mpcUtils.py:61-81)

        Arguments
        ---------
            x0 : Initial state (n,) -- or (..., n): a batch of independent instances
            **kwargs : solver options, named as the OSQP options the reference forwards through cvxpy
                (demos/lqrMpc.py:32): eps_abs, eps_rel (default 1e-5, cvxpy's OSQP default), max_iter (default 10000),
                rho, adaptive_rho (default True: the penalty moves between 7 tabulated levels rho * 5^l as OSQP's does),
                alpha (over-relaxation in (0, 2); default 1.6, OSQP's default, i.e. what the reference's solve runs with),
                eps_prim_inf (default 1e-4), warm_start (default True, as cvxpy: a solve for the same batch shape
                starts from the previous solve's ADMM iterates; `warm_start="shift"` (extension) advances them by one
                horizon step first, the right guess inside the receding-horizon loop of demos/lqrMpc.py:41-48);
                `solver` may be None or "OSQP" (the build has one solver); eps_dual_inf / verbose / polish are accepted
                and ignored.
                Extension (keywords): xRef (..., N+1, n), uRef (..., N, m) -- references to track: the cost becomes
                sum (x_k - xRef_k)'Q(x_k - xRef_k) + (u_k - uRef_k)'R(u_k - uRef_k) + (x_N - xRef_N)'Qf(x_N - xRef_N) under the same
                constraints.  Either may be None (zeros); a `Trajectory` may be given as xRef alone.  Row 0 of xRef only shifts the cost
                by a constant (accepted so that a Trajectory's xTraj passes as is).  Leading axes broadcast against those of x0 (and the
                problem shape).  In a receding-horizon loop the caller passes the moved reference window at every step.

        Returns
        -------
            u : Optimal control at current time step (…, m)
            traj : Trajectory tuple (xTraj (…, N+1, n), uTraj (…, N, m))
            status : problem status, one of [optimal, optimal_inaccurate, infeasible, user_limit] (a list of them for a batch)
        """
        xRef, uRef = kwargs.pop("xRef", None), kwargs.pop("uRef", None)
        solver = kwargs.pop("solver", None)
        if solver not in (None, "OSQP"):
            raise ValueError(f"solver {solver!r} is not available in zopt_amd (ADMM only; pass solver='OSQP' or None)")
        eps_abs = float(kwargs.pop("eps_abs", 1e-5))
        eps_rel = float(kwargs.pop("eps_rel", 1e-5))
        max_iter = int(kwargs.pop("max_iter", 10000))
        rho = kwargs.pop("rho", self.rho)
        if self.P is None:
            rho = float(rho)
        else:   # a scalar or an array that broadcasts to the problem shape
            try:
                rho = np.array(np.broadcast_to(_host_f64(rho), self.P))   # (a writable copy: torch refuses read-only views)
            except ValueError:
                raise ValueError(f"rho of shape {np.shape(rho)} does not broadcast to the problem shape {self.P}") from None
            if not np.all(rho > 0.0):
                raise ValueError("rho must be positive")
        adaptive = bool(kwargs.pop("adaptive_rho", True))        # OSQP / cvxpy default
        eps_pinf = float(kwargs.pop("eps_prim_inf", 1e-4))
        alpha = float(kwargs.pop("alpha", 1.6))
        if not (0.0 < alpha < 2.0):
            raise ValueError("alpha must lie in (0, 2)")
        warm = kwargs.pop("warm_start", kwargs.pop("warm_starting", True))
        shift = isinstance(warm, str) and warm == "shift"     # extension: previous iterates advanced by one horizon step
        warm = bool(warm)
        for k in ("eps_dual_inf", "verbose", "polish", "polishing"):
            kwargs.pop(k, None)
        if kwargs:
            raise TypeError(f"unknown solver options {sorted(kwargs)}")
        if xRef is not None or uRef is not None:
            return self._solve_tracking(x0, xRef, uRef, rho, eps_abs, eps_rel, max_iter, adaptive, eps_pinf, alpha, warm, shift)
        if self.P is not None:
            return self._solve_batched(x0, rho, eps_abs, eps_rel, max_iter, adaptive, eps_pinf, alpha, warm, shift)
        shp = tuple(x0.shape) if hasattr(x0, "shape") else tuple(np.shape(x0))
        if len(shp) < 1 or shp[-1] != self._n_user:
            raise ValueError(f"x0 has shape {shp}, expected (..., {self._n_user})")
        lead = shp[:-1]
        d, (K, Mi, n_levels, level0) = self._device_problem(rho, adaptive)
        dx0 = arr.to_device(x0, torch.float64).reshape(-1, self._n_user)
        if self.n != self._n_user:
            dx0 = torch.nn.functional.pad(dx0, (0, self.n - self._n_user))
        dx0 = dx0.contiguous()
        Bn = dx0.shape[0]
        dev = dx0.device
        N, n, m = self.N, self.n, self.m
        key = (Bn, str(dev), rho, adaptive)
        warm = warm and self._ws is not None and self._ws[0] == key
        if not warm:
            self._ws = (key, torch.empty(4 * Bn * N * (n + m), dtype=torch.float64, device=dev))
        ws = self._ws[1]
        xT = torch.empty((Bn, N + 1, n), dtype=torch.float64, device=dev)
        uT = torch.empty((Bn, N, m), dtype=torch.float64, device=dev)
        st = torch.empty(Bn, dtype=torch.int32, device=dev)
        its = torch.empty(Bn, dtype=torch.int32, device=dev)
        res = torch.empty((Bn, 2), dtype=torch.float64, device=dev)
        rc = _lib.lib().zm_mpc_solve_relaxed_f64(d["A"].data_ptr(), d["B"].data_ptr(), K.data_ptr(), Mi.data_ptr(), n_levels,
                                                  level0, self.RHO_STEP, alpha, d["x_lb"].data_ptr(), d["x_ub"].data_ptr(),
                                                  d["u_lb"].data_ptr(), d["u_ub"].data_ptr(), dx0.data_ptr(), rho, eps_abs,
                                                  eps_rel, eps_pinf, max_iter, (2 if shift else 1) if warm else 0,
                                                  ws.data_ptr(), xT.data_ptr(), uT.data_ptr(), st.data_ptr(), its.data_ptr(),
                                                  res.data_ptr(), Bn, N, n, m, ctypes.c_void_p(arr.stream_ptr(dx0)))
        _lib.check(rc, "lqrMpc.solve")
        self.last_iterations = its.reshape(lead).cpu().numpy()
        self.last_residuals = res.reshape(lead + (2,)).cpu().numpy()
        codes = st.cpu().numpy().reshape(lead)
        xo = arr.result_like(xT.reshape(lead + (N + 1, n))[..., :self._n_user], x0)
        uo = arr.result_like(uT.reshape(lead + (N, m))[..., :self._m_user], x0)
        if len(lead) == 0:
            status = _STATUS[int(codes)]
        else:
            status = np.vectorize(_STATUS.get, otypes=[object])(codes)
        return uo[..., 0, :], Trajectory(xo, uo), status

    def _solve_batched(self, x0, rho, eps_abs, eps_rel, max_iter, adaptive, eps_pinf, alpha, warm, shift):
        """solve() with per-problem data: x0 (..., n) broadcasts against P, every instance reads its problem's tables through an
        int32 instance -> problem map (one launch for all of them)."""
        shp = tuple(x0.shape) if hasattr(x0, "shape") else tuple(np.shape(x0))
        if len(shp) < 1 or shp[-1] != self._n_user:
            raise ValueError(f"x0 has shape {shp}, expected (..., {self._n_user})")
        try:
            lead = tuple(int(v) for v in np.broadcast_shapes(shp[:-1], self.P))
        except ValueError:
            raise ValueError(f"x0 of shape {shp} does not broadcast against the problem shape {self.P}: inconsistent shapes") from None
        N, n, m = self.N, self.n, self.m
        Pn, Bn = int(np.prod(self.P)), int(np.prod(lead))
        arr.require_gpu()
        if Bn == 0:   # no problems or no initial states: shaped empty results, nothing launched
            dev = x0.device if arr.is_torch(x0) and x0.is_cuda else torch.device("cuda")
            self.last_iterations = np.zeros(lead, dtype=np.int32)
            self.last_residuals = np.zeros(lead + (2,))
            xo = arr.result_like(torch.empty(lead + (N + 1, self._n_user), dtype=torch.float64, device=dev), x0)
            uo = arr.result_like(torch.empty(lead + (N, self._m_user), dtype=torch.float64, device=dev), x0)
            return uo[..., 0, :], Trajectory(xo, uo), np.empty(lead, dtype=object)
        d, (K, Mi, n_levels, level0, drho, _) = self._device_problem_batched(rho, adaptive)
        dev = d["A"].device
        dx0 = arr.to_device(x0, torch.float64, dev)
        dx0 = dx0.expand(lead + (self._n_user,)).reshape(-1, self._n_user)
        if n != self._n_user:
            dx0 = torch.nn.functional.pad(dx0, (0, n - self._n_user))
        dx0 = dx0.contiguous()
        prob = torch.as_tensor(np.ascontiguousarray(np.broadcast_to(np.arange(Pn, dtype=np.int32).reshape(self.P), lead)).reshape(-1),
                               device=dev)
        key = (lead, str(dev), rho.tobytes(), adaptive)
        warm = warm and self._ws is not None and self._ws[0] == key
        if not warm:
            self._ws = (key, torch.empty(4 * Bn * N * (n + m), dtype=torch.float64, device=dev))
        ws = self._ws[1]
        xT = torch.empty((Bn, N + 1, n), dtype=torch.float64, device=dev)
        uT = torch.empty((Bn, N, m), dtype=torch.float64, device=dev)
        st = torch.empty(Bn, dtype=torch.int32, device=dev)
        its = torch.empty(Bn, dtype=torch.int32, device=dev)
        res = torch.empty((Bn, 2), dtype=torch.float64, device=dev)
        rc = _lib.lib().zm_mpc_solve_batched_f64(d["A"].data_ptr(), d["B"].data_ptr(), K.data_ptr(), Mi.data_ptr(), n_levels, level0,
                                                  self.RHO_STEP, alpha, d["x_lb"].data_ptr(), d["x_ub"].data_ptr(),
                                                  d["u_lb"].data_ptr(), d["u_ub"].data_ptr(), dx0.data_ptr(), drho.data_ptr(),
                                                  prob.data_ptr(), Pn, eps_abs, eps_rel, eps_pinf, max_iter,
                                                  (2 if shift else 1) if warm else 0, ws.data_ptr(), xT.data_ptr(), uT.data_ptr(),
                                                  st.data_ptr(), its.data_ptr(), res.data_ptr(), Bn, N, n, m,
                                                  ctypes.c_void_p(arr.stream_ptr(dx0)))
        _lib.check(rc, "lqrMpc.solve")
        self.last_iterations = its.reshape(lead).cpu().numpy()
        self.last_residuals = res.reshape(lead + (2,)).cpu().numpy()
        codes = st.cpu().numpy().reshape(lead)
        xo = arr.result_like(xT.reshape(lead + (N + 1, n))[..., :self._n_user], x0)
        uo = arr.result_like(uT.reshape(lead + (N, m))[..., :self._m_user], x0)
        status = np.vectorize(_STATUS.get, otypes=[object])(codes)
        return uo[..., 0, :], Trajectory(xo, uo), status

    def _solve_tracking(self, x0, xRef, uRef, rho, eps_abs, eps_rel, max_iter, adaptive, eps_pinf, alpha, warm, shift):
        """solve() about a reference (shared or per-problem data): x0, xRef and uRef broadcast to one batch shape, the references are
        padded with zeros to the compiled shape, and zm_mpc_solve_tracking_f64 forms the linear term and runs the tracking kernels."""
        if isinstance(xRef, Trajectory):
            if uRef is not None:
                raise ValueError("a Trajectory given as xRef carries its own uTraj: pass it alone (uRef=None)")
            xRef, uRef = xRef.xTraj, xRef.uTraj
        N, n, m = self.N, self.n, self.m
        shape_of = lambda X: tuple(X.shape) if hasattr(X, "shape") else tuple(np.shape(X))
        shp = shape_of(x0)
        if len(shp) < 1 or shp[-1] != self._n_user:
            raise ValueError(f"x0 has shape {shp}, expected (..., {self._n_user})")
        leads = {"x0": (shp, shp[:-1])}
        for name, X, want in (("xRef", xRef, (N + 1, self._n_user)), ("uRef", uRef, (N, self._m_user))):
            if X is not None:
                s = shape_of(X)
                if len(s) < 2 or s[-2:] != want:
                    raise ValueError(f"{name} has shape {s}, expected (..., {want[0]}, {want[1]})")
                leads[name] = (s, s[:-2])
        try:
            lead = np.broadcast_shapes(*(l for _, l in leads.values()), *(() if self.P is None else (self.P,)))
        except ValueError:
            raise ValueError(", ".join(f"{k} of shape {s}" for k, (s, _) in leads.items()) + " do not broadcast against each other"
                             + ("" if self.P is None else f" and the problem shape {self.P}") + ": inconsistent shapes") from None
        lead = tuple(int(v) for v in lead)
        Bn = int(np.prod(lead))
        arr.require_gpu()
        if Bn == 0:   # nothing to solve: shaped empty results, nothing launched
            dev = x0.device if arr.is_torch(x0) and x0.is_cuda else torch.device("cuda")
            self.last_iterations = np.zeros(lead, dtype=np.int32)
            self.last_residuals = np.zeros(lead + (2,))
            xo = arr.result_like(torch.empty(lead + (N + 1, self._n_user), dtype=torch.float64, device=dev), x0)
            uo = arr.result_like(torch.empty(lead + (N, self._m_user), dtype=torch.float64, device=dev), x0)
            return uo[..., 0, :], Trajectory(xo, uo), np.empty(lead, dtype=object)
        if self.P is None:
            d, (K, Mi, n_levels, level0) = self._device_problem(rho, adaptive)
            dev = x0.device if arr.is_torch(x0) and x0.is_cuda else d["A"].device
            rho_s, drho, prob, Pn, rho_key = rho, None, None, 0, rho
        else:
            d, (K, Mi, n_levels, level0, drho, _) = self._device_problem_batched(rho, adaptive)
            dev = d["A"].device
            Pn = int(np.prod(self.P))
            prob = torch.as_tensor(np.ascontiguousarray(np.broadcast_to(np.arange(Pn, dtype=np.int32).reshape(self.P),
                                                                        lead)).reshape(-1), device=dev)
            rho_s, rho_key = 0.0, rho.tobytes()

        def flat(X, tail, width):   # broadcast to the batch, one row per instance, the padded components zero
            t = arr.to_device(X, torch.float64, dev)
            t = t.expand(lead + tail).reshape((Bn,) + tail)
            if width != tail[-1]:
                t = torch.nn.functional.pad(t, (0, width - tail[-1]))
            return t.contiguous()
        dx0 = flat(x0, (self._n_user,), n)
        dxr = None if xRef is None else flat(xRef, (N + 1, self._n_user), n)
        dur = None if uRef is None else flat(uRef, (N, self._m_user), m)
        # (a workspace of its own kind: the fifth block holds the linear term of the cost)
        key = ("tracking", lead, str(dev), rho_key, adaptive)
        warm = warm and self._ws is not None and self._ws[0] == key
        if not warm:
            self._ws = (key, torch.empty(5 * Bn * N * (n + m), dtype=torch.float64, device=dev))
        ws = self._ws[1]
        xT = torch.empty((Bn, N + 1, n), dtype=torch.float64, device=dev)
        uT = torch.empty((Bn, N, m), dtype=torch.float64, device=dev)
        st = torch.empty(Bn, dtype=torch.int32, device=dev)
        its = torch.empty(Bn, dtype=torch.int32, device=dev)
        res = torch.empty((Bn, 2), dtype=torch.float64, device=dev)
        ptr = lambda t: None if t is None else t.data_ptr()
        rc = _lib.lib().zm_mpc_solve_tracking_f64(d["A"].data_ptr(), d["B"].data_ptr(), d["Q"].data_ptr(), d["R"].data_ptr(),
                                                   d["Qf"].data_ptr(), K.data_ptr(), Mi.data_ptr(), n_levels, level0, self.RHO_STEP,
                                                   alpha, d["x_lb"].data_ptr(), d["x_ub"].data_ptr(), d["u_lb"].data_ptr(),
                                                   d["u_ub"].data_ptr(), dx0.data_ptr(), ptr(dxr), ptr(dur), rho_s, ptr(drho),
                                                   ptr(prob), Pn, eps_abs, eps_rel, eps_pinf, max_iter,
                                                   (2 if shift else 1) if warm else 0, ws.data_ptr(), xT.data_ptr(), uT.data_ptr(),
                                                   st.data_ptr(), its.data_ptr(), res.data_ptr(), Bn, N, n, m,
                                                   ctypes.c_void_p(arr.stream_ptr(dx0)))
        _lib.check(rc, "lqrMpc.solve")
        self.last_iterations = its.reshape(lead).cpu().numpy()
        self.last_residuals = res.reshape(lead + (2,)).cpu().numpy()
        codes = st.cpu().numpy().reshape(lead)
        xo = arr.result_like(xT.reshape(lead + (N + 1, n))[..., :self._n_user], x0)
        uo = arr.result_like(uT.reshape(lead + (N, m))[..., :self._m_user], x0)
        if len(lead) == 0:
            status = _STATUS[int(codes)]
        else:
            status = np.vectorize(_STATUS.get, otypes=[object])(codes)
        return uo[..., 0, :], Trajectory(xo, uo), status


def _host_f64(X):
    """float64 NumPy copy of an array-like; torch tensors (host or device) included"""
    if torch is not None and isinstance(X, torch.Tensor):
        X = X.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(X, dtype=np.float64))


def _has_leading_axes(A, B, Q, R, Qf, x_lb, x_ub, u_lb, u_ub):
    """True if any problem array carries axes in front of its single-problem shape (matrices 2-D, bounds 1-D)"""
    nd = lambda X: len(X.shape) if hasattr(X, "shape") else np.ndim(X)
    return any(nd(X) > 2 for X in (A, B, Q, R, Qf)) or any(nd(v) > 1 for v in (x_lb, x_ub, u_lb, u_ub))
