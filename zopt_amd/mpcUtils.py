"""Drop-in for the solve path of ``zopt.mpcUtils`` (class ``lqrMpc``) on MI355X HIP kernels.

Same constructor and ``solve`` signature as the reference (mpcUtils.py:14-26, 61-81).  New: ``x0`` may carry leading
batch axes -- every initial state is an independent QP instance solved by one GPU lane; `solve` takes references to track (keywords
xRef, uRef); `simulate` runs the whole receding-horizon loop of the reference's demo (demos/lqrMpc.py:40-47) on the device in one call;
`soften` makes chosen bounds soft (a penalty l1 d + l2 d^2 on the distance d from the box), in `solve` and in `simulate`.
`ltvMpc` (extension) is the same QP with stage-varying dynamics x+ = A_k x + B_k u + c_k, a linearisation about a trajectory.
The plotting / animation helpers
of the reference module (mpcUtils.py:84-202) are presentation code and not part of this package.
"""
from __future__ import annotations

import collections
import ctypes

import numpy as np

from . import _arrays as arr
from . import _lib
from . import models as _models
from .pytrees import Trajectory

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

# cvxpy's status strings (mpcUtils.py:74,78).  "optimal_inaccurate" = OSQP's "solved inaccurate": the iteration limit was reached with
# both residuals within 10x their tolerances.  "unbounded" cannot arise for this QP (Q, Qf >= 0, R > 0); an instance that is neither
# solved nor certified infeasible at the limit is "user_limit" (cvxpy's name for OSQP's "maximum iterations reached").
_STATUS = {1: "optimal", 2: "infeasible", 3: "user_limit", 4: "optimal_inaccurate"}

# what `lqrMpc.simulate` returns: the closed-loop states (..., S+1, n) and inputs (..., S, m), the status strings and ADMM iteration counts
# of every step (..., S), and -- on request -- the rollout every step planned, a Trajectory of (..., S, N+1, n) / (..., S, N, m)
MpcClosedLoop = collections.namedtuple("MpcClosedLoop", ("xTraj", "uTraj", "status", "iterations", "predictions"))


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

        A weight enters the cost through its quadratic form alone, so Q, R and Qf are replaced by their symmetric parts (W + W') / 2
        before anything is derived from them (exact, hence bit-neutral, for a symmetric weight): the setup entry points of the C ABI
        expect symmetric weights, and the attributes Q, R, Qf hold the symmetric parts.

        Extension: every array may carry leading axes (A, Q, Qf (..., n, n), B (..., n, m), R (..., m, m), bounds (..., n) /
        (..., m)); they broadcast to the problem shape `P` and each problem has its own data (gain-scheduled MPC, fleets,
        per-instance boxes).  `rho` then has shape `P` and `solve` runs every problem in one launch.
        """
        if Qf is None:
            Qf = Q
        batched = _has_leading_axes(A, B, Q, R, Qf, x_lb, x_ub, u_lb, u_ub)
        data = {k: _host_f64(X) for k, X in zip(_ARRAYS, (A, B, Q, R, Qf, x_lb, x_ub, u_lb, u_ub))}
        self.N = int(N)
        n, m, P = _problem_shape(data, self.N, batched)
        _symmetric_part(data)
        # one problem: P is None, rho a float -- solve() then runs the shared-problem kernels (scalar table loads)
        self.P = P if batched else None
        _check_psd(data, P)
        self._dev = None
        self._tables = {}
        self._ws = None   # (key, ADMM workspace) of the last solve: warm start
        rho = _penalty(data["Q"], data["R"], P)
        self.rho = rho if batched else float(rho)
        # The solve kernels are compiled for a few (n, m); any other n <= 24, m <= 8 is embedded in the next one: the extra
        # states follow x+ = 0 from x = 0 with unit weight and no bound, the extra controls act on nothing and cost u^2 --
        # they stay exactly zero and are sliced off the results.
        self._n_user, self._m_user = n, m
        fit = [(ns, mc) for (ns, mc) in self._COMPILED if ns >= n and mc >= m]
        if not fit:
            raise ValueError(f"lqrMpc: (n={n}, m={m}) outside the compiled kernels (n <= 24, m <= 8)")
        self.n, self.m = min(fit, key=lambda t: (t[0] * t[1], t[0]))
        if batched or (self.n, self.m) != (n, m):   # (per-problem data is also materialised to P here)
            data = _embed(data, P, self.n, self.m)
        for k, X in data.items():
            setattr(self, k, X)

    # (24, 8): beyond the 16-index tile of the 16-lanes-per-instance kernel -- the lane-per-instance kernel with a fixed penalty (no
    # tabulated levels): a coverage path, an order of magnitude slower per instance than the (12, 4) kernels
    _COMPILED = ((24, 8), (12, 4), (8, 4), (4, 2), (4, 1), (2, 2), (2, 1), (1, 1))

    _LTV = False                     # ltvMpc (below) shares `solve` and overrides this
    stage_varying = frozenset()      # ltvMpc: the names among Q, R and the four bounds that carry a stage axis
    _soft = None                     # the penalty weights of soft box constraints, as given (None: every bound is hard): soften(), ltvMpc
    _stage_entry = False             # ltvMpc: the data is kept in stage form and goes through the stage entry points

    N_LEVELS, RHO_STEP = 7, 5.0      # adaptive penalty: rho * 5^(l - 3), l = 0..6  (OSQP changes rho only by factors >= 5)

    _SOFT = ("x_soft_l1", "x_soft_l2", "u_soft_l1", "u_soft_l2")
    N_MAX = 75   # the 16-lanes-per-instance kernels: 4 instances x N stages x 64 doubles of LDS <= 150 KiB

    def soften(self, x_soft_l1=None, x_soft_l2=None, u_soft_l1=None, u_soft_l2=None):
        """
        Soft box constraints (extension; zm_mpc_solve_soft_f64, zm_mpc_closed_loop_soft_f64).  Returns self:

            prob = lqrMpc(A, B, Q, R, N, x_lb, x_ub, u_lb, u_ub).soften(x_soft_l1=l1)

        x_soft_l1, x_soft_l2 (n,), u_soft_l1, u_soft_l2 (m,) -- or (..., n) / (..., m) with leading axes that broadcast to the problem
        shape `P` of an object with per-problem data -- are penalty weights per component, constant over the stages, with ltvMpc's
        meaning and checks: with d the distance of a component of x_k (k >= 1) or u_k from its box the cost gains l1 d + l2 d^2 and the
        bounds of that component no longer constrain it; l1 = +inf (the default of a weight never given) keeps the component hard, and
        l2 must be 0 there.  `solve` then solves from an x0 outside the box in a soft component, where a hard one is "infeasible" as
        before; `simulate` does not clip the soft state components (see there).  With an l1 above the hard problem's multipliers the
        hard solution comes back whenever there is one; with every l1 = +inf the results are those of the object before `soften`, bit
        for bit.

        A later call replaces the weights it names and keeps the others.  Nothing is launched: the tables depend on the problem and the
        penalty only and stay, and so does the warm-start workspace (as after ltvMpc.update with new weights).

        A softened object runs on the 16-lanes-per-instance kernels alone: ValueError, before anything touches a device, if the compiled
        shape has n + m > 16 (the (24, 8) embedding) or N > 75.  ZOPT_AMD_MPC_PATH does not apply to it.
        """
        if self.n + self.m > 16:
            raise ValueError(f"lqrMpc.soften: (n={self._n_user}, m={self._m_user}) runs in the ({self.n}, {self.m}) kernels, beyond the "
                             f"16-lanes-per-instance kernels that take soft weights (n <= 12, m <= 4)")
        if self.N > self.N_MAX:
            raise ValueError(f"lqrMpc.soften: N={self.N} beyond the horizons whose iterates fit LDS (N <= {self.N_MAX}), which the kernels "
                             f"that take soft weights need")
        new = {k: X for k, X in zip(self._SOFT, (x_soft_l1, x_soft_l2, u_soft_l1, u_soft_l2)) if X is not None}
        given = {**(self._soft or dict.fromkeys(self._SOFT)), **new}
        l1, l2 = self._soft_stacked("lqrMpc.soften", given)
        self._soft, self.soft_l1, self.soft_l2 = given, l1, l2
        if self._dev is not None and "soft_l1" in self._dev:
            for k, X in (("soft_l1", l1), ("soft_l2", l2)):
                self._dev[k].copy_(arr.to_device(X.reshape(self._dev[k].shape), torch.float64, self._dev[k].device))
        return self

    def _soft_stacked(self, who, given):
        """(l1, l2), each P + (n + m,) in the kernels' stacked layout [x ; u] of the compiled shape, from the four weights as given (None:
        l1 = +inf, l2 = 0).  A padded component is hard: l1 = +inf, l2 = 0."""
        P = () if self.P is None else self.P   # (lqrMpc without per-problem data: one row)
        l1, l2 = np.full(P + (self.n + self.m,), np.inf), np.zeros(P + (self.n + self.m,))
        for name, at, k in (("x_soft_l1", 0, self._n_user), ("x_soft_l2", 0, self._n_user), ("u_soft_l1", self.n, self._m_user),
                            ("u_soft_l2", self.n, self._m_user)):
            if given[name] is None:
                continue
            w = _host_f64(given[name])
            try:
                ok = w.ndim >= 1 and w.shape[-1] == k and np.broadcast_shapes(w.shape[:-1], P) == P
            except ValueError:
                ok = False
            if not ok:
                raise ValueError(f"{who}: {name} has shape {w.shape}, expected (..., {k}) with leading axes that broadcast to the problem "
                                 f"shape {P}")
            if np.any(np.isnan(w)) or np.any(w < 0):
                raise ValueError(f"{who}: {name} has a negative or NaN entry: a penalty weight is >= 0 (l1 = +inf: a hard component)")
            if name.endswith("l2") and not np.all(np.isfinite(w)):
                raise ValueError(f"{who}: {name} has a non-finite entry: the quadratic weight is finite (a hard component is l1 = +inf)")
            (l1 if name.endswith("l1") else l2)[..., at:at + k] = w
        if np.any((l2 > 0) & np.isinf(l1)):
            raise ValueError(f"{who}: a quadratic weight l2 > 0 on a component whose l1 is +inf (hard): give that component a finite l1 "
                             f"(0 for a purely quadratic penalty)")
        return l1, l2

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
            rc = _lib.lib().zm_mpc_setup_batched_f64(*_ptrs(d, "A B Q R Qf", rtab), Pn, nl, self.N, self.n, self.m, *_ptrs(d, "", K, Mi),
                                                     ctypes.c_void_p(arr.stream_ptr(K)))
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
                rc = _lib.lib().zm_mpc_setup_f64(*_ptrs(d, "A B Q R Qf"), float(rho) * self.RHO_STEP ** (l - l0), self.N, self.n, self.m,
                                                 *_ptrs(d, "", K[l], Mi[l]), ctypes.c_void_p(arr.stream_ptr(K)))
                _lib.check(rc, "lqrMpc setup")
            self._tables[key] = (K, Mi, nl, l0)
        return self._dev, self._tables[key]

    def _solver_options(self, kwargs, warm_default):
        """The solver options of `solve` (and `simulate`) taken out of `kwargs`, which must be empty afterwards:
        (eps_abs, eps_rel, max_iter, rho, adaptive_rho, eps_prim_inf, alpha, warm) -- warm: the C side's warm_start, 0: cold, 1: from
        the previous iterates, 2: from those advanced by one horizon step."""
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
                rho = np.array(np.broadcast_to(_host_f64(rho).reshape(np.shape(rho)), self.P))   # (a writable copy; 0-d stays 0-d)
            except ValueError:
                raise ValueError(f"rho of shape {np.shape(rho)} does not broadcast to the problem shape {self.P}") from None
            if not np.all(rho > 0.0):
                raise ValueError("rho must be positive")
        adaptive = bool(kwargs.pop("adaptive_rho", True))        # OSQP / cvxpy default
        eps_pinf = float(kwargs.pop("eps_prim_inf", 1e-4))
        alpha = float(kwargs.pop("alpha", 1.6))
        if not (0.0 < alpha < 2.0):
            raise ValueError("alpha must lie in (0, 2)")
        warm = kwargs.pop("warm_start", kwargs.pop("warm_starting", warm_default))
        warm = 2 if isinstance(warm, str) and warm == "shift" else int(bool(warm))   # "shift": an extension
        for k in ("eps_dual_inf", "verbose", "polish", "polishing"):
            kwargs.pop(k, None)
        if kwargs:
            raise TypeError(f"unknown solver options {sorted(kwargs)}")
        return eps_abs, eps_rel, max_iter, rho, adaptive, eps_pinf, alpha, warm

    def _problem_on_device(self, rho, adaptive):
        """(device data, (K, Minv, n_levels, level0, rho per problem | None, ...), number of problems -- 0: the one shared problem)"""
        if self.P is None:
            d, tabs = self._device_problem(rho, adaptive)
            tabs, Pn = tabs + (None,), 0
        else:
            d, tabs = self._device_problem_batched(rho, adaptive)
            Pn = int(np.prod(self.P))
        if self._soft is not None and "soft_l1" not in d:   # (a softened lqrMpc: the weights beside the data, one row per problem)
            d.update({k: arr.to_device(getattr(self, k).reshape(max(Pn, 1), -1), torch.float64, d["A"].device) for k in ("soft_l1", "soft_l2")})
        return d, tabs, Pn

    def _batch_shape(self, x0, arrays, suffix="", plural=True, own=False, plan=None):
        """The batch shape `lead` that x0 (..., n) and the per-instance `arrays` -- (name, X | None, (rows, user width), padded width)
        each -- broadcast to with the problem shape, and its number of instances.  `suffix` ends the message about an array of another
        shape; plural / own pick the sentence about shapes that do not broadcast (own: realTimeIteration, where every instance is its own
        problem and `lead` must be the problem shape; its `plan` joins the broadcast)."""
        shp = _shape_of(x0)
        if len(shp) < 1 or shp[-1] != self._n_user:
            raise ValueError(f"x0 has shape {shp}, expected (..., {self._n_user})")
        leads = {"x0": (shp, shp[:-1])}
        for name, X, want, _ in arrays:
            if X is not None:
                sh = _shape_of(X)
                if len(sh) < 2 or sh[-2:] != want:
                    raise ValueError(f"{name} has shape {sh}, expected (..., {want[0]}, {want[1]}){suffix}")
                leads[name] = (sh, sh[:-2])
        if plan is not None:
            xs, us, pl = _plan_shapes("ltvMpc.realTimeIteration", plan, self.N, self._n_user, self._m_user)
            leads["plan.xTraj"], leads["plan.uTraj"] = (xs, pl), (us, pl)
        try:
            lead = np.broadcast_shapes(*(l for _, l in leads.values()), *(() if self.P is None else (self.P,)))
        except ValueError:
            lead = None
        if lead is None or (own and lead != self.P):
            who = ", ".join(f"{k} of shape {sh}" for k, (sh, _) in leads.items())
            if own:
                who += f" do not broadcast to the problem shape {self.P} (every instance is its own problem)"
            elif plural:
                who += " do not broadcast against each other" + ("" if self.P is None else f" and the problem shape {self.P}")
            else:   # (x0 alone: only a problem shape can be in its way)
                who += f" does not broadcast against the problem shape {self.P}"
            raise ValueError(who + ": inconsistent shapes")
        lead = tuple(int(v) for v in lead)
        return lead, int(np.prod(lead))

    def _device_rows(self, lead, Bn, d, tracking, x0, arrays, identity=False):
        """(device, x0, [each of `arrays` | None], instance -> problem map | None): one row per instance, the padded components zero.  A
        plain solve runs where x0 is (host data: on the current device), the others where the problem's tables are -- unless a single
        problem tracks from an x0 that is on a device already."""
        dx0 = _flat(x0, lead, Bn, (self._n_user,), self.n, d["A"].device if tracking or self.P is not None else None)
        dev = dx0.device if self.P is None else d["A"].device
        rows = [None if X is None else _flat(X, lead, Bn, want, width, dev) for _, X, want, width in arrays]
        prob = None
        if identity:   # (realTimeIteration: every instance its own problem)
            prob = torch.arange(Bn, dtype=torch.int32, device=dev)
        elif self.P is not None:
            Pn = int(np.prod(self.P))
            prob = torch.as_tensor(np.ascontiguousarray(np.broadcast_to(np.arange(Pn, dtype=np.int32).reshape(self.P), lead)).reshape(-1),
                                   device=dev)
        return dev, dx0, rows, prob

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
        eps_abs, eps_rel, max_iter, rho, adaptive, eps_pinf, alpha, warm = self._solver_options(kwargs, True)
        if isinstance(xRef, Trajectory):
            if uRef is not None:
                raise ValueError("a Trajectory given as xRef carries its own uTraj: pass it alone (uRef=None)")
            xRef, uRef = xRef.xTraj, xRef.uTraj
        tracking = xRef is not None or uRef is not None
        linear = tracking or self._LTV   # the workspace has a fifth block for the linear term of the cost
        N, n, m = self.N, self.n, self.m

        # 1. shapes: x0 and the references broadcast (with the problem shape) to the batch shape `lead`
        refs = (("xRef", xRef, (N + 1, self._n_user), n), ("uRef", uRef, (N, self._m_user), m))
        lead, Bn = self._batch_shape(x0, refs, plural=tracking)
        arr.require_gpu()

        # 2. nothing to solve: shaped empty results, nothing launched.  (Not for a plain solve: that one goes on, drops the warm start
        # and lets the C side return at batch == 0, as it always has.)
        if Bn == 0 and (tracking or self.P is not None):
            dev = x0.device if arr.is_torch(x0) and x0.is_cuda else torch.device("cuda")
            self.last_iterations = np.zeros(lead, dtype=np.int32)
            self.last_residuals = np.zeros(lead + (2,))
            xo = arr.result_like(torch.empty(lead + (N + 1, self._n_user), dtype=torch.float64, device=dev), x0)
            uo = arr.result_like(torch.empty(lead + (N, self._m_user), dtype=torch.float64, device=dev), x0)
            return uo[..., 0, :], Trajectory(xo, uo), np.empty(lead, dtype=object)

        # 3. the problem on the device and its tables
        d, tabs, Pn = self._problem_on_device(rho, adaptive)
        K, Mi, n_levels, level0, drho = tabs[:5]
        rho_key = rho if self.P is None else rho.tobytes()

        # 4. one row per instance and the instance -> problem map
        dev, dx0, (dxr, dur), prob = self._device_rows(lead, Bn, d, tracking or self._soft is not None, x0, refs)

        # 5. workspace (y, lam, kf, rv; tracking: a fifth block for the linear term of the cost) and the warm start from it.  A plain solve
        # is keyed on the number of instances, the others on the batch shape, tracking as a kind of its own.
        key = (("tracking", lead) if linear else lead if self.P is not None else Bn, str(dev), rho_key, adaptive)
        if not (warm and self._ws is not None and self._ws[0] == key):
            warm = 0
            self._ws = (key, torch.empty((5 if linear else 4) * Bn * N * (n + m), dtype=torch.float64, device=dev))
        ws = self._ws[1]

        # 6. outputs
        xT = torch.empty((Bn, N + 1, n), dtype=torch.float64, device=dev)
        uT = torch.empty((Bn, N, m), dtype=torch.float64, device=dev)
        st = torch.empty(Bn, dtype=torch.int32, device=dev)
        its = torch.empty(Bn, dtype=torch.int32, device=dev)
        res = torch.empty((Bn, 2), dtype=torch.float64, device=dev)

        # 7. the C call: the plain and the per-problem kernels, or the tracking variants of either (other kernels, slower per iteration)
        box = "x_lb0 x_ub0 lo hi" if self._stage_entry else "x_lb x_ub u_lb u_ub"
        if self._soft is not None:
            box += " soft_l1 soft_l2"
        opts = (n_levels, level0, self.RHO_STEP, alpha, *_ptrs(d, box, dx0))
        out = (eps_abs, eps_rel, eps_pinf, max_iter, warm, *_ptrs(d, "", ws, xT, uT, st, its, res), Bn, N, n, m,
               ctypes.c_void_p(arr.stream_ptr(dx0)))
        if self._LTV:   # (ltvMpc: stage-varying dynamics, always per-problem, a reference or none)
            D, ABt = tabs[6:8]
            if self._soft is not None:   # (soft box constraints: the stage form with the penalty weights behind the box)
                rc = _lib.lib().zm_mpc_solve_ltv_soft_f64(*_ptrs(d, "A B c", ABt), *_ptrs(d, "Qs Rs", K, Mi, D), *opts,
                                                           *_ptrs(d, "", dxr, dur, drho, prob), Pn, *out)
            elif self._stage_entry:   # (weights and box per stage: the sibling entry, the same kernels with the stage's box prefetched)
                rc = _lib.lib().zm_mpc_solve_ltv_stage_f64(*_ptrs(d, "A B c", ABt), *_ptrs(d, "Qs Rs", K, Mi, D), *opts,
                                                            *_ptrs(d, "", dxr, dur, drho, prob), Pn, *out)
            else:
                rc = _lib.lib().zm_mpc_solve_ltv_f64(*_ptrs(d, "A B c", ABt), *_ptrs(d, "Q R Qf", K, Mi, D), *opts,
                                                      *_ptrs(d, "", dxr, dur, drho, prob), Pn, *out)
        elif self._soft is not None:   # (soften: the tracking entry's arguments with the weights behind the box; a reference or none)
            rc = _lib.lib().zm_mpc_solve_soft_f64(*_ptrs(d, "A B Q R Qf", K, Mi), *opts, *_ptrs(d, "", dxr, dur),
                                                   rho if self.P is None else 0.0, *_ptrs(d, "", drho, prob), Pn, *out)
        elif tracking:
            rc = _lib.lib().zm_mpc_solve_tracking_f64(*_ptrs(d, "A B Q R Qf", K, Mi), *opts, *_ptrs(d, "", dxr, dur),
                                                       rho if self.P is None else 0.0, *_ptrs(d, "", drho, prob), Pn, *out)
        elif self.P is not None:
            rc = _lib.lib().zm_mpc_solve_batched_f64(*_ptrs(d, "A B", K, Mi), *opts, *_ptrs(d, "", drho, prob), Pn, *out)
        else:
            rc = _lib.lib().zm_mpc_solve_relaxed_f64(*_ptrs(d, "A B", K, Mi), *opts, rho, *out)
        _lib.check(rc, "lqrMpc.solve")

        # 8. results
        self.last_iterations = its.reshape(lead).cpu().numpy()
        self.last_residuals = res.reshape(lead + (2,)).cpu().numpy()
        codes = st.cpu().numpy().reshape(lead)
        xo = arr.result_like(xT.reshape(lead + (N + 1, n))[..., :self._n_user], x0)
        uo = arr.result_like(uT.reshape(lead + (N, m))[..., :self._m_user], x0)
        if len(lead) == 0:   # (one problem only: a problem shape has at least one axis)
            status = _STATUS[int(codes)]
        else:
            status = np.vectorize(_STATUS.get, otypes=[object])(codes)
        return uo[..., 0, :], Trajectory(xo, uo), status

    def simulate(self, x0, steps, disturbance=None, clip_tol=1e-6, return_predictions=False, xRef=None, uRef=None, **solver_opts):
        """
        The receding-horizon loop of the reference's demo (demos/lqrMpc.py:40-47) as one call, entirely on the device:

            x = x0
            for s in range(steps):
                if clip_tol is not None: x = clip(x, x_lb + clip_tol, x_ub - clip_tol)      # (after `soften`: the hard components only)
                xTraj[s] = x
                u, traj, status[s] = self.solve(x, warm_start=(False if s == 0 else W), window s of the references, **solver_opts)
                uTraj[s] = u;  iterations[s] = self.last_iterations
                x = traj.xTraj[1] + (disturbance[s] if disturbance is not None else 0)
            xTraj[steps] = clip(x, ...) if clip_tol is not None else x

        with the results that loop gives, whatever the status of a step (a step that is not "optimal" still leaves a rollout, and the step
        after it starts cold).  After `soften`, `clip` moves the HARD state components only: a component with a finite x_soft_l1 is never
        clipped, so xTraj[s + 1] is the plant's state there, outside the box if a disturbance has pushed it out, and the solve from it
        brings it back.  A regulator run is one launch of a kernel that has the step loop inside (a wave goes on to its next step
        as soon as its own four instances are through); tracking runs, (n, m) beyond the 16-lane kernels and horizons beyond LDS are a
        queue of launches without a host round trip.  `simulate` has its own workspace: a `solve` after it (warm start, `last_iterations`,
        `last_residuals`) behaves as if it had not happened.

        Arguments
        ---------
            x0 : initial state (..., n)
            steps : number S of MPC steps, >= 1
            disturbance : (..., S, n), added to the successor state of every step; None: none
            clip_tol : the demo's 1e-6; None: the state is not clipped
            return_predictions : keep the rollout of every step
            xRef (..., S + N, n), uRef (..., S + N - 1, m) : references to track; step s tracks rows s : s+N+1 of xRef and s : s+N of
                uRef.  Either may be None (a Trajectory is not accepted: the two lengths differ from a Trajectory's).
            **solver_opts : the options of `solve`; warm_start (default "shift") applies to the steps after the first, which is always
                a cold start.
            Leading axes of x0, disturbance, xRef, uRef broadcast against each other and the problem shape.

        Returns
        -------
            MpcClosedLoop(xTraj (..., S+1, n), uTraj (..., S, m), status (..., S) strings, iterations (..., S) int32,
                          predictions: None or Trajectory((..., S, N+1, n), (..., S, N, m)))
        """
        S, clip = _run_steps(steps, clip_tol)
        eps_abs, eps_rel, max_iter, rho, adaptive, eps_pinf, alpha, warm = self._solver_options(solver_opts, "shift")
        if isinstance(xRef, Trajectory) or isinstance(uRef, Trajectory):
            raise ValueError("simulate takes xRef (..., steps + N, n) and uRef (..., steps + N - 1, m) as arrays, not a Trajectory")
        tracking = xRef is not None or uRef is not None
        N, n, m = self.N, self.n, self.m

        # 1. shapes
        per = (("disturbance", disturbance, (S, self._n_user), n), ("xRef", xRef, (S + N, self._n_user), n),
               ("uRef", uRef, (S + N - 1, self._m_user), m))
        lead, Bn = self._batch_shape(x0, per, f" for steps = {S}, N = {N}")
        arr.require_gpu()

        # 2. the problem on the device and its tables (shared with `solve`: they depend on the problem and the penalty only)
        d, (K, Mi, n_levels, level0, drho, *_), Pn = self._problem_on_device(rho, adaptive)

        # 3. one row per instance (the disturbance step-major) and the instance -> problem map; device placement as in `solve`
        dev, dx0, (dw, dxr, dur), prob = self._device_rows(lead, Bn, d, tracking or self._soft is not None, x0, per)
        dw = None if dw is None else dw.transpose(0, 1).contiguous()

        # 4. outputs (step-major on the device) and the run's own workspace
        xs, us, st, its, xp, up, ws = _run_buffers(S, Bn, N, n, m, dev, return_predictions, tracking)

        # 5. the C call (after `soften`: the sibling entry, the weights behind the box)
        if Bn > 0:
            run, box = _lib.lib().zm_mpc_closed_loop_f64, "x_lb x_ub u_lb u_ub"
            if self._soft is not None:
                run, box = _lib.lib().zm_mpc_closed_loop_soft_f64, box + " soft_l1 soft_l2"
            rc = run(
                *_ptrs(d, "A B Q R Qf", K, Mi), n_levels, level0, self.RHO_STEP, alpha, *_ptrs(d, box, dx0, dxr, dur),
                S + N, S + N - 1, rho if self.P is None else 0.0, *_ptrs(d, "", drho, prob), Pn, eps_abs, eps_rel, eps_pinf, max_iter, warm,
                S, clip, *_ptrs(d, "", dw, ws, xs, us, st, its, xp, up), Bn, N, n, m, ctypes.c_void_p(arr.stream_ptr(dx0)))
            _lib.check(rc, "lqrMpc.simulate")

        return self._run_results(lead, S, x0, (xs, us, st, its, xp, up))

    def _run_results(self, lead, S, x0, out):
        """What a run returns: batch-leading views of its step-major device arrays (xs, us, st, its, xp | None, up | None)"""
        xs, us, st, its, xp, up = out
        N, n, m, nu, mu = self.N, self.n, self.m, self._n_user, self._m_user
        view = lambda t, tail, width: arr.result_like(t.transpose(0, 1).reshape(lead + tail)[..., :width], x0)
        codes = st.transpose(0, 1).reshape(lead + (S,)).cpu().numpy()
        status = np.vectorize(_STATUS.get, otypes=[object])(codes) if codes.size > 0 else np.empty(lead + (S,), dtype=object)
        pred = None
        if xp is not None:
            pred = Trajectory(view(xp, (S, N + 1, n), nu), view(up, (S, N, m), mu))
        return MpcClosedLoop(view(xs, (S + 1, n), nu), view(us, (S, m), mu), status, view(its, (S,), None), pred)


class ltvMpc(lqrMpc):
    """Box-constrained MPC with stage-varying affine dynamics (extension),

        x_{k+1} = A_k x_k + B_k u_k + c_k,   k = 0 .. N-1,

    under lqrMpc's cost, bounds and ADMM: the QP that linearising a model about a TRAJECTORY gives (real-time-iteration nonlinear MPC,
    gain-scheduled horizons, periodic systems).  `solve` is lqrMpc's, with its options, return values, status strings, warm and shifted
    starts and tracking keywords; the kernels read their dynamics per stage and carry the offset (zm_mpc_setup_ltv_f64,
    zm_mpc_solve_ltv_f64).  Only the 16-lanes-per-instance kernels exist for this form: n <= 12, m <= 4 (smaller shapes are embedded per
    stage, as lqrMpc embeds them) and horizons whose iterates fit LDS, N <= 75; ZOPT_AMD_MPC_PATH does not apply.

    With `stage_varying=` the weights and the box vary by stage as well (zm_mpc_setup_ltv_stage_f64, zm_mpc_solve_ltv_stage_f64):

        minimise   sum_{k<N} (x_k - xr_k)' Q_k (x_k - xr_k) + (u_k - ur_k)' R_k (u_k - ur_k)  +  (x_N - xr_N)' Q_N (x_N - xr_N)
        subject to x_lb[k] <= x_k <= x_ub[k],  k = 0 .. N;     u_lb[k] <= u_k <= u_ub[k],  k = 0 .. N-1

    -- a corridor or gate that moves along the horizon, a terminal set tighter than the stage box, tube tightening, a waypoint weight,
    a discounted cost, the blocks c_xx, c_uu of a cost expanded about the plan.  Row 0 of the state box is the test on x0 (an x0 outside
    it is "infeasible"); Q[..., 0] weights a fixed state and is only checked.

    With soft weights (x_soft_l1, x_soft_l2, u_soft_l1, u_soft_l2; zm_mpc_solve_ltv_soft_f64) a component of x_k (k >= 1) or u_k whose l1
    is finite is not held inside its box: it pays l1 d + l2 d^2 for its distance d from it.  Such a problem always has a solution -- a
    state that a disturbance has pushed outside a corridor is solved from, not "infeasible" --, and with l1 above the constraint's
    multiplier the solution is the hard one whenever that exists.  `update` takes new weights without a setup launch.
    """

    _LTV = True
    _COMPILED = tuple(s for s in lqrMpc._COMPILED if s[0] + s[1] <= 16)
    _STAGED = {"Q": 1, "R": 0, "x_lb": 1, "x_ub": 1, "u_lb": 0, "u_ub": 0}   # what may vary by stage: rows beyond N of its stage axis

    def __init__(self, A, B, Q, R, N, x_lb, x_ub, u_lb, u_ub, Qf=None, c=None, stage_varying=(), x_soft_l1=None, x_soft_l2=None,
                 u_soft_l1=None, u_soft_l2=None):
        """
        Arguments
        ---------
            A : (..., N, n, n)   B : (..., N, n, m)   c : (..., N, n) or None (zeros) -- the dynamics of every stage
            Q, R, Qf, x_lb, x_ub, u_lb, u_ub, N : as lqrMpc takes them, leading axes included (the weights, with or without a stage axis,
                are replaced by their symmetric parts, as lqrMpc replaces them; `update` does the same with new ones)
            stage_varying : names among "Q", "R", "x_lb", "x_ub", "u_lb", "u_ub"; a named argument carries a stage axis in front of its
                trailing axes -- Q (..., N+1, n, n), R (..., N, m, m), x_lb, x_ub (..., N+1, n), u_lb, u_ub (..., N, m).  (Named, because a
                stage axis cannot be told from a leading problem axis by its shape.)  With "Q" named, Q[..., N] is the terminal weight
                and Qf must be None.  The attributes keep the stage-axis shapes.
            x_soft_l1, x_soft_l2 (..., n), u_soft_l1, u_soft_l2 (..., m) : penalty weights of soft box constraints, per problem and
                component, constant over the stages.  With d the distance of a component of x_k (k >= 1) or u_k from its box the cost gains
                l1 d + l2 d^2 and the bounds of that component no longer constrain it; l1 = +inf (the default of a weight not given)
                keeps the component hard, and l2 must be 0 there.  A start x0 outside row 0 of the state box in a soft component is
                solved from; in a hard one it is "infeasible" as before.  With an l1 above the hard problem's multipliers the hard
                solution comes back whenever there is one.  All four None: every bound is hard, nothing changes.
        The leading axes broadcast to the problem shape `P`; () is one problem.  Nothing here touches a GPU.
        """
        self.stage_varying = frozenset(stage_varying)
        if self.stage_varying:
            self._init_stage_varying(A, B, Q, R, N, x_lb, x_ub, u_lb, u_ub, Qf, c)
            return self._init_soft(x_soft_l1, x_soft_l2, u_soft_l1, u_soft_l2)
        if Qf is None:
            Qf = Q
        self.N = int(N)
        data = {k: _host_f64(X) for k, X in zip(_ARRAYS, (A, B, Q, R, Qf, x_lb, x_ub, u_lb, u_ub))}
        data["c"] = None if c is None else _host_f64(c)
        n, m, P = _ltv_problem_shape(data, self.N)
        self.P = P
        _symmetric_part(data)
        _check_psd(data, P)
        if n > 12 or m > 4:
            raise ValueError(f"ltvMpc: (n={n}, m={m}) outside the kernels for stage-varying dynamics (n <= 12, m <= 4)")
        if self.N > self.N_MAX:
            raise ValueError(f"ltvMpc: N={self.N} beyond the horizons whose iterates fit LDS (N <= {self.N_MAX})")
        self._dev = None
        self._tables = {}
        self._ws = None
        self.rho = _penalty(data["Q"], data["R"], P)
        self._n_user, self._m_user = n, m
        self.n, self.m = min(((ns, mc) for (ns, mc) in self._COMPILED if ns >= n and mc >= m), key=lambda t: (t[0] * t[1], t[0]))
        # per stage what _embed does per problem: A_k, B_k padded with zero blocks, c_k with zeros, the extra weights 1, no extra bound
        stage = _embed({k: data[k] for k in ("A", "B")}, P + (self.N,), self.n, self.m)
        fixed = _embed({k: data[k] for k in _ARRAYS[2:]}, P, self.n, self.m)
        cs = np.zeros(P + (self.N, self.n))
        if data["c"] is not None:
            cs[..., :n] = data["c"]
        for k, X in {**stage, **fixed, "c": cs}.items():
            setattr(self, k, X)
        self._init_soft(x_soft_l1, x_soft_l2, u_soft_l1, u_soft_l2)

    def _init_soft(self, *weights):
        """The constructor's last step: the penalty weights of soft box constraints.  With any of them the object keeps its data in stage
        form (constant rows without stage_varying=, which give the plain tables and iterates bit for bit) and solves through
        zm_mpc_solve_ltv_soft_f64."""
        self._stage_entry = bool(self.stage_varying)
        if all(w is None for w in weights):
            return
        self._soft = dict(zip(self._SOFT, weights))
        self.soft_l1, self.soft_l2 = self._soft_stacked("ltvMpc", self._soft)
        self._stage_entry = True

    def _init_stage_varying(self, A, B, Q, R, N, x_lb, x_ub, u_lb, u_ub, Qf, c):
        """The constructor with a non-empty `stage_varying`: the same checks, per stage where an array has a stage axis."""
        sv = self.stage_varying
        if not sv <= set(self._STAGED):
            raise ValueError(f"ltvMpc: stage_varying names {sorted(sv - set(self._STAGED))}, expected names among {sorted(self._STAGED)}")
        if "Q" in sv:
            if Qf is not None:
                raise ValueError("ltvMpc: with \"Q\" in stage_varying Q[..., N] is the terminal weight: Qf must be None")
        elif Qf is None:
            Qf = Q
        self.N = N = int(N)
        data = {k: None if X is None else _host_f64(X) for k, X in zip(_ARRAYS, (A, B, Q, R, Qf, x_lb, x_ub, u_lb, u_ub))}
        data["c"] = None if c is None else _host_f64(c)
        n, m, P = _ltv_problem_shape(data, N, {k: N + self._STAGED[k] for k in sv})
        self.P = P
        _symmetric_part(data)
        _check_psd_stages(data, P, sv)
        if n > 12 or m > 4:
            raise ValueError(f"ltvMpc: (n={n}, m={m}) outside the kernels for stage-varying dynamics (n <= 12, m <= 4)")
        if N > self.N_MAX:
            raise ValueError(f"ltvMpc: N={N} beyond the horizons whose iterates fit LDS (N <= {self.N_MAX})")
        self._dev = None
        self._tables = {}
        self._ws = None
        # one penalty per problem: lqrMpc's rule on (the weight of x_{k+1}, the weight of u_k) of every stage, then the median over the
        # stages -- of constant rows the value itself.  (A Q without a stage axis stands for every row, as in ltvMpc's own rule.)
        Qn = data["Q"][..., 1:, :, :] if "Q" in sv else data["Q"][..., None, :, :]
        Rn = data["R"] if "R" in sv else data["R"][..., None, :, :]
        self.rho = np.asarray(np.median(_penalty(Qn, Rn, P + (N,)), axis=-1))
        self._n_user, self._m_user = n, m
        self.n, self.m = min(((ns, mc) for (ns, mc) in self._COMPILED if ns >= n and mc >= m), key=lambda t: (t[0] * t[1], t[0]))
        # per stage what _embed does per problem: extra weights 1, extra bounds +-inf
        out = _embed({k: data[k] for k in ("A", "B")}, P + (N,), self.n, self.m)
        for k in _ARRAYS[2:]:
            if data[k] is not None:
                out.update(_embed({k: data[k]}, P + ((N + self._STAGED[k],) if k in sv else ()), self.n, self.m))
        if "Q" in sv:
            out["Qf"] = out["Q"][..., N, :, :]
        cs = np.zeros(P + (N, self.n))
        if data["c"] is not None:
            cs[..., :n] = data["c"]
        for k, X in {**out, "c": cs}.items():
            setattr(self, k, X)

    def _stage_form(self):
        """The six in stage form (host): Qs (P,N,n,n) with Qs[k] the weight of x_{k+1}, Rs (P,N,m,m), the box in the kernels' stacked
        stage layout lo, hi (P,N,n+m) with row k = [bound of x_{k+1} ; bound of u_k], and row 0 of the state box x_lb0, x_ub0 (P,n)."""
        N, sv, P = self.N, self.stage_varying, self.P
        rows = lambda X, name, r: X if name in sv else np.broadcast_to(X[..., None, :], P + (r, X.shape[-1]))
        if "Q" in sv:
            Qs = self.Q[..., 1:, :, :]
        else:
            Qs = np.concatenate([np.broadcast_to(self.Q[..., None, :, :], P + (N - 1, self.n, self.n)), self.Qf[..., None, :, :]], axis=-3)
        Rs = self.R if "R" in sv else np.broadcast_to(self.R[..., None, :, :], P + (N, self.m, self.m))
        xl, xu = rows(self.x_lb, "x_lb", N + 1), rows(self.x_ub, "x_ub", N + 1)
        ul, uu = rows(self.u_lb, "u_lb", N), rows(self.u_ub, "u_ub", N)
        return {"Qs": Qs, "Rs": Rs, "lo": np.concatenate([xl[..., 1:, :], ul], axis=-1), "hi": np.concatenate([xu[..., 1:, :], uu], axis=-1),
                "x_lb0": xl[..., 0, :], "x_ub0": xu[..., 0, :]}

    @classmethod
    def fromExpansion(cls, dyn, traj, Q, R, x_lb, x_ub, u_lb, u_ub, Qf=None, stage_varying=(), **soft):
        """The problem of an `AffineDynamics` (f, f_x, f_u) expanded about `traj` (AffineDynamics.from_trajectory(model, traj)): in absolute
        coordinates x+ ~ f + f_x (x - xbar_k) + f_u (u - ubar_k), i.e. A_k = f_x, B_k = f_u, c_k = f - f_x xbar_k - f_u ubar_k.  N is the
        number of stages of the expansion; bounds and references are in absolute coordinates.  **soft: the constructor's x_soft_l1,
        x_soft_l2, u_soft_l1, u_soft_l2."""
        f, f_x, f_u = (_host_f64(X) for X in tuple.__iter__(dyn))
        xbar, ubar = _host_f64(tuple.__getitem__(traj, 0))[..., :-1, :], _host_f64(tuple.__getitem__(traj, 1))
        c = f - np.einsum("...ij,...j->...i", f_x, xbar) - np.einsum("...ij,...j->...i", f_u, ubar)
        return cls(f_x, f_u, Q, R, f.shape[-2], x_lb, x_ub, u_lb, u_ub, Qf=Qf, c=c, stage_varying=stage_varying, **soft)

    def update(self, A=None, B=None, c=None, Q=None, R=None, x_lb=None, x_ub=None, u_lb=None, u_ub=None, x_soft_l1=None, x_soft_l2=None,
               u_soft_l1=None, u_soft_l2=None):
        """New dynamics data of the same shapes (the next linearisation of a real-time-iteration loop).  NumPy arrays or torch tensors; a
        device tensor is copied device to device, without a host copy (the attributes A, B, c then keep the data they had).  The tables
        are rebuilt by one setup launch before the next solve; the warm-start workspace survives.

        An object built with `stage_varying=` also takes new weights and bounds, in the shapes its constructor took them (the next window
        of a moving corridor).  New bounds rewrite the device boxes and keep the tables: nothing is launched but the copies.  New Q or R
        are checked as the constructor checks them (on the host: a device tensor is copied there for it) and drop the tables.  The
        penalty `rho` stays what the constructor chose.  The warm-start workspace survives either.

        An object built with soft weights also takes new ones (x_soft_l1, x_soft_l2, u_soft_l1, u_soft_l2, in the constructor's shapes
        and under its checks; the others stay): the device weights are rewritten, the tables and the workspace stay, nothing is
        launched but the copy.  All-inf l1 makes every bound hard again."""
        soft = {k: X for k, X in zip(self._SOFT, (x_soft_l1, x_soft_l2, u_soft_l1, u_soft_l2)) if X is not None}
        if soft:
            self._update_soft(soft)
        more = {k: X for k, X in (("Q", Q), ("R", R), ("x_lb", x_lb), ("x_ub", x_ub), ("u_lb", u_lb), ("u_ub", u_ub)) if X is not None}
        if more:
            self._update_stage_data(more)
        n, m, N = self._n_user, self._m_user, self.N
        new = {}
        for name, X, tail in (("A", A, (N, n, n)), ("B", B, (N, n, m)), ("c", c, (N, n))):
            if X is None:
                continue
            shp = tuple(X.shape) if hasattr(X, "shape") else np.shape(X)
            ok = len(shp) >= len(tail) and shp[len(shp) - len(tail):] == tail
            if ok:
                try:
                    ok = np.broadcast_shapes(shp[:len(shp) - len(tail)], self.P) == self.P
                except ValueError:
                    ok = False
            if not ok:
                raise ValueError(f"ltvMpc.update: {name} has shape {shp}, expected {('...',) + tail} with leading axes that broadcast "
                                 f"to the problem shape {self.P} (N = {N})")
            new[name] = (X, tail)
        if not new:
            return
        arr.require_gpu()
        d = self._device_data()
        Pn = int(np.prod(self.P))
        for name, (X, tail) in new.items():
            t = arr.to_device(X, torch.float64, d["A"].device).expand(self.P + tail).reshape((Pn,) + tail)
            d[name][(slice(None), slice(None)) + tuple(slice(0, w) for w in tail[1:])].copy_(t)   # (the padded part stays as it is)
            if not (arr.is_torch(X) and X.is_cuda):
                getattr(self, name)[(Ellipsis,) + tuple(slice(0, w) for w in tail[1:])] = _host_f64(X)
        self._tables = {}

    def _update_soft(self, new):
        """update()'s penalty weights: checked with the ones that stay, then the host attributes and the device copies"""
        if self._soft is None:
            raise ValueError(f"ltvMpc.update: new {', '.join(new)} need an object built with soft weights (this one keeps every bound hard "
                             f"and solves through the entry points without them: build a new object)")
        given = {**self._soft, **new}
        l1, l2 = self._soft_stacked("ltvMpc.update", given)
        self._soft, self.soft_l1, self.soft_l2 = given, l1, l2
        if self._dev is not None:
            Pn = int(np.prod(self.P))
            for k, X in (("soft_l1", l1), ("soft_l2", l2)):
                self._dev[k].copy_(arr.to_device(X.reshape(Pn, -1), torch.float64, self._dev[k].device))

    def _update_stage_data(self, new):
        """update()'s weights and bounds: shape checks first, then the host attributes and the stage-form device arrays"""
        if not self.stage_varying:
            raise ValueError(f"ltvMpc.update: new {', '.join(new)} need an object built with stage_varying= (this one keeps one set of "
                             f"weights and bounds per problem: build a new object)")
        n, m, N, sv, P = self._n_user, self._m_user, self.N, self.stage_varying, self.P
        tails = {"Q": (n, n), "R": (m, m), "x_lb": (n,), "x_ub": (n,), "u_lb": (m,), "u_ub": (m,)}
        for name, X in new.items():
            tail = ((N + self._STAGED[name],) if name in sv else ()) + tails[name]
            shp = _shape_of(X)
            ok = len(shp) >= len(tail) and shp[len(shp) - len(tail):] == tail
            if ok:
                try:
                    ok = np.broadcast_shapes(shp[:len(shp) - len(tail)], P) == P
                except ValueError:
                    ok = False
            if not ok:
                raise ValueError(f"ltvMpc.update: {name} has shape {shp}, expected {('...',) + tail} with leading axes that broadcast "
                                 f"to the problem shape {P} (N = {N})")
            tails[name] = tail
        if "Q" in new and "Q" not in sv and self.N == 1:
            raise ValueError("ltvMpc.update: with N = 1 and no stage axis on Q the only weight is Qf, which update() does not take")
        host = {k: _host_f64(X) for k, X in new.items() if k in ("Q", "R") or not (arr.is_torch(X) and X.is_cuda)}
        _symmetric_part(host)
        new = {k: host[k] if k in ("Q", "R") else X for k, X in new.items()}   # (the weights go to the device as their symmetric parts)
        _check_psd_stages({k: host.get(k) for k in ("Q", "R", "Qf")}, P, sv)
        arr.require_gpu()
        d = self._device_data()
        Pn = int(np.prod(P))
        ns = self.n
        for name, X in new.items():
            tail = tails[name]
            if name in host:
                getattr(self, name)[(Ellipsis,) + tuple(slice(0, w) for w in tail[-(2 if name in ("Q", "R") else 1):])] = host[name]
            t = arr.to_device(X, torch.float64, d["A"].device).expand(P + tail).reshape((Pn,) + tail)
            if name not in sv:   # (one row for every stage)
                t = t[:, None]
            if name == "Q":      # row 0 weights the fixed x_0; without a stage axis the terminal row stays Qf
                src = t[:, 1:] if name in sv else t
                d["Qs"][:, :(N if name in sv else N - 1), :n, :n].copy_(src.expand((Pn, N if name in sv else N - 1, n, n)))
            elif name == "R":
                d["Rs"][:, :, :m, :m].copy_(t.expand((Pn, N, m, m)))
            elif name in ("x_lb", "x_ub"):
                box, row0 = ("lo", "x_lb0") if name == "x_lb" else ("hi", "x_ub0")
                d[row0][:, :n].copy_(t[:, 0])
                d[box][:, :, :n].copy_((t[:, 1:] if name in sv else t).expand((Pn, N, n)))
            else:
                d["lo" if name == "u_lb" else "hi"][:, :, ns:ns + m].copy_(t.expand((Pn, N, m)))
        if "Q" in new or "R" in new:
            self._tables = {}

    def soften(self, *args, **kwargs):
        raise TypeError("ltvMpc.soften: ltvMpc takes its soft weights as constructor arguments (x_soft_l1, x_soft_l2, u_soft_l1, "
                        "u_soft_l2) and new ones through update(x_soft_l1=..., ...)")

    def simulate(self, *args, **kwargs):
        raise NotImplementedError("ltvMpc.simulate: a moving window needs new tables at every step; loop over update() and solve(), or -- "
                                  "for a registered model linearised about the moving plan -- call realTimeIteration()")

    def _device_problem(self, rho, adaptive):   # (a single problem is the per-problem form with P = ())
        raise NotImplementedError

    def _device_data(self):
        if self._dev is None:
            Pn = int(np.prod(self.P))
            flat = lambda X: arr.to_device(np.ascontiguousarray(X).reshape((Pn,) + X.shape[len(self.P):]), torch.float64)
            if self._stage_entry:   # (the six once, in the stage form the stage entry points read; the soft weights behind them)
                self._dev = {**{k: flat(getattr(self, k)) for k in ("A", "B", "c")}, **{k: flat(X) for k, X in self._stage_form().items()}}
                if self._soft is not None:
                    self._dev.update(soft_l1=flat(self.soft_l1), soft_l2=flat(self.soft_l2))
            else:
                self._dev = {k: flat(getattr(self, k)) for k in _ARRAYS + ("c",)}
        return self._dev

    def _empty_tables(self, rho, adaptive):
        """The tuple `_device_problem_batched` keeps, its tables allocated and not yet written."""
        d = self._device_data()
        Pn = int(np.prod(self.P))
        nl = self.N_LEVELS if adaptive else 1
        l0 = nl // 2
        dev = d["A"].device
        fac = np.array([self.RHO_STEP ** (l - l0) for l in range(nl)])
        rtab = arr.to_device(rho.reshape(Pn, 1) * fac[None, :], torch.float64, dev)
        E = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
        K, Mi, D = E(Pn, nl, self.N, self.m, self.n), E(Pn, nl, self.N, self.m, self.m), E(Pn, nl, self.N, self.n)
        ABt = E(Pn, self.N, self.n + self.m, self.n)
        return (K, Mi, nl, l0, arr.to_device(rho.reshape(Pn), torch.float64, dev), rtab, D, ABt)

    def _device_problem_batched(self, rho, adaptive):
        """Device copies of the data and the tables of every (problem, penalty level): ONE setup launch.  The tuple lqrMpc keeps, then
        D (P, L, N, n) and ABt (P, N, n + m, n)."""
        arr.require_gpu()
        d = self._device_data()
        key = (rho.tobytes(), bool(adaptive))
        if key not in self._tables:
            tabs = self._empty_tables(rho, adaptive)
            K, Mi, nl, _, _, rtab, D, ABt = tabs
            setup, weights = ((_lib.lib().zm_mpc_setup_ltv_stage_f64, "Qs Rs") if self._stage_entry else
                              (_lib.lib().zm_mpc_setup_ltv_f64, "Q R Qf"))
            rc = setup(*_ptrs(d, "A B c " + weights, rtab), int(np.prod(self.P)), nl, self.N, self.n, self.m,
                       *_ptrs(d, "", K, Mi, D, ABt), ctypes.c_void_p(arr.stream_ptr(K)))
            _lib.check(rc, "ltvMpc setup")
            self._tables[key] = tabs
        return d, self._tables[key]

    # ---- real-time iteration: a registered model linearised about the moving plan --------------------------------------------------

    @classmethod
    def fromModel(cls, model, plan, Q, R, x_lb, x_ub, u_lb, u_ub, Qf=None, stage_varying=(), **soft):
        """The problem of a registered model (models.QuadcopterEuler, models.QuadcopterRigidBody with dt > 0, models.LinearModel; n <= 12,
        m <= 4) linearised about `plan`, a Trajectory (xTraj (..., N+1, n), uTraj (..., N, m)) in absolute coordinates: what
        `fromExpansion(AffineDynamics.from_trajectory(model, plan), plan, ...)` builds, with c_k formed on the device as `relinearize` forms
        it.  N is the plan's stage count and the plan's leading axes the problem shape (every trajectory is its own problem).  The
        expansion runs on the device once and is copied to the host for the constructor, which is host-only."""
        n, m = _model_shape("ltvMpc.fromModel", model)
        xs, us, lead = _plan_shapes("ltvMpc.fromModel", plan, None, n, m)
        N = us[-2]
        arr.require_gpu()
        Bn = int(np.prod(lead))
        xP = arr.to_device(tuple.__getitem__(plan, 0), torch.float64).expand(lead + (N + 1, n)).reshape(Bn, N + 1, n).contiguous()
        uP = arr.to_device(tuple.__getitem__(plan, 1), torch.float64, xP.device).expand(lead + (N, m)).reshape(Bn, N, m).contiguous()
        Z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=xP.device)
        A, B, c = Z(Bn, N, n, n), Z(Bn, N, n, m), Z(Bn, N, n)
        cs = model.c_struct()
        rc = _lib.lib().zm_mpc_relinearize_f64(ctypes.addressof(cs), xP.data_ptr(), uP.data_ptr(), A.data_ptr(), B.data_ptr(), c.data_ptr(),
                                               Bn, N, n, m, n, m, ctypes.c_void_p(arr.stream_ptr(xP)))
        _lib.check(rc, "ltvMpc.fromModel")
        host = lambda t, tail: t.cpu().numpy().reshape(lead + tail)
        return cls(host(A, (N, n, n)), host(B, (N, n, m)), Q, R, N, x_lb, x_ub, u_lb, u_ub, Qf=Qf, c=host(c, (N, n)),
                   stage_varying=stage_varying, **soft)

    def relinearize(self, model, plan):
        """The next linearisation of a real-time-iteration loop, on the device: `model` expanded about `plan` (a Trajectory, xTraj
        (..., N+1, n), uTraj (..., N, m) in absolute coordinates, leading axes that broadcast to the problem shape) straight into the
        problem's device arrays -- A_k = f_x, B_k = f_u, c_k = f - f_x xbar_k - f_u ubar_k (zm_mpc_relinearize_f64) -- the device-side
        equivalent of `update(A=f_x, B=f_u, c=c)` with device tensors: the host attributes A, B, c keep the data they had, the tables are
        rebuilt before the next solve, the warm-start workspace survives.  NumPy arrays or torch tensors; contiguous device tensors of
        the problem's shape are read in place."""
        n, m, N = self._n_user, self._m_user, self.N
        _model_shape("ltvMpc.relinearize", model, (n, m))
        _plan_shapes("ltvMpc.relinearize", plan, N, n, m, self.P)
        arr.require_gpu()
        d = self._device_data()
        Pn = int(np.prod(self.P))
        dev = d["A"].device
        xP = arr.to_device(tuple.__getitem__(plan, 0), torch.float64, dev).expand(self.P + (N + 1, n)).reshape(Pn, N + 1, n).contiguous()
        uP = arr.to_device(tuple.__getitem__(plan, 1), torch.float64, dev).expand(self.P + (N, m)).reshape(Pn, N, m).contiguous()
        cs = model.c_struct()
        rc = _lib.lib().zm_mpc_relinearize_f64(ctypes.addressof(cs), xP.data_ptr(), uP.data_ptr(), d["A"].data_ptr(), d["B"].data_ptr(),
                                               d["c"].data_ptr(), Pn, N, n, m, self.n, self.m, ctypes.c_void_p(arr.stream_ptr(xP)))
        _lib.check(rc, "ltvMpc.relinearize")
        self._tables = {}

    def realTimeIteration(self, model, x0, steps, plan=None, plant=None, disturbance=None, clip_tol=1e-6, return_predictions=False,
                          xRef=None, uRef=None, **solver_opts):
        """
        Real-time-iteration nonlinear MPC as one call, entirely on the device (zm_mpc_rti_f64): linearise `model` about the shifted
        previous plan, solve the stage-varying QP from the shifted iterates, apply the first input through the nonlinear `plant`, repeat.
        It replaces this loop of public calls, and gives its results bit for bit:

            plan given;  x = x0
            for s in range(steps):
                if clip_tol is not None: x = clip(x, x_lb + clip_tol, x_ub - clip_tol)
                xTraj[s] = x
                self.relinearize(model, plan)
                u, traj, status[s] = self.solve(x, window s of xRef / uRef, warm_start=(False if s == 0 else W), **solver_opts)
                uTraj[s] = u;  iterations[s] = self.last_iterations
                x = modelStep(plant, x, u) + (disturbance[s] if disturbance is not None else 0)
                plan = Trajectory(rows 1.. of traj.xTraj with the last repeated, rows 1.. of traj.uTraj with the last repeated)
            xTraj[steps] = clip(x, ...) if clip_tol is not None else x

        whatever the status of a step (a step that is not "optimal" still leaves a rollout, and the step after it starts cold).  The head
        of the shifted plan is the PREDICTED successor, not the measured one.  The object is left as that loop leaves it: its device
        dynamics are the last linearisation, its tables, warm-start workspace, `last_iterations` and `last_residuals` those of the last
        step; the host attributes A, B, c are untouched (as `update` with device tensors leaves them).

        Arguments
        ---------
            model : the registered model that is linearised, of the problem's (n, m)
            x0 : initial states, (..., n) with leading axes that broadcast to the problem shape: every instance is its own problem
            steps : number S of MPC steps, >= 1
            plan : the first expansion point, a Trajectory (xTraj (..., N+1, n), uTraj (..., N, m)) in absolute coordinates (it is not
                modified); None: the clipped x0 at every stage, with the first N rows of uRef as inputs (zeros without uRef)
            plant : the model the state is advanced with, of the same (n, m) (e.g. the quadcopter with wind); None: `model`
            disturbance (..., S, n), clip_tol, return_predictions, xRef (..., S + N, n), uRef (..., S + N - 1, m), **solver_opts :
                as `lqrMpc.simulate` takes them

        Returns
        -------
            MpcClosedLoop, as `lqrMpc.simulate` returns it

        Not with stage_varying= (NotImplementedError): the loop inside the call keeps one set of weights and bounds per problem.  Not
        with soft weights either: the loop inside the call solves with hard bounds.
        """
        if self._soft is not None:
            raise NotImplementedError("ltvMpc.realTimeIteration: the loop inside zm_mpc_rti_f64 solves with hard bounds; with soft weights "
                                      "write the loop out: relinearize(model, plan), solve(x, warm_start=\"shift\"), "
                                      "modelStep(plant, x, u)")
        if self.stage_varying:
            raise NotImplementedError("ltvMpc.realTimeIteration: the loop inside zm_mpc_rti_f64 keeps one set of weights and bounds per "
                                      "problem; with stage_varying= write the loop out: relinearize(model, plan), update(x_lb=..., "
                                      "x_ub=...), solve(x, warm_start=\"shift\"), modelStep(plant, x, u)")
        S, clip = _run_steps(steps, clip_tol)
        eps_abs, eps_rel, max_iter, rho, adaptive, eps_pinf, alpha, warm = self._solver_options(solver_opts, "shift")
        if isinstance(xRef, Trajectory) or isinstance(uRef, Trajectory):
            raise ValueError("realTimeIteration takes xRef (..., steps + N, n) and uRef (..., steps + N - 1, m) as arrays, not a Trajectory")
        N, n, m, nu, mu = self.N, self.n, self.m, self._n_user, self._m_user
        _model_shape("ltvMpc.realTimeIteration", model, (nu, mu))
        if plant is not None:
            _model_shape("ltvMpc.realTimeIteration", plant, (nu, mu), "plant")

        # 1. shapes: everything broadcasts to the problem shape (every instance is its own problem)
        per = (("disturbance", disturbance, (S, nu), n), ("xRef", xRef, (S + N, nu), n), ("uRef", uRef, (S + N - 1, mu), m))
        lead, Bn = self._batch_shape(x0, per, f" for steps = {S}, N = {N}", own=True, plan=plan)
        arr.require_gpu()

        # 2. the problem on the device; the tables of every step are written by the call (those of the last step stay, as a solve's do)
        d = self._device_data()
        tabs = self._empty_tables(rho, adaptive)
        K, Mi, n_levels, level0, drho, rtab, D, ABt = tabs

        # 3. one row per instance (the disturbance step-major), the identity as the instance -> problem map, the first plan
        dev, dx0, (dw, dxr, dur), prob = self._device_rows(lead, Bn, d, True, x0, per, identity=True)
        dw = None if dw is None else dw.transpose(0, 1).contiguous()
        if plan is not None:   # (copies: the call moves its plan on)
            xP = _flat(tuple.__getitem__(plan, 0), lead, Bn, (N + 1, nu), nu, dev).clone()
            uP = _flat(tuple.__getitem__(plan, 1), lead, Bn, (N, mu), mu, dev).clone()
        else:
            xh = dx0[:, :nu]
            if clip_tol is not None:
                xh = torch.minimum(torch.maximum(xh, d["x_lb"][:, :nu] + float(clip_tol)), d["x_ub"][:, :nu] - float(clip_tol))
            xP = xh[:, None, :].expand(Bn, N + 1, nu).contiguous()
            uP = torch.zeros((Bn, N, mu), dtype=torch.float64, device=dev) if dur is None else dur[:, :N, :mu].contiguous()

        # 4. outputs (step-major on the device); the workspace is the object's: step 0 starts cold, a later `solve` may start warm from it
        xs, us, st, its, xp, up, ws = _run_buffers(S, Bn, N, n, m, dev, return_predictions, True)
        res = torch.empty((Bn, 2), dtype=torch.float64, device=dev)
        self._ws = ((("tracking", lead), str(dev), rho.tobytes(), adaptive), ws)
        self._tables = {(rho.tobytes(), bool(adaptive)): tabs}

        # 5. the C call
        if Bn > 0:
            cs = model.c_struct()
            cp = None if plant is None else plant.c_struct()
            rc = _lib.lib().zm_mpc_rti_f64(
                ctypes.addressof(cs), None if cp is None else ctypes.addressof(cp), *_ptrs(d, "", xP, uP),
                *_ptrs(d, "A B c Q R Qf", rtab, K, Mi, D, ABt), n_levels, level0, self.RHO_STEP, alpha,
                *_ptrs(d, "x_lb x_ub u_lb u_ub", dx0, dxr, dur), S + N, S + N - 1, *_ptrs(d, "", drho, prob), eps_abs, eps_rel, eps_pinf,
                max_iter, warm, S, clip, *_ptrs(d, "", dw, ws, xs, us, st, its, res, xp, up), Bn, N, nu, mu, n, m,
                ctypes.c_void_p(arr.stream_ptr(dx0)))
            _lib.check(rc, "ltvMpc.realTimeIteration")

        # 6. results; the object's record of its last solve
        self.last_iterations = its[S - 1].reshape(lead).cpu().numpy()
        self.last_residuals = res.reshape(lead + (2,)).cpu().numpy()
        return self._run_results(lead, S, x0, (xs, us, st, its, xp, up))


def modelStep(model, x, u):
    """x+ = f(x, u): one step of a registered model (models.QuadcopterEuler, models.QuadcopterRigidBody, models.LinearModel; n <= 12,
    m <= 4) by its step function on the device (zm_model_step_f64) -- the plant of `ltvMpc.realTimeIteration` as a call of its own.
    x (..., n), u (..., m) with leading axes that broadcast against each other; NumPy in, NumPy out, device tensors in, device tensors out."""
    n, m = _model_shape("modelStep", model)
    sx, su = _shape_of(x), _shape_of(u)
    if len(sx) < 1 or sx[-1] != n or len(su) < 1 or su[-1] != m:
        raise ValueError(f"modelStep: x has shape {sx}, u has shape {su}, expected (..., {n}) and (..., {m})")
    try:
        lead = tuple(int(v) for v in np.broadcast_shapes(sx[:-1], su[:-1]))
    except ValueError:
        raise ValueError(f"modelStep: x of shape {sx}, u of shape {su} do not broadcast against each other: inconsistent shapes") from None
    arr.require_gpu()
    Bn = int(np.prod(lead))
    dx = arr.to_device(x, torch.float64)
    du = arr.to_device(u, torch.float64, dx.device)
    dx = dx.expand(lead + (n,)).reshape(Bn, n).contiguous()
    du = du.expand(lead + (m,)).reshape(Bn, m).contiguous()
    out = torch.empty((Bn, n), dtype=torch.float64, device=dx.device)
    cs = _models.model_struct(model, lead)
    rc = _lib.lib().zm_model_step_f64(ctypes.addressof(cs), dx.data_ptr(), du.data_ptr(), out.data_ptr(), Bn,
                                      ctypes.c_void_p(arr.stream_ptr(dx)))
    _lib.check(rc, "modelStep")
    return arr.result_like(out.reshape(lead + (n,)), x)


def _ptrs(d, names, *tensors):
    """The addresses a C call takes: of d[name] for every name in the string `names`, then of `tensors`; None stays None (NULL)"""
    return [None if t is None else t.data_ptr() for t in [d[k] for k in names.split()] + list(tensors)]


def _shape_of(X):
    return tuple(X.shape) if hasattr(X, "shape") else tuple(np.shape(X))


def _flat(X, lead, Bn, tail, width, dev):
    """X (..., *tail) on `dev` as one contiguous row per instance of the batch shape `lead` (Bn instances), its last axis zero-padded to
    `width`"""
    t = arr.to_device(X, torch.float64, dev)
    t = t.expand(lead + tail).reshape((Bn,) + tail)
    if width != tail[-1]:
        t = torch.nn.functional.pad(t, (0, width - tail[-1]))
    return t.contiguous()


def _run_steps(steps, clip_tol):
    """(S, the C side's clip_tol: -1 for none) of a run's `steps` and `clip_tol`"""
    S = int(steps)
    if S < 1:
        raise ValueError(f"steps must be at least 1, got {steps}")
    if clip_tol is not None and not (float(clip_tol) >= 0.0):
        raise ValueError(f"clip_tol must be non-negative (or None for no clip), got {clip_tol}")
    return S, -1.0 if clip_tol is None else float(clip_tol)


def _run_buffers(S, Bn, N, n, m, dev, keep, tracking):
    """The outputs of a run, step-major on the device: states, inputs, status, iterations, the predictions (`keep`, else None, None); then
    its workspace: the blocks of a solve (a fifth with `tracking`) and, unless the predictions are kept, the rollout every step
    overwrites"""
    f64 = dict(dtype=torch.float64, device=dev)
    xs = torch.empty((S + 1, Bn, n), **f64)
    us = torch.empty((S, Bn, m), **f64)
    st = torch.empty((S, Bn), dtype=torch.int32, device=dev)
    its = torch.empty((S, Bn), dtype=torch.int32, device=dev)
    xp = torch.empty((S, Bn, N + 1, n), **f64) if keep else None
    up = torch.empty((S, Bn, N, m), **f64) if keep else None
    ws = torch.empty((5 if tracking else 4) * Bn * N * (n + m) + (0 if keep else Bn * ((N + 1) * n + N * m)), **f64)
    return xs, us, st, its, xp, up, ws


def _model_shape(who, model, want=None, what="model"):
    """(n, m) of a registered model handle; ValueError outside the kernels' (12, 4), for a quadcopter without a step, or if it is not `want`"""
    n, m = getattr(model, "n", None), getattr(model, "m", None)
    if not callable(getattr(model, "c_struct", None)) or n is None or m is None:
        raise ValueError(f"{who}: the {what} must be a registered model (zopt_amd.models), got {type(model).__name__}")
    if who.startswith("ltvMpc"):      # (before anything touches the device)
        _models.refuse_traced(model, who, "the relinearisation and plant kernels of the real-time iteration on the tape interpreter "
                                          "are the follow-up")
    n, m = int(n), int(m)
    if n < 1 or m < 1 or n > 12 or m > 4:
        raise ValueError(f"{who}: the {what} has (n={n}, m={m}), outside the kernels for stage-varying dynamics (n <= 12, m <= 4)")
    if hasattr(model, "dt") and not (model.dt > 0.0):
        raise ValueError(f"{who}: the {what} needs a step dt > 0 (dt = {model.dt} is its continuous derivative)")
    if want is not None and (n, m) != tuple(want):
        raise ValueError(f"{who}: the {what} has (n={n}, m={m}), the problem (n={want[0]}, m={want[1]})")
    return n, m


def _plan_shapes(who, plan, N, n, m, P=None):
    """(shape of xTraj, shape of uTraj, their common leading axes) of a plan (xTraj (..., N+1, n), uTraj (..., N, m)); N None: the plan's
    own stage count; P: the leading axes must broadcast to it"""
    try:
        xT, uT = tuple.__getitem__(plan, 0), tuple.__getitem__(plan, 1)
    except Exception:
        raise ValueError(f"{who}: plan must be a Trajectory (xTraj, uTraj), got {type(plan).__name__}") from None
    xs, us = _shape_of(xT), _shape_of(uT)
    stages = us[-2] if (N is None and len(us) >= 2) else N
    ok = len(xs) >= 2 and len(us) >= 2 and stages is not None and stages >= 1 and xs[-2:] == (stages + 1, n) and us[-2:] == (stages, m)
    lead = None
    if ok:
        try:
            lead = tuple(int(v) for v in np.broadcast_shapes(xs[:-2], us[:-2]))
            ok = P is None or np.broadcast_shapes(lead, P) == P
        except ValueError:
            ok = False
    if not ok:
        want = "N" if stages is None else str(stages)
        raise ValueError(f"{who}: plan has xTraj of shape {xs} and uTraj of shape {us}, expected (..., {want} + 1, {n}) and (..., {want}, {m})"
                         + ("" if P is None else f" with leading axes that broadcast to the problem shape {P}"))
    return xs, us, lead


def _ltv_problem_shape(data, N, stage_rows=None):
    """(n, m, P) of ltvMpc's arrays: A (..., N, n, n), B (..., N, n, m), c (..., N, n) | None, the rest as lqrMpc's -- or, for a name in
    `stage_rows` (name -> rows), with a stage axis of that many rows in front of its trailing axes."""
    if data["B"].ndim < 3:
        raise ValueError("ltvMpc: B must have shape (..., N, n, m)")
    n, m = data["B"].shape[-2:]
    if N < 1:
        raise ValueError(f"ltvMpc: N = {N}, expected at least one stage")
    tails = {"A": (N, n, n), "B": (N, n, m), "c": (N, n), "Q": (n, n), "R": (m, m), "Qf": (n, n), "x_lb": (n,), "x_ub": (n,),
             "u_lb": (m,), "u_ub": (m,)}
    for k, r in (stage_rows or {}).items():
        tails[k] = (r,) + tails[k]
    lead = {}
    for k, t in tails.items():
        X = data[k]
        if X is None:
            continue
        staged = k in ("A", "B", "c") or k in (stage_rows or {})   # (the stage axis is checked on its own: its message names N)
        if X.ndim < len(t) or X.shape[X.ndim - len(t) + staged:] != t[staged:]:
            raise ValueError(f"inconsistent ltvMpc problem shapes: {k} has shape {X.shape}, expected (..., {', '.join(map(str, t))})")
        if staged and X.shape[X.ndim - len(t)] != t[0]:
            raise ValueError(f"inconsistent ltvMpc problem shapes: {k} of shape {X.shape} has {X.shape[X.ndim - len(t)]} stages, "
                             f"expected N = {N}" + ("" if t[0] == N else f" + {t[0] - N}"))
        lead[k] = X.shape[:X.ndim - len(t)]
    try:
        P = np.broadcast_shapes(*lead.values())
    except ValueError:
        raise ValueError("inconsistent ltvMpc problem shapes: the leading (problem) axes do not broadcast: "
                         + ", ".join(f"{k} {data[k].shape}" for k in lead)) from None
    return n, m, tuple(int(v) for v in P)



def _host_f64(X):
    """float64 NumPy copy of an array-like; torch tensors (host or device) included"""
    if torch is not None and isinstance(X, torch.Tensor):
        X = X.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(X, dtype=np.float64))


def _has_leading_axes(A, B, Q, R, Qf, x_lb, x_ub, u_lb, u_ub):
    """True if any problem array carries axes in front of its single-problem shape (matrices 2-D, bounds 1-D)"""
    nd = lambda X: len(X.shape) if hasattr(X, "shape") else np.ndim(X)
    return any(nd(X) > 2 for X in (A, B, Q, R, Qf)) or any(nd(v) > 1 for v in (x_lb, x_ub, u_lb, u_ub))


_ARRAYS = ("A", "B", "Q", "R", "Qf", "x_lb", "x_ub", "u_lb", "u_ub")


def _problem_shape(data, N, batched):
    """(n, m, P) of the constructor's arrays: P is the broadcast of their leading axes, () for one problem."""
    if data["B"].ndim < 2:
        raise ValueError("inconsistent lqrMpc problem shapes")
    n, m = data["B"].shape[-2:]
    tails = {"A": (n, n), "B": (n, m), "Q": (n, n), "R": (m, m), "Qf": (n, n), "x_lb": (n,), "x_ub": (n,), "u_lb": (m,), "u_ub": (m,)}
    if not batched:   # the single-problem constructor never looked at the other three
        tails = {k: tails[k] for k in ("A", "B", "Q", "R", "x_lb", "u_lb")}
    if N < 1 or any(data[k].ndim < len(t) or data[k].shape[data[k].ndim - len(t):] != t for k, t in tails.items()):
        raise ValueError("inconsistent lqrMpc problem shapes")
    try:
        P = np.broadcast_shapes(*(data[k].shape[:data[k].ndim - len(t)] for k, t in tails.items()))
    except ValueError:
        raise ValueError("inconsistent lqrMpc problem shapes: the leading (problem) axes do not broadcast: "
                         + ", ".join(f"{k} {data[k].shape}" for k in tails)) from None
    return n, m, tuple(int(v) for v in P)


def _symmetric_part(data):
    """The weights of `data` (Q, R, Qf where present and not None; trailing axes (k, k), any leading ones) replaced in place by their
    symmetric parts (W + W') / 2.  Only the quadratic form x'Wx enters the cost, which the antisymmetric part does not change; the setup
    kernels form the Hessian as 2 W and the tracking kernels the linear term with W + W', which agree for a symmetric W only.  For a
    symmetric W the result is W bit for bit (W + W is exact, and so is the halving)."""
    for name in ("Q", "R", "Qf"):
        W = data.get(name)
        if W is not None:
            data[name] = np.ascontiguousarray(0.5 * (W + np.swapaxes(W, -1, -2)))


def _check_psd(data, P):
    """cvxpy refuses the reference's problem (DCPError at solve time) unless every quad_form weight is positive semidefinite; here the
    ADMM's Hessians 2Q + rho I would hide a slightly indefinite weight and return the stationary point of a non-convex problem.  The
    first offending problem is named by its index in P."""
    for name in ("Q", "R", "Qf"):
        W = data[name]
        w = np.linalg.eigvalsh(0.5 * (W + np.swapaxes(W, -1, -2)))
        bad = np.broadcast_to(w[..., 0] < -1e-10 * np.maximum(1.0, np.abs(w[..., -1])), P)
        if bad.any():
            i = tuple(int(v) for v in np.argwhere(bad)[0])
            lo = float(np.broadcast_to(w[..., 0], P)[i])
            which = f"[{', '.join(map(str, i))}]" if i else ""
            raise ValueError(f"lqrMpc: {name}{which} is not positive semidefinite (smallest eigenvalue {lo:.3g}): "
                             f"the problem is not convex (cvxpy raises DCPError for the reference's quad_form)")


def _check_psd_stages(data, P, sv):
    """_check_psd for ltvMpc with stage_varying=: a weight named in `sv` is checked at every stage, and the first offender is named by
    its problem and its stage.  Entries that are None are skipped."""
    for name in ("Q", "R", "Qf"):
        W = data.get(name)
        if W is None:
            continue
        if name not in sv:
            _check_psd({k: (W if k == name else np.zeros((1, 1))) for k in ("Q", "R", "Qf")}, P)
            continue
        w = np.linalg.eigvalsh(0.5 * (W + np.swapaxes(W, -1, -2)))
        shape = P + (W.shape[-3],)
        bad = np.broadcast_to(w[..., 0] < -1e-10 * np.maximum(1.0, np.abs(w[..., -1])), shape)
        if bad.any():
            i = tuple(int(v) for v in np.argwhere(bad)[0])
            lo = float(np.broadcast_to(w[..., 0], shape)[i])
            which = f"[{', '.join(map(str, i[:-1]))}]" if i[:-1] else ""
            raise ValueError(f"ltvMpc: {name}{which} at stage {i[-1]} is not positive semidefinite (smallest eigenvalue {lo:.3g}): "
                             f"the problem is not convex")


def _penalty(Q, R, P):
    """One penalty per problem, shape P: the geometric mean of the cost curvatures keeps both blocks of the w-update Hessian
    (2Q + rho I, 2R + rho I) comparably conditioned.  A trace is the pairwise sum of the contiguous diagonal, as np.trace's."""
    tq = np.ascontiguousarray(np.diagonal(2 * Q, axis1=-2, axis2=-1)).sum(axis=-1) / Q.shape[-1]
    tr = np.ascontiguousarray(np.diagonal(2 * R, axis1=-2, axis2=-1)).sum(axis=-1) / R.shape[-1]
    return np.sqrt(np.broadcast_to(np.maximum(tq, 1e-12) * np.maximum(tr, 1e-12), P)).astype(np.float64)


def _embed(data, P, ns, mc):
    """Every array materialised to P and embedded in the compiled shape (ns, mc): zero blocks next to the matrices, the weights' new
    diagonal 1, A's and B's 0, the new components unbounded."""
    def mat(X, r, c, d):
        out = np.zeros(P + (r, c))
        out[..., :X.shape[-2], :X.shape[-1]] = X
        for i in range(min(r - X.shape[-2], c - X.shape[-1])):
            out[..., X.shape[-2] + i, X.shape[-1] + i] = d
        return out

    def vec(v, k, fill):
        out = np.full(P + (k,), fill)
        out[..., :v.shape[-1]] = v
        return out
    shape = {"A": (ns, ns, 0.0), "B": (ns, mc, 0.0), "Q": (ns, ns, 1.0), "R": (mc, mc, 1.0), "Qf": (ns, ns, 1.0)}
    bound = {"x_lb": (ns, -np.inf), "x_ub": (ns, np.inf), "u_lb": (mc, -np.inf), "u_ub": (mc, np.inf)}
    return {k: mat(X, *shape[k]) if k in shape else vec(X, *bound[k]) for k, X in data.items()}
