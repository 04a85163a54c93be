"""Every refusal of the MPC solve and run entry points that is reached before the first HIP call: return code and full message, and --
where two checks are violated at once -- which of them wins.  CPU only: the library is called with dummy pointers, as
test_abi.py::test_bad_arguments_return_codes_without_gpu does; nothing here dereferences one (the model blocks are real host structs).

Each row is (entry, overrides of that entry's valid argument set, return code, zm_last_error()).  The valid set itself would go on to
the device, so every row breaks at least one check; a row with None as its message only pins the return code (the early return of an
empty batch sets no message)."""
import ctypes

import pytest

from zopt_amd import _lib
from zopt_amd.models import ZM_MODEL_LINEAR, ZM_MODEL_QUADCOPTER_RB, zm_model_t

OK, EINVAL, EUNSUPPORTED = _lib.ZM_OK, _lib.ZM_EINVAL, _lib.ZM_EUNSUPPORTED
D = 0x1000          # a pointer that is never followed
BIG = 1 << 40       # a batch whose launch grids pass 2^31 - 1 blocks

# the parameters of every entry in ABI order, "name=value" of a valid call: batch 4, N = 3, shape (2, 1)
_SOLVER = "n_levels=7 level0=3 rho_step=5.0 alpha=1.6 x_lb=D x_ub=D u_lb=D u_ub=D x0=D"
_TAIL = "eps_abs=1e-5 eps_rel=1e-5 eps_prim_inf=1e-4 max_iter=100 warm_start=0"
_OUT = "workspace=D xTraj=D uTraj=D status=D iters=D resid=D batch=4 N=3 n=2 m=1 stream=None"
_RUN = "steps=2 clip_tol=1e-6 disturbance=None workspace=D states=D inputs=D status=D iters=D"
ENTRIES = {
    "zm_mpc_solve_relaxed_f64": f"A=D B=D K=D Minv=D {_SOLVER} rho=0.1 {_TAIL} {_OUT}",
    "zm_mpc_solve_batched_f64": f"A=D B=D K=D Minv=D {_SOLVER} rho_p=D problem=D P=2 {_TAIL} {_OUT}",
    "zm_mpc_solve_tracking_f64": f"A=D B=D Q=D R=D Qf=D K=D Minv=D {_SOLVER} xRef=None uRef=None rho=0.1 rho_p=None problem=None P=0 "
                                 f"{_TAIL} {_OUT}",
    "zm_mpc_solve_ltv_f64": f"A=D B=D c=D ABt=D Q=D R=D Qf=D K=D Minv=D D=D {_SOLVER} xRef=None uRef=None rho_p=D problem=D P=4 {_TAIL} "
                            f"{_OUT}",
    "zm_mpc_closed_loop_f64": f"A=D B=D Q=D R=D Qf=D K=D Minv=D {_SOLVER} xRef=None uRef=None xref_rows=5 uref_rows=4 rho=0.1 rho_p=None "
                              f"problem=None P=0 {_TAIL} {_RUN} xPred=None uPred=None batch=4 N=3 n=2 m=1 stream=None",
    "zm_mpc_rti_f64": f"model=LIN plant=None xPlan=D uPlan=D A=D B=D c=D Q=D R=D Qf=D rho_tab=D K=D Minv=D D=D ABt=D {_SOLVER} xRef=None "
                      f"uRef=None xref_rows=5 uref_rows=4 rho_p=D problem=D {_TAIL} {_RUN} resid=None xPred=None uPred=None batch=4 N=3 "
                      "n_user=2 m_user=1 ns=2 mc=1 stream=None",
    "zm_mpc_relinearize_f64": "model=LIN xPlan=D uPlan=D A=D B=D c=D batch=4 N=3 n_user=2 m_user=1 ns=2 mc=1 stream=None",
}

# host model blocks (kept alive here: the rows hold their addresses)
_MODELS = {
    "LIN": zm_model_t(ZM_MODEL_LINEAR, 2, 1, 0, 0.0, D, D, (ctypes.c_double * 3)(0, 0, 0)),
    "LIN_NO_AB": zm_model_t(ZM_MODEL_LINEAR, 2, 1, 0, 0.0, None, None, (ctypes.c_double * 3)(0, 0, 0)),
    "LIN_41": zm_model_t(ZM_MODEL_LINEAR, 4, 1, 0, 0.0, D, D, (ctypes.c_double * 3)(0, 0, 0)),
    "LIN_13": zm_model_t(ZM_MODEL_LINEAR, 13, 1, 0, 0.0, D, D, (ctypes.c_double * 3)(0, 0, 0)),
    "KIND9": zm_model_t(9, 2, 1, 0, 0.0, D, D, (ctypes.c_double * 3)(0, 0, 0)),
    "RB_NO_DT": zm_model_t(ZM_MODEL_QUADCOPTER_RB, 8, 4, 0, 0.0, None, None, (ctypes.c_double * 3)(0, 0, 0)),
}
_NAMES = {"D": D, "None": None, **{k: ctypes.addressof(v) for k, v in _MODELS.items()}}
RB = dict(n_user=8, m_user=4, ns=8, mc=4)   # the rigid-body quadcopter's sizes


def _args(entry, over):
    vals = {}
    for item in ENTRIES[entry].split():
        k, v = item.split("=")
        vals[k] = _NAMES[v] if v in _NAMES else (float(v) if ("." in v or "e" in v) else int(v))
    assert set(over) <= set(vals), f"{entry} has no parameter {set(over) - set(vals)}"
    vals.update({k: _NAMES.get(v, v) if isinstance(v, str) else v for k, v in over.items()})
    return list(vals.values())


def _nulls(entry, names):
    return [(entry, {k: None}, EINVAL, f"{entry}: null pointer") for k in names.split()]


RLX, BAT, TRK, LTV, CL, RTI, REL = ENTRIES
ROWS = [
    # ---- zm_mpc_solve_relaxed_f64 ----------------------------------------------------------------------------------------------
    (RLX, dict(batch=0, A=None, x0=None, alpha=9.0), OK, None),
    (RLX, dict(alpha=0.0), EINVAL, "zm_mpc_solve_relaxed_f64: alpha must lie in (0, 2)"),
    (RLX, dict(alpha=2.0), EINVAL, "zm_mpc_solve_relaxed_f64: alpha must lie in (0, 2)"),
    (RLX, dict(alpha=float("nan")), EINVAL, "zm_mpc_solve_relaxed_f64: alpha must lie in (0, 2)"),
    *_nulls(RLX, "A B K Minv x_lb x_ub u_lb u_ub x0 workspace xTraj uTraj status"),
    (RLX, dict(batch=-1), EINVAL, "zm_mpc_solve_relaxed_f64: bad size"),
    (RLX, dict(N=0), EINVAL, "zm_mpc_solve_relaxed_f64: bad size"),
    (RLX, dict(max_iter=-1), EINVAL, "zm_mpc_solve_relaxed_f64: bad size"),
    (RLX, dict(rho=0.0), EINVAL, "zm_mpc_solve_relaxed_f64: bad size"),
    (RLX, dict(n_levels=0), EINVAL, "zm_mpc_solve_relaxed_f64: bad penalty levels"),
    (RLX, dict(level0=-1), EINVAL, "zm_mpc_solve_relaxed_f64: bad penalty levels"),
    (RLX, dict(level0=7), EINVAL, "zm_mpc_solve_relaxed_f64: bad penalty levels"),
    (RLX, dict(rho_step=1.0), EINVAL, "zm_mpc_solve_relaxed_f64: bad penalty levels"),
    (RLX, dict(n=3, m=3), EUNSUPPORTED, "zm_mpc_solve_relaxed_f64: (n=3, m=3) not among the compiled shapes"),
    # two at once
    (RLX, dict(alpha=2.5, A=None), EINVAL, "zm_mpc_solve_relaxed_f64: alpha must lie in (0, 2)"),
    (RLX, dict(x0=None, N=0), EINVAL, "zm_mpc_solve_relaxed_f64: null pointer"),
    (RLX, dict(rho=-1.0, n_levels=0), EINVAL, "zm_mpc_solve_relaxed_f64: bad size"),
    (RLX, dict(level0=9, n=3, m=3), EINVAL, "zm_mpc_solve_relaxed_f64: bad penalty levels"),
    # ---- zm_mpc_solve_batched_f64 ----------------------------------------------------------------------------------------------
    (BAT, dict(batch=0, A=None, problem=None, alpha=9.0), OK, None),
    (BAT, dict(alpha=-0.5), EINVAL, "zm_mpc_solve_batched_f64: alpha must lie in (0, 2)"),
    *_nulls(BAT, "A B K Minv x_lb x_ub u_lb u_ub x0 rho_p problem workspace xTraj uTraj status"),
    (BAT, dict(batch=-1), EINVAL, "zm_mpc_solve_batched_f64: bad size"),
    (BAT, dict(N=0), EINVAL, "zm_mpc_solve_batched_f64: bad size"),
    (BAT, dict(max_iter=-1), EINVAL, "zm_mpc_solve_batched_f64: bad size"),
    (BAT, dict(P=0), EINVAL, "zm_mpc_solve_batched_f64: bad size"),
    (BAT, dict(n_levels=2, level0=2), EINVAL, "zm_mpc_solve_batched_f64: bad penalty levels"),
    (BAT, dict(rho_step=0.5), EINVAL, "zm_mpc_solve_batched_f64: bad penalty levels"),
    # two at once
    (BAT, dict(alpha=2.0, rho_p=None), EINVAL, "zm_mpc_solve_batched_f64: alpha must lie in (0, 2)"),
    (BAT, dict(problem=None, P=0), EINVAL, "zm_mpc_solve_batched_f64: null pointer"),
    (BAT, dict(P=-3, n_levels=0), EINVAL, "zm_mpc_solve_batched_f64: bad size"),
    # ---- zm_mpc_solve_tracking_f64 ---------------------------------------------------------------------------------------------
    (TRK, dict(batch=0, A=None, Q=None, alpha=9.0), OK, None),
    (TRK, dict(alpha=2.0), EINVAL, "zm_mpc_solve_tracking_f64: alpha must lie in (0, 2)"),
    *_nulls(TRK, "A B Q R Qf K Minv x_lb x_ub u_lb u_ub x0 workspace xTraj uTraj status"),
    (TRK, dict(problem=D), EINVAL, "zm_mpc_solve_tracking_f64: the problem map and the per-problem rho come together"),
    (TRK, dict(rho_p=D), EINVAL, "zm_mpc_solve_tracking_f64: the problem map and the per-problem rho come together"),
    (TRK, dict(batch=-1), EINVAL, "zm_mpc_solve_tracking_f64: bad size / rho"),
    (TRK, dict(N=0), EINVAL, "zm_mpc_solve_tracking_f64: bad size / rho"),
    (TRK, dict(max_iter=-1), EINVAL, "zm_mpc_solve_tracking_f64: bad size / rho"),
    (TRK, dict(n=0), EINVAL, "zm_mpc_solve_tracking_f64: bad size / rho"),
    (TRK, dict(m=0), EINVAL, "zm_mpc_solve_tracking_f64: bad size / rho"),
    (TRK, dict(rho=0.0), EINVAL, "zm_mpc_solve_tracking_f64: bad size / rho"),
    (TRK, dict(rho_p=D, problem=D, P=0), EINVAL, "zm_mpc_solve_tracking_f64: bad size / rho"),
    (TRK, dict(n_levels=0), EINVAL, "zm_mpc_solve_tracking_f64: bad penalty levels"),
    (TRK, dict(batch=BIG), EINVAL, "zm_mpc_solve_tracking_f64: batch x N x (n + m) too large"),
    # two at once
    (TRK, dict(alpha=0.0, Qf=None), EINVAL, "zm_mpc_solve_tracking_f64: alpha must lie in (0, 2)"),
    (TRK, dict(R=None, problem=D), EINVAL, "zm_mpc_solve_tracking_f64: null pointer"),
    (TRK, dict(problem=D, rho=0.0), EINVAL, "zm_mpc_solve_tracking_f64: the problem map and the per-problem rho come together"),
    (TRK, dict(n=0, rho_step=1.0), EINVAL, "zm_mpc_solve_tracking_f64: bad size / rho"),
    (TRK, dict(level0=7, batch=BIG), EINVAL, "zm_mpc_solve_tracking_f64: bad penalty levels"),
    (TRK, dict(batch=BIG, n=3, m=3), EINVAL, "zm_mpc_solve_tracking_f64: batch x N x (n + m) too large"),
    # ---- zm_mpc_solve_ltv_f64 --------------------------------------------------------------------------------------------------
    (LTV, dict(batch=0, A=None, c=None, alpha=9.0), OK, None),
    (LTV, dict(alpha=2.0), EINVAL, "zm_mpc_solve_ltv_f64: alpha must lie in (0, 2)"),
    *_nulls(LTV, "A B c ABt Q R Qf K Minv D x_lb x_ub u_lb u_ub x0 rho_p problem workspace xTraj uTraj status"),
    (LTV, dict(batch=-1), EINVAL, "zm_mpc_solve_ltv_f64: bad size / rho"),
    (LTV, dict(N=0), EINVAL, "zm_mpc_solve_ltv_f64: bad size / rho"),
    (LTV, dict(max_iter=-1), EINVAL, "zm_mpc_solve_ltv_f64: bad size / rho"),
    (LTV, dict(n=0), EINVAL, "zm_mpc_solve_ltv_f64: bad size / rho"),
    (LTV, dict(m=0), EINVAL, "zm_mpc_solve_ltv_f64: bad size / rho"),
    (LTV, dict(P=0), EINVAL, "zm_mpc_solve_ltv_f64: bad size / rho"),
    (LTV, dict(n_levels=3, level0=3), EINVAL, "zm_mpc_solve_ltv_f64: bad penalty levels"),
    (LTV, dict(batch=BIG), EINVAL, "zm_mpc_solve_ltv_f64: batch x N x (n + m) too large"),
    (LTV, dict(n=24, m=8), EUNSUPPORTED, "zm_mpc_solve_ltv_f64: (n=24, m=8) not among the shapes of the 16-lanes-per-instance kernels"),
    (LTV, dict(n=3, m=1), EUNSUPPORTED, "zm_mpc_solve_ltv_f64: (n=3, m=1) not among the shapes of the 16-lanes-per-instance kernels"),
    (LTV, dict(N=76), EUNSUPPORTED, "zm_mpc_solve_ltv_f64: N=76 beyond the horizons whose iterates fit LDS (N <= 75)"),
    # two at once
    (LTV, dict(alpha=0.0, D=None), EINVAL, "zm_mpc_solve_ltv_f64: alpha must lie in (0, 2)"),
    (LTV, dict(ABt=None, P=0), EINVAL, "zm_mpc_solve_ltv_f64: null pointer"),
    (LTV, dict(P=0, n_levels=0), EINVAL, "zm_mpc_solve_ltv_f64: bad size / rho"),
    (LTV, dict(rho_step=1.0, n=24, m=8), EINVAL, "zm_mpc_solve_ltv_f64: bad penalty levels"),
    (LTV, dict(batch=BIG, N=76), EINVAL, "zm_mpc_solve_ltv_f64: batch x N x (n + m) too large"),
    (LTV, dict(n=24, m=8, N=76), EUNSUPPORTED, "zm_mpc_solve_ltv_f64: (n=24, m=8) not among the shapes of the 16-lanes-per-instance kernels"),
    # ---- zm_mpc_closed_loop_f64 ------------------------------------------------------------------------------------------------
    (CL, dict(batch=0, A=None, states=None, alpha=9.0, steps=0), OK, None),
    (CL, dict(alpha=2.0), EINVAL, "zm_mpc_closed_loop_f64: alpha must lie in (0, 2)"),
    *_nulls(CL, "A B K Minv x_lb x_ub u_lb u_ub x0 workspace states inputs status iters"),
    (CL, dict(xRef=D, Q=None), EINVAL, "zm_mpc_closed_loop_f64: null pointer"),
    (CL, dict(uRef=D, R=None), EINVAL, "zm_mpc_closed_loop_f64: null pointer"),
    (CL, dict(uRef=D, Qf=None), EINVAL, "zm_mpc_closed_loop_f64: null pointer"),
    (CL, dict(problem=D), EINVAL, "zm_mpc_closed_loop_f64: the problem map and the per-problem rho come together"),
    (CL, dict(rho_p=D), EINVAL, "zm_mpc_closed_loop_f64: the problem map and the per-problem rho come together"),
    (CL, dict(batch=-1), EINVAL, "zm_mpc_closed_loop_f64: bad size"),
    (CL, dict(N=0), EINVAL, "zm_mpc_closed_loop_f64: bad size"),
    (CL, dict(max_iter=-1), EINVAL, "zm_mpc_closed_loop_f64: bad size"),
    (CL, dict(rho=0.0), EINVAL, "zm_mpc_closed_loop_f64: bad size"),
    (CL, dict(rho_p=D, problem=D, P=0), EINVAL, "zm_mpc_closed_loop_f64: bad size"),
    (CL, dict(xRef=D, n=0), EINVAL, "zm_mpc_closed_loop_f64: bad size / rho"),
    (CL, dict(xRef=D, rho=0.0), EINVAL, "zm_mpc_closed_loop_f64: bad size / rho"),
    (CL, dict(n_levels=0), EINVAL, "zm_mpc_closed_loop_f64: bad penalty levels"),
    (CL, dict(xRef=D, batch=BIG), EINVAL, "zm_mpc_closed_loop_f64: batch x N x (n + m) too large"),
    (CL, dict(steps=0), EINVAL, "zm_mpc_closed_loop_f64: steps must be at least 1"),
    (CL, dict(n=0), EINVAL, "zm_mpc_closed_loop_f64: bad size"),
    (CL, dict(m=0), EINVAL, "zm_mpc_closed_loop_f64: bad size"),
    (CL, dict(xPred=D), EINVAL, "zm_mpc_closed_loop_f64: the two prediction arrays come together"),
    (CL, dict(uPred=D), EINVAL, "zm_mpc_closed_loop_f64: the two prediction arrays come together"),
    (CL, dict(xRef=D, xref_rows=4), EINVAL,
     "zm_mpc_closed_loop_f64: a reference needs steps + N rows of xRef and steps + N - 1 rows of uRef"),
    (CL, dict(uRef=D, uref_rows=5), EINVAL,
     "zm_mpc_closed_loop_f64: a reference needs steps + N rows of xRef and steps + N - 1 rows of uRef"),
    (CL, dict(batch=BIG), EINVAL, "zm_mpc_closed_loop_f64: batch x (n + m) too large"),
    # two at once
    (CL, dict(alpha=0.0, inputs=None), EINVAL, "zm_mpc_closed_loop_f64: alpha must lie in (0, 2)"),
    (CL, dict(iters=None, steps=0), EINVAL, "zm_mpc_closed_loop_f64: null pointer"),
    (CL, dict(n_levels=0, steps=0), EINVAL, "zm_mpc_closed_loop_f64: bad penalty levels"),
    (CL, dict(steps=0, m=0), EINVAL, "zm_mpc_closed_loop_f64: steps must be at least 1"),
    (CL, dict(n=0, xPred=D), EINVAL, "zm_mpc_closed_loop_f64: bad size"),
    (CL, dict(uPred=D, xRef=D, xref_rows=9), EINVAL, "zm_mpc_closed_loop_f64: the two prediction arrays come together"),
    (CL, dict(xPred=D, batch=BIG), EINVAL, "zm_mpc_closed_loop_f64: the two prediction arrays come together"),
    (CL, dict(xRef=D, batch=BIG, steps=0), EINVAL, "zm_mpc_closed_loop_f64: batch x N x (n + m) too large"),
    # ---- zm_mpc_rti_f64 --------------------------------------------------------------------------------------------------------
    (RTI, dict(batch=0, A=None, model=None, alpha=9.0, steps=0), OK, None),
    (RTI, dict(alpha=2.0), EINVAL, "zm_mpc_rti_f64: alpha must lie in (0, 2)"),
    *_nulls(RTI, "xPlan uPlan A B c Q R Qf rho_tab K Minv D ABt x_lb x_ub u_lb u_ub x0 rho_p problem workspace states inputs status iters"),
    (RTI, dict(batch=-1), EINVAL, "zm_mpc_rti_f64: bad size / rho"),
    (RTI, dict(N=0), EINVAL, "zm_mpc_rti_f64: bad size / rho"),
    (RTI, dict(max_iter=-1), EINVAL, "zm_mpc_rti_f64: bad size / rho"),
    (RTI, dict(ns=0), EINVAL, "zm_mpc_rti_f64: bad size / rho"),
    (RTI, dict(mc=0), EINVAL, "zm_mpc_rti_f64: bad size / rho"),
    (RTI, dict(n_levels=0), EINVAL, "zm_mpc_rti_f64: bad penalty levels"),
    (RTI, dict(batch=BIG), EINVAL, "zm_mpc_rti_f64: batch x N x (n + m) too large"),
    (RTI, dict(steps=0), EINVAL, "zm_mpc_rti_f64: steps must be at least 1"),
    (RTI, dict(n_user=0), EINVAL, "zm_mpc_rti_f64: bad size"),
    (RTI, dict(m_user=0), EINVAL, "zm_mpc_rti_f64: bad size"),
    (RTI, dict(n_user=3), EINVAL, "zm_mpc_rti_f64: bad size"),
    (RTI, dict(m_user=2), EINVAL, "zm_mpc_rti_f64: bad size"),
    (RTI, dict(xPred=D), EINVAL, "zm_mpc_rti_f64: the two prediction arrays come together"),
    (RTI, dict(uPred=D), EINVAL, "zm_mpc_rti_f64: the two prediction arrays come together"),
    (RTI, dict(xRef=D, xref_rows=4), EINVAL, "zm_mpc_rti_f64: a reference needs steps + N rows of xRef and steps + N - 1 rows of uRef"),
    (RTI, dict(uRef=D, uref_rows=5), EINVAL, "zm_mpc_rti_f64: a reference needs steps + N rows of xRef and steps + N - 1 rows of uRef"),
    (RTI, dict(ns=24, mc=8), EUNSUPPORTED, "zm_mpc_rti_f64: (n=24, m=8) not among the shapes of the 16-lanes-per-instance kernels"),
    (RTI, dict(ns=3, mc=1), EUNSUPPORTED, "zm_mpc_rti_f64: (n=3, m=1) not among the shapes of the 16-lanes-per-instance kernels"),
    (RTI, dict(N=76, xref_rows=78, uref_rows=77), EUNSUPPORTED,
     "zm_mpc_rti_f64: N=76 beyond the horizons whose iterates fit LDS (N <= 75)"),
    (RTI, dict(model=None), EINVAL, "zm_mpc_rti_f64: null model"),
    (RTI, dict(model="KIND9"), EUNSUPPORTED, "zm_mpc_rti_f64: unknown model kind 9"),
    (RTI, dict(model="LIN_NO_AB"), EINVAL, "zm_mpc_rti_f64: linear model needs A, B"),
    (RTI, dict(model="LIN_13"), EUNSUPPORTED, "zm_mpc_rti_f64: (n=13, m=1) not covered (n<=12, m<=4)"),
    (RTI, dict(model="LIN_41"), EINVAL, "zm_mpc_rti_f64: the model has (n=4, m=1), the problem (n=2, m=1)"),
    (RTI, dict(model="RB_NO_DT", **RB), EINVAL, "zm_mpc_rti_f64: the model needs a step dt > 0"),
    (RTI, dict(plant="KIND9"), EUNSUPPORTED, "zm_mpc_rti_f64: unknown model kind 9"),
    (RTI, dict(plant="LIN_41"), EINVAL, "zm_mpc_rti_f64: the plant has (n=4, m=1), the problem (n=2, m=1)"),
    (RTI, dict(model="LIN_41", plant="RB_NO_DT", ns=8, mc=4, n_user=4, m_user=1), EINVAL,
     "zm_mpc_rti_f64: the plant has (n=8, m=4), the problem (n=4, m=1)"),
    # (2^37 instances at N = 1: the grid of the tracking term still fits, that of the plan shift does not)
    (RTI, dict(batch=1 << 37, N=1, xref_rows=3, uref_rows=2), EINVAL, "zm_mpc_rti_f64: batch x N x (n + m) too large"),
    # two at once
    (RTI, dict(alpha=0.0, xPlan=None), EINVAL, "zm_mpc_rti_f64: alpha must lie in (0, 2)"),
    (RTI, dict(rho_tab=None, steps=0), EINVAL, "zm_mpc_rti_f64: null pointer"),
    (RTI, dict(n_levels=0, steps=0), EINVAL, "zm_mpc_rti_f64: bad penalty levels"),
    (RTI, dict(batch=BIG, steps=0), EINVAL, "zm_mpc_rti_f64: batch x N x (n + m) too large"),
    (RTI, dict(steps=0, n_user=0), EINVAL, "zm_mpc_rti_f64: steps must be at least 1"),
    (RTI, dict(n_user=3, uPred=D), EINVAL, "zm_mpc_rti_f64: bad size"),
    (RTI, dict(xPred=D, uRef=D, uref_rows=0), EINVAL, "zm_mpc_rti_f64: the two prediction arrays come together"),
    (RTI, dict(xRef=D, xref_rows=0, ns=3, mc=1), EINVAL,
     "zm_mpc_rti_f64: a reference needs steps + N rows of xRef and steps + N - 1 rows of uRef"),
    (RTI, dict(ns=24, mc=8, N=76, xref_rows=78, uref_rows=77), EUNSUPPORTED,
     "zm_mpc_rti_f64: (n=24, m=8) not among the shapes of the 16-lanes-per-instance kernels"),
    (RTI, dict(N=76, xref_rows=78, uref_rows=77, model=None), EUNSUPPORTED,
     "zm_mpc_rti_f64: N=76 beyond the horizons whose iterates fit LDS (N <= 75)"),
    (RTI, dict(model="LIN_41", plant="KIND9"), EINVAL, "zm_mpc_rti_f64: the model has (n=4, m=1), the problem (n=2, m=1)"),
    (RTI, dict(plant="LIN_41", batch=1 << 37, N=1, xref_rows=3, uref_rows=2), EINVAL,
     "zm_mpc_rti_f64: the plant has (n=4, m=1), the problem (n=2, m=1)"),
    # ---- zm_mpc_relinearize_f64 ------------------------------------------------------------------------------------------------
    (REL, dict(batch=0, A=None, model=None), OK, None),
    *_nulls(REL, "xPlan uPlan A B c"),
    (REL, dict(batch=-1), EINVAL, "zm_mpc_relinearize_f64: bad size"),
    (REL, dict(N=0), EINVAL, "zm_mpc_relinearize_f64: bad size"),
    (REL, dict(n_user=0), EINVAL, "zm_mpc_relinearize_f64: bad size"),
    (REL, dict(m_user=0), EINVAL, "zm_mpc_relinearize_f64: bad size"),
    (REL, dict(ns=1), EINVAL, "zm_mpc_relinearize_f64: bad size"),
    (REL, dict(mc=0), EINVAL, "zm_mpc_relinearize_f64: bad size"),
    (REL, dict(ns=13), EUNSUPPORTED, "zm_mpc_relinearize_f64: (n=13, m=1) not covered (n <= 12, m <= 4)"),
    (REL, dict(mc=5), EUNSUPPORTED, "zm_mpc_relinearize_f64: (n=2, m=5) not covered (n <= 12, m <= 4)"),
    (REL, dict(batch=BIG), EINVAL, "zm_mpc_relinearize_f64: batch x N too large"),
    (REL, dict(model=None), EINVAL, "zm_mpc_relinearize_f64: null model"),
    (REL, dict(model="KIND9"), EUNSUPPORTED, "zm_mpc_relinearize_f64: unknown model kind 9"),
    (REL, dict(model="LIN_NO_AB"), EINVAL, "zm_mpc_relinearize_f64: linear model needs A, B"),
    (REL, dict(model="LIN_13"), EUNSUPPORTED, "zm_mpc_relinearize_f64: (n=13, m=1) not covered (n<=12, m<=4)"),
    (REL, dict(model="LIN_41"), EINVAL, "zm_mpc_relinearize_f64: the model has (n=4, m=1), the problem (n=2, m=1)"),
    (REL, dict(model="RB_NO_DT", **RB), EINVAL, "zm_mpc_relinearize_f64: the model needs a step dt > 0"),
    # two at once
    (REL, dict(c=None, N=0), EINVAL, "zm_mpc_relinearize_f64: null pointer"),
    (REL, dict(n_user=0, ns=13), EINVAL, "zm_mpc_relinearize_f64: bad size"),
    (REL, dict(mc=5, batch=BIG), EUNSUPPORTED, "zm_mpc_relinearize_f64: (n=2, m=5) not covered (n <= 12, m <= 4)"),
    (REL, dict(batch=BIG, model=None), EINVAL, "zm_mpc_relinearize_f64: batch x N too large"),
]


def test_every_entry_has_rows_that_break_two_checks():
    assert {r[0] for r in ROWS} == set(ENTRIES)
    for entry in ENTRIES:
        assert sum(1 for e, over, rc, _ in ROWS if e == entry and rc != OK and len(over) >= 2) >= 2


@pytest.mark.parametrize("row", range(len(ROWS)), ids=lambda i: f"{ROWS[i][0]}-{'-'.join(ROWS[i][1])}-{i}")
def test_refusal(row):
    entry, over, rc, msg = ROWS[row]
    lib = _lib.lib()
    assert getattr(lib, entry)(*_args(entry, over)) == rc
    if msg is not None:
        assert lib.zm_last_error().decode() == msg
