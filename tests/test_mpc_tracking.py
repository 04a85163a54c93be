"""CPU test of the tracking checkers (tests/mpc_tracking_ref.py): the NumPy restatement of the tracking ADMM -- what the GPU tests hold the
kernels to iterate by iterate -- against the independent SciPy solve of the condensed tracking QP, on references that leave the box."""
import numpy as np
import pytest

from tests import mpc_tracking_ref as tr

# Bound on |u_admm - u_scipy|: a residual test at eps bounds the distance to the optimum only up to the ADMM's convergence rate (a
# fixed-penalty run on the quadcopter contracts slowly: ~2e4 iterations at eps = 1e-7), so no bound follows from eps alone; this is the
# bound the suite already holds the kernels to against the same SciPy solve at the same eps = 1e-7 (tests/test_mpc_gpu.py:
# test_shapes_between_the_compiled_kernels).  Measured: 2.8e-6, 2.3e-7 on the random cases, 1.03e-5 on the quadcopter (1.03e-7 at eps = 1e-9:
# the distance scales with eps, the restatement converges to the SciPy optimum).
EPS, AGREE = 1e-7, 2e-4


def _cases():
    yield "random (2, 1, 20)", tr.random_case(2, 1, 20, seed=21)
    yield "random (4, 2, 12)", tr.random_case(4, 2, 12, seed=42)
    N = 25
    yield "quadcopter (12, 4, 25)", (tr.quad_data(N),) + tr.quad_reference(N)


@pytest.mark.parametrize("name, case", list(_cases()), ids=[c[0] for c in _cases()])
def test_tracking_admm_against_independent_solve(name, case):
    data, x0, xRef, uRef = case
    A, B, Q, R, Qf, x_lb, x_ub, u_lb, u_ub = data
    N = uRef.shape[1]
    xs, us, fs = tr.solve_reference(*data[:5], N, *data[5:], x0[0], xRef[0], uRef[0])
    act = tr.n_active(xs, us, x_lb, x_ub, u_lb, u_ub)
    assert act >= 1, "the case proves nothing without an active bound"
    x, u, status, it = tr.admm(*data[:5], N, *data[5:], x0[0], xRef[0], uRef[0], rho=tr.default_rho(Q, R), eps_abs=EPS, eps_rel=EPS,
                               max_iter=100000, alpha=1.6)
    err = float(np.max(np.abs(u - us)))
    print(f"{name}: |u - u_scipy| = {err:.2e}, {it} ADMM iterations, {act} active bounds")
    assert status == "optimal"
    assert err <= AGREE
    kkt = tr.kkt_residuals(*data[:5], N, *data[5:], x0[0], x, u, xRef[0], uRef[0], act_tol=1e-5)
    assert kkt["dyn"] <= 1e-12 and kkt["bound"] <= 1e-5 and kkt["stat"] <= 1e-4     # (the bounds of test_mpc_gpu.py at eps = 1e-7)
    # the reference matters: the regulator's optimum is a different point
    x_reg, u_reg, _ = tr.solve_reference(*data[:5], N, *data[5:], x0[0], 0 * xRef[0], 0 * uRef[0])
    assert np.max(np.abs(u_reg - us)) > 1e-2
    assert tr.cost(Q, R, Qf, x, u, xRef[0], uRef[0]) <= fs + 1e-6 * max(1.0, abs(fs))
