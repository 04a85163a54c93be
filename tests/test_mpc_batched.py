"""lqrMpc with per-problem data (leading axes on A, B, Q, R, Qf and the bounds): the host side -- construction, checks, penalty,
embedding -- needs no GPU; neither do the argument checks of the two batched C entry points."""
import numpy as np
import pytest

from zopt_amd import _lib, mpcUtils


def _family(P, n, m, seed=0):
    rng = np.random.default_rng(seed)
    A = np.eye(n) + 0.1 * rng.standard_normal(P + (n, n))
    B = 0.1 * rng.standard_normal(P + (n, m))
    G = rng.standard_normal(P + (n, n))
    Q = G @ np.swapaxes(G, -1, -2) / n + 0.1 * np.eye(n)
    H = rng.standard_normal(P + (m, m))
    R = H @ np.swapaxes(H, -1, -2) / m + 0.5 * np.eye(m)
    x_ub = rng.uniform(0.5, 2.0, P + (n,))
    u_ub = rng.uniform(0.5, 2.0, P + (m,))
    return A, B, Q, R, -x_ub, x_ub, -u_ub, u_ub


@pytest.mark.parametrize("n, m", [(12, 4), (3, 2), (9, 4), (16, 5), (24, 8), (1, 1)])
def test_batched_construction_matches_the_single_problem_constructor(n, m):
    A, B, Q, R, xl, xu, ul, uu = _family((5,), n, m, seed=n * 10 + m)
    prob = mpcUtils.lqrMpc(A, B, Q, R, 7, xl, xu, ul, uu)
    assert prob.P == (5,) and prob.rho.shape == (5,) and prob.rho.dtype == np.float64
    assert (prob._n_user, prob._m_user) == (n, m)
    for i in range(5):
        one = mpcUtils.lqrMpc(A[i], B[i], Q[i], R[i], 7, xl[i], xu[i], ul[i], uu[i])
        assert one.P is None and isinstance(one.rho, float)
        assert prob.rho[i] == one.rho                        # bit for bit
        assert (prob.n, prob.m) == (one.n, one.m)
        for k in ("A", "B", "Q", "R", "Qf", "x_lb", "x_ub", "u_lb", "u_ub"):
            assert np.array_equal(getattr(prob, k)[i], getattr(one, k)), k


def test_problem_shape_broadcasts_over_every_array():
    A, B, Q, R, xl, xu, ul, uu = _family((3, 4), 4, 2, seed=1)
    # A, B batched (3, 4); Q, R shared; state bounds batched over the first axis only; control bounds shared
    prob = mpcUtils.lqrMpc(A, B, Q[0, 0], R[0, 0], 5, xl[:, :1], xu[:, :1], ul[0, 0], uu[0, 0], Qf=2 * Q[0, 0])
    assert prob.P == (3, 4) and prob.rho.shape == (3, 4)
    assert prob.A.shape == (3, 4, 4, 4) and prob.x_lb.shape == (3, 4, 4) and prob.u_ub.shape == (3, 4, 2)
    one = mpcUtils.lqrMpc(A[2, 1], B[2, 1], Q[0, 0], R[0, 0], 5, xl[2, 0], xu[2, 0], ul[0, 0], uu[0, 0], Qf=2 * Q[0, 0])
    assert prob.rho[2, 1] == one.rho and np.all(prob.rho == one.rho)
    assert np.array_equal(prob.Qf[2, 1], one.Qf) and np.array_equal(prob.x_ub[2, 1], one.x_ub)
    # torch tensors (host) are accepted as well
    torch = pytest.importorskip("torch")
    prob_t = mpcUtils.lqrMpc(torch.as_tensor(A), torch.as_tensor(B), Q[0, 0], R[0, 0], 5, xl[:, :1], xu[:, :1], ul[0, 0], uu[0, 0],
                             Qf=2 * Q[0, 0])
    assert np.array_equal(prob_t.rho, prob.rho) and np.array_equal(prob_t.A, prob.A)


def test_unbatched_data_keeps_the_single_problem_path():
    A, B, Q, R, xl, xu, ul, uu = _family((), 12, 4, seed=3)
    prob = mpcUtils.lqrMpc(A, B, Q, R, 5, xl, xu, ul, uu)
    assert prob.P is None and isinstance(prob.rho, float) and prob.A.shape == (12, 12)


def test_leading_shapes_that_do_not_broadcast_are_refused():
    A, B, Q, R, xl, xu, ul, uu = _family((3,), 4, 2, seed=2)
    with pytest.raises(ValueError, match="shapes"):
        mpcUtils.lqrMpc(A, B[:2], Q, R, 5, xl, xu, ul, uu)
    with pytest.raises(ValueError, match="shapes"):
        mpcUtils.lqrMpc(A, B, Q, R, 5, xl, xu, ul[:2], uu)
    with pytest.raises(ValueError, match="shapes"):          # trailing shapes: as for one problem
        mpcUtils.lqrMpc(A, B, Q[..., :3, :3], R, 5, xl, xu, ul, uu)
    with pytest.raises(ValueError, match="shapes"):
        mpcUtils.lqrMpc(A, B, Q, R, 5, xl[..., :3], xu, ul, uu)


def test_one_non_psd_weight_in_a_batch_is_refused_and_named():
    A, B, Q, R, xl, xu, ul, uu = _family((5, 2), 4, 2, seed=4)
    Qbad = Q.copy()
    Qbad[3, 1] = np.diag([1.0, 1.0, -0.5, 1.0])
    with pytest.raises(ValueError, match=r"Q\[3, 1\] is not positive semidefinite"):
        mpcUtils.lqrMpc(A, B, Qbad, R, 5, xl, xu, ul, uu)
    Qf = np.broadcast_to(np.eye(4), (5, 2, 4, 4)).copy()
    Qf[0, 1] = np.array([[0.0, 1.0, 0, 0], [1.0, 0.0, 0, 0], [0, 0, 1.0, 0], [0, 0, 0, 1.0]])
    with pytest.raises(ValueError, match=r"Qf\[0, 1\] is not positive semidefinite"):
        mpcUtils.lqrMpc(A, B, Q, R, 5, xl, xu, ul, uu, Qf=Qf)
    # a shared non-PSD weight is named without an index
    with pytest.raises(ValueError, match=r"R\[0, 0\] is not positive semidefinite"):
        mpcUtils.lqrMpc(A, B, Q, -np.eye(2), 5, xl, xu, ul, uu)


def test_solve_argument_checks_before_any_launch():
    A, B, Q, R, xl, xu, ul, uu = _family((3,), 4, 2, seed=5)
    prob = mpcUtils.lqrMpc(A, B, Q, R, 5, xl, xu, ul, uu)
    with pytest.raises(ValueError, match="shapes"):
        prob.solve(np.zeros((2, 4)))                          # (2,) against P = (3,)
    with pytest.raises(ValueError):
        prob.solve(np.zeros((3, 5)))
    with pytest.raises(ValueError, match="broadcast"):
        prob.solve(np.zeros((3, 4)), rho=np.ones(2))
    with pytest.raises(ValueError, match="positive"):
        prob.solve(np.zeros((3, 4)), rho=np.array([1.0, 0.0, 1.0]))


def test_batched_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _lib.lib()
    null = None
    rc = lib.zm_mpc_setup_batched_f64(null, null, null, null, null, null, 4, 7, 10, 12, 4, null, null, null)
    assert rc == _lib.ZM_EINVAL and b"zm_mpc_setup_batched_f64" in lib.zm_last_error()
    assert lib.zm_mpc_setup_batched_f64(null, null, null, null, null, null, 0, 7, 10, 12, 4, null, null, null) == _lib.ZM_OK
    args = [null] * 4 + [7, 3, 5.0, 1.6] + [null] * 7 + [4, 1e-5, 1e-5, 1e-4, 100, 0] + [null] * 6 + [8, 10, 12, 4, null]
    assert lib.zm_mpc_solve_batched_f64(*args) == _lib.ZM_EINVAL and b"zm_mpc_solve_batched_f64" in lib.zm_last_error()
    args[-5] = 0   # empty batch: nothing to do
    assert lib.zm_mpc_solve_batched_f64(*args) == _lib.ZM_OK
