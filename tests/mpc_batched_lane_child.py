"""Child process of tests/test_mpc_batched_gpu.py: with whatever ZOPT_AMD_MPC_PATH the parent put into the environment (read once per
process), one batched lqrMpc solve over a family of problems must equal the loop of single-problem solves bit for bit.  Prints
"MPC-BATCHED-OK" and exits 0 when it does."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from tests.test_mpc_batched import _family
    from zopt_amd import mpcUtils
    for (n, m, N) in ((12, 4, 30), (3, 2, 12)):
        A, B, Q, R, xl, xu, ul, uu = _family((9,), n, m, seed=n + m)
        x0 = 0.5 * xu * np.random.default_rng(n).uniform(-1, 1, (9, n))
        prob = mpcUtils.lqrMpc(A, B, Q, R, N, xl, xu, ul, uu)
        kw = dict(eps_abs=1e-5, eps_rel=1e-5, max_iter=3000)
        u, traj, status = prob.solve(x0, **kw)
        for i in range(9):
            one = mpcUtils.lqrMpc(A[i], B[i], Q[i], R[i], N, xl[i], xu[i], ul[i], uu[i])
            u1, t1, s1 = one.solve(x0[i], **kw)
            assert np.array_equal(traj.xTraj[i], t1.xTraj) and np.array_equal(traj.uTraj[i], t1.uTraj), (n, m, i)
            assert status[i] == s1 and prob.last_iterations[i] == one.last_iterations, (n, m, i)
            assert np.array_equal(prob.last_residuals[i], one.last_residuals), (n, m, i)
    print("MPC-BATCHED-OK")


if __name__ == "__main__":
    main()
