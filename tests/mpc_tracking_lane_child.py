"""Child process of tests/test_mpc_tracking_gpu.py: with whatever ZOPT_AMD_MPC_PATH the parent put into the environment (read once per
process), (a) one per-problem tracking solve over a family of problems must equal the loop of single-problem tracking solves bit for bit,
(b) the shared-problem tracking solve of `shared_case` is written to the .npz file named on the command line, for the parent to compare
with the other dispatch path.  Prints "MPC-TRACKING-LANE-OK" and exits 0."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def shared_case():
    from tests import mpc_tracking_ref as tr
    N = 12
    data, x0, xRef, uRef = tr.random_case(4, 2, N, seed=42, nb=6)
    return data, x0, xRef, uRef, N


def main():
    from tests.test_mpc_batched import _family
    from zopt_amd import mpcUtils
    for (n, m, N) in ((12, 4, 30), (3, 2, 12)):
        A, B, Q, R, xl, xu, ul, uu = _family((9,), n, m, seed=n + m)
        rng = np.random.default_rng(n)
        x0 = 0.5 * xu * rng.uniform(-1, 1, (9, n))
        t = np.arange(N + 1)
        xRef = 1.5 * xu[:, None, :] * np.sin(2 * np.pi * t[None, :, None] / N + rng.uniform(0, 6, (9, 1, n)))    # leaves each box
        uRef = 0.5 * uu[:, None, :] * np.ones((1, N, 1))
        prob = mpcUtils.lqrMpc(A, B, Q, R, N, xl, xu, ul, uu)
        kw = dict(eps_abs=1e-5, eps_rel=1e-5, max_iter=3000)
        u, traj, status = prob.solve(x0, xRef=xRef, uRef=uRef, **kw)
        for i in range(9):
            one = mpcUtils.lqrMpc(A[i], B[i], Q[i], R[i], N, xl[i], xu[i], ul[i], uu[i])
            u1, t1, s1 = one.solve(x0[i], xRef=xRef[i], uRef=uRef[i], **kw)
            assert np.array_equal(traj.xTraj[i], t1.xTraj) and np.array_equal(traj.uTraj[i], t1.uTraj), (n, m, i)
            assert status[i] == s1 and prob.last_iterations[i] == one.last_iterations, (n, m, i)
            assert np.array_equal(prob.last_residuals[i], one.last_residuals), (n, m, i)
        # the reference is felt: not the regulator's answer
        assert np.max(np.abs(traj.uTraj - prob.solve(x0, warm_start=False, **kw)[1].uTraj)) > 1e-3
    data, x0, xRef, uRef, N = shared_case()
    prob = mpcUtils.lqrMpc(*data[:4], N, *data[5:], Qf=data[4])
    u, traj, status = prob.solve(x0, xRef=xRef, uRef=uRef, warm_start=False)
    np.savez(sys.argv[1], xTraj=traj.xTraj, uTraj=traj.uTraj, status=status.astype(str), iters=prob.last_iterations)
    print("MPC-TRACKING-LANE-OK")


if __name__ == "__main__":
    main()
