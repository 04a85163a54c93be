"""Child process of tests/test_mpc_closed_loop_gpu.py: with ZOPT_AMD_MPC_PATH=lane in the environment (read once per process) the shapes of
the 16-lane kernels run the lane-per-instance kernel, and lqrMpc.simulate its host loop of launches.  Runs simulate and the yardstick loop
over `solve` (tests/mpc_closed_loop_cases.py) for (12, 4, 5) and (2, 1, 3) and writes both to the .npz file named on the command line; the
parent compares.  Prints "MPC-CLOSED-LOOP-LANE-OK" when it is through."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(out_file):
    from tests import mpc_closed_loop_cases as cc
    from zopt_amd import mpcUtils
    assert os.environ.get("ZOPT_AMD_MPC_PATH") == "lane"
    out = {}
    for shape in ((12, 4, 5), (2, 1, 3)):
        n, m, N = shape
        prob, prob2, x0, _ = cc.random_pair(mpcUtils, n, m, N, 5)
        w = 0.05 * np.random.default_rng(11).standard_normal((5, 4, n))
        kw = dict(disturbance=w, eps_abs=1e-5, eps_rel=1e-5)
        ref = cc.loop(prob2, x0, 4, **kw)
        got = cc.as_arrays(prob.simulate(x0, 4, return_predictions=True, **kw))
        for tag, r in (("got", got), ("ref", ref)):
            for k in ("xTraj", "uTraj", "iterations", "px", "pu"):
                out[f"{shape}|{tag}|{k}"] = getattr(r, k)
            out[f"{shape}|{tag}|status"] = r.status.astype(str)
    np.savez(out_file, **out)
    print("MPC-CLOSED-LOOP-LANE-OK")


if __name__ == "__main__":
    main(sys.argv[1])
