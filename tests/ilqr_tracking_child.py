"""Child process of tests/test_ilqr_tracking_gpu.py: a fixed set of tracking-cost solves, saved to the .npz named on the command line.

The kernel forms a solve goes through are chosen by switches that the library reads once per process (the -DZM_LAB build:
ZOPT_AMD_ILQR_TAIL=0 keeps the line search in its two-pass form where the default takes the all-store form, ZOPT_AMD_EXPAND=group
runs the 16-lane expansion where the default runs the one-lane one), so each form gets a process of its own and the parent compares
the files bit for bit.

    python tests/ilqr_tracking_child.py OUT.npz
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def cases():
    """name -> (model factory, cost factory, x0, uGuess, ddp): small (12, 4) problems, full and diagonal weights, every reference layout"""
    from zopt_amd import models
    rng = np.random.default_rng(77)
    out = {}
    B, T = 5, 7
    x0 = np.zeros((B, 12))
    x0[:, 9:12] = rng.uniform(-3, 3, (B, 3))
    x0[:, 6:8] = 0.1 * rng.standard_normal((B, 2))
    ug = np.tile(models.QuadcopterEuler.uTrim, (B, T, 1))
    goal = np.zeros((B, 12))
    goal[:, 9:12] = rng.uniform(-2, 2, (B, 3))
    ramp = np.linspace(0, 1, T + 1)[None, :, None] * goal[:, None, :]
    full = np.eye(12) + 0.05 * rng.standard_normal((12, 12))
    quad = lambda: models.QuadcopterEuler(0.1)
    out["quad_diag_goal"] = (quad, lambda: models.TrackingCost(np.eye(12), 0.5 * np.eye(4), 10 * np.eye(12), goal[:, None, :],
                                                               models.QuadcopterEuler.uTrim), x0, ug, 0)
    out["quad_diag_ramp_ddp"] = (quad, lambda: models.TrackingCost(np.eye(12), 0.5 * np.eye(4), 10 * np.eye(12), ramp,
                                                                   np.tile(models.QuadcopterEuler.uTrim, (B, T, 1))), x0, ug, 1)
    out["quad_full_shared"] = (quad, lambda: models.TrackingCost(full, np.eye(4), 10 * np.eye(12), goal[0], None), x0, ug, 0)
    A = np.eye(12) + 0.05 * rng.standard_normal((12, 12))
    Bm = 0.3 * rng.standard_normal((12, 4))
    xl = rng.standard_normal((B, 12))
    out["lin12_full_ramp"] = (lambda: models.LinearModel(A, Bm),
                              lambda: models.TrackingCost(full, np.eye(4) + 0.1, 5 * full, ramp, 0.1 * np.ones(4)), xl,
                              np.zeros((B, T, 4)), 0)
    return out


def run(name, case, maxIter=6):
    from zopt_amd import ilqrUtils
    mk_model, mk_cost, x0, ug, ddp = case
    model, cost = mk_model(), mk_cost()
    solve = ilqrUtils.differentialDynamicProgramming if ddp else ilqrUtils.iterativeLqr
    ilqrUtils._TRACE = []
    try:
        traj, L, J, conv = solve(model, cost, cost, x0, ug, maxIter=maxIter, tol=1e-9)
        rec = dict(ilqrUtils._TRACE)
    finally:
        ilqrUtils._TRACE = None
    return {f"{name}/x": traj.xTraj, f"{name}/u": traj.uTraj, f"{name}/L": L, f"{name}/J": J, f"{name}/conv": conv,
            f"{name}/J_trace": rec["J_trace"], f"{name}/alpha_trace": rec["alpha_trace"]}


def main(path):
    out = {}
    for name, case in cases().items():
        out.update(run(name, case))
    np.savez(path, **out)
    print("TRACKING-CHILD-OK")


if __name__ == "__main__":
    main(sys.argv[1])
