"""One iteration of iterativeLqr / differentialDynamicProgramming from the hard points of tests/model_hp_ref.py, for
tests/test_expand_forms_hard_gpu.py: the solvers' expansion kernels (expand_quad_points_kernel, quad_hessian_points_kernel, the packed
instantiations of linearize_dynamics_kernel, quad_hessian_pairs16_kernel) have no entry point of their own -- a solve is how they run.

    python tests/expand_forms_child.py OUT.npz

The forms are chosen by the lab switches ZOPT_AMD_EXPAND (points | group), ZOPT_AMD_JAC (packed | full) and ZOPT_AMD_HES (sparse |
dense), read once per process from the lab build of the library (ZOPT_AMD_LIB): one child process per combination.

Problems (`problems()`): per case (family, with / without wind) the 88 points of the family as initial states of horizon-2 solves in
batches of 1, 3, 17 and 67 -- with N = 2 the first gain L_0 = Q_uu^-1 f_u^T V_1 f_x reads every row of the expansion at x_0 and,
through V_1, every row of the first (and, for DDP, second) derivatives at x_1 --, and one batch of 3 with N = 40: more than the 32
points of a chunk of the one-lane kernels, so chunks and tails run.  maxIter = 1: the gains of the first backward pass come back.
Also saved: the initial rollout, by the very call the solver makes, so that the parent knows the expansion points."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DT = 0.1
Q, R, QF = np.eye(12), np.eye(4), 10.0 * np.eye(12)
SHAPES = [(1, 2), (3, 2), (17, 2), (67, 2)]
LONG = (3, 40)


def problems():
    """(key, wind, x0 (b, 12), uGuess (b, N, 4)) of every solve"""
    from tests import model_hp_ref as hp
    for fam, windy in hp.CASES:
        w = hp.WINDS[fam] if windy else (0.0, 0.0, 0.0)
        x, u = hp.family(fam, hp.NPOINTS)
        rng = np.random.default_rng([5, hp.FAMILIES.index(fam)])
        off = 0
        for b, N in SHAPES + [LONG]:
            sl = slice(off, off + b) if (b, N) != LONG else slice(0, b)
            off += b if (b, N) != LONG else 0
            ug = hp.U_TRIM + 0.1 * rng.standard_normal((b, N, 4))
            ug[:, 0] = u[sl]
            yield f"{hp.case_id((fam, windy))}_{b}x{N}", w, x[sl].copy(), ug


def initial_rollout(model, cost, x0, ug):
    """zm_rollout_linesearch_f64 as zm_ilqr_solve_f64 calls it: policy (uGuess, 0) about the zero trajectory, one step size 1"""
    import torch
    from zopt_amd import _lib
    b, N = ug.shape[:2]
    md, cs = model.c_struct(), cost.c_struct()
    dev = [torch.as_tensor(np.ascontiguousarray(X), device="cuda") for X in
           (x0, ug, np.zeros((b, N, 4, 12)), np.zeros((b, N + 1, 12)), np.zeros((b, N, 4)))]
    al = torch.ones(1, dtype=torch.float64, device="cuda")
    xT = torch.empty((b, N + 1, 12), dtype=torch.float64, device="cuda")
    uT = torch.empty((b, N, 4), dtype=torch.float64, device="cuda")
    J = torch.empty((b,), dtype=torch.float64, device="cuda")
    _lib.check(_lib.lib().zm_rollout_linesearch_f64(ctypes.addressof(md), ctypes.addressof(cs), *[t.data_ptr() for t in dev], al.data_ptr(),
                                                    1, None, xT.data_ptr(), uT.data_ptr(), J.data_ptr(), None, b, N, None), "rollout")
    torch.cuda.synchronize()
    return xT.cpu().numpy(), uT.cpu().numpy()


def main():
    from zopt_amd import ilqrUtils, models
    cost = models.QuadraticCost(Q, R, QF)
    out = {}
    for key, w, x0, ug in problems():
        model = models.QuadcopterEuler(DT, wind_ned=w)
        out[key + "_xinit"], out[key + "_uinit"] = initial_rollout(model, cost, x0, ug)
        for name, solve in (("ilqr", ilqrUtils.iterativeLqr), ("ddp", ilqrUtils.differentialDynamicProgramming)):
            traj, L, J, conv = solve(model, cost, cost, x0, ug, maxIter=1)
            out[f"{key}_{name}_x"], out[f"{key}_{name}_u"] = np.asarray(traj.xTraj), np.asarray(traj.uTraj)
            out[f"{key}_{name}_L"], out[f"{key}_{name}_J"] = np.asarray(L), np.asarray(J)
    np.savez(sys.argv[1], **out)
    print("CHILD-OK", len(out))


if __name__ == "__main__":
    main()
