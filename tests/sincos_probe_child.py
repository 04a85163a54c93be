"""Probes that make zm_sincos (zopt_amd/csrc/trig.h) observable bit for bit through the public calls, for tests/test_sincos_gpu.py.

With state [1,0,0, 0,0,0, 0,0,psi, 0,0,0] every other factor of the position rows of inertialDynamics is exactly 1 or 0 (the sines
and cosines of the zero angles are exactly 0 and 1), so xDot[9], xDot[10] = cos psi, sin psi whatever the order of the sums and
whichever products a compiler fuses; with the angle in theta, xDot[9], xDot[11] = cos theta, -sin theta; with v = 1 instead of
u = 1 and the angle in phi, xDot[10], xDot[11] = cos phi, sin phi.  A step x + dt xDot with dt = 1 from zero position is as exact.

Run as a program (`python tests/sincos_probe_child.py OUT.npz N_ALPHA`) it performs the one-step line-search rollout of the probe
states and saves the states after the step: the rollout's kernel selection is read from the environment once per process
(ZOPT_AMD_ROLLOUT_PATH=generic), so the generic kernel needs a process of its own."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ANGLE_SLOT = {"psi": 8, "theta": 7, "phi": 6}
UNIT_SLOT = {"psi": 0, "theta": 0, "phi": 1}
# (components of xDot, sign) that carry (cos, sin) of the probed angle
READ = {"psi": ((9, 1.0), (10, 1.0)), "theta": ((9, 1.0), (11, -1.0)), "phi": ((10, 1.0), (11, 1.0))}


def states(angle, which):
    """(len(angle), 12) probe states"""
    x = np.zeros((len(angle), 12))
    x[:, UNIT_SLOT[which]] = 1.0
    x[:, ANGLE_SLOT[which]] = angle
    return x


def controls(count, seed=5):
    """any control: the position rows do not read it"""
    rng = np.random.default_rng(seed)
    return np.array([9.807, 0.0, 0.0, 0.0]) + rng.standard_normal((count, 4))


def read(xd, which):
    """(cos, sin) as the probe's output carries them"""
    (ic, sc), (js, ss) = READ[which]
    return sc * xd[:, ic], ss * xd[:, js]


def rollout_step(x0, u, n_alpha):
    """x_1 of the one-step rollout (dt = 1) of zm_rollout_linesearch_f64 WITH a cost (without one the entry takes the generic
    kernel whatever the environment says) and the winning step-size index.
    n_alpha = 1: u_0 = u.  n_alpha = 16: u_0 = u + alpha e_mz with cost alpha^2 (R = Qf = e e^T on mz / r, Q = 0; u's own mz is
    set to 0), so the smallest step size, index 15, wins strictly and the winner is re-rolled (rollout_quad_reroll_kernel on the
    fast path: four lanes per rollout) -- the position rows do not see mz."""
    import torch
    from zopt_amd import _lib, models
    b = len(x0)
    u = np.array(u, dtype=np.float64)
    l = np.zeros((b, 1, 4))
    R, Qf = np.zeros((4, 4)), np.zeros((12, 12))
    if n_alpha == 16:
        u[:, 3] = 0.0
        l[:, 0, 3] = 1.0
        R[3, 3] = Qf[5, 5] = 1.0
    cost = models.QuadraticCost(np.zeros((12, 12)), R, Qf)
    md, cs = models.QuadcopterEuler(1.0).c_struct(), cost.c_struct()
    dev = [torch.as_tensor(np.ascontiguousarray(X), device="cuda") for X in
           (x0, l, np.zeros((b, 1, 4, 12)), np.zeros((b, 2, 12)), u[:, None, :])]
    al = torch.as_tensor(0.5 ** np.arange(n_alpha), device="cuda")
    xT = torch.full((b, 2, 12), -7.0, dtype=torch.float64, device="cuda")
    uT = torch.full((b, 1, 4), -7.0, dtype=torch.float64, device="cuda")
    J = torch.full((b,), -7.0, dtype=torch.float64, device="cuda")
    idx = torch.full((b,), -1, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib().zm_rollout_linesearch_f64(
        ctypes.addressof(md), ctypes.addressof(cs), *[t.data_ptr() for t in dev], al.data_ptr(), n_alpha, None, xT.data_ptr(),
        uT.data_ptr(), J.data_ptr(), idx.data_ptr() if n_alpha == 16 else None, b, 1,
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "rollout")
    torch.cuda.synchronize()
    return xT.cpu().numpy()[:, 1, :], idx.cpu().numpy()


def main():
    from tests import trig_host
    ang = trig_host.all_arguments()
    out = {}
    for which in ANGLE_SLOT:
        x1, idx = rollout_step(states(ang, which), controls(len(ang)), int(sys.argv[2]))
        out["x_" + which], out["i_" + which] = x1, idx
    np.savez(sys.argv[1], **out)
    print("CHILD-OK")


if __name__ == "__main__":
    main()
