"""The solvers' expansion kernels on the hard point families, on the device.  expand_quad_points_kernel (one lane per point, LDS tile,
chunks of at most 32 points), quad_hessian_points_kernel, the packed instantiations of linearize_dynamics_kernel and
quad_hessian_pairs16_kernel (16 lanes per point) have no entry point: they run inside zm_ilqr_solve_f64.  So one iteration of
iterativeLqr and differentialDynamicProgramming is run from the hard points (tests/expand_forms_child.py: every point of every
family as x_0 of a horizon-2 solve in batches of 1, 3, 17, 67, and a horizon of 40 for the chunks and tails), in one child process
per form with the lab build of the library:

    form      ZOPT_AMD_EXPAND  ZOPT_AMD_JAC  ZOPT_AMD_HES
    points    points           packed        sparse         expand_quad_points_kernel, quad_hessian_points_kernel (the default)
    group     group            packed        sparse         linearize_dynamics_kernel<.., PACKED>, quad_hessian_pairs16_kernel<.., SPARSE>
    points-d  points           packed        dense          ... with the dense 28 x 12 rows (zm_quadratic_dynamics_pairs_list_f64)
    group-d   group            packed        dense
    full      points           full          dense          the full [f_x | f_u] and the dense pairs

1. Every form returns the bits of `full`: trajectory, gains, cost, for both solvers, with and without wind (NaN meets NaN: from gimbal
   lock the first step leaves the fp64 range).  The kernels behind `full` are the ones tests/test_models_hard_gpu.py holds to long double.
2. iLQR's gains of `full` against a long-double Riccati sweep (hp_reference.ilqr_backward_ld) over the long-double expansion
   (model_hp_ref) at the expansion points -- the initial rollout, which the child obtains by the solver's own call.  Metric: per
   trajectory, max |L - L_ref| / max |L_ref|.  Bound: per trajectory, 100 x the error of the fp64 oracle (zo.backwardPass_ilqr over the
   complex-step expansion) against the same reference, floor 100 x 2^-52; where the oracle's own error has reached 1e-4, or the
   reference is not finite in fp64, the trajectory is not determined and is not compared (the rule of model_hp_ref.RolloutCase);
   every trajectory of the nominal, many_turns, scaled and zeros families must be determined.
   DDP's gains also pass through the PD projection, whose resolution (2e-11 |X|_F) tests/test_sweeps_hard_gpu.py bounds on its own
   families; here DDP is held to `full` bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import zopt_oracle as zo
from tests import expand_forms_child as child
from tests import hp_reference as hpr
from tests import model_hp_ref as hp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAB = os.path.join(ROOT, "zopt_amd", "csrc", "libzopt_amd_lab.so")
FORMS = {"points": ("points", "packed", "sparse"), "group": ("group", "packed", "sparse"), "points-d": ("points", "packed", "dense"),
         "group-d": ("group", "packed", "dense"), "full": ("points", "full", "dense")}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{form: the child's arrays}: five child processes, one after the other"""
    import torch
    assert torch.cuda.is_available()
    d = tmp_path_factory.mktemp("expand_forms")
    out = {}
    for form, (ex, jac, hes) in FORMS.items():
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "expand_forms_child.py"), str(d / f"{form}.npz")],
                           env=dict(os.environ, ZOPT_AMD_LIB=LAB, ZOPT_AMD_EXPAND=ex, ZOPT_AMD_JAC=jac, ZOPT_AMD_HES=hes),
                           capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert p.returncode == 0 and "CHILD-OK" in p.stdout, (form, p.stdout[-300:], p.stderr[-1500:])
        out[form] = dict(np.load(d / f"{form}.npz"))
    return out


@pytest.mark.parametrize("form", [f for f in FORMS if f != "full"])
def test_every_form_returns_the_bits_of_the_full_form(runs, form):
    ref, got = runs["full"], runs[form]
    assert set(ref) == set(got) and len(ref) == 9 * 5 * 10
    for k in sorted(ref):
        assert np.array_equal(ref[k], got[k], equal_nan=True), (form, k)
    # the comparison is of real solves: gains were written, and they differ between the two solvers where second derivatives matter
    assert np.all(np.isfinite(ref["nominal_67x2_ilqr_L"])) and np.any(ref["nominal_67x2_ilqr_L"] != 0.0)
    assert not np.array_equal(ref["nominal_67x2_ilqr_L"], ref["nominal_67x2_ddp_L"])


def _gain_reference(x, u, w):
    """(L_ref (b, N, 4, 12) long double, oracle's L (b, N, 4, 12)) of the iLQR backward pass about the trajectory x (b, N + 1, 12), u"""
    b, N = u.shape[:2]
    xs, us = x[:, :N].reshape(-1, 12), u.reshape(-1, 4)
    f, F, _ = hp.step_reference("inertial", xs, us, w, child.DT)
    fo, Fo = hp.step_oracle("inertial", xs, us, w, child.DT)
    Qx, Ru = 2 * child.Q, 2 * child.R

    def parts(f, F, dtype):
        F = F.reshape(b, N, 12, 16)
        dyn = (f.reshape(b, N, 12), F[..., :12], F[..., 12:])
        X, U = x[:, :N].astype(dtype), u.astype(dtype)
        cost = (np.zeros((b, N), dtype), X @ Qx.astype(dtype), U @ Ru.astype(dtype), np.broadcast_to(Qx.astype(dtype), (b, N, 12, 12)),
                np.zeros((b, N, 4, 12), dtype), np.broadcast_to(Ru.astype(dtype), (b, N, 4, 4)))
        Vf = (np.zeros(b, dtype), x[:, N].astype(dtype) @ (2 * child.QF).astype(dtype), np.broadcast_to((2 * child.QF).astype(dtype), (b, 12, 12)))
        return dyn, cost, Vf
    with np.errstate(all="ignore"):
        Lref = hpr.ilqr_backward_ld(*parts(f, F, hp.LD))["L"]
        dyn, cost, Vf = parts(fo, Fo, np.float64)
        Lo = np.full((b, N, 4, 12), np.nan)
        for i in range(b):
            if np.all(np.isfinite(dyn[1][i])) and np.all(np.isfinite(Vf[1][i])):
                try:
                    Lo[i] = zo.backwardPass_ilqr(zo.AffineDynamics(*(t[i] for t in dyn)), zo.QuadraticCostFunction(*(np.array(t[i]) for t in cost)),
                                                 zo.QuadraticValueFunction(*(np.array(t[i]) for t in Vf))).L
                except np.linalg.LinAlgError:
                    pass
    return Lref, Lo


def _traj_err(L, Lref):
    """(b,): max |L - L_ref| / max |L_ref| per trajectory; inf where L is not finite"""
    with np.errstate(all="ignore"):
        d = np.max(np.abs(L.astype(hp.LD) - Lref).reshape(len(L), -1), axis=1) / np.max(np.abs(Lref).reshape(len(L), -1), axis=1)
    return np.where(np.all(np.isfinite(L.reshape(len(L), -1)), axis=1), d.astype(np.float64), np.inf)


@pytest.mark.parametrize("case", hp.CASES, ids=[hp.case_id(c) for c in hp.CASES])
def test_first_gains_against_the_long_double_riccati_sweep(runs, case):
    full = runs["full"]
    w = hp.WINDS[case[0]] if case[1] else (0.0, 0.0, 0.0)
    for b, N in child.SHAPES:
        key = f"{hp.case_id(case)}_{b}x{N}"
        Lref, Lo = _gain_reference(full[key + "_xinit"], full[key + "_uinit"], w)
        fin = np.all(np.isfinite(Lref.astype(np.float64)).reshape(b, -1), axis=1)
        with np.errstate(all="ignore"):
            eo = np.where(fin, _traj_err(Lo, Lref), np.inf)
        det = fin & (eo <= hp.DETERMINED)
        bound = np.maximum(hp.FLOOR, 100.0 * np.where(det, eo, 0.0))
        err = _traj_err(full[key + "_ilqr_L"], Lref)
        ratio = np.where(det, err / bound, 0.0)
        print(f"{key}: {int(det.sum())}/{b} determined, oracle error up to {np.max(eo[det], initial=0.0):.1e}, worst error / bound {ratio.max():.3f}")
        if case[0] in ("nominal", "many_turns", "scaled", "zeros"):
            assert det.all(), key
        assert np.all(ratio <= 1.0), (key, np.flatnonzero(ratio > 1.0)[:5], err[ratio > 1.0][:5], bound[ratio > 1.0][:5])
