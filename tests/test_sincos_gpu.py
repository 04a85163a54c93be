"""zm_sincos on the device, through every consumer, bit for bit against the host build of the same header (tests/trig_shim.cpp,
whose error against 400-bit arithmetic tests/test_sincos.py asserts): a wrong quadrant for negative k, a lost FMA of the two-step
reduction or a compiler contraction inside one consumer changes bits here.  No new entry point: tests/sincos_probe_child.py
explains why the position rows of inertialDynamics carry cos / sin of one angle exactly.

Consumers: Quadcopter.inertialDynamics (dt = 0; the value path of linearize_dynamics_kernel), mpcUtils.modelStep, a one-step
trajectoryRollout (no cost: the generic lane-per-trajectory kernel), the fast line-search kernel with one step size (one lane per
rollout) and with 16 (winner re-rolled on four lanes per rollout), the generic 16-step-size kernel (ZOPT_AMD_ROLLOUT_PATH=generic,
a child process), and the 8-state model through rigidBodyDynamics and modelStep.

The 8-state model has no position rows.  Its value expressions that are exact at probe inputs (models.h, quad_rigid_body_trig):
    thetaDot = cphi q - sphi r          -> cos phi at (q, r) = (1, 0), -sin phi at (0, 1)
    phiDot = p + sphi tth q + cphi tth r -> tan theta = fl(sin theta / cos theta) at phi = 0, (p, q, r) = (0, 0, 1)
(the uvw rows add gravity and drag terms to the sines: not exact).  The last one is compared with the IEEE quotient of the host
build's sine and cosine: fp64 division is correctly rounded on both sides.

Zeros are compared as values (-0.0 == +0.0): a sum `s + 0 * y` does not keep the sign of a zero.  NaN must meet NaN."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import sincos_probe_child as probe
from tests import trig_host

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANGLES = ("psi", "theta", "phi")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    """the whole argument set of the CPU test plus the non-finite arguments, and the host build's bits on it"""
    import torch
    assert torch.cuda.is_available()
    host = trig_host.build(tmp_path_factory.mktemp("trig"))
    x = np.concatenate([trig_host.all_arguments(), trig_host.SPECIALS])
    s, c = trig_host.sincos(host, x)
    return x, s, c


def _same(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    nan = np.isnan(want)
    if not np.array_equal(np.isnan(got), nan):
        return False
    return np.array_equal((got[~nan] + 0.0).view(np.uint64), (want[~nan] + 0.0).view(np.uint64))


def _check(xd, which, s, c, what):
    gc, gs = probe.read(xd, which)
    bad = np.flatnonzero(~((gc == c) | (np.isnan(gc) & np.isnan(c))) | ~((gs == s) | (np.isnan(gs) & np.isnan(s))))
    assert _same(gc, c) and _same(gs, s), (what, which, len(bad), bad[:5])


# batch sizes that do not fill a 16-lane group or a wave, and the whole set (25,719 arguments) in one launch
def _batches(count):
    return [slice(0, 1), slice(7, 10), slice(4000, 4067), slice(0, count)]


@pytest.mark.parametrize("which", ANGLES)
def test_inertial_dynamics(ref, which):
    from zopt_amd import models
    x, s, c = ref
    ac = models.Quadcopter()
    for sl in _batches(len(x)):
        xd = ac.inertialDynamics(probe.states(x[sl], which), probe.controls(len(x[sl])))
        _check(xd, which, s[sl], c[sl], "inertialDynamics")


@pytest.mark.parametrize("which", ANGLES)
def test_model_step(ref, which):
    from zopt_amd import models, mpcUtils
    x, s, c = ref
    for sl in _batches(len(x)):
        xn = mpcUtils.modelStep(models.QuadcopterEuler(1.0), probe.states(x[sl], which), probe.controls(len(x[sl])))
        _check(xn, which, s[sl], c[sl], "modelStep")


@pytest.mark.parametrize("which", ANGLES)
def test_trajectory_rollout_generic_lane_kernel(ref, which):
    from zopt_amd import ilqrUtils, models, pytrees as pt
    x, s, c = ref
    for sl in _batches(len(x)):
        b = len(x[sl])
        traj = ilqrUtils.trajectoryRollout(probe.states(x[sl], which), models.QuadcopterEuler(1.0),
                                           pt.AffinePolicy(np.zeros((b, 1, 4)), np.zeros((b, 1, 4, 12))),
                                           pt.Trajectory(np.zeros((b, 2, 12)), probe.controls(b)[:, None, :]))
        _check(traj.xTraj[:, 1, :], which, s[sl], c[sl], "trajectoryRollout")


@pytest.mark.parametrize("n_alpha", [1, 16])
@pytest.mark.parametrize("which", ANGLES)
def test_fast_rollout_kernels_one_lane_and_four_lanes(ref, which, n_alpha):
    """finite arguments only: a NaN cost has no winner"""
    x, s, c = ref
    fin = np.isfinite(x)
    x, s, c = x[fin], s[fin], c[fin]
    for sl in _batches(len(x)):
        x1, idx = probe.rollout_step(probe.states(x[sl], which), probe.controls(len(x[sl])), n_alpha)
        if n_alpha == 16:
            assert np.all(idx == 15)           # every winner was re-rolled: the four-lane kernel wrote these rows
        _check(x1, which, s[sl], c[sl], f"fast rollout, {n_alpha} step sizes")


def test_generic_line_search_kernel(ref, tmp_path):
    x, s, c = ref
    fin = np.isfinite(x)
    out = tmp_path / "generic.npz"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "sincos_probe_child.py"), str(out), "16"],
                       env=dict(os.environ, ZOPT_AMD_ROLLOUT_PATH="generic"), capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0 and "CHILD-OK" in p.stdout, (p.stdout[-300:], p.stderr[-1500:])
    res = np.load(out)
    for which in ANGLES:
        assert np.all(res["i_" + which] == 15)
        _check(res["x_" + which], which, s[fin], c[fin], "generic line search")


def test_rigid_body_model(ref):
    from zopt_amd import models, mpcUtils
    x, s, c = ref
    ac = models.Quadcopter()
    with np.errstate(all="ignore"):
        t = s / c
    for sl in _batches(len(x)):
        b = len(x[sl])
        u = probe.controls(b)
        z = np.zeros((b, 8))
        for q, r, want in ((1.0, 0.0, c[sl]), (0.0, 1.0, -s[sl])):
            st = z.copy()
            st[:, 4], st[:, 5], st[:, 6] = q, r, x[sl]
            assert _same(ac.rigidBodyDynamics(st, u)[:, 7], want), ("rigidBodyDynamics", q, r)
            assert _same(mpcUtils.modelStep(models.QuadcopterRigidBody(1.0), st, u)[:, 7], want), ("modelStep, 8 states", q, r)
        st = z.copy()
        st[:, 5], st[:, 7] = 1.0, x[sl]
        assert _same(ac.rigidBodyDynamics(st, u)[:, 6], t[sl]), "rigidBodyDynamics, tan"
        assert _same(mpcUtils.modelStep(models.QuadcopterRigidBody(1.0), st, u)[:, 6], t[sl]), "modelStep, 8 states, tan"
