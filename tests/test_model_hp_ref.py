"""Pins of tests/model_hp_ref.py, the long-double / sympy restatement of the quadcopter models that tests/test_models_hard_gpu.py holds
the kernels to -- on the CPU, against everything independent of it in the tree: the oracle's values and the reference's known
answers, the oracle's complex-step Jacobians, torch autograd of the oracle's torch restatement for the second derivatives, and
200-bit mpmath for the claim that long double sits at least 100 times below fp64 rounding on the hard points."""
import json
import os

import numpy as np
import pytest

from oracle import zopt_oracle as zo
from tests import model_hp_ref as hp

KATS = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "reference_kats.json")))["A10_quadcopter"]
WIND = (3.0, 1.0, -0.5)


def _points(P=12):
    """mild and hard points together"""
    xs, us = zip(*[hp.family(name, P, seed=3) for name in hp.FAMILIES])
    return np.concatenate(xs), np.concatenate(us)


def test_values_match_the_oracle_and_the_reference_known_answers():
    x, u = _points()
    for kind, w in (("inertial", (0, 0, 0)), ("inertial", WIND), ("rigid", (0, 0, 0)), ("rigid", (0.5, -0.2, 0.1))):
        n = 12 if kind == "inertial" else 8
        fo, _ = hp.oracle_expansion(kind, x, u, w)
        scale = hp.value_terms(kind, x[:, :n], u, w)
        for f in (hp.values_ld(kind, x[:, :n], u, w), hp.model(kind).values(np.hstack([x[:, :n], u]), w)):
            assert hp.row_error(fo, f, scale) <= 16 * hp.EPS, (kind, w)
    hover = np.array([[9.807, 0, 0, 0]])
    z8, z12 = np.zeros((1, 8)), np.zeros((1, 12))
    assert hp.values_ld("rigid", z8, np.zeros((1, 4)), (0, 0, 0))[0] == pytest.approx(KATS["rigidBody_rest_zero_thrust"]["xDot"])
    assert hp.values_ld("rigid", z8, hover, (0, 0, 0))[0] == pytest.approx(np.zeros(8), abs=1e-18)
    assert hp.values_ld("inertial", z12, hover, (0, 0, 0))[0] == pytest.approx(np.zeros(12), abs=1e-18)
    s = z12.copy()
    s[0, 0:3] = KATS["inertial_norot"]["uvw"]
    assert hp.values_ld("inertial", s, hover, (0, 0, 0))[0, 9:] == pytest.approx(KATS["inertial_norot"]["xyzDot"], abs=1e-16)
    s[0, 8] = np.pi / 2
    assert hp.values_ld("inertial", s, hover, (0, 0, 0))[0, 9:] == pytest.approx(KATS["inertial_psi90"]["xyzDot"], abs=1e-16)
    # quirk Q4 as the oracle documents it: entry [0][2] of the rotation matrix
    R = hp.rotation(hp.LD(0.3), hp.LD(0.2), hp.LD(0.1), hp._NumpyLD)
    assert float(R[0][2]) == pytest.approx(zo.quad_bodyToInertialRotationMatrix(0.3, 0.2, 0.1)[0, 2], rel=1e-15)
    # quirk Q5: psi and the position do not reach the first eight rows
    x, u = hp.family("nominal", 5)
    x2 = x.copy()
    x2[:, 8:] += 1.0
    assert np.array_equal(hp.values_ld("inertial", x, u, (0, 0, 0))[:, :8], hp.values_ld("inertial", x2, u, (0, 0, 0))[:, :8])


def test_jacobians_match_the_complex_step_oracle():
    x, u = _points()
    for kind, w in (("inertial", (0, 0, 0)), ("inertial", WIND), ("rigid", (0, 0, 0)), ("rigid", (0.5, -0.2, 0.1))):
        n = 12 if kind == "inertial" else 8
        _, Jo = hp.oracle_expansion(kind, x, u, w)
        J = hp.model(kind).jacobian(np.hstack([x[:, :n], u]), w)
        assert hp.row_error(Jo, J) <= 64 * hp.EPS, (kind, w)


def test_still_air_second_derivatives_match_autograd():
    x, u = _points(6)
    for kind in ("inertial", "rigid"):
        n = 12 if kind == "inertial" else 8
        H = hp.model(kind).hessian(np.hstack([x[:, :n], u]))
        assert hp.row_error(hp.oracle_hessian(kind, x, u), H) <= 256 * hp.EPS, kind
        assert np.array_equal(H, np.swapaxes(H, -1, -2))


def test_declared_pairs_cover_every_nonzero_second_derivative():
    """the 28 pairs of models.h (model_pair_table) contain every pair sympy finds not identically zero, wind included"""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zopt_amd", "csrc", "models.h")).read().lower()
    assert len(hp.PAIR_TABLE) == 28 and all(f"0x{ab:02x}" in src for ab in hp.PAIR_TABLE)      # the one Python copy is models.h's table
    declared = {tuple(sorted((ab >> 4, ab & 15))) for ab in hp.PAIR_TABLE}
    assert set(hp.model("inertial").nonzero_pairs()) <= declared


def test_long_double_sits_100_times_below_fp64_rounding_on_hard_points():
    """about 20 hard points: values, Jacobians and second derivatives in long double against 200-bit mpmath, in the row metric"""
    xs, us = zip(*[hp.family(name, 4, seed=9) for name in ("many_turns", "quadrants", "gimbal", "scaled", "zeros")])
    x, u = np.concatenate(xs), np.concatenate(us)
    worst = 0.0
    for kind, w in (("inertial", (-30.0, 12.0, 4.0)), ("rigid", (5.0, -3.0, 1.0))):
        n = 12 if kind == "inertial" else 8
        m, z = hp.model(kind), np.hstack([x[:, :n], u])
        scale = hp.value_terms(kind, x[:, :n], u, w)
        worst = max(worst, hp.row_error(m.values(z, w), m.values(z, w, backend="mp"), scale),
                    hp.row_error(hp.values_ld(kind, x[:, :n], u, w), m.values(z, w, backend="mp"), scale),
                    hp.row_error(m.jacobian(z, w), m.jacobian(z, w, backend="mp")),
                    hp.row_error(m.hessian(z, w), m.hessian(z, w, backend="mp")))
    print(f"long double against mpmath: worst row error {worst:.2e} (fp64 rounding / 100 = {hp.EPS / 100:.2e})")
    assert worst <= hp.EPS / 100


def test_row_metric_and_rollout_helper():
    ref = np.array([[[1e20, 1.0], [0.5, 0.25]]])
    got = ref + np.array([[[1e4, 0.0], [1e-3, 0.0]]])
    assert hp.row_error(got, ref) == pytest.approx(1e-3)                  # the large row does not excuse the small one
    assert hp.row_error(np.array([[[np.nan, 1.0]]]), np.array([[[np.inf, 1.0]]])) == 0.0
    assert hp.row_error(np.array([[[np.nan, 1.0]]]), np.array([[[2.0, 1.0]]])) == np.inf
    assert hp.bound(0.0) == hp.FLOOR and hp.bound(1e-12) == pytest.approx(1e-10)
    # the batch rollout against the oracle's single-trajectory one
    rng = np.random.default_rng(0)
    x0, u = hp.family("nominal", 3)
    N = 4
    l, L = 0.1 * rng.standard_normal((3, N, 4)), 0.01 * rng.standard_normal((3, N, 4, 12))
    xp, up = rng.standard_normal((3, N + 1, 12)), hp.U_TRIM + 0.1 * rng.standard_normal((3, N, 4))
    xs, us = hp.rollout(x0, l, L, xp, up, 0.5, hp.euler_step_oracle((0, 0, 0), 0.1))
    xl, _ = hp.rollout(x0.astype(hp.LD), l, L, xp, up, 0.5, hp.euler_step_ld((0, 0, 0), 0.1))
    for b in range(3):
        r = zo.trajectoryRollout(x0[b], zo.quad_euler_step(0.1), zo.AffinePolicy(l[b], L[b]), zo.Trajectory(xp[b], up[b]), 0.5)
        assert np.allclose(xs[b], r.xTraj, rtol=0, atol=1e-13) and np.allclose(us[b], r.uTraj, rtol=0, atol=1e-13)
    assert hp.traj_error(xs, xl) <= 1e-13
