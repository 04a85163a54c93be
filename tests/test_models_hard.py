"""The host builds of the model code on the hard point families, without a GPU: the generated closed forms (quad_derivs_gen.h through
tests/quad_derivs_shim.cpp: full Jacobians, the packed image and its one-lane straight-line form, the declared pairs, the sparse
second-derivative image) and the fast rollout kernels' step (trig.h + quad_step.h through tests/trig_shim.cpp) against the long-double
reference of tests/model_hp_ref.py, in its row metric and within its bounds (100 x the fp64 oracle's own error on the same points).

The packed images are what the solvers' expansion kernels write (expand_quad_points_kernel: one lane per point; with the lab switch
ZOPT_AMD_EXPAND=group, 16 lanes per point).  Those kernels have no entry point of their own -- they run inside a solve -- so their
formulas are held to the hard families entry by entry here; tests/test_expand_forms_hard_gpu.py runs the kernels themselves on the
families through one iteration of the solvers (every form bit for bit the full form, the first gains against long double).
(quad_derivs_shim.cpp takes its sines and cosines from libm: zm_sincos has its own tests, tests/test_sincos.py.)"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import model_hp_ref as hp
from tests import trig_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE_IDS = [hp.case_id(c) for c in hp.CASES]
dp = ctypes.POINTER(ctypes.c_double)


def _p(a):
    return a.ctypes.data_as(dp)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = tmp_path_factory.mktemp("quad_derivs_hard") / "quad_derivs_shim.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-o", str(so),
                    os.path.join(ROOT, "tests", "quad_derivs_shim.cpp")], check=True)
    lib = ctypes.CDLL(str(so))
    lib.quad_jacobian.argtypes = [dp, dp, dp, ctypes.c_int, dp]
    lib.quad_hessian_pairs.argtypes = [dp, dp, dp, ctypes.c_int, ctypes.c_int, dp]
    lib.quad_jacobian_packed.argtypes = [dp, dp, dp, ctypes.c_int, ctypes.c_double, dp, ctypes.POINTER(ctypes.c_ubyte)]
    lib.quad_jacobian_packed.restype = ctypes.c_int
    lib.quad_hessian_sparse.argtypes = [dp, dp, dp, ctypes.c_int, ctypes.c_double, dp, ctypes.POINTER(ctypes.c_ushort)]
    lib.quad_hessian_sparse.restype = ctypes.c_int
    lib.quad_all_packed.argtypes = [dp, dp, dp, ctypes.c_int, ctypes.c_double, dp, dp]
    lib.quad_all_packed.restype = None
    return lib


def _forms(c):
    """[still_air flag]: the wind form always; at zero wind also the still-air form"""
    return [0] if any(c.w) else [0, 1]


def _pairs_of(H):
    """(P, 12, 16, 16) -> (P, 28, 12): the declared pairs in the order of the table"""
    return np.stack([H[:, :, ab >> 4, ab & 15] for ab in hp.PAIR_TABLE], axis=1)


@pytest.mark.parametrize("case", hp.CASES, ids=CASE_IDS)
def test_closed_form_jacobians(shim, case):
    c = hp.expansion_case("inertial", case[0], case[1], 0.0)
    w = np.array(c.w)
    with np.errstate(all="ignore"):
        for still in _forms(c):
            J = np.zeros((hp.NPOINTS, 12, 16))
            for p in range(hp.NPOINTS):
                shim.quad_jacobian(_p(c.x[p]), _p(c.u[p]), _p(w), still, _p(J[p]))
            assert hp.finite_where_reference_is(J, c.F)
            err = hp.row_error(J, c.F)
            print(f"{hp.case_id(case)} still={still}: {err:.2e} (oracle {c.e_F:.2e}, bound {c.b_F:.2e})")
            assert err <= c.b_F


@pytest.mark.parametrize("case", hp.CASES, ids=CASE_IDS)
def test_packed_jacobian_image_and_its_straight_line_form(shim, case):
    """the image rebuilt to [f_x | f_u] = I + dt J (entries outside it: the identity's) against the reference; the one-lane form
    writes the same bits as the per-column form"""
    dt = 0.1
    c = hp.expansion_case("inertial", case[0], case[1], dt)
    w = np.array(c.w)
    with np.errstate(all="ignore"):
        for still in _forms(c):
            F = np.zeros((hp.NPOINTS, 12, 16))
            for p in range(hp.NPOINTS):
                t, pos = np.full(64, np.nan), np.zeros(192, dtype=np.uint8)
                nj = shim.quad_jacobian_packed(_p(c.x[p]), _p(c.u[p]), _p(w), still, dt, _p(t), pos.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)))
                pos = pos.reshape(12, 16)
                F[p] = np.hstack([np.eye(12), np.zeros((12, 4))])
                F[p][pos != 255] = t[pos[pos != 255]]
                aj, ah = np.full(64, np.nan), np.full(96, np.nan)
                shim.quad_all_packed(_p(c.x[p]), _p(c.u[p]), _p(w), still, dt, _p(aj), _p(ah))
                assert np.array_equal(aj[:nj], t[:nj], equal_nan=True), (p, still)
            assert hp.finite_where_reference_is(F, c.F)
            assert hp.row_error(F, c.F) <= c.b_F, still


@pytest.mark.parametrize("case", hp.CASES, ids=CASE_IDS)
def test_closed_form_second_derivatives_and_their_sparse_image(shim, case):
    """the 28 declared pairs against the reference (every undeclared pair of the reference is identically zero:
    tests/test_model_hp_ref.py); the sparse image holds dt times the same bits"""
    dt = 0.1
    c0 = hp.expansion_case("inertial", case[0], case[1], 0.0)
    w = np.array(c0.w)
    ref = np.swapaxes(_pairs_of(c0.H), 1, 2)                      # (P, 12 rows, 28 pairs)
    with np.errstate(all="ignore"):
        for still in _forms(c0):
            H = np.zeros((hp.NPOINTS, 28, 12))
            for p in range(hp.NPOINTS):
                shim.quad_hessian_pairs(_p(c0.x[p]), _p(c0.u[p]), _p(w), still, 28, _p(H[p]))
                t, dense = np.full(96, np.nan), np.zeros(96, dtype=np.uint16)
                nh = shim.quad_hessian_sparse(_p(c0.x[p]), _p(c0.u[p]), _p(w), still, dt, _p(t), dense.ctypes.data_as(ctypes.POINTER(ctypes.c_ushort)))
                R = np.zeros(28 * 12)
                R[dense[:nh]] = t[:nh]
                assert np.array_equal(R.reshape(28, 12), dt * H[p], equal_nan=True), (p, still)
            got = np.swapaxes(H, 1, 2)
            assert hp.finite_where_reference_is(got, ref)
            # rows scaled by the whole row of the reference tensor, as on the device
            scale = np.max(np.abs(c0.H.reshape(hp.NPOINTS, 12, -1)), axis=2)
            err = hp.row_error(got, ref, np.where(np.isfinite(scale), scale, 0))
            print(f"{hp.case_id(case)} still={still}: {err:.2e} (oracle {c0.e_H:.2e}, bound {c0.b_H:.2e})")
            assert err <= c0.b_H


@pytest.fixture(scope="module")
def host():
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        yield trig_host.build(d)


@pytest.mark.parametrize("fam", hp.FAMILIES)
def test_fast_rollout_step_on_the_host(host, fam):
    """one step of the fast rollout kernels' arithmetic (zm_sincos + quad_euler_step_trig, built for the host) from every point of
    the family against the long-double step, within the values' bound"""
    c = hp.expansion_case("inertial", fam, False, 0.1)
    with np.errstate(all="ignore"):
        xn = trig_host.quad_step(host, c.x, c.u, 0.1)
    assert hp.finite_where_reference_is(xn, c.f)
    err = hp.row_error(xn[:, :, None], c.f[:, :, None], c.fscale)
    print(f"{fam}: {err:.2e} (oracle {c.e_f:.2e}, bound {c.b_f:.2e})")
    assert err <= c.b_f


@pytest.mark.parametrize("N", [1, 2, 3, 7])
@pytest.mark.parametrize("fam", hp.FAMILIES)
def test_fast_rollouts_on_the_host(host, fam, N):
    """short rollouts from the hard initial states with the host build of the fast kernels' step, per trajectory and per prefix of
    steps within 100 x the oracle rollout's own error (model_hp_ref.RolloutCase)"""
    rc = hp.rollout_case(fam, N)
    assert rc.determined[:, 0].all()                   # every initial state is compared on its first step at least
    x0, l, L, xp, up = rc.problem
    with np.errstate(all="ignore"):
        xs, us = hp.rollout(x0, l, L, xp, up, hp.ROLLOUT_ALPHA, lambda x, u: trig_host.quad_step(host, x, u, hp.ROLLOUT_DT))
    worst, finite = rc.worst(xs, us)
    print(f"{fam} N={N}: worst error / bound {worst:.3f}; {rc.summary()}")
    assert finite and worst <= 1.0


def test_long_spinning_rollout_on_the_host(host):
    """N = 200, dt = 0.1, r = 50 rad/s: psi passes 1e3 rad (model_hp_ref.spinning_problem)"""
    x0, l, L, xp, up = hp.spinning_problem()
    xl, ul = hp.rollout(x0.astype(hp.LD), l, L, xp, up, 1.0, hp.euler_step_ld((0, 0, 0), 0.1))
    xo, _ = hp.rollout(x0, l, L, xp, up, 1.0, hp.euler_step_oracle((0, 0, 0), 0.1))
    xs, _ = hp.rollout(x0, l, L, xp, up, 1.0, lambda x, u: trig_host.quad_step(host, x, u, 0.1))
    assert float(xl[0, -1, 8]) > 1e3 and 0.1 < float(np.abs(xl[0, -1, :2]).max()) < 10.0 and np.all(np.isfinite(xs))
    e = hp.traj_error(xo, xl)
    print(f"spinning: host step {hp.traj_error(xs, xl):.2e}, oracle {e:.2e}, bound {hp.bound(e):.2e}")
    assert hp.traj_error(xs, xl) <= hp.bound(e)
