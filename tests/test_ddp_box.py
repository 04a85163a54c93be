"""CPU tests of DDP with an input box: the conditions the GPU tests' cases rest on (tests/ddp_box_cases.py), the restatement
(tests/ddp_box_ref.py) against the references without a box, and the host-side surface of the feature."""
import ctypes

import numpy as np
import pytest

from tests import ddp_box_cases as cases
from tests import ddp_box_ref as dr
from tests import hp_reference as hp

INF = np.inf
EPS64 = float(np.finfo(np.float64).eps)


# ------------------------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("family", cases.SWEEP_FAMILIES)
def test_sweep_cases_hold_their_conditions(family):
    """every step of every case has a strict-complementarity margin, the fp64 restatement finds the long-double clamped sets, the
    sets survive a perturbation of every projected matrix by 10 x the projection's resolution, the family clamps somewhere, and
    u + l stays inside the box"""
    clamped = 0
    for shape in cases.family_shapes(family):
        c = cases.sweep_case(family, *shape)
        ref = c["ref"]
        assert ref["margin"].min() >= cases.MARGIN, (family, shape, ref["margin"].min())
        assert c["same64"] and c["stable"], (family, shape)
        clamped += int(np.count_nonzero(ref["clamped"]))
        u, lb, ub = c["args"][3:]
        B, m = shape[3], shape[1]
        for o in (ref, c["o64"]):             # (each in its own precision: lb - u_k is exact in long double, rounded in fp64)
            dt = o["l"].dtype
            lo = np.expand_dims(np.broadcast_to(lb, (B, m)), 1).astype(dt) - u.astype(dt)
            hi = np.expand_dims(np.broadcast_to(ub, (B, m)), 1).astype(dt) - u.astype(dt)
            assert np.all(o["l"] >= lo) and np.all(o["l"] <= hi), (family, shape)
        assert np.isfinite(c["s_l"]) and np.isfinite(c["s_L"])
    assert clamped > 0, family


@pytest.mark.parametrize("name", cases.SOLVE_CASES)
def test_solve_cases_hold_their_conditions(name):
    """the restatement's solves: every backward pass has its margin and clamps something, the best two of the 16 costs of every
    line search are apart by COST_GAP (the winning index cannot hinge on rounding) or, on the rigid-body case only, tie exactly;
    every stored input is feasible; the torch restatement of the rigid-body step is the oracle's step"""
    if name == "rb":
        import torch
        from oracle import zopt_oracle as zo
        rng = np.random.default_rng(3)
        for _ in range(5):
            x, u = 0.3 * rng.standard_normal(8), np.array([9.807, 0, 0, 0]) + 0.1 * rng.standard_normal(4)
            xt = dr.rigid_body_step_torch(0.1)(torch.as_tensor(x), torch.as_tensor(u)).numpy()
            assert np.max(np.abs(xt - (x + 0.1 * zo.quad_rigidBodyDynamics(x, u)))) <= 4 * EPS64 * max(1.0, np.max(np.abs(xt)))
    c = cases.solve_case(name)
    for b, r in enumerate(cases.solve_reference(name)):
        assert r["converged"] and 1 <= r["its"] < c["kw"]["maxIter"], (name, b)
        for J_new, idx, Js, clamped, margin in r["trace"]:
            assert margin.min() >= cases.MARGIN, (name, b, margin.min())
            assert np.count_nonzero(clamped) > 0, (name, b)
            # rb: an exact tie (coinciding clipped rollouts) is allowed -- the accepted cost is then the same whichever index wins,
            # and the GPU test compares no index there; a gap between 0 and COST_GAP is allowed nowhere
            gap = cases.cost_gap(Js)
            assert gap >= cases.COST_GAP or (name == "rb" and gap == 0.0), (name, b, gap)
            assert cases.index_comparable(Js) == (gap >= cases.COST_GAP)
            assert Js[idx] == J_new
        assert np.all(r["traj"].uTraj >= c["lb"]) and np.all(r["traj"].uTraj <= c["ub"])


# ------------------------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("family", ["plain", "strongly_indefinite", "control_affine_8"])
def test_restatement_without_bounds_is_the_unboxed_reference(family):
    """With infinite bounds nothing is clamped and the restatement is the DDP sweep: in long double it reproduces hp.ddp_backward_hp,
    in fp64 zo.backwardPass_ddp.  Up to the box step the two pairs run the same operations; the box step forms v_x' and v_xx' from
    four terms where the unboxed tail uses two and solves through the masked system, so the pairs differ by rounding of their own
    precision, accumulated over the horizon as the references' own rounding is.  The yardstick is therefore the two references'
    own difference d = metric(zo.backwardPass_ddp, hp.ddp_backward_hp) (fp64 rounding over the same horizon, never below one ulp):
    fp64 pair <= 10 d, long-double pair <= 10 d eps_ld / eps_64."""
    eps_ld = float(np.finfo(np.longdouble).eps)
    for (n, m, T, B, _) in cases.SWEEP_SHAPES:
        c = cases.unbounded_case(family, n, m, T, B)
        dyn, cost, Vf = c["args"]
        u = np.zeros((B, T, m))
        o64 = dr.ddp_box_backward(dyn, cost, Vf, u, np.full(m, -INF), np.full(m, INF))
        old = dr.ddp_box_backward(dyn, cost, Vf, u, np.full(m, -INF), np.full(m, INF), ld=True)
        assert not o64["clamped"].any() and not old["clamped"].any()
        for name, ref64 in (("l", c["o64"].l), ("L", c["o64"].L)):
            d = max(float(hp.sweep_metric(ref64, c["ref"][name]).max()), EPS64)
            e64 = float(hp.sweep_metric(o64[name], ref64).max())
            eld = float(hp.sweep_metric(old[name], c["ref"][name]).max())
            assert e64 <= 10 * d, (family, (n, m, T, B), name, e64, d)
            assert eld <= 10 * d * eps_ld / EPS64, (family, (n, m, T, B), name, eld, d)


# ------------------------------------------------------------------------------------------------------------------------------- 3
ENTRY_POINTS = ("zm_ddp_backward_box_list_f64", "zm_ddp_backward_box_f64", "zm_ddp_backward_pairs_box_list_f64", "zm_ilqr_solve_box_f64",
                "zm_ilqr_solve_box_trace_f64")


def test_library_exports_the_entry_points():
    from zopt_amd import _lib
    handle = ctypes.CDLL(_lib.LIB_PATH)
    lab = ctypes.CDLL(_lib.LAB_LIB_PATH)
    for name in ENTRY_POINTS:
        assert hasattr(handle, name) and hasattr(lab, name), name
        assert name in _lib.SYMBOLS, name


def test_entry_points_check_their_arguments_before_any_launch():
    """bad arguments come back with their code from a machine without a device: no check sits behind a launch"""
    from zopt_amd import _lib, models
    lib = _lib.lib()
    p = ctypes.addressof((ctypes.c_double * 2)())                 # a non-null address that no check dereferences
    box = models.zm_inputbox_t(p, p, 0)
    pb = ctypes.addressof(box)
    tens = lambda f_ux=p, f_uu=p, uT=p, bx=pb, n=3, m=2, cnt=0, lst=None: (      # noqa: E731
        p, p, p, f_ux, f_uu, p, p, p, p, p, p, p, uT, bx, lst, cnt, None, 0, p, p, None, 4, 3, n, m, None)
    call = lib.zm_ddp_backward_box_list_f64
    assert call(*tens(uT=None)) == _lib.ZM_EINVAL
    assert call(*tens(f_uu=None)) == _lib.ZM_EINVAL                # f_ux and f_uu only together
    assert call(*tens(n=13)) == _lib.ZM_EUNSUPPORTED and b"not covered" in lib.zm_last_error()
    assert call(*tens(m=5)) == _lib.ZM_EUNSUPPORTED and b"not covered" in lib.zm_last_error()
    assert call(*tens(bx=None)) == _lib.ZM_EINVAL
    assert call(*tens(bx=ctypes.addressof(models.zm_inputbox_t(p, p, 3)))) == _lib.ZM_EINVAL      # stride neither 0 nor m
    assert call(*tens(lst=p, cnt=5)) == _lib.ZM_EINVAL             # a list longer than the batch
    md = models.QuadcopterEuler(0.1).c_struct()
    pairs = lambda mdl, uT=p, bx=pb: (mdl, p, p, p, p, p, p, p, p, p, p, uT, bx, None, 0, None, 1, p, p, None, 4, 3, None)      # noqa: E731
    call = lib.zm_ddp_backward_pairs_box_list_f64
    assert call(*pairs(ctypes.addressof(md), uT=None)) == _lib.ZM_EINVAL
    assert call(*pairs(ctypes.addressof(md), bx=None)) == _lib.ZM_EINVAL


def test_host_side_refusals_of_the_wrappers():
    from zopt_amd import ilqrUtils, models
    z = lambda *s: np.zeros(s)      # noqa: E731
    for n, m in ((13, 2), (4, 5)):
        dyn = (None, z(2, 3, n, n), z(2, 3, n, m), z(2, 3, n, n, n), z(2, 3, n, m, n), z(2, 3, n, m, m))
        with pytest.raises(ValueError, match="not covered"):
            ilqrUtils.backwardPass_ddp_box(dyn, (None,) * 6, (None,) * 3, None, -1.0, 1.0)
    lin = models.LinearModel(np.eye(3), np.ones((3, 2)))
    cost = models.QuadraticCost(np.eye(3), np.eye(2))
    with pytest.raises(ValueError, match="takes no InputBox.*no second derivatives.*iterativeLqr"):
        ilqrUtils.differentialDynamicProgramming(models.InputBox(lin, -1.0, 1.0), cost, cost, np.zeros(3), np.zeros((4, 2)))
    with pytest.raises(TypeError, match="registered device model"):          # a torch callable still gets no box
        models.InputBox(lambda x, u: x, -1.0, 1.0)
