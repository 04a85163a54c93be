"""CPU checks of models.TracedModel: the recorder (zopt_amd/tape.py), its caps and refusals, and the host build of the device
interpreter (tests/tape_shim.cpp around zopt_amd/csrc/tape_model.h) against the NumPy evaluator and the long-double references of
tests/model_hp_ref.py.

Bit-for-bit reference of the recording.  The callables without `@` (pendulum, car, cart-pole) are held to `f` called on float64
arrays.  The oracle's quadcopter forms three of its products with `@`; on float64 arrays NumPy hands those to BLAS, whose dot product
need not be the left-to-right unfused sum, while on the object arrays of the recording `@` IS that sum.  So the traced quadcopter is held
bit for bit to `f` called on float64 values that go through the same operator protocol as the recording (object arrays of `Boxed`
float64 scalars), rows 0..5 (no `@`) also to the float64-array call, and rows 6..11 to the float64-array call within 8 ulp of the
row's largest term (three-term dot products: 2 roundings of the sum + 3 of the products, either order, under 8 eps of the largest).
"""
import numpy as np
import pytest

from oracle import zopt_oracle as zo
from tests import model_hp_ref as hp
from tests import tape_ref as R
from tests import trig_host
from tests.tape_fuzz import Boxed            # (the operator-protocol float64; `**` is the recorder's product for k = 1..8)
from zopt_amd import models, tape as T

WIND = np.array([3.0, 1.0, 0.0])
FUNCS = {
    "quadcopter": (zo.quad_euler_step(0.1), 12, 4),
    "quadcopter+wind": ((lambda x, u: x + 0.1 * zo.quad_inertialDynamics(x, u, wind_ned=WIND)), 12, 4),
    "pendulum": (R.pendulum, 2, 1),
    "car": (R.car, 4, 2),
    "cartpole": (R.cartpole, 4, 1),
}


def boxed_call(f, x, u):
    box = lambda a: np.array([Boxed(v) for v in a] + [None], dtype=object)[:-1]          # noqa: E731
    return np.array([o.v if isinstance(o, Boxed) else o for o in f(box(x), box(u))], dtype=np.float64)


def points(n, m, P=64, seed=3):
    rng = np.random.default_rng([seed, n, m])
    x, u = rng.standard_normal((P, n)) * 2.0, rng.standard_normal((P, m))
    x[0, 0], x[1, -1], x[2, 0] = np.nan, np.inf, -np.inf
    return x, u


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("tape_shim")
    return R.build(d), trig_host.build(d)


# ---- recording ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FUNCS))
def test_recording_is_faithful(name):
    f, n, m = FUNCS[name]
    md = models.TracedModel(f, n, m)
    t = md.tape
    x, u = points(n, m)
    with np.errstate(all="ignore"):
        got = R.evaluate(t, x, u)
        direct = np.stack([f(x[i], u[i]) for i in range(len(x))])
        called = np.stack([md(x[i], u[i]) for i in range(len(x))])
    assert np.array_equal(called, direct, equal_nan=True)                    # calling the model evaluates f
    if "quadcopter" in name:
        with np.errstate(all="ignore"):
            boxed = np.stack([boxed_call(f, x[i], u[i]) for i in range(len(x))])
        assert np.array_equal(got, boxed, equal_nan=True)
        assert np.array_equal(got[:, :6], direct[:, :6], equal_nan=True)
        fin = np.isfinite(direct).all(1)
        scale = np.maximum(1.0, np.abs(x[fin]).max(1, keepdims=True) ** 2)
        assert np.all(np.abs(got[fin] - direct[fin]) <= 8 * 2.0 ** -52 * scale)
    else:
        assert np.array_equal(got, direct, equal_nan=True)
    # no slot is read before it is written, no instruction touches the pinned inputs, the outputs survive to the end
    peak, writer = R.liveness(t)
    assert peak == t.n_slots
    code = t.decode()
    for s in t.outputs:
        if s >= n + m:
            k = writer[s]
            assert all(c[1] != s for c in code[k + 1:]), "an output slot is overwritten after its value was formed"
    assert len(t.code) <= T.MAX_INSTR and t.n_slots <= T.MAX_SLOTS and len(t.consts) <= T.MAX_CONSTS
    print(f"{name}: {len(t.code)} instructions, {len(t.consts)} constants, {t.n_slots} slots, mask {t.mask:#x}")


def test_structural_masks():
    mask = {k: models.TracedModel(*FUNCS[k]).tape.mask for k in FUNCS}
    assert mask["quadcopter"] == 0x1FF and mask["quadcopter+wind"] == 0x1FF       # model_nonlinear_mask of the registered quadcopter
    assert mask["pendulum"] == 0x1
    assert mask["car"] == 0x1C and mask["car"] >> 4 & 1                            # heading, speed and the steering control
    assert mask["cartpole"] == 0x1A and mask["cartpole"] >> 4 & 1                  # angle, rate and the force
    assert models.TracedModel(lambda x, u: x + u, 3, 3).tape.mask == 0


def test_folding_sharing_dead_code_and_no_algebra():
    def f(x, u):
        dead = np.sin(x[0]) * 7.0                        # noqa: F841  never reaches an output
        a = (2.0 * 3.0) * x[0]                           # the product of the constants is folded
        b = np.cos(x[1]) + np.cos(x[1])                  # one cosine
        return np.array([a + 0.0 * u[0], b])             # 0.0 * u stays
    t = models.TracedModel(f, 2, 1).tape
    ops = [c[0] for c in t.decode()]
    assert ops.count("sin") == 0 and ops.count("cos") == 1
    assert 6.0 in t.consts and 2.0 not in t.consts and 3.0 not in t.consts
    assert ops.count("mul") == 2
    assert np.isnan(R.evaluate(t, np.array([[1.0, 2.0]]), np.array([[np.inf]]))[0, 0])     # 0.0 * inf: NaN, as the callable gives


def test_parameters_are_inputs_without_derivatives():
    md = models.TracedModel(R.pendulum_p, 2, 1, params=np.array([[0.5], [1.0], [2.0]]))
    assert md.n_params == 1 and md.tape.mask == 0x1
    x, u = np.array([[0.3, -0.2]] * 3), np.array([[0.1]] * 3)
    got = R.evaluate(md.tape, x, u, md.params)
    want = np.stack([R.pendulum_p(x[i], u[i], md.params[i]) for i in range(3)])
    assert np.array_equal(got, want)
    with pytest.raises(ValueError):
        md.c_struct()                                    # per-trajectory params need the batch of a call


# ---- at the caps ------------------------------------------------------------------------------------------------------------------
def test_slot_cap():
    t = models.TracedModel(R.wide_live(62), 1, 1).tape
    assert t.n_slots == 64 and R.liveness(t)[0] == 64
    x, u = points(1, 1)
    with np.errstate(all="ignore"):
        want = np.stack([R.wide_live(62)(x[i], u[i]) for i in range(len(x))])
    assert np.array_equal(R.evaluate(t, x, u), want, equal_nan=True)
    with pytest.raises(ValueError, match="64 slots"):
        models.TracedModel(R.wide_live(63), 1, 1)


def test_instruction_cap():
    t = models.TracedModel(R.long_chain(1024), 1, 1).tape
    assert len(t.code) == 1024
    x, u = points(1, 1)
    with np.errstate(all="ignore"):
        want = np.stack([R.long_chain(1024)(x[i], u[i]) for i in range(len(x))])
    assert np.array_equal(R.evaluate(t, x, u), want, equal_nan=True)
    with pytest.raises(ValueError, match="1025 instructions"):
        models.TracedModel(R.long_chain(1025), 1, 1)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals():
    with pytest.raises(TypeError, match="exp"):
        models.TracedModel(lambda x, u: np.exp(x), 1, 1)
    with pytest.raises(TypeError, match="data-dependent branch"):
        models.TracedModel(lambda x, u: x if x[0] > 0 else -x, 1, 1)
    with pytest.raises(TypeError, match="data-dependent branch"):
        models.TracedModel(lambda x, u: x if x[0] else -x, 1, 1)
    with pytest.raises(TypeError, match=r"\*\*"):
        models.TracedModel(lambda x, u: x ** 0.5, 1, 1)
    with pytest.raises(ValueError, match="returned 2 values"):
        models.TracedModel(lambda x, u: np.array([x[0], u[0]]), 1, 1)
    with pytest.raises(ValueError, match="n=13"):
        models.TracedModel(lambda x, u: x, 13, 1)
    with pytest.raises(ValueError):
        models.TracedModel(lambda x, u: x, 2, 5)
    with pytest.raises(ValueError):
        models.TracedModel(lambda x, u, p: x, 2, 1, params=np.zeros(9))


def test_out_of_scope_combinations_are_refused_before_the_device():
    from zopt_amd import ilqrUtils, mpcUtils
    from zopt_amd.pytrees import AffinePolicy, Trajectory
    md = models.TracedModel(R.car, 4, 2)
    with pytest.raises(TypeError, match="follow-up"):
        models.InputBox(md, -1.0, 1.0)
    with pytest.raises(TypeError, match="follow-up"):
        models.StateBox(md, -1.0, 1.0)
    track = models.TrackingCost(np.eye(4), np.eye(2), xRef=np.ones(4))
    x0, ug = np.zeros(4), np.zeros((5, 2))
    for solve in (ilqrUtils.iterativeLqr, ilqrUtils.differentialDynamicProgramming):
        with pytest.raises(TypeError, match="follow-up"):
            solve(md, track.runningCost, track.terminalCost, x0, ug)
    pol, prev = AffinePolicy(np.zeros((5, 2)), np.zeros((5, 2, 4))), Trajectory(np.zeros((6, 4)), np.zeros((5, 2)))
    with pytest.raises(TypeError, match="follow-up"):
        ilqrUtils.forwardPass2(x0, md, track, pol, prev)
    plan = Trajectory(np.zeros((6, 4)), np.zeros((5, 2)))
    with pytest.raises(TypeError, match="follow-up"):
        mpcUtils.ltvMpc.fromModel(md, plan, np.eye(4), np.eye(2), -np.ones(4), np.ones(4), -np.ones(2), np.ones(2))
    A, B = np.tile(np.eye(4), (5, 1, 1)), np.zeros((5, 4, 2))
    prob = mpcUtils.ltvMpc(A, B, np.eye(4), np.eye(2), 5, -np.ones(4), np.ones(4), -np.ones(2), np.ones(2))
    with pytest.raises(TypeError, match="follow-up"):
        prob.relinearize(md, plan)
    with pytest.raises(TypeError, match="follow-up"):
        prob.realTimeIteration(md, np.zeros(4), 2)


def test_c_abi_knows_the_kind_and_refuses_bad_descriptors():
    """host-only entry points: the mask and the (absent) pair table of a traced model; counts and pointers outside the caps"""
    import ctypes
    from zopt_amd import _lib
    lib = _lib.lib()
    t = models.TracedModel(R.car, 4, 2).tape
    st = models.zm_traced_model_t(models.ZM_MODEL_TRACED, 4, 2, t.mask, 0.0, 0x1000, None, 0, len(t.code), len(t.consts), t.n_slots, 0)
    mask, npairs = ctypes.c_uint32(0), ctypes.c_int32(-1)
    assert lib.zm_model_nonlinear_mask(ctypes.addressof(st), ctypes.addressof(mask)) == 0 and mask.value == 0x1C
    assert lib.zm_model_hessian_pairs(ctypes.addressof(st), None, ctypes.addressof(npairs)) == 0 and npairs.value == 0
    assert lib.zm_ilqr_solve_workspace_f64(ctypes.addressof(st), 8, 5, 1) > lib.zm_ilqr_solve_workspace_f64(ctypes.addressof(st), 8, 5, 0) > 0
    assert ctypes.sizeof(models.zm_traced_model_t) == ctypes.sizeof(models.zm_model_t) == 64
    for field, value in (("n_slots", 65), ("n_slots", 5), ("n_instr", 1025), ("n_const", 257), ("n_params", 9), ("tape", None),
                         ("tape", 0x1004), ("mask", 1 << 6), ("n", 13)):
        bad = models.zm_traced_model_t.from_buffer_copy(st)
        setattr(bad, field, value)
        rc = lib.zm_model_step_f64(ctypes.addressof(bad), 0x1000, 0x1000, 0x1000, 4, None)
        assert rc in (_lib.ZM_EINVAL, _lib.ZM_EUNSUPPORTED), field
        assert b"traced" in lib.zm_last_error(), field
    bad = models.zm_traced_model_t.from_buffer_copy(st)
    bad.n_params = 2                                      # parameters without a params pointer
    assert lib.zm_model_step_f64(ctypes.addressof(bad), 0x1000, 0x1000, 0x1000, 4, None) == _lib.ZM_EINVAL


# ---- host build of the interpreter ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FUNCS) + ["scalar11", "wide64"])
def test_host_interpreter_values_bit_for_bit(shim, name):
    f, n, m = FUNCS.get(name) or {"scalar11": (R.scalar11, 1, 1), "wide64": (R.wide_live(62), 1, 1)}[name]
    lib, trig = shim
    t = models.TracedModel(f, n, m).tape
    x, u = points(n, m, P=256)
    x[3:40] *= 1e3                                        # many-turn angles
    got = R.host_step(lib, t, x, u)
    want = R.evaluate(t, x, u, num=R.Real(np.float64, lambda a: trig_host.sincos(trig, a)))
    assert np.array_equal(got, want, equal_nan=True)      # NaN meets NaN
    assert np.isnan(got[0]).any() and np.isfinite(got[40:]).all()


def test_host_interpreter_parameters(shim):
    lib, trig = shim
    md = models.TracedModel(R.pendulum_p, 2, 1, params=np.linspace(0.5, 2.0, 7)[:, None])
    x, u = points(2, 1, P=7)
    sc = R.Real(np.float64, lambda a: trig_host.sincos(trig, a))
    assert np.array_equal(R.host_step(lib, md.tape, x, u, md.params), R.evaluate(md.tape, x, u, md.params, num=sc), equal_nan=True)
    assert np.array_equal(R.host_step(lib, md.tape, x, u, md.params[:1]), R.evaluate(md.tape, x, u, md.params[:1], num=sc), equal_nan=True)


@pytest.mark.parametrize("case", hp.CASES, ids=hp.case_id)
def test_host_interpreter_derivatives_on_the_hard_families(shim, case):
    """Dual and Hyper on the traced quadcopter (the oracle's own callable, with the case's wind) against the long-double / sympy
    reference, per output row, bound(oracle_error) = 100 x the fp64 oracle's own error with its floor -- model_hp_ref's rule."""
    lib, _ = shim
    fam, windy = case
    c = hp.expansion_case("inertial", fam, windy, 0.1)
    w = np.array(c.w, dtype=np.float64)
    t = models.TracedModel(lambda x, u: x + 0.1 * zo.quad_inertialDynamics(x, u, wind_ned=w), 12, 4).tape
    f, F = R.host_jacobian(lib, t, c.x, c.u)
    H = R.host_hessian(lib, t, c.x, c.u)
    e_f, e_F, e_H = hp.row_error(f, c.f, c.fscale), hp.row_error(F, c.F), hp.row_error(H, c.H)
    print(f"{hp.case_id(case)}: values {e_f:.1e} (bound {c.b_f:.1e})  Jacobians {e_F:.1e} ({c.b_F:.1e})  second {e_H:.1e} ({c.b_H:.1e})")
    assert hp.finite_where_reference_is(f, c.f) and hp.finite_where_reference_is(F, c.F) and hp.finite_where_reference_is(H, c.H)
    assert e_f <= c.b_f and e_F <= c.b_F and e_H <= c.b_H


def test_host_interpreter_derivatives_of_control_nonlinear_models(shim):
    """car and cart-pole: Dual against long-double dual numbers on the same tape, Hyper against sympy on the same expression; f_ux and
    f_uu are nonzero where sympy's are"""
    lib, _ = shim
    for f, n, m in (FUNCS["car"][:3], FUNCS["cartpole"][:3]):
        t = models.TracedModel(f, n, m).tape
        x, u = points(n, m, P=40)
        x, u = x[3:], 0.4 * u[3:]
        fh, Jh = R.host_jacobian(lib, t, x, u)
        fl, Jl = R.jacobian(t, x, u)
        assert hp.row_error(Jh, Jl) <= hp.FLOOR and hp.row_error(fh, fl) <= hp.FLOOR
        Hs = R.sympy_hessian(f, n, m, x, u)
        H = R.host_hessian(lib, t, x, u)
        assert hp.row_error(H, Hs) <= hp.FLOOR
        assert np.any(Hs[:, :, n:, :n] != 0) and (f is not R.car or np.any(Hs[:, :, n:, n:] != 0))   # (the cart-pole's f_uu is zero)
        assert np.array_equal(H[:, :, n:, :] != 0, Hs[:, :, n:, :] != 0)
