"""CPU checks of models.TracedCost: the recording of cost callables (zopt_amd/tape.py with one output), its caps and refusals, the host
build of the cost interpreter (tests/tape_cost_shim.cpp around zopt_amd/csrc/tape_cost.h) against NumPy and the long-double / sympy
references, the NumPy restatement of the solve loops (tests/traced_cost_ref.py) against the oracle's, the decision that every start
of tests/traced_cost_cases.py is a fair comparison, and the C ABI's refusals of bad descriptors.

Values: costs without trigonometry are held bit for bit to the callable on float64 arrays; the interpreter's sine and cosine are
zm_sincos (trig.h), not libm's, so costs with them are held bit for bit to the NumPy evaluator of the tape on the host build of trig.h,
as tests/test_traced_model.py does.  A cost written with `@` is held to the operator-protocol evaluation (NumPy's float64 matmul is BLAS).

Derivative bound, per row (the gradient; each row of the Hessian): the larger of model_hp_ref.FLOOR (100 x 2^-52 of the row's largest
entry) and 100 x the error of the fp64 NumPy evaluation of the same expression against long double (dual numbers on the tape for
gradients, the lambdified sympy derivatives for Hessians).
"""
import ctypes

import numpy as np
import pytest

from oracle import zopt_oracle as zo
from tests import model_hp_ref as hp
from tests import tape_ref as R
from tests import traced_cost_cases as C
from tests import traced_cost_ref as TR
from tests import trig_host
from tests.test_traced_model import Boxed
from zopt_amd import ilqrUtils, models
from zopt_amd.pytrees import AffinePolicy, Trajectory

LD = np.longdouble
Q2, R1 = np.array([[2.0, 0.5], [0.5, 1.0]]), np.array([[0.3]])


def quad_at(x, u):
    return x @ Q2 @ x + u @ R1 @ u


def wide_cost(k):
    """(1, 1) cost with 2 inputs + k temporaries live at once (tests/tape_ref.py: wide_live), as a scalar"""
    f = R.wide_live(k)
    return lambda x, u: f(x, u)[0]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("tape_cost_shim")
    return TR.build(d), trig_host.build(d)


# ---- recording ----------------------------------------------------------------------------------------------------------------------
def test_recording_of_a_quadratic_form():
    c = models.TracedCost(quad_at, None, 2, 1)
    t = c.running_tape
    # x @ Q: 2 x (2 products + 1 sum); (x Q) @ x: 2 products + 1 sum; u @ R: 1 product; (u R) @ u: 1 product; the final sum
    assert len(t.code) == 12 and [op for op, *_ in t.decode()].count("mul") == 8
    assert sorted(t.consts) == [0.3, 0.5, 1.0, 2.0] and t.n_slots == 6 and t.outputs == (3,)
    assert t.mask == 0b111 and c.terminal_tape.mask == 0b011
    assert t.n == 2 and t.m == 1 and t.n_params == 0 and len(t.outputs) == 1
    peak, _ = R.liveness(t)
    assert peak == t.n_slots


def test_a_cost_affine_in_the_controls_has_no_control_bits():
    c = models.TracedCost(lambda x, u: np.cos(x[0]) * x[1] + 3.0 * u[0] - u[1], lambda x: x[0] * x[0], 2, 2)
    assert c.running_tape.mask == 0b0011 and c.terminal_tape.mask == 0b0001
    d = models.TracedCost(lambda x, u: x[0] * u[1], None, 2, 2)          # bilinear: state 0 and control 1
    assert d.running_tape.mask == 0b1001 and d.terminal_tape.mask == 0


def test_terminal_none_records_the_running_cost_at_zero_controls():
    c = models.TracedCost(lambda x, u: x[0] * x[0] + np.cos(u[0]) * x[1], None, 2, 1)
    x = np.random.default_rng(0).standard_normal((9, 2))
    got = R.evaluate(c.terminal_tape, x, np.full((9, 1), 123.0))[:, 0]             # (its control slot is never read)
    assert np.array_equal(got, x[:, 0] * x[:, 0] + np.cos(0.0) * x[:, 1])
    for op, _, (a_const, a), (b_const, b) in c.terminal_tape.decode():       # no instruction reads the control slot (slot 2)
        assert (a_const or a != 2) and (op not in ("add", "sub", "mul", "div") or b_const or b != 2)
    p = models.TracedCost(lambda x, u, p: (x[0] - p[0]) ** 2 + u[0] * u[0], None, 1, 1, params=np.array([[1.0], [2.0]]))
    assert np.array_equal(R.evaluate(p.terminal_tape, np.array([[3.0], [3.0]]), np.zeros((2, 1)), p.params)[:, 0], [4.0, 1.0])
    assert p.terminalCost(np.array([3.0]), np.array([2.0])) == 1.0 and p.runningCost(np.array([3.0]), np.array([2.0]), np.array([1.0])) == 8.0


def test_result_shapes_and_recorder_refusals():
    for good in (lambda x, u: x[0] * u[0], lambda x, u: np.array(x[0] * u[0]), lambda x, u: np.array([x[0] * u[0]]),
                 lambda x, u: np.array([[x[0]]]), lambda x, u: 3.0):
        assert len(models.TracedCost(good, lambda x: x[0], 1, 1).running_tape.outputs) == 1
    with pytest.raises(ValueError, match="returned 2 values"):
        models.TracedCost(lambda x, u: np.array([x[0], u[0]]), None, 1, 1)
    with pytest.raises(ValueError, match="returned 2 values"):
        models.TracedCost(lambda x, u: x[0], lambda x: x, 2, 1)
    with pytest.raises(TypeError, match="exp"):
        models.TracedCost(lambda x, u: np.exp(x[0]), None, 1, 1)
    with pytest.raises(TypeError, match="data-dependent branch"):
        models.TracedCost(lambda x, u: x[0] if x[0] > 0 else -x[0], None, 1, 1)
    with pytest.raises(TypeError, match="data-dependent branch"):
        models.TracedCost(lambda x, u: x[0], lambda x: abs(x[0]) if x[0] else x[0], 1, 1)
    with pytest.raises(TypeError, match="callable"):
        models.TracedCost(3.0, None, 1, 1)


def test_caps():
    assert models.TracedCost(wide_cost(62), lambda x: x[0], 1, 1).running_tape.n_slots == 64
    with pytest.raises(ValueError, match="64 slots"):
        models.TracedCost(wide_cost(63), lambda x: x[0], 1, 1)
    chain = lambda k: (lambda x, u: R.long_chain(k)(x, u)[0])            # noqa: E731
    assert len(models.TracedCost(chain(1024), lambda x: x[0], 1, 1).running_tape.code) == 1024
    with pytest.raises(ValueError, match="1025 instructions"):
        models.TracedCost(chain(1025), lambda x: x[0], 1, 1)
    with pytest.raises(ValueError, match="n=13"):
        models.TracedCost(lambda x, u: x[0], None, 13, 1)
    with pytest.raises(ValueError):
        models.TracedCost(lambda x, u: x[0], None, 2, 5)
    with pytest.raises(ValueError):
        models.TracedCost(lambda x, u, p: x[0], None, 2, 1, params=np.zeros(9))
    with pytest.raises(ValueError, match="constants"):
        models.TracedCost(lambda x, u: sum(x[0] * (1.0 + 0.001 * i) for i in range(300)), lambda x: x[0], 1, 1)


def test_record_keeps_its_old_signature():
    from zopt_amd import tape as T
    t = T.record(R.car, 4, 2)
    u = models.TracedModel(R.car, 4, 2).tape
    assert len(t.outputs) == 4 and np.array_equal(t.code, u.code) and np.array_equal(t.consts, u.consts) and t[2:] == u[2:]
    with pytest.raises(ValueError, match="the next state has n = 1"):
        T.record(lambda x, u: np.array([x[0], u[0]]), 1, 1)


def test_out_of_scope_combinations_are_refused_before_the_device():
    cost = models.TracedCost(quad_at, None, 2, 1)
    lin = models.LinearModel(np.eye(2), np.ones((2, 1)))
    x0, ug = np.zeros(2), np.zeros((5, 1))
    pol, prev = AffinePolicy(np.zeros((5, 1)), np.zeros((5, 1, 2))), Trajectory(np.zeros((6, 2)), np.zeros((5, 1)))
    box, sbox = models.InputBox(lin, -1.0, 1.0), models.StateBox(lin, -1.0, 1.0)
    cost12 = models.TracedCost(C.quad_running, C.quad_terminal, 12, 4)
    qbox = models.InputBox(models.QuadcopterEuler(0.1), -20.0, 20.0)
    with pytest.raises(TypeError, match="follow-up"):
        ilqrUtils.iterativeLqr(box, cost, cost, x0, ug)
    for solve in (ilqrUtils.iterativeLqr, ilqrUtils.differentialDynamicProgramming):
        with pytest.raises(TypeError, match="follow-up"):
            solve(qbox, cost12, cost12, np.zeros(12), np.zeros((5, 4)))
        with pytest.raises(TypeError, match="NumPy"):
            solve(lambda x, u: x + u, cost.runningCost, cost.terminalCost, x0, ug)
        with pytest.raises(TypeError, match=r"\(n=2, m=1\)"):
            solve(models.LinearModel(np.eye(3), np.ones((3, 1))), cost, cost, np.zeros(3), ug)
    with pytest.raises(TypeError, match="follow-up"):
        ilqrUtils.iterativeLqr(sbox, cost, cost, x0, ug)
    with pytest.raises(TypeError, match="follow-up"):
        ilqrUtils.constrainedIterativeLqr(sbox, cost, cost, x0, ug)
    with pytest.raises(TypeError, match="follow-up"):
        ilqrUtils.forwardPass2(x0, box, cost, pol, prev)
    with pytest.raises(TypeError, match="NumPy"):
        ilqrUtils.forwardPass2(x0, lambda x, u: x + u, cost, pol, prev)
    with pytest.raises(TypeError, match=r"\(n=2, m=1\)"):
        ilqrUtils.forwardPass2(np.zeros(4), models.TracedModel(R.car, 4, 2), cost, AffinePolicy(np.zeros((5, 2)), np.zeros((5, 2, 4))),
                               Trajectory(np.zeros((6, 4)), np.zeros((5, 2))))
    with pytest.raises(TypeError, match="same"):
        ilqrUtils.iterativeLqr(lin, cost.runningCost, models.TracedCost(quad_at, None, 2, 1).terminalCost, x0, ug)


# ---- host build against NumPy: values -------------------------------------------------------------------------------------------------
def _points(n, m, P=96, seed=5):
    rng = np.random.default_rng([seed, n, m])
    x, u = rng.standard_normal((P, n)) * 2.0, rng.standard_normal((P, m))
    x[P // 2:] += 2 * np.pi * rng.integers(-1000, 1001, (P - P // 2, n))            # many-turn angles
    x[0, 0], x[1, -1], x[2, 0] = np.nan, np.inf, -np.inf
    return x, u


def _case_points(case, P=96):
    x, u = _points(case.n, case.m, P)
    p = None
    if case.params is not None:
        rng = np.random.default_rng(9)
        p = rng.uniform(-3, 3, (P, case.params.shape[1]))
        p[P // 3: 2 * P // 3] += 1e6 * rng.choice([-1.0, 1.0], (2 * P // 3 - P // 3, p.shape[1]))       # goals 1e6 from the origin
    return x, u, p


@pytest.mark.parametrize("name", ["pendulum", "car", "quadcopter"])
def test_host_values_bit_for_bit(shim, name):
    lib, trig = shim
    case = C.by_name(name)
    x, u, p = _case_points(case)
    cost = models.TracedCost(case.running, case.terminal, case.n, case.m, params=p)
    sc = R.Real(np.float64, lambda a: trig_host.sincos(trig, a))
    with np.errstate(all="ignore"):
        for tape, uu, fn in ((cost.running_tape, u, case.running), (cost.terminal_tape, None, case.terminal)):
            got = TR.host_value(lib, tape, x, uu, p)
            want = R.evaluate(tape, x, np.zeros_like(u) if uu is None else uu, p, num=sc)[:, 0]
            assert np.array_equal(got, want, equal_nan=True)
            args = lambda i: ((x[i],) if uu is None else (x[i], uu[i])) + (() if p is None else (p[i],))      # noqa: E731
            direct = np.array([float(fn(*args(i))) for i in range(len(x))])
            assert np.array_equal(R.evaluate(tape, x, np.zeros_like(u) if uu is None else uu, p)[:, 0], direct, equal_nan=True)
            if name != "pendulum":                        # no sine or cosine: the callable on float64 arrays, bit for bit
                assert np.array_equal(got, direct, equal_nan=True)
    assert np.isnan(got[0]) and np.isfinite(got[3:]).all()


def test_host_values_of_a_cost_written_with_matmul(shim):
    lib, _ = shim
    cost = models.TracedCost(quad_at, None, 2, 1)
    x, u = _points(2, 1)
    box = lambda a: np.array([Boxed(v) for v in a] + [None], dtype=object)[:-1]          # noqa: E731
    with np.errstate(all="ignore"):
        want = np.array([quad_at(box(x[i]), box(u[i])).v for i in range(len(x))])
        assert np.array_equal(TR.host_value(lib, cost.running_tape, x, u), want, equal_nan=True)
        direct = np.array([quad_at(x[i], u[i]) for i in range(len(x))])
    fin = np.isfinite(direct)
    assert np.all(np.abs(want[fin] - direct[fin]) <= 8 * 2.0 ** -52 * np.maximum(1.0, np.abs(x[fin]).max(1) ** 2 * 4))


# ---- host build against the references: derivatives -----------------------------------------------------------------------------------
def _derivative_errors(case, cost, grad, hess, x, u, p):
    """worst ratio error / bound of (gradient, Hessian) for the running and the terminal cost; grad / hess: callables
    (tape, x, u | None, p) -> fp64 arrays"""
    out = []
    for tape, uu, fn, controls in ((cost.running_tape, u, case.running, True), (cost.terminal_tape, None, case.terminal, False)):
        K = case.n + case.m
        _, g_ld = TR.tape_gradient_ld(tape, x, uu, p)
        _, g_64 = TR.tape_gradient_ld(tape, x, uu, p, dtype=np.float64)
        sym = TR.SymbolicSecond(fn, case.n, case.m, 0 if p is None else p.shape[1], controls)
        H_ld, H_64 = sym(x, uu, p)[:, 0], sym(x, uu, p, dtype=np.float64)[:, 0]
        g, H = grad(tape, x, uu, p), hess(tape, x, uu, p)
        bg = hp.bound(hp.row_error(g_64[:, None, :], g_ld[:, None, :]))
        bH = hp.bound(hp.row_error(H_64, H_ld))
        eg, eH = hp.row_error(g[:, None, :], g_ld[:, None, :]), hp.row_error(H, H_ld)
        assert hp.finite_where_reference_is(g, g_ld) and hp.finite_where_reference_is(H, H_ld)
        S = sym.pattern()[0]                     # zero exactly where sympy's derivative is identically zero, nonzero elsewhere
        assert not H[:, ~S].any() and np.all((H != 0).any(0) == S), "the Hessian's nonzero pattern is sympy's"
        assert K == H.shape[-1]
        out.append((eg, bg, eH, bH))
    return out


@pytest.mark.parametrize("name", ["pendulum", "car", "quadcopter"])
def test_host_derivatives_against_long_double_and_sympy(shim, name):
    lib, _ = shim
    case = C.by_name(name)
    x, u, p = _case_points(case, P=48)
    x, u, p = x[3:], u[3:], (None if p is None else p[3:])          # (finite points: the references' derivatives exist)
    cost = models.TracedCost(case.running, case.terminal, case.n, case.m, params=p)
    res = _derivative_errors(case, cost, lambda *a: TR.host_gradient(lib, *a), lambda *a: TR.host_hessian(lib, *a), x, u, p)
    for (eg, bg, eH, bH), which in zip(res, ("running", "terminal")):
        print(f"{name} {which}: gradient {eg:.1e} (bound {bg:.1e})  Hessian {eH:.1e} (bound {bH:.1e})")
        assert eg <= bg and eH <= bH


# ---- the restatement is pinned ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ddp", [False, True], ids=["ilqr", "ddp"])
def test_restatement_reproduces_the_oracle_loop_for_a_quadratic_cost(ddp):
    """the quadratic cost written as a function: traced_cost_ref.solve against zo.iterativeLqr / zo.differentialDynamicProgramming,
    iterate by iterate -- same step indices, costs to 1e-12 relative"""
    Q, R_, Qf = np.diag([10.0, 1.0]), 0.1 * np.eye(1), np.diag([100.0, 10.0])
    run = lambda x, u: 10.0 * x[0] * x[0] + x[1] * x[1] + 0.1 * u[0] * u[0]          # noqa: E731
    term = lambda x: 100.0 * x[0] * x[0] + 10.0 * x[1] * x[1]                        # noqa: E731
    rc = TR.RefCost(models.TracedCost(run, term, 2, 1))
    qd = TR.symbolic_quadratic_dynamics(R.pendulum, 2, 1)
    for x0 in ([0.5, 0.0], [-1.0, 0.3], [2.5, -1.0]):
        ug = np.zeros((7, 1))
        tr, tro = [], []
        got = TR.solve(R.pendulum, rc, np.array(x0), ug, None, 30, 1e-6, ddp, qd, tr)
        if ddp:
            import torch
            ft = lambda x, u: torch.stack([x[0] + 0.05 * x[1], x[1] + 0.05 * (u[0] - 9.81 * torch.sin(x[0]))])      # noqa: E731
            want = zo.differentialDynamicProgramming(R.pendulum, ft, Q, R_, Qf, np.array(x0), ug, 30, 1e-6, True, tro)
        else:
            want = zo.iterativeLqr(R.pendulum, Q, R_, Qf, np.array(x0), ug, 30, 1e-6, True, tro)
        assert got[4] == want[4] and got[3] == want[3] and len(tr) == len(tro) >= 2
        for (J, i, _), (Jo, io, _) in zip(tr, tro):
            assert i == io and abs(J - Jo) <= 1e-12 * abs(Jo)


# ---- the solve cases are decided -------------------------------------------------------------------------------------------------------
def case_quadratic_dynamics(case):
    if case.name == "quadcopter":
        return lambda traj: zo.quadratic_dynamics_from_trajectory(zo.quad_euler_step_torch(0.1), traj)
    return TR.symbolic_quadratic_dynamics(case.step, case.n, case.m)


def test_solve_cases_are_decided():
    """for every start of every case, iLQR and DDP, the restatement alone: converges within maxIter; its two best line-search costs
    differ by more than DETERMINED (relative) in every iteration; and somewhere in the set a PD projection changes a Hessian"""
    import warnings
    any_projection = False
    for case in C.cases():
        rc = TR.RefCost(case.cost(models))
        qd = case_quadratic_dynamics(case)
        for ddp in (False, True):
            for i in range(len(case.x0)):
                tr, pr = [], []
                p = None if case.params is None else case.params[i]
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    _, _, J, conv, it = TR.solve(case.step, rc, case.x0[i], case.uGuess[i], p, case.maxIter, case.tol, ddp, qd, tr, pr)
                assert conv and 2 <= it < case.maxIter, (case.name, ddp, i, it)
                for _, _, Js in tr:
                    o = np.sort(Js)
                    assert np.all(np.isfinite(Js)) and o[1] - o[0] > hp.DETERMINED * abs(o[0]), (case.name, ddp, i, o[:3])
                any_projection |= any(pr)
    assert any_projection


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------------
def test_solve_argument_names_follow_the_header():
    """the record ilqrUtils fills is keyed by the header's parameter names, in order (as tests/test_abi.py holds SOLVE_ARGS)"""
    import os
    import re
    from zopt_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "zopt_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(_lib.TRACED_COST_SOLVE_ARGS) == ["zm_traced_cost_solve_f64", "zm_traced_cost_solve_trace_f64"]
    assert not any(k.startswith("zm_traced") for k in _lib.SOLVE_ARGS)
    for name, args in _lib.TRACED_COST_SOLVE_ARGS.items():
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        params = [re.search(r"(\w+)\s*$", p).group(1) for p in decl.group(1).split(",")]
        assert args == params and len(_lib.SYMBOLS[name][1]) == len(params), name


def test_c_abi_refuses_bad_descriptors_from_host_code():
    from zopt_amd import _lib
    lib = _lib.lib()
    cost = models.TracedCost(C.car_running, C.car_terminal, 4, 2, params=np.zeros(4))
    tr, tt = cost.running_tape, cost.terminal_tape
    assert ctypes.sizeof(models.zm_tracedcost_t) == 96 and ctypes.sizeof(models.zm_traced_t) == 40

    def descriptor():
        mk = lambda t: models.zm_traced_t(0x1000, 0x2000, 0, len(t.code), len(t.consts), t.n_slots, 4)        # noqa: E731
        return models.zm_tracedcost_t(mk(tr), mk(tt), 4, 2, tr.mask, tt.mask)
    d = 0x1000
    md = models.TracedModel(R.car, 4, 2)
    mt = md.tape
    model = models.zm_traced_model_t(models.ZM_MODEL_TRACED, 4, 2, mt.mask, 0.0, 0x1000, None, 0, len(mt.code), len(mt.consts), mt.n_slots, 0)
    pm = ctypes.addressof(model)

    def calls(st):
        ps = ctypes.addressof(st)
        return (lib.zm_traced_cost_linesearch_list_f64(pm, ps, d, d, d, d, d, d, 16, None, 0, None, d, d, d, None, 3, 5, None),
                lib.zm_traced_cost_expand_list_f64(ps, d, d, None, 0, None, d, d, d, d, d, d, d, d, d, 3, 5, None),
                lib.zm_traced_cost_solve_f64(pm, ps, d, d, 0, 5, 1e-3, 4, d, 1 << 40, d, d, d, d, d, d, None, 3, 5, None))
    good = descriptor()
    assert lib.zm_traced_cost_solve_workspace_f64(pm, ctypes.addressof(good), 8, 5, 0) > lib.zm_ilqr_solve_workspace_f64(pm, 8, 5, 0) > 0
    # the growth: the four shared Hessians become per-point arrays (pieces rounded up to an even count); a traced model has no
    # all-store block
    n, m, b, T = 4, 2, 8, 5
    even = lambda v: (v + 1) & ~1                                                      # noqa: E731
    grow = sum(even(v) for v in (b * T * n * n, b * T * m * n, b * T * m * m, b * n * n)) - sum(even(v) for v in (n * n, m * n, m * m, n * n))
    for ddp in (0, 1):
        assert lib.zm_traced_cost_solve_workspace_f64(pm, ctypes.addressof(good), b, T, ddp) - lib.zm_ilqr_solve_workspace_f64(pm, b, T, ddp) == grow
    for tape in ("running", "terminal"):
        for field, value in (("n_slots", 65), ("n_slots", 5), ("n_instr", 1025), ("n_const", 257), ("n_params", 9), ("tape", None),
                             ("tape", 0x1004), ("params", None), ("param_stride", -1)):
            bad = descriptor()
            setattr(getattr(bad, tape), field, value)
            for rc in calls(bad):
                assert rc in (_lib.ZM_EINVAL, _lib.ZM_EUNSUPPORTED), (tape, field)
                assert tape.encode() in lib.zm_last_error(), (tape, field)
    for field, value in (("n", 13), ("n", 0), ("m", 5), ("running_mask", 1 << 6), ("terminal_mask", 1 << 4)):
        bad = descriptor()
        setattr(bad, field, value)
        for rc in calls(bad):
            assert rc in (_lib.ZM_EINVAL, _lib.ZM_EUNSUPPORTED), field
    # the model's shape against the cost's; a null descriptor
    other = descriptor()
    other.n, other.m = 3, 2
    other.running.n_slots = other.terminal.n_slots = 20
    other.running_mask = other.terminal_mask = 0
    assert lib.zm_traced_cost_linesearch_list_f64(pm, ctypes.addressof(other), d, d, d, d, d, d, 16, None, 0, None, d, d, d, None, 3, 5,
                                                  None) == _lib.ZM_EINVAL
    assert lib.zm_traced_cost_solve_f64(pm, ctypes.addressof(other), d, d, 0, 5, 1e-3, 4, d, 1 << 40, d, d, d, d, d, d, None, 3, 5,
                                        None) == _lib.ZM_EINVAL
    assert lib.zm_traced_cost_expand_list_f64(None, d, d, None, 0, None, d, d, d, d, d, d, d, d, d, 3, 5, None) == _lib.ZM_EINVAL
    assert lib.zm_traced_cost_solve_workspace_f64(pm, None, 8, 5, 0) == -1
