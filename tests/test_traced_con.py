"""CPU checks of models.TracedConstraint: the recording of constraint callables (zopt_amd/tape.py with n_con outputs), its caps and
refusals, the host build of the constraint interpreter (tests/tape_con_shim.cpp around zopt_amd/csrc/tape_con.h) against NumPy, the
NumPy restatement of the augmented-Lagrangian solve (tests/traced_con_ref.py) against the state box's restatement and against SciPy,
the hygiene of every case the GPU file compares exactly (tests/traced_con_cases.py), and the C ABI's refusals.  No GPU."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest

from oracle import zopt_oracle as zo
from tests import ilqr_state_cases as scases
from tests import ilqr_state_ref as sref
from tests import tape_ref as R
from tests import traced_con_cases as C
from tests import traced_con_ref as CR
from tests import trig_host
from zopt_amd import ilqrUtils, models
from zopt_amd.pytrees import AffinePolicy, Trajectory

INF = np.inf


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("tape_con_shim")
    return CR.build(d), trig_host.build(d)


def _lin():
    return models.LinearModel(C.DI["A"], C.DI["B"])


# ---- recording ----------------------------------------------------------------------------------------------------------------------
def test_recording_of_several_outputs_constants_and_a_terminal_only_constraint():
    con = C.constraint("car8")
    t = con.stage_tape
    assert len(t.outputs) == 8 and t.n == 4 and t.m == 2 and t.n_params == 3 and con.terminal_tape is None and con.n_con_terminal == 0
    assert len(set(t.outputs)) == 8 and min(t.outputs) >= 4 + 2 + 3              # every row in a slot of its own, behind the inputs
    peak, _ = R.liveness(t)
    assert peak == t.n_slots <= 64
    # a row that is a constant, a row that is an input itself, and the same expression twice
    k = models.TracedConstraint(_lin(), lambda x, u: np.array([-1.0, x[0], u[0] - 2.0, u[0] - 2.0]), 4)
    assert len(k.stage_tape.outputs) == 4 and k.stage_tape.outputs[1] == 0 and k.stage_tape.outputs[2] == k.stage_tape.outputs[3]
    assert np.array_equal(R.evaluate(k.stage_tape, np.array([[0.5, 7.0]]), np.array([[3.0]]))[0], [-1.0, 0.5, 1.0, 1.0])
    # g = None: a terminal set only; its tape keeps the control slot reserved and unread
    tt = models.TracedConstraint(_lin(), None, 0, C.terminal_band, 3)
    assert tt.n_con == 0 and tt.stage_tape is None and len(tt.terminal_tape.outputs) == 3
    for op, dst, (ac, a), (bc, b) in tt.terminal_tape.decode():
        assert (ac or a != 2) and (bc or b != 2 or op in ("neg", "sin", "cos", "tan", "sqrt", "mov")) and dst > 2
    # the handle evaluates its callables on numbers
    assert np.array_equal(C.constraint("lin21_T9").g(np.array([1.0, 2.0]), np.array([0.0])), [0.3 + 2.0 - 0.7])
    assert tt.terminal(np.array([-0.5, 0.0])).shape == (3,)


def test_caps_are_value_errors_that_name_the_cap():
    g9 = lambda x, u: np.array([x[0]] * 9)                                        # noqa: E731
    with pytest.raises(ValueError, match="n_con <= 8"):
        models.TracedConstraint(_lin(), g9, 9)
    with pytest.raises(ValueError, match="n_con_terminal <= 8"):
        models.TracedConstraint(_lin(), None, 0, lambda x: np.array([x[0]] * 9), 9)
    with pytest.raises(ValueError, match="expected 2"):
        models.TracedConstraint(_lin(), C.halfplane, 2)
    with pytest.raises(ValueError, match="give g, terminal"):
        models.TracedConstraint(_lin(), None, 0)
    with pytest.raises(ValueError, match="1 <= n <= 12"):
        models.TracedConstraint(models.LinearModel(np.eye(13), np.ones((13, 1))), lambda x, u: np.array([x[0]]), 1)
    with pytest.raises(ValueError, match="params <= 8"):
        models.TracedConstraint(_lin(), lambda x, u, p: np.array([x[0] - p[0]]), 1, params=np.zeros(9))
    with pytest.raises(ValueError, match="instructions"):
        models.TracedConstraint(models.LinearModel(np.eye(1), np.ones((1, 1))), lambda x, u: np.array([R.long_chain(1025)(x, u)[0]]), 1)
    with pytest.raises(ValueError, match="slots"):
        models.TracedConstraint(models.LinearModel(np.eye(1), np.ones((1, 1))), lambda x, u: np.array([R.wide_live(63)(x, u)[0]]), 1)
    with pytest.raises(ValueError, match="mu0 > 0"):
        models.TracedConstraint(_lin(), C.halfplane, 1, mu0=0.0)
    with pytest.raises(TypeError, match="branch"):
        models.TracedConstraint(_lin(), lambda x, u: np.array([x[0] if x[0] > 0 else -x[0]]), 1)


def test_refusals_name_the_follow_up_before_anything_touches_the_device():
    lin = _lin()
    con = C.constraint("lin21_T9")
    cost = models.QuadraticCost(C.DI["Q"], C.DI["R"], C.DI["Qf"])
    x0, ug = C.DI["x0"], np.zeros((9, 1))
    with pytest.raises(ValueError, match="follow-up"):
        ilqrUtils.differentialDynamicProgramming(con, cost, cost, x0, ug)
    with pytest.raises(ValueError, match="follow-up"):
        ilqrUtils.forwardPass2(x0, con, cost, AffinePolicy(ug, np.zeros((9, 1, 2))), Trajectory(np.zeros((10, 2)), ug))
    tc = models.TracedCost(lambda x, u: x @ x + u @ u, None, 2, 1)
    with pytest.raises(TypeError, match="follow-up"):
        ilqrUtils.iterativeLqr(con, tc, tc, x0, ug)
    with pytest.raises(TypeError, match="follow-up"):
        ilqrUtils.constrainedIterativeLqr(con, tc.runningCost, tc.terminalCost, x0, ug)
    for wrap in (lambda: models.InputBox(con, -1.0, 1.0), lambda: models.StateBox(con, -1.0, 1.0),
                 lambda: models.TracedConstraint(models.InputBox(lin, -1.0, 1.0), C.halfplane, 1),
                 lambda: models.TracedConstraint(models.StateBox(lin, -1.0, 1.0), C.halfplane, 1),
                 lambda: models.TracedConstraint(con, C.halfplane, 1),
                 lambda: models.TracedConstraint(lambda x, u: x + u, C.halfplane, 1)):
        with pytest.raises(TypeError, match="follow-up"):
            wrap()
    # what existing tests pin stays: the boxes still refuse a traced model, a bare model still names StateBox
    tm = models.TracedModel(R.pendulum, 2, 1)
    for box in (lambda: models.InputBox(tm, -1.0, 1.0), lambda: models.StateBox(tm, -1.0, 1.0)):
        with pytest.raises(TypeError):
            box()
    with pytest.raises(TypeError, match="StateBox"):
        ilqrUtils.constrainedIterativeLqr(lin, cost, cost, x0, ug)
    assert [f for f, _ in models.zm_statebox_t._fields_] == ["lb", "ub", "stride", "lam_lb", "lam_ub", "mu"]
    # a TracedModel takes a QuadraticCost only; shapes are checked on the host
    pend = C.constraint("pendulum")
    with pytest.raises(TypeError, match="follow-up"):
        ilqrUtils.iterativeLqr(pend, *(2 * (models.TrackingCost(np.eye(2), np.eye(1), xRef=np.ones(2)),)), np.zeros(2), np.zeros((4, 1)))
    with pytest.raises(ValueError, match="do not match"):
        ilqrUtils.iterativeLqr(con, cost, cost, np.zeros(3), ug)


# ---- host build against NumPy ---------------------------------------------------------------------------------------------------------
def _points(c, P=64, seed=5):
    rng = np.random.default_rng([seed, c.n, c.m])
    x, u = rng.standard_normal((P, c.n)) * 2.0, rng.standard_normal((P, c.m))
    x[0, 0], x[1, -1], x[2, 0] = np.nan, np.inf, -np.inf
    p = None if c.params is None else rng.uniform(-3, 3, (P, c.params.shape[1]))
    return x, u, p


@pytest.mark.parametrize("name", C.NAMES)
def test_host_values_bit_for_bit(shim, name):
    """the host build of the interpreter on the constraint tapes equals NumPy evaluation of g bit for bit: the callable itself on
    float64 arrays where it has no sine or cosine, the NumPy evaluator of the tape on the host build of trig.h where it has"""
    lib, trig = shim
    c = C.by_name(name)
    x, u, p = _points(c)
    con = models.TracedConstraint(c.model(), c.g, c.n_con, c.terminal, c.n_con_terminal, params=p)
    sc = R.Real(np.float64, lambda a: trig_host.sincos(trig, a))
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for tape, uu, fn in ((con.stage_tape, u, c.g), (con.terminal_tape, None, c.terminal)):
            if tape is None:
                continue
            got = CR.host_value(lib, tape, x, uu, p)
            want = R.evaluate(tape, x, np.zeros_like(u) if uu is None else uu, p, num=sc)
            assert got.shape == want.shape == (len(x), len(tape.outputs)) and np.array_equal(got, want, equal_nan=True)
            if name != "quadcopter":
                args = lambda i: ((x[i],) if uu is None else (x[i], uu[i])) + (() if p is None else (p[i],))      # noqa: E731
                direct = np.stack([np.asarray(fn(*args(i)), dtype=np.float64) for i in range(len(x))])
                assert np.array_equal(got, direct, equal_nan=True)
            # the Dual build's values are the double build's, its derivatives the NumPy dual numbers' on float64 to a few ulp
            G = CR.host_jacobian(lib, tape, x[3:], None if uu is None else uu[3:], None if p is None else p[3:])
            Gn = R.jacobian(tape, x[3:], np.zeros_like(u[3:]) if uu is None else uu[3:], None if p is None else p[3:], np.float64)[1]
            assert np.max(np.abs(G - Gn)) <= 64 * 2.0 ** -52 * max(1.0, np.max(np.abs(Gn)))


def test_host_psi_is_the_numpy_penalty_term(shim):
    lib, _ = shim
    rng = np.random.default_rng(1)
    g = rng.standard_normal(500) * 10.0 ** rng.uniform(-3, 3, 500)
    lam = np.where(rng.random(500) < 0.3, 0.0, 10.0 ** rng.uniform(-2, 6, 500))
    mu = 10.0 ** rng.uniform(0, 8, 500)
    g[:3] = [np.nan, np.inf, -np.inf]
    with np.errstate(all="ignore"):
        p = CR.pos(lam + mu * g)
        want = (p * p - lam * lam) / (2.0 * mu)
    assert np.array_equal(CR.host_psi(lib, g, lam, mu), want, equal_nan=True)
    # ... and the restatement's accumulator is that sum in order
    G, L = g[3:11].reshape(4, 2), lam[3:11].reshape(4, 2)
    acc = 0.0
    for v in CR.host_psi(lib, G, L, mu[3]).ravel():
        acc = acc + v
    assert CR.penalty(G, np.zeros(0), L, np.zeros(0), mu[3]) == acc


# ---- the restatement against the state box's and against SciPy ---------------------------------------------------------------------------
def _box_rows(lb, ub):
    fu, fl = np.flatnonzero(np.isfinite(ub)), np.flatnonzero(np.isfinite(lb))
    return (lambda x, u=None: np.array([x[i] - ub[i] for i in fu] + [lb[i] - x[i] for i in fl])), len(fu) + len(fl), fu, fl


@pytest.mark.parametrize("name,scale", [("dint", 1.0), ("stable5", 0.3), ("unstable12", 0.3)])
def test_restatement_on_a_box_written_as_g_is_the_state_box_restatement(name, scale):
    """g = [x - ub; lb - x] on the stages and on the terminal state is the state box on k = 1..T when x_0 is strictly inside: the same
    outer and inner counts, the same step indices, values to 1e-9"""
    p = scases.qp_problem(name)
    n, m = p["B"].shape
    rows, nc, fu, fl = _box_rows(p["x_lb"], p["x_ub"])
    x0 = scale * p["x0"]                                                           # (scaled until it is strictly inside the box)
    assert np.all(rows(x0) < 0)
    model = models.LinearModel(p["A"], p["B"])
    con = models.TracedConstraint(model, lambda x, u: rows(x), nc, lambda x: rows(x), nc, outer=scases.LOOSE["outer"], ctol=scases.LOOSE["ctol"])
    dyn = lambda x, u: p["A"] @ x + p["B"] @ u                                     # noqa: E731
    tr = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        o = CR.constrainedIterativeLqr(dyn, p["Q"], p["R"], p["Qf"], x0, np.zeros((p["T"], m)), con, maxIter=scases.LOOSE["maxIter"],
                                       tol=scases.LOOSE["tol"], trace=tr)
        ts = []
        s = sref.constrainedIterativeLqr(dyn, p["Q"], p["R"], p["Qf"], x0, np.zeros((p["T"], m)), p["x_lb"], p["x_ub"], trace=ts, **scases.LOOSE)
        s["trace"] = ts
    assert o["converged"] == s["converged"] and o["outer"] == s["outer"] and o["inner"] == s["inner"]
    for a, b in zip(tr, s["trace"]):
        assert abs(a["violation"] - b["violation"]) <= 1e-9 * max(1.0, abs(b["violation"])) and a["mu"] == b["mu"]
        for ia, ib in zip(a["inner"], b["inner"]):
            srt = np.sort(ib["Js"])
            if srt[1] - srt[0] >= 1e-9 * abs(srt[0]):
                assert ia["idx"] == ib["idx"]
            assert abs(ia["J"] - ib["J"]) <= 1e-9 * abs(ib["J"]) and abs(ia["Jcost"] - ib["Jcost"]) <= 1e-9 * abs(ib["Jcost"])
    assert abs(o["J"] - s["J"]) <= 1e-9 * abs(s["J"]) and abs(o["violation"] - s["violation"]) <= 1e-9
    assert np.max(np.abs(o["traj"].uTraj - s["traj"].uTraj)) <= 1e-9 * max(1.0, np.max(np.abs(s["traj"].uTraj)))
    # the multipliers: stage k of g is row k of the box (k >= 1), the terminal rows are row T
    lam_box = np.concatenate([s["lam_ub"][:, fu], s["lam_lb"][:, fl]], axis=1)
    scale = max(1.0, np.max(np.abs(lam_box)))
    assert np.max(np.abs(o["lam"][1:] - lam_box[1:-1])) <= 1e-9 * scale and np.max(np.abs(o["lam_terminal"] - lam_box[-1])) <= 1e-9 * scale
    assert not o["lam"][0].any()


@pytest.mark.parametrize("which", ["stage", "mixed"])
def test_restatement_against_scipy_on_half_planes(which):
    """a linear model with half-plane constraints is a convex QP: with tight settings the restatement is done, feasible to ctol, and its
    inputs are SciPy's (SLSQP on the condensed problem from u = 0) to 1e-5"""
    from scipy.optimize import minimize
    p = dict(C.DI)
    T, n, m = 12, 2, 1
    p["T"] = T
    Sx, Su, H, f = scases.condensed(p)
    a, bb, cu = C.HP_A, C.HP_B, (0.4 if which == "mixed" else 0.0)                # a'x + cu u <= b on (x_k, u_k), k = 0..T-1; a'x_T <= b
    g = (lambda x, u: np.array([a[0] * x[0] + a[1] * x[1] + cu * u[0] - bb]))
    con = models.TracedConstraint(models.LinearModel(p["A"], p["B"]), g, 1, lambda x: np.array([a[0] * x[0] + a[1] * x[1] - bb]), 1,
                                  outer=20, ctol=1e-8)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        o = CR.constrainedIterativeLqr(lambda x, u: p["A"] @ x + p["B"] @ u, p["Q"], p["R"], p["Qf"], p["x0"], np.zeros((T, m)), con,
                                       maxIter=100, tol=1e-10)
    assert o["converged"] and o["violation"] <= 1e-8 and np.all(o["lam"] >= 0) and np.all(o["lam_terminal"] >= 0)
    assert (o["lam"] > 0).sum() + (o["lam_terminal"] > 0).sum() >= 1                # the constraint binds somewhere
    c0 = Sx @ p["x0"]
    X = lambda uu: np.concatenate([p["x0"], c0 + Su @ uu]).reshape(T + 1, n)      # noqa: E731

    def margin(uu):                                                                # >= 0 when feasible
        x = X(uu)
        return np.concatenate([bb - x[:T] @ a - cu * uu, [bb - x[T] @ a]])
    res = None
    for ftol in (1e-14, 1e-12, 1e-10):
        res = minimize(lambda uu: uu @ H @ uu + 2 * f @ uu, np.zeros(T * m), jac=lambda uu: 2 * (H @ uu + f), method="SLSQP",
                       constraints=[dict(type="ineq", fun=margin)], options=dict(ftol=ftol, maxiter=2000))
        if res.success:
            break
    assert res.success, res.message
    dist = float(np.max(np.abs(o["traj"].uTraj.ravel() - res.x)))
    print(f"half-planes ({which}): outer {o['outer']} inner {o['inner']} violation {o['violation']:.2e} distance to SciPy {dist:.2e}")
    assert dist <= 1e-5


# ---- the cases of the GPU file -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.NAMES)
def test_case_hygiene(name):
    """every solve case the GPU file compares exactly, on the restatement alone: in every iteration the best two of the 16 costs are at
    least 1e-9 apart, relative; the inner test |dJ| - tol and the outer test viol - ctol are 1e-6 relative away from zero.  A case
    that fails is replaced in tests/traced_con_cases.py, not skipped on the device."""
    c = C.by_name(name)
    con = C.constraint(name)
    assert C.NAMES == tuple(k.name for k in C.cases())
    for b in range(c.x0.shape[0]):
        o = C.restatement(name, b)
        assert CR.min_gap(o) >= 1e-9, (name, b, CR.min_gap(o))
        for out in o["trace"]:
            assert abs(out["violation"] - con.ctol) >= 1e-6 * con.ctol, (name, b)
            for it in out["inner"]:
                assert np.all(np.isfinite(it["Js"])) and abs(it["dJ"] - c.tol) >= 1e-6 * c.tol, (name, b, it["dJ"])
    if name == "car":
        done = [C.restatement(name, b)["converged"] for b in range(5)]
        assert done[2] and C.restatement(name, 2)["outer"] == 1 and not C.restatement(name, 2)["lam"].any()      # never active
        assert not done[3] and C.restatement(name, 3)["outer"] == con.outer                                    # the start is inside
        assert any(done[b] and C.restatement(name, b)["lam"].any() for b in (0, 1, 4))                         # active and done
    if name == "quadcopter":
        for b in range(3):
            lam = C.restatement(name, b)["lam"]
            assert lam[:, 0].any() and lam[:, 1].any(), (b, "the sphere and the tilt limit both bind")


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------------
def test_solve_argument_names_follow_the_header():
    from zopt_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "zopt_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(_lib.TRACED_CON_SOLVE_ARGS) == ["zm_traced_con_solve_f64", "zm_traced_con_solve_trace_f64"]
    for name, args in _lib.TRACED_CON_SOLVE_ARGS.items():
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        params = [re.search(r"(\w+)\s*$", p).group(1) for p in decl.group(1).split(",")]
        assert args == params and len(_lib.SYMBOLS[name][1]) == len(params), name
    assert ctypes.sizeof(models.zm_tracedcon_t) == 120


def test_c_abi_refuses_bad_arguments_from_host_code():
    """null pointers, bad sizes, ddp = 1 and tapes outside the caps on dummy pointers: each is refused before any launch (a launch
    would fault on these pointers, or fail for want of a device)"""
    from zopt_amd import _lib
    lib = _lib.lib()
    con = C.constraint("car8")
    t = con.stage_tape
    d = 0x1000

    def descriptor(nc=8, nct=0):
        mk = lambda k: models.zm_traced_t(0x1000, 0x2000, 0, len(t.code), len(t.consts), t.n_slots, 3) if k else models.zm_traced_t(None, None, 0, 0, 0, 0, 0)    # noqa: E731
        return models.zm_tracedcon_t(mk(nc), mk(nct), 4, 2, nc, nct, d, d, d)
    md = models.TracedModel(R.car, 4, 2)
    mt = md.tape
    model = models.zm_traced_model_t(models.ZM_MODEL_TRACED, 4, 2, mt.mask, 0.0, 0x1000, None, 0, len(mt.code), len(mt.consts), mt.n_slots, 0)
    pm = ctypes.addressof(model)
    qc = models.zm_quadcost_t(d, d, d, 0, 0)
    pq = ctypes.addressof(qc)
    ws = 1 << 40

    def solve(ps, model=pm, cost=pq, track=None, ddp=0, batch=3, T=5, outer=10, mu0=1.0, x0=d, viol=d, workspace=ws, max_iter=5):
        return lib.zm_traced_con_solve_f64(model, cost, track, ps, mu0, 10.0, 1e8, outer, 1e-4, x0, d, ddp, max_iter, 1e-3, 4, d, workspace, d,
                                           d, d, d, d, d, viol, d, d, None, batch, T, None)

    def calls(st):
        ps = ctypes.addressof(st)
        return (lib.zm_traced_con_values_f64(ps, d, d, d, d, 3, 5, None),
                lib.zm_traced_con_linesearch_list_f64(pm, pq, None, ps, d, d, d, d, d, d, 16, None, 0, None, d, d, d, d, d, 3, 5, None),
                lib.zm_traced_con_expand_list_f64(ps, d, d, None, 0, None, d, d, d, d, d, d, d, d, d, d, d, 3, 5, None),
                lib.zm_traced_con_multiplier_update_f64(ps, d, d, d, d, d, None, None, 1e-4, 10.0, 1e8, 1, 3, 5, None),
                solve(ps))
    good = descriptor()
    pg = ctypes.addressof(good)
    assert lib.zm_traced_con_solve_workspace_f64(pm, 8, 5) > lib.zm_traced_cost_solve_workspace_f64(pm, pg, 8, 5, 0) > 0
    assert lib.zm_traced_con_solve_workspace_f64(None, 8, 5) == -1 and lib.zm_traced_con_solve_workspace_f64(pm, 8, 0) == -1
    for tape in ("stage",):
        for field, value in (("n_slots", 65), ("n_slots", 5), ("n_instr", 1025), ("n_const", 257), ("n_params", 9), ("tape", None),
                             ("tape", 0x1004), ("params", None), ("param_stride", -1)):
            bad = descriptor()
            setattr(getattr(bad, tape), field, value)
            for rc in calls(bad):
                assert rc in (_lib.ZM_EINVAL, _lib.ZM_EUNSUPPORTED), (tape, field)
                assert tape.encode() in lib.zm_last_error(), (tape, field)
    bad = descriptor(0, 3)
    bad.terminal.n_instr = 1025
    assert all(rc == _lib.ZM_EUNSUPPORTED for rc in calls(bad)) and b"terminal" in lib.zm_last_error()
    for field, value in (("n", 13), ("n", 0), ("m", 5), ("n_con", 9), ("n_con", -1), ("n_con_terminal", 9)):
        bad = descriptor()
        setattr(bad, field, value)
        for rc in calls(bad):
            assert rc in (_lib.ZM_EINVAL, _lib.ZM_EUNSUPPORTED), field
    none = descriptor(0, 0)
    assert all(rc == _lib.ZM_EINVAL for rc in calls(none))
    for field in ("lam", "mu"):                      # the entries that read the multipliers need them
        bad = descriptor()
        setattr(bad, field, None)
        assert all(rc == _lib.ZM_EINVAL for rc in calls(bad)[1:]), field
    # the solve: null pointers, sizes, ddp, settings, the workspace, the cost, the model's shape
    assert solve(None) == _lib.ZM_EINVAL and solve(pg, x0=None) == _lib.ZM_EINVAL and solve(pg, viol=None) == _lib.ZM_EINVAL
    assert solve(pg, model=None) == _lib.ZM_EINVAL
    assert solve(pg, ddp=1) == _lib.ZM_EUNSUPPORTED and b"DDP" in lib.zm_last_error()
    assert solve(pg, T=0) == _lib.ZM_EINVAL and solve(pg, batch=-1) == _lib.ZM_EINVAL and solve(pg, max_iter=-1) == _lib.ZM_EINVAL
    assert solve(pg, outer=0) == _lib.ZM_EINVAL and solve(pg, mu0=0.0) == _lib.ZM_EINVAL
    assert solve(pg, workspace=10) == _lib.ZM_EINVAL and b"workspace" in lib.zm_last_error()
    assert solve(pg, cost=None) == _lib.ZM_EINVAL and solve(pg, track=pq) == _lib.ZM_EINVAL
    tk = models.zm_trackcost_t(d, d, d, 0, 0, None, None, 0, 0, 0, 0)
    assert solve(pg, cost=None, track=ctypes.addressof(tk)) == _lib.ZM_EUNSUPPORTED       # a traced model takes a zm_quadcost_t
    other = descriptor()
    other.n = 3
    assert solve(ctypes.addressof(other)) == _lib.ZM_EINVAL
    assert solve(pg, batch=0) == _lib.ZM_OK                                                 # nothing to do
    # the array-level entries: null operands and bad sizes
    assert lib.zm_traced_con_values_f64(pg, None, d, d, d, 3, 5, None) == _lib.ZM_EINVAL
    assert lib.zm_traced_con_values_f64(pg, d, d, d, d, 3, 0, None) == _lib.ZM_EINVAL
    assert lib.zm_traced_con_linesearch_list_f64(pm, pq, None, pg, d, d, d, d, d, d, 5, None, 0, None, d, d, d, d, d, 3, 5, None) == _lib.ZM_EINVAL
    assert lib.zm_traced_con_linesearch_list_f64(pm, pq, None, pg, d, d, d, d, d, d, 16, d, 4, None, d, d, d, d, d, 3, 5, None) == _lib.ZM_EINVAL
    assert lib.zm_traced_con_expand_list_f64(pg, d, d, None, 0, None, d, d, d, None, d, d, d, d, d, d, d, 3, 5, None) == _lib.ZM_EINVAL
    assert lib.zm_traced_con_multiplier_update_f64(pg, d, d, None, d, d, None, None, 1e-4, 10.0, 1e8, 1, 3, 5, None) == _lib.ZM_EINVAL
    assert lib.zm_traced_con_multiplier_update_f64(pg, d, d, d, d, d, None, None, 1e-4, 0.5, 1e8, 1, 3, 5, None) == _lib.ZM_EINVAL
