"""GPU tests that pin riccati_ode_kernel (finiteHorizonLqr) step by step against its NumPy restatement, tests/riccati_ode_ref.py.

The global error against a tight DOP853 integration (tests/test_continuous_lqr_gpu.py, 2e-6) cannot see a wrong coefficient of the
embedded error estimate, a wrong first-step rule, wrong controller clamps, a wrong divisor in the RMS norm or a broken "clipped step
keeps h" rule: the controller would take other steps and still control the local error.  The number of attempted steps (`K.info`)
can: every one of those changes the step sequence.  The cases are admitted by tests/test_riccati_ode_ref.py (the fp64 and the
long-double restatement take the same steps, no accept / reject decision is closer than 1e-3 to err = 1), so that the kernel's fma
contraction and the summation order of its 16-wide products cannot legitimately change the count; the value bound
max(1e-12, 100 x delta_case) x max|V| is built from delta_case, the fp64-vs-long-double deviation of the restatement itself.

Measured on an MI355X (profiles/care_hard_spectrum.txt): the step counts are equal in all 12 cases and at all 3 tolerances, V deviates
by 2e-16 ... 2e-11 (stiff_12x4, bound 3e-9), 1.5 % of its bound at the most (large_Qf_8x2: 7.5e-13 against 5.1e-11).
With the coefficient e5 of the error estimate off by 6.8e-6 every case fails on its step count (231 against 59 steps at 16 x 16)
although V moves by no more than 1.4e-7, far inside the 2e-6 of the DOP853 check."""
import numpy as np
import pytest

from oracle import zopt_oracle as zo
from tests import riccati_ode_ref as rr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lqr():
    import torch
    assert torch.cuda.is_available()
    from zopt_amd import lqrUtils
    return lqrUtils


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def _run(lqr, name, **kw):
    c = rr.case(name)
    K = lqr.finiteHorizonLqr(c["A"], c["B"], c["Q"], c["R_inv"], c["Qf"], c["T"], N=c["N"], n_samples=c["ns"], **kw)
    assert K.n_samples == c["ns"]        # the kernel saw exactly the samples the restatement takes
    return c, K


@pytest.mark.parametrize("name", sorted(rr.CASES))
def test_step_count_and_values_match_the_restatement(lqr, name):
    c, K = _run(lqr, name)
    ref = rr.runs(name)
    delta = rr.delta_case(name)
    bound = max(1e-12, 100 * delta)
    steps = [r.steps for r in ref]
    dev = [_rel(K.V[b], r.V) for b, r in enumerate(ref)]
    print(f"{name}: steps kernel {np.asarray(K.info).tolist()} restatement {steps} (rejected {[r.rejected for r in ref]})  "
          f"max|V - V_ref|/max|V| {max(dev):.1e}  bound {bound:.1e} (delta_case {delta:.1e})")
    assert np.asarray(K.info).tolist() == steps
    assert max(dev) <= bound
    for b in range(len(ref)):
        pick = lambda f: (lambda t: f(t)[b])        # noqa: E731
        _, _, Vr = zo.finiteHorizonLqr(pick(c["A"]), pick(c["B"]), pick(c["Q"]), pick(c["R_inv"]), c["Qf"][b], c["T"], N=c["N"])
        assert _rel(K.V[b], Vr) <= 2e-6


def test_tolerance_is_honoured(lqr):
    """rtol = atol in {1e-6, 1e-8, 1e-10}: the restatement's step count at each setting, and an error against the 1e-12 DOP853
    integration that decreases monotonically"""
    name = rr.TOLERANCE_CASE
    c = rr.case(name)
    Vr = []
    for b in range(c["Qf"].shape[0]):
        pick = lambda f: (lambda t: f(t)[b])        # noqa: E731
        Vr.append(zo.finiteHorizonLqr(pick(c["A"]), pick(c["B"]), pick(c["Q"]), pick(c["R_inv"]), c["Qf"][b], c["T"], N=c["N"])[2])
    errs = []
    for tol in rr.TOLERANCES:
        _, K = _run(lqr, name, rtol=tol, atol=tol)
        ref = rr.runs(name, tol)
        assert np.asarray(K.info).tolist() == [r.steps for r in ref], tol
        assert max(_rel(K.V[b], r.V) for b, r in enumerate(ref)) <= max(1e-12, 100 * rr.delta_case(name, tol)), tol
        errs.append([_rel(K.V[b], Vr[b]) for b in range(len(ref))])
        print(f"{name} rtol = atol = {tol:g}: steps {np.asarray(K.info).tolist()}  error against DOP853 {errs[-1]}")
    for b in range(len(Vr)):
        assert errs[0][b] > errs[1][b] > errs[2][b]


@pytest.mark.parametrize("name", ["known_answer_2x2", "time_varying_6x2"])
def test_max_steps_exactly(lqr, name):
    """max_steps equal to the count the run needs succeeds; one fewer ends with info = -1, NaN at the output times that were not
    reached and the reached ones bit-equal to the successful run"""
    ref = rr.runs(name)[0]
    c = rr.case(name)
    one = lambda f: (lambda t: f(t)[:1])        # noqa: E731  (a batch of one design: max_steps is a per-call cap)
    call = lambda **kw: lqr.finiteHorizonLqr(one(c["A"]), one(c["B"]), one(c["Q"]), one(c["R_inv"]), c["Qf"][:1], c["T"], N=c["N"],      # noqa: E731
                                             n_samples=c["ns"], **kw)
    full = call()
    ok = call(max_steps=ref.steps)
    assert int(ok.info[0]) == ref.steps and np.array_equal(ok.V, full.V)
    cut = call(max_steps=ref.steps - 1)
    cut_ref = rr.riccati_ode(*(x[0] for x in rr.samples(c)), c["Qf"][0], c["T"], c["N"], max_steps=ref.steps - 1)
    assert int(cut.info[0]) == -1 == cut_ref.info
    reached = ~np.isnan(cut_ref.V[:, 0, 0])
    assert reached[-1] and not reached[0]
    assert np.all(np.isnan(cut.V[0, ~reached])) and np.array_equal(cut.V[0, reached], full.V[0, reached])


def test_long_horizon_meets_care(lqr):
    """the Riccati flow of a time-invariant design converges to the algebraic Riccati solution: V(0) of the (8, 4) long-horizon case
    (exp(-2 * 1.1 * 8) ~ 2e-8 from it) against infiniteHorizonLqr's P, two kernels that share no arithmetic.  1e-5: the ODE's local
    tolerance is 1.4e-8 per step."""
    c, K = _run(lqr, "long_horizon_8x4")
    A, B, Q, Ri = c["A"](0.0), c["B"](0.0), c["Q"](0.0), c["R_inv"](0.0)
    Kc, P, it = lqr.infiniteHorizonLqr(A, B, Q, np.linalg.inv(Ri), return_value=True)
    assert np.all(it > 0) and np.all(np.asarray(K.info) > 0)
    for b in range(P.shape[0]):
        assert np.max(np.linalg.eigvals(A[b] - B[b] @ Kc[b]).real) < -1.0
        assert _rel(K.V[b, 0], P[b]) <= 1e-5
        assert _rel(K(0.0)[b], Kc[b]) <= 1e-5
