"""CPU tests of tests/riccati_ode_ref.py: the NumPy restatement of riccati_ode_kernel is pinned against the oracle's DOP853
integration and the scalar closed form, and every case of tests/test_riccati_ode_steps_gpu.py is ADMITTED: its fp64 and long-double
runs must take the same attempted and rejected steps, keep every accept / reject decision at least 1e-3 away from err = 1 and agree
in V.  A case that fails these is not a usable pin (the kernel's fma contraction and summation order could flip a decision as
legitimately as the change of precision does): re-seed or shorten it.  The deviation delta_case between the two runs is what the GPU
bound max(1e-12, 100 * delta_case) is built from.

Admitted (steps / rejected per design, delta_case):
    known_answer_2x2      14 / 2                     6e-17
    full_tile_16x16       59, 58 / 1, 1              8e-16
    single_input_16x1     84, 114 / 2, 4             1e-12
    wide_3x7              51, 45 / 0, 0              2e-16
    ragged_13x16          43, 41 / 1, 1              1e-16
    large_Qf_8x2          191, 206 / 4, 5            5e-13
    stiff_12x4            267, 265 / 44, 43          3e-11
    time_varying_6x2      60, 86 / 6, 5              1e-15
    time_varying_16x16    69, 69 / 3, 4              3e-16
    kinked_6x2            87, 82 / 12, 5             1e-15
    kinked_16x16          70, 64 / 4, 3              3e-16
    long_horizon_8x4      61, 60 / 0, 0              6e-13
A T = 40 variant of the long-horizon case was not: 158 against 160 steps."""
import numpy as np
import pytest

from oracle import zopt_oracle as zo
from tests import riccati_ode_ref as rr

LD = np.longdouble


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


@pytest.mark.parametrize("name", sorted(rr.CASES))
def test_case_is_admitted(name):
    r64, rld = rr.runs(name), rr.runs(name, 1.4e-8, LD)
    assert len(r64) == len(rld) >= 1
    for a, b in zip(r64, rld):
        assert a.info == a.steps > 0 and b.info == b.steps
        assert (a.steps, a.rejected) == (b.steps, b.rejected)
        assert min(a.margin, b.margin) >= 1e-3
        assert a.V.dtype == np.float64 and b.V.dtype == LD and np.all(np.isfinite(a.V))
    delta = rr.delta_case(name)
    print(f"{name}: steps {[r.steps for r in r64]} rejected {[r.rejected for r in r64]} "
          f"min|err-1| {min(r.margin for r in r64 + rld):.1e} delta_case {delta:.1e}")
    assert delta <= 1e-10       # the two precisions agree in V: the GPU bound 100 * delta stays far below the 2e-6 of the oracle check


@pytest.mark.parametrize("tol", rr.TOLERANCES)
def test_tolerance_case_is_admitted(tol):
    r64, rld = rr.runs(rr.TOLERANCE_CASE, tol), rr.runs(rr.TOLERANCE_CASE, tol, LD)
    for a, b in zip(r64, rld):
        assert (a.steps, a.rejected) == (b.steps, b.rejected) and a.steps > 0
        assert min(a.margin, b.margin) >= 1e-3
    assert rr.delta_case(rr.TOLERANCE_CASE, tol) <= 1e-10


def test_tolerance_is_honoured_by_the_restatement():
    """tighter tolerance: more steps, and a monotonically smaller error against the 1e-12 DOP853 integration"""
    c = rr.case(rr.TOLERANCE_CASE)
    pick = lambda f: (lambda t: f(t)[0])        # noqa: E731
    _, _, Vr = zo.finiteHorizonLqr(pick(c["A"]), pick(c["B"]), pick(c["Q"]), pick(c["R_inv"]), c["Qf"][0], c["T"], N=c["N"])
    runs = [rr.runs(rr.TOLERANCE_CASE, tol)[0] for tol in rr.TOLERANCES]
    errs = [_rel(r.V, Vr) for r in runs]
    assert runs[0].steps < runs[1].steps < runs[2].steps
    assert errs[0] > errs[1] > errs[2] and errs[2] <= 1e-8


@pytest.mark.parametrize("name", sorted(rr.CASES))
def test_restatement_matches_dop853(name):
    c = rr.case(name)
    for b, run in enumerate(rr.runs(name)):
        pick = lambda f: (lambda t: f(t)[b])        # noqa: E731
        _, t, Vr = zo.finiteHorizonLqr(pick(c["A"]), pick(c["B"]), pick(c["Q"]), pick(c["R_inv"]), c["Qf"][b], c["T"], N=c["N"])
        assert run.V.shape == Vr.shape and _rel(run.V, Vr) <= 2e-6
        assert np.array_equal(run.V[-1], c["Qf"][b])


def test_known_answer_closed_form():
    """A = B = Q = R_inv = Qf = I2, T = 1 (the reference's known-answer test): V(t) = k(t) I with the scalar Riccati solution"""
    run, = rr.runs("known_answer_2x2")
    s2 = np.sqrt(2)
    k = lambda t: ((1 + s2) * np.exp(2 * s2) - (s2 - 1) * np.exp(2 * s2 * t)) / (np.exp(2 * s2 * t) + np.exp(2 * s2))      # noqa: E731
    for j, tj in enumerate(np.linspace(0, 1, 4)):
        assert run.V[j] == pytest.approx(k(tj) * np.eye(2), rel=1e-7, abs=1e-9)
    assert (run.steps, run.rejected) == (14, 2)


def test_max_steps_and_nan_exit():
    """max_steps exactly: the run with the full count succeeds, one fewer ends with info = -1, NaN at the output times not reached and
    the reached ones unchanged; a finite escape time (Q = -100 I) ends with info = -2."""
    c = rr.case("known_answer_2x2")
    A_s, B_s, Ri_s, Q_s = (x[0] for x in rr.samples(c))
    full = rr.riccati_ode(A_s, B_s, Ri_s, Q_s, c["Qf"][0], c["T"], c["N"])
    same = rr.riccati_ode(A_s, B_s, Ri_s, Q_s, c["Qf"][0], c["T"], c["N"], max_steps=full.steps)
    cut = rr.riccati_ode(A_s, B_s, Ri_s, Q_s, c["Qf"][0], c["T"], c["N"], max_steps=full.steps - 1)
    assert same.info == full.steps and np.array_equal(same.V, full.V)
    assert cut.info == -1 and np.all(np.isnan(cut.V[0])) and np.array_equal(cut.V[1:], full.V[1:])
    with np.errstate(all="ignore"):
        esc = rr.riccati_ode(0 * A_s, B_s, Ri_s, -100.0 * Q_s, c["Qf"][0], 1.0, 6)
    assert esc.info == -2 and np.all(np.isnan(esc.V[0])) and np.array_equal(esc.V[-1], c["Qf"][0])


def test_interpolation_of_samples():
    """ns > 1: coefficients linear in t are reproduced exactly by the interpolation, whatever the number of samples"""
    c = rr.case("time_varying_6x2")
    ts = lambda ns: np.linspace(0.0, c["T"], ns)        # noqa: E731
    smp = lambda ns: tuple(np.stack([c[k](float(t))[0] for t in ts(ns)]) for k in ("A", "B", "R_inv", "Q"))      # noqa: E731
    a = rr.riccati_ode(*smp(17), c["Qf"][0], c["T"], c["N"])
    b = rr.riccati_ode(*smp(2), c["Qf"][0], c["T"], c["N"])
    assert a.steps == b.steps == rr.runs("time_varying_6x2")[0].steps and _rel(a.V, b.V) <= 1e-12


@pytest.mark.parametrize("name", ["kinked_6x2", "kinked_16x16"])
def test_kinked_cases_see_the_sample_interval(name):
    """the samples of the kinked cases are drawn one by one, so an interpolation that picked the neighbouring interval would take
    coefficients and reach another V: the restatement fed the samples shifted by one is far outside the GPU test's value bound
    (the step count may or may not move).  (On the
    coefficients that are linear over the whole interval the same shift would go unseen: every interval extrapolates the same line.)"""
    c = rr.case(name)
    smp = [x[0] for x in rr.samples(c)]
    shifted = [np.concatenate([x[1:], x[-1:]]) for x in smp]
    a = rr.runs(name)[0]
    b = rr.riccati_ode(*shifted, c["Qf"][0], c["T"], c["N"])
    assert b.steps > 0 and _rel(b.V, a.V) > 1e-3
