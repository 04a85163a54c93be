"""zm_sincos (zopt_amd/csrc/trig.h), the sine / cosine behind every quadcopter rollout, expansion, trim and model step, on the CPU:
the header itself compiled by g++ (tests/trig_shim.cpp) against 400-bit mpmath.

Contract asserted (k = rint(2x/pi), |x| <= 1e6):   |error| <= 1.4 ulp(result) + (|k| + 1) * 1.6e-33
-- the header's own ulp figure plus its own neglected third term of pi/2 (1.497e-33 per unit of k).  The plain "1.4 ulp" does not
hold next to the zeros of sin and cos, at small arguments either: test_ulp_bound_alone_fails_next_to_the_zeros pins that fact, so
that the header's comment cannot drift back to the stronger claim.

Measured on this argument set (g++ -ffp-contract=off; 25,716 arguments): worst ratio to the contract 0.93; away from the zeros
<= 1.3 ulp; next to the zeros up to 451 ulp for |k| <= 64 and 119 ulp on the 4,000 random |k| <= 636,000 drawn here.

tests/test_sincos_gpu.py then asserts that the device computes the same bits as this host build, through every consumer."""
import numpy as np
import pytest

from tests import trig_host


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return trig_host.build(tmp_path_factory.mktemp("trig"))


@pytest.fixture(scope="module")
def measured(host):
    """{family: (x, s, c, ratio to the contract, error in ulp)}: one pass of the multi-precision reference for the module"""
    out = {}
    for name, x in trig_host.arguments().items():
        s, c = trig_host.sincos(host, x)
        out[name] = (x, s, c) + trig_host.contract_ratio(x, s, c)
    return out


@pytest.mark.parametrize("family", list(trig_host.arguments()))
def test_contract_holds_on_every_family(measured, family):
    x, s, c, ratio, ulps = measured[family]
    assert np.all(np.isfinite(s)) and np.all(np.isfinite(c))
    w = int(np.argmax(ratio))
    print(f"{family}: {len(x)} arguments, worst ratio to the contract {ratio[w]:.3f} at x = {x[w]!r}, worst error {ulps.max():.1f} ulp")
    assert ratio[w] <= 1.0, (family, x[w], s[w], c[w], ratio[w])


def test_away_from_the_zeros_the_ulp_bound_alone_holds(measured):
    """uniform arguments (none within 1e-9 relative of a multiple of pi/2): the absolute term is invisible, 1.4 ulp is the bound"""
    for family in ("uniform7", "uniform100", "uniform1e6"):
        assert measured[family][4].max() <= 1.4, family


def test_ulp_bound_alone_fails_next_to_the_zeros(measured):
    """... and next to a zero it does not, for small k either: what the header's comment now says.  (The result there is the
    reduction's own last bits: ~1e-17 |k| or less, against a neglected 1.5e-33 |k|.)
    This is a PIN OF THE DOCUMENTED CONTRACT, not a requirement: it asserts an inaccuracy so that trig.h's comment cannot drift back
    to the plain ulp claim.  If the function is improved (a third Cody-Waite term, say) this test fails by design: remove it
    together with that paragraph of the header comment -- it is not a regression."""
    assert measured["zeros_small_k"][4].max() > 10.0
    assert measured["zeros_large_k"][4].max() > 100.0


def test_pythagoras_and_symmetry(host):
    """cheap structure checks on the same arguments: s^2 + c^2 = 1 to rounding, cos even, sin odd (bit for bit, except sin(-0.0))"""
    x = trig_host.all_arguments()
    s, c = trig_host.sincos(host, x)
    sm, cm = trig_host.sincos(host, -x)
    assert np.max(np.abs(s * s + c * c - 1.0)) <= 8 * 2.0 ** -53
    assert np.array_equal(cm, c) and np.array_equal(sm, -s)


def test_zero_subnormal_and_non_finite_arguments(host):
    s, c = trig_host.sincos(host, np.array([0.0, -0.0]))
    assert np.array_equal(c, [1.0, 1.0]) and np.array_equal(s, [0.0, 0.0])
    assert not np.signbit(s[0]) and not np.signbit(s[1])                      # sin(-0.0) = +0.0: documented in trig.h
    tiny = np.array([5e-324, -5e-324, 1e-320, 2.2250738585072014e-308, -1e-300, 1e-160])
    s, c = trig_host.sincos(host, tiny)
    assert np.array_equal(s, tiny) and np.array_equal(c, np.ones(6))          # sin x = x, cos x = 1 exactly
    s, c = trig_host.sincos(host, trig_host.SPECIALS)
    assert np.all(np.isnan(s)) and np.all(np.isnan(c))                        # +-inf, NaN -> NaN
