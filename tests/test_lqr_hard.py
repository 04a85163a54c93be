"""CPU side of the hard-family tests of `discreteFiniteHorizonLqr` (tests/lqr_hard_ref.py; GPU side: tests/test_lqr_hard_gpu.py).

Three things are proven here, without a GPU:
  * every family of `problems.HARD_LQR` has the feature it was built for, and the CPU models predict, with a margin of 8 either way
    on the guard's residual ratio, which steps leave K1's cofactor solve and which stay on it; the elimination without row exchanges
    of the other kernels is predicted likewise.  The product library counts nothing, so on the GPU this prediction is the evidence that
    the pivoted re-solve ran;
  * the conditions under which the bounds discriminate: every case's fp64 oracle error is below 1e-9, and the fp32 tile kernel's
    families are those whose fp32 yardstick is below 1e-3;
  * `check_gains` bites: two honest fp64 evaluations pass it, seven planted errors fail it.
"""
import numpy as np
import pytest

from oracle import zopt_oracle as zo
from tests import hp_reference as hp
from tests import lqr_hard_ref as ref
from tests import problems
from tools import k1_solve_model as km

K1_CASES = [(n, m, T) for n, m in ref.K1_SHAPES for T in ref.K1_T]
ALL_SHAPES = ([(n, m, ref.K1_T) for n, m in ref.K1_SHAPES] + [(n, m, ref.REG_T) for n, m in ref.REG_SHAPES]
              + [(n, m, ref.TILE_T) for n, m in ref.TILE_SHAPES])


def _blocks(c):
    return km.riccati_blocks(*c.args)


# --------------------------------------------------------------------------------------------------------- conditions of the bounds
@pytest.mark.parametrize("n,m,Ts", ALL_SHAPES, ids=lambda x: str(x))
def test_oracle_error_keeps_every_bound_discriminating(n, m, Ts):
    """Every case of every path: the fp64 oracle's own error against long double is <= 1e-9, and the bound is `hp.sweep_bounds` of
    it and of `plain`'s at the same shape, horizon and batch -- computed per case, about 1e-13 where the family is well conditioned"""
    for T in Ts + (ref.CHILD_T if (n, m) in sum(ref.CHILD_SHAPES.values(), []) else []):
        for f in ref.FAMILIES:
            c = ref.case(f, n, m, T)
            assert c.e_case <= ref.ORACLE_LIMIT, (f, n, m, T, c.e_case)
            assert c.bound == 100.0 * max(c.e_case, ref.case("plain", n, m, T).e_case) and c.e_plain <= 1e-14
            assert np.all(np.isfinite(c.ref.astype(np.float64))) and np.all(c.scale > 0)


@pytest.mark.parametrize("n,m", ref.K1_SHAPES, ids=str)
def test_fp32_storage_cases_are_bounded_by_their_own_fp64_error(n, m):
    """K1 on fp32 storage: the case is the fp32-rounded arrays, its reference the long-double sweep of exactly those numbers, its
    fp64 bound the oracle's error on them (<= 1e-9 again)"""
    for T in ref.K1_T_F32:
        for f in ref.FAMILIES:
            c = ref.case(f, n, m, T, storage="f32")
            assert all(X.dtype == np.float32 for X in c.args) and c.e_case <= ref.ORACLE_LIMIT, (f, T, c.e_case)


@pytest.mark.parametrize("n,m", ref.TILE_SHAPES, ids=str)
def test_fp32_tile_families_are_those_the_fp32_yardstick_resolves(n, m):
    """The fp32 tile kernel is held to the families on which NumPy's own fp32 recursion stays below 1e-3 of the long-double gains:
    `plain`, `permuted_R`, `input_units` and `unstable` always are; `dominant_input` at r = 1e-2 is not at the large shapes"""
    for T in ref.TILE_T:
        inc = ref.tile32_families(n, m, T)
        assert {"plain", "permuted_R", "input_units", "unstable"} <= set(inc), (T, inc)
        for f in inc:
            c = ref.case(f, n, m, T, storage="f32")
            assert c.bound32 == 100.0 * max(c.e32_case, c.e32_plain) <= 100.0 * ref.YARDSTICK32_LIMIT
    assert "dominant_input_1e-2" not in ref.tile32_families(n, m, 6) or n < 16


# ------------------------------------------------------------------------------------------------------------ features of the families
@pytest.mark.parametrize("n,m,T", K1_CASES)
def test_guard_predictions_have_margin(n, m, T):
    """K1's model on every step (residual ratio of the cofactor solve; the guard's threshold is 1): >= 8 on every step that must
    take the pivoted re-solve, <= 1/8 on every step that must stay on the cofactor solve.
        input_units, dominant_input_1e-2   every step fires
        dominant_every_3                   exactly the steps = 0 mod 3 fire
        plain, permuted_R                  none fires"""
    k = np.arange(T)
    g = {f: ref.guard_ratio(ref.case(f, n, m, T).args) for f in ref.FAMILIES}
    print({f: (float(v.min()), float(v.max())) for f, v in g.items()})
    assert g["input_units"].min() >= ref.FIRES and g["dominant_input_1e-2"].min() >= ref.FIRES
    assert g["plain"].max() <= ref.ADMITS and g["permuted_R"].max() <= ref.ADMITS
    assert g["dominant_every_3"][:, k % 3 == 0].min() >= ref.FIRES
    assert T < 2 or g["dominant_every_3"][:, k % 3 != 0].max() <= ref.ADMITS
    for f in ("unstable", "cheap", "expensive", "nonsymmetric"):     # no prediction is needed of them; the model has them on the fast path
        assert g[f].max() < 1.0


@pytest.mark.parametrize("n,m", ref.K1_SHAPES, ids=str)
def test_dominant_input_mixes_both_solves_inside_a_sweep(n, m):
    """`dominant_input` at r = 1, T = 11: at least a third of the steps fire with margin (ratio >= 8), and some stay on the cofactor
    solve with margin -- the two solves alternate irregularly inside one trajectory's sweep"""
    g = ref.guard_ratio(ref.case("dominant_input", n, m, 11).args)
    assert 3 * int((g >= ref.FIRES).sum()) >= g.size and int((g <= ref.ADMITS).sum()) >= 1, (int((g >= 8).sum()), g.size)
    per_traj = (g >= ref.FIRES).any(axis=1) & (g <= ref.ADMITS).any(axis=1)
    assert per_traj.sum() >= 3


@pytest.mark.parametrize("n,m,Ts", [s for s in ALL_SHAPES if s[1] >= 2], ids=lambda x: str(x))
def test_growth_predictions(n, m, Ts):
    """The elimination without row exchanges (register and tile kernels; abandoned above a multiplier of 4, the fp32 tile kernel above
    a squared column sum of 16): on `permuted_R` every step of every shape meets a multiplier >= 8; on `dominant_input` (r = 1e-2)
    some step of every shape does; `plain` stays below 4 everywhere"""
    worst_dom = 0.0
    for T in Ts:
        big, sq = ref.growth_of(ref.case("permuted_R", n, m, T).args)
        assert big.min() >= 8.0 and sq.min() >= 64.0, (T, big.min())
        big, sq = ref.growth_of(ref.case("plain", n, m, T).args)
        assert big.max() < 4.0 and sq.max() < 16.0, (T, big.max(), sq.max())
        worst_dom = max(worst_dom, float(ref.growth_of(ref.case("dominant_input_1e-2", n, m, T).args)[0].max()))
    assert worst_dom >= 8.0, worst_dom


def test_input_units_is_graded_and_undoes_exactly():
    """`input_units`: Suu's entries span more than ten decades although the problem in its own units is plain; the long-double gains,
    units undone, are those of the unscaled problem (the scaling is by powers of two: every product and sum scales exactly)"""
    for n, m in ref.K1_SHAPES + [(5, 2), (24, 8)]:
        T = 2
        c = ref.case("input_units", n, m, T)
        Suu = np.abs(_blocks(c)[0])
        assert np.all(Suu.max(axis=(-2, -1)) / Suu.min(axis=(-2, -1)) >= 1e10)
        d, e = problems.lqr_units(n, m)
        assert np.all(np.log2(d) == np.round(np.log2(d))) and np.all(np.log2(e) == np.round(np.log2(e)))
        assert d[0] < 1e-2 * 1.3 and d[-1] > 1e2 / 1.3 and e[0] < 1e-3 * 1.3 and e[-1] > 1e3 / 1.3
        base = problems.lqr_mildly_unstable(c.batch, T, n, m, problems.hard_lqr_seed("input_units", n, m, T))
        assert np.allclose(np.max(np.abs(np.linalg.eigvals(base[0])), axis=-1), 1.05)
        Lb = hp.finite_horizon_ld(*base, T)
        assert hp.sweep_metric(c.ref, Lb).max() <= 1e-17
        # and the small rows would be hidden without undoing: the raw gains' rows span the six decades of E
        raw = np.abs(hp.finite_horizon_ld(*c.args, T)).max(axis=-1)
        assert np.all(raw[..., -1] / raw[..., 0] >= 1e4)


def test_dominant_input_has_rank_one_B():
    for name, every in (("dominant_input", 1), ("dominant_input_1e-2", 1), ("dominant_every_3", 3)):
        c = ref.case(name, 12, 4, 7)
        s = np.linalg.svd(c.args[1], compute_uv=False)
        hit = np.arange(7) % every == 0
        assert np.all(s[:, hit, 1] <= 1e-14 * s[:, hit, 0]) and np.all(s[:, ~hit, 3] >= 1e-2 * s[:, ~hit, 0])
    p, d = ref.case("plain", 12, 4, 7), ref.case("dominant_input_1e-2", 12, 4, 7)
    assert np.array_equal(d.args[3], 1e-2 * p.args[3]) and np.array_equal(d.args[0], p.args[0])


def test_permuted_R_is_well_conditioned():
    """`permuted_R`: Suu is a perturbed permutation (condition below 2, oracle error at the plain level), nonsymmetric, with a
    leading entry ~0.01"""
    for n, m in ref.K1_SHAPES + [(24, 8)]:
        c = ref.case("permuted_R", n, m, 6 if n > 12 else 7)
        Suu = _blocks(c)[0]
        assert np.linalg.cond(Suu).max() < 2.0 and c.e_case <= 2e-15
        assert np.abs(Suu[..., 0, 0]).max() < 0.25 and np.abs(Suu - np.swapaxes(Suu, -1, -2)).max() > 0.5


def test_unstable_value_grows_along_the_sweep():
    c, p = ref.case("unstable", 12, 4, 11), ref.case("plain", 12, 4, 11)
    assert np.allclose(np.max(np.abs(np.linalg.eigvals(c.args[0])), axis=-1), 1.3)
    tr_c, tr_p = [], []
    ref.riccati64(*c.args, 11, trace=tr_c)
    ref.riccati64(*p.args, 11, trace=tr_p)
    # largest value entry after the last (k = 0) update against the first: the controls hold the growth
    # back, but the value ends well above the plain family's, which settles
    assert np.mean(tr_c[-1]) >= 2 * np.mean(tr_c[0]) and np.mean(tr_c[-1]) >= 1.5 * np.mean(tr_p[-1]), (tr_c[-1], tr_p[-1], tr_c[0])
    assert np.all(tr_p[-1] <= 2 * tr_p[0])


def test_cheap_and_expensive_dominance():
    """`cheap`: Suu is B^T V B to 1e-6 and the dynamics are unstable (1.2); `expensive`: Suu is R to 1e-6 and the gains are ~1e-7"""
    c = ref.case("cheap", 12, 4, 7)
    Suu = _blocks(c)[0]
    assert np.all(np.abs(c.args[3]).max(axis=(-2, -1)) <= 1e-6 * np.abs(Suu).max(axis=(-2, -1)))
    assert np.allclose(np.max(np.abs(np.linalg.eigvals(c.args[0])), axis=-1), 1.2)
    c = ref.case("expensive", 12, 4, 7)
    Suu = _blocks(c)[0]
    assert np.all(np.abs(Suu - c.args[3]).max(axis=(-2, -1)) <= 1e-6 * np.abs(Suu).max(axis=(-2, -1)))
    assert np.all(c.scale < 1e-6) and np.all(c.scale > 1e-9)


def test_nonsymmetric_parts_are_of_order_one():
    c = ref.case("nonsymmetric", 12, 4, 7)
    for X in (c.args[2], c.args[3]):
        assert np.all(np.abs(X - np.swapaxes(X, -1, -2)).max(axis=(-2, -1)) >= 0.5)


# ------------------------------------------------------------------------------------------------------------------- the checker bites
HONEST = [(f, n, m, T) for f in ref.FAMILIES for n, m, T in [(12, 4, 11), (8, 4, 7), (5, 2, 5), (24, 8, 6)]]


@pytest.mark.parametrize("name,n,m,T", HONEST)
def test_honest_evaluations_pass(name, n, m, T):
    """The fp64 oracle, and the same recursion with its products reassociated -- B^T (V B) for (B^T V) B, LAPACK's solve -- pass"""
    c = ref.case(name, n, m, T)
    e0 = ref.check_gains(zo.discreteFiniteHorizonLqr(*c.args, T), c)
    e1 = ref.check_gains(ref.riccati64(*c.args, T, reorder=True), c)
    print(f"{name} ({n}, {m}, {T}): oracle {e0:.2e}, reordered {e1:.2e}, bound {c.bound:.2e}")
    if m == 4 and n in (8, 12):          # K1's model itself, guard and re-solve included, passes too
        ref.check_gains(ref.riccati64(*c.args, T, solve=lambda S, b: km.cofactor_solve(S, b)[0]), c)


def _caught(L, c):
    with pytest.raises(AssertionError):
        ref.check_gains(L, c)


@pytest.mark.parametrize("name", ["plain", "expensive", "input_units"])
def test_planted_single_entry_row_swap_and_neighbour_are_caught(name):
    """One entry of one late step off by 1e-11 of its trajectory's scale (in the undone units); two rows of one L_k swapped; one
    step's gain taken from the neighbouring trajectory"""
    c = ref.case(name, 12, 4, 11)
    good = zo.discreteFiniteHorizonLqr(*c.args, 11)
    ref.check_gains(good, c)
    d, e = problems.lqr_units(12, 4) if name == "input_units" else (np.ones(12), np.ones(4))
    L = good.copy()
    L[2, 9, 1, 5] += 1e-11 * c.scale[2] * e[1] / d[5]
    _caught(L, c)
    L = good.copy()
    L[3, 4, [0, 1]] = L[3, 4, [1, 0]]
    _caught(L, c)
    L = good.copy()
    L[1, 6] = good[2, 6]
    _caught(L, c)


def test_planted_unchecked_elimination_is_caught_on_permuted_R():
    """`km.nopivot_solve`'s result used without its growth check (multipliers in the thousands) on `permuted_R`: outside the bound;
    with the check (and its pivoted re-solve) inside it"""
    c = ref.case("permuted_R", 8, 4, 11)
    ref.check_gains(ref.riccati64(*c.args, 11, solve=lambda S, b: km.nopivot_solve(S, b)[0]), c)
    _caught(ref.riccati64(*c.args, 11, solve=ref.nopivot_unchecked), c)


@pytest.mark.parametrize("name", ["dominant_input", "dominant_input_1e-2", "dominant_every_3"])
@pytest.mark.parametrize("n,m", ref.K1_SHAPES, ids=str)
def test_planted_unguarded_cofactor_solve_is_caught(name, n, m):
    """The cofactor result used without its guard on the `dominant_input` families: outside the bound at these seeds (by a factor
    7 at r = 1, by five orders at r = 1e-2).  On `input_units` it is NOT caught: a graded Suu trips the residual guard, but the cofactor
    gains themselves stay accurate there, so that family holds the re-solve's data path, not the guard."""
    c = ref.case(name, n, m, 11)
    L = ref.riccati64(*c.args, 11, solve=ref.cofactor_unguarded)
    print(f"{name} ({n}, {m}): unguarded {hp.sweep_metric(L, c.ref).max():.2e}, bound {c.bound:.2e}")
    _caught(L, c)


def test_planted_symmetrised_Q_is_caught():
    c = ref.case("nonsymmetric", 12, 4, 11)
    _caught(ref.riccati64(*c.args, 11, symmetrise_Q=True), c)


@pytest.mark.parametrize("n,m", ref.K1_SHAPES, ids=str)
def test_planted_schur_form_is_caught_on_cheap(n, m):
    """V' = Q + A^T V A - Sux^T L in place of the Joseph form on `cheap`: the subtraction's error grows with the unstable dynamics, and
    at T = 30 it is outside the bound (at T = 11 it is still inside: the GPU test runs `cheap` at T = 30 as well)"""
    c = ref.case("cheap", n, m, 30)
    assert c.e_case <= ref.ORACLE_LIMIT
    ref.check_gains(zo.discreteFiniteHorizonLqr(*c.args, 30), c)
    _caught(ref.riccati64(*c.args, 30, value="schur"), c)
