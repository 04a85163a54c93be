"""CPU side of the MPC table tests (tests/test_mpc_tables_gpu.py holds the setup kernels to the same cases): the hard families have their
feature, the long-double reference agrees with an independent formula, the bounds derived from the fp64 oracle's own error stay below
the cap, and the unsymmetrised recursion the kernels had is told apart from the symmetrised one."""
import numpy as np
import pytest

from tests import mpc_tables_ref as tr
from tests import problems

SHAPES = problems.MPC_TABLE_SHAPES


def _radius(A):
    return np.max(np.abs(np.linalg.eigvals(A)), axis=-1)


@pytest.mark.parametrize("n,m,N", SHAPES)
@pytest.mark.parametrize("name", problems.MPC_FAMILIES)
def test_family_is_a_convex_problem_with_an_offset(name, n, m, N):
    """Every family: symmetric weights, Q >= 0, R > 0, c != 0, two problems with different data, seven increasing penalty levels."""
    A, B, c, Qs, Rs, rho = problems.hard_mpc(name, n, m, N)
    assert A.shape == (2, N, n, n) and B.shape == (2, N, n, m) and c.shape == (2, N, n) and Qs.shape == (2, N, n, n)
    assert Rs.shape == (2, N, m, m) and rho.shape == (2, 7)
    assert np.array_equal(Qs, np.swapaxes(Qs, -1, -2)) and np.array_equal(Rs, np.swapaxes(Rs, -1, -2))
    wq, wr = np.linalg.eigvalsh(Qs), np.linalg.eigvalsh(Rs)
    assert np.all(wq[..., 0] >= -1e-12 * np.maximum(1.0, wq[..., -1])) and np.all(wr[..., 0] > 0)
    assert np.all(np.max(np.abs(c), axis=-1) > 0)
    assert not np.array_equal(B[0], B[1]) and not np.array_equal(Qs[0], Qs[1]) and not np.array_equal(c[0], c[1])
    assert np.all(rho > 0) and np.allclose(rho[:, 1:] / rho[:, :-1], 5.0, rtol=1e-14)


@pytest.mark.parametrize("n,m,N", SHAPES)
def test_families_have_their_feature(n, m, N):
    fam = {name: problems.hard_mpc(name, n, m, N) for name in problems.MPC_FAMILIES}
    # spectral radius: every stage of `unstable` at 1.3; the LTI families one matrix for every stage at 1.3 / 1.05
    assert np.allclose(_radius(fam["unstable"][0]), 1.3, rtol=1e-12)
    for name, r in problems.MPC_LTI_RADIUS.items():
        A, B, _, Qs, Rs, _ = fam[name]
        assert np.allclose(_radius(A), r, rtol=1e-12)
        assert all(np.array_equal(X[:, k], X[:, 0]) for X in (A, B, Rs) for k in range(N))
        assert all(np.array_equal(Qs[:, k], Qs[:, 0]) for k in range(N - 1))
        assert N == 1 or not np.array_equal(Qs[:, N - 1], Qs[:, 0])
    # the control weight: eight decades down / up against the plain family
    rp = np.linalg.eigvalsh(fam["plain"][4])
    small = 1e-8 if m <= n else 1e-4
    assert np.allclose(np.linalg.eigvalsh(fam["cheap_control"][4]), small * rp, rtol=1e-9)
    assert np.allclose(np.linalg.eigvalsh(fam["expensive_control"][4]), 1e8 * rp, rtol=1e-9)
    assert np.max(np.linalg.eigvalsh(fam["cheap_control"][4])[..., 0]) <= 1e2 * small      # min eig R
    assert np.min(np.linalg.eigvalsh(fam["expensive_control"][4])[..., 0]) >= 1e6
    # cond(Suu) at the lowest penalty level, from the reference's Minv: rank-one B under a small R (m = 1: a rank-one B has full rank)
    cond = lambda name: np.linalg.cond(tr.case(name, n, m, N)["ref"][1][:, 0].astype(np.float64))      # noqa: E731
    if m > 1:
        assert np.max(cond("illcond_quu")) >= 1e5 and np.max(cond("illcond_quu")) >= 1e3 * np.max(cond("plain"))
    # coordinates over four decades: the columns of K over as many
    if n > 1:
        K = np.abs(tr.case("badly_scaled", n, m, N)["ref"][0].astype(np.float64))
        col = np.max(K, axis=(0, 1, 2, 3))
        assert np.max(col) / np.min(col) >= 1e3
    # stage weights: no state weight at most stages, a heavy terminal one, R over four decades
    _, _, _, Qs, Rs, _ = fam["stage_weights"]
    zero = np.array([not np.any(Qs[:, k]) for k in range(N)])
    assert not zero[N - 1] and np.sum(zero) >= (N - 1) * 0.8
    assert np.allclose(Qs[:, N - 1], 100.0 * fam["plain"][3][:, N - 1], rtol=1e-14)
    if N > 1:
        assert np.allclose(Rs[:, N - 1], 1e4 * fam["plain"][4][:, N - 1], rtol=1e-12)
        assert np.array_equal(Rs[:, 0], fam["plain"][4][:, 0])


@pytest.mark.parametrize("name,n,m,N", tr.ALL_CASES)
def test_reference_agrees_with_the_other_formula(name, n, m, N):
    """`tables_ld` (Joseph form) against `tables_ld_plain` (the non-Joseph update, symmetrised), both in long double: two formulas for
    the same tables whose rounding errors differ.  Their distance, in the tests' metric, must stay below 1 % of the fp64 oracle's own
    error on the case (or on `plain`, whichever the bound takes) -- i.e. below 1e-4 of the bound the GPU test applies, so the reference's
    own error cannot decide a test.  (The unit roundoffs are 2^-64 against 2^-53: a ratio of 4.9e-4; the two formulas amplify it by
    different constants, for which the 1 % leaves a factor 20.)"""
    c = tr.case(name, n, m, N)
    alt = tr.tables_ld_plain(*c["args"])
    err = [float(np.max(e)) for e in tr.table_errors(name, n, alt, c["ref"])]
    bound = tr.case_bound(name, n, m, N)
    print(f"{name} ({n},{m},{N}): |Joseph - plain| K {err[0]:.1e} Minv {err[1]:.1e} D {err[2]:.1e}; bounds {bound}")
    for e, b in zip(err, bound):
        assert e <= 1e-4 * b


@pytest.mark.parametrize("name,n,m,N", tr.ALL_CASES)
def test_bound_is_below_the_cap(name, n, m, N):
    """100 x the oracle's own error is at most 1e-7 on every admitted case: an oracle that ran the unsymmetrised recursion would sit at
    O(1) and beyond on the unstable families and grant a vacuous bound."""
    bound = tr.case_bound(name, n, m, N)
    print(f"{name} ({n},{m},{N}): oracle error {tr.case(name, n, m, N)['e']}, bounds {bound}")
    assert all(0.0 < b <= tr.CAP for b in bound)


def test_unsymmetrised_recursion_fails_on_lti_unstable():
    """The fp64 restatement of the recursion the kernels had, P <- (2Q + rho I) + A'PA - Sux'K with no symmetrisation, is off by more
    than 1e-3 on `lti_unstable` at (12, 4, 75) -- ten thousand times the cap -- while the symmetrised oracle is within the case's bound
    by construction: the family tells the two recursions apart."""
    c = tr.case("lti_unstable", 12, 4, 75)
    bad = tr.tables_unsymmetrised(*c["args"])
    eK = float(np.nanmax(tr.table_errors("lti_unstable", 12, bad, c["ref"])[0]))
    print(f"unsymmetrised recursion, lti_unstable (12,4,75): error of K {eK:.2e}; symmetrised oracle {c['e'][0]:.2e}")
    assert eK > 1e-3
    assert c["e"][0] <= 1e-2 * tr.case_bound("lti_unstable", 12, 4, 75)[0]


def test_unbounded_lqr_reference_is_stationary():
    """`lqr_rollout_ld` is the minimiser of the box-free problem: the gradient of the cost in the condensed inputs vanishes there (long
    double, on the affine time-varying `unstable` family), and it follows the dynamics."""
    A, B, c, Qs, Rs, _ = (X[0] for X in problems.hard_mpc("unstable", 4, 2, 12))
    x0 = np.random.default_rng(3).standard_normal(4)
    x, u = tr.lqr_rollout_ld(A, B, c, Qs, Rs, x0)
    LD = np.longdouble
    A, B, c, Qs, Rs = (np.asarray(X, dtype=LD) for X in (A, B, c, Qs, Rs))
    N = u.shape[0]
    assert max(float(np.max(np.abs(x[k + 1] - (A[k] @ x[k] + B[k] @ u[k] + c[k])))) for k in range(N)) <= 1e-17 * float(np.max(np.abs(x)))
    lam = 2 * Qs[N - 1] @ x[N]      # costate: d cost / d x_N
    g = np.empty_like(u)
    for k in range(N - 1, -1, -1):
        g[k] = 2 * Rs[k] @ u[k] + B[k].T @ lam
        lam = (2 * Qs[k - 1] @ x[k] if k >= 1 else 0) + A[k].T @ lam
    scale = float(np.max(np.abs(2 * Rs @ u[..., None])))
    assert float(np.max(np.abs(g))) <= 1e-15 * max(1.0, scale)


@pytest.mark.parametrize("module,name", [("mpc_iterates_cases", "unstable:12,4,40"), ("mpc_ltv_ref", "ltvunstable:8,4,30")])
def test_unstable_iterate_cases_are_decisive_and_constrained(module, name):
    """The two iterate cases on unstable plants (tests/test_mpc_iterates_gpu.py, tests/test_mpc_ltv_gpu.py): the restatement ends
    "optimal" on every instance, clear of every rounding-sensitive decision (the thresholds of tests/test_mpc_levels_oracle.py), with at
    least one active input bound on most instances, and its result passes the KKT certificate the GPU tests apply to the kernel's."""
    import importlib
    from oracle import mpc_oracle as mo
    from tests import mpc_tracking_ref as trk
    mod = importlib.import_module("tests." + module)
    c, (row,) = mod.build(name), mod.reference(name)
    active = 0
    for b, r in enumerate(row):
        assert r.status == "optimal" and r.level_margin >= 1e-4 and r.stop_margin >= 1e-6, (name, b, r.status, r.level_margin, r.stop_margin)
        if module == "mpc_ltv_ref":
            A, B, ck, Q, R, Qf, *box = c.inst[b]
        else:
            (A, B, Q, R, Qf, *box), ck = c.inst[b], None
            A, B = np.tile(A, (c.N, 1, 1)), np.tile(B, (c.N, 1, 1))
        assert np.all(np.abs(np.linalg.eigvals(A)).max(axis=-1) > 1.25)
        active += trk.n_active(r.x, r.u, *box) >= 1
        kkt = mo.kkt_residuals_stage(A, B, ck, *mo.stage_args(Q, R, Qf, c.N, *box), c.x0[b], r.x, r.u, act_tol=1e-4)
        assert kkt["dyn"] <= 1e-12 and kkt["bound"] <= 1e-4 and kkt["stat"] <= 1e-3, (name, b, kkt)
    assert active >= 3
