"""GPU tests of the MPC setup kernels (zopt_amd/csrc/mpc.hip: mpc_setup_body.h in mpc_setup_kernel / mpc_setup_batched_kernel,
mpc_setup_ltv_kernel, mpc_setup_ltv_stage_kernel): the Riccati tables K, Minv, D of every (problem, level, stage) against the long-double
Joseph-form reference of tests/mpc_tables_ref.py, on the hard families of tests/problems.py: hard_mpc -- open-loop-unstable plants,
cheap / expensive control, an ill-conditioned Suu, badly scaled coordinates, stage weights.  The four entry points are called through
the C ABI on device tensors.

Bound: `hp_reference.sweep_bounds` = 100 x max(the error of the fp64 oracle `mpc_oracle.riccati_tables` on the case, its error on
`plain` at the same shape), in `hp_reference.sweep_metric` per (problem, level), on K, Minv and D separately (K of `badly_scaled` as
K diag(d)); tests/test_mpc_tables.py asserts, without a GPU, that every bound is <= 1e-7 and that the reference agrees with a second
long-double formula to 1e-4 of the bound.  The oracle's largest error over the shapes of each family (K, Minv, D), P = 2 problems x
L = 7 levels, and the bound that follows (the largest of the three tables, at the worst shape):

    family              oracle error (K, Minv, D), worst shape        bound, worst shape
    plain               2.1e-15  1.6e-15  1.1e-15                     2.1e-13  (12,4,75)
    unstable            9.8e-15  6.4e-15  4.6e-15                     9.8e-13  (4,2,75)
    cheap_control       1.6e-14  1.6e-14  6.5e-15                     1.6e-12  (4,2,75)
    expensive_control   1.3e-15  5.0e-16  5.5e-16                     2.1e-13  (12,4,75; plain's)
    illcond_quu         7.5e-10  3.4e-10  5.6e-11                     7.5e-8   (8,4,75)
    badly_scaled        7.8e-10  7.2e-10  8.5e-10                     8.5e-8   (5,3,20)
    lti_unstable        1.6e-14  3.6e-15  5.3e-15                     1.6e-12  (8,4,75)
    lti_marginal        5.3e-15  1.8e-15  1.4e-15                     5.3e-13  (8,4,75)
    stage_weights       2.3e-15  1.7e-15  4.9e-16                     2.3e-13  (12,4,2)

The fp64 recursion without the symmetrisation of the value matrix -- the kernels' formula before they stored P symmetrised -- is off by
3e3 (K) on lti_unstable at (12, 4, 75), 7e1 on `unstable` at (12, 4, 75), 2e-4 at (12, 4, 50), 1e-4 on badly_scaled at (8, 4, 75) and
5e-6 on lti_marginal at (12, 4, 75): far outside these bounds.

Relations between the entry points (bit for bit, on `lti_unstable` and `badly_scaled` data): ABt is the transposed input and does not
depend on the levels; c = NULL gives D = 0 and the same K, Minv; one launch with L levels is L launches with one; constant rows give
zm_mpc_setup_ltv_f64's tables; constant A_k, B_k give zm_mpc_setup_batched_f64's; its (p, l) slice is zm_mpc_setup_f64's.  With the
stage entry point held to the reference on the same data, all four kernels are.

End to end: box-free solves of lqrMpc / ltvMpc on the unstable families against the long-double LQR rollout, and nonsymmetric weights
against their symmetric parts (bit for bit)."""
import ctypes

import numpy as np
import pytest

from tests import mpc_tables_ref as tr
from tests import problems
from tests.hp_reference import sweep_bounds

pytestmark = pytest.mark.gpu

SENT = -7.25e77      # what every output holds before a launch
PAD = 64             # guard doubles on either side of an output
LTV_SHAPES = [s for s in problems.MPC_TABLE_SHAPES if s[0] <= 12 and s[1] <= 4]
LARGE_SHAPES = [s for s in problems.MPC_TABLE_SHAPES if s not in LTV_SHAPES]


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from zopt_amd import _lib
    return torch, _lib


class _Out:
    """An output of `shape` inside a sentinel-filled buffer with PAD guard doubles on either side."""

    def __init__(self, torch, shape):
        self.shape, self.size = shape, int(np.prod(shape))
        self.buf = torch.full((self.size + 2 * PAD,), SENT, dtype=torch.float64, device="cuda")

    def ptr(self):
        return self.buf.data_ptr() + 8 * PAD

    def read(self, at):
        """The output; asserts that every element of it was written and the guards were not."""
        h = self.buf.cpu().numpy()
        assert np.all(h[:PAD] == SENT) and np.all(h[PAD + self.size:] == SENT), (at, "written outside its slices")
        out = h[PAD:PAD + self.size].reshape(self.shape)
        assert not np.any(out == SENT), (at, "elements inside the slices left unwritten", int(np.sum(out == SENT)))
        return out.copy()


def _dev(torch, *arrays):
    return [None if X is None else torch.as_tensor(np.ascontiguousarray(X, dtype=np.float64), device="cuda") for X in arrays]


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream(torch):
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def setup_stage(gpu, A, B, c, Qs, Rs, rho, at="stage"):
    """zm_mpc_setup_ltv_stage_f64 -> (K, Minv, D, ABt)"""
    torch, _lib = gpu
    Pn, L = rho.shape
    N, n, m = B.shape[-3:]
    d = _dev(torch, A, B, c, Qs, Rs, rho)
    out = [_Out(torch, s) for s in ((Pn, L, N, m, n), (Pn, L, N, m, m), (Pn, L, N, n), (Pn, N, n + m, n))]
    _lib.check(_lib.lib().zm_mpc_setup_ltv_stage_f64(*[_ptr(t) for t in d], Pn, L, N, n, m, *[o.ptr() for o in out], _stream(torch)), at)
    torch.cuda.synchronize()
    return tuple(o.read((at, i)) for i, o in enumerate(out))


def setup_ltv(gpu, A, B, c, Q, R, Qf, rho, at="ltv"):
    """zm_mpc_setup_ltv_f64 -> (K, Minv, D, ABt)"""
    torch, _lib = gpu
    Pn, L = rho.shape
    N, n, m = B.shape[-3:]
    d = _dev(torch, A, B, c, Q, R, Qf, rho)
    out = [_Out(torch, s) for s in ((Pn, L, N, m, n), (Pn, L, N, m, m), (Pn, L, N, n), (Pn, N, n + m, n))]
    _lib.check(_lib.lib().zm_mpc_setup_ltv_f64(*[_ptr(t) for t in d], Pn, L, N, n, m, *[o.ptr() for o in out], _stream(torch)), at)
    torch.cuda.synchronize()
    return tuple(o.read((at, i)) for i, o in enumerate(out))


def setup_batched(gpu, A, B, Q, R, Qf, rho, N, at="batched"):
    """zm_mpc_setup_batched_f64 -> (K, Minv)"""
    torch, _lib = gpu
    Pn, L = rho.shape
    n, m = B.shape[-2:]
    d = _dev(torch, A, B, Q, R, Qf, rho)
    out = [_Out(torch, s) for s in ((Pn, L, N, m, n), (Pn, L, N, m, m))]
    _lib.check(_lib.lib().zm_mpc_setup_batched_f64(*[_ptr(t) for t in d], Pn, L, N, n, m, *[o.ptr() for o in out], _stream(torch)), at)
    torch.cuda.synchronize()
    return tuple(o.read((at, i)) for i, o in enumerate(out))


def setup_one(gpu, A, B, Q, R, Qf, rho, N, at="one"):
    """zm_mpc_setup_f64 for ONE problem at ONE penalty -> (K, Minv)"""
    torch, _lib = gpu
    n, m = B.shape
    d = _dev(torch, A, B, Q, R, Qf)
    out = [_Out(torch, s) for s in ((N, m, n), (N, m, m))]
    _lib.check(_lib.lib().zm_mpc_setup_f64(*[_ptr(t) for t in d], float(rho), N, n, m, *[o.ptr() for o in out], _stream(torch)), at)
    torch.cuda.synchronize()
    return tuple(o.read((at, i)) for i, o in enumerate(out))


def _hold(name, n, got, ref, bound, at, tables="K Minv D"):
    """Every (problem, level, stage) of the tables within the bound; prints the largest error of each before it asserts."""
    errs = tr.table_errors(name, n, got if len(got) == 3 else tuple(got) + (ref[2],), ref)
    line, bad = [], []
    for i, t in enumerate(("K", "Minv", "D")):
        if t in tables.split():
            e = np.nan_to_num(errs[i], nan=np.inf)
            line.append(f"{t} {float(np.max(e)):.2e} (bound {bound[i]:.2e})")
            if not np.all(e <= bound[i]):
                pl, k = np.unravel_index(int(np.argmax(e)), e.shape)
                bad.append((t, float(np.max(e)), bound[i], f"(problem, level) {divmod(int(pl), problems.MPC_N_LEVELS)} stage {int(k)}"))
    print(f"{at}: " + ", ".join(line))
    assert not bad, (at, bad)


@pytest.mark.parametrize("n,m,N", LTV_SHAPES)
@pytest.mark.parametrize("name", problems.MPC_FAMILIES)
def test_stage_entry_point_against_long_double(gpu, name, n, m, N):
    """zm_mpc_setup_ltv_stage_f64 on every family x shape it takes: every (problem, level, stage) of K, Minv, D within the case's bound;
    ABt the transposed inputs bit for bit; every element inside the outputs written, none outside them."""
    c = tr.case(name, n, m, N)
    A, B = c["args"][:2]
    K, Mi, D, ABt = setup_stage(gpu, *c["args"], at=(name, n, m, N))
    _hold(name, n, (K, Mi, D), c["ref"], tr.case_bound(name, n, m, N), f"{name} ({n},{m},{N}) stage entry")
    assert np.array_equal(ABt[:, :, :n, :], np.swapaxes(A, -1, -2)) and np.array_equal(ABt[:, :, n:, :], np.swapaxes(B, -1, -2))


@pytest.mark.parametrize("n,m,N", LARGE_SHAPES)
@pytest.mark.parametrize("name", problems.MPC_LTI_FAMILIES)
def test_time_invariant_entry_points_beyond_12_4(gpu, name, n, m, N):
    """(13, 2, 40) and (24, 8, 40) run the <24, 8> instantiation of mpc_setup_body.h, which only zm_mpc_setup_f64 and
    zm_mpc_setup_batched_f64 reach: the LTI families through both, held to the reference; the batched (p, l) slice is the single call's
    bits; the stage-varying entry points refuse the shape."""
    torch, _lib = gpu
    c = tr.case(name, n, m, N)
    A, B, cc, Qs, Rs, rho = c["args"]
    Q, R, Qf = Qs[:, 0], Rs[:, 0], Qs[:, N - 1]
    bound = tr.case_bound(name, n, m, N)
    K, Mi = setup_batched(gpu, A[:, 0], B[:, 0], Q, R, Qf, rho, N)
    _hold(name, n, (K, Mi), c["ref"], bound, f"{name} ({n},{m},{N}) batched", tables="K Minv")
    for p in range(rho.shape[0]):
        for l in (0, 3, 6):
            K1, M1 = setup_one(gpu, A[p, 0], B[p, 0], Q[p], R[p], Qf[p], rho[p, l], N)
            assert np.array_equal(K1, K[p, l]) and np.array_equal(M1, Mi[p, l]), (name, p, l)
    d = _dev(torch, A, B, cc, Qs, Rs, rho)
    o = torch.zeros(8, dtype=torch.float64, device="cuda")
    rc = _lib.lib().zm_mpc_setup_ltv_stage_f64(*[_ptr(t) for t in d], *rho.shape, N, n, m, *[o.data_ptr()] * 4, _stream(torch))
    assert rc == _lib.ZM_EUNSUPPORTED


def _lti_variant(name, n, m, N):
    """The case's data as a time-invariant problem (stage 0's A, B, Q, R for every stage, the case's terminal weight): the case itself
    for the LTI families.  Returns (stage-form args, (A, B, Q, R, Qf) per problem)."""
    A, B, c, Qs, Rs, rho = tr.case(name, n, m, N)["args"]
    rep = lambda X: np.array(np.broadcast_to(X[:, :1], X.shape))      # noqa: E731
    Qc = rep(Qs)
    Qc[:, N - 1] = Qs[:, N - 1]
    args = (rep(A), rep(B), c, Qc, rep(Rs), rho)
    return args, (A[:, 0], B[:, 0], Qs[:, 0], Rs[:, 0], Qs[:, N - 1])


@pytest.mark.parametrize("n,m,N", [(12, 4, 75), (5, 3, 20)])
@pytest.mark.parametrize("name", ["lti_unstable", "badly_scaled"])
def test_entry_points_agree_bit_for_bit_on_hard_data(gpu, name, n, m, N):
    """The four setup kernels on one time-invariant hard problem: the stage entry point is held to the long-double reference, and the
    others to its bits -- so all four are held to the reference."""
    args, (A1, B1, Q, R, Qf) = _lti_variant(name, n, m, N)
    A, B, c, Qs, Rs, rho = args
    ref = tr.tables_ld(*args)
    e = [float(np.max(x)) for x in tr.table_errors(name, n, tr.tables_oracle(*args), ref)]
    plain = tr.case("plain", n, m, N)["e"]
    bound = tuple(sweep_bounds(e[i], plain[i]) for i in range(3))
    assert max(bound) <= tr.CAP, bound
    K, Mi, D, ABt = setup_stage(gpu, *args)
    _hold(name, n, (K, Mi, D), ref, bound, f"{name} ({n},{m},{N}) time-invariant variant, stage entry")
    # ABt: the transposed inputs, whatever the levels are
    assert np.array_equal(ABt[:, :, :n, :], np.swapaxes(A, -1, -2)) and np.array_equal(ABt[:, :, n:, :], np.swapaxes(B, -1, -2))
    # one launch with L levels is L launches with one: the (p L + l) offsets of K, Minv, D; ABt identical from every level's launch
    for l in range(rho.shape[1]):
        Kl, Ml, Dl, ABl = setup_stage(gpu, A, B, c, Qs, Rs, rho[:, l:l + 1])
        assert np.array_equal(Kl[:, 0], K[:, l]) and np.array_equal(Ml[:, 0], Mi[:, l]) and np.array_equal(Dl[:, 0], D[:, l]), l
        assert np.array_equal(ABl, ABt), l
    # one problem alone is its slice of the batch
    Kp, Mp, Dp, ABp = setup_stage(gpu, A[1:], B[1:], c[1:], Qs[1:], Rs[1:], rho[1:])
    assert np.array_equal(Kp[0], K[1]) and np.array_equal(Mp[0], Mi[1]) and np.array_equal(Dp[0], D[1]) and np.array_equal(ABp[0], ABt[1])
    # c = NULL: D = 0, the rest unchanged
    K0, M0, D0, AB0 = setup_stage(gpu, A, B, None, Qs, Rs, rho)
    assert np.array_equal(K0, K) and np.array_equal(M0, Mi) and np.array_equal(AB0, ABt) and not np.any(D0)
    # constant rows: zm_mpc_setup_ltv_f64's bits (also with c = NULL)
    Kv, Mv, Dv, ABv = setup_ltv(gpu, A, B, c, Q, R, Qf, rho)
    assert np.array_equal(Kv, K) and np.array_equal(Mv, Mi) and np.array_equal(Dv, D) and np.array_equal(ABv, ABt)
    Kv0, Mv0, Dv0, _ = setup_ltv(gpu, A, B, None, Q, R, Qf, rho)
    assert np.array_equal(Kv0, K) and np.array_equal(Mv0, Mi) and not np.any(Dv0)
    # constant A_k, B_k: zm_mpc_setup_batched_f64's bits, whose (p, l) slice is zm_mpc_setup_f64's
    Kb, Mb = setup_batched(gpu, A1, B1, Q, R, Qf, rho, N)
    assert np.array_equal(Kb, K) and np.array_equal(Mb, Mi)
    for p in range(rho.shape[0]):
        for l in range(rho.shape[1]):
            K1, M1 = setup_one(gpu, A1[p], B1[p], Q[p], R[p], Qf[p], rho[p, l], N)
            assert np.array_equal(K1, K[p, l]) and np.array_equal(M1, Mi[p, l]), (p, l)


# ---- end to end: box-free solves are the LQR ------------------------------------------------------------------------------------------------

def _x0(n, nb, seed):
    return np.random.default_rng(seed).standard_normal((nb, n))


@pytest.mark.parametrize("n,m,N", [(12, 4, 75), (12, 4, 40), (24, 8, 40)])
def test_unbounded_lqrmpc_on_an_unstable_plant_equals_lqr(gpu, n, m, N):
    """lqrMpc on `lti_unstable` (spectral radius 1.3) without a box, eps 1e-10: u against the long-double finite-horizon LQR rollout at
    test_unbounded_box_equals_lqr's 1e-7 max(1, max|u_ref|).  With unsymmetrised tables the restatement of the solve reports "optimal"
    and is off by 6e-7 at (12, 4, 75) -- outside this tolerance -- and by 9e-13 at (12, 4, 40), where the tables' error has not yet reached u."""
    from zopt_amd import mpcUtils
    A, B, _, Qs, Rs, _ = (X[0] for X in problems.hard_mpc("lti_unstable", n, m, N))
    Q, R, Qf = Qs[0], Rs[0], Qs[N - 1]
    inf_n, inf_m = np.full(n, np.inf), np.full(m, np.inf)
    prob = mpcUtils.lqrMpc(A[0], B[0], Q, R, N, -inf_n, inf_n, -inf_m, inf_m, Qf=Qf)
    x0 = _x0(n, 5, 11)
    _, traj, status = prob.solve(x0, eps_abs=1e-10, eps_rel=1e-10)
    xr, ur = tr.lqr_rollout_ld(A, B, None, Qs, Rs, x0)
    u = np.asarray(traj.uTraj)
    err = np.max(np.abs(u - ur.astype(np.float64)), axis=(1, 2))
    tol = 1e-7 * np.maximum(1.0, np.max(np.abs(ur.astype(np.float64)), axis=(1, 2)))
    print(f"lti_unstable ({n},{m},{N}): status {list(status)}, iterations {prob.last_iterations}, |u - u_lqr| {err} (tolerance {tol})")
    assert np.all(status == "optimal")
    assert np.all(err <= tol)


def test_unbounded_ltvmpc_on_the_unstable_family_equals_affine_lqr(gpu):
    """ltvMpc on `unstable` at (12, 4, 75): stage-varying A_k (every stage at spectral radius 1.3), B_k, c_k != 0 and stage weights,
    no box, eps 1e-10 -- against the long-double affine LQR rollout, same tolerance."""
    from zopt_amd import mpcUtils
    n, m, N = 12, 4, 75
    A, B, c, Qs, Rs, _ = (X[0] for X in problems.hard_mpc("unstable", n, m, N))
    inf_n, inf_m = np.full(n, np.inf), np.full(m, np.inf)
    prob = mpcUtils.ltvMpc(A, B, np.concatenate([Qs[:1], Qs]), Rs, N, -inf_n, inf_n, -inf_m, inf_m, c=c, stage_varying=("Q", "R"))
    x0 = _x0(n, 5, 12)
    _, traj, status = prob.solve(x0, eps_abs=1e-10, eps_rel=1e-10)
    xr, ur = tr.lqr_rollout_ld(A, B, c, Qs, Rs, x0)
    u = np.asarray(traj.uTraj)
    err = np.max(np.abs(u - ur.astype(np.float64)), axis=(1, 2))
    tol = 1e-7 * np.maximum(1.0, np.max(np.abs(ur.astype(np.float64)), axis=(1, 2)))
    print(f"unstable ({n},{m},{N}) ltvMpc: status {list(status)}, iterations {prob.last_iterations}, |u - u_lqr| {err} (tolerance {tol})")
    assert np.all(status == "optimal")
    assert np.all(err <= tol)


# ---- nonsymmetric weights are their symmetric parts, bit for bit ----------------------------------------------------------------------------

def _anti(rng, shape, scale=0.3):
    S = scale * rng.standard_normal(shape)
    return S - np.swapaxes(S, -1, -2)


def _sym(W):
    return 0.5 * (W + np.swapaxes(W, -1, -2))


def _plain(a):
    a = np.asarray(a)
    return a.astype(str) if a.dtype == object else a


def _same(a, b, at):
    (ua, ta, sa), (ub, tb, sb) = a, b
    assert np.array_equal(np.asarray(sa, dtype=str), np.asarray(sb, dtype=str)), at
    assert np.array_equal(np.asarray(ua), np.asarray(ub)) and np.array_equal(np.asarray(ta.xTraj), np.asarray(tb.xTraj)), at
    assert np.array_equal(np.asarray(ta.uTraj), np.asarray(tb.uTraj)), at


def test_nonsymmetric_weights_of_lqrmpc_are_their_symmetric_parts(gpu):
    """Q + S, R + S', Qf + S'' with O(1) antisymmetric S: solve, tracking with references and a three-step simulate return bit for bit
    what the symmetric parts return (the setup forms 2 W, the tracking kernels W + W': only a symmetric W makes them one Hessian)."""
    from tests import mpc_tracking_ref as trk
    from zopt_amd import mpcUtils
    n, m, N, nb = 4, 2, 8, 5
    (A, B, Q, R, Qf, xl, xu, ul, uu), x0, xRef, uRef = trk.random_case(n, m, N, seed=41, nb=nb)
    rng = np.random.default_rng(77)
    Wq, Wr, Wf = Q + _anti(rng, (n, n)), R + _anti(rng, (m, m)), Qf + _anti(rng, (n, n))
    assert not np.array_equal(Wq, Wq.T) and not np.array_equal(Wr, Wr.T) and not np.array_equal(Wf, Wf.T)
    raw = mpcUtils.lqrMpc(A, B, Wq, Wr, N, xl, xu, ul, uu, Qf=Wf)
    sym = mpcUtils.lqrMpc(A, B, _sym(Wq), _sym(Wr), N, xl, xu, ul, uu, Qf=_sym(Wf))
    assert raw.rho == sym.rho
    kw = dict(eps_abs=1e-6, eps_rel=1e-6, max_iter=3000)
    ra, sa = raw.solve(x0, **kw), sym.solve(x0, **kw)
    _same(ra, sa, "solve")
    assert np.array_equal(raw.last_iterations, sym.last_iterations) and "optimal" in set(ra[2])
    rb, sb = raw.solve(x0, xRef=xRef, uRef=uRef, **kw), sym.solve(x0, xRef=xRef, uRef=uRef, **kw)
    _same(rb, sb, "tracking")
    assert np.array_equal(raw.last_iterations, sym.last_iterations) and "optimal" in set(rb[2])
    rc, sc = raw.simulate(x0, 3, **kw), sym.simulate(x0, 3, **kw)
    assert all(np.array_equal(_plain(a), _plain(b)) for a, b in zip(rc[:4], sc[:4])) and "optimal" in set(rc.status.reshape(-1))
    S = 3
    xR, uR = np.concatenate([xRef, xRef[:, -1:].repeat(S - 1, axis=1)], axis=1), np.concatenate([uRef, uRef[:, -1:].repeat(S - 1, axis=1)], axis=1)
    rd, sd = raw.simulate(x0, S, xRef=xR, uRef=uR, **kw), sym.simulate(x0, S, xRef=xR, uRef=uR, **kw)
    assert all(np.array_equal(_plain(a), _plain(b)) for a, b in zip(rd[:4], sd[:4])) and "optimal" in set(rd.status.reshape(-1))


@pytest.mark.parametrize("staged", [False, True])
def test_nonsymmetric_weights_of_ltvmpc_are_their_symmetric_parts(gpu, staged):
    """The same for ltvMpc, with one set of weights and with a stage axis on Q and R (every stage its own antisymmetric part), and for
    weights that `update` brings."""
    from tests import mpc_ltv_ref as lr
    from tests import mpc_tracking_ref as trk
    from zopt_amd import mpcUtils
    n, m, N, nb = 4, 2, 7, 5
    (A, B, c, Q, R, Qf, xl, xu, ul, uu), x0 = lr.recipe(n, m, N, nb)
    _, _, xRef, uRef = trk.random_case(n, m, N, seed=41, nb=nb)
    rng = np.random.default_rng(78)
    kw = dict(eps_abs=1e-6, eps_rel=1e-6, max_iter=3000)
    if staged:
        scale = 1.0 + 0.1 * np.arange(N + 1)
        Wq = Q * scale[:, None, None] + _anti(rng, (N + 1, n, n))
        Wr = R * scale[:N, None, None] + _anti(rng, (N, m, m))
        make = lambda q, r: mpcUtils.ltvMpc(A, B, q, r, N, xl, xu, ul, uu, c=c, stage_varying=("Q", "R"))      # noqa: E731
        raw, sym = make(Wq, Wr), make(_sym(Wq), _sym(Wr))
    else:
        Wq, Wr, Wf = Q + _anti(rng, (n, n)), R + _anti(rng, (m, m)), Qf + _anti(rng, (n, n))
        raw = mpcUtils.ltvMpc(A, B, Wq, Wr, N, xl, xu, ul, uu, Qf=Wf, c=c)
        sym = mpcUtils.ltvMpc(A, B, _sym(Wq), _sym(Wr), N, xl, xu, ul, uu, Qf=_sym(Wf), c=c)
    assert np.array_equal(raw.rho, sym.rho)
    ra, sa = raw.solve(x0, **kw), sym.solve(x0, **kw)
    _same(ra, sa, "solve")
    assert np.array_equal(raw.last_iterations, sym.last_iterations) and "optimal" in set(ra[2])
    rb, sb = raw.solve(x0, xRef=xRef, uRef=uRef, **kw), sym.solve(x0, xRef=xRef, uRef=uRef, **kw)
    _same(rb, sb, "tracking")
    assert np.array_equal(raw.last_iterations, sym.last_iterations) and "optimal" in set(rb[2])
    if staged:
        W2 = Wq * 1.5 + _anti(rng, (N + 1, n, n))
        raw.update(Q=W2)
        sym.update(Q=_sym(W2))
        _same(raw.solve(x0, warm_start=False, **kw), sym.solve(x0, warm_start=False, **kw), "update")
