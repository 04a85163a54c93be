"""The forward half of every iLQR / DDP iteration -- the rollouts of the 16 step sizes, the cost J of each and the choice of the winner
(forwardPass2, K6) -- in every form reachable through the public C ABI and the Python layer, against the long-double reference of
tests/linesearch_hp_ref.py on its hard families, and bit for bit on its exact families.

Forms: the fast one-lane kernel (rollout_fast.hip: general weights, diagonal weights by the flag and by the in-kernel ballot), the
generic lane-per-rollout kernel (rollout.hip: other shapes, 2..15 step sizes at (12, 4), and (12, 4) with
ZOPT_AMD_ROLLOUT_PATH=generic in a child process), the wide kernel at every NP (rollout_wide.hip), the list forms with `active`, the
quadcopter's two-pass search with the four-lane re-roll (rollout_quad.hip) and -- in a child on the lab library with
ZOPT_AMD_ROLLOUT_QUAD=0 -- its one-kernel form, the quadcopter with general weights, the tracking cost on the fast and the generic
kernel (references per step, per trajectory with step stride 0, one shared row), and ilqrUtils.forwardPass2 on top.  For every form
the 16 costs are obtained once more by 16 calls with one step size each.

The all-store line search is reachable only from inside the solvers; it stays held by tests/test_ilqr_tail_gpu.py (bit-identical
solves for every switch-over between the two forms) and gets no entry point here.

Metric, bounds and the candidate-set rule: tests/linesearch_hp_ref.py (everything derives from the fp64 oracle's own error against
long double, x 100, floor 100 x 2^-52; computed on the CPU at test time, never from a kernel).  tests/test_linesearch_hp_ref.py holds
the conditions: every choice determined (near_tie: exactly two adjacent candidates), the oracle alone passes, planted errors fail.
Each check prints its worst error-to-bound ratio; DESIGN.md section 3.4 has the table.

The exact families assert the non-finite classes NaN, +inf and -inf on linear models; on the quadcopter (no exact arithmetic: sines
and cosines) ties and NaNs are held against the kernel's own 16 single-step-size costs, which the same kernel computes bit for bit."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import linesearch_hp_ref as ls

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAB = os.path.join(ROOT, "zopt_amd", "csrc", "libzopt_amd_lab.so")
CHILD = os.path.join(ROOT, "tests", "linesearch_hard_child.py")


class Device:
    """the line search through the C ABI: zm_rollout_linesearch[_tracking][_list]_f64"""

    def __init__(self):
        import torch
        assert torch.cuda.is_available()
        from zopt_amd import _lib, ilqrUtils, models, pytrees
        self.torch, self.lib, self.models, self.ilqr, self.pt = torch, _lib, models, ilqrUtils, pytrees

    def dev(self, a, dtype=np.float64):
        return self.torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device="cuda")

    def model(self, p):
        return self.models.LinearModel(p.A, p.B) if p.kind == "linear" else self.models.QuadcopterEuler(p.dt)

    def cost(self, p):
        if p.tracking:
            return self.models.TrackingCost(p.Q, p.R, p.Qf, p.xRef, p.uRef)
        return self.models.QuadraticCost(p.Q, p.R, p.Qf)

    def run(self, p, alphas=None, diagonal=None, lst=None, active=None, fill=float("nan")):
        """(xTraj, uTraj, J, idx); diagonal: force zm_quadcost_t.diagonal; lst / active: the list form; fill: what the outputs hold before"""
        torch = self.torch
        al = p.alphas if alphas is None else np.asarray(alphas, dtype=np.float64)
        model, cost = self.model(p), self.cost(p)
        md = model.c_struct()
        cs = cost.track_struct((p.b,), p.N) if p.tracking else cost.c_struct()
        if diagonal is not None:
            cs.diagonal = diagonal
        ins = [self.dev(X) for X in (p.x0, p.l, p.L, p.xPrev, p.uPrev)]
        dal = self.dev(al)
        xT = torch.full((p.b, p.N + 1, p.n), fill, dtype=torch.float64, device="cuda")
        uT = torch.full((p.b, p.N, p.m), fill, dtype=torch.float64, device="cuda")
        J = torch.full((p.b,), fill, dtype=torch.float64, device="cuda")
        idx = torch.full((p.b,), -1, dtype=torch.int32, device="cuda")
        dact = None if active is None else self.dev(active, np.int32)
        head = [ctypes.addressof(md), ctypes.addressof(cs)] + [t.data_ptr() for t in ins] + [dal.data_ptr(), len(al)]
        tail = [None if dact is None else dact.data_ptr(), xT.data_ptr(), uT.data_ptr(), J.data_ptr(), idx.data_ptr(), p.b, p.N, None]
        lib = self.lib.lib()
        if lst is None:
            fn = lib.zm_rollout_linesearch_tracking_f64 if p.tracking else lib.zm_rollout_linesearch_f64
            rc = fn(*head, *tail)
        else:
            dl = self.dev(lst, np.int32)
            fn = lib.zm_rollout_linesearch_tracking_list_f64 if p.tracking else lib.zm_rollout_linesearch_list_f64
            rc = fn(*head, dl.data_ptr(), len(lst), *tail)
        self.lib.check(rc, "rollout")
        torch.cuda.synchronize()
        return xT.cpu().numpy(), uT.cpu().numpy(), J.cpu().numpy(), idx.cpu().numpy()

    def costs16(self, p, **kw):
        """(n_alpha, b): the cost of every step size from a call of its own with n_alpha = 1"""
        return np.stack([self.run(p, alphas=p.alphas[a:a + 1], **kw)[2] for a in range(len(p.alphas))])


@pytest.fixture(scope="module")
def dev():
    return Device()


# ---- the checks, as plain functions: the child processes run them too ---------------------------------------------------------------
def check_key(dev, key, **kw):
    p = ls.problem(*key)
    if key[0] == "linear" and key[1] == "one_offdiag" and not p.tracking:
        assert dev.cost(p).c_struct().diagonal == int(key[6] == "none"), ls.key_id(key)
    xT, uT, J, idx = dev.run(p, **kw)
    return ls.check(ls.reference(p), xT, uT, J, idx, dev.costs16(p, **kw), what=ls.key_id(key) + (f" {kw}" if kw else "")), idx


def check_form_shape(dev, form, shape, **kw):
    keys = [k for k in ls.form_cases(form) if k[2:6] == tuple(shape)]
    assert keys
    for key in keys:
        check_key(dev, key, **kw)


def check_exact(dev, n, m, n_alpha=16, ref=None):
    cases = ls.EXACT_CASES if n_alpha == 16 else ls.EXACT_SHORT
    for case in cases:
        p = ls.exact_problem(case, n, m, n_alpha=n_alpha, ref=ref)
        xT, uT, J, idx = dev.run(p)
        assert np.all((idx >= 0) & (idx < n_alpha)), (case, idx)
        ls.check_exact(p, xT, uT, J, idx, what=f"{case} ({n}, {m}) n_alpha={n_alpha} ref={ref}")


def check_quad(dev, key):
    """a quadcopter case: at least quad_required trajectories compared (fewer: the test fails), more than one winner among them"""
    p = ls.problem(*key)
    ref = ls.reference(p)
    count = int(ref.comparable.sum())
    print(f"{ls.key_id(key)}: {count} of {p.b} trajectories compared")
    assert count >= ls.quad_required(key[1], key[2]), (ls.key_id(key), count)
    assert dev.cost(p).c_struct().diagonal == int(key[3])
    _, idx = check_key(dev, key)
    assert len(set(idx[ref.comparable].tolist())) > 1, idx


def check_quad_ties_and_nans(dev, diagonal):
    """the quadcopter's line search against the kernel's own single-step-size costs, bit for bit: equal costs, repeated step sizes,
    NaN at index 9, NaN at 5 and 11 -- the winner is np.argmin of the 16 costs (NaN is the minimum, the first index wins)"""
    base = ls.problem("quad", "nominal", 3, diagonal)
    flat, big = base.rows(np.arange(base.b)), base.rows(np.arange(base.b))
    flat.l = np.zeros_like(base.l)
    big.l = np.where(base.l < 0, -1e10, 1e10)        # 2^1000 l overflows: u = +-inf, the next step's sines and cosines are NaN
    rep = ls.ALPHAS[[4, 2, 4, 2, 6, 2, 9, 4, 6, 6, 2, 9, 4, 2, 9, 6]]
    nan9, nan511 = ls.ALPHAS.copy(), ls.ALPHAS.copy()
    nan9[9], nan511[[5, 11]] = ls.OVER, ls.OVER
    for what, p, expect, nans in (("l = 0", flat, 0, []), ("one step size 16 times", base.with_alphas(np.full(16, 0.25)), 0, []),
                                  ("repeated step sizes", base.with_alphas(rep), None, []), ("NaN at 9", big.with_alphas(nan9), 9, [9]),
                                  ("NaN at 5 and 11", big.with_alphas(nan511), 5, [5, 11])):
        xT, uT, J, idx = dev.run(p)
        J16 = dev.costs16(p)
        assert np.flatnonzero(np.isnan(J16).any(axis=1)).tolist() == nans and np.isnan(J16[nans]).all(), (what, J16)
        assert np.array_equal(idx, np.argmin(J16, axis=0)), (what, idx, np.argmin(J16, axis=0))
        if expect is not None:
            assert np.all(idx == expect), (what, idx)
        else:
            first = np.array([int(np.flatnonzero(p.alphas == p.alphas[k])[0]) for k in idx])
            assert np.array_equal(idx, first) and len(set(idx.tolist())) > 1, (what, idx)
        assert np.array_equal(J, J16[idx, np.arange(p.b)], equal_nan=True), what
        for a in sorted(set(idx.tolist())):
            x1, u1, _, _ = dev.run(p, alphas=p.alphas[a:a + 1])
            assert np.array_equal(xT[idx == a], x1[idx == a], equal_nan=True) and np.array_equal(uT[idx == a], u1[idx == a], equal_nan=True), (what, a)


def check_list(dev, shape):
    """the list forms: a shuffled strict subset, one listed trajectory inactive; unlisted and inactive rows keep the sentinel"""
    n, m, N, b = shape
    lst = np.array([7, 2, 5, 0, 3, 8] if b == 9 else [4, 1, 3])
    off = 5 if b == 9 else 1
    active = np.ones(b, dtype=np.int32)
    active[off] = 0
    rows = np.array(sorted(set(lst.tolist()) - {off}))
    rest = np.array(sorted(set(range(b)) - set(rows.tolist())))
    for key in [k for k in ls.form_cases("list") if k[2:6] == tuple(shape)]:
        p = ls.problem(*key)
        xT, uT, J, idx = dev.run(p, lst=lst, active=active, fill=-7.0)
        assert np.all(xT[rest] == -7.0) and np.all(uT[rest] == -7.0) and np.all(J[rest] == -7.0) and np.all(idx[rest] == -1), ls.key_id(key)
        q = p.rows(rows)
        ls.check(ls.Reference(q), xT[rows], uT[rows], J[rows], idx[rows], dev.costs16(q), what="listed " + ls.key_id(key))


def check_python(dev, key):
    """ilqrUtils.forwardPass2 returns the C ABI's results bit for bit"""
    p = ls.problem(*key)
    xT, uT, J, _ = dev.run(p)
    traj, Jp = dev.ilqr.forwardPass2(p.x0, dev.model(p), dev.cost(p), dev.pt.AffinePolicy(p.l, p.L), dev.pt.Trajectory(p.xPrev, p.uPrev))
    assert np.array_equal(np.asarray(traj.xTraj), xT) and np.array_equal(np.asarray(traj.uTraj), uT) and np.array_equal(np.asarray(Jp), J), ls.key_id(key)


def child(mode):
    """python tests/linesearch_hard_child.py MODE, with the environment of `_child` below"""
    dev = Device()
    if mode == "generic":         # ZOPT_AMD_ROLLOUT_PATH=generic: (12, 4) on the lane-per-rollout kernel, 16 and 1 step sizes
        check_form_shape(dev, "generic", (12, 4, 7, 5))
        check_exact(dev, 12, 4)
        for ref in ("zero", "exact"):
            check_exact(dev, 12, 4, ref=ref)
        for key in [k for k in ls.form_cases("track") if k[2:6] == (12, 4, 7, 5)]:
            check_key(dev, key)
        check_quad(dev, ("quad", "nominal", 3, False))
    elif mode == "noquad":        # lab library, ZOPT_AMD_ROLLOUT_QUAD=0: the quadcopter's search in one kernel
        for key in ls.quad_cases():
            if key[3]:
                check_quad(dev, key)
        check_quad_ties_and_nans(dev, True)
    else:
        raise SystemExit(f"unknown mode {mode}")
    print("LINESEARCH-CHILD-OK")


def _child(mode, env):
    r = subprocess.run([sys.executable, CHILD, mode], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600, cwd=ROOT)
    print(r.stdout)
    assert r.returncode == 0 and "LINESEARCH-CHILD-OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


# ---- the tests --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ls.FORM_SHAPES["fast"] + [ls.UNSTABLE_LONG], ids=str)
def test_fast_kernel_general_weights(dev, shape):
    """rollout_ls_fast_kernel (LinearModel at (12, 4)), 16 step sizes and one; every family at every horizon remainder of its
    four-step loop; `unstable` also at T = 30 with 67 trajectories"""
    check_form_shape(dev, "fast", shape)


@pytest.mark.parametrize("shape", ls.FORM_SHAPES["fast_diag"], ids=str)
def test_fast_kernel_diagonal_weights_by_flag_and_by_ballot(dev, shape):
    """diagonal weights with zm_quadcost_t.diagonal = 1 (only the diagonal path is compiled in) and = 0 (the kernel's ballot over its
    off-diagonal scan finds it): both pass, and agree bit for bit"""
    for key in [k for k in ls.form_cases("fast_diag") if k[2:6] == tuple(shape)]:
        outs = []
        for flag in (1, 0):
            check_key(dev, key, diagonal=flag)
            outs.append(dev.run(ls.problem(*key), diagonal=flag))
        assert all(np.array_equal(a, b) for a, b in zip(*outs)), ls.key_id(key)


@pytest.mark.parametrize("shape", [s for s in ls.FORM_SHAPES["generic"] if s[:2] != (12, 4)], ids=str)
def test_generic_kernel(dev, shape):
    check_form_shape(dev, "generic", shape)


@pytest.mark.parametrize("n_alpha", [2, 3, 5, 15])
def test_generic_kernel_with_dead_lanes(dev, n_alpha):
    """2..15 step sizes: the lanes beyond n_alpha carry the sentinel (+inf, index 16); also at (12, 4), which the fast path takes only
    with 16 or 1.  Hard families on the first n_alpha step sizes, and the NaN / all-+inf cases: idx < n_alpha always"""
    for n, m, N, b in ((5, 3, 7, 5), (12, 4, 7, 5)):
        for fam in ("index_j", "permuted", "nonsymmetric", "near_tie"):
            p = ls.problem("linear", fam, n, m, N, b, None, None, 0)
            q = p.with_alphas(p.alphas[:n_alpha])
            xT, uT, J, idx = dev.run(q)
            assert np.all((idx >= 0) & (idx < n_alpha)), idx
            ls.check(ls.Reference(q), xT, uT, J, idx, dev.costs16(q), what=f"{q.name} n_alpha={n_alpha}")
        check_exact(dev, n, m, n_alpha=n_alpha)


def test_generic_kernel_at_12_4_in_a_child_process(dev):
    """ZOPT_AMD_ROLLOUT_PATH=generic is read once per process: every family, the exact families and the tracking cost at (12, 4) on the
    lane-per-rollout kernels, and the quadcopter with general weights"""
    _child("generic", {"ZOPT_AMD_ROLLOUT_PATH": "generic"})


@pytest.mark.parametrize("shape", ls.FORM_SHAPES["wide"], ids=str)
def test_wide_kernel(dev, shape):
    """rollout_wide.hip at NP = 16, 32, 48 and 64, n and m at and off the tile sizes"""
    check_form_shape(dev, "wide", shape)


@pytest.mark.parametrize("shape", ls.FORM_SHAPES["list"], ids=str)
def test_list_forms_with_active(dev, shape):
    check_list(dev, shape)


@pytest.mark.parametrize("fam", ls.hp.FAMILIES)
@pytest.mark.parametrize("N", ls.QUAD_HORIZONS)
def test_quadcopter_two_pass_search_and_general_weights(dev, fam, N):
    """diagonal weights: the line-search kernel names the winners, rollout_quad_reroll_kernel re-rolls them on four lanes; general
    (nonsymmetric) weights: the fast kernel's general path.  l of trajectory i is scaled by 2^(i mod 16)"""
    check_quad(dev, ("quad", fam, N, True))
    check_quad(dev, ("quad", fam, N, False))


def test_quadcopter_ties_and_nans(dev):
    check_quad_ties_and_nans(dev, True)
    check_quad_ties_and_nans(dev, False)


def test_quadcopter_one_kernel_form_in_a_child_process(dev):
    """ZOPT_AMD_ROLLOUT_QUAD=0 (a kernel-lab switch: the lab build of the library): the winners' re-roll inside the line-search kernel"""
    assert os.path.exists(LAB)
    _child("noquad", {"ZOPT_AMD_LIB": LAB, "ZOPT_AMD_ROLLOUT_QUAD": "0"})


@pytest.mark.parametrize("shape", ls.FORM_SHAPES["track"], ids=str)
def test_tracking_cost(dev, shape):
    """zm_rollout_linesearch_tracking_f64 on the fast kernel ((12, 4)) and the generic one ((8, 4)): references ~1e6 from the origin,
    the state within a few units of them; xRef / uRef per step, per trajectory with step stride 0, one shared row"""
    check_form_shape(dev, "track", shape)


def test_tracking_cost_list_form(dev):
    p = ls.problem("linear", "index_j", 12, 4, 7, 5, None, "step", 0)
    lst, active = np.array([4, 1, 3]), np.array([1, 0, 1, 1, 1], dtype=np.int32)
    xT, uT, J, idx = dev.run(p, lst=lst, active=active, fill=-7.0)
    assert np.all(xT[[0, 1, 2]] == -7.0) and np.all(uT[[0, 1, 2]] == -7.0) and np.all(J[[0, 1, 2]] == -7.0) and np.all(idx[[0, 1, 2]] == -1)
    q = p.rows(np.array([3, 4]))
    ls.check(ls.Reference(q), xT[[3, 4]], uT[[3, 4]], J[[3, 4]], idx[[3, 4]], dev.costs16(q), what="listed tracking")


@pytest.mark.parametrize("form,n,m", [("fast", 12, 4), ("generic", 5, 3), ("wide", 17, 3), ("wide", 33, 5)])
def test_exact_families(dev, form, n, m):
    """bit for bit against the fp64 oracle and the winner known by construction: equal costs, repeated step sizes, a zero step size,
    NaN at 9 / at 5 and 11 / at 7 with -inf at 2, +inf everywhere but 13 / everywhere, -inf at 5 and 9"""
    check_exact(dev, n, m)


@pytest.mark.parametrize("n,m", [(12, 4), (5, 3)])
@pytest.mark.parametrize("ref", ["zero", "exact"])
def test_exact_families_tracking(dev, n, m, ref):
    """the tracking kernels (fast and generic) with a zero reference and with one of small integers"""
    check_exact(dev, n, m, ref=ref)


@pytest.mark.parametrize("key", [("linear", "index_j", 12, 4, 7, 5, None, None, 0), ("linear", "nonsymmetric", 33, 5, 6, 2, None, None, 0),
                                 ("linear", "index_j", 12, 4, 7, 5, None, "goal", 0), ("quad", "nominal", 3, True)], ids=ls.key_id)
def test_python_surface(dev, key):
    check_python(dev, key)
