"""GPU checks of the traced-tape kernels (zopt_amd/csrc/traced.hip, traced_cost.hip, traced_con.hip) in every launch regime, on the
shaped and random callables of tests/tape_fuzz.py.

Regimes of traced_quadratic_kernel / traced_cost_hessian_kernel (derived here from the recorded tape by the launch's own formulas and
asserted, so that a change of the generator cannot move a case out of its regime): 16, 32 and 64 lanes per point; one, two and three
trips of the pair loop; the Hyper slot file in LDS and in private scratch, 32 and 33 slots on either side of the switch; V = 0; masks
with control bits only and with gaps; every combination of lanes per point of the running and the terminal cost.

Shapes: batch 5 x T 3 (15 points: a partial last wave at 4, 2 and 1 points per wave) and batch 1 x T 1.
Values are held bit for bit to the host build of the interpreter; derivatives per output row to tape_fuzz's allowance
max(FLOOR, 100 x the float64 hyper-dual evaluation's own error against long double); entries outside the mask are exactly 0.0.

Measured on an MI355X, worst error / allowance (Jacobians, second derivatives); none is above 0.5, the largest is 0.042:
    linear 0 / 0           full16 0.007 / 0.004     lpp32-lo 0.003 / 0.005    lpp32-hi 0.001 / 0.004    lds64 0.003 / 0.006
    two-trips 0.001 / 0.003    three-trips 0.002 / 0.008    slots32 0.001 / 0.002    slots33 0.001 / 0.002 (bit for bit slots32's)
    controls-only 0.010 / 0.012    sparse 0.011 / 0.010    sparse-32 0.009 / 0.010 (35 slots as recorded: lanes/point 32 on scratch)
    random V = 6, 7, 11, 12, 13, 14: 0.010 / 0.019, 0.010 / 0.015, 0.013 / 0.023, 0.013 / 0.017, 0.019 / 0.013, 0.016 / 0.014
    cost (lanes running, lanes terminal), gradients / Hessians: (16, 32) 0.004 / 0.004, (16, 64) 0.005 / 0.005, (32, 16) 0.002 / 0.003,
    (32, 32) 0.003 / 0.002, (32, 64) 0.001 / 0.002, (64, 16) 0.006 / 0.004, (64, 32) 0.003 / 0.002
    constraint penalty expansions, error / bound: (4, 2) 1 row 0.009, 8 rows 0.017; (12, 4) 1 row 0.032, 8 rows 0.042
"""
import ctypes
import types

import numpy as np
import pytest

from tests import tape_fuzz as F
from tests import tape_ref as R
from tests import traced_con_ref as CR
from tests import traced_cost_ref as TR

pytestmark = pytest.mark.gpu
LD = np.longdouble
SHAPES = ((5, 3), (1, 1))

@pytest.fixture(scope="module")
def mods():
    import torch
    assert torch.cuda.is_available()
    from zopt_amd import _lib, ilqrUtils, models, mpcUtils, pytrees
    return types.SimpleNamespace(ilqr=ilqrUtils, models=models, mpc=mpcUtils, pt=pytrees, lib=_lib)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("tape_fuzz_gpu_shims")
    return types.SimpleNamespace(model=R.build(d), cost=TR.build(d), con=CR.build(d))


def _trajectory(seed, b, N, n, m):
    rng = np.random.default_rng([53, seed, b, N, n, m])
    return F.X_SCALE * rng.standard_normal((b, N + 1, n)), F.X_SCALE * rng.standard_normal((b, N, m))


def _assemble(n, f_xx, f_ux, f_uu):
    """(P, rows, K, K) from the three blocks the kernels store; the block they do not store is f_ux transposed"""
    P, r = f_xx.shape[:2]
    m = f_uu.shape[-1]
    H = np.zeros((P, r, n + m, n + m))
    H[:, :, :n, :n], H[:, :, n:, :n], H[:, :, n:, n:], H[:, :, :n, n:] = f_xx, f_ux, f_uu, np.swapaxes(f_ux, -1, -2)
    return H


def _outside(mask, K):
    mk = np.array([mask >> k & 1 for k in range(K)], dtype=bool)
    return ~(mk[:, None] & mk[None, :])


# ---- a. values, bit for bit --------------------------------------------------------------------------------------------------------------
def _draw(seed):
    rng = np.random.default_rng([78, seed])
    return int(rng.integers(1, 13)), int(rng.integers(1, 5)), int(rng.integers(0, 4)), int(rng.integers(3, 61))


def test_wild_model_values_bit_for_bit(mods, host):
    nans = 0
    for seed in range(24):
        n, m, npar, n_ops = _draw(seed)
        f = F.random_callable(seed, n, m, n_ops, "wild", npar)
        x, u, p = F.points(seed, n, m, 67, npar, wild=True)
        md = mods.models.TracedModel(f, n, m, params=p)
        want = R.host_step(host.model, md.tape, x, u, p)
        assert np.array_equal(mods.mpc.modelStep(md, x, u), want, equal_nan=True), seed
        nans += int(np.isnan(want).any())
    assert nans >= 12


def test_wild_cost_values_bit_for_bit(mods, host):
    nans = 0
    for seed in range(8):
        n, m, npar, n_ops = _draw(100 + seed)
        run = F.random_callable(seed, n, m, n_ops, "wild", npar, n_out=1)
        term = F.random_callable(seed, n, m, n_ops, "wild", npar, n_out=1, controls=False)
        x, u, p = F.points(seed, n, m, 2 * 67, npar, wild=True)
        cost = mods.models.TracedCost(run, term, n, m, params=p[:67] if npar else None)
        traj = mods.pt.Trajectory(np.stack([x[:67], x[67:]], 1), u[:67, None, :])
        pp = p[:67] if npar else None
        with np.errstate(all="ignore"):
            want = TR.host_cost_of_trajectory(host.cost, cost, traj.xTraj, traj.uTraj, pp)
            assert np.array_equal(cost(traj), want, equal_nan=True), seed
            assert np.array_equal(cost(traj, 0), TR.host_value(host.cost, cost.running_tape, x[:67], u[:67], pp), equal_nan=True), seed
        nans += int(np.isnan(want).any())
    assert nans >= 4


def test_wild_constraint_values_bit_for_bit(mods, host):
    nans = 0
    for seed in range(8):
        n, m, npar, n_ops = _draw(200 + seed)
        nc, nct = (1, 8) if seed % 2 else (8, 3)
        g = F.random_callable(seed, n, m, n_ops, "wild", npar, n_out=nc)
        term = F.random_callable(seed, n, m, n_ops, "wild", npar, n_out=nct, controls=False)
        x, u, p = F.points(seed, n, m, 2 * 67, npar, wild=True)
        pp = p[:67] if npar else None
        con = mods.models.TracedConstraint(mods.models.LinearModel(np.eye(n), np.ones((n, m))), g, nc, term, nct, params=pp)
        gd, gT = con.values(np.stack([x[:67], x[67:]], 1), u[:67, None, :])
        want, wantT = CR.host_value(host.con, con.stage_tape, x[:67], u[:67], pp), CR.host_value(host.con, con.terminal_tape, x[67:], None, pp)
        assert np.array_equal(gd[:, 0], want, equal_nan=True) and np.array_equal(gT, wantT, equal_nan=True), seed
        nans += int(np.isnan(want).any() or np.isnan(wantT).any())
    assert nans >= 4


# ---- b. model expansions, one case per regime ---------------------------------------------------------------------------------------------
# id: (n, m), mask bits, n_slots asked for, (V, pairs, lanes per point, trips, slot file), slots expected (None: as recorded, in LDS)
REGIMES = {
    "linear": ((3, 2), (), None, (0, 0, 16, 0, "LDS"), None),
    "full16": ((4, 1), range(5), None, (5, 15, 16, 1, "LDS"), None),
    "lpp32-lo": ((4, 2), range(6), None, (6, 21, 32, 1, "LDS"), None),
    "lpp32-hi": ((4, 3), range(7), None, (7, 28, 32, 1, "LDS"), None),
    "lds64": ((6, 2), range(8), None, (8, 36, 64, 1, "LDS"), None),
    "two-trips": ((8, 3), range(11), None, (11, 66, 64, 2, "LDS"), None),
    "three-trips": ((12, 4), range(16), None, (16, 136, 64, 3, "LDS"), 28),
    "slots32": ((12, 4), range(16), 32, (16, 136, 64, 3, "LDS"), 32),
    "slots33": ((12, 4), range(16), 33, (16, 136, 64, 3, "scratch"), 33),
    "controls-only": ((5, 4), (5, 6, 7, 8), None, (4, 10, 16, 1, "LDS"), None),
    "sparse": ((12, 4), (0, 5, 10, 15), None, (4, 10, 16, 1, "LDS"), None),
    "sparse-32": ((12, 4), (1, 3, 6, 8, 11, 13, 14), None, (7, 28, 32, 1, "scratch"), 35),      # (as recorded: 35 slots)
}
# tame random (12, 4) models by the size of their recorded mask: seed, operations of the plan, V
RANDOM = {"random-V6": (6194, 60, 6), "random-V7": (7065, 60, 7), "random-V11": (21691, 150, 11), "random-V12": (22907, 150, 12),
          "random-V13": (20367, 150, 13), "random-V14": (21195, 150, 14)}
_RESULTS = {}


def _expansion(mods, host, name):
    """the device's expansions of a case at both shapes, checked; cached for the tests that compare cases"""
    if name in _RESULTS:
        return _RESULTS[name]
    if name in REGIMES:
        (n, m), mask_bits, ask, want, slots = REGIMES[name]
        f = F.shaped_model(n, m, tuple(mask_bits), ask)
    else:
        seed, n_ops, V = RANDOM[name]
        n, m = 12, 4
        f = F.random_callable(seed, n, m, n_ops, "tame")
    md = mods.models.TracedModel(f, n, m)
    t = md.tape
    reg = F.regime(t.mask, t.n_slots)
    if name in REGIMES:
        assert t.mask == F.bits(tuple(mask_bits)) and reg == want and (slots is None or t.n_slots == slots), (name, hex(t.mask), t.n_slots, reg)
    else:
        assert reg[0] == V and reg[2] == (32 if V < 8 else 64) and reg[3] == (1 if V < 11 else 2), (name, reg)
    K = n + m
    out = types.SimpleNamespace(regime=reg, slots=t.n_slots, rJ=0.0, rH=0.0, H=[], ok=True)
    for b, N in SHAPES:
        xT, uT = _trajectory(len(name), b, N, n, m)
        traj = mods.pt.Trajectory(xT, uT)
        a, q = mods.pt.AffineDynamics.from_trajectory(md, traj), mods.pt.QuadraticDynamics.from_trajectory(md, traj)
        x, u = xT[:, :-1].reshape(-1, n), uT.reshape(-1, m)
        fh = R.host_step(host.model, t, x, u)
        assert np.array_equal(a.f.reshape(-1, n), fh) and np.array_equal(q.f.reshape(-1, n), fh), name
        assert np.array_equal(a.f_x, q.f_x) and np.array_equal(a.f_u, q.f_u), name
        val, J, S = F.expand(f, n, m, x, u)
        _, J64, S64 = F.expand(f, n, m, x, u, dtype=np.float64)
        Jd = np.concatenate([q.f_x, q.f_u], -1).reshape(-1, n, K)
        Hd = _assemble(n, q.f_xx.reshape(-1, n, n, n), q.f_ux.reshape(-1, n, m, n), q.f_uu.reshape(-1, n, m, m))
        out.rJ, out.rH = max(out.rJ, F.ratio(Jd, J64, J)), max(out.rH, F.ratio(Hd, S64, S))
        off = _outside(t.mask, K)
        assert not Hd[:, :, off].any() and not np.signbit(Hd[:, :, off]).any(), (name, "an entry outside the mask is not +0.0")
        assert np.all(Hd[S.astype(np.float64) != 0] != 0), (name, "a zero where the reference has a second derivative")
        if name in REGIMES:                              # every pair of the mask, every row
            assert np.all(Hd[:, :, ~off] != 0), name
        out.H.append((Hd, S64, S))
    print(f"{name:14s} (n, m) = ({n}, {m})  mask {t.mask:#06x}  V {reg[0]:2d}  pairs {reg[1]:3d}  lanes/point {reg[2]}  trips {reg[3]}  "
          f"slots {t.n_slots} ({reg[4]})  worst error / allowance: Jacobians {out.rJ:.3f}, second derivatives {out.rH:.3f}")
    _RESULTS[name] = out
    return out


@pytest.mark.parametrize("name", list(REGIMES) + list(RANDOM))
def test_model_expansion_in_its_regime(mods, host, name):
    r = _expansion(mods, host, name)
    assert r.rJ <= 1.0 and r.rH <= 1.0, (name, r.rJ, r.rH)


def test_the_slot_file_switch_changes_nothing(mods, host):
    """32 slots (LDS) and 33 slots (private scratch): the same callable up to padding that adds 0.0 * t"""
    a, b = _expansion(mods, host, "slots32"), _expansion(mods, host, "slots33")
    assert a.regime[4] == "LDS" and b.regime[4] == "scratch"
    for (Ha, S64, S), (Hb, _, _) in zip(a.H, b.H):
        e = F.row_errors(Ha, Hb.astype(LD)) / F.allowance(S64, S)[None, :]
        print(f"slots32 against slots33: bit for bit {np.array_equal(Ha, Hb)}, worst difference / allowance {e.max():.3f}")
        assert e.max() <= 1.0


# ---- c. list and active forms ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lpp32-lo", "two-trips"])
def test_list_forms_touch_only_listed_active_trajectories(mods, name):
    import torch
    (n, m), mask_bits, ask, want, _ = REGIMES[name]
    md = mods.models.TracedModel(F.shaped_model(n, m, tuple(mask_bits), ask), n, m)
    assert F.regime(md.tape.mask, md.tape.n_slots) == want
    lib = mods.lib.lib()
    B, N = 5, 3
    xT, uT = (torch.as_tensor(a, device="cuda") for a in _trajectory(3, B, N, n, m))
    ms = mods.models.model_struct(md, (B,))
    pm = ctypes.addressof(ms)
    ids = torch.tensor([3, 0, 4], dtype=torch.int32, device="cuda")
    act = torch.ones(B, dtype=torch.int32, device="cuda")
    act[4] = 0
    shapes = {"f": (B, N, n), "f_x": (B, N, n, n), "f_u": (B, N, n, m), "f_xx": (B, N, n, n, n), "f_ux": (B, N, n, m, n), "f_uu": (B, N, n, m, m)}
    full = {k: torch.full(s, 7.0, dtype=torch.float64, device="cuda") for k, s in shapes.items()}
    part = {k: torch.full(s, 7.0, dtype=torch.float64, device="cuda") for k, s in shapes.items()}
    p = lambda t: t.data_ptr()                                                                                         # noqa: E731
    assert lib.zm_linearize_dynamics_f64(pm, p(xT), p(uT), None, p(full["f"]), p(full["f_x"]), p(full["f_u"]), B, N, None) == 0
    assert lib.zm_quadratic_dynamics_f64(pm, p(xT), p(uT), None, p(full["f_xx"]), p(full["f_ux"]), p(full["f_uu"]), B, N, None) == 0
    assert lib.zm_linearize_dynamics_list_f64(pm, p(xT), p(uT), p(ids), 3, p(act), p(part["f"]), p(part["f_x"]), p(part["f_u"]), B, N, None) == 0
    assert lib.zm_quadratic_dynamics_list_f64(pm, p(xT), p(uT), p(ids), 3, p(act), p(part["f_xx"]), p(part["f_ux"]), p(part["f_uu"]), B, N,
                                              None) == 0
    torch.cuda.synchronize()
    for k in shapes:
        assert not bool((full[k] == 7.0).any()), k
        for b in range(B):
            if b in (3, 0):
                assert torch.equal(part[k][b], full[k][b]), (name, k, b)
            else:
                assert bool((part[k][b] == 7.0).all()), (name, k, b)


# ---- d. cost expansions: every combination of lanes per point ----------------------------------------------------------------------------
# (lanes running, lanes terminal): (n, m), running mask bits, terminal mask bits -- the smallest n + m that reaches the combination
COST_REGIMES = {
    (16, 32): ((6, 1), (0, 6), range(6)),
    (16, 64): ((8, 1), (0, 8), range(8)),
    (32, 16): ((5, 1), range(6), (0,)),
    (32, 32): ((6, 1), range(7), range(6)),
    (32, 64): ((8, 1), (0, 1, 2, 3, 4, 5, 8), range(8)),
    (64, 16): ((7, 1), range(8), (2, 6)),
    (64, 32): ((6, 2), range(8), range(6)),
}


def _cost_case(mods, lanes):
    (n, m), rb, tb = COST_REGIMES[lanes]
    run, term = F.shaped_cost(n, m, tuple(rb)), F.shaped_terminal(n, m, tuple(tb))
    cost = mods.models.TracedCost(run, term, n, m)
    rt, tt = cost.running_tape, cost.terminal_tape
    slots = max(rt.n_slots, tt.n_slots)
    assert rt.mask == F.bits(tuple(rb)) and tt.mask == F.bits(tuple(tb)) and tt.mask >> n == 0
    assert (F.regime(rt.mask, slots)[2], F.regime(tt.mask, slots)[2]) == lanes and F.regime(rt.mask, slots)[4] == "LDS"
    return n, m, run, term, cost


@pytest.mark.parametrize("lanes", list(COST_REGIMES), ids=lambda l: f"{l[0]}-{l[1]}")
def test_cost_expansion_lanes_per_point(mods, host, lanes):
    from tests.test_traced_cost_gpu import _raw_expand
    n, m, run, term, cost = _cost_case(mods, lanes)
    K = n + m
    worst = [0.0, 0.0]
    for b, N in SHAPES:
        xT, uT = _trajectory(7, b, N, n, m)
        cs = cost.tcost_struct((b,))
        c, c_x, c_u, c_xx, c_ux, c_uu, v, v_x, v_xx = _raw_expand(mods.lib, cs, n, m, xT, uT)
        x, u, xf = xT[:, :-1].reshape(-1, n), uT.reshape(-1, m), xT[:, -1]
        assert np.array_equal(c.reshape(-1), TR.host_value(host.cost, cost.running_tape, x, u))
        assert np.array_equal(v, TR.host_value(host.cost, cost.terminal_tape, xf, None))
        for fn, tape, xx, uu, g, H in (
                (run, cost.running_tape, x, u, np.concatenate([c_x, c_u], -1).reshape(-1, 1, K),
                 _assemble(n, c_xx.reshape(-1, 1, n, n), c_ux.reshape(-1, 1, m, n), c_uu.reshape(-1, 1, m, m))),
                (term, cost.terminal_tape, xf, None, np.concatenate([v_x, np.zeros((b, m))], -1)[:, None, :],
                 _assemble(n, v_xx[:, None], np.zeros((b, 1, m, n)), np.zeros((b, 1, m, m))))):
            val, J, S = F.expand(fn, n, m, xx, uu, controls=uu is not None)
            _, J64, S64 = F.expand(fn, n, m, xx, uu, dtype=np.float64, controls=uu is not None)
            worst = [max(worst[0], F.ratio(g, J64, J)), max(worst[1], F.ratio(H, S64, S))]
            off = _outside(tape.mask, K)
            assert not H[:, :, off].any() and np.all(H[:, :, ~off] != 0), (lanes, "zero exactly outside the mask")
    print(f"cost lanes/point (running, terminal) = {lanes}  (n, m) = ({n}, {m}): worst error / allowance gradients {worst[0]:.3f}, "
          f"Hessians {worst[1]:.3f}")
    assert worst[0] <= 1.0 and worst[1] <= 1.0


def test_cost_expansion_list_form(mods):
    from tests.test_traced_cost_gpu import _raw_expand
    n, m, run, term, cost = _cost_case(mods, (32, 64))
    B, N = 5, 3
    xT, uT = _trajectory(8, B, N, n, m)
    cs = cost.tcost_struct((B,))
    act = np.ones(B, dtype=np.int32)
    act[4] = 0
    dense = _raw_expand(mods.lib, cs, n, m, xT, uT)
    part = _raw_expand(mods.lib, cs, n, m, xT, uT, ids=[3, 0, 4], act=act)
    for a, d in zip(part, dense):
        assert not (d == 7.5).any()
        for i in range(B):
            assert np.array_equal(a[i], d[i]) if i in (3, 0) else np.all(a[i] == 7.5), i


# ---- e. constraint expansions ------------------------------------------------------------------------------------------------------------
def constraint_problem(seed, n, m, nc, nct, B=5, N=3):
    """random tame g and terminal rows, a trajectory, multipliers and penalties; the long-double and float64 addends of the penalty
    expansion per trajectory (tests/test_traced_con_gpu.py's construction, with the hyper-dual Jacobians of the callables)"""
    g = F.random_callable(seed, n, m, 40, "tame", n_out=nc)
    term = F.random_callable(seed, n, m, 40, "tame", n_out=nct, controls=False)
    xT, uT = _trajectory(seed, B, N, n, m)
    rng = np.random.default_rng([59, seed, n])

    def draw(shape):
        v = 10.0 ** rng.uniform(-2, 4, shape)
        v[rng.random(shape) < 1 / 3] = 0.0
        return v
    lam, lamT, mu = draw((B, N, nc)), draw((B, nct)), rng.permutation(10.0 ** np.linspace(0, 4, B))
    refs = []
    for b in range(B):
        per = []
        for dt in (LD, np.float64):
            gv, G, _ = F.expand(g, n, m, xT[b, :-1], uT[b], dtype=dt)
            tv, GT, _ = F.expand(term, n, m, xT[b, -1:], None, dtype=dt, controls=False)
            if dt is LD:
                s = np.concatenate([(lam[b] + mu[b] * gv).ravel(), (lamT[b] + mu[b] * tv[0]).ravel()]).astype(np.float64)
                size = np.concatenate([(lam[b] + mu[b] * np.abs(gv)).ravel(), (lamT[b] + mu[b] * np.abs(tv[0])).ravel()]).astype(np.float64)
                assert np.all((np.abs(s) >= 1e-9 * np.maximum(size, 1e-300)) | (size == 0)), (seed, b, "a row on the edge of activity: reseed")
            per.append(CR.addends(gv, G, lam[b].astype(dt), dt(mu[b])) + CR.addends(tv[0], GT[0][:, :n], lamT[b].astype(dt), dt(mu[b])))
        refs.append(per)
    assert sum(bool(r[0][1].any()) for r in refs) >= 3 and sum(bool(r[0][3].any()) for r in refs) >= 3, "too few active rows: reseed"
    return g, term, xT, uT, lam, lamT, mu, refs


CON_CASES = {"4x2-1row": (30, 4, 2, 1, 8), "4x2-8rows": (30, 4, 2, 8, 8), "12x4-1row": (30, 12, 4, 1, 8), "12x4-8rows": (30, 12, 4, 8, 8)}


@pytest.mark.parametrize("name", list(CON_CASES))
def test_penalty_expansion_of_random_constraints(mods, name):
    from tests.test_traced_con_gpu import _expand, _row_bound
    seed, n, m, nc, nct = CON_CASES[name]
    g, term, xT, uT, lam, lamT, mu, refs = constraint_problem(seed, n, m, nc, nct)
    B, N = uT.shape[:2]
    K = n + m
    con = mods.models.TracedConstraint(mods.models.LinearModel(np.eye(n), np.ones((n, m))), g, nc, term, nct)
    c = types.SimpleNamespace(n=n, m=m, T=N)
    zero_sh = (np.zeros((n, n)), np.zeros((m, n)), np.zeros((m, m)), np.zeros((n, n)))
    zero_pre = (np.zeros((B, N, n)), np.zeros((B, N, m)), np.zeros((B, n)))
    (gx, gu, gv), (Hxx, Hux, Huu, Hv) = _expand((mods.ilqr, mods.models, mods.pt, mods.lib), c, con, xT, uT, lam, lamT, mu, zero_sh, zero_pre)
    worst = 0.0
    for b in range(B):
        (grad, H, gradT, HT), (grad64, H64, gradT64, HT64) = refs[b]
        dev_H = _assemble(n, Hxx[b][:, None], Hux[b][:, None], Huu[b][:, None])[:, 0]
        for dv, ld, f64 in ((np.concatenate([gx[b], gu[b]], -1), grad, grad64), (dev_H, H, H64), (gv[b], gradT, gradT64), (Hv[b], HT, HT64)):
            bound = _row_bound(ld, f64)
            err = np.abs(dv.astype(LD) - ld).astype(np.float64)
            assert np.all(err <= bound), (name, b, float(np.max(err / np.maximum(bound, 1e-300))))
            worst = max(worst, float(np.max(np.where(bound > 0, err / np.maximum(bound, 1e-300), 0.0))))
    print(f"constraint {name}: worst error / bound {worst:.3f}")
