"""CPU fuzz of the recorder (zopt_amd/tape.py) and of the host builds of the tape interpreter (tests/tape_shim.cpp, tape_cost_shim.cpp,
tape_con_shim.cpp around zopt_amd/csrc/tape_model.h, tape_cost.h, tape_con.h) on the random expressions of tests/tape_fuzz.py.

Per seed: the recording is faithful (the NumPy evaluator of the tape equals the callable behind the operator protocol bit for bit, NaN
included; liveness; the caps; the host interpreter equals the evaluator on the host build of trig.h bit for bit), the structural mask
is sound (every pair with a nonzero long-double second derivative at any of 8 points has both bits; no bit at or above n + m), and,
for the tame seeds, the host build's Dual and Hyper derivatives are within tape_fuzz's allowance of the long-double hyper-dual
reference, per output row.  No seed is skipped: a refused recording or a non-finite tame reference fails.
"""
import numpy as np
import pytest

from tests import model_hp_ref as hp
from tests import tape_fuzz as F
from tests import tape_ref as R
from tests import traced_con_ref as CR
from tests import traced_cost_ref as TR
from tests import trig_host
from zopt_amd import models, tape as T

LD = np.longdouble
N_SEEDS, N_COST_SEEDS, N_CON_SEEDS = 320, 64, 64
P = 8


def draw(seed):
    """(n, m, n_params, n_ops, family) of a seed: one seed in four is wild"""
    rng = np.random.default_rng([77, seed])
    return (int(rng.integers(1, 13)), int(rng.integers(1, 5)), int(rng.integers(0, 4)), int(rng.integers(3, 61)),
            "wild" if seed % 4 == 3 else "tame")


@pytest.fixture(scope="module")
def shims(tmp_path_factory):
    d = tmp_path_factory.mktemp("tape_fuzz_shims")
    trig = trig_host.build(d)
    return dict(model=R.build(d), cost=TR.build(d), con=CR.build(d), sc=R.Real(np.float64, lambda a: trig_host.sincos(trig, a)))


def check_recording(tape, f, x, u, p, controls, host_values, sc):
    """item 1 for one tape; host_values(x, u | None, p) -> (P, n_out) by the host build on double"""
    n, m = tape.n, tape.m
    uu = u if controls else None
    with np.errstate(all="ignore"):
        got = R.evaluate(tape, x, u, p)
        boxed = np.stack([F.boxed_call(f, x[i], None if uu is None else u[i], None if p is None else p[i]) for i in range(len(x))])
    assert got.shape == boxed.shape and np.array_equal(got, boxed, equal_nan=True)
    peak, writer = R.liveness(tape)
    assert peak == tape.n_slots or (not len(tape.code) and tape.n_slots == n + m + tape.n_params)
    code = tape.decode()
    for s in tape.outputs:
        if s >= n + m + tape.n_params:
            assert all(c[1] != s for c in code[writer[s] + 1:]), "an output slot is overwritten after its value was formed"
        else:
            assert s not in writer
    assert len(tape.code) <= T.MAX_INSTR and tape.n_slots <= T.MAX_SLOTS and len(tape.consts) <= T.MAX_CONSTS
    if not controls:                                     # no instruction reads a control slot
        for op, _, (ac, a), (bc, b) in code:
            assert ac or not n <= a < n + m
            assert op not in T._BINARY or bc or not n <= b < n + m
    with np.errstate(all="ignore"):
        want = R.evaluate(tape, x, u, p, num=sc)
    assert np.array_equal(host_values(x, uu, p), want, equal_nan=True)


def check_mask(tape, S, controls=True):
    """item 2: S (P, n_out, K, K) long-double second derivatives at tame points"""
    K = tape.n + tape.m
    assert tape.mask >> (K if controls else tape.n) == 0
    nz = (np.isfinite(S) & (S != 0)).any(axis=(0, 1))
    for a, b in zip(*np.nonzero(nz)):
        assert tape.mask >> a & 1 and tape.mask >> b & 1, f"pair ({a}, {b}) has a second derivative, mask {tape.mask:#x}"


@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_random_model(shims, seed):
    n, m, npar, n_ops, fam = draw(seed)
    f = F.random_callable(seed, n, m, n_ops, fam, npar)
    x, u, p = F.points(seed, n, m, P, npar, wild=fam == "wild")
    md = models.TracedModel(f, n, m, params=p)
    t = md.tape
    lib = shims["model"]
    with np.errstate(all="ignore"):
        for i in range(P):
            args = (x[i], u[i]) + (() if p is None else (p[i],))
            assert np.array_equal(np.asarray(md(*args), dtype=np.float64), np.asarray(f(*args), dtype=np.float64), equal_nan=True)
    check_recording(t, f, x, u, p, True, lambda xx, uu, pp: R.host_step(lib, t, xx, uu, pp), shims["sc"])
    xt, ut, pt = F.points(seed, n, m, P, npar)
    val, J, S = F.expand(f, n, m, xt, ut, pt)
    check_mask(t, S)
    if fam == "wild":
        return
    _, J64, S64 = F.expand(f, n, m, xt, ut, pt, dtype=np.float64)
    fh, Jh = R.host_jacobian(lib, t, xt, ut, pt)
    Hh = R.host_hessian(lib, t, xt, ut, pt)
    rJ, rH = F.ratio(Jh, J64, J), F.ratio(Hh, S64, S)
    print(f"seed {seed} ({n}, {m}, {npar}) {len(t.code)} instructions mask {t.mask:#x}: Jacobian error / allowance {rJ:.2e}, second {rH:.2e}")
    assert np.array_equal(fh, R.host_step(lib, t, xt, ut, pt))
    assert rJ <= 1.0 and rH <= 1.0
    K = n + m
    mk = np.array([t.mask >> k & 1 for k in range(K)], dtype=bool)
    assert not Hh[:, :, ~(mk[:, None] & mk[None, :])].any(), "an entry outside the mask"
    if K <= 5:                                           # HyperLD against sympy derivatives of the same expression
        Hs = R.sympy_hessian(f, n, m, xt, ut, pt, exact=True)
        assert hp.row_error(S, Hs) <= 1e-16


@pytest.mark.parametrize("seed", range(N_COST_SEEDS))
def test_random_cost(shims, seed):
    n, m, npar, n_ops, fam = draw(1000 + seed)
    run = F.random_callable(seed, n, m, n_ops, fam, npar, n_out=1)
    term = F.random_callable(seed, n, m, n_ops, fam, npar, n_out=1, controls=False)
    x, u, p = F.points(seed, n, m, P, npar, wild=fam == "wild")
    cost = models.TracedCost(run, term, n, m, params=p)
    lib = shims["cost"]
    xt, ut, pt = F.points(seed, n, m, P, npar)
    for tape, fn, controls in ((cost.running_tape, run, True), (cost.terminal_tape, term, False)):
        assert len(tape.outputs) == 1
        check_recording(tape, fn, x, u, p, controls, lambda xx, uu, pp: TR.host_value(lib, tape, xx, uu, pp)[:, None], shims["sc"])
        uc = ut if controls else None
        val, J, S = F.expand(fn, n, m, xt, uc, pt, controls=controls)
        check_mask(tape, S, controls)
        if fam == "wild":
            continue
        _, J64, S64 = F.expand(fn, n, m, xt, uc, pt, dtype=np.float64, controls=controls)
        g = TR.host_gradient(lib, tape, xt, uc, pt)[:, None, :]
        H = TR.host_hessian(lib, tape, xt, uc, pt)[:, None]
        rg, rH = F.ratio(g, J64, J), F.ratio(H, S64, S)
        print(f"cost seed {seed} ({n}, {m}, {npar}) {'running' if controls else 'terminal'} mask {tape.mask:#x}: gradient {rg:.2e}, Hessian {rH:.2e}")
        assert rg <= 1.0 and rH <= 1.0
        mk = np.array([tape.mask >> k & 1 for k in range(n + m)], dtype=bool)
        assert not H[:, :, ~(mk[:, None] & mk[None, :])].any() and (controls or not g[:, :, n:].any())


@pytest.mark.parametrize("seed", range(N_CON_SEEDS))
def test_random_constraint(shims, seed):
    n, m, npar, n_ops, fam = draw(2000 + seed)
    nc, nct = 1 + seed % models.TRACEDCON_MAX, 1 + (seed // 8) % models.TRACEDCON_MAX
    g = F.random_callable(seed, n, m, n_ops, fam, npar, n_out=nc)
    term = F.random_callable(seed, n, m, n_ops, fam, npar, n_out=nct, controls=False)
    x, u, p = F.points(seed, n, m, P, npar, wild=fam == "wild")
    con = models.TracedConstraint(models.LinearModel(np.eye(n), np.ones((n, m))), g, nc, term, nct, params=p)
    lib = shims["con"]
    xt, ut, pt = F.points(seed, n, m, P, npar)
    for tape, fn, controls, rows in ((con.stage_tape, g, True, nc), (con.terminal_tape, term, False, nct)):
        assert len(tape.outputs) == rows
        check_recording(tape, fn, x, u, p, controls, lambda xx, uu, pp: CR.host_value(lib, tape, xx, uu, pp), shims["sc"])
        uc = ut if controls else None
        val, J, S = F.expand(fn, n, m, xt, uc, pt, controls=controls)
        check_mask(tape, S, controls)
        if fam == "wild":
            continue
        _, J64, _ = F.expand(fn, n, m, xt, uc, pt, dtype=np.float64, controls=controls)
        G = CR.host_jacobian(lib, tape, xt, uc, pt)
        rG = F.ratio(G, J64, J)
        print(f"constraint seed {seed} ({n}, {m}, {npar}) rows {rows} {'stage' if controls else 'terminal'}: Jacobian {rG:.2e}")
        assert rG <= 1.0 and (controls or not G[:, :, n:].any())


# ---- shaped callables: the mask is the one asked for, the slot count exact ------------------------------------------------------------
SHAPES = [((3, 2), ()), ((4, 1), range(5)), ((4, 2), range(6)), ((4, 3), range(7)), ((6, 2), range(8)), ((8, 3), range(11)),
          ((12, 4), range(16)), ((5, 4), (5, 6, 7, 8)), ((12, 4), (0, 5, 10, 15)), ((12, 4), (1, 3, 6, 8, 11, 13, 14))]


@pytest.mark.parametrize("shape,mask_bits", SHAPES)
def test_shaped_model_mask_is_exact(shims, shape, mask_bits):
    n, m = shape
    mask_bits = tuple(mask_bits)
    f = F.shaped_model(n, m, mask_bits)
    t = T.record(f, n, m)
    assert t.mask == F.bits(mask_bits)
    x, u, _ = F.points(5, n, m, P)
    check_recording(t, f, x, u, None, True, lambda xx, uu, pp: R.host_step(shims["model"], t, xx, uu), shims["sc"])
    val, J, S = F.expand(f, n, m, x, u)
    _, J64, S64 = F.expand(f, n, m, x, u, dtype=np.float64)
    check_mask(t, S)
    nz = (S != 0).all(axis=(0, 1))                       # every pair of the mask has a second derivative in every row
    mk = np.array([b in mask_bits for b in range(n + m)])
    assert np.array_equal(nz, mk[:, None] & mk[None, :])
    assert F.ratio(R.host_hessian(shims["model"], t, x, u), S64, S) <= 1.0 and F.ratio(R.host_jacobian(shims["model"], t, x, u)[1], J64, J) <= 1.0
    print(f"shaped ({n}, {m}) mask {t.mask:#x}: {t.n_slots} slots, regime {F.regime(t.mask, t.n_slots)}")


def test_shaped_slot_counts():
    """the plain form's slot counts, and the padding: 32 and 33 slots at every V that the device tests use, the same function"""
    assert T.record(F.shaped_model(12, 4, range(16)), 12, 4).n_slots == 28
    assert T.record(F.shaped_model(8, 3, range(11)), 8, 3).n_slots == 19
    assert T.record(F.shaped_model(4, 2, range(6)), 4, 2).n_slots == 10
    x, u, _ = F.points(6, 12, 4, P)
    base = F.shaped_model(12, 4, range(16))
    for slots in (32, 33):
        f = F.shaped_model(12, 4, range(16), n_slots=slots)
        t = T.record(f, 12, 4)
        assert t.n_slots == slots and t.mask == 0xFFFF and R.liveness(t)[0] == slots
        assert np.array_equal(R.evaluate(t, x, u), R.evaluate(T.record(base, 12, 4), x, u))
    for (n, m), mb in (((8, 3), range(11)), ((4, 2), range(6))):
        for slots in (32, 33):
            assert T.record(F.shaped_model(n, m, mb, n_slots=slots), n, m).n_slots == slots
    c, v = F.shaped_cost(6, 2, range(8), n_slots=32), F.shaped_terminal(6, 2, range(6), n_slots=20)
    tc, tv = T.record(c, 6, 2, n_out=1), T.record(v, 6, 2, n_out=1, controls=False)
    assert (tc.mask, tc.n_slots, tv.mask, tv.n_slots) == (0xFF, 32, 0x3F, 20)
