"""Every refusal of the LQR family that is reached before the first HIP call: for the seven C entries the return code and the full
message, and -- where two checks are violated at once -- which of them wins; for the Python functions the ValueError text of the
shape checks, which run before the first device access.  CPU only: the library is called with dummy pointers, as
test_abi.py::test_bad_arguments_return_codes_without_gpu and test_mpc_refusals.py do; nothing here dereferences one.

Each C row is (entry, overrides of that entry's valid argument set, return code, zm_last_error()).  The valid set itself would go on
to the device, so every row breaks at least one check or returns early; a row with None as its message only pins the return code (an
early ZM_OK sets no message).  Rows that would launch or allocate are left out on purpose: zm_lqr_backward_f32 has no T*n*n bound
and zm_lqr_backward_host_f64 neither that bound nor one on the batch, so those sizes go on to the device there."""
import numpy as np
import pytest

from zopt_amd import _lib, lqrUtils

OK, EINVAL, EUNSUPPORTED = _lib.ZM_OK, _lib.ZM_EINVAL, _lib.ZM_EUNSUPPORTED
D = 0x1000          # a pointer that is never followed
P31 = 1 << 31       # the first batch that is refused as too large
NAN = float("nan")

# the parameters of every entry in ABI order, "name=value" of a valid call: batch 4, T = 3, shape (2, 1)
ENTRIES = {
    "zm_lqr_backward_f64": "A=D B=D Q=D R=D L=D batch=4 T=3 n=2 m=1 stream=None",
    "zm_lqr_backward_f32": "A=D B=D Q=D R=D L=D batch=4 T=3 n=2 m=1 stream=None",
    "zm_lqr_backward_host_f64": "A=D B=D Q=D R=D L=D batch=4 T=3 n=2 m=1",
    "zm_lqr_backward_affine_f64": "A=D B=D d=D Q=D R=D H=D q=D r=D L=D l=D batch=4 T=3 n=2 m=1 stream=None",
    "zm_dare_f64": "A=D B=D Q=D R=D L=D P=D iters=D batch=4 n=2 m=1 tol=1e-14 max_iter=100 stream=None",
    "zm_care_f64": "A=D B=D Q=D R=D K=D P=D info=D batch=4 n=2 m=1 tol=1e-14 max_iter=60 stream=None",
    "zm_riccati_ode_f64": "A_s=D B_s=D Rinv_s=D Q_s=D Qf=D V=D info=D batch=4 n=2 m=1 n_samples=1 N=5 T=1.0 rtol=1e-8 atol=1e-8 "
                          "max_steps=100 stream=None",
}
_NAMES = {"D": D, "None": None}


def _args(entry, over):
    vals = {}
    for item in ENTRIES[entry].split():
        k, v = item.split("=")
        vals[k] = _NAMES[v] if v in _NAMES else (float(v) if ("." in v or "e" in v) else int(v))
    assert set(over) <= set(vals), f"{entry} has no parameter {set(over) - set(vals)}"
    vals.update(over)
    return list(vals.values())


def _nulls(entry, names):
    return [(entry, {k: None}, EINVAL, f"{entry}: null pointer") for k in names.split()]


def _bad_size(entry, **over):
    """the sweeps' "bad size" message prints the four sizes"""
    v = {**dict(batch=4, T=3, n=2, m=1), **over}
    return (entry, over, EINVAL, f"{entry}: bad size batch={v['batch']} T={v['T']} n={v['n']} m={v['m']}")


F64, F32, HOST, AFF, DARE, CARE, ODE = ENTRIES
ROWS = [
    # ---- zm_lqr_backward_f64 ---------------------------------------------------------------------------------------------------
    (F64, dict(batch=0, A=None, B=None, Q=None, R=None, L=None), OK, None),
    (F64, dict(batch=0, T=0, n=0, m=99), OK, None),
    *_nulls(F64, "A B Q R L"),
    _bad_size(F64, batch=-1), _bad_size(F64, T=0), _bad_size(F64, T=-2), _bad_size(F64, n=0), _bad_size(F64, m=0),
    (F64, dict(n=65, m=16), EUNSUPPORTED, "zm_lqr_backward_f64: (n=65, m=16) not covered (need n<=64, m<=16)"),
    (F64, dict(n=12, m=17), EUNSUPPORTED, "zm_lqr_backward_f64: (n=12, m=17) not covered (need n<=64, m<=16)"),
    (F64, dict(batch=P31), EUNSUPPORTED, "zm_lqr_backward_f64: T*n*n or batch too large"),
    (F64, dict(T=1 << 19, n=64, m=16), EUNSUPPORTED, "zm_lqr_backward_f64: T*n*n or batch too large"),
    (F64, dict(T=1 << 29, n=2), EUNSUPPORTED, "zm_lqr_backward_f64: T*n*n or batch too large"),
    # two at once
    (F64, dict(Q=None, T=0), EINVAL, "zm_lqr_backward_f64: null pointer"),
    (F64, dict(L=None, n=65), EINVAL, "zm_lqr_backward_f64: null pointer"),
    _bad_size(F64, T=0, n=65),
    _bad_size(F64, batch=-1, m=17),
    (F64, dict(n=65, m=16, batch=P31), EUNSUPPORTED, "zm_lqr_backward_f64: (n=65, m=16) not covered (need n<=64, m<=16)"),
    # ---- zm_lqr_backward_f32: T == 0 is accepted, an oversize batch is ZM_EINVAL, no bound on T*n*n ------------------------------
    (F32, dict(batch=0, A=None, B=None, Q=None, R=None, L=None), OK, None),
    (F32, dict(batch=0, T=-1, n=0, m=99), OK, None),
    (F32, dict(T=0), OK, None),
    *_nulls(F32, "A B Q R L"),
    (F32, dict(batch=-1), EINVAL, "zm_lqr_backward_f32: bad size"),
    (F32, dict(T=-1), EINVAL, "zm_lqr_backward_f32: bad size"),
    (F32, dict(n=0), EINVAL, "zm_lqr_backward_f32: bad size"),
    (F32, dict(m=0), EINVAL, "zm_lqr_backward_f32: bad size"),
    (F32, dict(n=65, m=16), EUNSUPPORTED, "zm_lqr_backward_f32: n=65, m=16 outside n <= 64, m <= 16"),
    (F32, dict(n=12, m=17), EUNSUPPORTED, "zm_lqr_backward_f32: n=12, m=17 outside n <= 64, m <= 16"),
    (F32, dict(batch=P31), EINVAL, "zm_lqr_backward_f32: batch too large for one launch"),
    # two at once
    (F32, dict(R=None, T=-1), EINVAL, "zm_lqr_backward_f32: null pointer"),
    (F32, dict(A=None, T=0), EINVAL, "zm_lqr_backward_f32: null pointer"),
    (F32, dict(n=0, m=17), EINVAL, "zm_lqr_backward_f32: bad size"),
    (F32, dict(n=65, batch=P31), EUNSUPPORTED, "zm_lqr_backward_f32: n=65, m=1 outside n <= 64, m <= 16"),
    (F32, dict(T=0, batch=P31), EINVAL, "zm_lqr_backward_f32: batch too large for one launch"),
    (F32, dict(T=0, n=65), EUNSUPPORTED, "zm_lqr_backward_f32: n=65, m=1 outside n <= 64, m <= 16"),
    # ---- zm_lqr_backward_host_f64: neither "too large" bound (the sizes go on to hipMalloc) --------------------------------------
    (HOST, dict(batch=0, A=None, B=None, Q=None, R=None, L=None), OK, None),
    (HOST, dict(batch=0, T=0, n=0, m=99), OK, None),
    *_nulls(HOST, "A B Q R L"),
    (HOST, dict(batch=-1), EINVAL, "zm_lqr_backward_host_f64: bad size"),
    (HOST, dict(T=0), EINVAL, "zm_lqr_backward_host_f64: bad size"),
    (HOST, dict(n=0), EINVAL, "zm_lqr_backward_host_f64: bad size"),
    (HOST, dict(m=0), EINVAL, "zm_lqr_backward_host_f64: bad size"),
    (HOST, dict(n=65, m=16), EUNSUPPORTED, "zm_lqr_backward_host_f64: (n=65, m=16) not covered"),
    (HOST, dict(n=12, m=17), EUNSUPPORTED, "zm_lqr_backward_host_f64: (n=12, m=17) not covered"),
    # two at once
    (HOST, dict(B=None, m=0), EINVAL, "zm_lqr_backward_host_f64: null pointer"),
    (HOST, dict(T=0, n=65), EINVAL, "zm_lqr_backward_host_f64: bad size"),
    (HOST, dict(batch=-1, m=17), EINVAL, "zm_lqr_backward_host_f64: bad size"),
    # ---- zm_lqr_backward_affine_f64 --------------------------------------------------------------------------------------------
    (AFF, dict(batch=0, A=None, d=None, r=None, l=None), OK, None),
    (AFF, dict(batch=0, T=0, n=0, m=99), OK, None),
    *_nulls(AFF, "A B d Q R H q r L l"),
    _bad_size(AFF, batch=-1), _bad_size(AFF, T=0), _bad_size(AFF, n=0), _bad_size(AFF, m=0),
    (AFF, dict(n=49, m=4), EUNSUPPORTED, "zm_lqr_backward_affine_f64: (n=49, m=4) not covered (need n<=48, m<=16)"),
    (AFF, dict(n=12, m=17), EUNSUPPORTED, "zm_lqr_backward_affine_f64: (n=12, m=17) not covered (need n<=48, m<=16)"),
    (AFF, dict(batch=P31), EUNSUPPORTED, "zm_lqr_backward_affine_f64: T*n*n or batch too large"),
    (AFF, dict(T=1 << 21, n=32, m=8), EUNSUPPORTED, "zm_lqr_backward_affine_f64: T*n*n or batch too large"),
    # two at once
    (AFF, dict(H=None, T=0), EINVAL, "zm_lqr_backward_affine_f64: null pointer"),
    _bad_size(AFF, m=0, n=49),
    (AFF, dict(n=49, batch=P31), EUNSUPPORTED, "zm_lqr_backward_affine_f64: (n=49, m=1) not covered (need n<=48, m<=16)"),
    # ---- zm_dare_f64 (P and iters are optional) -----------------------------------------------------------------------------------
    (DARE, dict(batch=0, A=None, B=None, Q=None, R=None, L=None), OK, None),
    (DARE, dict(batch=0, n=0, max_iter=0, tol=-1.0), OK, None),
    *_nulls(DARE, "A B Q R L"),
    *[(DARE, over, EINVAL, "zm_dare_f64: bad argument") for over in
      (dict(batch=-1), dict(n=0), dict(m=0), dict(max_iter=0), dict(tol=-1.0), dict(tol=NAN))],
    (DARE, dict(n=65, m=16), EUNSUPPORTED, "zm_dare_f64: (n=65, m=16) not covered (need n<=64, m<=16)"),
    (DARE, dict(n=12, m=17), EUNSUPPORTED, "zm_dare_f64: (n=12, m=17) not covered (need n<=64, m<=16)"),
    (DARE, dict(batch=P31), EUNSUPPORTED, "zm_dare_f64: batch too large"),
    # two at once
    (DARE, dict(R=None, max_iter=0), EINVAL, "zm_dare_f64: null pointer"),
    (DARE, dict(tol=NAN, n=65), EINVAL, "zm_dare_f64: bad argument"),
    (DARE, dict(m=17, batch=P31), EUNSUPPORTED, "zm_dare_f64: (n=2, m=17) not covered (need n<=64, m<=16)"),
    # ---- zm_care_f64 (P and info are optional) ------------------------------------------------------------------------------------
    (CARE, dict(batch=0, A=None, B=None, Q=None, R=None, K=None), OK, None),
    (CARE, dict(batch=0, n=0, max_iter=0, tol=-1.0), OK, None),
    *_nulls(CARE, "A B Q R K"),
    *[(CARE, over, EINVAL, "zm_care_f64: bad argument") for over in
      (dict(batch=-1), dict(n=0), dict(m=0), dict(max_iter=0), dict(tol=-1.0), dict(tol=NAN))],
    (CARE, dict(n=17, m=2), EUNSUPPORTED, "zm_care_f64: (n=17, m=2) not covered (need n<=16, m<=16)"),
    (CARE, dict(n=2, m=17), EUNSUPPORTED, "zm_care_f64: (n=2, m=17) not covered (need n<=16, m<=16)"),
    (CARE, dict(batch=P31), EUNSUPPORTED, "zm_care_f64: batch too large"),
    # two at once
    (CARE, dict(K=None, n=0), EINVAL, "zm_care_f64: null pointer"),
    (CARE, dict(max_iter=0, n=17), EINVAL, "zm_care_f64: bad argument"),
    (CARE, dict(n=17, batch=P31), EUNSUPPORTED, "zm_care_f64: (n=17, m=1) not covered (need n<=16, m<=16)"),
    # ---- zm_riccati_ode_f64 (info is optional) ------------------------------------------------------------------------------------
    (ODE, dict(batch=0, A_s=None, B_s=None, Rinv_s=None, Q_s=None, Qf=None, V=None), OK, None),
    (ODE, dict(batch=0, n=0, N=0, T=0.0), OK, None),
    *_nulls(ODE, "A_s B_s Rinv_s Q_s Qf V"),
    *[(ODE, over, EINVAL, "zm_riccati_ode_f64: bad argument") for over in
      (dict(batch=-1), dict(n=0), dict(m=0), dict(n_samples=0), dict(N=0), dict(max_steps=0), dict(T=0.0), dict(T=-1.0), dict(T=NAN),
       dict(rtol=-1e-8), dict(atol=-1e-8), dict(rtol=NAN), dict(atol=NAN), dict(rtol=0.0, atol=0.0))],
    (ODE, dict(n=17, m=2), EUNSUPPORTED, "zm_riccati_ode_f64: (n=17, m=2) not covered (need n<=16, m<=16)"),
    (ODE, dict(n=2, m=17), EUNSUPPORTED, "zm_riccati_ode_f64: (n=2, m=17) not covered (need n<=16, m<=16)"),
    (ODE, dict(batch=P31), EUNSUPPORTED, "zm_riccati_ode_f64: batch / sample count too large"),
    (ODE, dict(n=16, n_samples=1 << 22), EUNSUPPORTED, "zm_riccati_ode_f64: batch / sample count too large"),
    (ODE, dict(n=16, N=1 << 22), EUNSUPPORTED, "zm_riccati_ode_f64: batch / sample count too large"),
    # two at once
    (ODE, dict(Qf=None, T=0.0), EINVAL, "zm_riccati_ode_f64: null pointer"),
    (ODE, dict(N=0, n=17), EINVAL, "zm_riccati_ode_f64: bad argument"),
    (ODE, dict(m=17, batch=P31), EUNSUPPORTED, "zm_riccati_ode_f64: (n=2, m=17) not covered (need n<=16, m<=16)"),
]


def test_every_entry_has_rows_that_break_two_checks():
    assert {r[0] for r in ROWS} == set(ENTRIES)
    for entry in ENTRIES:
        assert sum(1 for e, over, rc, _ in ROWS if e == entry and rc != OK and len(over) >= 2) >= 2


@pytest.mark.parametrize("row", range(len(ROWS)), ids=lambda i: f"{ROWS[i][0]}-{'-'.join(ROWS[i][1])}-{i}")
def test_refusal(row):
    entry, over, rc, msg = ROWS[row]
    lib = _lib.lib()
    assert getattr(lib, entry)(*_args(entry, over)) == rc
    if msg is not None:
        assert lib.zm_last_error().decode() == msg


def test_support_matrix():
    """the values of test_abi.py::test_version_and_support_matrix and the four corners of the limit (1, 1) .. (64, 16)"""
    sup = _lib.lib().zm_lqr_backward_supported
    yes = [(12, 4, 8), (4, 1, 8), (8, 4, 8), (64, 16, 4), (64, 16, 8), (1, 1, 8), (1, 16, 8), (64, 1, 8), (1, 1, 4)]
    no = [(65, 16, 8), (12, 17, 4), (0, 1, 8), (1, 0, 8), (65, 1, 8), (1, 17, 8), (64, 17, 4), (65, 16, 4), (12, 4, 2), (12, 4, 16),
          (12, 4, 0), (-1, 4, 8)]
    assert [sup(*a) for a in yes] == [1] * len(yes)
    assert [sup(*a) for a in no] == [0] * len(no)


# ---- the Python layer: ValueError texts of the checks that run before the first device access --------------------------------------
def _z(*shape):
    return np.zeros(shape)


def _dfh(N=3, **over):
    """discreteFiniteHorizonLqr at lead (2,), N = 3, (n, m) = (2, 2)"""
    ops = dict(A=_z(2, 3, 2, 2), B=_z(2, 3, 2, 2), Q=_z(2, 3, 2, 2), R=_z(2, 3, 2, 2))
    ops.update(over)
    return lambda: lqrUtils.discreteFiniteHorizonLqr(ops["A"], ops["B"], ops["Q"], ops["R"], N)


def _inf(fn, **over):
    """the two infinite-horizon designs at lead (2,), (n, m) = (4, 2)"""
    ops = dict(A=_z(2, 4, 4), B=_z(2, 4, 2), Q=_z(2, 4, 4), R=_z(2, 2, 2))
    ops.update(over)
    return lambda: getattr(lqrUtils, fn)(ops["A"], ops["B"], ops["Q"], ops["R"])


def _aff(N=3, **over):
    """bilinearAffineLqr at lead (2,), N = 3, (n, m) = (3, 2)"""
    ops = dict(A=_z(2, 3, 3, 3), B=_z(2, 3, 3, 2), d=_z(2, 3, 3), Q=_z(2, 3, 3, 3), R=_z(2, 3, 2, 2), H=_z(2, 3, 2, 3), q=_z(2, 3, 3),
               r=_z(2, 3, 2), q0=_z(2, 3))
    ops.update(over)
    return lambda: lqrUtils.bilinearAffineLqr(*[ops[k] for k in "A B d Q R H q r q0".split()], N)


def _fh(**kw):
    c = lambda t: np.eye(2)   # noqa: E731
    return lambda: lqrUtils.finiteHorizonLqr(c, c, c, c, np.eye(2), **{"T": 1.0, **kw})


DISC, CONT = "discreteInfiniteHorizonLqr", "infiniteHorizonLqr"
PY_ROWS = [
    (_dfh(R=_z(2, 3, 2, 3)), "R has shape (2, 3, 2, 3), expected (2, '>=N', 2, 2) with N=3"),
    (_dfh(Q=_z(2, 2, 2, 2)), "Q has shape (2, 2, 2, 2), expected (2, '>=N', 2, 2) with N=3"),          # time axis shorter than N
    (_dfh(A=_z(3, 3, 2, 2)), "A has shape (3, 3, 2, 2), expected (2, '>=N', 2, 2) with N=3"),          # wrong leading axis
    (_dfh(A=_z(3, 2, 2)), "A has shape (3, 2, 2), expected (2, '>=N', 2, 2) with N=3"),                # a leading axis missing
    (_dfh(Q=_z(2, 2)), "Q has shape (2, 2), expected (2, '>=N', 2, 2) with N=3"),
    (_dfh(A=_z(2, 3, 2, 3), Q=_z(2, 3, 3, 3)), "A has shape (2, 3, 2, 3), expected (2, '>=N', 2, 2) with N=3"),   # the first in A, B, Q, R
    (_dfh(B=_z(2, 2)), "B must have shape (..., N, n, m)"),
    (_dfh(N=0), "N must be >= 1"),
    (_dfh(N=0, R=_z(2, 3, 2, 3)), "R has shape (2, 3, 2, 3), expected (2, '>=N', 2, 2) with N=0"),     # the shape wins over N
    (_dfh(N=4), "A has shape (2, 3, 2, 2), expected (2, '>=N', 2, 2) with N=4"),
    (_dfh(A=_z(3, 2, 2), B=_z(3, 2, 2), Q=_z(3, 2, 2), R=_z(3, 2, 3)), "R has shape (3, 2, 3), expected ('>=N', 2, 2) with N=3"),
    (_inf(DISC, Q=_z(4, 4)), "Q has shape (4, 4), expected (2, 4, 4)"),
    (_inf(DISC, A=_z(2, 4, 3)), "A has shape (2, 4, 3), expected (2, 4, 4)"),
    (_inf(DISC, R=_z(3, 2, 2)), "R has shape (3, 2, 2), expected (2, 2, 2)"),
    (_inf(DISC, B=_z(4)), "B must have shape (..., n, m)"),
    (_inf(CONT, Q=_z(4, 4)), "Q has shape (4, 4), expected (2, 4, 4)"),
    (_inf(CONT, A=_z(2, 4, 3)), "A has shape (2, 4, 3), expected (2, 4, 4)"),
    (_inf(CONT, R=_z(2, 2, 2, 2)), "R has shape (2, 2, 2, 2), expected (2, 2, 2)"),
    (_inf(CONT, B=_z(4)), "B must have shape (..., n, m)"),
    (_aff(r=_z(2, 2, 2)), "r has shape (2, 2, 2), expected (2, '>=N', 2) with N=3"),
    (_aff(d=_z(2, 3, 2)), "d has shape (2, 3, 2), expected (2, '>=N', 3) with N=3"),
    (_aff(H=_z(2, 3, 3, 2)), "H has shape (2, 3, 3, 2), expected (2, '>=N', 2, 3) with N=3"),
    (_aff(q=_z(3, 3)), "q has shape (3, 3), expected (2, '>=N', 3) with N=3"),
    (_aff(Q=_z(4, 3, 3, 3)), "Q has shape (4, 3, 3, 3), expected (2, '>=N', 3, 3) with N=3"),
    (_aff(B=_z(3, 2)), "B must have shape (..., N, n, m)"),
    (_aff(N=0), "N must be >= 1"),
    (_aff(N=0, r=_z(2, 3, 3)), "r has shape (2, 3, 3), expected (2, '>=N', 2) with N=0"),
    (_fh(T=0.0), "T must be > 0 and N >= 1"),
    (_fh(T=NAN), "T must be > 0 and N >= 1"),
    (_fh(N=0), "T must be > 0 and N >= 1"),
    (_fh(n_samples=0), "n_samples must be >= 1"),
    (_fh(T=0.0, n_samples=0), "T must be > 0 and N >= 1"),
]


@pytest.mark.parametrize("row", range(len(PY_ROWS)))
def test_python_refusal(row):
    call, msg = PY_ROWS[row]
    with pytest.raises(ValueError) as e:
        call()
    assert str(e.value) == msg
