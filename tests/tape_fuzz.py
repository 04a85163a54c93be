"""Random expressions for the recorder (zopt_amd/tape.py) and the tape interpreter, shaped callables that put a kernel into a chosen
launch regime, and a reference that never touches the tape: hyper-dual numbers in long double behind the operator protocol.

random_callable   a seeded plan over a growing pool of values -> f(x, u[, p]); the same seed is the same expression everywhere.
                  "tame": every value is bounded and every denominator, tangent and root is away from its singularity, so that the
                  long-double derivatives are finite for inputs 0.7 x standard normal; "wild": raw `/`, tan, sqrt (the value path).
shaped_model / shaped_cost / shaped_terminal
                  the variables of `mask_bits` enter one product of sines, the others linearly: the recorded structural mask is
                  exactly `mask_bits`; optional padding with live temporaries that are multiplied by 0.0 (the recorder simplifies
                  nothing) to an exact slot count -- the function and its derivatives stay what they were.
hyper_class       (value, d1, d2, d12) of NumPy arrays of one dtype: HyperLD (long double, the reference) and Hyper64 (what float64
                  can do on the callable's own operators: the "oracle error" the bound follows).
expand            values, Jacobians and second derivatives of a callable at P points, every pair a <= b in one call.
regime            lanes per point, trips of the pair loop and the Hyper slot file of a tape, by traced_quadratic's formulas.

Bound (row_errors, allowance): an entry's error is measured relative to the largest reference entry of its row at its point
(model_hp_ref.row_error's measure); the allowance of an output row is max(FLOOR, 100 x e_row), e_row the Hyper64 error of that output
row, the worst over the points of the test.  The worst over the points and not the point's own: the realised float64 error at one
point is one draw from [0, conditioning x 2^-52]; the interpreter associates the derivative terms differently and draws again, and the
ratio of two single draws is unbounded, while the largest of the 8 or 15 draws of a row estimates the conditioning itself.
"""
import numpy as np

from tests import model_hp_ref as hp
from zopt_amd import tape as T

LD = np.longdouble
CONSTS = (-0.0, 0.5, -1.5, 2.0, 0.3, 1.0, 3.0, -0.25, 0.0, 1.75, -2.5, 0.125)
X_SCALE = 0.7


# ---- hyper-dual numbers behind the operator protocol ----------------------------------------------------------------------------------
def hyper_class(dtype, name):
    class H:
        """value, first derivatives along two directions and the mixed second derivative; arrays of one dtype that broadcast"""
        __slots__ = ("v", "d1", "d2", "d12")

        def __init__(self, v, d1=0, d2=0, d12=0):
            self.v, self.d1, self.d2, self.d12 = (np.asarray(t, dtype=dtype) for t in (v, d1, d2, d12))

        @staticmethod
        def _c(o):
            if isinstance(o, H):
                return o
            c = T._number(o)
            if c is None:
                raise TypeError(f"{name}: operand {o!r}")
            return H(c)

        def __add__(self, o):
            o = self._c(o)
            return H(self.v + o.v, self.d1 + o.d1, self.d2 + o.d2, self.d12 + o.d12)

        def __radd__(self, o):
            o = self._c(o)
            return H(o.v + self.v, o.d1 + self.d1, o.d2 + self.d2, o.d12 + self.d12)

        def __sub__(self, o):
            o = self._c(o)
            return H(self.v - o.v, self.d1 - o.d1, self.d2 - o.d2, self.d12 - o.d12)

        def __rsub__(self, o):
            return self._c(o) - self

        def __mul__(self, o):
            o = self._c(o)
            return H(self.v * o.v, self.v * o.d1 + self.d1 * o.v, self.v * o.d2 + self.d2 * o.v,
                     self.v * o.d12 + self.d1 * o.d2 + self.d2 * o.d1 + self.d12 * o.v)

        def __rmul__(self, o):
            return self._c(o) * self

        def __truediv__(self, o):
            o = self._c(o)
            q = self.v / o.v
            q1, q2 = (self.d1 - q * o.d1) / o.v, (self.d2 - q * o.d2) / o.v
            return H(q, q1, q2, (self.d12 - q1 * o.d2 - q2 * o.d1 - q * o.d12) / o.v)

        def __rtruediv__(self, o):
            return self._c(o) / self

        def __neg__(self):
            return H(-self.v, -self.d1, -self.d2, -self.d12)

        def __pos__(self):
            return self

        def __pow__(self, k):
            k = int(k)
            assert 1 <= k <= 8
            r = self
            for _ in range(k - 1):          # the recorder's left-to-right product
                r = r * self
            return r

        def _fn(self, f, f1, f2):
            return H(f, f1 * self.d1, f1 * self.d2, f2 * self.d1 * self.d2 + f1 * self.d12)

        def sin(self):
            s, c = np.sin(self.v), np.cos(self.v)
            return self._fn(s, c, -s)

        def cos(self):
            s, c = np.sin(self.v), np.cos(self.v)
            return self._fn(c, -s, -c)

        def tan(self):
            t = np.tan(self.v)
            return self._fn(t, 1 + t * t, 2 * t * (1 + t * t))

        def sqrt(self):
            r = np.sqrt(self.v)
            return self._fn(r, 1 / (2 * r), -1 / (4 * r * r * r))
    H.__name__ = H.__qualname__ = name
    H.dtype = dtype
    return H


HyperLD = hyper_class(LD, "HyperLD")
Hyper64 = hyper_class(np.float64, "Hyper64")


class Boxed:
    """a float64 behind the operator protocol the recording goes through (NumPy object arrays call these per element); `**` is the
    recorder's left-to-right product"""
    __slots__ = ("v",)

    def __init__(self, v):
        self.v = np.float64(v)

    @staticmethod
    def _v(o):
        return o.v if isinstance(o, Boxed) else np.float64(o)

    def __add__(self, o): return Boxed(self.v + self._v(o))
    def __radd__(self, o): return Boxed(self._v(o) + self.v)
    def __sub__(self, o): return Boxed(self.v - self._v(o))
    def __rsub__(self, o): return Boxed(self._v(o) - self.v)
    def __mul__(self, o): return Boxed(self.v * self._v(o))
    def __rmul__(self, o): return Boxed(self._v(o) * self.v)
    def __truediv__(self, o): return Boxed(self.v / self._v(o))
    def __rtruediv__(self, o): return Boxed(self._v(o) / self.v)
    def __neg__(self): return Boxed(-self.v)
    def __pos__(self): return self

    def __pow__(self, k):
        if T._number(k) is None or k != int(k) or not 1 <= int(k) <= 8:
            return NotImplemented
        r = self.v
        for _ in range(int(k) - 1):
            r = r * self.v
        return Boxed(r)

    def sin(self): return Boxed(np.sin(self.v))
    def cos(self): return Boxed(np.cos(self.v))
    def tan(self): return Boxed(np.tan(self.v))
    def sqrt(self): return Boxed(np.sqrt(self.v))


def _objects(items):
    return np.array(list(items) + [None], dtype=object)[:-1]


def boxed_call(f, x, u=None, p=None):
    """f on float64 values behind the operator protocol -> float64 (n_out,); u = None: a terminal callable f(x[, p])"""
    box = lambda a: _objects(Boxed(v) for v in a)                                              # noqa: E731
    args = (box(x),) + (() if u is None else (box(u),)) + (() if p is None else (box(p),))
    out = np.asarray(f(*args), dtype=object).reshape(-1)
    return np.array([o.v if isinstance(o, Boxed) else o for o in out], dtype=np.float64)


def expand(f, n, m, x, u=None, p=None, dtype=LD, controls=True):
    """(values (P, n_out), Jacobian (P, n_out, K), second derivatives (P, n_out, K, K)), K = n + m, of the callable f(x, u[, p])
    (controls=False: f(x[, p]); its control columns are zero) by one call on hyper-dual numbers of `dtype`: every pair a <= b of the
    variables is a column"""
    H = HyperLD if dtype is LD else Hyper64
    x = np.atleast_2d(np.asarray(x, dtype=dtype))
    P, K = x.shape[0], n + m
    u = np.zeros((P, m), dtype=dtype) if u is None else np.atleast_2d(np.asarray(u, dtype=dtype))
    ia, ib = np.triu_indices(K)
    z = np.concatenate([x, u], 1)
    with np.errstate(all="ignore"):
        ins = [H(z[:, k:k + 1], (ia == k)[None, :], (ib == k)[None, :], 0) for k in range(K)]
        args = (_objects(ins[:n]),) + ((_objects(ins[n:]),) if controls else ())
        if p is not None:
            pp = np.broadcast_to(np.atleast_2d(np.asarray(p, dtype=dtype)), (P, np.shape(p)[-1]))
            args += (_objects(H(pp[:, k:k + 1]) for k in range(pp.shape[1])),)
        out = np.asarray(f(*args), dtype=object).reshape(-1)
    n_out = len(out)
    val, J, S = np.zeros((P, n_out), dtype=dtype), np.zeros((P, n_out, K), dtype=dtype), np.zeros((P, n_out, K, K), dtype=dtype)
    diag = np.flatnonzero(ia == ib)
    for i, o in enumerate(out):
        if not isinstance(o, H):
            val[:, i] = T._number(o)
            continue
        full = lambda a: np.broadcast_to(a, (P, len(ia)))                                      # noqa: E731
        val[:, i] = full(o.v)[:, 0]
        J[:, i, :] = full(o.d1)[:, diag]
        S[:, i, ia, ib] = S[:, i, ib, ia] = full(o.d12)
    return val, J, S


def jacobian_ld(f, n, m, x, u=None, p=None, controls=True):
    """(values, [f_x | f_u]) in long double"""
    return expand(f, n, m, x, u, p, LD, controls)[:2]


def hessian_ld(f, n, m, x, u=None, p=None, controls=True):
    """(P, n_out, n + m, n + m) in long double"""
    return expand(f, n, m, x, u, p, LD, controls)[2]


# ---- the bound ------------------------------------------------------------------------------------------------------------------------
def row_errors(got, ref):
    """(P, rows): max over a row's entries of |got - ref| / max(1, largest |ref| of the row) -- model_hp_ref.row_error before its
    maximum over points and rows.  A non-finite reference entry fails: the tame family has none."""
    ref, got = np.asarray(ref, dtype=LD), np.asarray(got, dtype=LD)
    assert np.all(np.isfinite(ref)), "a non-finite reference value"
    P, r = ref.shape[:2]
    R_, G = ref.reshape(P, r, -1), got.reshape(P, r, -1)
    with np.errstate(invalid="ignore"):
        err = np.abs(G - R_)
    err = np.where(np.isfinite(G), err, np.inf)
    return (np.max(err, axis=2) / np.maximum(1, np.max(np.abs(R_), axis=2))).astype(np.float64)


def allowance(ref64, ref):
    """(rows,): max(FLOOR, 100 x e_row), e_row the float64 evaluation's error of the output row, the worst over the points"""
    return np.maximum(hp.FLOOR, 100.0 * np.max(row_errors(ref64, ref), axis=0))


def ratio(got, ref64, ref):
    """worst error / allowance over points and rows"""
    e = row_errors(got, ref)
    assert np.isclose(float(np.max(e)) if e.size else 0.0, hp.row_error(got, ref), rtol=1e-12, atol=0)
    return float(np.max(e / allowance(ref64, ref)[None, :])) if e.size else 0.0


# ---- launch regime of a tape (traced.hip: traced_quadratic; traced_cost.hip: zm_traced_cost_expand_list_f64) -----------------------------
def regime(mask, n_slots):
    """(V, pairs, lanes per point, trips of the pair loop, "LDS" | "scratch")"""
    V = bin(mask).count("1")
    pairs = V * (V + 1) // 2
    lpp = 16
    while lpp < 64 and lpp < pairs:
        lpp *= 2
    return V, pairs, lpp, -(-pairs // lpp), "LDS" if n_slots * 4 * 64 * 8 <= 64 * 1024 else "scratch"


# ---- random expressions ---------------------------------------------------------------------------------------------------------------
_BIN = {"add": lambda a, b: a + b, "sub": lambda a, b: a - b, "mul": lambda a, b: a * b, "div": lambda a, b: a / b}
_UN = {"neg": lambda a: -a, "sin": np.sin, "cos": np.cos, "tan": np.tan, "sqrt": np.sqrt}


class _Plan:
    """steps over a pool of values; `bound[i]`: a bound of |value i| for inputs within +-3 (the tame family keeps it small: factors
    and the arguments of sine and cosine within 3, terms within 8 -- a many-turn angle inside a chain costs the long-double reference
    its digits)"""

    def __init__(self, rng, n_in, tame):
        self.rng, self.tame, self.steps = rng, tame, []
        self.n_in, self.used = n_in, set()
        self.bound = [3.0] * n_in

    def emit(self, step, bound):
        self.steps.append(step)
        self.bound.append(bound)
        return len(self.bound) - 1

    def pick(self):
        """an operand: an input, a value that nothing has read yet (so that little of the plan is dead), or any value"""
        r, size = self.rng, len(self.bound)
        t = r.random()
        unused = [i for i in range(self.n_in, size) if i not in self.used]
        if t < 0.25 or size == self.n_in:
            i = int(r.integers(self.n_in))
        elif t < 0.75 and unused:
            i = unused[int(r.integers(len(unused)))]
        else:
            i = int(r.integers(size))
        self.used.add(i)
        return i

    def small(self, i, limit):
        """value i, or its sine where it may be larger than `limit`"""
        if not self.tame or self.bound[i] <= limit:
            return i
        return self.emit(("un", "sin", i), 1.0)

    def binary(self, op, a, b):
        """a, b: ("v", index) or ("c", constant)"""
        ba, bb = (self.bound[o[1]] if o[0] == "v" else abs(o[1]) for o in (a, b))
        return self.emit(("bin", op, a, b), ba * bb if op == "mul" else ba + bb)

    def grow(self):
        r = self.rng
        if self.steps and r.random() < 0.08:                    # the same subexpression again (recorded once)
            k = int(r.integers(len(self.steps)))
            return self.emit(self.steps[k], self.bound[self.n_in + k])
        kind = r.choice(["add", "sub", "mul", "div", "neg", "pow", "sin", "cos", "tan", "sqrt"],
                        p=[0.15, 0.15, 0.2, 0.12, 0.05, 0.1, 0.07, 0.06, 0.05, 0.05])
        const = lambda: ("c", float(CONSTS[int(r.integers(len(CONSTS)))]))                       # noqa: E731
        if kind in ("add", "sub", "mul", "div"):
            lim = 3.0 if kind in ("mul", "div") else 8.0
            a, b = self.small(self.pick(), lim), self.small(self.pick(), lim)
            side = r.random()
            oa, ob = (const() if side < 0.22 else ("v", a)), (const() if 0.22 <= side < 0.44 else ("v", b))
            if kind == "div" and self.tame:                     # by b * b + 0.5
                if ob[0] == "c":
                    ob = ("v", b)
                sq = self.binary("mul", ob, ob)
                den = self.binary("add", ("v", sq), ("c", 0.5))
                ba = self.bound[oa[1]] if oa[0] == "v" else abs(oa[1])
                return self.emit(("bin", "div", oa, ("v", den)), 2.0 * ba)
            return self.binary(kind, oa, ob)
        a = self.pick()
        if kind == "neg":
            return self.emit(("un", "neg", a), self.bound[a])
        if kind == "pow":
            a = self.small(a, 1.2)
            k = int(r.integers(1, 9))
            return self.emit(("pow", k, a), min(max(1.0, self.bound[a]), 1e30) ** k)
        if kind in ("sin", "cos"):
            return self.emit(("un", kind, self.small(a, 3.0)), 1.0)
        if kind == "tan":
            if self.tame:                                       # tan(0.4 sin v)
                s = self.emit(("un", "sin", a), 1.0)
                a = self.binary("mul", ("c", 0.4), ("v", s))
            return self.emit(("un", "tan", a), 0.5 if self.tame else 1e3)
        if self.tame:                                           # sqrt(v v + 0.25)
            a = self.small(a, 3.0)
            sq = self.binary("mul", ("v", a), ("v", a))
            a = self.binary("add", ("v", sq), ("c", 0.25))
        return self.emit(("un", "sqrt", a), self.bound[a] + 1.0)


def random_callable(seed, n, m, n_ops, family="tame", n_params=0, n_out=None, controls=True):
    """f(x, u[, p]) (controls=False: f(x[, p])) -> n_out values (default n) from a plan seeded by every argument"""
    assert family in ("tame", "wild")
    n_out = n if n_out is None else n_out
    rng = np.random.default_rng([int(seed), n, m, n_ops, family == "wild", n_params, n_out, int(controls)])
    n_in = n + (m if controls else 0) + n_params
    plan = _Plan(rng, n_in, family == "tame")
    while len(plan.steps) < n_ops:
        plan.grow()
    size = len(plan.bound)
    outs = []
    for i in range(n_out):
        t = rng.random()
        if t < 0.62 or (i == 0 and t < 0.9):
            unused = [k for k in range(n_in, size) if k not in plan.used]
            k = unused[int(rng.integers(len(unused)))] if unused and rng.random() < 0.8 else int(rng.integers(n_in, size))
            plan.used.add(k)
            outs.append(("v", k))
        elif t < 0.76:
            outs.append(("v", int(rng.integers(n_in))))                                        # a raw input
        elif t < 0.88 and outs:
            outs.append(outs[int(rng.integers(len(outs)))])                                    # the same value twice
        else:
            outs.append(("c", float(CONSTS[int(rng.integers(len(CONSTS)))])))                  # a plain number
    steps = tuple(plan.steps)

    def f(*args):
        pool = [v for a in args for v in a]
        assert len(pool) == n_in
        get = lambda o: pool[o[1]] if o[0] == "v" else o[1]                                    # noqa: E731
        with np.errstate(all="ignore"):
            for st in steps:
                if st[0] == "bin":
                    pool.append(_BIN[st[1]](get(st[2]), get(st[3])))
                elif st[0] == "un":
                    pool.append(_UN[st[1]](pool[st[2]]))
                else:
                    pool.append(pool[st[2]] ** st[1])
        res = [get(o) for o in outs]
        if all(T._number(v) is not None for v in res):
            return np.array(res, dtype=np.float64)
        return _objects(res)
    f.plan = (steps, tuple(outs))
    return f


def points(seed, n, m, P, n_params=0, wild=False):
    """x (P, n), u (P, m), p (P, n_params) | None: 0.7 x standard normal; wild: NaN, +-inf and many-turn angles as well"""
    rng = np.random.default_rng([41, int(seed), n, m, P])
    x, u = X_SCALE * rng.standard_normal((P, n)), X_SCALE * rng.standard_normal((P, m))
    p = X_SCALE * rng.standard_normal((P, n_params)) if n_params else None
    if wild:
        x, u = 2.0 * x / X_SCALE, u / X_SCALE
        x[P // 2:] += 2 * np.pi * rng.integers(-1000, 1001, (P - P // 2, n))
        for k, v in enumerate((np.nan, np.inf, -np.inf)):
            if k < P:
                x[k, k % n] = v
    return x, u, p


# ---- shaped callables -----------------------------------------------------------------------------------------------------------------
def _shaped(z, mask_bits, rows, pad):
    """rows of: c_i x product over mask_bits of sin(k_b z_b + phase_b)  +  a few linear terms of the other variables; `pad` live
    temporaries sin(c_j z_first) are formed first and enter row 0 at the end multiplied by 0.0"""
    mask_bits = list(mask_bits)
    rest = [k for k in range(len(z)) if k not in mask_bits]
    temps = [np.sin((0.5 + 0.01 * j) * z[mask_bits[0]]) for j in range(pad)]
    prod = None
    for b in mask_bits:
        s = np.sin((0.6 + 0.05 * b) * z[b] + (0.3 + 0.1 * b))
        prod = s if prod is None else prod * s
    out = []
    for i in range(rows):
        r = None if prod is None else (1.0 + 0.25 * i) * prod
        for j in range(min(3, len(rest))):
            t = (0.5 + 0.125 * ((i + 2 * j) % 5)) * z[rest[(i + j) % len(rest)]]
            r = t if r is None else r + t
        out.append(0.0 * z[0] + 1.0 if r is None else r)
    for t in temps:
        out[0] = out[0] + 0.0 * t
    return out


def _padded(make, n, m, n_slots, **kw):
    """make(pad) with the padding at which the recorded tape has exactly n_slots slots"""
    if n_slots is None:
        return make(0)
    for pad in range(T.MAX_SLOTS):
        f = make(pad)
        if T.record(f, n, m, **kw).n_slots == n_slots:
            return f
    raise AssertionError(f"no padding gives {n_slots} slots")


def shaped_model(n, m, mask_bits, n_slots=None):
    """tame f(x, u) -> n values whose recorded mask is exactly `mask_bits` (bit i: state i, bit n + j: control j)"""
    def make(pad):
        return lambda x, u: _objects(_shaped(list(x) + list(u), mask_bits, n, pad))
    return _padded(make, n, m, n_slots)


def shaped_cost(n, m, mask_bits, n_slots=None):
    """tame running cost c(x, u) -> one value, mask exactly `mask_bits`"""
    def make(pad):
        return lambda x, u: _shaped(list(x) + list(u), mask_bits, 1, pad)[0]
    return _padded(make, n, m, n_slots, n_out=1)


def shaped_terminal(n, m, mask_bits, n_slots=None):
    """tame terminal cost v(x) -> one value, mask exactly `mask_bits` (states only)"""
    assert all(b < n for b in mask_bits)

    def make(pad):
        return lambda x: _shaped(list(x), mask_bits, 1, pad)[0]
    return _padded(make, n, m, n_slots, n_out=1, controls=False)


def bits(mask_bits):
    return sum(1 << b for b in mask_bits)
