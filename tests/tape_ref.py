"""NumPy evaluator of a TracedModel's tape (zopt_amd/tape.py) on float64, longdouble and dual numbers, the example callables the
traced-model tests share, and the host build of the device interpreter (tests/tape_shim.cpp around zopt_amd/csrc/tape_model.h).

The evaluator restates the interpreter's semantics independently of the C++: one pass over the instruction words, operands from the
slot file or the constant table, the outputs read from their slots at the end.  Vectorised over points: x (P, n), u (P, m), p (P, np).
"""
import ctypes
import os
import subprocess

import numpy as np

from zopt_amd import tape as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "zopt_amd", "csrc")


# ---- the example callables (plain NumPy; traced unmodified) ---------------------------------------------------------------------------
def pendulum(x, u, dt=0.05, g=9.81, length=1.0):
    th, om = x[0], x[1]
    return np.array([th + dt * om, om + dt * (u[0] - (g / length) * np.sin(th))])


def pendulum_p(x, u, p, dt=0.05, g=9.81):
    """the pendulum with its length as a per-problem parameter"""
    th, om = x[0], x[1]
    return np.array([th + dt * om, om + dt * (u[0] - (g / p[0]) * np.sin(th))])


def car(x, u, dt=0.1, wheelbase=2.5):
    """kinematic car, state [px, py, heading, speed], control [steering angle, acceleration]: not affine in the steering angle"""
    px, py, th, v = x
    return np.array([px + dt * v * np.cos(th), py + dt * v * np.sin(th), th + dt * v * np.tan(u[0]) / wheelbase, v + dt * u[1]])


def cartpole(x, u, dt=0.02, mc=1.0, mp=0.1, length=0.5, g=9.81):
    """cart-pole, state [position, angle, velocity, rate], control [force]: the force is divided by a state-dependent mass"""
    pos, th, v, om = x
    s, c = np.sin(th), np.cos(th)
    den = mc + mp * s ** 2
    acc = (u[0] + mp * s * (length * om ** 2 + g * c)) / den
    alpha = (-u[0] * c - mp * length * om ** 2 * c * s - (mc + mp) * g * s) / (length * den)
    return np.array([pos + dt * v, th + dt * om, v + dt * acc, om + dt * alpha])


def scalar11(x, u):
    return np.array([0.9 * x[0] + np.sqrt(x[0] * x[0] + 1.0) * u[0]])


def wide_live(k):
    """(1, 1) callable with 2 inputs + k temporaries live at once: sin(c_i x) for i < k, then summed from the last to the first"""
    def f(x, u):
        t = [np.sin((0.5 + 0.01 * i) * x[0]) for i in range(k)]
        acc = t[k - 1] * u[0]
        for i in range(k - 2, -1, -1):
            acc = acc + t[i]
        return np.array([acc])
    return f


def long_chain(k):
    """(1, 1) callable of exactly k instructions: x <- x * c + u, (k - 1) / 2 times, closed by one more product when k is even"""
    def f(x, u):
        acc = x[0] * 0.999
        left = k - 1
        while left >= 2:
            acc = acc * 0.999 + u[0]
            left -= 2
        if left:
            acc = acc * 1.0009765625
        return np.array([acc])
    return f


# ---- number systems ----------------------------------------------------------------------------------------------------------------
class Real:
    """float64 or longdouble arrays; sincos: None (NumPy's) or a callable x -> (sin x, cos x) on float64 (the host build of trig.h)"""

    def __init__(self, dtype=np.float64, sincos=None):
        self.dtype, self.sincos = dtype, sincos

    def lift(self, v, shape):
        return np.broadcast_to(np.asarray(v, dtype=self.dtype), shape).copy()

    def const(self, c, shape):
        return self.lift(c, shape)

    def _sc(self, a):
        if self.sincos is None:
            return np.sin(a), np.cos(a)
        s, c = self.sincos(np.ascontiguousarray(a, dtype=np.float64))
        return s.reshape(a.shape), c.reshape(a.shape)

    def unary(self, op, a):
        with np.errstate(all="ignore"):
            if op == "neg":
                return -a
            if op == "sqrt":
                return np.sqrt(a)
            s, c = self._sc(a)
            return {"sin": s, "cos": c, "tan": s / c if self.sincos is not None else np.tan(a)}[op]

    def binary(self, op, a, b):
        with np.errstate(all="ignore"):
            return T._BINARY[op](a, b)


class DualNumber:
    """(value, derivative) pairs of longdouble (or float64) arrays"""

    def __init__(self, dtype=np.longdouble):
        self.r = Real(dtype)
        self.dtype = dtype

    def lift(self, v, shape, d=0.0):
        return (self.r.lift(v, shape), self.r.lift(d, shape))

    def const(self, c, shape):
        return self.lift(c, shape)

    def unary(self, op, a):
        v, d = a
        if op == "neg":
            return (-v, -d)
        if op == "sqrt":
            r = np.sqrt(v)
            return (r, d / (2 * r))
        s, c = np.sin(v), np.cos(v)
        if op == "sin":
            return (s, c * d)
        if op == "cos":
            return (c, -s * d)
        t = s / c
        return (t, (1 + t * t) * d)

    def binary(self, op, a, b):
        (av, ad), (bv, bd) = a, b
        if op == "add":
            return (av + bv, ad + bd)
        if op == "sub":
            return (av - bv, ad - bd)
        if op == "mul":
            return (av * bv, av * bd + ad * bv)
        q = av / bv
        return (q, (ad - q * bd) / bv)


def evaluate(tape, x, u, p=None, num=None, seed=None):
    """x+ (P, n) of the tape at x (P, n), u (P, m), p (P, np) in the number system `num` (default float64 with NumPy's functions).
    seed: for DualNumber, the index of the variable (state i, control n + j) whose derivative is 1.  Raises if a slot is read before
    it is written."""
    num = num or Real()
    x, u = np.atleast_2d(x), np.atleast_2d(u)
    P = x.shape[0]
    ins = [x[:, i] for i in range(tape.n)] + [u[:, j] for j in range(tape.m)]
    if tape.n_params:
        p = np.broadcast_to(np.atleast_2d(p), (P, tape.n_params))
        ins += [p[:, j] for j in range(tape.n_params)]
    slots = [None] * tape.n_slots
    for s, v in enumerate(ins):
        slots[s] = num.lift(v, (P,), 1.0 if s == seed else 0.0) if isinstance(num, DualNumber) else num.lift(v, (P,))
    for op, dst, (ac, a), (bc, b) in tape.decode():
        def fetch(is_const, idx):
            if is_const:
                return num.const(tape.consts[idx], (P,))
            if slots[idx] is None:
                raise AssertionError(f"slot {idx} read before it is written")
            return slots[idx]
        va = fetch(ac, a)
        if op == "mov":
            r = va
        elif op in T._UNARY:
            r = num.unary(op, va)
        else:
            r = num.binary(op, va, fetch(bc, b))
        slots[dst] = r
    outs = [slots[s] for s in tape.outputs]
    if any(o is None for o in outs):
        raise AssertionError("an output slot was never written")
    if isinstance(num, DualNumber):
        return np.stack([o[0] for o in outs], -1), np.stack([o[1] for o in outs], -1)
    return np.stack(outs, -1)


def jacobian(tape, x, u, p=None, dtype=np.longdouble):
    """(f (P, n), [f_x | f_u] (P, n, n + m)) of the tape by dual numbers of `dtype`"""
    cols = []
    for j in range(tape.n + tape.m):
        f, d = evaluate(tape, np.asarray(x, dtype=dtype), np.asarray(u, dtype=dtype), p, DualNumber(dtype), seed=j)
        cols.append(d)
    return f, np.stack(cols, -1)


def liveness(tape):
    """(peak number of slots in use, True if every output slot is written last by the instruction that defines it and not overwritten
    before the end) -- from the instruction words alone"""
    n_in = tape.n + tape.m + tape.n_params
    written = set(range(n_in))
    final_writer = {}
    for k, (op, dst, (ac, a), (bc, b)) in enumerate(tape.decode()):
        for is_c, s in ((ac, a), (bc, b) if op in T._BINARY else (True, 0)):
            assert is_c or s in written, f"instruction {k} reads slot {s} before it is written"
        assert dst >= n_in, f"instruction {k} overwrites the pinned input slot {dst}"
        written.add(dst)
        final_writer[dst] = k
    return max(written) + 1, final_writer


# ---- host build of the interpreter ------------------------------------------------------------------------------------------------
def build(outdir):
    """Compile tests/tape_shim.cpp against the tree's tape_model.h as tests/trig_host.py builds its shim; returns the loaded library."""
    outdir = str(outdir)
    os.makedirs(os.path.join(outdir, "stub", "hip"), exist_ok=True)
    open(os.path.join(outdir, "stub", "hip", "hip_runtime.h"), "w").close()
    so = os.path.join(outdir, "tape_shim.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", HEADER_DIR,
                    "-I", os.path.join(outdir, "stub"), "-o", so, os.path.join(ROOT, "tests", "tape_shim.cpp")], check=True)
    lib = ctypes.CDLL(so)
    vp, dp = ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)
    # (code, n_instr, consts, outputs, n, m, np, x, u, p, p_stride, P, out...)
    head = [vp, ctypes.c_int, vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, dp, dp, vp, ctypes.c_long, ctypes.c_long]
    lib.tape_step.argtypes = head + [dp]
    lib.tape_jacobian.argtypes = head + [dp, dp]
    lib.tape_hessian.argtypes = head + [dp]
    for fn in (lib.tape_step, lib.tape_jacobian, lib.tape_hessian):
        fn.restype = None
    return lib


def _host_args(tape, x, u, p):
    x = np.ascontiguousarray(np.atleast_2d(x), dtype=np.float64)
    u = np.ascontiguousarray(np.atleast_2d(u), dtype=np.float64)
    P = x.shape[0]
    code = np.ascontiguousarray(tape.code, dtype=np.uint32)
    consts = np.ascontiguousarray(tape.consts, dtype=np.float64)
    outs = np.array(tape.outputs, dtype=np.uint32)
    stride, pp = 0, None
    if tape.n_params:
        pp = np.ascontiguousarray(np.atleast_2d(p), dtype=np.float64)
        stride = tape.n_params if pp.shape[0] == P and P > 1 else 0
    dp = ctypes.POINTER(ctypes.c_double)
    keep = (x, u, code, consts, outs, pp)
    args = [code.ctypes.data, len(code), consts.ctypes.data, outs.ctypes.data, tape.n, tape.m, tape.n_params,
            x.ctypes.data_as(dp), u.ctypes.data_as(dp), None if pp is None else pp.ctypes.data, stride, P]
    return keep, args, P


def host_step(lib, tape, x, u, p=None):
    """x+ (P, n) by the host build of the interpreter on double"""
    keep, args, P = _host_args(tape, x, u, p)
    out = np.empty((P, tape.n))
    lib.tape_step(*args, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    return out


def host_jacobian(lib, tape, x, u, p=None):
    """(f (P, n), [f_x | f_u] (P, n, n + m)) by the host build on Dual"""
    keep, args, P = _host_args(tape, x, u, p)
    f, J = np.empty((P, tape.n)), np.empty((P, tape.n, tape.n + tape.m))
    dp = ctypes.POINTER(ctypes.c_double)
    lib.tape_jacobian(*args, f.ctypes.data_as(dp), J.ctypes.data_as(dp))
    return f, J


def host_hessian(lib, tape, x, u, p=None):
    """H (P, n, n + m, n + m), H[:, i, a, b] = d2 f_i / dz_a dz_b, by the host build on Hyper (every pair a <= b, mirrored)"""
    keep, args, P = _host_args(tape, x, u, p)
    K = tape.n + tape.m
    H = np.empty((P, tape.n, K, K))
    lib.tape_hessian(*args, H.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    return H


# ---- exact second derivatives of a callable by sympy, evaluated in long double --------------------------------------------------------
class _Sym:
    """sympy expressions behind the operator protocol (np.sin on an object array calls .sin())"""

    def __init__(self, e):
        self.e = e

    @staticmethod
    def _e(o):
        import sympy
        return o.e if isinstance(o, _Sym) else sympy.Float(float(o), 40) if not float(o).is_integer() else sympy.Integer(int(o))

    def __add__(self, o): return _Sym(self.e + self._e(o))
    def __radd__(self, o): return _Sym(self._e(o) + self.e)
    def __sub__(self, o): return _Sym(self.e - self._e(o))
    def __rsub__(self, o): return _Sym(self._e(o) - self.e)
    def __mul__(self, o): return _Sym(self.e * self._e(o))
    def __rmul__(self, o): return _Sym(self._e(o) * self.e)
    def __truediv__(self, o): return _Sym(self.e / self._e(o))
    def __rtruediv__(self, o): return _Sym(self._e(o) / self.e)
    def __neg__(self): return _Sym(-self.e)
    def __pow__(self, k): return _Sym(self.e ** int(k))

    def sin(self):
        import sympy
        return _Sym(sympy.sin(self.e))

    def cos(self):
        import sympy
        return _Sym(sympy.cos(self.e))

    def tan(self):
        import sympy
        return _Sym(sympy.tan(self.e))

    def sqrt(self):
        import sympy
        return _Sym(sympy.sqrt(self.e))


def sympy_call(f, xs, us, ps=None):
    """the expressions `f` builds, one per output (an output that is a plain number becomes a sympy number)"""
    box = lambda a: np.array([_Sym(v) for v in a] + [None], dtype=object)[:-1]          # noqa: E731
    out = f(box(xs), box(us)) if ps is None else f(box(xs), box(us), box(ps))
    return [o.e if isinstance(o, _Sym) else _Sym._e(o) for o in np.asarray(out, dtype=object).reshape(-1)]


def _mp_to_ld(v):
    hi = float(v)
    return np.longdouble(hi) + np.longdouble(float(v - hi)) if np.isfinite(hi) else np.longdouble(hi)


def sympy_hessian(f, n, m, x, u, p=None, exact=False):
    """H (P, n_out, n + m, n + m) in long double: sympy derivatives of the expression `f` builds (constants at their float64 values).
    The default evaluation is the lambdified NumPy code on long-double arrays, whose numeric literals are float64: a constant that
    sympy folded from two of the callable's (0.3 * 0.4) is rounded to 2^-53.  exact=True evaluates with mpmath at 128 bits instead, the
    result rounded once to long double (slow: a few points of a small model)."""
    import sympy
    z = sympy.symbols(f"z0:{n + m}", real=True)
    q = sympy.symbols(f"q0:{max(1, 0 if p is None else np.shape(p)[-1])}", real=True)
    exprs = sympy_call(f, z[:n], z[n:], None if p is None else q)
    zz = np.concatenate([x, u] + ([] if p is None else [np.broadcast_to(np.atleast_2d(p), (len(x), np.shape(p)[-1]))]), 1)
    syms = tuple(z) + (() if p is None else tuple(q))
    Hs = np.zeros((len(x), len(exprs), n + m, n + m), dtype=np.longdouble)
    for i in range(len(exprs)):
        for a in range(n + m):
            for b in range(a, n + m):
                d = sympy.diff(exprs[i], z[a], z[b])
                if d != 0 and exact:
                    import mpmath
                    fn = sympy.lambdify(syms, d, modules="mpmath")
                    with mpmath.workprec(128):
                        Hs[:, i, a, b] = Hs[:, i, b, a] = [_mp_to_ld(fn(*[mpmath.mpf(float(v)) for v in row])) for row in zz]
                elif d != 0:
                    fn = sympy.lambdify(syms, d, modules="numpy")
                    Hs[:, i, a, b] = Hs[:, i, b, a] = fn(*[zz[:, k].astype(np.longdouble) for k in range(zz.shape[1])])
    return Hs
