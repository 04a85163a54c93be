"""Recorder behind `models.TracedModel`: a dynamics callable `f(x, u[, p]) -> x+` is called once on NumPy object arrays of recording
scalars and leaves a straight-line tape that the device interpreter (zopt_amd/csrc/tape_model.h) evaluates on double, dual and
hyper-dual numbers.

Recorded: `+ - * /` and unary minus (either side, with Python and NumPy numbers), `** k` for k = 1..8 as products, and the ufuncs
np.sin, np.cos, np.tan, np.sqrt (NumPy dispatches a ufunc on an object array to the method of that name of each element), so indexing,
np.array, np.concatenate, `@` and np.cross work as they are.  Anything else is a TypeError that names the operation; `bool()` of a
recorded scalar or a comparison -- a data-dependent branch -- is a TypeError that says so.

Constants are folded, equal subexpressions are recorded once, dead code is dropped; nothing is simplified algebraically (`0.0 * e`
stays an instruction: the value path is IEEE-faithful to the callable, NaN included).

The tape: 32-bit words  op | a_is_const << 6 | b_is_const << 7 | dst << 8 | a << 16 | b << 24  over a slot file; the inputs x, u, p
are pinned in slots 0 .. n+m+np-1, temporaries are reused after their last use (lowest free slot first, in recording order), `outputs`
names the n slots that hold x+ at the end.  An operand flagged as a constant indexes the fp64 constant table instead of the slot file.

`models.TracedCost` records its two cost callables with the same recorder (`record(..., n_out=1)`: one output; `controls=False` for
terminalCost(x[, p]), whose tape keeps the control slots reserved and unread so that both tapes share the layout x, u, p); the device
side is zopt_amd/csrc/tape_cost.h.  `models.TracedConstraint` records g(x, u[, p]) and terminal(x[, p]) likewise, with `n_out = n_con`
resp. `n_con_terminal` outputs (device side: zopt_amd/csrc/tape_con.h).
"""
from __future__ import annotations

import struct
from typing import NamedTuple

import numpy as np

OPS = ("add", "sub", "mul", "div", "neg", "sin", "cos", "tan", "sqrt", "mov")
OP = {name: i for i, name in enumerate(OPS)}
A_CONST, B_CONST = 0x40, 0x80
MAX_N, MAX_M, MAX_P = 12, 4, 8
MAX_INSTR, MAX_SLOTS, MAX_CONSTS = 1024, 64, 256
_UNARY = {"neg": lambda a: -a, "sin": np.sin, "cos": np.cos, "tan": np.tan, "sqrt": np.sqrt}
_BINARY = {"add": lambda a, b: a + b, "sub": lambda a, b: a - b, "mul": lambda a, b: a * b, "div": lambda a, b: a / b}


class Tape(NamedTuple):
    """code (K,) uint32, consts (C,) float64, outputs (n,) slot numbers ((1,) for a cost), n_slots (inputs included), n, m, n_params,
    mask"""
    code: np.ndarray
    consts: np.ndarray
    outputs: tuple
    n_slots: int
    n: int
    m: int
    n_params: int
    mask: int

    def decode(self):
        """[(op name, dst, (a_is_const, a), (b_is_const, b))] -- for tests and documentation"""
        return [(OPS[w & 0x3F], (w >> 8) & 0xFF, (bool(w & A_CONST), (w >> 16) & 0xFF), (bool(w & B_CONST), (w >> 24) & 0xFF))
                for w in (int(v) for v in self.code)]


def _number(v):
    """a Python float for what counts as a number on the other side of an operator, else None"""
    if isinstance(v, (bool, np.bool_)):
        return None
    if isinstance(v, (int, float, np.integer, np.floating)):
        return float(v)
    if isinstance(v, np.ndarray) and v.ndim == 0 and v.dtype.kind in "iuf":
        return float(v)
    return None


class _Trace:
    def __init__(self):
        self.nodes = []         # (op, (is_const, index), (is_const, index) | None); inputs: ("in", slot, None)
        self.dep = []           # per node: bit mask of the variables (states, controls) it depends on
        self.memo = {}
        self.consts = []
        self.const_ids = {}

    def const(self, v):
        key = struct.pack("<d", float(v))      # by bit pattern: -0.0 is not 0.0, a NaN is itself
        if key not in self.const_ids:
            self.const_ids[key] = len(self.consts)
            self.consts.append(float(v))
        return (True, self.const_ids[key])

    def node(self, op, a, b=None):
        key = (op, a, b)
        if key not in self.memo:
            self.memo[key] = len(self.nodes)
            self.nodes.append(key)
            self.dep.append((0 if a[0] else self.dep[a[1]]) | (0 if b is None or b[0] else self.dep[b[1]]))
        return _Rec(self, self.memo[key])

    def input(self, slot, bit):
        self.nodes.append(("in", slot, None))
        self.dep.append(bit)
        return _Rec(self, len(self.nodes) - 1)


def _refuse(what):
    raise TypeError(f"TracedModel: `{what}` is not a recorded operation (recorded: + - * / unary minus, ** k for k = 1..8, np.sin, "
                    "np.cos, np.tan, np.sqrt)")


def _branch(what):
    raise TypeError(f"TracedModel: {what} of a recorded scalar is a data-dependent branch; a traced model is one straight-line "
                    "expression")


class _Rec:
    """a recording scalar"""
    __slots__ = ("tr", "id")

    def __init__(self, tr, node_id):
        self.tr, self.id = tr, node_id

    def _operand(self, v):
        if isinstance(v, _Rec):
            if v.tr is not self.tr:
                raise TypeError("TracedModel: a recorded scalar of another trace")
            return (False, v.id)
        c = _number(v)
        return None if c is None else self.tr.const(c)

    def _binary(self, op, other, swap=False):
        o = self._operand(other)
        if o is None:
            return NotImplemented
        a, b = ((False, self.id), o) if not swap else (o, (False, self.id))
        return self.tr.node(op, a, b)

    def __add__(self, o): return self._binary("add", o)
    def __radd__(self, o): return self._binary("add", o, True)
    def __sub__(self, o): return self._binary("sub", o)
    def __rsub__(self, o): return self._binary("sub", o, True)
    def __mul__(self, o): return self._binary("mul", o)
    def __rmul__(self, o): return self._binary("mul", o, True)
    def __truediv__(self, o): return self._binary("div", o)
    def __rtruediv__(self, o): return self._binary("div", o, True)
    def __neg__(self): return self.tr.node("neg", (False, self.id))
    def __pos__(self): return self

    def __pow__(self, k, mod=None):
        c = _number(k)
        if mod is not None or c is None or c != int(c) or not 1 <= int(c) <= 8:
            _refuse(f"** {k!r}")
        r = self
        for _ in range(int(c) - 1):
            r = r * self
        return r

    def __rpow__(self, o): _refuse("** with a recorded exponent")
    def sin(self): return self.tr.node("sin", (False, self.id))
    def cos(self): return self.tr.node("cos", (False, self.id))
    def tan(self): return self.tr.node("tan", (False, self.id))
    def sqrt(self): return self.tr.node("sqrt", (False, self.id))

    def __bool__(self): _branch("bool()")
    def __lt__(self, o): _branch("a comparison (<)")
    def __le__(self, o): _branch("a comparison (<=)")
    def __gt__(self, o): _branch("a comparison (>)")
    def __ge__(self, o): _branch("a comparison (>=)")
    def __eq__(self, o): _branch("a comparison (==)")
    def __ne__(self, o): _branch("a comparison (!=)")
    __hash__ = object.__hash__
    def __float__(self): _refuse("float()")
    def __int__(self): _refuse("int()")
    def __abs__(self): _refuse("abs")
    def __floordiv__(self, o): _refuse("//")
    def __rfloordiv__(self, o): _refuse("//")
    def __mod__(self, o): _refuse("%")
    def __rmod__(self, o): _refuse("%")

    def __getattr__(self, name):
        # NumPy looks a ufunc up as a method of the element (np.exp -> .exp): name what is not recorded
        if name.startswith("__"):
            raise AttributeError(name)
        _refuse(f"np.{name}")


def _fold(tr):
    """constant folding: a node all of whose operands are constants becomes a constant (computed as the callable itself would on
    float64); returns per node None or the (True, index) operand that replaces it"""
    repl = [None] * len(tr.nodes)
    sub = lambda o: o if o is None or o[0] or repl[o[1]] is None else repl[o[1]]          # noqa: E731
    nodes = []
    for i, (op, a, b) in enumerate(tr.nodes):
        if op == "in":
            nodes.append((op, a, b))
            continue
        a, b = sub(a), sub(b)
        if a[0] and (b is None or b[0]):
            with np.errstate(all="ignore"):
                va = np.float64(tr.consts[a[1]])
                v = _UNARY[op](va) if b is None else _BINARY[op](va, np.float64(tr.consts[b[1]]))
            repl[i] = tr.const(float(v))
        nodes.append((op, a, b))
    return nodes, repl


def record(f, n, m, n_params=0, n_out=None, controls=True, who="TracedModel"):
    """Trace `f` once; returns the Tape.  ValueError for sizes outside the caps or a wrong output length, TypeError for what the
    recorder refuses.  n_out: how many values `f` returns (None: n, a dynamics function; 1: a cost, whose result may also be a
    recorded scalar or a 0-d array).  controls=False: `f` is called as f(x) / f(x, p); the control slots n .. n+m-1 stay reserved, so
    that the slot layout [x | u | p] is the same, and are never read.  who: the name the messages of this call carry."""
    n, m, n_params = int(n), int(m), int(n_params)
    n_out = n if n_out is None else int(n_out)
    if not (1 <= n <= MAX_N and 1 <= m <= MAX_M and 0 <= n_params <= MAX_P):
        raise ValueError(f"{who}: (n={n}, m={m}, params={n_params}) outside the interpreter's caps (1 <= n <= {MAX_N}, "
                         f"1 <= m <= {MAX_M}, params <= {MAX_P})")
    tr = _Trace()
    n_in = n + m + n_params
    ins = [tr.input(s, (1 << s) if s < n + m else 0) for s in range(n_in)]
    obj = lambda lst: np.array(lst + [None], dtype=object)[:-1]                               # noqa: E731  (1-d, whatever it holds)
    x, u, p = obj(ins[:n]), obj(ins[n:n + m]), obj(ins[n + m:])
    args = ((x, u) if controls else (x,)) + ((p,) if n_params else ())
    out = f(*args)
    out = np.asarray(out, dtype=object).reshape(-1)
    if out.shape[0] != n_out:
        raise ValueError(f"{who}: the callable returned {out.shape[0]} values, " +
                         (f"the next state has n = {n}" if n_out == n and who == "TracedModel" else f"expected {n_out}"))
    nodes, repl = _fold(tr)
    outs = []
    for v in out:
        if isinstance(v, _Rec):
            outs.append((False, v.id) if repl[v.id] is None else repl[v.id])
        else:
            c = _number(v)
            if c is None:
                raise TypeError(f"{who}: the callable returned a {type(v).__name__}, expected recorded scalars or numbers")
            outs.append(tr.const(c))
    # a constant output is moved into a slot of its own by one instruction
    for k, o in enumerate(outs):
        if o[0]:
            nodes.append(("mov", o, None))
            tr.dep.append(0)
            repl.append(None)
            outs[k] = (False, len(nodes) - 1)
    # dead code: what no output reaches
    live = [False] * len(nodes)
    stack = [o[1] for o in outs]
    while stack:
        i = stack.pop()
        if live[i]:
            continue
        live[i] = True
        for o in nodes[i][1:] if nodes[i][0] != "in" else ():
            if o is not None and not o[0]:
                stack.append(o[1])
    order = [i for i, nd in enumerate(nodes) if live[i] and nd[0] != "in"]
    # the constants that are left, renumbered in order of first use
    cmap, consts = {}, []

    def cref(o):
        if o[1] not in cmap:
            cmap[o[1]] = len(consts)
            consts.append(tr.consts[o[1]])
        return cmap[o[1]]
    # structural mask: sums pass dependencies on; a product of two operands that depend on a variable marks the union of their
    # dependencies, a quotient its denominator's as well; a unary function marks its operand's
    mask = 0
    dep = tr.dep
    for i in order:
        op, a, b = nodes[i]
        da = 0 if a[0] else dep[a[1]]
        db = 0 if b is None or b[0] else dep[b[1]]
        if op in ("sin", "cos", "tan", "sqrt"):
            mask |= da
        elif op == "mul" and da and db:
            mask |= da | db
        elif op == "div" and db:
            mask |= da | db
    # slots: inputs pinned, temporaries by linear scan in recording order
    last = {}
    for pos, i in enumerate(order):
        for o in nodes[i][1:]:
            if o is not None and not o[0]:
                last[o[1]] = pos
    for o in outs:
        last[o[1]] = len(order)            # outputs survive to the end
    slot = {i: nodes[i][1] for i, nd in enumerate(nodes) if nd[0] == "in"}
    import heapq
    free, top, code = [], n_in, []
    for pos, i in enumerate(order):
        op, a, b = nodes[i]
        word = OP[op]
        fields = []
        for o, flag in ((a, A_CONST), (b, B_CONST)):
            if o is None:
                fields.append(0)
            elif o[0]:
                word |= flag
                fields.append(cref(o))
            else:
                fields.append(slot[o[1]])
        # an operand that dies here gives its slot up before the destination is chosen (the interpreter reads both operands first)
        for o in {o[1] for o in (a, b) if o is not None and not o[0]}:
            if last[o] == pos and nodes[o][0] != "in":
                heapq.heappush(free, slot[o])
        if free:
            d = heapq.heappop(free)
        else:
            d, top = top, top + 1
        slot[i] = d
        if last.get(i, -1) < pos + 1 and i not in {o[1] for o in outs}:      # (cannot happen for a live node; kept as a guard)
            heapq.heappush(free, d)
        code.append(word | (d & 0xFF) << 8 | fields[0] << 16 | fields[1] << 24)
        if top > 256:
            break
    if len(code) > MAX_INSTR or len(order) > MAX_INSTR:
        raise ValueError(f"{who}: {len(order)} instructions, the interpreter takes {MAX_INSTR}")
    if top > MAX_SLOTS:
        raise ValueError(f"{who}: more than {MAX_SLOTS} slots are live at once (inputs included)")
    if len(consts) > MAX_CONSTS:
        raise ValueError(f"{who}: {len(consts)} constants, the interpreter takes {MAX_CONSTS}")
    return Tape(np.array(code, dtype=np.uint32), np.array(consts, dtype=np.float64), tuple(slot[o[1]] for o in outs), top, n, m,
                n_params, mask)


def blob(tape):
    """The tape as the device reads it, one buffer of 8-byte words: the constants, then the instruction words, then the n output
    slots as 32-bit words (zero padded to a whole 8-byte word)."""
    words = np.concatenate([tape.code.astype(np.uint32), np.array(tape.outputs, dtype=np.uint32)])
    if words.size % 2:
        words = np.concatenate([words, np.zeros(1, dtype=np.uint32)])
    return np.concatenate([tape.consts.view(np.uint64), words.view(np.uint64)])
