"""
Reacting tracers: a tracer source that is an expression of tracer fields,

    options.add_tracer_2d('a_2d', ..., function=a_2d, source=gamma - a_2d*b_2d**2 - gamma*a_2d)

(the reference's examples/reaction/gray_scott.py), compiled into a small postfix program that the device evaluates in front of every
stage of that tracer (csrc/swe2d_reaction.hip; include/swe2d.h has the instruction set and the formulas).  The reference's source
term is ``inner(source, test)*dx`` with the live Functions (tracer_eq_2d.py:281-298): at the points of a quadrature rule the
operands are interpolated, the program gives the source, the results are integrated against the basis functions and the reference
cell's mass inverse makes nodal values of them - the L2 projection of the source into P1DG, which is what the stage kernels take.

* ``compile_source(expr, tracer_of)`` walks the structure every ``thetis_amd.expr.Expr`` records next to its lambda and returns a
  ``Program``.  ``tracer_of(function)`` is the tracer id of a Function that is the solution of a tracer on the same device (through
  ``Function._device_field``), else None.
* A source is REACTIVE only if a leaf is such a Function (``is_reactive``); every other source keeps the frozen nodal path.
* ``HostReaction`` is the numpy restatement of exactly the device pass: a device class without ``tracer_set_reaction`` is served by
  it per stage (pull the tracers, evaluate, ``tracer_set_source``).

Which values an operand sees: during a stage of tracer ``id`` the operand ``TRACER id`` is that stage's input, every other tracer
is its current buffer 0 - already stepped for tracers before it, old for tracers after it (coupled_timeintegrator_2d.py:93-113:
the reference's forms see the live Functions in that order).  With ``use_conservative_form`` the operand is the STORED field
q = H*T, and the stage kernel multiplies the source by H as it does for every source.

Not there: operands from the flow (elev, uv, depth), trigonometric functions, general quadrilaterals, several ranks, and any
implicit treatment of stiff kinetics - the explicit step bounds k*dt.
"""
import numpy as np

from .expr import Expr
from .function import Function, farm_quadrature
from .log import print_output
from .options import Constant

__all__ = ['compile_source', 'is_reactive', 'Program', 'HostReaction', 'OPS', 'MAX_CODE', 'MAX_STACK', 'MAX_CONSTS', 'MAX_FIELDS',
           'MAX_TRACERS', 'MAX_QUAD', 'MAX_DEGREE']

# include/swe2d.h SWE2D_REACTION_*, swe2d_reaction_op
MAX_CODE, MAX_STACK, MAX_CONSTS, MAX_FIELDS, MAX_TRACERS, MAX_QUAD = 64, 8, 16, 4, 8, 64
MAX_DEGREE = 14
_NAMES = ('CONST TRACER FIELD X Y ADD SUB MUL DIV NEG ABS MIN MAX POWI SQRT EXP LOG LT LE GT GE EQ NE AND OR NOT SELECT').split()
OPS = {name: i for i, name in enumerate(_NAMES)}

_BINARY = {'add': 'ADD', 'sub': 'SUB', 'mul': 'MUL', 'div': 'DIV', 'min': 'MIN', 'max': 'MAX', 'lt': 'LT', 'le': 'LE', 'gt': 'GT',
           'ge': 'GE', 'eq': 'EQ', 'ne': 'NE', 'and': 'AND', 'or': 'OR'}
_UNARY = {'neg': 'NEG', 'abs': 'ABS', 'sqrt': 'SQRT', 'exp': 'EXP', 'ln': 'LOG', 'not': 'NOT'}
_UNSUPPORTED = ('sin', 'cos', 'tan', 'tanh', 'cosh', 'sinh', 'sign')
_SUM_LIKE = ('ADD', 'SUB', 'MIN', 'MAX')
_COMPARISONS = ('LT', 'LE', 'GT', 'GE', 'EQ', 'NE', 'AND', 'OR')


def _is_number(a):
    return isinstance(a, (int, float, np.integer, np.floating)) and not isinstance(a, bool)


def _leaves(expr):
    """the Function leaves of an expression (None in the list: an Expr without a recorded structure)"""
    if isinstance(expr, Function):
        return [expr]
    if not isinstance(expr, Expr):
        return []
    if expr.node is None:
        return [None]
    out = []
    for a in expr.node[1]:
        out.extend(_leaves(a))
    return out


def has_function_leaf(expr):
    """an expression with a Function leaf, or a bare Function (``source=a_2d``)"""
    return isinstance(expr, (Expr, Function)) and any(f is not None for f in _leaves(expr))


def is_reactive(expr, tracer_of):
    """does a leaf of the expression (or the bare Function) name a field that lives on the device: the solution Function of a
    tracer, or one of the flow (which ``compile_source`` refuses)?"""
    return isinstance(expr, (Expr, Function)) and any(f is not None and tracer_of(f) is not None for f in _leaves(expr))


class Program(object):
    """A compiled source: ``code`` (int32 words op | arg << 8), ``constants`` (numbers and Constants, in slot order), ``fields``
    (coefficient Functions, slot order), ``tracers`` (ids named), ``degree`` (estimated polynomial degree), the rule ``phi``, ``w``."""

    def __init__(self, code, constants, fields, tracers, degree, npc):
        self.code = np.asarray(code, dtype=np.int32)
        self.constants, self.fields, self.tracers, self.degree, self.npc = list(constants), list(fields), list(tracers), int(degree), npc
        want = self.degree + 1                                  # + 1: the test function
        if want > MAX_DEGREE:
            print_output('reaction source of estimated degree {:d}: the quadrature degree {:d} is capped at {:d}'.format(
                self.degree, want, MAX_DEGREE))
        self.quadrature_degree = min(want, MAX_DEGREE)
        self.phi, self.w = farm_quadrature(npc, self.quadrature_degree)
        if len(self.w) > MAX_QUAD:
            raise NotImplementedError('a rule of {:d} points: the reaction pass takes at most SWE2D_REACTION_MAX_QUAD = {:d}'.format(
                len(self.w), MAX_QUAD))

    def constant_values(self):
        out = []
        for c in self.constants:
            if isinstance(c, Constant):
                v = c.values()
                if len(v) != 1:
                    raise NotImplementedError('a vector Constant in a reaction source')
                out.append(float(v[0]))
            else:
                out.append(float(c))
        return np.array(out, dtype=np.float64)

    def field_values(self):
        """the coefficient fields as (N, npc) nodal arrays (CG and DG alike: the values at the nodes of every cell)"""
        return [np.ascontiguousarray(f.cell_node_values(), dtype=np.float64) for f in self.fields]

    def signature(self):
        """changes when the device's copy is stale: the constants' values and the coefficient Functions' host versions (the tracer
        operands are read where they live)"""
        return (id(self), tuple(self.constant_values()), tuple((id(f), f._host_version) for f in self.fields))

    def disassemble(self):
        return ['{:s} {:d}'.format(_NAMES[int(w) & 255], int(w) >> 8) if _NAMES[int(w) & 255] in ('CONST', 'TRACER', 'FIELD', 'POWI')
                else _NAMES[int(w) & 255] for w in self.code]


class _Compiler(object):
    def __init__(self, tracer_of, fields=None):
        self.tracer_of = tracer_of
        self.code, self.constants, self.fields, self.tracers = [], [], list(fields or []), []
        self.depth, self.max_depth = 0, 0

    def emit(self, name, arg=0, pops=0):
        self.code.append(OPS[name] | (int(arg) << 8))
        if len(self.code) > MAX_CODE:
            raise NotImplementedError('a reaction source of more than SWE2D_REACTION_MAX_CODE = {:d} instructions'.format(MAX_CODE))
        self.depth += 1 - pops
        if self.depth > MAX_STACK:
            raise NotImplementedError('a reaction source that needs more than SWE2D_REACTION_MAX_STACK = {:d} values on the '
                                      'stack'.format(MAX_STACK))
        self.max_depth = max(self.max_depth, self.depth)

    def const(self, c):
        for i, k in enumerate(self.constants):
            if k is c or (_is_number(k) and _is_number(c) and float(k) == float(c) and np.signbit(k) == np.signbit(c)):
                break
        else:
            i = len(self.constants)
            self.constants.append(c if isinstance(c, Constant) else float(c))
            if len(self.constants) > MAX_CONSTS:
                raise NotImplementedError('a reaction source with more than SWE2D_REACTION_MAX_CONSTS = {:d} constants'.format(MAX_CONSTS))
        self.emit('CONST', i)
        return 0

    def function(self, f):
        fs = f.function_space()
        if fs.vector:
            raise NotImplementedError('a vector Function in a reaction source')
        j = self.tracer_of(f)
        if j is not None:
            if j < 0:
                raise NotImplementedError('operands from the flow (elev, uv) in a reaction source')
            if j not in self.tracers:
                self.tracers.append(j)
                if len(self.tracers) > MAX_TRACERS:
                    raise NotImplementedError('a reaction source of more than SWE2D_REACTION_MAX_TRACERS = {:d} tracers'.format(MAX_TRACERS))
            self.emit('TRACER', j)
            return 1
        if fs.degree != 1:
            raise NotImplementedError('a coefficient Function of a reaction source must be P1 (CG or DG)')
        for i, g in enumerate(self.fields):
            if g is f:
                break
        else:
            i = len(self.fields)
            self.fields.append(f)
            if len(self.fields) > MAX_FIELDS:
                raise NotImplementedError('reaction sources with more than SWE2D_REACTION_MAX_FIELDS = {:d} coefficient '
                                          'fields'.format(MAX_FIELDS))
        self.emit('FIELD', i)
        return 1

    def visit(self, a):
        """emit the code of operand ``a``; returns its estimated degree (UFL's rule)"""
        if _is_number(a) or isinstance(a, Constant):
            return self.const(a)
        if isinstance(a, Function):
            return self.function(a)
        if not isinstance(a, Expr):
            raise NotImplementedError('a {:} in a reaction source'.format(type(a).__name__))
        if a.node is None:
            raise NotImplementedError('an expression without a recorded structure in a reaction source')
        op, args = a.node
        if op == 'x' or op == 'y':
            self.emit(op.upper())
            return 1
        if op == 'function':
            return self.function(args[0])
        if op == 'constant':
            return self.const(args[0])
        if op in _UNSUPPORTED:
            raise NotImplementedError('{:s}() in a reaction source is not on the device'.format(op))
        if op in ('vector', 'component'):
            raise NotImplementedError('vector expressions in a reaction source')
        if op == 'pow':
            return self.power(*args)
        if op == 'conditional':
            self.visit(args[0])
            d1, d2 = self.visit(args[1]), self.visit(args[2])
            self.emit('SELECT', pops=3)
            return max(d1, d2)
        if op in _UNARY:
            d = self.visit(args[0])
            name = _UNARY[op]
            self.emit(name, pops=1)
            return d if name in ('NEG', 'ABS') else (0 if name == 'NOT' else d + 2)
        name = _BINARY[op]
        d1, d2 = self.visit(args[0]), self.visit(args[1])
        self.emit(name, pops=2)
        if name in _SUM_LIKE:
            return max(d1, d2)
        if name in _COMPARISONS:
            return 0
        return d1 + d2 if name == 'MUL' else max(d1, d2) + 2        # DIV

    def power(self, base, exponent):
        if not _is_number(exponent):
            raise NotImplementedError('a reaction source with an exponent that is not a number')
        e = float(exponent)
        if e == 0.5:
            d = self.visit(base)
            self.emit('SQRT', pops=1)
            return d + 2
        if e != int(e):
            raise NotImplementedError('a reaction source with the non-integer exponent {:g} (0.5 is the only one)'.format(e))
        n = int(e)
        if n == 0:
            return self.const(1.0)
        if n == 1:
            return self.visit(base)
        if not 2 <= n <= 16:
            raise NotImplementedError('a reaction source with the exponent {:d}: integer exponents are 0 .. 16'.format(n))
        d = self.visit(base)
        self.emit('POWI', n, pops=1)
        return n*d


def compile_source(expr, tracer_of, npc=3, fields=None):
    """``expr`` -> Program.  ``fields``: the coefficient Functions other programs of the same device already hold slots for (the
    slots are the device's, not the program's); the returned program's ``fields`` continues that list."""
    c = _Compiler(tracer_of, fields)
    degree = c.visit(expr)
    assert c.depth == 1
    p = Program(c.code, c.constants, c.fields, c.tracers, degree, npc)
    p.max_depth = c.max_depth
    return p


class HostReaction(object):
    """The device pass in numpy, operation for operation (include/swe2d.h): ``evaluate`` gives the (N, npc) nodal source."""

    def __init__(self, program, cell_xy):
        self.program = program
        self.xy = np.asarray(cell_xy, dtype=np.float64)                     # (N, npc, 2)

    def _at(self, q, c):
        phi = self.program.phi[q]
        v = phi[0]*c[:, 0] + phi[1]*c[:, 1]
        for i in range(2, c.shape[1]):
            v = v + phi[i]*c[:, i]
        return v

    def evaluate(self, tracer_values, field_values=None, constants=None):
        """``tracer_values``: tracer id -> (N, npc) nodal values of the operand"""
        p = self.program
        consts = p.constant_values() if constants is None else constants
        fields = p.field_values() if field_values is None else field_values
        n, npc = self.xy.shape[:2]
        b = [np.zeros(n) for _ in range(npc)]
        one, zero = np.ones(n), np.zeros(n)
        with np.errstate(all='ignore'):
            for q in range(len(p.w)):
                st = []
                for word in p.code:
                    name, arg = _NAMES[int(word) & 255], int(word) >> 8
                    if name == 'CONST':
                        st.append(np.full(n, consts[arg]))
                    elif name == 'TRACER':
                        st.append(self._at(q, np.asarray(tracer_values[arg], dtype=np.float64).reshape(n, npc)))
                    elif name == 'FIELD':
                        st.append(self._at(q, fields[arg]))
                    elif name == 'X':
                        st.append(self._at(q, self.xy[:, :, 0]))
                    elif name == 'Y':
                        st.append(self._at(q, self.xy[:, :, 1]))
                    elif name == 'NEG':
                        st[-1] = -st[-1]
                    elif name == 'ABS':
                        st[-1] = np.abs(st[-1])
                    elif name == 'POWI':
                        x = st[-1]
                        r = x
                        for _ in range(arg - 1):
                            r = r*x
                        st[-1] = r
                    elif name == 'SQRT':
                        st[-1] = np.sqrt(st[-1])
                    elif name == 'EXP':
                        st[-1] = np.exp(st[-1])
                    elif name == 'LOG':
                        st[-1] = np.log(st[-1])
                    elif name == 'NOT':
                        st[-1] = np.where(st[-1] == 0.0, one, zero)
                    elif name == 'SELECT':
                        y = st.pop()
                        x = st.pop()
                        c = st.pop()
                        st.append(np.where(c != 0.0, x, y))
                    else:
                        y = st.pop()
                        x = st.pop()
                        if name == 'ADD':
                            r = x + y
                        elif name == 'SUB':
                            r = x - y
                        elif name == 'MUL':
                            r = x*y
                        elif name == 'DIV':
                            r = x/y
                        elif name == 'MIN':
                            r = np.where(y < x, y, x)
                        elif name == 'MAX':
                            r = np.where(y > x, y, x)
                        elif name == 'AND':
                            r = np.where((x != 0.0) & (y != 0.0), one, zero)
                        elif name == 'OR':
                            r = np.where((x != 0.0) | (y != 0.0), one, zero)
                        else:
                            cmp_ = {'LT': np.less, 'LE': np.less_equal, 'GT': np.greater, 'GE': np.greater_equal, 'EQ': np.equal,
                                    'NE': np.not_equal}[name]
                            r = np.where(cmp_(x, y), one, zero)
                        st.append(r)
                s = st.pop()
                assert not st
                for i in range(npc):
                    b[i] = b[i] + (p.w[q]*p.phi[q][i])*s
            if npc == 3:
                t = (b[0] + b[1]) + b[2]
                out = [12.0*b[i] - 3.0*t for i in range(3)]
            else:
                out = [(16.0*b[i] - 8.0*(b[(i + 1) % 4] + b[(i + 3) % 4])) + 4.0*b[(i + 2) % 4] for i in range(4)]
        return np.stack(out, axis=1)
