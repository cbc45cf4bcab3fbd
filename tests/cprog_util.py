"""Test helper: constraint programs (wf_cprog, include/wf_lde.h) and their interpreter restated on Python integers.

Values are the library's in-memory elements as Python integers (f64: Montgomery residues x * 2^64 mod p; f128: canonical), so a
product is a * b * 2^-64 mod p for f64 and a * b mod p for f128 -- the canonical product carried back into memory form -- and
sums and differences are the plain ones mod p.  The three extension products are written out from the reference
(math/src/field/f64/mod.rs:401-472, math/src/field/f128/mod.rs:273-279).  A program is evaluated for all steps at once on numpy
object arrays of integers.  The typing rules are restated here as well (a value is a base array or a list of `ext` arrays).

Builders: do_work, fib, periodic, sequence, stress (see each)."""
import numpy as np

import edge_util as E

F64, F128 = 1, 2
ADD, SUB, MUL = 1, 2, 3
REG, CUR, NEXT, CONST, ECONST, TABLE, X = 0, 1, 2, 3, 4, 5, 6
P = E.MODULUS
RINV = {F64: E.R64_INV, F128: 1}
TWO_ADICITY = {F64: 32, F128: 40}
TWO_ADIC_ROOT = {F64: 7277203076849721926, F128: 23953097886125630542083529559205016746}
MAX_FOOTPRINT = {F64: 64, F128: 32}


def to_mem(field, v):
    """canonical integer -> memory representation"""
    return v * 2**64 % P[field] if field == F64 else v % P[field]


def root_of_unity(field, log_n):
    """canonical"""
    return pow(TWO_ADIC_ROOT[field], 1 << (TWO_ADICITY[field] - log_n), P[field])


class Prog:
    """instrs: [(op, dst, (a_src, a), (b_src, b))]; consts: integers; econsts: tuples of `ext` integers; tables: [(values, shift)]."""

    def __init__(self, n_regs):
        self.instrs, self.n_regs, self.out_regs = [], n_regs, []
        self.consts, self.econsts, self.tables = [], [], []

    def op(self, op, dst, a, b):
        self.instrs.append((op, dst, a, b))
        return (REG, dst)

    def add(self, dst, a, b):
        return self.op(ADD, dst, a, b)

    def sub(self, dst, a, b):
        return self.op(SUB, dst, a, b)

    def mul(self, dst, a, b):
        return self.op(MUL, dst, a, b)

    def const(self, v):
        self.consts.append(v)
        return (CONST, len(self.consts) - 1)

    def econst(self, v):
        self.econsts.append(tuple(v))
        return (ECONST, len(self.econsts) - 1)

    def table(self, values, shift=0):
        self.tables.append((list(values), shift))
        return (TABLE, len(self.tables) - 1)


def to_capi(capi, prog, field, ext):
    """-> (Cprog, keep) of capi.make_cprog"""
    consts = E.elements(field, prog.consts) if prog.consts else None
    econsts = E.elements(field, [c for e in prog.econsts for c in e]) if prog.econsts else None
    tables = [(E.elements(field, v), s) for v, s in prog.tables]
    return capi.make_cprog(field, ext, prog.instrs, prog.n_regs, prog.out_regs, consts, econsts, tables)


# ------------------------------------------------------------------------------------------------ field arithmetic
def _mul(field, a, b):
    return a * b * RINV[field] % P[field]


def ext_mul(field, ext, a, b):
    p = P[field]
    m = lambda x, y: _mul(field, x, y)  # noqa: E731
    if ext == 2 and field == F64:      # phi^2 = phi - 2
        a0b0 = m(a[0], b[0])
        return [(a0b0 - 2 * m(a[1], b[1])) % p, (m((a[0] + a[1]) % p, (b[0] + b[1]) % p) - a0b0) % p]
    if ext == 2:                        # f128: phi^2 = phi + 1
        a0b0, a1b1 = m(a[0], b[0]), m(a[1], b[1])
        return [(a0b0 + a1b1) % p, (m((a[0] + a[1]) % p, (b[0] + b[1]) % p) - a0b0) % p]
    # cubic over f64: phi^3 = phi + 1
    d0 = m(a[0], b[0])
    d1 = (m(a[0], b[1]) + m(a[1], b[0])) % p
    d2 = (m(a[0], b[2]) + m(a[1], b[1]) + m(a[2], b[0])) % p
    d3 = (m(a[1], b[2]) + m(a[2], b[1])) % p
    d4 = m(a[2], b[2])
    return [(d0 + d3) % p, (d1 + d3 + d4) % p, (d2 + d4) % p]


def _apply(field, ext, op, a, b):
    """a, b: base arrays or lists of `ext` arrays"""
    p = P[field]
    ae, be = isinstance(a, list), isinstance(b, list)
    if not ae and not be:
        return (a + b) % p if op == ADD else (a - b) % p if op == SUB else _mul(field, a, b)
    if op == MUL:
        if ae and be:
            return ext_mul(field, ext, a, b)
        e, s = (a, b) if ae else (b, a)
        return [_mul(field, c, s) for c in e]  # mul_base
    zero = 0 * (a[0] if ae else b[0])
    a = a if ae else [a] + [zero] * (ext - 1)
    b = b if be else [b] + [zero] * (ext - 1)
    return [(x + y) % p if op == ADD else (x - y) % p for x, y in zip(a, b)]


def typing(prog, ext):
    """Per register 0 (never written), 1 (base) or 2 (E), and the sets of CUR / NEXT columns read -- the header's rules."""
    types = [0] * prog.n_regs
    cur, nxt = set(), set()
    for op, dst, a, b in prog.instrs:
        is_e = False
        for src, idx in (a, b):
            if src == REG:
                assert types[idx], "read before written"
                is_e |= types[idx] == 2
            elif src == ECONST:
                is_e |= ext > 1
            elif src == CUR:
                cur.add(idx)
            elif src == NEXT:
                nxt.add(idx)
        t = 2 if is_e else 1
        assert types[dst] in (0, t), "second type"
        types[dst] = t
    return types, cur, nxt


def frame_rows(lde, lde_blowup, ce_blowup):
    """lde: (n, row_width) object array -> (cur, next) of shape (ce, row_width) (trace_lde.rs:78-93)"""
    n = lde.shape[0]
    ce = n // lde_blowup * ce_blowup
    steps = np.arange(ce) * (lde_blowup // ce_blowup)
    return lde[steps], lde[(steps + lde_blowup) % n]


def ce_points(field, ce, offset):
    """x at every step, memory representation: offset * g_ce^step (domain.rs:124-131)"""
    p, g = P[field], root_of_unity(field, ce.bit_length() - 1)
    out, x = [], offset % p
    for _ in range(ce):
        out.append(to_mem(field, x))
        x = x * g % p
    return np.array(out, dtype=object)


def evaluate(prog, field, ext, cur, nxt, xs):
    """The evaluation columns: a list of (ce * ext,) object arrays, coordinates of an element side by side."""
    ce = len(xs)
    steps = np.arange(ce)
    regs = [None] * prog.n_regs

    def fetch(src, idx):
        if src == REG:
            assert regs[idx] is not None
            return regs[idx]
        if src == CUR:
            return cur[:, idx]
        if src == NEXT:
            return nxt[:, idx]
        if src == CONST:
            return np.array([prog.consts[idx]] * ce, dtype=object)
        if src == ECONST:
            cols = [np.array([c] * ce, dtype=object) for c in prog.econsts[idx]]
            return cols if ext > 1 else cols[0]
        if src == TABLE:
            values, shift = prog.tables[idx]
            return np.array(values, dtype=object)[(steps - shift) % len(values)]
        assert src == X
        return xs

    for op, dst, a, b in prog.instrs:
        r = _apply(field, ext, op, fetch(*a), fetch(*b))
        assert regs[dst] is None or isinstance(regs[dst], list) == isinstance(r, list)
        regs[dst] = r
    out = []
    for r in prog.out_regs:
        v = regs[r]
        if not isinstance(v, list):
            v = [v] + [np.array([0] * ce, dtype=object)] * (ext - 1)
        col = np.empty(ce * ext, dtype=object)
        for w in range(ext):
            col[w::ext] = v[w]
        out.append(col)
    return out


def lde_ints(field, arr):
    """a read_lde array -> (n, row_width) object array of integers"""
    a = np.asarray(arr, dtype=np.uint64)
    if field == F64:
        return a.astype(object)
    n, rw = a.shape[0], a.shape[1]
    return np.array(E.f128_ints(a), dtype=object).reshape(n, rw)


def column_ints(field, arr):
    return np.asarray(arr, dtype=np.uint64).tolist() if field == F64 else E.f128_ints(arr)


# ------------------------------------------------------------------------------------------------ draws
def draw(rng, field, n):
    """n integers from the field's limb alphabet"""
    a = E.alphabet_array(field)
    rows = a[rng.integers(0, a.shape[0], size=n)]
    return column_ints(field, rows)


def draw_e(rng, field, ext):
    return tuple(draw(rng, field, ext))


# ------------------------------------------------------------------------------------------------ the programs
def do_work(field, ext, coef, start, result, bcoefs):
    """examples/src/do_work/air.rs: next - (cur^3 + 42) merged with one E coefficient (evaluator.rs:266-275), and the two single
    assertions as boundary columns (cur[0] - value) * coef.  start / result: memory representation."""
    g = Prog(5)
    c = (CUR, 0)
    g.mul(0, c, c)
    g.mul(0, (REG, 0), c)
    g.add(0, (REG, 0), g.const(to_mem(field, 42)))
    g.sub(0, (NEXT, 0), (REG, 0))
    g.mul(1, g.econst(coef), (REG, 0))
    for k, (value, bc) in enumerate(((start, bcoefs[0]), (result, bcoefs[1]))):
        g.sub(2, c, g.const(value))
        g.mul(3 + k, (REG, 2), g.econst(bc))
    g.out_regs = [1, 3, 4]
    return g


def fib(field, ext, coefs):
    """Two columns, two constraints: next0 = cur0 + cur1, next1 = cur1 + next0; merged with two E coefficients."""
    g = Prog(4)
    g.add(0, (CUR, 0), (CUR, 1))
    g.sub(0, (NEXT, 0), (REG, 0))
    g.add(1, (CUR, 1), (NEXT, 0))
    g.sub(1, (NEXT, 1), (REG, 1))
    g.mul(2, (REG, 0), g.econst(coefs[0]))
    g.mul(3, (REG, 1), g.econst(coefs[1]))
    g.add(2, (REG, 2), (REG, 3))
    g.out_regs = [2]
    return g


def periodic(field, ext, rng, ce_blowup):
    """A degree-7 S-box-style round over 4 columns: t_i = cur_i + k_(i mod 2) with two periodic tables of 2 and 8 times ce_blowup
    values, s_i = t_i^7, next_i - (s_i + m_i * s_(i+1)); merged with four E coefficients; the first difference is a second,
    base-typed, evaluation column."""
    g = Prog(14)
    tabs = [g.table(draw(rng, field, 2 * ce_blowup)), g.table(draw(rng, field, 8 * ce_blowup))]
    for i in range(4):
        t = g.add(8, (CUR, i), tabs[i % 2])
        t2 = g.mul(9, t, t)
        t4 = g.mul(10, t2, t2)
        t6 = g.mul(10, t4, t2)
        g.mul(i, t6, t)
    for i in range(4):
        m = g.mul(8, (REG, (i + 1) % 4), g.const(draw(rng, field, 1)[0]))
        m = g.add(8, (REG, i), m)
        g.sub(4 + i, (NEXT, i), m)
    for i in range(4):
        g.mul(13 if i else 12, (REG, 4 + i), g.econst(draw_e(rng, field, ext)))
        if i:
            g.add(12, (REG, 12), (REG, 13))
    g.out_regs = [12, 4]
    return g


def sequence(field, ext, rng, ce, n_cols):
    """Two boundary columns: one whose value comes from a TABLE with a non-zero shift (LargePolyConstraint::evaluate,
    boundary.rs:447-460), one whose value is a Horner polynomial in X (SmallPolyConstraint)."""
    g = Prog(5)
    length = max(2, ce // 4)
    t = g.table(draw(rng, field, length), shift=length - 1)
    g.sub(0, (CUR, 0), t)
    g.mul(1, (REG, 0), g.econst(draw_e(rng, field, ext)))
    h = g.const(draw(rng, field, 1)[0])
    for _ in range(3):
        h = g.mul(2, h, (X, 0))
        h = g.add(2, h, g.const(draw(rng, field, 1)[0]))
    g.sub(3, (CUR, n_cols - 1), h)
    g.mul(4, g.econst(draw_e(rng, field, ext)), (REG, 3))
    g.out_regs = [1, 4]
    return g


def stress(field, ext, rng, ce, n_cols, n_instrs=300):
    """A random straight-line program of n_instrs instructions on the full register footprint (64 f64 / 32 f128 base elements):
    register reuse, r = r * r, both operands the same register, all op typings (BB, EB, BE, EE with ext > 1), every source
    kind, tables of 2 and ce values (the long one shifted), constants and table values from the limb alphabet.  Products of TWO
    alphabet values -- what tells a wrong carry mask apart -- are there by construction: CONST x CONST and TABLE x CONST for both
    tables, added into two of the evaluation columns at the end.  (Column 0 times a constant is in as well, but a frame value is
    an LDE row on a coset: the extension of an alphabet-valued trace column is not alphabet-valued.)"""
    fp = MAX_FOOTPRINT[field]
    n_e = 0 if ext == 1 else fp // (2 * ext)
    n_b = fp - n_e * ext
    g = Prog(n_b + n_e)
    for v in draw(rng, field, 12):
        g.const(v)
    for _ in range(4):
        g.econst(draw_e(rng, field, ext))
    g.table(draw(rng, field, 2))
    g.table(draw(rng, field, ce), shift=int(rng.integers(1, ce)))
    is_e = [r >= n_b for r in range(g.n_regs)]
    written = [False] * g.n_regs

    def base_src():
        k = int(rng.integers(0, 7))
        regs = [r for r in range(n_b) if written[r]]
        if k <= 1 and regs:
            return (REG, regs[int(rng.integers(0, len(regs)))])
        if k == 2:
            return (NEXT, int(rng.integers(0, n_cols)))
        if k == 3:
            return (CONST, int(rng.integers(0, len(g.consts))))
        if k == 4:
            return (TABLE, int(rng.integers(0, 2)))
        if k == 5:
            return (X, 0)
        return (CUR, int(rng.integers(0, n_cols)))

    def e_src():
        regs = [r for r in range(n_b, g.n_regs) if written[r]]
        if regs and rng.integers(0, 4):
            return (REG, regs[int(rng.integers(0, len(regs)))])
        return (ECONST, int(rng.integers(0, len(g.econsts))))

    def emit(dst):
        op = int(rng.integers(1, 4))
        if not is_e[dst]:
            a, b = base_src(), base_src()
        else:
            a, b = [(e_src(), base_src()), (base_src(), e_src()), (e_src(), e_src())][int(rng.integers(0, 3))]
        g.op(op, dst, a, b)
        written[dst] = True

    order = list(rng.permutation(g.n_regs))
    for r in order:  # every register written once: the whole footprint is in use
        emit(int(r))
    for k in range(4):  # a frame column times an alphabet constant, then squared in place
        g.mul(k, (CUR, 0), (CONST, k))
        g.mul(k, (REG, k), (REG, k))
    if n_e:
        g.mul(n_b, (REG, n_b), (REG, n_b))
        g.mul(n_b + 1, (REG, n_b), (REG, n_b))
    while len(g.instrs) < n_instrs - 6:
        emit(int(rng.integers(0, g.n_regs)))
    for out, a, b in ((0, (CONST, 4), (CONST, 5)), (1, (TABLE, 0), (CONST, 6)), (0, (TABLE, 1), (CONST, 7))):
        g.mul(4, a, b)  # alphabet x alphabet
        g.add(out, (REG, out), (REG, 4))
    outs = [0, 1, n_b - 1] + ([n_b, n_b + 1, g.n_regs - 1] if n_e else [2, 3])
    g.out_regs = outs
    return g


def wide_frame(field, n_read):
    """Columns 0 .. n_read - 1 read in BOTH rows, on a full register file of base registers: 2 * n_read + 64 (f64) / 32 (f128) LDS
    slots.  One evaluation column: the sum of all registers."""
    fp = MAX_FOOTPRINT[field]
    g = Prog(fp)
    for r in range(fp):
        g.add(r, (CUR, r % n_read), (NEXT, r % n_read))
    for c in range(n_read):
        g.mul(c % fp, (REG, c % fp), (CUR, c))
        g.add(c % fp, (REG, c % fp), (NEXT, c))
    for r in range(1, fp):
        g.add(0, (REG, 0), (REG, r))
    g.out_regs = [0]
    return g


def build(name, field, ext, rng, ce, ce_blowup, n_cols):
    """One of the five programs for a trace of n_cols columns (programs that need more columns than there are fold the index)."""
    if name == "do_work":
        return do_work(field, ext, draw_e(rng, field, ext), draw(rng, field, 1)[0], draw(rng, field, 1)[0],
                       [draw_e(rng, field, ext), draw_e(rng, field, ext)])
    if name == "fib":
        g = fib(field, ext, [draw_e(rng, field, ext), draw_e(rng, field, ext)])
    elif name == "periodic":
        g = periodic(field, ext, rng, ce_blowup)
    elif name == "sequence":
        return sequence(field, ext, rng, ce, n_cols)
    else:
        return stress(field, ext, rng, ce, n_cols)
    if n_cols < 4:  # fib wants 2 columns, periodic 4
        g.instrs = [(op, d, (a[0], a[1] % n_cols if a[0] in (CUR, NEXT) else a[1]), (b[0], b[1] % n_cols if b[0] in (CUR, NEXT) else b[1]))
                    for op, d, a, b in g.instrs]
    return g


PROGRAMS = ("do_work", "fib", "periodic", "sequence", "stress")
