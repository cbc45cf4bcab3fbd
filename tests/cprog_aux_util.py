"""Test helper: constraint programs that read the auxiliary segment's frame (wf_constraint_evaluate_aux, include/wf_lde.h) and
their interpreter restated on Python integers.  Field helpers, the program builder and the five main-only programs are those of
tests/cprog_util.py; this file adds the two sources AUX_CUR / AUX_NEXT -- element c of E of an auxiliary row is the `ext`
base elements at c * ext --, which are of type E, and the programs perm, full, aux_only and aux_stress (see each)."""
import numpy as np

import cprog_util as U
from cprog_util import ADD, CONST, CUR, ECONST, MUL, NEXT, REG, SUB, TABLE, X, Prog  # noqa: F401

AUX_CUR, AUX_NEXT = 7, 8
F64, F128 = U.F64, U.F128


def typing(prog, ext):
    """Per register 0 (never written), 1 (base) or 2 (E), and the sets of CUR / NEXT / AUX_CUR / AUX_NEXT columns read."""
    types = [0] * prog.n_regs
    cur, nxt, acur, anxt = set(), set(), set(), set()
    for op, dst, a, b in prog.instrs:
        is_e = False
        for src, idx in (a, b):
            if src == REG:
                assert types[idx], "read before written"
                is_e |= types[idx] == 2
            elif src in (ECONST, AUX_CUR, AUX_NEXT):
                is_e |= ext > 1
                if src == AUX_CUR:
                    acur.add(idx)
                elif src == AUX_NEXT:
                    anxt.add(idx)
            elif src == CUR:
                cur.add(idx)
            elif src == NEXT:
                nxt.add(idx)
        t = 2 if is_e else 1
        assert types[dst] in (0, t), "second type"
        types[dst] = t
    return types, cur, nxt, acur, anxt


def strip_aux(prog):
    """The program with every auxiliary source replaced by ECONST 0 (the same type): what is left reads the main segment only."""
    g = Prog(prog.n_regs)
    g.consts, g.econsts, g.tables, g.out_regs = list(prog.consts), list(prog.econsts), list(prog.tables), list(prog.out_regs)
    sub = lambda o: (ECONST, 0) if o[0] in (AUX_CUR, AUX_NEXT) else o  # noqa: E731
    g.instrs = [(op, dst, sub(a), sub(b)) for op, dst, a, b in prog.instrs]
    return g


def evaluate(prog, field, ext, cur, nxt, aux_cur, aux_nxt, xs):
    """cprog_util.evaluate with the auxiliary frame: aux_cur / aux_nxt are (ce, aux row width) object arrays, or None for a
    program that reads none.  The evaluation columns: a list of (ce * ext,) object arrays."""
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
        if src in (AUX_CUR, AUX_NEXT):
            rows = aux_cur if src == AUX_CUR else aux_nxt
            cols = [rows[:, idx * ext + w] for w in range(ext)]
            return cols if ext > 1 else cols[0]
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
        r = U._apply(field, ext, op, fetch(*a), fetch(*b))
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


# ------------------------------------------------------------------------------------------------ the programs
def perm(field, ext, alphas, n=1):
    """The permutation argument, n times: main columns a = 2k, b = 2k + 1, a random alpha_k of E, the running product z = aux
    column k with z_0 = 1, z_(i+1) = z_i (a_i + alpha) / (b_i + alpha).  Per k one transition column
    AUX_NEXT k * (CUR b + alpha) - AUX_CUR k * (CUR a + alpha), then per k one boundary column AUX_CUR k - 1."""
    g = Prog(3 + 2 * n)
    one = g.const(U.to_mem(field, 1))
    for k in range(n):
        alpha = g.econst(alphas[k])
        g.add(0, (CUR, 2 * k + 1), alpha)
        g.mul(0, (AUX_NEXT, k), (REG, 0))
        g.add(1, (CUR, 2 * k), alpha)
        g.mul(1, (AUX_CUR, k), (REG, 1))
        g.sub(3 + k, (REG, 0), (REG, 1))
    for k in range(n):
        g.sub(3 + n + k, (AUX_CUR, k), one)
    g.out_regs = list(range(3, 3 + 2 * n))
    return g


def full(field, ext, rng, ce_blowup, n_cols, n_aux):
    """The shape of evaluate_fragment_full (evaluator.rs:190-241): two main transition constraints in the base field (one with a
    periodic table), each merged with an E coefficient by mul_base; two auxiliary transition constraints in E (a running sum
    over a main column with a random element, and a product of two auxiliary elements), merged with further coefficients into
    the same column; a boundary column over X for an auxiliary column.  Column indices fold onto the columns there are."""
    m, x = (lambda c: c % n_cols), (lambda c: c % n_aux)
    g = Prog(8)
    tab = g.table(U.draw(rng, field, 2 * ce_blowup))
    coef = [g.econst(U.draw_e(rng, field, ext)) for _ in range(4)]
    gamma = g.econst(U.draw_e(rng, field, ext))
    # main: next0 - (cur0 * cur1 + k), next1 - (cur1 + next0)^2
    g.mul(0, (CUR, m(0)), (CUR, m(1)))
    g.add(0, (REG, 0), tab)
    g.sub(0, (NEXT, m(0)), (REG, 0))
    g.add(1, (CUR, m(1)), (NEXT, m(0)))
    g.mul(1, (REG, 1), (REG, 1))
    g.sub(1, (NEXT, m(1)), (REG, 1))
    g.mul(2, coef[0], (REG, 0))          # mul_base
    g.mul(3, (REG, 1), coef[1])
    g.add(2, (REG, 2), (REG, 3))
    # aux: next_aux0 - (aux0 + gamma * cur_last), next_aux1 - aux1 * aux0
    g.mul(4, gamma, (CUR, m(n_cols - 1)))
    g.add(4, (AUX_CUR, x(0)), (REG, 4))
    g.sub(4, (AUX_NEXT, x(0)), (REG, 4))
    g.mul(5, (AUX_CUR, x(1)), (AUX_CUR, x(0)))
    g.sub(5, (AUX_NEXT, x(1)), (REG, 5))
    g.mul(4, (REG, 4), coef[2])
    g.mul(5, coef[3], (REG, 5))
    g.add(2, (REG, 2), (REG, 4))
    g.add(2, (REG, 2), (REG, 5))
    # boundary: (aux_last - (c1 * x + c0)) * coefficient
    g.mul(6, g.const(U.draw(rng, field, 1)[0]), (X, 0))
    g.add(6, (REG, 6), g.const(U.draw(rng, field, 1)[0]))
    g.sub(7, (AUX_CUR, x(n_aux - 1)), (REG, 6))
    g.mul(7, (REG, 7), g.econst(U.draw_e(rng, field, ext)))
    g.out_regs = [2, 7]
    return g


def aux_only(field, ext, rng, n_aux):
    """No main column: per auxiliary column next - cur^2 * alpha, summed; the first difference is a second column."""
    g = Prog(3)
    alpha = g.econst(U.draw_e(rng, field, ext))
    for c in range(n_aux):
        g.mul(0, (AUX_CUR, c), (AUX_CUR, c))
        g.mul(0, alpha, (REG, 0))
        g.sub(0, (AUX_NEXT, c), (REG, 0))
        if c == 0:
            g.add(1, (REG, 0), (AUX_CUR, 0))
            g.add(2, (REG, 0), g.econst([0] * ext))
        else:
            g.add(2, (REG, 2), (REG, 0))
    g.out_regs = [2, 1]
    return g


BASE_KINDS = (REG, CUR, NEXT, CONST, TABLE, X)
E_KINDS = (REG, ECONST, AUX_CUR, AUX_NEXT)


def aux_stress(field, ext, rng, ce, n_cols, n_aux, n_instrs=300):
    """cprog_util.stress with the auxiliary sources: n_instrs instructions on the full register footprint, every source kind on
    both operand sides (by construction: one instruction per kind and side first, see stress_coverage), every auxiliary column
    as AUX_CUR and as AUX_NEXT, tables of 2 and ce values, constants, coefficients and table values from the limb alphabet, and
    the products of two alphabet values (CONST x CONST, TABLE x CONST, ECONST x ECONST) added into evaluation columns."""
    fp = U.MAX_FOOTPRINT[field]
    n_e = 0 if ext == 1 else fp // (2 * ext)
    n_b = fp - n_e * ext
    g = Prog(n_b + n_e)
    for v in U.draw(rng, field, 12):
        g.const(v)
    for _ in range(4):
        g.econst(U.draw_e(rng, field, ext))
    g.table(U.draw(rng, field, 2))
    g.table(U.draw(rng, field, ce), shift=int(rng.integers(1, ce)))
    is_e = [r >= n_b for r in range(g.n_regs)]
    written = [False] * g.n_regs
    pick = lambda n: int(rng.integers(0, n))  # noqa: E731

    def of_kind(k, e_type):
        if k == REG:
            regs = [r for r in range(g.n_regs) if written[r] and is_e[r] == e_type]
            return (REG, regs[pick(len(regs))])
        n = {CUR: n_cols, NEXT: n_cols, CONST: len(g.consts), ECONST: len(g.econsts), TABLE: 2, X: 1, AUX_CUR: n_aux, AUX_NEXT: n_aux}[k]
        return (k, pick(n))

    # with ext == 1 there is one type: the E kinds are base sources like the others
    base_kinds = BASE_KINDS if ext > 1 else BASE_KINDS + E_KINDS[1:]

    def base_src():
        k = base_kinds[pick(len(base_kinds))]
        if k == REG and not any(written[r] for r in range(n_b)):
            k = CUR
        return of_kind(k, False)

    def e_src():
        k = E_KINDS[pick(len(E_KINDS))]
        if k == REG and not any(written[r] for r in range(n_b, g.n_regs)):
            k = ECONST
        return of_kind(k, True)

    def emit(dst, a=None, b=None):
        if not is_e[dst]:
            a, b = a or base_src(), b or base_src()
        elif a is None and b is None:
            a, b = [(e_src(), base_src()), (base_src(), e_src()), (e_src(), e_src())][pick(3)]
        g.op(int(rng.integers(1, 4)), dst, a, b)
        written[dst] = True

    for r in rng.permutation(g.n_regs):  # every register written once: the whole footprint is in use
        emit(int(r))
    for k in base_kinds:                 # every kind on either side of a base op ..
        emit(pick(n_b), a=of_kind(k, False), b=base_src())
        emit(pick(n_b), a=base_src(), b=of_kind(k, False))
    if n_e:                              # .. and of an E op, the other side base or E
        for k in E_KINDS:
            emit(n_b + pick(n_e), a=of_kind(k, True), b=base_src())
            emit(n_b + pick(n_e), a=e_src(), b=of_kind(k, True))
        for k in BASE_KINDS:
            emit(n_b + pick(n_e), a=of_kind(k, False), b=e_src())
            emit(n_b + pick(n_e), a=e_src(), b=of_kind(k, False))
    acc = n_b if n_e else 5              # every auxiliary column, both rows, into one accumulator
    for c in range(n_aux):
        g.mul(acc, (REG, acc), (AUX_CUR, c))
        g.add(acc, (AUX_NEXT, c), (REG, acc))
    while len(g.instrs) < n_instrs - 8:
        emit(pick(g.n_regs))
    for out, a, b in ((0, (CONST, 4), (CONST, 5)), (1, (TABLE, 0), (CONST, 6)), (0, (TABLE, 1), (CONST, 7))):
        g.mul(4, a, b)                   # alphabet x alphabet
        g.add(out, (REG, out), (REG, 4))
    last = g.n_regs - 1
    g.mul(last, (ECONST, 0), (ECONST, 1))
    g.add(acc, (REG, acc), (REG, last))
    g.out_regs = [0, 1, n_b - 1] + ([n_b, n_b + 1, last] if n_e else [2, 3, acc])
    assert len(g.instrs) == n_instrs
    return g


def stress_coverage(prog):
    """(kinds on side a, kinds on side b, AUX_CUR columns, AUX_NEXT columns) of a program"""
    ka = {a[0] for _, _, a, _ in prog.instrs}
    kb = {b[0] for _, _, _, b in prog.instrs}
    ops = [o for _, _, a, b in prog.instrs for o in (a, b)]
    return ka, kb, {i for s, i in ops if s == AUX_CUR}, {i for s, i in ops if s == AUX_NEXT}


AUX_PROGRAMS = ("perm", "full", "aux_only", "aux_stress")


def build(name, field, ext, rng, ce, ce_blowup, n_cols, n_aux):
    """One of the four auxiliary programs for n_cols main and n_aux auxiliary columns (indices fold where there are fewer)."""
    if name == "perm":
        g = perm(field, ext, [U.draw_e(rng, field, ext)])
        if n_cols < 2:
            g.instrs = [(op, d, (a[0], a[1] % n_cols if a[0] in (CUR, NEXT) else a[1]), (b[0], b[1] % n_cols if b[0] in (CUR, NEXT) else b[1]))
                        for op, d, a, b in g.instrs]
        return g
    if name == "full":
        return full(field, ext, rng, ce_blowup, n_cols, n_aux)
    if name == "aux_only":
        return aux_only(field, ext, rng, n_aux)
    return aux_stress(field, ext, rng, ce, n_cols, n_aux)


def wide_aux_slots(field, ext, n_main, n_aux, use_x=False):
    return 2 * n_main + 2 * n_aux * ext + int(use_x) + U.MAX_FOOTPRINT[field] // ext * ext


def wide_aux_frame(field, ext, n_main, n_aux, use_x=False):
    """Main columns 0 .. n_main - 1 and auxiliary columns 0 .. n_aux - 1 read in BOTH rows, x if asked for, and as many registers
    of type E as the footprint holds: wide_aux_slots LDS slots.  One evaluation column: the sum of all registers."""
    fp = U.MAX_FOOTPRINT[field]
    n_regs = fp // ext
    g = Prog(n_regs)
    zero = g.econst([0] * ext)
    for r in range(n_regs):
        g.add(r, (X, 0) if (use_x and r == 0) else (CUR, r % n_main), zero)
    for c in range(n_main):
        g.mul(c % n_regs, (REG, c % n_regs), (CUR, c))
        g.add(c % n_regs, (REG, c % n_regs), (NEXT, c))
    for c in range(n_aux):
        g.mul(c % n_regs, (REG, c % n_regs), (AUX_CUR, c))
        g.add(c % n_regs, (REG, c % n_regs), (AUX_NEXT, c))
    for r in range(1, n_regs):
        g.add(0, (REG, 0), (REG, r))
    g.out_regs = [0]
    return g
