"""GPU: the proof-side entry points on carry-edge and degenerate operands, against the oracle, bit for bit.

tests/test_gpu_field_edges.py feeds the column patterns of tests/edge_util.py to the transforms, the trace commitment, the
stand-alone folding and the stand-alone out-of-domain evaluation.  Everything a proof runs after the trace commitment --
the DEEP composition (csrc/deep.hpp), the constraint side from evaluation tables (csrc/constraint_poly.hpp), the
out-of-domain frame of resident polynomials and the resident FRI prover -- is a further inlining context of the same 32-bit
carry and borrow chains, and was only ever fed uniform elements.  Here those entry points get the patterns as *coefficients*
(resident polynomials are committed from the oracle's evaluations of the chosen vectors, edge_util.commit_resident_with_polys),
edge points for z, alpha and final_coeff, and the branches of their own that uniform data never reaches: a divisor's
numerator vanishing inside the domain, the switch between host and device inverses, eight exemption points, z with every scan
multiplier equal to one, z with base part 0, alpha = 0, the zero polynomial.

What the wrong-mask reduction (docs/STATUS.md, "Carry-edge operands") needs in order to show: a product of *two* alphabet
values.  It agrees with the real one whenever one factor is uniform, whatever the other is (0 of 86 000 alphabet x uniform
products differ, 92 of the 1849 alphabet pairs do).  So every function below has at least one multiplication whose two
operands both come from the alphabet: composition coefficient x column, divisor value x column (_alphabet_factor_columns),
transform twiddle x coefficient."""
import zlib

import numpy as np
import pytest

import edge_util as E

pytestmark = pytest.mark.gpu

F64, F128 = E.F64, E.F128
FIELD_EXT = [(F64, 1), (F64, 2), (F64, 3), (F128, 1), (F128, 2)]
OFFSETS = {F64: (7, E.P64 - 1), F128: (3, E.P128 - 1)}   # canonical domain offsets: a small one and -1


def _seed(*key):
    return zlib.crc32(repr(key).encode())   # (hash() of a string differs from process to process)


# Scalars are prepared on Python integers: canonical value <-> the stored form (f64: Montgomery residue, f128: the value).
def _mem(field, v):
    return v * E.R64 % E.P64 if field == F64 else v


def _canon(field, m):
    return m * E.R64_INV % E.P64 if field == F64 else m


def _root(orc, field, logn):
    """The generator of the domain of 2^logn points (the reference's get_root_of_unity), canonical."""
    p = E.MODULUS[field]
    g = _canon(F64, int(orc.lib().orc_f64_get_root_of_unity(logn))) if field == F64 else orc.f128_root_of_unity(logn)
    assert pow(g, 1 << logn, p) == 1 and pow(g, 1 << (logn - 1), p) == p - 1
    return g


def _scalar(field, v):
    """One base-field element from its canonical value."""
    return E.elements(field, [_mem(field, v)])


def _embed(field, ext, v):
    return E.elements(field, [_mem(field, v)] + [0] * (ext - 1))


def _times_base(field, point, v):
    """An element of E times the base-field element v (canonical): every coordinate times v."""
    p = E.MODULUS[field]
    coords = np.asarray(point).reshape(-1).tolist() if field == F64 else E.f128_ints(point)
    return E.elements(field, [_mem(field, _canon(field, c) * v % p) for c in coords])


def _flat(field, xs):
    w = 1 if field == F64 else 2
    return np.concatenate([np.asarray(x, dtype=np.uint64).reshape(-1, w) for x in xs]).reshape((-1, w) if w > 1 else -1)


def _edge_coefficients(rng, field, ext, count, first=0):
    """`count` elements of E cycling through 0, one, p - 1 (in every coordinate) and an alphabet draw per coordinate."""
    p = E.MODULUS[field]
    fixed = [[0] * ext, [E.ONE[field]] + [0] * (ext - 1), [p - 1] * ext]
    return [E.elements(field, fixed[(first + i) % 4]) if (first + i) % 4 < 3 else E.alphabet_draw(rng, field, ext)
            for i in range(count)]


# ------------------------------------------------------------------------------------------------ DEEP composition
DEEP_SHAPES = [
    # logn, n_main, n_aux, n_traces, n_cons
    (3, 2, 1, 1, 1),     # the smallest trace
    (10, 3, 2, 1, 2),    # exactly one DEEP_BLOCK
    (11, 3, 1, 2, 2),    # two blocks: a carry crosses
    (5, 8, 2, 3, 2),     # 32 columns (26 without the auxiliary ones): n_chunks = 4, k_deep_reduce runs
]


def _deep_rounds(rng, field, ext, logn, n_main, n_aux, n_traces, n_cons):
    """Coefficient vectors (main, aux, cons), round by round: the patterns in turn, neighbouring columns different, until every
    pattern has been in the main segment; at logn = 11 one more round whose columns have their single entry at the last index of
    block 0, the first of block 1 and the degree bound."""
    n = 1 << logn
    total = n_main * n_traces
    for first in range(0, len(E.PATTERNS), total):
        yield (E.pattern_columns(rng, field, total, n, 1, first),
               E.pattern_columns(rng, field, n_aux * n_traces, n, ext, first + 3),
               E.pattern_columns(rng, field, n_cons, n, ext, first + 5))
    if logn == 11:
        at = (1023, 1024, n - 1)
        yield ([E.single_at(field, n, 1, at[c % 3]) for c in range(3)] + E.pattern_columns(rng, field, total - 3, n, 1),
               [E.single_at(field, n, ext, 1024)] + E.pattern_columns(rng, field, n_aux * n_traces - 1, n, ext) if n_aux else [],
               [E.single_at(field, n, ext, n - 1), E.single_at(field, n, ext, 1023)] + E.pattern_columns(rng, field, n_cons - 2, n, ext))


@pytest.mark.parametrize("field,ext", FIELD_EXT)
@pytest.mark.parametrize("logn,n_main,n_aux,n_traces,n_cons", DEEP_SHAPES)
def test_deep_compose_on_edge_operands(ctx, orc, capi, field, ext, logn, n_main, n_aux, n_traces, n_cons):
    if ext == 1:
        n_aux = 0   # as in test_gpu_deep.py: the auxiliary segment would be another base-field segment
    rng = np.random.default_rng(_seed("deep", field, ext, logn))
    n, p = 1 << logn, E.MODULUS[field]
    g = _root(orc, field, logn)
    # z: every non-zero edge point (base part 0 with another coordinate set among them; z = 1 makes every scan multiplier of
    # the first stream one), g^-1 (the second stream's y = z g is one) and an alphabet draw per coordinate
    zs = E.edge_points_nonzero(field, ext) + [_embed(field, ext, pow(g, -1, p)), E.alphabet_draw(rng, field, ext)]
    for rnd, (main, aux, cons) in enumerate(_deep_rounds(rng, field, ext, logn, n_main, n_aux, n_traces, n_cons)):
        c_main = E.commit_resident_with_polys(ctx, orc, capi.make_params(field, 1, logn, 1, n_main, n_traces), main, 1)
        handles = [c_main]
        if n_aux:
            handles.append(E.commit_resident_with_polys(ctx, orc, capi.make_params(field, ext, logn, 1, n_aux, n_traces), aux, ext))
        c_cons = ctx.constraint_commit_resident(capi.make_params(field, ext, logn, 1, n_cons, 1), cons)
        # the reference's TracePolyTable t: main columns of trace t, then its auxiliary columns (composer/mod.rs:84-128)
        tables = [[(main[t * n_main + c], 1) for c in range(n_main)] + [(aux[t * n_aux + c], ext) for c in range(n_aux)]
                  for t in range(n_traces)]
        width = n_main + n_aux
        for coeff_kind in ("edge", "zero"):
            if coeff_kind == "edge":
                cc = _edge_coefficients(rng, field, ext, width * n_traces + n_cons, first=rnd)
            else:
                cc = [E.elements(field, [0] * ext)] * (width * n_traces + n_cons)
            cc_tables = [cc[t * width:(t + 1) * width] for t in range(n_traces)]
            cc_cons = cc[width * n_traces:]
            # the C ABI takes the coefficients handle by handle (main segments of all traces, then the auxiliary ones)
            abi = [cc_tables[t][c] for t in range(n_traces) for c in range(n_main)]
            abi += [cc_tables[t][n_main + c] for t in range(n_traces) for c in range(n_aux)]
            for z in (zs if coeff_kind == "edge" else zs[:1]):
                want = orc.deep_compose(field, ext, n, tables, cons, z, [c for tab in cc_tables for c in tab], cc_cons)
                got = ctx.deep_compose(field, ext, n, handles, c_cons, z, _flat(field, abi), _flat(field, cc_cons))
                assert np.array_equal(got, want), f"round {rnd}, {coeff_kind} coefficients, z {z.tolist()}"
                assert not got.reshape(n, -1)[-1].any()   # degree n - 2 at most (composer/mod.rs:151)
                if coeff_kind == "zero":
                    assert not got.any()
        for h in handles:
            h.close()
        c_cons.close()


# ------------------------------------------------------------------------------------------------ constraint evaluation tables
def _transition_divisor(field, n, b, exemptions):
    """(x^n - b) / prod (x - e_k): ConstraintDivisor::from_transition (air/src/air/divisor.rs:52-66) has b = 1 and exemptions
    on the trace domain; the formula takes any elements below p."""
    return (n, E.elements(field, [b]), E.elements(field, exemptions) if exemptions else None)


def _exemptions8(rng, field):
    """MAX_EXEMPTIONS exemption points (stored form): the edge scalars, then alphabet draws."""
    pts = E.edge_scalars(field) + E.alphabet_draw(rng, field, 8).reshape(-1).tolist() if field == F64 else \
        E.edge_scalars(field) + E.f128_ints(E.alphabet_draw(rng, field, 8))
    return pts[:8]


def _alphabet_factor_columns(rng, field, ext, ce, offset, count=3):
    """`count` (column, divisor) pairs: an alphabet column under a divisor x^ce - b whose one inverse 1 / (offset^ce - b) is a
    value t of the limb alphabet, so that k_acc_column multiplies the whole column by t -- alphabet value by alphabet value
    (nz = 1: the host's inverse).  Several, with t drawn anew: 10 of the 43 f64 alphabet values are factors under which the
    wrong-mask reduction agrees with the real one on the whole alphabet."""
    p = E.MODULUS[field]
    out = []
    while len(out) < count:
        t = E.alphabet_draw(rng, field, 1)
        t = _canon(field, int(t[0]) if field == F64 else E.f128_ints(t)[0])
        if t:
            b = (pow(offset, ce, p) - pow(t, -1, p)) % p
            out.append((E.alphabet_draw(rng, field, ce * ext), (ce, _scalar(field, b), None)))
    return out


def _vanishing_at(orc, field, log_ce, offset, i, a):
    """b = (offset g^i)^a, g the generator of the constraint evaluation domain: x^a - b vanishes at the domain's point i (and,
    for a > 1, at every point i + k nz, nz = ce / a)."""
    p = E.MODULUS[field]
    return _scalar(field, pow(offset * pow(_root(orc, field, log_ce), i, p), a, p))


def _commit_tables(ctx, orc, capi, field, ext, logR, logB, n_cols, tables, fc):
    """wf_constraint_commit_from_tables against combine_evaluation_table -> composition_poly_from_evaluations ->
    build_constraint_commitment; polynomials and root.  -> the oracle's combined tables."""
    off = OFFSETS[field][0]
    combined = [orc.combine_evaluation_table(field, ext, [c for c, _ in t], [d for _, d in t], off) for t in tables]
    want_cols = orc.composition_poly_from_evaluations(field, ext, combined, logR, n_cols, off, fc)
    want = orc.build_constraint_commitment(field, want_cols, ext, logR, logB, off)
    com, polys = ctx.constraint_commit_from_tables(capi.make_params(field, ext, logR, logB, n_cols, 1), tables,
                                                   fc if len(tables) > 1 else None, want_polys=True)
    for c in range(n_cols):
        assert np.array_equal(polys[c], want_cols[c]), f"column {c}"
    assert com.root() == want["root"]
    com.close()
    return combined


@pytest.mark.parametrize("field,ext", FIELD_EXT)
@pytest.mark.parametrize("logR,log_ce_blowup,logB", [(5, 2, 2), (10, 1, 1)])   # every inverse on the host; a = 1 on the device
def test_constraint_tables_with_edge_divisors(ctx, orc, capi, field, ext, logR, log_ce_blowup, logB):
    """One table per non-zero edge scalar b: transition divisors x^n - b without and with eight exemption points, x - b,
    x^(n/4) - b over pattern columns, and the alphabet-factor columns."""
    rng = np.random.default_rng(_seed("divisors", field, ext, logR))
    n, ce = 1 << logR, 1 << (logR + log_ce_blowup)
    tables = []
    for k, b in enumerate(v for v in E.edge_scalars(field) if v):
        divs = [_transition_divisor(field, n, b, None), _transition_divisor(field, n, b, _exemptions8(rng, field)),
                (1, E.elements(field, [b]), None), (n // 4, E.elements(field, [b]), None)]
        cols = E.pattern_columns(rng, field, len(divs), ce, ext, first=k)
        tables.append(list(zip(cols, divs)) + _alphabet_factor_columns(rng, field, ext, ce, OFFSETS[field][0]))
    assert len(tables) >= 2
    _commit_tables(ctx, orc, capi, field, ext, logR, logB, 1 << log_ce_blowup, tables, E.alphabet_draw(rng, field, ext))


@pytest.mark.parametrize("field,ext", FIELD_EXT)
@pytest.mark.parametrize("logR,log_ce_blowup,logB", [(6, 3, 1), (9, 2, 1)])   # all on the host; a = 1: 2048 inverses on the device
def test_constraint_tables_with_vanishing_numerator(ctx, orc, capi, field, ext, logR, log_ce_blowup, logB):
    """The numerator of every divisor of a table vanishes at point i of the constraint evaluation domain, i in {0, 5, ce - 1}
    (ce - 1 = nz - 1 mod nz for every nz): the inverse there is taken as 0 (math::batch_inversion), by f_inv for a = n
    (nz = ce / n) and a = n / 4 (the zero repeats with period nz through the column) and by dev_inv or f_inv for a = 1."""
    rng = np.random.default_rng(_seed("vanishing", field, ext, logR))
    n, log_ce = 1 << logR, logR + log_ce_blowup
    ce, off = 1 << log_ce, OFFSETS[field][0]
    assert (ce > 1024) == (logR == 9)   # which side of the switch a = 1 is on
    tables = []
    for i in (0, 5, ce - 1):
        divs = [(n, _vanishing_at(orc, field, log_ce, off, i, n), E.elements(field, _exemptions8(rng, field))),
                (1, _vanishing_at(orc, field, log_ce, off, i, 1), None),
                (n // 4, _vanishing_at(orc, field, log_ce, off, i, n // 4), None)]
        cols = [E.pattern_column(rng, field, "pm1", ce, ext), E.alphabet_draw(rng, field, ce * ext),
                E.pattern_column(rng, field, "const", ce, ext)]
        rows = orc.combine_evaluation_table(field, ext, cols, divs, off).reshape(ce, -1)
        assert not rows[i].any() and rows[(i + 1) % ce].any()              # every divisor leaves a zero at i ..
        per = orc.combine_evaluation_table(field, ext, cols[2:], divs[2:], off).reshape(ce, -1)
        nz = 4 * ce // n
        assert not per[i % nz::nz].any() and per[(i + 1) % nz::nz].any()   # .. and x^(n/4) - b at every i + k nz
        tables.append(list(zip(cols, divs)) + _alphabet_factor_columns(rng, field, ext, ce, off))
    _commit_tables(ctx, orc, capi, field, ext, logR, logB, 2, tables, E.alphabet_draw(rng, field, ext))


@pytest.mark.parametrize("field,ext", FIELD_EXT)
@pytest.mark.parametrize("logR,log_ce_blowup", [(8, 2), (9, 2)])   # ce = 1024: the last host size; ce = 2048: the first device size
def test_constraint_tables_at_the_inverse_route_switch(ctx, orc, capi, field, ext, logR, log_ce_blowup):
    """a = 1 has nz = ce inverses: combine_table_dev takes them from the host up to 1024 and from k_divisor_inverses above."""
    rng = np.random.default_rng(_seed("switch", field, ext, logR))
    n, log_ce = 1 << logR, logR + log_ce_blowup
    ce, off, p = 1 << log_ce, OFFSETS[field][0], E.MODULUS[field]
    g = _root(orc, field, logR)
    divs = [(1, _scalar(field, pow(g, int(rng.integers(0, n)), p)), None),    # an assertion at one step (divisor.rs:68-96)
            (1, _vanishing_at(orc, field, log_ce, off, ce - 1, 1), None)]      # and one whose last inverse is the 0 -> 0 one
    cols = [E.alphabet_draw(rng, field, ce * ext) for _ in divs]
    _commit_tables(ctx, orc, capi, field, ext, logR, 1, 2, [list(zip(cols, divs)) + _alphabet_factor_columns(rng, field, ext, ce, off)], None)


@pytest.mark.parametrize("field,ext", FIELD_EXT)
def test_constraint_tables_with_edge_final_coeff(ctx, orc, capi, field, ext):
    """Three tables combined with the powers of final_coeff, final_coeff over the edge points: with zero only table 0 survives,
    with one and -1 the tables are added and subtracted."""
    rng = np.random.default_rng(_seed("final_coeff", field, ext))
    logR, log_ce_blowup, logB = 5, 2, 3
    n, ce, off, p = 1 << logR, 1 << (logR + log_ce_blowup), OFFSETS[field][0], E.MODULUS[field]
    g = _root(orc, field, logR)
    tables = []
    for t in range(3):
        # the three kinds of tests/test_gpu_constraint_poly.py::_divisors, and the alphabet-factor columns
        ex = E.elements(field, [_mem(field, pow(g, n - 1 - i, p)) for i in range(2)])
        divs = [(n, E.elements(field, [E.ONE[field]]), ex), (1, _scalar(field, pow(g, int(rng.integers(0, n)), p)), None),
                (n // 4, _scalar(field, pow(g, (3 * n) // 4 % n, p)), None)]
        cols = E.pattern_columns(rng, field, 3, ce, ext, first=3 * t)
        tables.append(list(zip(cols, divs)) + _alphabet_factor_columns(rng, field, ext, ce, off))
    for fc in E.edge_points(field, ext):
        combined = _commit_tables(ctx, orc, capi, field, ext, logR, logB, 3, tables, fc)
        if not fc.any():   # what "only table 0 survives" means, on the oracle
            alone = orc.composition_poly_from_evaluations(field, ext, combined[:1], logR, 3, off)
            both = orc.composition_poly_from_evaluations(field, ext, combined, logR, 3, off, fc)
            assert all(np.array_equal(a, b) for a, b in zip(alone, both))


# ------------------------------------------------------------------------------------------------ from evaluations, resident OOD
@pytest.mark.parametrize("field,ext", FIELD_EXT)
@pytest.mark.parametrize("logR,log_ce_blowup,n_cols,n_tables,logB", [(3, 1, 1, 1, 1), (10, 1, 2, 3, 2)])
def test_constraint_commit_from_evaluations_on_edge_operands(ctx, orc, capi, field, ext, logR, log_ce_blowup, n_cols, n_tables, logB):
    """Pattern tables, final_coeff over the edge points (rounds go on until every pattern has been a table), then the
    out-of-domain evaluation of the resident columns at every edge point."""
    rng = np.random.default_rng(_seed("from_evaluations", field, ext, logR))
    off = OFFSETS[field][0]
    ce = 1 << (logR + log_ce_blowup)
    points = E.edge_points(field, ext)
    params = capi.make_params(field, ext, logR, logB, n_cols, 1)
    for rnd in range(max(len(points), -(-len(E.PATTERNS) // n_tables))):
        tables = E.pattern_columns(rng, field, n_tables, ce, ext, first=rnd * n_tables)
        fc = points[rnd % len(points)]
        want_cols = orc.composition_poly_from_evaluations(field, ext, tables, logR, n_cols, off, fc)
        want = orc.build_constraint_commitment(field, want_cols, ext, logR, logB, off)
        com, polys = ctx.constraint_commit_from_evaluations(params, tables, fc if n_tables > 1 else None, want_polys=True)
        for c in range(n_cols):
            assert np.array_equal(polys[c], want_cols[c]), f"round {rnd}, column {c}"
        assert com.root() == want["root"], f"round {rnd}"
        for z in points:
            ood = com.evaluate_polys_at(z, ext, n_cols)
            for c in range(n_cols):
                assert np.array_equal(ood[c], orc.eval_column_at(field, want_cols[c], ext, z, ext)), f"round {rnd}, column {c}, z {z.tolist()}"
        com.close()


@pytest.mark.parametrize("field,ext_z", [(F64, 2), (F64, 3), (F128, 1), (F128, 2)])
@pytest.mark.parametrize("logR", [7, 13])   # below one 4096-coefficient block, two blocks
def test_ood_frame_of_resident_edge_polynomials(ctx, orc, capi, field, ext_z, logR):
    """get_ood_frame on base-field trace polynomials that are the eight patterns as coefficient vectors: (z, z g) for every
    edge point z, in one call and in single calls."""
    rng = np.random.default_rng(_seed("resident_ood", field, ext_z, logR))
    n_cols, n_traces = 4, 2
    total = n_cols * n_traces
    polys = E.pattern_columns(rng, field, total, 1 << logR, 1)
    com = E.commit_resident_with_polys(ctx, orc, capi.make_params(field, 1, logR, 1, n_cols, n_traces), polys, 1)
    g = _root(orc, field, logR)
    for z in E.edge_points(field, ext_z):
        zg = _times_base(field, z, g)   # z * E::from(g)
        frame = com.evaluate_polys_at_points(_flat(field, [z, zg]), 2, ext_z, total)
        for q, point in enumerate((z, zg)):
            for c in range(total):
                assert np.array_equal(frame[q][c], orc.eval_column_at(field, polys[c], 1, point, ext_z)), f"z {z.tolist()}, point {q}, column {c}"
            assert np.array_equal(com.evaluate_polys_at(point, ext_z, total), frame[q]), f"z {z.tolist()}, point {q}"
    com.close()


# ------------------------------------------------------------------------------------------------ resident FRI prover
@pytest.mark.parametrize("field,ext,folding,blowup,max_rem,log_trace", [
    (F64, 1, 2, 4, 7, 7), (F64, 2, 4, 8, 7, 8), (F64, 3, 16, 8, 7, 8), (F128, 1, 8, 8, 15, 8), (F128, 2, 4, 8, 7, 8)])
def test_resident_fri_prover_on_edge_operands(ctx, orc, capi, field, ext, folding, blowup, max_rem, log_trace):
    """A whole commit phase per low-degree polynomial -- zero, all p - 1, a single top coefficient, alphabet draws -- with
    alphas that cycle through the edge points instead of being derived from the roots; every root, rows 0, 1 and the last of
    every layer, the remainder and its digest.  The non-zero polynomials also enter as coefficients (begin_poly): that is where
    the device's transform meets the alphabet."""
    rng = np.random.default_rng(_seed("fri", field, ext, folding))
    trace_len = 1 << log_trace
    n = trace_len * blowup
    w = 1 if field == F64 else 2
    offset = OFFSETS[field][0]
    off_elem = _mem(field, offset)
    n_layers = capi.fri_num_layers(folding, blowup, max_rem, n)
    assert n_layers >= 2
    points = E.edge_points(field, ext)
    k = -n_layers % len(points)   # the zero polynomial takes the alphas before the cycle's start: alpha = 0 folds all p - 1
    zero_alpha_on = []
    tw = orc.get_twiddles(field, n)
    pr = capi.FriProver(ctx, field, ext, folding, blowup, max_rem, offset)
    for kind in ("zero", "pm1", "single_last", "alphabet"):
        low = E.pattern_column(rng, field, kind, trace_len, ext)
        for entry in ("begin", "begin_poly"):
            if entry == "begin":   # evaluations of a polynomial of degree < trace_len over the unshifted domain (fri/src/prover/tests.rs)
                ev = np.zeros((n * ext, 2) if w == 2 else n * ext, dtype=np.uint64)
                ev[:trace_len * ext] = low
                orc.evaluate_poly(field, ev, n, ext, tw)
                pr.begin(ev)
            elif kind == "zero":
                continue
            else:                  # its coset LDE, produced on the device
                ev = orc.evaluate_poly_with_offset(field, low, trace_len, ext, orc.get_twiddles(field, trace_len), off_elem, blowup)
                pr.begin_poly(low, blowup)
            size, cur = n, ev
            for i in range(n_layers):
                want = orc.fri_layer_commit(field, cur, size, ext, folding)
                assert pr.commit_layer() == want["root"], f"{kind}, {entry}, layer {i}"
                target = size // folding
                alpha = points[k % len(points)]
                k += 1
                if not alpha.any() and kind != "zero":
                    zero_alpha_on.append(kind)
                cur = orc.apply_drp(field, want["transposed"], target, ext, folding, offset, alpha)
                pr.fold(alpha)   # (the layer becomes readable once it has been folded)
                rows = pr.layer(i).read_rows(np.array([0, 1, target - 1], dtype=np.uint64))
                tr = want["transposed"].reshape((target, folding * ext) + ((2,) if w == 2 else ()))
                assert np.array_equal(rows, tr[[0, 1, target - 1]]), f"{kind}, {entry}, layer {i}"
                size = target
            assert pr.num_layers() == n_layers
            rem, digest = pr.set_remainder(size)
            want_rem = cur.copy()
            orc.interpolate_poly_with_offset(field, want_rem, size, ext, orc.get_twiddles(field, size, inverse=True), off_elem)
            keep = (size // blowup) * ext * w
            assert np.array_equal(rem.reshape(-1), want_rem.reshape(-1)[:keep]), f"{kind}, {entry}"
            assert digest == orc.hash_elements(field, want_rem.reshape(-1)[:keep]), f"{kind}, {entry}"
            if kind == "zero":
                assert not rem.any()
            pr.reset()
    pr.close()
    assert zero_alpha_on, "alpha = 0 never folded a non-zero polynomial"


@pytest.mark.parametrize("field,ext,folding,blowup,max_rem,log_trace", [(F64, 2, 4, 8, 7, 8), (F128, 1, 8, 8, 15, 8)])
def test_resident_fri_prover_begin_poly_on_the_offset_minus_one(ctx, orc, capi, field, ext, folding, blowup, max_rem, log_trace):
    """begin_poly with the domain offset p - 1: the first layer of the alphabet polynomial's coset LDE, folded once with -1."""
    rng = np.random.default_rng(_seed("fri_minus_one", field))
    trace_len = 1 << log_trace
    n = trace_len * blowup
    offset = OFFSETS[field][1]
    low = E.alphabet_draw(rng, field, trace_len * ext)
    lde = orc.evaluate_poly_with_offset(field, low, trace_len, ext, orc.get_twiddles(field, trace_len), _mem(field, offset), blowup)
    pr = capi.FriProver(ctx, field, ext, folding, blowup, max_rem, offset)
    pr.begin_poly(low, blowup)
    want = orc.fri_layer_commit(field, lde, n, ext, folding)
    assert pr.commit_layer() == want["root"]
    alpha = E.elements(field, [E.MODULUS[field] - 1] * ext)
    pr.fold(alpha)
    nxt = orc.apply_drp(field, want["transposed"], n // folding, ext, folding, offset, alpha)
    assert pr.commit_layer() == orc.fri_layer_commit(field, nxt, n // folding, ext, folding)["root"]
    pr.close()
