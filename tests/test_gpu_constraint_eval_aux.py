"""GPU: constraint programs over the main and the auxiliary segment (wf_constraint_evaluate_aux, csrc/constraint_eval.hip) --
every element of every evaluation column against tests/cprog_aux_util.py, the interpreter with both auxiliary sources restated
on Python integers, which runs on the LDE rows of BOTH commitments read back through wf_commitment_read_lde -- and the chain
into the constraint commitment with the columns left on the device.

The main commitment is trace_commit_resident with ext_degree 1, the auxiliary one the same parameters with ext_degree = the
program's.  Shapes: trace lengths 2^3, 2^5, 2^8 at LDE blowup 8 with ce blowup 2, 4, 8 (a ce of 16 is one partial wave), 1 / 8 / 10
main and 1 / 3 / 5 auxiliary columns (5 columns of degree 3 are 15 base elements: rows of 16 with a padding lane), three packed
traces on each side read at (main 0, aux 2) and (main 2, aux 0).  Auxiliary columns are the patterns of tests/edge_util.py,
alpha and the coefficients limb-alphabet draws.

One refusal of the header is not reached here: a commitment without resident rows exists only as the polynomial handle of a
sharded commitment; tests/test_cprog_aux_host.py produces it from the planner."""
import ctypes as C

import numpy as np
import pytest

import cprog_aux_util as A
import cprog_util as U
import edge_util as E

pytestmark = pytest.mark.gpu
F64, F128 = 1, 2
FIELDS = [(F64, 1), (F64, 2), (F64, 3), (F128, 1), (F128, 2)]
LOG_B = 3
#        log2 R, log2 ce blowup, main columns, aux columns, packed traces, main read, aux read
SHAPES = [(3, 1, 1, 1, 1, 0, 0), (5, 2, 8, 3, 3, 0, 2), (8, 3, 10, 5, 3, 2, 0)]
OFFSET = {F64: 7, F128: 3}
ERR_ARG, ERR_EXTENSION, ERR_BLOWUP = -19, -11, -13

_COMMITS = {}


def _commit(ctx, capi, field, ext, log_r, n_cols, n_traces, aux=False):
    """A resident commitment of pattern columns of extension degree `ext` (the main one, or with aux=True the auxiliary one: its
    own handle also where the parameters coincide) and, per trace, its LDE rows as integers: made once per shape, left unchanged."""
    key = (field, ext, log_r, n_cols, n_traces, aux)
    if key not in _COMMITS:
        rng = np.random.default_rng([int(k) for k in key])
        cols = [c for t in range(n_traces) for c in E.pattern_columns(rng, field, n_cols, 1 << log_r, ext=ext, first=t + 3 * aux)]
        com, _ = ctx.trace_commit_resident(capi.make_params(field, ext, log_r, LOG_B, n_cols, n_traces), cols)
        n = 1 << (log_r + LOG_B)
        ldes = [U.lde_ints(field, com.read_lde(t, 0, n)) for t in range(n_traces)]
        assert ldes[0].shape[1] >= n_cols * ext
        _COMMITS[key] = (com, ldes)
    return _COMMITS[key]


def _reference(g, field, ext, lde, aux_lde, log_ce_b):
    cur, nxt = U.frame_rows(lde, 1 << LOG_B, 1 << log_ce_b)
    acur, anxt = U.frame_rows(aux_lde, 1 << LOG_B, 1 << log_ce_b)
    return A.evaluate(g, field, ext, cur, nxt, acur, anxt, U.ce_points(field, cur.shape[0], OFFSET[field]))


def _compare(ev, want, field, what):
    assert ev.n_columns == len(want)
    for j, w in enumerate(want):
        got = U.column_ints(field, ev.read(j))
        assert len(got) == len(w) == ev.ce_domain_size * ev.ext_degree
        bad = [i for i, (a, b) in enumerate(zip(got, w)) if a != b]
        assert not bad, f"{what}: column {j}: {len(bad)} of {len(w)} elements differ, first at {bad[0]}"


@pytest.mark.parametrize("name", A.AUX_PROGRAMS)
@pytest.mark.parametrize("log_r,log_ce_b,n_cols,n_aux,n_traces,main_index,aux_index", SHAPES)
@pytest.mark.parametrize("field,ext", FIELDS)
def test_aux_programs_match_the_python_reference(ctx, capi, field, ext, log_r, log_ce_b, n_cols, n_aux, n_traces, main_index, aux_index, name):
    com, ldes = _commit(ctx, capi, field, 1, log_r, n_cols, n_traces)
    aux, aux_ldes = _commit(ctx, capi, field, ext, log_r, n_aux, n_traces, aux=True)
    ce = 1 << (log_r + log_ce_b)
    rng = np.random.default_rng([field, ext, log_r, A.AUX_PROGRAMS.index(name)])
    g = A.build(name, field, ext, rng, ce, 1 << log_ce_b, n_cols, n_aux)
    if name == "aux_stress":
        ka, kb, acur, anxt = A.stress_coverage(g)
        assert ka == kb == set(range(9)) and acur == anxt == set(range(n_aux)) and len(g.instrs) == 300
    if name == "aux_only":
        assert not A.typing(g, ext)[1] and not A.typing(g, ext)[2]
    ev = ctx.constraint_evaluate_aux(com, main_index, aux, aux_index, U.to_capi(capi, g, field, ext), ext, log_ce_b)
    assert (ev.n_columns, ev.ce_domain_size, ev.ext_degree) == (len(g.out_regs), ce, ext)
    _compare(ev, _reference(g, field, ext, ldes[main_index], aux_ldes[aux_index], log_ce_b), field, name)
    ev.close()


@pytest.mark.parametrize("name", U.PROGRAMS)
@pytest.mark.parametrize("log_r,log_ce_b,n_cols,n_aux,n_traces,main_index,aux_index", SHAPES)
@pytest.mark.parametrize("field,ext", FIELDS)
def test_main_only_programs_give_the_columns_of_the_main_call(ctx, capi, field, ext, log_r, log_ce_b, n_cols, n_aux, n_traces, main_index, aux_index, name):
    """The five programs of cprog_util, unchanged, through the new call: the columns of wf_constraint_evaluate on the same handle
    (which tests/test_gpu_constraint_eval.py compares with the Python interpreter), byte for byte."""
    com, _ = _commit(ctx, capi, field, 1, log_r, n_cols, n_traces)
    aux, _ = _commit(ctx, capi, field, ext, log_r, n_aux, n_traces, aux=True)
    ce = 1 << (log_r + log_ce_b)
    rng = np.random.default_rng([field, ext, log_r, U.PROGRAMS.index(name)])
    g = U.build(name, field, ext, rng, ce, 1 << log_ce_b, n_cols)
    cp = U.to_capi(capi, g, field, ext)
    ev = ctx.constraint_evaluate_aux(com, main_index, aux, aux_index, cp, ext, log_ce_b)
    old = ctx.constraint_evaluate(com, main_index, cp, ext, log_ce_b)
    assert (ev.n_columns, ev.ce_domain_size, ev.ext_degree) == (old.n_columns, old.ce_domain_size, old.ext_degree) == (len(g.out_regs), ce, ext)
    for j in range(ev.n_columns):
        assert np.array_equal(ev.read(j), old.read(j)), f"{name}: column {j}"
    ev.close()
    old.close()


@pytest.mark.parametrize("field,ext", [(F64, 2), (F128, 2)])
def test_handles_of_the_asynchronous_commitment_are_valid_input_before_wait(ctx, capi, field, ext):
    log_r, n_cols, n_aux, log_ce_b = 8, 8, 3, 2
    rng = np.random.default_rng(field)
    com = ctx.trace_commit_resident_async(capi.make_params(field, 1, log_r, LOG_B, n_cols, 1), E.pattern_columns(rng, field, n_cols, 1 << log_r))
    aux = ctx.trace_commit_resident_async(capi.make_params(field, ext, log_r, LOG_B, n_aux, 1),
                                          E.pattern_columns(rng, field, n_aux, 1 << log_r, ext=ext))
    g = A.build("full", field, ext, rng, 1 << (log_r + log_ce_b), 1 << log_ce_b, n_cols, n_aux)
    ev = ctx.constraint_evaluate_aux(com, 0, aux, 0, U.to_capi(capi, g, field, ext), ext, log_ce_b)   # queued behind both commitments
    com.wait()
    aux.wait()
    n = 1 << (log_r + LOG_B)
    lde, aux_lde = U.lde_ints(field, com.read_lde(0, 0, n)), U.lde_ints(field, aux.read_lde(0, 0, n))
    _compare(ev, _reference(g, field, ext, lde, aux_lde, log_ce_b), field, "full on asynchronous commitments")
    ev.close()
    com.close()
    aux.close()


def test_two_evaluations_back_to_back_keep_their_own_columns(ctx, capi):
    field, ext, log_r, n_cols, n_aux, log_ce_b = F64, 2, 8, 10, 5, 2
    com, ldes = _commit(ctx, capi, field, 1, log_r, n_cols, 3)
    aux, aux_ldes = _commit(ctx, capi, field, ext, log_r, n_aux, 3, aux=True)
    ce = 1 << (log_r + log_ce_b)
    rng = np.random.default_rng(77)
    g1 = A.build("full", field, ext, rng, ce, 1 << log_ce_b, n_cols, n_aux)
    g2 = A.build("aux_only", field, ext, rng, ce, 1 << log_ce_b, n_cols, n_aux)   # the same number of columns: the same buffer size
    ev1 = ctx.constraint_evaluate_aux(com, 1, aux, 1, U.to_capi(capi, g1, field, ext), ext, log_ce_b)
    ev2 = ctx.constraint_evaluate_aux(com, 1, aux, 1, U.to_capi(capi, g2, field, ext), ext, log_ce_b)
    _compare(ev2, _reference(g2, field, ext, ldes[1], aux_ldes[1], log_ce_b), field, "second")
    _compare(ev1, _reference(g1, field, ext, ldes[1], aux_ldes[1], log_ce_b), field, "first, read after the second ran")
    ev1.close()
    ev2.close()


def test_handles_destroyed_at_once_leave_the_queued_work_intact(ctx, capi):
    field, ext, log_r, n_cols, n_aux, log_ce_b = F64, 2, 8, 10, 5, 2
    com, ldes = _commit(ctx, capi, field, 1, log_r, n_cols, 3)
    aux, aux_ldes = _commit(ctx, capi, field, ext, log_r, n_aux, 3, aux=True)
    ce = 1 << (log_r + log_ce_b)
    rng = np.random.default_rng(5)
    progs = [A.build(name, field, ext, rng, ce, 1 << log_ce_b, n_cols, n_aux) for name in ("aux_stress", "full", "aux_stress")]
    for g in progs:
        ctx.constraint_evaluate_aux(com, 0, aux, 0, U.to_capi(capi, g, field, ext), ext, log_ce_b).close()
    g = progs[1]
    ev = ctx.constraint_evaluate_aux(com, 2, aux, 1, U.to_capi(capi, g, field, ext), ext, log_ce_b)
    ctx.constraint_evaluate_aux(com, 0, aux, 0, U.to_capi(capi, progs[0], field, ext), ext, log_ce_b).close()
    _compare(ev, _reference(g, field, ext, ldes[2], aux_ldes[1], log_ce_b), field, "kept handle")
    ev.close()


# ------------------------------------------------------------------------------------------------ the limits of local memory
def test_aux_frames_of_more_than_64_kib_of_exactly_160_kib_and_one_column_more(ctx, capi):
    """f64, degree 2, 8 main columns in both rows and 64 register elements: 30 auxiliary columns in both rows are 200 slots (100
    KiB for one wave: the launch has to ask for more than the default 64 KiB), 60 are 320 slots (all 160 KiB of a compute unit),
    61 are refused."""
    field, ext, log_r, log_ce_b, n_main = F64, 2, 5, 3, 8
    com, ldes = _commit(ctx, capi, field, 1, log_r, n_main, 1)
    aux, aux_ldes = _commit(ctx, capi, field, ext, log_r, 61, 1, aux=True)
    for n_aux, slots in ((30, 200), (60, 320)):
        assert A.wide_aux_slots(field, ext, n_main, n_aux) == slots
        g = A.wide_aux_frame(field, ext, n_main, n_aux)
        ev = ctx.constraint_evaluate_aux(com, 0, aux, 0, U.to_capi(capi, g, field, ext), ext, log_ce_b)
        _compare(ev, _reference(g, field, ext, ldes[0], aux_ldes[0], log_ce_b), field, f"{slots} slots")
        ev.close()
    with pytest.raises(capi.WfError) as e:
        ctx.constraint_evaluate_aux(com, 0, aux, 0, U.to_capi(capi, A.wide_aux_frame(field, ext, n_main, 61), field, ext), ext, log_ce_b)
    assert e.value.code == ERR_ARG and "do not fit" in str(e.value)


# ------------------------------------------------------------------------------------------------ the chain
def _trace_domain_point(field, log_r, e):
    v = pow(U.root_of_unity(field, log_r), e, U.P[field])
    return E.elements(field, [U.to_mem(field, v)])


def _divisors(field, log_r, kinds):
    """'t': the transition divisor (x^R - 1) / (x - g^(R-1)); 'first': the single assertion's (x - 1)"""
    R = 1 << log_r
    one = E.elements(field, [E.ONE[field]])
    return [(R, one, _trace_domain_point(field, log_r, R - 1)) if k == "t" else (1, _trace_domain_point(field, log_r, 0), None) for k in kinds]


@pytest.mark.parametrize("name,field,ext,n_traces", [("perm", F128, 2, 1), ("perm", F64, 2, 3), ("full", F64, 3, 1), ("full", F128, 1, 3)])
def test_commit_from_device_tables_is_the_host_table_call(ctx, capi, name, field, ext, n_traces):
    """perm and full into wf_constraint_commit_from_device_tables: root, rows and polynomials are those of
    wf_constraint_commit_from_tables fed the wf_evaluations_read copies."""
    log_r, log_ce_b, n_cols_c, n_cols, n_aux = 8, 2, 4, 8, 3
    com, ldes = _commit(ctx, capi, field, 1, log_r, n_cols, n_traces)
    aux, aux_ldes = _commit(ctx, capi, field, ext, log_r, n_aux, n_traces, aux=True)
    ce = 1 << (log_r + log_ce_b)
    rng = np.random.default_rng([field, ext, n_traces])
    divs = _divisors(field, log_r, ["t", "first"])
    evs, host_tables = [], []
    for t in range(n_traces):
        g = A.build(name, field, ext, rng, ce, 1 << log_ce_b, n_cols, n_aux)
        ev = ctx.constraint_evaluate_aux(com, t, aux, n_traces - 1 - t, U.to_capi(capi, g, field, ext), ext, log_ce_b)
        _compare(ev, _reference(g, field, ext, ldes[t], aux_ldes[n_traces - 1 - t], log_ce_b), field, f"trace {t}")
        evs.append(ev)
        host_tables.append(list(zip([ev.read(j) for j in range(ev.n_columns)], divs)))
    fc = E.elements(field, U.draw(rng, field, ext))
    p = capi.make_params(field, ext, log_r, LOG_B, n_cols_c, 1)
    dev, dev_polys = ctx.constraint_commit_from_device_tables(p, [(ev, divs) for ev in evs], fc if n_traces > 1 else None, want_polys=True)
    host, host_polys = ctx.constraint_commit_from_tables(p, host_tables, fc if n_traces > 1 else None, want_polys=True)
    assert dev.root() == host.root()
    for c in range(n_cols_c):
        assert np.array_equal(dev_polys[c], host_polys[c]), f"column {c}"
    pos = np.unique(rng.integers(0, 1 << (log_r + LOG_B), size=12))
    rows_d, proof_d = dev.query(pos)
    rows_h, proof_h = host.query(pos)
    assert np.array_equal(rows_d, rows_h) and proof_d == proof_h
    for ev, table in zip(evs, host_tables):   # the columns were read in place, not consumed
        assert np.array_equal(ev.read(0), table[0][0])
        ev.close()
    dev.close()
    host.close()


# ------------------------------------------------------------------------------------------------ meaning
def _e_mul(field, ext, a, b):
    return U.ext_mul(field, ext, list(a), list(b)) if ext > 1 else [a[0] * b[0] % U.P[field]]


def _e_inv(field, ext, a):
    """1 / a in E over f128 (memory form = canonical): degree 1, or the quadratic extension phi^2 = phi + 1, where the conjugate of
    a0 + a1 phi is (a0 + a1) - a1 phi and the norm a0^2 + a0 a1 - a1^2"""
    p = U.P[field]
    if ext == 1:
        return [pow(a[0], -1, p)]
    inv = pow((a[0] * a[0] + a[0] * a[1] - a[1] * a[1]) % p, -1, p)
    return [(a[0] + a[1]) * inv % p, -a[1] * inv % p]


@pytest.mark.parametrize("ext", [1, 2])
def test_perm_on_a_valid_trace_divides_to_a_low_degree_polynomial(ctx, capi, ext):
    """b is a shuffle of a and z the running product z_0 = 1, z_(i+1) = z_i (a_i + alpha) / (b_i + alpha), built on Python
    integers: the transition column divided by (x^R - 1) / (x - g^(R-1)) interpolates to a polynomial of degree < ce - R -- the top R
    coefficients are zero --, and with one element of b changed under the same z they are not."""
    field, log_r, log_ce_b = F128, 8, 2
    p, R, ce = U.P[field], 1 << log_r, 1 << (log_r + log_ce_b)
    rng = np.random.default_rng(ext)
    a = [int(v) for v in rng.integers(1, 2**62, size=R)]
    b = [a[i] for i in rng.permutation(R)]
    alpha = list(U.draw_e(rng, field, ext))
    emb = lambda v: [(v + alpha[0]) % p] + alpha[1:]  # noqa: E731
    z, cur = [], [1] + [0] * (ext - 1)
    for i in range(R):
        z.append(cur)
        cur = _e_mul(field, ext, _e_mul(field, ext, cur, emb(a[i])), _e_inv(field, ext, emb(b[i])))
    assert cur == [1] + [0] * (ext - 1)   # the grand product: b is a permutation of a
    g = A.perm(field, ext, [alpha])
    aux, _ = ctx.trace_commit_resident(capi.make_params(field, ext, log_r, LOG_B, 1, 1), [E.elements(field, [c for e in z for c in e])])
    gR = pow(U.root_of_unity(field, log_r), R - 1, p)
    xs = U.ce_points(field, ce, OFFSET[field])
    inv_z = [(x - gR) * pow(pow(x, R, p) - 1, -1, p) % p for x in xs]
    tops = []
    for b_col in (b, b[:100] + [b[100] + 1] + b[101:]):
        com, _ = ctx.trace_commit_resident(capi.make_params(field, 1, log_r, LOG_B, 2, 1), [E.elements(field, a), E.elements(field, b_col)])
        ev = ctx.constraint_evaluate_aux(com, 0, aux, 0, U.to_capi(capi, g, field, ext), ext, log_ce_b)
        col = U.column_ints(field, ev.read(0))
        q = [col[i] * inv_z[i // ext] % p for i in range(ce * ext)]
        poly = ctx.fft_interpolate_poly_with_offset(field, ext, E.elements(field, q), OFFSET[field])
        tops.append(U.column_ints(field, poly)[(ce - R) * ext:])
        ev.close()
        com.close()
    aux.close()
    assert not any(tops[0]), "the valid trace does not satisfy the program: it is not the AIR"
    assert any(tops[1])


# ------------------------------------------------------------------------------------------------ refusals
def _small(ext=2, n_aux=5):
    g = U.Prog(3)
    g.add(0, (U.CUR, 0), g.const(5))
    g.mul(0, (U.REG, 0), g.table([1, 2, 3, 4], shift=1))
    g.mul(1, (A.AUX_CUR, 0), g.econst([3] * ext))
    g.add(1, (U.REG, 1), (A.AUX_NEXT, n_aux - 1))
    g.mul(1, (U.REG, 1), (U.REG, 0))
    g.out_regs = [1]
    return g


def _with(i, **kw):
    g = _small()
    op, dst, a, b = g.instrs[i]
    g.instrs[i] = (kw.get("op", op), kw.get("dst", dst), kw.get("a", a), kw.get("b", b))
    return g


def _reserved0(cp, keep):
    cp.instrs[1].reserved0 = 1


# (what, code, a word of the message, program, patch of the C structure, other arguments)
#   aux: parameters of the auxiliary commitment that differ from (F64, ext 2, 2^5 rows, blowup 8, 5 columns, 3 traces, offset 7)
REFUSALS = [
    ("main_trace is null", ERR_ARG, "null", None, None, dict(null_main=True)),
    ("aux_trace is null", ERR_ARG, "null", None, None, dict(null_aux=True)),
    ("prog is null", ERR_ARG, "null", None, None, dict(null_prog=True)),
    ("out is null", ERR_ARG, "null", None, None, dict(null_out=True)),
    ("aux_trace of another context", ERR_ARG, "context", None, None, dict(other_ctx=True)),
    ("aux field differs", ERR_ARG, "shape", None, None, dict(aux=dict(field=F128))),
    ("aux log2_trace_len differs", ERR_ARG, "shape", None, None, dict(aux=dict(log_r=6))),
    ("aux log2_blowup differs", ERR_ARG, "shape", None, None, dict(aux=dict(log_b=2))),
    ("aux domain_offset differs", ERR_ARG, "domain_offset", None, None, dict(aux=dict(offset=49))),
    ("aux ext_degree 3, program in degree 2", ERR_ARG, "extension degree", None, None, dict(aux=dict(ext=3))),
    ("aux ext_degree 1, program in degree 2", ERR_ARG, "extension degree", None, None, dict(aux=dict(ext=1))),
    ("aux_index == n_traces", ERR_ARG, "trace", None, None, dict(aux_index=3)),
    ("AUX_CUR column == n_cols", ERR_ARG, "column", _with(2, a=(A.AUX_CUR, 5)), None, {}),
    ("AUX_NEXT column 9: a main column only", ERR_ARG, "column", _with(3, b=(A.AUX_NEXT, 9)), None, {}),
    ("source 9", ERR_ARG, "source", _with(0, a=(9, 0)), None, {}),
    ("source 255", ERR_ARG, "source", _with(4, b=(255, 0)), None, {}),
    ("main column == n_cols", ERR_ARG, "column", _with(0, a=(U.CUR, 10)), None, {}),
    ("op 0", ERR_ARG, "op", _with(0, op=0), None, {}),
    ("reserved0", ERR_ARG, "reserved", None, _reserved0, {}),
    ("main_index == n_traces", ERR_ARG, "trace", None, None, dict(main_index=3)),
    ("main commitment of extension columns", ERR_ARG, "extension degree", None, None, dict(main_is_aux=True)),
    ("ext_degree 0", ERR_EXTENSION, "extension", None, None, dict(ext=0)),
    ("ext_degree 4", ERR_EXTENSION, "extension", None, None, dict(ext=4)),
    ("log2_ce_blowup 0", ERR_BLOWUP, "blowup", None, None, dict(log_ce_b=0)),
    ("log2_ce_blowup > log2_blowup", ERR_BLOWUP, "blowup", None, None, dict(log_ce_b=LOG_B + 1)),
]


@pytest.mark.parametrize("what,code,word,g,patch,args", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusal_through_the_c_abi(ctx, capi, what, code, word, g, patch, args):
    """Each refusal with its code and a word of its message; nothing is launched (one profile mark stands in front of every
    launch), *out stays untouched, and a valid call on the same handles succeeds afterwards."""
    field, log_r = F64, 5
    com, ldes = _commit(ctx, capi, field, 1, log_r, 10, 3)
    aux, aux_ldes = _commit(ctx, capi, field, 2, log_r, 5, 3, aux=True)
    bad_aux, made, other = aux, None, None
    if args.get("aux"):
        a = dict(field=field, ext=2, log_r=log_r, log_b=LOG_B, offset=OFFSET[field])
        a.update(args["aux"])
        rng = np.random.default_rng(1)
        cols = E.pattern_columns(rng, a["field"], 5, 1 << a["log_r"], ext=a["ext"])
        made, _ = ctx.trace_commit_resident(capi.make_params(a["field"], a["ext"], a["log_r"], a["log_b"], 5, 1, offset=a["offset"]), cols)
        bad_aux = made
    if args.get("other_ctx"):
        other = capi.Context(0)
        cols = E.pattern_columns(np.random.default_rng(1), field, 5, 1 << log_r, ext=2)
        made, _ = other.trace_commit_resident(capi.make_params(field, 2, log_r, LOG_B, 5, 1), cols)
        bad_aux = made
    ext = args.get("ext", 2)
    cp, keep = U.to_capi(capi, g or _small(), field, 2)
    if patch:
        patch(cp, keep)
    h = C.c_void_p()
    L = capi.load()
    ctx.synchronize()
    ctx.profile_enable(2)   # one mark in front of every launch from here on
    rc = L.wf_constraint_evaluate_aux(None if args.get("null_main") else (aux._h if args.get("main_is_aux") else com._h),
                                      args.get("main_index", 0), None if args.get("null_aux") else bad_aux._h, args.get("aux_index", 0),
                                      None if args.get("null_prog") else C.byref(cp), ext, args.get("log_ce_b", 2),
                                      None if args.get("null_out") else C.byref(h))
    marks = ctx.profile_read()
    ctx.profile_enable(0)
    assert rc == code, L.wf_last_error()
    assert word in L.wf_last_error().decode() and not h.value
    assert marks == [], f"the refused call launched: {marks}"
    if made is not None:
        made.close()
    if other is not None:
        other.close()
    # a further valid call on the same handles
    g2 = _small()
    ev = ctx.constraint_evaluate_aux(com, 0, aux, 0, U.to_capi(capi, g2, field, 2), 2, 2)
    _compare(ev, _reference(g2, field, 2, ldes[0], aux_ldes[0], 2), field, "valid call after the refusal")
    ev.close()


def test_the_main_call_still_refuses_the_auxiliary_sources(ctx, capi):
    com, _ = _commit(ctx, capi, F64, 1, 5, 10, 3)
    for i, a in ((2, (A.AUX_CUR, 0)), (2, (A.AUX_NEXT, 0))):
        with pytest.raises(capi.WfError) as e:
            ctx.constraint_evaluate(com, 0, U.to_capi(capi, _with(i, a=a), F64, 2), 2, 2)
        assert e.value.code == ERR_ARG and "source" in str(e.value)


def test_device_tables_of_different_contexts_or_sizes_are_refused_as_before(ctx, capi):
    field, log_r = F64, 5
    com, _ = _commit(ctx, capi, field, 1, log_r, 10, 3)
    aux, _ = _commit(ctx, capi, field, 2, log_r, 5, 3, aux=True)
    div = [(1 << log_r, E.elements(field, [E.ONE[field]]), None)]
    cp = U.to_capi(capi, _small(), field, 2)
    ev = ctx.constraint_evaluate_aux(com, 0, aux, 0, cp, 2, 2)
    ev_other_size = ctx.constraint_evaluate_aux(com, 0, aux, 0, cp, 2, 1)
    ev_main = ctx.constraint_evaluate(com, 0, U.to_capi(capi, U.build("fib", field, 2, np.random.default_rng(1), 128, 4, 10), field, 2), 2, 2)
    p = capi.make_params(field, 2, log_r, LOG_B, 2, 1)
    fc = E.elements(field, [5, 6])
    other = capi.Context(0)
    try:
        with pytest.raises(capi.WfError) as e:
            ctx.constraint_commit_from_device_tables(p, [(ev, div), (ev_other_size, div)], fc)
        assert e.value.code == ERR_ARG
        with pytest.raises(capi.WfError) as e:
            other.constraint_commit_from_device_tables(p, [(ev, div)])
        assert e.value.code == ERR_ARG and "context" in str(e.value)
    finally:
        other.close()
    c, _ = ctx.constraint_commit_from_device_tables(p, [(ev, div), (ev_main, div)], fc)   # handles of both calls side by side
    c.close()
    for x in (ev, ev_other_size, ev_main):
        x.close()
