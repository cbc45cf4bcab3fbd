"""GPU: constraint programs on the resident trace LDE (wf_constraint_evaluate, csrc/constraint_eval.hip) -- every element of
every evaluation column against tests/cprog_util.py, the interpreter restated on Python integers, which runs on the LDE rows
read back through wf_commitment_read_lde -- and the chain into the constraint commitment with the columns left on the device
(wf_constraint_commit_from_device_tables) against the host-table call and the oracle's route of test_gpu_constraint_poly.py.

Shapes: trace lengths 2^3, 2^5, 2^8 at LDE blowup 8 with ce blowup 2, 4, 8 -- a ce of 16 (a partial work-group whatever size the
planner picks), several work-groups, lde_step = step << 2, 1, 0, and NEXT wrapping in the last ce_blowup steps --, 1, 8 and 10
columns (10: rows of 16 with padding lanes), three packed traces read at index 0 and 2.  Trace columns are the patterns of
tests/edge_util.py (limb-alphabet draws, p - 1, zeros, ..), constants and tables limb-alphabet draws.

One refusal of the header is not reached here: a commitment without resident rows exists only as the polynomial handle of a
sharded commitment (a communicator); tests/test_cprog_host.py produces it from the planner."""
import ctypes as C

import numpy as np
import pytest

import cprog_util as U
import edge_util as E

pytestmark = pytest.mark.gpu
F64, F128 = 1, 2
FIELDS = [(F64, 1), (F64, 2), (F64, 3), (F128, 1), (F128, 2)]
LOG_B = 3
#        log2 R, log2 ce blowup, columns, packed traces, trace read
SHAPES = [(3, 1, 1, 1, 0), (5, 2, 8, 3, 2), (8, 3, 10, 3, 0)]
OFFSET = {F64: 7, F128: 3}

_COMMITS = {}


def _commit(ctx, capi, field, log_r, n_cols, n_traces):
    """A resident commitment of pattern columns and, per trace, its LDE rows as integers: made once per shape, left unchanged."""
    key = (field, log_r, n_cols, n_traces)
    if key not in _COMMITS:
        rng = np.random.default_rng(hash(key) % 2**32)
        cols = [c for t in range(n_traces) for c in E.pattern_columns(rng, field, n_cols, 1 << log_r, first=t)]
        com, _ = ctx.trace_commit_resident(capi.make_params(field, 1, log_r, LOG_B, n_cols, n_traces), cols)
        n = 1 << (log_r + LOG_B)
        ldes = [U.lde_ints(field, com.read_lde(t, 0, n)) for t in range(n_traces)]
        assert ldes[0].shape[1] == 8 * ((n_cols + 7) // 8)
        _COMMITS[key] = (com, ldes, cols)
    return _COMMITS[key]


def _reference(g, field, ext, lde, log_ce_b):
    cur, nxt = U.frame_rows(lde, 1 << LOG_B, 1 << log_ce_b)
    return U.evaluate(g, field, ext, cur, nxt, U.ce_points(field, cur.shape[0], OFFSET[field]))


def _compare(ev, want, field, what):
    assert ev.n_columns == len(want)
    for j, w in enumerate(want):
        got = U.column_ints(field, ev.read(j))
        assert len(got) == len(w) == ev.ce_domain_size * ev.ext_degree
        bad = [i for i, (a, b) in enumerate(zip(got, w)) if a != b]
        assert not bad, f"{what}: column {j}: {len(bad)} of {len(w)} elements differ, first at {bad[0]}"


@pytest.mark.parametrize("name", U.PROGRAMS)
@pytest.mark.parametrize("log_r,log_ce_b,n_cols,n_traces,trace_index", SHAPES)
@pytest.mark.parametrize("field,ext", FIELDS)
def test_programs_match_the_python_reference(ctx, capi, field, ext, log_r, log_ce_b, n_cols, n_traces, trace_index, name):
    com, ldes, _ = _commit(ctx, capi, field, log_r, n_cols, n_traces)
    ce = 1 << (log_r + log_ce_b)
    rng = np.random.default_rng([field, ext, log_r, U.PROGRAMS.index(name)])
    g = U.build(name, field, ext, rng, ce, 1 << log_ce_b, n_cols)
    if name == "periodic" and log_r == 3:
        assert sorted(len(v) for v, _ in g.tables) == [2 << log_ce_b, ce]   # a table as long as the domain
    if name == "stress":
        assert sorted(len(v) for v, _ in g.tables) == [2, ce] and len(g.instrs) == 300
    ev = ctx.constraint_evaluate(com, trace_index, U.to_capi(capi, g, field, ext), ext, log_ce_b)
    assert (ev.n_columns, ev.ce_domain_size, ev.ext_degree) == (len(g.out_regs), ce, ext)
    _compare(ev, _reference(g, field, ext, ldes[trace_index], log_ce_b), field, name)
    ev.close()


@pytest.mark.parametrize("field,ext", [(F64, 2), (F128, 2)])
def test_a_handle_of_the_asynchronous_commitment_is_valid_input_before_wait(ctx, capi, field, ext):
    log_r, n_cols, log_ce_b = 8, 8, 2
    rng = np.random.default_rng(field)
    cols = E.pattern_columns(rng, field, n_cols, 1 << log_r)
    com = ctx.trace_commit_resident_async(capi.make_params(field, 1, log_r, LOG_B, n_cols, 1), cols)
    g = U.build("fib", field, ext, rng, 1 << (log_r + log_ce_b), 1 << log_ce_b, n_cols)
    ev = ctx.constraint_evaluate(com, 0, U.to_capi(capi, g, field, ext), ext, log_ce_b)   # queued behind the commitment's kernels
    com.wait()
    lde = U.lde_ints(field, com.read_lde(0, 0, 1 << (log_r + LOG_B)))
    _compare(ev, _reference(g, field, ext, lde, log_ce_b), field, "fib on an asynchronous commitment")
    ev.close()
    com.close()


def test_two_evaluations_back_to_back_keep_their_own_columns(ctx, capi):
    field, ext, log_r, n_cols, log_ce_b = F64, 2, 8, 10, 2
    com, ldes, _ = _commit(ctx, capi, field, log_r, n_cols, 3)
    ce = 1 << (log_r + log_ce_b)
    rng = np.random.default_rng(77)
    g1 = U.build("periodic", field, ext, rng, ce, 1 << log_ce_b, n_cols)
    g2 = U.build("sequence", field, ext, rng, ce, 1 << log_ce_b, n_cols)   # the same number of columns: the same buffer size
    ev1 = ctx.constraint_evaluate(com, 1, U.to_capi(capi, g1, field, ext), ext, log_ce_b)
    ev2 = ctx.constraint_evaluate(com, 1, U.to_capi(capi, g2, field, ext), ext, log_ce_b)
    _compare(ev2, _reference(g2, field, ext, ldes[1], log_ce_b), field, "second")
    _compare(ev1, _reference(g1, field, ext, ldes[1], log_ce_b), field, "first, read after the second ran")
    ev1.close()
    ev2.close()


def test_a_wide_frame_takes_more_than_64_kib_of_local_memory(ctx, capi):
    """70 columns read in both rows: 141 slots of 8 bytes are 70.5 KiB for one wave -- the launch that has to ask for more than
    the default 64 KiB of dynamic local memory."""
    field, ext, log_r, n_cols, log_ce_b = F64, 1, 5, 70, 3
    com, ldes, _ = _commit(ctx, capi, field, log_r, n_cols, 1)
    g = U.Prog(1)
    g.add(0, (U.CUR, 0), (U.NEXT, 0))
    for c in range(1, n_cols):
        g.add(0, (U.REG, 0), (U.CUR, c))
        g.mul(0, (U.REG, 0), (U.NEXT, c))
    g.out_regs = [0]
    ev = ctx.constraint_evaluate(com, 0, U.to_capi(capi, g, field, ext), ext, log_ce_b)
    _compare(ev, _reference(g, field, ext, ldes[0], log_ce_b), field, "wide frame")
    ev.close()


def test_a_frame_that_just_fits_and_one_that_does_not(ctx, capi):
    """128 columns in both rows and 64 registers are 320 slots: 163840 bytes for one wave, all the local memory of a compute
    unit.  One column more is refused (a refusal the issue does not list: the planner's own, see wf_lde.h)."""
    field, log_r, log_ce_b = F64, 5, 3
    com, ldes, _ = _commit(ctx, capi, field, log_r, 130, 1)
    g = U.wide_frame(field, 128)
    ev = ctx.constraint_evaluate(com, 0, U.to_capi(capi, g, field, 1), 1, log_ce_b)
    _compare(ev, _reference(g, field, 1, ldes[0], log_ce_b), field, "320 slots")
    ev.close()
    with pytest.raises(capi.WfError) as e:
        ctx.constraint_evaluate(com, 0, U.to_capi(capi, U.wide_frame(field, 129), field, 1), 1, log_ce_b)
    assert e.value.code == -19 and "do not fit" in str(e.value)


def test_handles_destroyed_at_once_leave_the_queued_work_intact(ctx, capi):
    """evaluate(...).close() back to back: destroy waits for the queued upload of the program (not for the kernel), the buffers
    go back to the pool and are taken again by the next call on the same stream.  The evaluation that is kept reads right."""
    field, ext, log_r, n_cols, log_ce_b = F64, 2, 8, 10, 2
    com, ldes, _ = _commit(ctx, capi, field, log_r, n_cols, 3)
    ce = 1 << (log_r + log_ce_b)
    rng = np.random.default_rng(5)
    progs = [U.build(name, field, ext, rng, ce, 1 << log_ce_b, n_cols) for name in ("stress", "periodic", "stress")]
    for g in progs:
        ctx.constraint_evaluate(com, 0, U.to_capi(capi, g, field, ext), ext, log_ce_b).close()
    g = progs[1]
    ev = ctx.constraint_evaluate(com, 2, U.to_capi(capi, g, field, ext), ext, log_ce_b)
    ctx.constraint_evaluate(com, 0, U.to_capi(capi, progs[0], field, ext), ext, log_ce_b).close()
    _compare(ev, _reference(g, field, ext, ldes[2], log_ce_b), field, "kept handle")
    ev.close()


# ------------------------------------------------------------------------------------------------ the chain
def _trace_domain_point(orc, field, log_r, e):
    """g_R^e in memory representation, as an array"""
    v = pow(U.root_of_unity(field, log_r), e, U.P[field])
    return E.elements(field, [U.to_mem(field, v)])


def _divisors(orc, field, log_r, kinds):
    """'t': the transition divisor (x^R - 1) / (x - g^(R-1)); 'first' / 'last': the single assertions' (x - g^step)"""
    R = 1 << log_r
    one = E.elements(field, [E.ONE[field]])
    out = []
    for k in kinds:
        if k == "t":
            out.append((R, one, _trace_domain_point(orc, field, log_r, R - 1)))
        else:
            out.append((1, _trace_domain_point(orc, field, log_r, 0 if k == "first" else R - 1), None))
    return out


@pytest.mark.parametrize("name,field,ext,n_traces", [("do_work", F128, 1, 1), ("do_work", F128, 2, 1), ("do_work", F128, 1, 3),
                                                     ("do_work", F128, 2, 3), ("periodic", F64, 2, 1)])
def test_commit_from_device_tables_is_the_host_table_call_and_the_oracle(ctx, orc, capi, name, field, ext, n_traces):
    log_r, log_ce_b, n_cols_c = 8, 2, 4
    n_cols = 1 if name == "do_work" else 8
    com, ldes, _ = _commit(ctx, capi, field, log_r, n_cols, n_traces)
    ce = 1 << (log_r + log_ce_b)
    rng = np.random.default_rng([field, ext, n_traces])
    kinds = ["t", "first", "last"] if name == "do_work" else ["t", "t"]
    divs = _divisors(orc, field, log_r, kinds)
    evs, host_tables, combined = [], [], []
    for t in range(n_traces):
        g = U.build(name, field, ext, rng, ce, 1 << log_ce_b, n_cols)
        ev = ctx.constraint_evaluate(com, t, U.to_capi(capi, g, field, ext), ext, log_ce_b)
        cols = [ev.read(j) for j in range(ev.n_columns)]
        _compare(ev, _reference(g, field, ext, ldes[t], log_ce_b), field, f"trace {t}")
        evs.append(ev)
        host_tables.append(list(zip(cols, divs)))
        combined.append(orc.combine_evaluation_table(field, ext, cols, divs, OFFSET[field]))
    fc = E.elements(field, U.draw(rng, field, ext))
    p = capi.make_params(field, ext, log_r, LOG_B, n_cols_c, 1)
    dev, dev_polys = ctx.constraint_commit_from_device_tables(p, [(ev, divs) for ev in evs], fc if n_traces > 1 else None, want_polys=True)
    host, host_polys = ctx.constraint_commit_from_tables(p, host_tables, fc if n_traces > 1 else None, want_polys=True)
    want_cols = orc.composition_poly_from_evaluations(field, ext, combined, log_r, n_cols_c, OFFSET[field], fc)
    want = orc.build_constraint_commitment(field, want_cols, ext, log_r, LOG_B, OFFSET[field])
    assert dev.root() == host.root() == want["root"]
    for c in range(n_cols_c):
        assert np.array_equal(dev_polys[c], host_polys[c]) and np.array_equal(dev_polys[c], want_cols[c]), f"column {c}"
    N = 1 << (log_r + LOG_B)
    pos = np.unique(rng.integers(0, N, size=12))
    rows_d, proof_d = dev.query(pos)
    rows_h, proof_h = host.query(pos)
    assert np.array_equal(rows_d, rows_h) and proof_d == proof_h
    assert proof_d == orc.merkle_prove_batch(want["nodes"], want["leaves"], [int(q) for q in pos])
    flat = rows_d.reshape(len(pos), -1)
    assert np.array_equal(flat, want["lde"].reshape(N, -1)[pos][:, :flat.shape[1]])
    for ev in evs:   # the columns were read in place, not consumed
        assert np.array_equal(ev.read(0), host_tables[evs.index(ev)][0][0])
        ev.close()
    dev.close()
    host.close()


@pytest.mark.parametrize("ext", [1, 2])
def test_do_work_on_a_valid_trace_divides_to_a_low_degree_polynomial(ctx, capi, ext):
    """The trace as examples/src/do_work/prover.rs builds it (state' = state^3 + 42): the transition column divided by
    (x^R - 1) / (x - g^(R-1)) interpolates to a polynomial of degree < ce - R -- the top R coefficients are zero --, and on a
    trace with one wrong state they are not."""
    field, log_r, log_ce_b = F128, 8, 2
    p, R, ce = U.P[field], 1 << log_r, 1 << (log_r + log_ce_b)
    state, trace = 7, []
    for _ in range(R):
        trace.append(state)
        state = (pow(state, 3, p) + 42) % p
    rng = np.random.default_rng(ext)
    coef = U.draw_e(rng, field, ext)
    g = U.do_work(field, ext, coef, trace[0], trace[-1], [U.draw_e(rng, field, ext), U.draw_e(rng, field, ext)])
    gR = pow(U.root_of_unity(field, log_r), R - 1, p)
    xs = U.ce_points(field, ce, OFFSET[field])
    inv_z = [(x - gR) * pow(pow(x, R, p) - 1, -1, p) % p for x in xs]
    tops = []
    for column in (trace, trace[:100] + [trace[100] + 1] + trace[101:]):
        com, _ = ctx.trace_commit_resident(capi.make_params(field, 1, log_r, LOG_B, 1, 1), [E.elements(field, column)])
        ev = ctx.constraint_evaluate(com, 0, U.to_capi(capi, g, field, ext), ext, log_ce_b)
        col = U.column_ints(field, ev.read(0))
        q = [col[i] * inv_z[i // ext] % p for i in range(ce * ext)]
        poly = ctx.fft_interpolate_poly_with_offset(field, ext, E.elements(field, q), OFFSET[field])
        tops.append(U.column_ints(field, poly)[(ce - R) * ext:])
        ev.close()
        com.close()
    assert not any(tops[0]), "the valid trace does not satisfy the program: it is not the AIR"
    assert any(tops[1])


# ------------------------------------------------------------------------------------------------ refusals
ERR_ARG, ERR_EXTENSION, ERR_BLOWUP = -19, -11, -13


def _small(ext=2):
    g = U.Prog(3)
    g.add(0, (U.CUR, 0), g.const(5))
    g.mul(0, (U.REG, 0), g.table([1, 2, 3, 4], shift=1))
    g.mul(1, (U.REG, 0), g.econst([3] * ext))
    g.out_regs = [1]
    return g


def _with(i, **kw):
    g = _small()
    op, dst, a, b = g.instrs[i]
    g.instrs[i] = (kw.get("op", op), kw.get("dst", dst), kw.get("a", a), kw.get("b", b))
    return g


def _footprint(field, ext):
    g = U.Prog(64)
    n_e = 0 if ext == 1 else 4
    for r in range(n_e):
        g.mul(r, (U.CUR, 0), g.econst([1] * ext))
    for r in range(n_e, n_e + U.MAX_FOOTPRINT[field] - n_e * ext + 1):
        g.add(r, (U.CUR, 0), (U.CUR, 1))
    g.out_regs = [0]
    return g


def _set(**fields):
    def patch(cp, keep):
        for k, v in fields.items():
            setattr(cp, k, v)
    return patch


def _instr(i, **fields):
    def patch(cp, keep):
        for k, v in fields.items():
            setattr(cp.instrs[i], k, v)
    return patch


def _table0(**fields):
    def patch(cp, keep):
        for k, v in fields.items():
            setattr(cp.tables[0], k, v)
    return patch


def _bad_const(cp, keep):
    keep[1][0] = np.uint64(E.P64)


def _bad_table(cp, keep):
    keep[4][0][2] = np.uint64(2**64 - 1)


def _out_reg(v):
    def patch(cp, keep):
        cp.out_regs[0] = v
    return patch


def _tab_len_128(g):
    g.tables[0] = ([1] * 128, 0)
    return g


def _second_type(g):
    g.add(0, (U.REG, 1), (U.REG, 1))
    return g


# (what, code, program, patch of the C structure, other arguments)
REFUSALS = [
    ("prog is null", ERR_ARG, None, None, dict(null_prog=True)),
    ("instrs is null", ERR_ARG, None, _set(instrs=None), {}),
    ("out_regs is null", ERR_ARG, None, _set(out_regs=None), {}),
    ("consts is null", ERR_ARG, None, _set(consts=None), {}),
    ("econsts is null", ERR_ARG, None, _set(econsts=None), {}),
    ("tables is null", ERR_ARG, None, _set(tables=None), {}),
    ("table values is null", ERR_ARG, None, _table0(values=None), {}),
    ("out is null", ERR_ARG, None, None, dict(null_out=True)),
    ("commitment is null", ERR_ARG, None, None, dict(null_com=True)),
    ("reserved0", ERR_ARG, None, _instr(1, reserved0=1), {}),
    ("reserved1", ERR_ARG, None, _instr(0, reserved1=9), {}),
    ("table reserved", ERR_ARG, None, _table0(reserved=1), {}),
    ("op 0", ERR_ARG, _with(0, op=0), None, {}),
    ("op 4", ERR_ARG, _with(0, op=4), None, {}),
    ("source 7 (reserved: aux frame)", ERR_ARG, _with(0, a=(7, 0)), None, {}),
    ("source 255", ERR_ARG, _with(2, b=(255, 0)), None, {}),
    ("n_instrs 0", ERR_ARG, None, _set(n_instrs=0), {}),
    ("n_instrs 4097", ERR_ARG, None, _set(n_instrs=4097), {}),
    ("n_regs 0", ERR_ARG, None, _set(n_regs=0), {}),
    ("n_regs 65", ERR_ARG, None, _set(n_regs=65), {}),
    ("n_out 0", ERR_ARG, None, _set(n_out=0), {}),
    ("n_out 33", ERR_ARG, None, _set(n_out=33), {}),
    ("dst out of range", ERR_ARG, _with(0, dst=3), None, {}),
    ("register out of range", ERR_ARG, _with(1, a=(U.REG, 3)), None, {}),
    ("constant out of range", ERR_ARG, _with(0, b=(U.CONST, 1)), None, {}),
    ("E constant out of range", ERR_ARG, _with(2, b=(U.ECONST, 1)), None, {}),
    ("table out of range", ERR_ARG, _with(1, b=(U.TABLE, 1)), None, {}),
    ("column index == n_cols", ERR_ARG, _with(0, a=(U.CUR, 10)), None, {}),
    ("register read before it is written", ERR_ARG, _with(0, a=(U.REG, 1)), None, {}),
    ("register written with a second type", ERR_ARG, _second_type(_small()), None, {}),
    ("out_regs entry never written", ERR_ARG, None, _out_reg(2), {}),
    ("out_regs entry out of range", ERR_ARG, None, _out_reg(3), {}),
    ("constant that is no field element", ERR_ARG, None, _bad_const, {}),
    ("table value that is no field element", ERR_ARG, None, _bad_table, {}),
    ("shift == len", ERR_ARG, None, _table0(shift=4), {}),
    ("len > ce", ERR_ARG, _tab_len_128(_small()), None, dict(log_ce_b=1, small=True)),
    ("trace_index == n_traces", ERR_ARG, None, None, dict(trace_index=3)),
    ("footprint f64 ext 2", ERR_ARG, _footprint(F64, 2), None, {}),
    ("footprint f64 ext 3", ERR_ARG, _footprint(F64, 3), None, dict(ext=3)),
    ("footprint f128 ext 1", ERR_ARG, _footprint(F128, 1), None, dict(field=F128, ext=1)),
    ("footprint f128 ext 2", ERR_ARG, _footprint(F128, 2), None, dict(field=F128)),
    ("commitment of extension columns", ERR_ARG, None, None, dict(trace_ext=2)),
    ("ext_degree 0", ERR_EXTENSION, None, None, dict(ext=0)),
    ("ext_degree 4", ERR_EXTENSION, None, None, dict(ext=4)),
    ("ext_degree 3 over f128", ERR_EXTENSION, _small(3), None, dict(field=F128, ext=3)),
    ("log2_ce_blowup 0", ERR_BLOWUP, None, None, dict(log_ce_b=0)),
    ("log2_ce_blowup > log2_blowup", ERR_BLOWUP, None, None, dict(log_ce_b=LOG_B + 1)),
]


@pytest.mark.parametrize("what,code,g,patch,args", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusal_through_the_c_abi(ctx, capi, what, code, g, patch, args):
    """Each refusal with its code; nothing is launched (the answer comes from the host-side planner), and a valid call on the same
    context succeeds afterwards."""
    field, ext = args.get("field", F64), args.get("ext", 2)
    log_r = 3 if args.get("small") else 5
    if args.get("trace_ext"):
        rng = np.random.default_rng(1)
        cols = E.pattern_columns(rng, field, 10, 1 << log_r, ext=2)
        com, _ = ctx.trace_commit_resident(capi.make_params(field, 2, log_r, LOG_B, 10, 1), cols)
    else:
        com, ldes, _ = _commit(ctx, capi, field, log_r, 10, 3)
    good = _small(ext if 1 <= ext <= 3 else 1)
    cp, keep = U.to_capi(capi, g or good, field, ext if 1 <= ext <= 3 else 1)
    if patch:
        patch(cp, keep)
    h = C.c_void_p()
    L = capi.load()
    ctx.synchronize()
    ctx.profile_enable(2)   # one mark in front of every launch from here on
    rc = L.wf_constraint_evaluate(None if args.get("null_com") else com._h, args.get("trace_index", 0),
                                  None if args.get("null_prog") else C.byref(cp), ext, args.get("log_ce_b", 2),
                                  None if args.get("null_out") else C.byref(h))
    marks = ctx.profile_read()
    ctx.profile_enable(0)
    assert rc == code, L.wf_last_error()
    assert L.wf_last_error() and not h.value
    assert marks == [], f"the refused call launched: {marks}"
    if args.get("trace_ext"):
        com.close()
        com, ldes, _ = _commit(ctx, capi, F64, 5, 10, 3)
    # a further valid call on the same context
    f2 = com.field
    g2 = _small(2)
    ev = ctx.constraint_evaluate(com, 0, U.to_capi(capi, g2, f2, 2), 2, 2)
    _compare(ev, _reference(g2, f2, 2, ldes[0], 2), f2, "valid call after the refusal")
    ev.close()


def test_device_tables_of_different_contexts_sizes_or_extensions_are_refused(ctx, capi):
    field, log_r = F64, 5
    com, _, _ = _commit(ctx, capi, field, log_r, 10, 3)
    one = E.elements(field, [E.ONE[field]])
    div = [(1 << log_r, one, None)]
    g = _small(2)
    ev = ctx.constraint_evaluate(com, 0, U.to_capi(capi, g, field, 2), 2, 2)
    ev_other_size = ctx.constraint_evaluate(com, 0, U.to_capi(capi, g, field, 2), 2, 1)
    ev_other_ext = ctx.constraint_evaluate(com, 0, U.to_capi(capi, _small(3), field, 3), 3, 2)
    p = capi.make_params(field, 2, log_r, LOG_B, 2, 1)
    fc = E.elements(field, [5, 6])
    other = capi.Context(0)
    try:
        for tables in ([(ev, div), (ev_other_size, div)], [(ev, div), (ev_other_ext, div)], [(ev_other_ext, div)]):
            with pytest.raises(capi.WfError) as e:
                ctx.constraint_commit_from_device_tables(p, tables, fc)
            assert e.value.code == ERR_ARG
        with pytest.raises(capi.WfError) as e:
            other.constraint_commit_from_device_tables(p, [(ev, div)])
        assert e.value.code == ERR_ARG and "context" in str(e.value)
    finally:
        other.close()
    c, _ = ctx.constraint_commit_from_device_tables(p, [(ev, div), (ev, div)], fc)   # the context is fine afterwards
    c.close()
    for x in (ev, ev_other_size, ev_other_ext):
        x.close()
