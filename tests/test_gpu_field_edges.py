"""GPU: the product kernels on carry-edge data, against the oracle, bit for bit.

Every other GPU test draws its field elements uniformly, and the rare branches of the device's 32-bit carry / borrow chains
(csrc/field.hpp) fire about once in 2^32 operations on such data.  Here the transforms, the trace commitment, the FRI
folding, the out-of-domain evaluation and the Rescue row hash run on the column patterns of tests/edge_util.py: all zero,
all p - 1, one constant, a single non-zero entry, alternating 0 and p - 1, and elements drawn from the limb alphabet --
mixed across the columns of one matrix, so that packed rows and segments hold different patterns side by side.  The oracle
is unsigned __int128 arithmetic that shares nothing with the limb chains.

The shapes are the smallest that still select each kernel family (see the comments of tests/test_gpu_parity.py);
tests/test_gpu_plans.py runs this file again under every forced plan, which is how the same data reaches the three- and
four-pass plans, the wide strided kernel, the generic tiles and the per-tile factor tables."""
import zlib

import numpy as np
import pytest

import edge_util as E

pytestmark = pytest.mark.gpu

F64, F128 = E.F64, E.F128
OFFSETS = {F64: (7, E.P64 - 1), F128: (3, E.P128 - 1)}   # canonical domain offsets: a small one and -1


def _seed(*key):
    return zlib.crc32(repr(key).encode())   # (hash() of a string differs from process to process)


# ------------------------------------------------------------------------------------------------ stand-alone transforms
FIELD_EXT = [(F64, 1), (F64, 2), (F64, 3), (F128, 1), (F128, 2)]


@pytest.mark.parametrize("field,ext", FIELD_EXT)
@pytest.mark.parametrize("logn", [1, 4, 10, 11, 13])
def test_fft_on_edge_patterns(ctx, orc, field, ext, logn):
    n = 1 << logn
    tw = orc.get_twiddles(field, n)
    inv_tw = orc.get_twiddles(field, n, inverse=True)
    rng = np.random.default_rng(_seed("fft", field, ext, logn))
    for kind in E.PATTERNS:
        p = E.pattern_column(rng, field, kind, n, ext)
        want = p.copy()
        orc.evaluate_poly(field, want, n, ext, tw)
        got = ctx.fft_evaluate_poly(field, ext, p)
        assert np.array_equal(got, want), kind
        want_i = p.copy()
        orc.interpolate_poly(field, want_i, n, ext, inv_tw)
        assert np.array_equal(ctx.fft_interpolate_poly(field, ext, p), want_i), kind
        assert np.array_equal(ctx.fft_interpolate_poly(field, ext, got), p), kind


@pytest.mark.parametrize("field,ext", FIELD_EXT)
@pytest.mark.parametrize("logn", [1, 4, 10, 11, 13])
def test_fft_with_offset_on_edge_patterns(ctx, orc, field, ext, logn):
    n = 1 << logn
    tw = orc.get_twiddles(field, n)
    inv_tw = orc.get_twiddles(field, n, inverse=True)
    rng = np.random.default_rng(_seed("fft_offset", field, ext, logn))
    for offset in OFFSETS[field]:
        off_mem = orc.lib().orc_f64_new(offset) if field == F64 else offset
        for kind in E.PATTERNS:
            p = E.pattern_column(rng, field, kind, n, ext)
            want = p.copy()
            orc.interpolate_poly_with_offset(field, want, n, ext, inv_tw, off_mem)
            assert np.array_equal(ctx.fft_interpolate_poly_with_offset(field, ext, p, offset), want), (offset, kind)
            for blowup in (2, 8):
                want_e = orc.evaluate_poly_with_offset(field, p, n, ext, tw, off_mem, blowup)
                got_e = ctx.fft_evaluate_poly_with_offset(field, ext, p, offset, blowup)
                assert np.array_equal(got_e, want_e), (offset, kind, blowup)


# ------------------------------------------------------------------------------------------------ trace commitment
CASES = [
    # field, ext, logR, logB, n_cols, n_traces
    (F64, 1, 3, 1, 1, 1),      # smallest legal trace
    (F64, 1, 10, 2, 3, 1),     # single pass, ragged
    (F64, 1, 11, 3, 8, 1),     # two passes, fused persistent last pass
    (F64, 1, 11, 7, 2, 1),     # coset-packed lanes
    (F64, 1, 13, 1, 17, 2),    # three segments, packed
    (F64, 3, 11, 2, 2, 1),     # cubic extension
    (F128, 1, 10, 3, 10, 1),   # do_work shape, tail-packed last segment
    (F128, 1, 12, 2, 3, 1),    # f128 fused last pass
    (F128, 2, 11, 2, 3, 1),    # quadratic extension over f128
]


@pytest.mark.parametrize("field,ext,logR,logB,n_cols,n_traces", CASES)
def test_trace_commit_on_edge_patterns(ctx, orc, capi, field, ext, logR, logB, n_cols, n_traces):
    """Polynomials, LDE, leaves, nodes and root.  The columns take the patterns in turn; a matrix of fewer columns than patterns
    is committed again with the next patterns until every pattern has been in it."""
    rng = np.random.default_rng(_seed("trace", field, ext, logR, logB, n_cols, n_traces))
    R = 1 << logR
    offset = OFFSETS[field][0]
    params = capi.make_params(field, ext, logR, logB, n_cols, n_traces)
    total = n_cols * n_traces
    for first in range(0, len(E.PATTERNS), total):
        cols = E.pattern_columns(rng, field, total, R, ext, first)
        traces = [cols[t * n_cols:(t + 1) * n_cols] for t in range(n_traces)]
        want = orc.build_trace_commitment(field, traces, ext, logR, logB, offset)
        got = ctx.trace_commit(params, cols)
        for t in range(n_traces):
            for c in range(n_cols):
                assert np.array_equal(got["polys"][t * n_cols + c], want["polys"][t][c]), f"poly {t},{c} (patterns from {first})"
            assert np.array_equal(got["lde"][t], want["lde"][t]), f"lde {t} (patterns from {first})"
        assert np.array_equal(got["leaves"], want["leaves"])
        assert np.array_equal(got["nodes"], want["nodes"])
        assert got["root"] == want["root"]


# ------------------------------------------------------------------------------------------------ FRI folding
@pytest.mark.parametrize("field,ext", FIELD_EXT)
@pytest.mark.parametrize("folding", [2, 4, 8, 16])
def test_fri_apply_drp_with_edge_alphas(ctx, orc, field, ext, folding):
    rng = np.random.default_rng(_seed("drp", field, ext, folding))
    rows = 512   # the domain is a power of two; several work-groups
    values = E.alphabet_draw(rng, field, rows * folding * ext)
    offset = OFFSETS[field][0]
    for alpha in E.edge_points(field, ext):
        want = orc.apply_drp(field, values, rows, ext, folding, offset, alpha)
        got = ctx.fri_apply_drp(field, ext, values, folding, offset, alpha)
        assert np.array_equal(got, want), f"alpha {alpha.tolist()}"


# ------------------------------------------------------------------------------------------------ out-of-domain evaluation
@pytest.mark.parametrize("field,ext_c,ext_z", [(F64, 1, 1), (F64, 1, 2), (F64, 1, 3), (F64, 2, 2), (F64, 3, 3),
                                               (F128, 1, 1), (F128, 1, 2), (F128, 2, 2)])
@pytest.mark.parametrize("logn", [7, 13])   # below one 4096-coefficient block, two blocks
def test_evaluate_columns_at_edge_points(ctx, orc, field, ext_c, ext_z, logn):
    rng = np.random.default_rng(_seed("ood", field, ext_c, ext_z, logn))
    n = 1 << logn
    cols = [E.alphabet_draw(rng, field, n * ext_c) for _ in range(2)] + [E.pattern_column(rng, field, "pm1", n, ext_c)]
    for z in E.edge_points(field, ext_z):
        got = ctx.evaluate_columns_at(field, ext_c, cols, z, ext_z)
        for i, c in enumerate(cols):
            assert np.array_equal(got[i], orc.eval_column_at(field, c, ext_c, z, ext_z)), f"column {i}, z {z.tolist()}"


# ------------------------------------------------------------------------------------------------ Rescue row hash
@pytest.fixture(scope="module")
def rctx(capi):
    """A context of its own whose hasher is Rp64_256 (the session's `ctx` stays on BLAKE3)."""
    c = capi.Context(0)
    c.set_hasher(capi.RP64_256)
    yield c
    c.close()


@pytest.mark.parametrize("row_elems", [8, 9])   # one full block; a full block and a partial one
def test_rp64_hash_rows_on_alphabet_rows(rctx, row_elems):
    import rp64_util as R
    before = R.PERMUTATIONS
    rng = np.random.default_rng(row_elems)
    rows = E.alphabet_draw(rng, F64, 64 * row_elems).reshape(64, row_elems)
    rows[0] = 0
    rows[1] = E.P64 - 1
    got = rctx.hash_rows(F64, rows, 64, row_elems)
    assert np.array_equal(got, R.hash_rows(rows))
    assert R.PERMUTATIONS - before <= 2048
