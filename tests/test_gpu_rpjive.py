"""GPU: RpJive64_256 (Rescue Prime of width 8 with the Jive compression) as hasher 18 (enum wf_hasher) -- row hashing,
Merkle trees, commitments in every single-GPU form, queries, FRI -- bit for bit against tests/rpjive_util.py (the function
restated on Python integers, parameters from tests/golden/rpjive64_256_params.json); polynomials and LDE values against
the oracle.

No test needs more than 2048 reference permutations: trees above 2^10 leaves are checked on a fixed sample (node[i] ==
merge(node[2i], node[2i+1]) on the device's own children: sample_indices), and of the 70 rows of 255 elements (64
permutations each) 31 are compared."""
import numpy as np
import pytest

import edge_util as E
import rpjive_util as R
from conftest import rand_cols, rand_f64, rand_f128
from loopback import Loopback

pytestmark = pytest.mark.gpu
F64, F128 = 1, 2
P = R.P
SPAN = 128        # parents per work-group of k_merkle_subtree_lanes<rpj::Lanes> (MERKLE_PLAN_RPJIVE.subtree_span, csrc/merkle_plan.hpp)
BUDGET = 2048     # reference permutations per test


@pytest.fixture(autouse=True)
def _permutation_budget():
    before = R.PERMUTATIONS
    yield
    assert R.PERMUTATIONS - before <= BUDGET, "the Python reference ran more permutations than a test may need"


@pytest.fixture(scope="module")
def jctx(capi):
    """A context of its own whose hasher is RpJive64_256 (the session's `ctx` stays on BLAKE3)."""
    c = capi.Context(0)
    c.set_hasher(capi.RPJIVE64_256)
    yield c
    c.close()


def _hash_rows_poisoned_tail(capi, c, rows, n_rows, row_elems, tail=5):
    """wf_hash_rows into a buffer with `tail` poisoned digests behind the last row: they must stay as they were."""
    a = np.ascontiguousarray(rows, dtype=np.uint64)
    out = np.full((n_rows + tail, 32), 0xA5, dtype=np.uint8)
    rc = capi.load().wf_hash_rows(c._h, F64, a.ctypes.data, n_rows, row_elems, out.ctypes.data)
    assert rc == 0, capi.load().wf_last_error()
    assert (out[n_rows:] == 0xA5).all()
    return out[:n_rows]


# ---------------------------------------------------------------------------------------------------------- hash_rows
# one rate block is 4 elements: 3, 4, 5 around one block, 7, 8, 9 around two, 12 and 13 around three; 300 rows cross a wave
# (64) and a work-group (256) and end in a partial wave (44 lanes)
@pytest.mark.parametrize("row_elems", [1, 3, 4, 5, 7, 8, 9, 12, 13])
def test_hash_rows(capi, jctx, row_elems):
    rng = np.random.default_rng(row_elems)
    rows = rand_f64(rng, 300 * row_elems).reshape(300, row_elems)
    rows[0, :] = 0                                   # canonical 0
    rows[1, :] = np.uint64(P - 1)                    # the largest residue: every addition into the rate wraps or lands in [p, 2^64)
    got = _hash_rows_poisoned_tail(capi, jctx, rows, 300, row_elems)
    assert np.array_equal(got, R.hash_rows(rows))
    assert (got.view(np.uint64) < np.uint64(P)).all()   # digests are written canonical
    assert np.array_equal(jctx.hash_rows(F64, rows, 300, row_elems), got)


def test_hash_rows_of_255_elements(capi, jctx):
    """70 rows of 255 elements (64 permutations each, the last block one element short); 31 of them are compared -- the
    first 20, the wave's last and the partial wave's 6, and four from the middle."""
    rng = np.random.default_rng(255)
    rows = rand_f64(rng, 70 * 255).reshape(70, 255)
    got = _hash_rows_poisoned_tail(capi, jctx, rows, 70, 255)
    keep = list(range(20)) + [31, 32, 40, 50, 63] + list(range(64, 70))
    assert len(keep) == 31
    assert np.array_equal(got[keep], R.hash_rows(rows[keep]))


@pytest.mark.parametrize("kind", ["zero", "pm1", "alt", "alphabet"])
@pytest.mark.parametrize("row_elems", [5, 8])
def test_hash_rows_of_carry_edge_patterns(capi, jctx, kind, row_elems):
    """The carry-edge patterns of tests/edge_util.py: all-zero rows, rows of p - 1, rows alternating between the two, and rows
    drawn from the limb alphabet (70 rows: a wave and a partial one)."""
    rng = np.random.default_rng(row_elems)
    cols = [E.pattern_column(rng, F64, kind, 70) for _ in range(row_elems)]
    rows = np.stack(cols, axis=1)
    got = _hash_rows_poisoned_tail(capi, jctx, rows, 70, row_elems)
    assert np.array_equal(got, R.hash_rows(rows))


@pytest.mark.parametrize("ext,folding", [(2, 2), (3, 2), (3, 4)])
def test_rows_of_extension_elements_count_base_elements(jctx, ctx, ext, folding):
    """A FRI layer's rows are `folding` extension elements: hash_elements flattens them (slice_as_base_elements), so the
    sponge sees folding * ext base elements -- 4, 6 and 12 here: state[0] is 0, 1 and 0."""
    n = 1 << 6
    ev = rand_f64(np.random.default_rng(10 * ext + folding), n * ext)
    got = jctx.fri_layer_commit(F64, ext, ev, folding)
    assert np.array_equal(got["transposed"], ctx.fri_layer_commit(F64, ext, ev, folding)["transposed"])
    rows = got["transposed"].reshape(n // folding, folding * ext)
    leaves = R.hash_rows(rows)
    assert np.array_equal(got["leaves"], leaves)
    nodes = R.merkle_nodes(leaves)
    assert np.array_equal(got["nodes"], nodes) and got["root"] == bytes(nodes[1])


# ---------------------------------------------------------------------------------------------------------- combined rows
@pytest.mark.parametrize("n_traces,n_cols", [(3, 3), (8, 8)])
def test_combined_rows_of_several_traces(capi, ctx, orc, n_traces, n_cols):
    """2^3 rows, blowup 2: the leaf is hash_elements over trace 0's columns, trace 1's, ..; the padding lanes of the stored
    rows (3 of 8 used) are neither counted nor absorbed -- the device-buffer form runs on an LDE buffer that was poisoned
    beforehand."""
    import torch
    logR, logB = 3, 1
    rng = np.random.default_rng(100 * n_traces + n_cols)
    traces = [rand_cols(rng, F64, n_cols, 1 << logR) for _ in range(n_traces)]
    want = orc.build_trace_commitment(F64, traces, 1, logR, logB, 7)
    p = capi.make_params(F64, 1, logR, logB, n_cols, n_traces, hasher=capi.RPJIVE64_256)
    flat = [c for t in traces for c in t]
    got = ctx.trace_commit(p, flat)
    for t in range(n_traces):
        assert np.array_equal(got["lde"][t], want["lde"][t])
    leaves = R.combined_leaves(want["lde"], n_cols)
    nodes = R.merkle_nodes(leaves)
    assert np.array_equal(got["leaves"], leaves)
    assert np.array_equal(got["nodes"], nodes)
    assert got["root"] == bytes(nodes[1])

    dev = torch.device("cuda", 0)
    N, rw = 1 << (logR + logB), 8
    d_trace = torch.from_numpy(np.concatenate(flat).view(np.int64)).to(dev)
    d_polys = torch.empty_like(d_trace)
    d_lde = torch.full((n_traces * N * rw,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device=dev)
    d_leaves = torch.full((N, 32), 0xA5, dtype=torch.uint8, device=dev)
    d_nodes = torch.full((N, 32), 0xA5, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ctx.trace_commit_dev(p, d_trace.data_ptr(), d_polys.data_ptr(), d_lde.data_ptr(), d_leaves.data_ptr(), d_nodes.data_ptr())
    ctx.synchronize()
    lde = d_lde.cpu().numpy().view(np.uint64).reshape(n_traces, N, rw)
    for t in range(n_traces):
        assert np.array_equal(lde[t][:, :n_cols], want["lde"][t][:, :n_cols])
    assert np.array_equal(d_leaves.cpu().numpy(), leaves) and np.array_equal(d_nodes.cpu().numpy(), nodes)


# ---------------------------------------------------------------------------------------------------------- merkle_build
# The switches of the tree (MERKLE_PLAN_RPJIVE, csrc/merkle_plan.hpp):
#   a level of >= 2^17 parents (>= 2^18 children) is one k_merkle_level<rpj::Merge> launch (one lane per parent): 2^16 and
#   2^17 leaves below the switch, 2^18 at it;
#   below that k_merkle_subtree_lanes<rpj::Lanes> (8 lanes per parent, 128 parents per work-group of 16 waves) folds up to 8 levels per
#   launch: 2^1 .. 2^3 leaves one to four groups of one wave, 2^4 exactly one wave, 2^5 two waves, 2^6 and 2^7 a partly idle
#   work-group, 2^8 exactly eight levels in one launch, 2^9 two work-groups and a second launch of one level, 2^10 four.
def _leaves(log_n):
    n = 1 << log_n
    rng = np.random.default_rng(log_n)
    leaves = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)
    # digest words a caller hands in may be any u64: some at and above p, read as BaseElement::new reads them
    edge = np.array([P, P + 1, 2**64 - 1, 2**64 - 2**32], dtype=np.uint64)
    leaves[0] = edge
    leaves[n - 1] = edge[::-1]
    leaves[1, 2] = np.uint64(P)
    return leaves.view(np.uint8).reshape(n, 32)


def _build_dev(jctx, leaves):
    import torch
    n = leaves.shape[0]
    dev = torch.device("cuda", 0)
    d_leaves = torch.from_numpy(leaves).to(dev)
    d_nodes = torch.full((n, 32), 0xA5, dtype=torch.uint8, device=dev)  # poisoned: every node must be written, [0] with zeros
    torch.cuda.synchronize()
    jctx.merkle_build_dev(d_leaves.data_ptr(), n, d_nodes.data_ptr())
    jctx.synchronize()
    return d_nodes.cpu().numpy()


@pytest.mark.parametrize("log_n", [1, 2, 3, 4, 5, 6, 7, 8, 9, 10])
def test_merkle_build_in_full(jctx, log_n):
    leaves = _leaves(log_n)
    want = R.merkle_nodes(leaves)
    got = _build_dev(jctx, leaves)
    assert not got[0].any()
    assert np.array_equal(got, want)
    assert (got.view(np.uint64) < np.uint64(P)).all()
    if log_n <= 3:  # the host-buffer form
        assert np.array_equal(jctx.merkle_build(leaves), want)


def test_merge_is_not_hash_elements_of_the_same_words(jctx):
    leaves = np.arange(1, 9, dtype=np.uint64).view(np.uint8).reshape(2, 32)
    got = _build_dev(jctx, leaves)
    assert bytes(got[1]) == R.merge(bytes(leaves[0]), bytes(leaves[1]))
    assert bytes(got[1]) != R.digest_bytes(R.hash_elements(list(range(1, 9))))


@pytest.mark.parametrize("log_n", [16, 17, 18])
def test_merkle_build_sampled(jctx, log_n):
    """Sizes on each side of the level / subtree switch; node[i] == merge(node[2i], node[2i+1]) on the device's own
    children over sample_indices with the sub-tree kernel's span.  (The leaves hold words >= p.)"""
    leaves = _leaves(log_n)
    got = _build_dev(jctx, leaves)
    assert not got[0].any()
    assert not (got[1:] == 0xA5).all(axis=1).any()      # no node was left as the buffer was
    assert (got.view(np.uint64) < np.uint64(P)).all()
    idx = R.sample_indices(1 << log_n, spans=(SPAN,), budget=BUDGET, seed=log_n)
    assert len(idx) == BUDGET
    R.check_tree_sampled(got, leaves, idx)


# ---------------------------------------------------------------------------------------------------------- commitments
@pytest.fixture(scope="module")
def small(orc):
    """f64 2^3 x 2 columns, blowup 2: the oracle's polynomials and LDE, the reference's leaves and tree (31 permutations)."""
    logR, logB, n_cols = 3, 1, 2
    cols = rand_cols(np.random.default_rng(33), F64, n_cols, 1 << logR)
    want = orc.build_trace_commitment(F64, [cols], 1, logR, logB, 7)
    leaves = R.combined_leaves(want["lde"], n_cols)
    return dict(logR=logR, logB=logB, n_cols=n_cols, cols=cols, want=want, leaves=leaves, nodes=R.merkle_nodes(leaves))


def _check_resident(com, orc, s):
    N = 1 << (s["logR"] + s["logB"])
    assert com.root() == bytes(s["nodes"][1])
    assert np.array_equal(com.read_lde(0, 0, N), s["want"]["lde"][0])
    for j in range(N):  # every path: together they hold every node of the tree
        assert com.prove(j) == orc.merkle_prove(s["nodes"], s["leaves"], j)


def test_small_commitment_in_every_form(capi, ctx, orc, small, monkeypatch):
    """Host form, device-buffer form, resident, resident asynchronous, the constraint side (the trace's own polynomials as
    its columns: the same LDE), and a resident commitment on a context that uploads through the pipelined route: the same
    leaves, nodes and root in each; the BLAKE3 twin before and after still equals the oracle's."""
    import torch
    s = small
    logR, logB, n_cols, cols, want, leaves, nodes = (s[k] for k in ("logR", "logB", "n_cols", "cols", "want", "leaves", "nodes"))
    p = capi.make_params(F64, 1, logR, logB, n_cols, 1, hasher=capi.RPJIVE64_256)
    pb = capi.make_params(F64, 1, logR, logB, n_cols, 1)
    assert ctx.trace_commit(pb, cols, want_lde=False, want_polys=False)["root"] == want["root"]

    got = ctx.trace_commit(p, cols)
    for c in range(n_cols):
        assert np.array_equal(got["polys"][c], want["polys"][0][c])
    assert np.array_equal(got["lde"][0], want["lde"][0])
    assert np.array_equal(got["leaves"], leaves) and np.array_equal(got["nodes"], nodes) and got["root"] == bytes(nodes[1])

    dev = torch.device("cuda", 0)
    N, rw = 1 << (logR + logB), 8
    d_trace = torch.from_numpy(np.concatenate(cols).view(np.int64)).to(dev)
    d_polys = torch.empty_like(d_trace)
    d_lde = torch.empty(N * rw, dtype=torch.int64, device=dev)
    d_leaves = torch.full((N, 32), 0xA5, dtype=torch.uint8, device=dev)
    d_nodes = torch.full((N, 32), 0xA5, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ctx.trace_commit_dev(p, d_trace.data_ptr(), d_polys.data_ptr(), d_lde.data_ptr(), d_leaves.data_ptr(), d_nodes.data_ptr())
    ctx.synchronize()
    assert np.array_equal(d_polys.cpu().numpy().view(np.uint64), np.concatenate(want["polys"][0]))
    assert np.array_equal(d_lde.cpu().numpy().view(np.uint64).reshape(N, rw), want["lde"][0])
    assert np.array_equal(d_leaves.cpu().numpy(), leaves) and np.array_equal(d_nodes.cpu().numpy(), nodes)

    com, polys = ctx.trace_commit_resident(p, cols, want_polys=True)
    for c in range(n_cols):
        assert np.array_equal(polys[c], want["polys"][0][c])
    _check_resident(com, orc, s)
    com.close()

    com = ctx.trace_commit_resident_async(p, cols)
    com.wait()
    _check_resident(com, orc, s)
    com.close()

    got = ctx.constraint_commit(p, want["polys"][0])
    assert np.array_equal(got["lde"][:, :n_cols], want["lde"][0][:, :n_cols])
    assert np.array_equal(got["leaves"], leaves) and np.array_equal(got["nodes"], nodes) and got["root"] == bytes(nodes[1])
    d_cpolys = torch.from_numpy(np.concatenate(want["polys"][0]).view(np.int64)).to(dev)
    d_leaves.fill_(0xA5)
    d_nodes.fill_(0xA5)
    torch.cuda.synchronize()
    ctx.constraint_commit_dev(p, d_cpolys.data_ptr(), d_lde.data_ptr(), d_leaves.data_ptr(), d_nodes.data_ptr())
    ctx.synchronize()
    assert np.array_equal(d_leaves.cpu().numpy(), leaves) and np.array_equal(d_nodes.cpu().numpy(), nodes)
    com = ctx.constraint_commit_resident(p, want["polys"][0])
    assert com.root() == bytes(nodes[1])
    com.close()

    monkeypatch.setenv("WF_EXP_ENABLE", "1")
    monkeypatch.setenv("WF_EXP_PIPELINE_MIN_BYTES", "0")
    c2 = capi.Context(0)   # (the switches are read when a context is created)
    try:
        com, _ = c2.trace_commit_resident(p, cols)
        _check_resident(com, orc, s)
        com.close()
    finally:
        c2.close()

    assert ctx.trace_commit(pb, cols, want_lde=False, want_polys=False)["root"] == want["root"]


def test_pipelined_upload_of_a_multi_segment_commitment(capi, orc, monkeypatch):
    """Host columns of a two-segment, two-pass matrix (2^11 x 9, the smallest that is both) go up under the kernels
    (trace_commit_pipelined).  2^12 leaves of three permutations each: 200 sampled leaves against their rows, the tree on a
    sample."""
    logR, logB, n_cols = 11, 1, 9
    assert len(capi.plan_digits(F64, logR, 2)) >= 2
    monkeypatch.setenv("WF_EXP_ENABLE", "1")
    monkeypatch.setenv("WF_EXP_PIPELINE_MIN_BYTES", "0")
    c = capi.Context(0)
    try:
        N = 1 << (logR + logB)
        cols = rand_cols(np.random.default_rng(119), F64, n_cols, 1 << logR)
        want = orc.build_trace_commitment(F64, [cols], 1, logR, logB, 7)
        p = capi.make_params(F64, 1, logR, logB, n_cols, 1, hasher=capi.RPJIVE64_256)
        com, polys = c.trace_commit_resident(p, cols, want_polys=True)
        for k in range(n_cols):
            assert np.array_equal(polys[k], want["polys"][0][k])
        assert np.array_equal(com.read_lde(0, 0, N), want["lde"][0])
        # the same commitment through the host form gives the arrays to check
        got = c.trace_commit(p, cols, want_lde=False, want_polys=False)
        assert got["root"] == com.root() == bytes(got["nodes"][1])
        rows = [0, 1, 63, 64, 255, 256, N - 1] + [int(x) for x in np.random.default_rng(5).integers(0, N, size=193)]
        for j in rows:
            assert bytes(got["leaves"][j]) == R.digest_bytes(R.hash_elements(R.combined_row(want["lde"], n_cols, j))), j
        R.check_tree_sampled(got["nodes"], got["leaves"], R.sample_indices(N, spans=(SPAN,), budget=BUDGET - 3 * len(rows)))
        path = com.prove(1000)
        assert path[0] == bytes(got["leaves"][1000]) and path == orc.merkle_prove(got["nodes"], got["leaves"], 1000)
        com.close()
        com, _ = c.trace_commit_resident(capi.make_params(F64, 1, logR, logB, n_cols, 1), cols)
        assert com.root() == want["root"]
        com.close()
    finally:
        c.close()


def test_constraint_commit_from_evaluations_ext2(capi, ctx, orc):
    """The constraint side from the combined evaluations (two packed tables, quadratic extension): rows of n_cols * 2 base
    elements."""
    field, ext, logR, log_ce_blowup, n_cols, logB = F64, 2, 3, 2, 3, 1
    rng = np.random.default_rng(631)
    tables = [rand_cols(rng, field, 1, (1 << (logR + log_ce_blowup)) * ext)[0] for _ in range(2)]
    fc = rand_f64(rng, ext)
    want_cols = orc.composition_poly_from_evaluations(field, ext, tables, logR, n_cols, 7, fc)
    want = orc.build_constraint_commitment(field, want_cols, ext, logR, logB, 7)
    leaves = R.combined_leaves([want["lde"]], n_cols * ext)
    nodes = R.merkle_nodes(leaves)
    p = capi.make_params(field, ext, logR, logB, n_cols, 1, hasher=capi.RPJIVE64_256)
    com, polys = ctx.constraint_commit_from_evaluations(p, tables, fc, want_polys=True)
    assert com.root() == bytes(nodes[1])
    for k in range(n_cols):
        assert np.array_equal(polys[k], want_cols[k])
    for j in (0, 5, (1 << (logR + logB)) - 1):
        assert com.prove(j) == orc.merkle_prove(nodes, leaves, j)
    com.close()
    got = ctx.constraint_commit(p, want_cols)
    assert np.array_equal(got["leaves"], leaves) and np.array_equal(got["nodes"], nodes)
    com, _ = ctx.constraint_commit_from_evaluations(capi.make_params(field, ext, logR, logB, n_cols, 1), tables, fc)
    assert com.root() == want["root"]
    com.close()


# ---------------------------------------------------------------------------------------------------------- queries
def test_queries_on_a_resident_commitment(capi, ctx, orc):
    field, logR, logB, n_cols, n_traces = F64, 5, 1, 3, 2   # 2^6 leaves
    rng = np.random.default_rng(77)
    traces = [rand_cols(rng, field, n_cols, 1 << logR) for _ in range(n_traces)]
    want = orc.build_trace_commitment(field, traces, 1, logR, logB, 7)
    leaves = R.combined_leaves(want["lde"], n_cols)
    nodes = R.merkle_nodes(leaves)
    root = bytes(nodes[1])
    N = 1 << (logR + logB)
    p = capi.make_params(field, 1, logR, logB, n_cols, n_traces, hasher=capi.RPJIVE64_256)
    com, _ = ctx.trace_commit_resident(p, [c for t in traces for c in t])
    assert com.root() == root
    pos = np.array([0, N - 1, 5, 32, 33, 31], dtype=np.uint64)
    rows, (q_leaves, q_nodes, depth) = com.query(pos)
    assert depth == logR + logB
    for i, j in enumerate(pos):
        assert np.array_equal(rows[i], np.concatenate([want["lde"][t][int(j), :n_cols] for t in range(n_traces)]))
        assert q_leaves[i] == R.hash_row(rows[i])   # the returned rows re-hashed
    b_leaves, b_nodes, b_depth = com.prove_batch(pos)
    assert (b_leaves, b_nodes, b_depth) == (q_leaves, q_nodes, depth)
    assert (b_leaves, b_nodes, b_depth) == orc.merkle_prove_batch(nodes, leaves, [int(j) for j in pos])
    for j in (0, N - 1, 37):
        path = com.prove(j)
        assert len(path) == depth + 1 and path[0] == bytes(leaves[j])
        assert path == orc.merkle_prove(nodes, leaves, j)
        assert R.verify_path(root, j, path)
        bad = list(path)
        bad[-1] = bytes(32)
        assert not R.verify_path(root, j, bad)      # (the check can fail)
    com.close()


# ---------------------------------------------------------------------------------------------------------- FRI
def test_fri_layer_commit(ctx, jctx):
    field, ext, n, folding = F64, 2, 1 << 8, 4
    ev = rand_f64(np.random.default_rng(8), n * ext)
    blake = ctx.fri_layer_commit(field, ext, ev, folding)
    got = jctx.fri_layer_commit(field, ext, ev, folding)
    assert np.array_equal(got["transposed"], blake["transposed"])
    leaves = R.hash_rows(got["transposed"].reshape(n // folding, folding * ext))
    nodes = R.merkle_nodes(leaves)
    assert np.array_equal(got["leaves"], leaves) and np.array_equal(got["nodes"], nodes) and got["root"] == bytes(nodes[1])
    assert got["root"] != blake["root"]


@pytest.mark.parametrize("folding", [4, 2])
def test_fri_prover(capi, ctx, jctx, orc, folding):
    """The same proof driven with the same caller-supplied alphas on a BLAKE3 and on an RpJive64_256 context: every layer's
    rows are equal, every layer root is the reference tree over those rows, the remainder digest is hash_elements of the
    remainder's base elements."""
    field, ext, blowup, max_rem, n = F64, 2, 4, 3, 1 << 8
    rng = np.random.default_rng(folding)
    ev = rand_f64(rng, n * ext)
    n_layers = capi.fri_num_layers(folding, blowup, max_rem, n)
    assert n_layers >= 2
    alphas = [rand_f64(rng, ext) for _ in range(n_layers)]
    provers = [capi.FriProver(c, field, ext, folding, blowup, max_rem, 7) for c in (ctx, jctx)]
    roots = []
    for pr in provers:
        pr.begin(ev)
        rr = []
        for a in alphas:
            rr.append(pr.commit_layer())
            pr.fold(a)
        roots.append(rr)
    size = n
    for i in range(n_layers):
        size //= folding
        all_rows = np.arange(size, dtype=np.uint64)
        lb, ls = provers[0].layer(i), provers[1].layer(i)
        rows = ls.read_rows(all_rows)
        assert np.array_equal(rows, lb.read_rows(all_rows))
        leaves = R.hash_rows(rows.reshape(size, folding * ext))
        nodes = R.merkle_nodes(leaves)
        assert roots[1][i] == bytes(nodes[1]) == ls.root()
        assert roots[1][i] != roots[0][i]
        assert ls.prove_batch(np.array([0, size - 1], dtype=np.uint64)) == orc.merkle_prove_batch(nodes, leaves, [0, size - 1])
    rem_b, _ = provers[0].set_remainder(size)
    rem_s, digest = provers[1].set_remainder(size)
    assert np.array_equal(rem_b, rem_s)
    assert digest == R.hash_row(rem_s.reshape(-1))
    for pr in provers:
        pr.close()


# ---------------------------------------------------------------------------------------------------------- refusals
def test_f128_is_refused_at_every_entry_point(capi, orc):
    """WF_FIELD_F128 under RpJive64_256: WF_ERR_FIELD (-10) before anything is launched, and nothing changes -- the BLAKE3
    commitment made on the same context afterwards equals the oracle's."""
    import torch
    c = capi.Context(0)
    try:
        logR, logB, n_cols = 3, 1, 2
        rng = np.random.default_rng(128)
        cols = rand_cols(rng, F128, n_cols, 1 << logR)
        p = capi.make_params(F128, 1, logR, logB, n_cols, 1, hasher=capi.RPJIVE64_256)
        p2 = capi.make_params(F128, 2, logR, logB, n_cols, 1, hasher=capi.RPJIVE64_256)
        dev = torch.device("cuda", 0)
        N, rw = 1 << (logR + logB), 4
        d_trace = torch.from_numpy(np.concatenate(cols).view(np.int64).reshape(-1)).to(dev)
        d_polys = torch.empty_like(d_trace)
        d_lde = torch.empty(N * rw * 2, dtype=torch.int64, device=dev)
        d_leaves = torch.full((N, 32), 0xA5, dtype=torch.uint8, device=dev)
        d_nodes = torch.full((N, 32), 0xA5, dtype=torch.uint8, device=dev)
        ext_cols = rand_cols(rng, F128, n_cols, (1 << logR) * 2)
        tables = [rand_cols(rng, F128, 1, (1 << (logR + 1)) * 2)[0] for _ in range(2)]
        calls = [
            lambda: c.trace_commit(p, cols),
            lambda: c.trace_commit_dev(p, d_trace.data_ptr(), d_polys.data_ptr(), d_lde.data_ptr(), d_leaves.data_ptr(),
                                       d_nodes.data_ptr()),
            lambda: c.trace_commit_resident(p, cols),
            lambda: c.trace_commit_resident_async(p, cols),
            lambda: c.constraint_commit(p, cols),
            lambda: c.constraint_commit_dev(p, d_trace.data_ptr(), d_lde.data_ptr(), d_leaves.data_ptr(), d_nodes.data_ptr()),
            lambda: c.constraint_commit_resident(p, cols),
            lambda: c.constraint_commit(p2, ext_cols),
            lambda: c.constraint_commit_from_evaluations(p2, tables, rand_f128(rng, 2)),
        ]
        for k, call in enumerate(calls):
            with pytest.raises(capi.WfError) as e:
                call()
            assert e.value.code == -10, k
        torch.cuda.synchronize()
        assert (d_leaves.cpu().numpy() == 0xA5).all() and (d_nodes.cpu().numpy() == 0xA5).all()   # nothing was launched

        # the entry points that take the context's hasher
        c.set_hasher(capi.RPJIVE64_256)
        rows = rand_f128(rng, 8 * 4).reshape(8, 4, 2)
        ev = rand_f128(rng, 64)
        ctx_calls = [
            lambda: c.hash_rows(F128, rows, 8, 4),
            lambda: c.fri_layer_commit(F128, 1, ev, 4),
            lambda: c.fri_apply_drp(F128, 1, ev, 4, 3, rand_f128(rng, 1)),
            lambda: capi.FriProver(c, F128, 1, 4, 4, 3, 3),
        ]
        for k, call in enumerate(ctx_calls):
            with pytest.raises(capi.WfError) as e:
                call()
            assert e.value.code == -10 and "RpJive64_256" in str(e.value), k
            assert c.hasher == capi.RPJIVE64_256 and c.digest_bytes == 32
        # a prover made while the context hashed with BLAKE3 meets the refusal when it first hashes
        c.set_hasher(capi.BLAKE3)
        pr = capi.FriProver(c, F128, 1, 4, 4, 3, 3)
        pr.begin(ev)
        c.set_hasher(capi.RPJIVE64_256)
        with pytest.raises(capi.WfError) as e:
            pr.commit_layer()
        assert e.value.code == -10
        with pytest.raises(capi.WfError) as e:
            pr.set_remainder(64)
        assert e.value.code == -10
        assert c.hasher == capi.RPJIVE64_256 and c.digest_bytes == 32
        # f64 on the same context is served, and BLAKE3 afterwards is what it was
        r64 = rand_f64(rng, 8 * 4).reshape(8, 4)
        assert np.array_equal(c.hash_rows(F64, r64, 8, 4), R.hash_rows(r64))
        c.set_hasher(capi.BLAKE3)
        root = pr.commit_layer()           # the same prover goes on under BLAKE3: the refusals left it as it was
        b = capi.FriProver(c, F128, 1, 4, 4, 3, 3)
        b.begin(ev)
        assert b.commit_layer() == root
        b.close()
        pr.close()
        want = orc.build_trace_commitment(F128, [cols], 1, logR, logB, 3)
        got = c.trace_commit(capi.make_params(F128, 1, logR, logB, n_cols, 1), cols)
        assert got["root"] == want["root"] and np.array_equal(got["nodes"], want["nodes"])
    finally:
        c.close()


def test_inconsistent_pairs_and_sharded_entry_points_are_refused(capi):
    import torch
    from starkpack_winterfell_amd.shard import Comm
    c = capi.Context(0)
    try:
        c.set_hasher(capi.RPJIVE64_256)
        with pytest.raises(capi.WfError) as e:
            c.set_digest_bytes(24)
        assert e.value.code == -31 and c.digest_bytes == 32
        rows = rand_f64(np.random.default_rng(1), 8 * 4).reshape(8, 4)
        assert np.array_equal(c.hash_rows(F64, rows, 8, 4), R.hash_rows(rows))   # unchanged: still RpJive64_256, 32 bytes
        for unknown in (17, 19):
            with pytest.raises(capi.WfError) as e:
                c.set_hasher(unknown)
            assert e.value.code == -31 and c.hasher == capi.RPJIVE64_256
        c.set_hasher(capi.BLAKE3)
        c.set_digest_bytes(24)
        with pytest.raises(capi.WfError) as e:
            c.set_hasher(capi.RPJIVE64_256)
        assert e.value.code == -31 and c.hasher == capi.BLAKE3
        assert c.hash_rows(F64, rows, 8, 4).shape == (8, 24)                      # unchanged: still Blake3_192
        c.set_digest_bytes(32)
        with pytest.raises(capi.WfError) as e:
            c.trace_commit(capi.make_params(F64, 1, 3, 1, 2, 1, digest_bytes=24, hasher=capi.RPJIVE64_256),
                           rand_cols(np.random.default_rng(3), F64, 2, 8))
        assert e.value.code == -31
        assert c.hasher == capi.BLAKE3 and c.digest_bytes == 32

        # the multi-GPU entry points: WF_ERR_ARG before any collective (a loopback communicator of world 1)
        logR, logB, n_cols = 3, 1, 2
        p = capi.make_params(F64, 1, logR, logB, n_cols, 1, hasher=capi.RPJIVE64_256)
        cols = rand_cols(np.random.default_rng(2), F64, n_cols, 1 << logR)
        comm = Comm.with_transport(c, 0, 1, *Loopback(1).collectives(0))
        with pytest.raises(capi.WfError) as e:
            comm.trace_commit_sharded_resident(p, cols)
        assert e.value.code == -19 and "BLAKE3" in str(e.value)
        dev = torch.device("cuda", 0)
        N, rw = 1 << (logR + logB), 8
        d_trace = torch.from_numpy(np.concatenate(cols).view(np.int64)).to(dev)
        d_polys = torch.empty_like(d_trace)
        d_lde = torch.empty(N * rw, dtype=torch.int64, device=dev)
        d_leaves, d_nodes, d_top = (torch.empty((N, 32), dtype=torch.uint8, device=dev) for _ in range(3))
        with pytest.raises(capi.WfError) as e:
            comm.trace_commit_sharded_dev(p, d_trace.data_ptr(), d_polys.data_ptr(), d_lde.data_ptr(), d_leaves.data_ptr(),
                                          d_nodes.data_ptr(), d_top.data_ptr())
        assert e.value.code == -19
        with pytest.raises(capi.WfError) as e:
            c.trace_commit_shard_dev(p, 0, 2, d_trace.data_ptr(), d_polys.data_ptr(), d_lde.data_ptr(), d_leaves.data_ptr())
        assert e.value.code == -19
        assert c.hasher == capi.BLAKE3 and c.digest_bytes == 32
        comm.close()
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------------------- graph
def test_commitment_replays_from_a_graph(capi, ctx):
    """The device-buffer commitment of 2^7 x 8, blowup 2, captured and replayed into poisoned buffers as
    tests/test_gpu_graph.py does for BLAKE3: the tree is a pure kernel sequence (nodes[0] is written by the launch that
    produces the root).  The eager run's leaves and tree are the reference's over the LDE it produced (767 permutations)."""
    import torch
    dev = torch.device("cuda", 0)
    logR, logB, n_cols = 7, 1, 8
    R_, N, rw = 1 << logR, 1 << (logR + logB), 8
    gen = torch.Generator(device=dev)
    gen.manual_seed(1008)
    trace = torch.randint(0, 2**62, (n_cols * R_,), dtype=torch.int64, device=dev, generator=gen)
    polys = torch.empty_like(trace)
    lde = torch.empty(N * rw, dtype=torch.int64, device=dev)
    leaves = torch.empty((N, 32), dtype=torch.uint8, device=dev)
    nodes = torch.empty((N, 32), dtype=torch.uint8, device=dev)
    p = capi.make_params(F64, 1, logR, logB, n_cols, 1, hasher=capi.RPJIVE64_256)
    s = torch.cuda.Stream(device=dev)

    def call(stream):
        ctx.trace_commit_dev(p, trace.data_ptr(), polys.data_ptr(), lde.data_ptr(), leaves.data_ptr(), nodes.data_ptr(), stream)

    with torch.cuda.stream(s):
        for _ in range(2):   # scratch buffers and tables exist before the capture
            call(s.cuda_stream)
        torch.cuda.synchronize()
    want = [t.clone() for t in (polys, lde, leaves, nodes)]
    h_leaves = R.combined_leaves([lde.cpu().numpy().view(np.uint64).reshape(N, rw)], n_cols)
    h_nodes = R.merkle_nodes(h_leaves)
    assert np.array_equal(leaves.cpu().numpy(), h_leaves)
    assert np.array_equal(nodes.cpu().numpy(), h_nodes)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for _ in range(3):
        for t in (polys, lde, leaves, nodes):
            t.fill_(-1 if t.dtype == torch.int64 else 255)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        for got, exp, name in zip((polys, lde, leaves, nodes), want, ("polys", "lde", "leaves", "nodes")):
            assert torch.equal(got, exp), name
    assert bytes(nodes.cpu().numpy()[1]) == bytes(h_nodes[1])
    for t in (polys, lde, leaves, nodes):
        t.fill_(-1 if t.dtype == torch.int64 else 255)
    call(0)
    torch.cuda.synchronize()
    assert torch.equal(nodes, want[3]) and torch.equal(lde, want[1])
