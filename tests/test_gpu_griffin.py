"""GPU: GriffinJive64_256 (Griffin of width 8 with the Jive compression) as hasher 20 (enum wf_hasher) -- row hashing, Merkle
trees, commitments, queries, FRI and the refusals -- bit for bit against the two references of tests/griffin_util.py: the
function on Python integers (at most 2048 permutations per test) and the plain C reference tests/cpp/griffin_ref.c (at most
2^18 per test; pinned to the Python one by tests/test_griffin_host.py).  Both budgets are asserted by counting.  Polynomials
and LDE values come from the oracle.  Buffers are poisoned behind their last element; digests are asserted canonical; nothing
is sampled."""
import numpy as np
import pytest

import edge_util as E
import griffin_edge_util as D
import griffin_util as G
from conftest import rand_cols, rand_f64, rand_f128
from loopback import Loopback

pytestmark = pytest.mark.gpu
F64, F128 = 1, 2
P = G.P
PY_BUDGET, C_BUDGET = 2048, 1 << 18
SWITCH = 17   # log2 leaves of the smallest tree whose first level runs in k_merkle_level (MERKLE_PLAN_GRIFFIN.level_min_log + 1)


@pytest.fixture(scope="module")
def cref():
    return G.CRef()


@pytest.fixture(autouse=True)
def _budgets(cref):
    before = G.PERMUTATIONS
    cref.spent = 0
    yield
    assert G.PERMUTATIONS - before <= PY_BUDGET, f"{G.PERMUTATIONS - before} Python permutations in one test"
    assert cref.spent <= C_BUDGET, f"{cref.spent} C-reference permutations in one test"


@pytest.fixture(scope="module")
def gctx(capi):
    """A context of its own whose hasher is GriffinJive64_256 (the session's `ctx` stays on BLAKE3)."""
    c = capi.Context(0)
    c.set_hasher(capi.GRIFFINJIVE64_256)
    yield c
    c.close()


def _canonical(digests):
    return bool((np.ascontiguousarray(digests).view(np.uint64) < np.uint64(P)).all())


def _hash_rows(capi, c, rows, tail=5):
    """wf_hash_rows into a buffer with `tail` poisoned digests behind the last row: they must stay as they were."""
    a = np.ascontiguousarray(rows, dtype=np.uint64)
    n, k = a.shape
    out = np.full((n + tail, 32), 0xA5, dtype=np.uint8)
    rc = capi.load().wf_hash_rows(c._h, F64, a.ctypes.data, n, k, out.ctypes.data)
    assert rc == 0, capi.load().wf_last_error()
    assert (out[n:] == 0xA5).all(), "hash_rows wrote behind its last digest"
    assert _canonical(out[:n])
    return out[:n]


# ---------------------------------------------------------------------------------------------------------- hash_rows
# one rate block is 4 elements: 3, 4, 5 around one block, 7, 8, 9 around two, 12 and 13 around three; 70 rows are a wave and a
# partial one
@pytest.mark.parametrize("row_elems", [1, 3, 4, 5, 7, 8, 9, 12, 13])
def test_hash_rows(capi, gctx, cref, row_elems):
    rng = np.random.default_rng(row_elems)
    rows = rand_f64(rng, 70 * row_elems).reshape(70, row_elems)
    rows[0, :] = 0                                   # canonical 0
    rows[1, :] = np.uint64(P - 1)                    # the largest residue: every addition into the rate wraps or lands in [p, 2^64)
    got = _hash_rows(capi, gctx, rows)
    assert np.array_equal(got, G.hash_rows(rows))
    assert np.array_equal(got, cref.hash_rows(rows))
    assert np.array_equal(gctx.hash_rows(F64, rows, 70, row_elems), got)


def test_hash_rows_of_255_elements(capi, gctx, cref):
    """70 rows of 255 elements (64 permutations each, the last block one element short): every row against the C reference,
    the first 20 against Python as well."""
    rows = rand_f64(np.random.default_rng(255), 70 * 255).reshape(70, 255)
    got = _hash_rows(capi, gctx, rows)
    assert np.array_equal(got, cref.hash_rows(rows))
    assert np.array_equal(got[:20], G.hash_rows(rows[:20]))


@pytest.mark.parametrize("kind", ["zero", "pm1", "alt", "alphabet"])
@pytest.mark.parametrize("row_elems", [5, 8])
def test_hash_rows_of_carry_edge_patterns(capi, gctx, kind, row_elems):
    """The carry-edge patterns of tests/edge_util.py: all-zero rows, rows of p - 1, rows alternating between the two, and rows
    drawn from the limb alphabet (70 rows: a wave and a partial one)."""
    rng = np.random.default_rng(row_elems)
    rows = np.stack([E.pattern_column(rng, F64, kind, 70) for _ in range(row_elems)], axis=1)
    assert np.array_equal(_hash_rows(capi, gctx, rows), G.hash_rows(rows))


def test_hash_rows_directed(capi, gctx, cref):
    """Rows of one rate block (and of one element more) whose first non-linear layer meets every (i, case) of gfj::linear a
    row can reach -- i = 2, 3, 4 -- among uniform rows, ending in a partial wave."""
    ins = D.row_states()
    assert sorted(ins) == sorted(D.reachable("row")) and {i for i, _ in ins} == {2, 3, 4}
    for extra in (0, 1):
        directed = np.array([D.stored(ins[rc] + [11] * extra) for rc in D.reachable("row")], dtype=np.uint64)
        rng = np.random.default_rng(5 + extra)
        k = 4 + extra
        rows = np.concatenate([directed, rand_f64(rng, 41 * k).reshape(41, k)])
        rows = np.ascontiguousarray(rows[rng.permutation(rows.shape[0])])
        assert rows.shape[0] % 64 != 0
        got = _hash_rows(capi, gctx, rows)
        want = G.hash_rows(rows)
        assert np.array_equal(want, cref.hash_rows(rows))
        assert np.array_equal(got, want)


@pytest.mark.parametrize("ext,folding", [(2, 2), (3, 2), (3, 4)])
def test_rows_of_extension_elements_count_base_elements(gctx, ctx, ext, folding):
    """A FRI layer's rows are `folding` extension elements: hash_elements flattens them, so the sponge sees folding * ext base
    elements -- 4, 6 and 12 here: state[4] is 0, 1 and 0."""
    n = 1 << 6
    ev = rand_f64(np.random.default_rng(10 * ext + folding), n * ext)
    got = gctx.fri_layer_commit(F64, ext, ev, folding)
    assert np.array_equal(got["transposed"], ctx.fri_layer_commit(F64, ext, ev, folding)["transposed"])
    leaves = G.hash_rows(got["transposed"].reshape(n // folding, folding * ext))
    assert np.array_equal(got["leaves"], leaves)
    nodes = G.merkle_nodes(leaves)
    assert np.array_equal(got["nodes"], nodes) and got["root"] == bytes(nodes[1])


def test_combined_rows_of_two_traces(capi, ctx, orc):
    """n_traces = 2: the leaf is hash_elements over trace 0's columns, then trace 1's; the padding lanes of the stored rows (3
    of 8 used) are neither counted nor absorbed."""
    logR, logB, n_cols, n_traces = 3, 1, 3, 2
    rng = np.random.default_rng(203)
    traces = [rand_cols(rng, F64, n_cols, 1 << logR) for _ in range(n_traces)]
    want = orc.build_trace_commitment(F64, traces, 1, logR, logB, 7)
    p = capi.make_params(F64, 1, logR, logB, n_cols, n_traces, hasher=capi.GRIFFINJIVE64_256)
    got = ctx.trace_commit(p, [c for t in traces for c in t])
    for t in range(n_traces):
        assert np.array_equal(got["lde"][t], want["lde"][t])
    N = 1 << (logR + logB)
    leaves = np.array([np.frombuffer(G.digest_bytes(G.hash_elements(G.combined_row(want["lde"], n_cols, j))), dtype=np.uint8)
                       for j in range(N)])
    nodes = G.merkle_nodes(leaves)
    assert np.array_equal(got["leaves"], leaves) and np.array_equal(got["nodes"], nodes) and got["root"] == bytes(nodes[1])


# ---------------------------------------------------------------------------------------------------------- merkle_build_dev
def _leaves(log_n):
    """Random u64 words, the words at and above p in the first and the last leaf (read as BaseElement::new reads them)."""
    n = 1 << log_n
    rng = np.random.default_rng(log_n)
    leaves = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)
    edge = np.array([P, P + 1, 2**64 - 1, 2**64 - 2**32], dtype=np.uint64)
    leaves[0] = edge
    leaves[n - 1] = edge[::-1]
    if n > 2:
        leaves[1, 2] = np.uint64(P)
    return leaves.view(np.uint8).reshape(n, 32)


def _build_dev(c, leaves, tail=7):
    """wf_merkle_build_dev into a node buffer poisoned throughout, with `tail` digests behind the last node that must stay."""
    import torch
    n = leaves.shape[0]
    dev = torch.device("cuda", 0)
    d_leaves = torch.from_numpy(leaves).to(dev)
    d_nodes = torch.full((n + tail, 32), 0xA5, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    c.merkle_build_dev(d_leaves.data_ptr(), n, d_nodes.data_ptr())
    c.synchronize()
    got = d_nodes.cpu().numpy()
    assert (got[n:] == 0xA5).all(), "the tree wrote behind its last node"
    assert not got[0].any() and _canonical(got[:n])
    return got[:n]


@pytest.mark.parametrize("log_n", list(range(1, 12)))
def test_merkle_build_against_python(gctx, cref, log_n):
    """Every node of every size 2^1 .. 2^11 (2^10 and 2^11 leaves take two sub-tree launches), against both references."""
    leaves = _leaves(log_n)
    got = _build_dev(gctx, leaves)
    assert np.array_equal(got, G.merkle_nodes(leaves))
    assert np.array_equal(got, cref.merkle_nodes(leaves))


@pytest.mark.parametrize("at", [-1, 0, 1])
def test_merkle_build_around_the_switch(gctx, cref, at):
    """One size below the level / sub-tree switch (sub-tree launches only), the size at it (one lane-per-parent launch) and one
    above (two of them): every node against the C reference."""
    leaves = _leaves(SWITCH + at)
    want = cref.merkle_nodes(leaves)
    got = _build_dev(gctx, leaves)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"{bad.size} nodes differ, the first at {bad[:8].tolist()}"


def _directed_pairs(part):
    """64 pairs of leaves whose merge meets a directed case of gfj::linear in its first non-linear layer.  A merge reaches every
    i = 2..7, 81 (i, case) pairs in all: part 0 holds the first 64 of them, part 1 the other 17 and a second draw of 47."""
    first, more = D.merge_states(0), D.merge_states(1)
    order = D.reachable("merge")
    assert sorted(first) == sorted(order) and {i for i, _ in first} == set(range(2, 8)) and len(order) == 81
    pairs = ([first[rc] for rc in order] + [more[rc] for rc in order])[64 * part:64 * part + 64]
    assert len(pairs) == 64 and all(len(p) == 8 and max(p) < P for p in pairs)
    return np.array(pairs, dtype=np.uint64).reshape(128, 4).view(np.uint8).reshape(128, 32)


@pytest.mark.parametrize("part", [0, 1])
def test_merkle_subtree_on_directed_pairs(gctx, cref, part):
    """2^7 leaves, every pair a directed one: the bottom level runs in k_merkle_subtree<gfj::Merge>."""
    leaves = _directed_pairs(part)
    want = G.merkle_nodes(leaves)
    assert np.array_equal(want, cref.merkle_nodes(leaves))
    assert np.array_equal(_build_dev(gctx, leaves), want)


@pytest.mark.parametrize("part", [0, 1])
def test_merkle_level_on_directed_pairs(gctx, cref, part):
    """The switch-size tree whose first and last 64 leaves are the directed pairs: they go through k_merkle_level<gfj::Merge>."""
    leaves = _leaves(SWITCH).copy()
    d = _directed_pairs(part)
    leaves[:64] = d[:64]
    leaves[-64:] = d[64:]
    assert np.array_equal(_build_dev(gctx, leaves), cref.merkle_nodes(leaves))


def test_merge_is_not_hash_elements_of_the_same_words(capi, gctx):
    words = np.arange(11, 19, dtype=np.uint64)
    tree = _build_dev(gctx, words.view(np.uint8).reshape(2, 32))
    row = np.array([D.stored(words.tolist())], dtype=np.uint64)
    assert bytes(tree[1]) == G.digest_bytes(G.merge_words(words.tolist())) != bytes(_hash_rows(capi, gctx, row)[0])


# ---------------------------------------------------------------------------------------------------------- commitments
def _ref_commitment(cref, orc, ext, logR, logB, n_cols, n_traces, seed):
    rng = np.random.default_rng(seed)
    traces = [rand_cols(rng, F64, n_cols, (1 << logR) * ext) for _ in range(n_traces)]
    want = orc.build_trace_commitment(F64, traces, ext, logR, logB, 7, threads=8)
    epr = n_cols * ext
    rows = np.ascontiguousarray(np.hstack([m[:, :epr] for m in want["lde"]]))
    leaves = cref.hash_rows(rows)
    return traces, want, leaves, cref.merkle_nodes(leaves)


SHAPES = [(1, 12, 3, 8, 1), (1, 11, 2, 17, 2), (2, 11, 3, 3, 1), (3, 10, 3, 2, 1)]


@pytest.mark.parametrize("shape", SHAPES)
def test_trace_commit_dev_every_leaf_and_node(capi, orc, ctx, cref, shape):
    """wf_trace_commit_dev: 2^15 rows of 8; a multi-segment packed shape (two traces of 17 columns, 34 elements a row); a
    quadratic-extension one (6 base elements a row) and a cubic one (6 as well).  The oracle's LDE hashed with the C reference."""
    import torch
    ext, logR, logB, n_cols, n_traces = shape
    traces, want, leaves, nodes = _ref_commitment(cref, orc, ext, logR, logB, n_cols, n_traces, sum(shape))
    p = capi.make_params(F64, ext, logR, logB, n_cols, n_traces, hasher=capi.GRIFFINJIVE64_256)
    dev = torch.device("cuda", 0)
    N, rw = 1 << (logR + logB), orc.row_width(n_cols, ext)
    d_trace = torch.from_numpy(np.concatenate([col for t in traces for col in t]).view(np.int64)).to(dev)
    d_polys = torch.empty_like(d_trace)
    d_lde = torch.full((n_traces * N * rw,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device=dev)
    d_leaves = torch.full((N + 3, 32), 0xA5, dtype=torch.uint8, device=dev)
    d_nodes = torch.full((N + 3, 32), 0xA5, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ctx.trace_commit_dev(p, d_trace.data_ptr(), d_polys.data_ptr(), d_lde.data_ptr(), d_leaves.data_ptr(), d_nodes.data_ptr())
    ctx.synchronize()
    lde = d_lde.cpu().numpy().view(np.uint64).reshape(n_traces, N, rw)
    for t in range(n_traces):
        assert np.array_equal(lde[t][:, :n_cols * ext], want["lde"][t][:, :n_cols * ext])
    g_leaves, g_nodes = d_leaves.cpu().numpy(), d_nodes.cpu().numpy()
    assert (g_leaves[N:] == 0xA5).all() and (g_nodes[N:] == 0xA5).all()
    assert np.array_equal(g_leaves[:N], leaves), "leaves"
    assert np.array_equal(g_nodes[:N], nodes), "nodes"
    assert not g_nodes[0].any() and _canonical(g_leaves[:N]) and _canonical(g_nodes[:N])


def test_trace_commit_from_host_buffers(capi, orc, ctx, cref):
    """The first shape through the host-buffer form."""
    ext, logR, logB, n_cols, n_traces = SHAPES[0]
    traces, want, leaves, nodes = _ref_commitment(cref, orc, ext, logR, logB, n_cols, n_traces, sum(SHAPES[0]))
    got = ctx.trace_commit(capi.make_params(F64, ext, logR, logB, n_cols, n_traces, hasher=capi.GRIFFINJIVE64_256), traces[0])
    assert np.array_equal(got["lde"][0], want["lde"][0])
    assert np.array_equal(got["leaves"], leaves) and np.array_equal(got["nodes"], nodes) and got["root"] == bytes(nodes[1])


def test_resident_commitment_batch_query(capi, orc, ctx, cref):
    """The first shape resident: the root, and a batch query of 40 positions against proofs cut from the reference tree, each
    of them verified with the reference's merge."""
    ext, logR, logB, n_cols, n_traces = SHAPES[0]
    traces, want, leaves, nodes = _ref_commitment(cref, orc, ext, logR, logB, n_cols, n_traces, 24)
    N = 1 << (logR + logB)
    com, _ = ctx.trace_commit_resident(capi.make_params(F64, ext, logR, logB, n_cols, n_traces, hasher=capi.GRIFFINJIVE64_256), traces[0])
    try:
        assert com.root() == bytes(nodes[1])
        rng = np.random.default_rng(40)
        pos = [0, 1, N - 1, N - 2, N // 2 - 1, N // 2] + [int(x) for x in rng.choice(np.arange(2, N - 2), size=34, replace=False)]
        pos = list(dict.fromkeys(pos))[:40]
        assert len(pos) == 40
        rows, (q_leaves, q_nodes, depth) = com.query(np.array(pos, dtype=np.uint64))
        assert depth == logR + logB
        assert (q_leaves, q_nodes, depth) == orc.merkle_prove_batch(nodes, leaves, pos)
        for i, j in enumerate(pos):
            assert np.array_equal(rows[i], want["lde"][0][j, :n_cols])
            assert q_leaves[i] == bytes(leaves[j])
            assert G.verify_path(com.root(), j, G.cut_path(nodes, leaves, j), cref.merge)
    finally:
        com.close()


def test_commitment_replays_from_a_graph(capi, ctx, cref):
    """The device-buffer commitment of the first shape captured and replayed into poisoned buffers, as tests/test_gpu_graph.py
    does for BLAKE3: the tree is a pure kernel sequence (nodes[0] is written by the launch that produces the root)."""
    import torch
    dev = torch.device("cuda", 0)
    ext, logR, logB, n_cols, _ = SHAPES[0]
    R_, N, rw = 1 << logR, 1 << (logR + logB), 8
    gen = torch.Generator(device=dev)
    gen.manual_seed(1020)
    trace = torch.randint(0, 2**62, (n_cols * R_,), dtype=torch.int64, device=dev, generator=gen)
    polys = torch.empty_like(trace)
    lde = torch.empty(N * rw, dtype=torch.int64, device=dev)
    leaves = torch.empty((N, 32), dtype=torch.uint8, device=dev)
    nodes = torch.empty((N, 32), dtype=torch.uint8, device=dev)
    p = capi.make_params(F64, 1, logR, logB, n_cols, 1, hasher=capi.GRIFFINJIVE64_256)
    s = torch.cuda.Stream(device=dev)

    def call(stream):
        ctx.trace_commit_dev(p, trace.data_ptr(), polys.data_ptr(), lde.data_ptr(), leaves.data_ptr(), nodes.data_ptr(), stream)

    with torch.cuda.stream(s):
        for _ in range(2):   # scratch buffers and tables exist before the capture
            call(s.cuda_stream)
        torch.cuda.synchronize()
    want = [t.clone() for t in (polys, lde, leaves, nodes)]
    h_leaves = cref.hash_rows(lde.cpu().numpy().view(np.uint64).reshape(N, rw)[:, :n_cols])
    h_nodes = cref.merkle_nodes(h_leaves)
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


# ---------------------------------------------------------------------------------------------------------- FRI
@pytest.mark.parametrize("folding", [4, 2])
def test_fri_layer_commit(orc, gctx, cref, folding):
    """n = 2^12 evaluations of the quadratic extension: rows of folding * 2 base elements, every leaf and node."""
    ext, n = 2, 1 << 12
    ev = rand_f64(np.random.default_rng(12 + folding), n * ext)
    got = gctx.fri_layer_commit(F64, ext, ev, folding)
    tr = orc.transpose_slice(F64, ev, n, ext, folding)
    assert np.array_equal(got["transposed"], tr)
    leaves = cref.hash_rows(np.ascontiguousarray(tr.reshape(n // folding, folding * ext)))
    nodes = cref.merkle_nodes(leaves)
    assert np.array_equal(got["leaves"], leaves), "leaves"
    assert np.array_equal(got["nodes"], nodes), "nodes"
    assert got["root"] == bytes(nodes[1]) and _canonical(got["leaves"]) and _canonical(got["nodes"])


def test_fri_prover(capi, ctx, gctx, orc, cref):
    """The same proof driven with the same caller-supplied alphas on a BLAKE3 and on a GriffinJive64_256 context: every layer's
    rows are equal, every layer root is the reference tree over those rows, the remainder digest is hash_elements of the
    remainder's base elements."""
    field, ext, folding, blowup, max_rem, n = F64, 2, 4, 4, 3, 1 << 8
    rng = np.random.default_rng(folding)
    ev = rand_f64(rng, n * ext)
    n_layers = capi.fri_num_layers(folding, blowup, max_rem, n)
    assert n_layers >= 2
    alphas = [rand_f64(rng, ext) for _ in range(n_layers)]
    provers = [capi.FriProver(c, field, ext, folding, blowup, max_rem, 7) for c in (ctx, gctx)]
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
        leaves = cref.hash_rows(rows.reshape(size, folding * ext))
        nodes = cref.merkle_nodes(leaves)
        assert np.array_equal(nodes, G.merkle_nodes(leaves))
        assert roots[1][i] == bytes(nodes[1]) == ls.root()
        assert roots[1][i] != roots[0][i]
        assert ls.prove_batch(np.array([0, size - 1], dtype=np.uint64)) == orc.merkle_prove_batch(nodes, leaves, [0, size - 1])
    rem_b, _ = provers[0].set_remainder(size)
    rem_s, digest = provers[1].set_remainder(size)
    assert np.array_equal(rem_b, rem_s)
    assert digest == G.hash_row(rem_s.reshape(-1))
    for pr in provers:
        pr.close()


# ---------------------------------------------------------------------------------------------------------- refusals
def test_f128_is_refused_before_any_launch(capi, orc):
    """WF_FIELD_F128 under GriffinJive64_256: WF_ERR_FIELD (-10) before anything is launched, and nothing changes -- the
    BLAKE3 commitment made on the same context afterwards equals the oracle's."""
    import torch
    c = capi.Context(0)
    try:
        logR, logB, n_cols = 3, 1, 2
        rng = np.random.default_rng(128)
        cols = rand_cols(rng, F128, n_cols, 1 << logR)
        p = capi.make_params(F128, 1, logR, logB, n_cols, 1, hasher=capi.GRIFFINJIVE64_256)
        dev = torch.device("cuda", 0)
        N, rw = 1 << (logR + logB), 4
        d_trace = torch.from_numpy(np.concatenate(cols).view(np.int64).reshape(-1)).to(dev)
        d_polys = torch.empty_like(d_trace)
        d_lde = torch.empty(N * rw * 2, dtype=torch.int64, device=dev)
        d_leaves = torch.full((N, 32), 0xA5, dtype=torch.uint8, device=dev)
        d_nodes = torch.full((N, 32), 0xA5, dtype=torch.uint8, device=dev)
        calls = [
            lambda: c.trace_commit(p, cols),
            lambda: c.trace_commit_dev(p, d_trace.data_ptr(), d_polys.data_ptr(), d_lde.data_ptr(), d_leaves.data_ptr(),
                                       d_nodes.data_ptr()),
            lambda: c.trace_commit_resident(p, cols),
            lambda: c.constraint_commit(p, cols),
        ]
        for k, call in enumerate(calls):
            with pytest.raises(capi.WfError) as e:
                call()
            assert e.value.code == -10 and "GriffinJive64_256" in str(e.value), k
        torch.cuda.synchronize()
        assert (d_leaves.cpu().numpy() == 0xA5).all() and (d_nodes.cpu().numpy() == 0xA5).all()   # nothing was launched

        c.set_hasher(capi.GRIFFINJIVE64_256)   # the entry points that take the context's hasher
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
            assert e.value.code == -10 and "GriffinJive64_256" in str(e.value), k
            assert c.hasher == capi.GRIFFINJIVE64_256 and c.digest_bytes == 32
        r64 = rand_f64(rng, 8 * 4).reshape(8, 4)   # f64 on the same context is served, and BLAKE3 afterwards is what it was
        assert np.array_equal(c.hash_rows(F64, r64, 8, 4), G.hash_rows(r64))
        c.set_hasher(capi.BLAKE3)
        want = orc.build_trace_commitment(F128, [cols], 1, logR, logB, 3)
        got = c.trace_commit(capi.make_params(F128, 1, logR, logB, n_cols, 1), cols)
        assert got["root"] == want["root"] and np.array_equal(got["nodes"], want["nodes"])
    finally:
        c.close()


def test_inconsistent_pairs_unknown_ids_and_sharded_entry_points_are_refused(capi):
    import torch
    from starkpack_winterfell_amd.shard import Comm
    c = capi.Context(0)
    try:
        c.set_hasher(capi.GRIFFINJIVE64_256)
        with pytest.raises(capi.WfError) as e:
            c.set_digest_bytes(24)
        assert e.value.code == -31 and c.digest_bytes == 32
        rows = rand_f64(np.random.default_rng(1), 8 * 4).reshape(8, 4)
        assert np.array_equal(c.hash_rows(F64, rows, 8, 4), G.hash_rows(rows))   # unchanged: still GriffinJive64_256, 32 bytes
        for unknown in (17, 19, 21):
            with pytest.raises(capi.WfError) as e:
                c.set_hasher(unknown)
            assert e.value.code == -31 and c.hasher == capi.GRIFFINJIVE64_256
        assert np.array_equal(c.hash_rows(F64, rows, 8, 4), G.hash_rows(rows))
        c.set_hasher(capi.BLAKE3)
        c.set_digest_bytes(24)
        with pytest.raises(capi.WfError) as e:
            c.set_hasher(capi.GRIFFINJIVE64_256)
        assert e.value.code == -31 and c.hasher == capi.BLAKE3
        assert c.hash_rows(F64, rows, 8, 4).shape == (8, 24)                      # unchanged: still Blake3_192
        c.set_digest_bytes(32)
        with pytest.raises(capi.WfError) as e:
            c.trace_commit(capi.make_params(F64, 1, 3, 1, 2, 1, digest_bytes=24, hasher=capi.GRIFFINJIVE64_256),
                           rand_cols(np.random.default_rng(3), F64, 2, 8))
        assert e.value.code == -31
        assert c.hasher == capi.BLAKE3 and c.digest_bytes == 32

        # the multi-GPU entry points: WF_ERR_ARG before any collective (a loopback communicator of world 1)
        logR, logB, n_cols = 3, 1, 2
        p = capi.make_params(F64, 1, logR, logB, n_cols, 1, hasher=capi.GRIFFINJIVE64_256)
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
        d_leaves, d_nodes, d_top = (torch.full((N, 32), 0xA5, dtype=torch.uint8, device=dev) for _ in range(3))
        with pytest.raises(capi.WfError) as e:
            comm.trace_commit_sharded_dev(p, d_trace.data_ptr(), d_polys.data_ptr(), d_lde.data_ptr(), d_leaves.data_ptr(),
                                          d_nodes.data_ptr(), d_top.data_ptr())
        assert e.value.code == -19
        with pytest.raises(capi.WfError) as e:
            c.trace_commit_shard_dev(p, 0, 2, d_trace.data_ptr(), d_polys.data_ptr(), d_lde.data_ptr(), d_leaves.data_ptr())
        assert e.value.code == -19
        torch.cuda.synchronize()
        for t in (d_leaves, d_nodes, d_top):
            assert (t.cpu().numpy() == 0xA5).all()   # nothing was launched
        assert c.hasher == capi.BLAKE3 and c.digest_bytes == 32
        comm.close()
    finally:
        c.close()
