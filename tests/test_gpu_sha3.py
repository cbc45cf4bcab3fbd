"""GPU: Sha3_256 as the second hasher (enum wf_hasher) -- row hashing, Merkle trees, commitments in every single-GPU form,
queries, FRI -- bit for bit against hashlib.sha3_256 (tests/sha3_util.py); polynomials and LDE values against the oracle.
The BLAKE3 twin of every commitment, made on the same context before and after, still equals the oracle's: the hasher
travels in wf_params and does not leak between calls."""
import hashlib

import numpy as np
import pytest

import sha3_util as S
from conftest import rand_cols, rand_f64, rand_f128
from loopback import Loopback

pytestmark = pytest.mark.gpu
F64, F128 = 1, 2


def _offset(field):
    return 7 if field == F64 else 3


@pytest.fixture(scope="module")
def sctx(capi):
    """A context of its own whose hasher is Sha3_256 (the session's `ctx` stays on BLAKE3)."""
    c = capi.Context(0)
    c.set_hasher(capi.SHA3_256)
    yield c
    c.close()


def _rows(rng, field, n_rows, row_elems):
    if field == F64:
        return rand_f64(rng, n_rows * row_elems).reshape(n_rows, row_elems)
    return rand_f128(rng, n_rows * row_elems).reshape(n_rows, row_elems, 2)


# ---------------------------------------------------------------------------------------------------------- hash_rows
# one rate block is 136 bytes = 17 f64 elements = 8.5 f128 elements: 120..144 bytes around one block, 264..280 around two,
# 136 and 272 exactly (a further block holds only the padding); the 9th f128 element straddles lane 16 / lane 0
@pytest.mark.parametrize("field,row_elems", [(F64, e) for e in (1, 8, 15, 16, 17, 18, 33, 34, 35, 255)] +
                         [(F128, e) for e in (1, 8, 9, 17, 255)])
def test_hash_rows(sctx, field, row_elems):
    rng = np.random.default_rng(1000 * field + row_elems)
    rows = _rows(rng, field, 64, row_elems)
    got = sctx.hash_rows(field, rows, 64, row_elems)
    assert np.array_equal(got, S.hash_rows(field, rows))


# ---------------------------------------------------------------------------------------------------------- combined rows
@pytest.mark.parametrize("field,logR,logB,n_traces,n_cols", [
    (F64, 4, 2, 3, 5),    # 120 bytes: just inside one block; padding lanes of every trace's row skipped
    (F64, 4, 2, 3, 6),    # 144 bytes: one lane into the second block
    (F128, 4, 1, 2, 5),   # 160 bytes
])
def test_combined_rows_of_several_traces(capi, ctx, orc, field, logR, logB, n_traces, n_cols):
    rng = np.random.default_rng(logR * 10 + n_cols + field)
    traces = [rand_cols(rng, field, n_cols, 1 << logR) for _ in range(n_traces)]
    want = orc.build_trace_commitment(field, traces, 1, logR, logB, _offset(field))
    p = capi.make_params(field, 1, logR, logB, n_cols, n_traces, hasher=capi.SHA3_256)
    got = ctx.trace_commit(p, [c for t in traces for c in t])
    for t in range(n_traces):
        assert np.array_equal(got["lde"][t], want["lde"][t])
    leaves = S.combined_leaves(field, want["lde"], n_cols)
    nodes = S.merkle_nodes(leaves)
    assert np.array_equal(got["leaves"], leaves)
    assert np.array_equal(got["nodes"], nodes)
    assert got["root"] == bytes(nodes[1])


# ---------------------------------------------------------------------------------------------------------- merkle_build
# The switches of the Sha3 tree (MERKLE_PLAN_SHA3, csrc/merkle_plan.hpp; the same level switch as BLAKE3's one-lane-per-node rule):
#   a level of >= 2^15 parents (>= 2^16 children) is one k_merkle_level<k3::Merge> launch: 2^15 leaves below, 2^16 at, 2^17 above;
#   below that k_merkle_subtree<k3::Merge> folds up to 9 levels per launch: 2^8 (partial work-group, one launch), 2^9 (exactly
#   nine levels, one launch), 2^10 (nine levels + a second launch of one level);
#   2 and 4 leaves: a work-group of one and two active lanes.
@pytest.mark.parametrize("log_n", [1, 2, 8, 9, 10, 15, 16, 17])
def test_merkle_build_dev(sctx, log_n):
    import torch
    n = 1 << log_n
    rng = np.random.default_rng(log_n)
    leaves = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    want = S.merkle_nodes(leaves)
    dev = torch.device("cuda", 0)
    d_leaves = torch.from_numpy(leaves).to(dev)
    d_nodes = torch.full((n, 32), 0xA5, dtype=torch.uint8, device=dev)  # poisoned: every node must be written, [0] with zeros
    torch.cuda.synchronize()
    sctx.merkle_build_dev(d_leaves.data_ptr(), n, d_nodes.data_ptr())
    sctx.synchronize()
    got = d_nodes.cpu().numpy()
    assert not got[0].any()
    assert np.array_equal(got, want)
    if log_n <= 2:  # the host-buffer form
        assert np.array_equal(sctx.merkle_build(leaves), want)


# ---------------------------------------------------------------------------------------------------------- commitments
def _expect(orc, field, cols, logR, logB, n_cols):
    want = orc.build_trace_commitment(field, [cols], 1, logR, logB, _offset(field))
    leaves = S.combined_leaves(field, want["lde"], n_cols)
    return want, leaves, S.merkle_nodes(leaves)


def _blake3_root(capi, ctx, field, logR, logB, n_cols, cols):
    return ctx.trace_commit(capi.make_params(field, 1, logR, logB, n_cols, 1), cols, want_lde=False, want_polys=False)["root"]


def test_small_commitment_in_every_form(capi, ctx, orc):
    """f64 2^5 x 3, blowup 4: host form, device-buffer form, resident, resident asynchronous."""
    import torch
    field, logR, logB, n_cols = F64, 5, 2, 3
    rng = np.random.default_rng(53)
    cols = rand_cols(rng, field, n_cols, 1 << logR)
    want, leaves, nodes = _expect(orc, field, cols, logR, logB, n_cols)
    p = capi.make_params(field, 1, logR, logB, n_cols, 1, hasher=capi.SHA3_256)
    assert _blake3_root(capi, ctx, field, logR, logB, n_cols, cols) == want["root"]

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
    assert com.root() == bytes(nodes[1])
    assert np.array_equal(com.read_lde(0, 0, N), want["lde"][0])
    com.close()

    com = ctx.trace_commit_resident_async(p, cols)
    com.wait()
    assert com.root() == bytes(nodes[1])
    assert np.array_equal(com.read_lde(0, 0, N), want["lde"][0])
    com.close()

    assert _blake3_root(capi, ctx, field, logR, logB, n_cols, cols) == want["root"]


@pytest.mark.parametrize("field,logR,logB,n_cols", [
    (F64, 11, 3, 8),     # a two-pass plan whose BLAKE3 twin hashes its leaves inside the last pass
    (F128, 10, 3, 10),   # three segments, the last one half full: the tail-pack shape -- Sha3 takes the unfused route
])
def test_commitment_takes_the_unfused_route(capi, ctx, orc, field, logR, logB, n_cols):
    rng = np.random.default_rng(logR + n_cols)
    cols = rand_cols(rng, field, n_cols, 1 << logR)
    want, leaves, nodes = _expect(orc, field, cols, logR, logB, n_cols)
    assert _blake3_root(capi, ctx, field, logR, logB, n_cols, cols) == want["root"]
    got = ctx.trace_commit(capi.make_params(field, 1, logR, logB, n_cols, 1, hasher=capi.SHA3_256), cols)
    for c in range(n_cols):
        assert np.array_equal(got["polys"][c], want["polys"][0][c])
    assert np.array_equal(got["lde"][0], want["lde"][0])
    assert np.array_equal(got["leaves"], leaves) and np.array_equal(got["nodes"], nodes) and got["root"] == bytes(nodes[1])
    assert _blake3_root(capi, ctx, field, logR, logB, n_cols, cols) == want["root"]


def test_constraint_commitment_ext2(capi, ctx, orc):
    """Composition columns over the quadratic extension: host form (padded rows) and resident form (dense rows)."""
    field, ext, logR, logB, n_cols = F64, 2, 6, 2, 2
    rng = np.random.default_rng(62)
    cols = rand_cols(rng, field, n_cols, (1 << logR) * ext)
    want = orc.build_constraint_commitment(field, cols, ext, logR, logB, 7)
    leaves = S.combined_leaves(field, [want["lde"]], n_cols * ext)
    nodes = S.merkle_nodes(leaves)
    pb = capi.make_params(field, ext, logR, logB, n_cols, 1)
    p = capi.make_params(field, ext, logR, logB, n_cols, 1, hasher=capi.SHA3_256)
    assert ctx.constraint_commit(pb, cols)["root"] == want["root"]
    got = ctx.constraint_commit(p, cols)
    assert np.array_equal(got["lde"], want["lde"])
    assert np.array_equal(got["leaves"], leaves) and np.array_equal(got["nodes"], nodes) and got["root"] == bytes(nodes[1])
    com = ctx.constraint_commit_resident(p, cols)
    assert com.root() == bytes(nodes[1])
    pos = np.array([0, (1 << (logR + logB)) - 1, 17], dtype=np.uint64)
    rows, (q_leaves, q_nodes, depth) = com.query(pos)
    assert np.array_equal(rows, want["lde"][pos.astype(np.int64), :n_cols * ext])
    assert q_leaves == [bytes(leaves[int(i)]) for i in pos]
    assert S.verify_batch(bytes(nodes[1]), [int(i) for i in pos], q_leaves, q_nodes, depth)
    com.close()
    assert ctx.constraint_commit(pb, cols)["root"] == want["root"]


def test_pipelined_upload_of_a_resident_commitment(capi, orc, monkeypatch):
    """Host columns of a multi-segment, multi-pass matrix go up under the kernels (trace_commit_pipelined: the strided passes
    segment by segment, then the last pass and the hashing); the threshold switch sends this small shape there."""
    field, logR, logB, n_cols = F64, 11, 1, 9
    assert len(capi.plan_digits(field, logR, 2)) >= 2
    monkeypatch.setenv("WF_EXP_ENABLE", "1")
    monkeypatch.setenv("WF_EXP_PIPELINE_MIN_BYTES", "0")
    c = capi.Context(0)   # (the switches are read when a context is created)
    try:
        rng = np.random.default_rng(119)
        cols = rand_cols(rng, field, n_cols, 1 << logR)
        want, leaves, nodes = _expect(orc, field, cols, logR, logB, n_cols)
        com, polys = c.trace_commit_resident(capi.make_params(field, 1, logR, logB, n_cols, 1, hasher=capi.SHA3_256), cols,
                                             want_polys=True)
        assert com.root() == bytes(nodes[1])
        for k in range(n_cols):
            assert np.array_equal(polys[k], want["polys"][0][k])
        assert np.array_equal(com.read_lde(0, 0, 1 << (logR + logB)), want["lde"][0])
        pos = np.array([0, (1 << (logR + logB)) - 1, 1000], dtype=np.uint64)
        q_leaves, q_nodes, depth = com.prove_batch(pos)
        assert q_leaves == [bytes(leaves[int(i)]) for i in pos]
        assert S.verify_batch(bytes(nodes[1]), [int(i) for i in pos], q_leaves, q_nodes, depth)
        com.close()
        com, _ = c.trace_commit_resident(capi.make_params(field, 1, logR, logB, n_cols, 1), cols)
        assert com.root() == want["root"]
        com.close()
    finally:
        c.close()


def test_constraint_commit_from_evaluations(capi, ctx, orc):
    """The constraint side from the combined evaluations on (two packed tables, quadratic extension) with Sha3 leaves."""
    field, ext, logR, log_ce_blowup, n_cols, logB = F64, 2, 6, 2, 3, 2
    rng = np.random.default_rng(631)
    tables = [rand_cols(rng, field, 1, (1 << (logR + log_ce_blowup)) * ext)[0] for _ in range(2)]
    fc = rand_f64(rng, ext)
    want_cols = orc.composition_poly_from_evaluations(field, ext, tables, logR, n_cols, 7, fc)
    want = orc.build_constraint_commitment(field, want_cols, ext, logR, logB, 7)
    nodes = S.merkle_nodes(S.combined_leaves(field, [want["lde"]], n_cols * ext))
    com, polys = ctx.constraint_commit_from_evaluations(capi.make_params(field, ext, logR, logB, n_cols, 1, hasher=capi.SHA3_256),
                                                        tables, fc, want_polys=True)
    assert com.root() == bytes(nodes[1])
    for k in range(n_cols):
        assert np.array_equal(polys[k], want_cols[k])
    com.close()
    com, _ = ctx.constraint_commit_from_evaluations(capi.make_params(field, ext, logR, logB, n_cols, 1), tables, fc)
    assert com.root() == want["root"]
    com.close()


# ---------------------------------------------------------------------------------------------------------- queries
def test_queries_on_a_resident_commitment(capi, ctx, orc):
    field, logR, logB, n_cols, n_traces = F64, 5, 2, 3, 2
    rng = np.random.default_rng(77)
    traces = [rand_cols(rng, field, n_cols, 1 << logR) for _ in range(n_traces)]
    want = orc.build_trace_commitment(field, traces, 1, logR, logB, 7)
    leaves = S.combined_leaves(field, want["lde"], n_cols)
    nodes = S.merkle_nodes(leaves)
    root = bytes(nodes[1])
    N = 1 << (logR + logB)
    p = capi.make_params(field, 1, logR, logB, n_cols, n_traces, hasher=capi.SHA3_256)
    com, _ = ctx.trace_commit_resident(p, [c for t in traces for c in t])
    assert com.root() == root
    pos = np.array([0, N - 1, 5, 64, 65, 31], dtype=np.uint64)
    rows, (q_leaves, q_nodes, depth) = com.query(pos)
    assert depth == logR + logB
    for i, j in enumerate(pos):
        assert np.array_equal(rows[i], np.concatenate([want["lde"][t][int(j), :n_cols] for t in range(n_traces)]))
        assert q_leaves[i] == hashlib.sha3_256(S.row_bytes(field, rows[i])).digest()   # the returned rows re-hashed
    assert S.verify_batch(root, [int(j) for j in pos], q_leaves, q_nodes, depth)
    b_leaves, b_nodes, b_depth = com.prove_batch(pos)
    assert (b_leaves, b_nodes, b_depth) == (q_leaves, q_nodes, depth)
    w_leaves, w_nodes, w_depth = orc.merkle_prove_batch(nodes, leaves, [int(j) for j in pos])
    assert (b_leaves, b_nodes, b_depth) == (w_leaves, w_nodes, w_depth)
    bad = [list(v) for v in q_nodes]
    bad[0][-1] = bytes(32)
    assert not S.verify_batch(root, [int(j) for j in pos], q_leaves, bad, depth)       # (the check can fail)
    for j in (0, N - 1, 37):
        path = com.prove(j)
        assert len(path) == depth + 1 and path[0] == bytes(leaves[j])
        assert S.verify_path(root, j, path)
    com.close()


# ---------------------------------------------------------------------------------------------------------- FRI
def test_fri_layer_commit(ctx, sctx):
    field, ext, n, folding = F64, 2, 1 << 8, 4
    rng = np.random.default_rng(8)
    ev = rand_f64(rng, n * ext)
    blake = ctx.fri_layer_commit(field, ext, ev, folding)
    got = sctx.fri_layer_commit(field, ext, ev, folding)
    assert np.array_equal(got["transposed"], blake["transposed"])
    leaves = S.hash_rows(field, got["transposed"].reshape(n // folding, folding * ext))
    nodes = S.merkle_nodes(leaves)
    assert np.array_equal(got["leaves"], leaves) and np.array_equal(got["nodes"], nodes) and got["root"] == bytes(nodes[1])
    assert got["root"] != blake["root"]


@pytest.mark.parametrize("folding", [4, 2])
def test_fri_prover(capi, ctx, sctx, folding):
    """The same proof driven with the same caller-supplied alphas on a BLAKE3 and on a Sha3 context: every layer's rows are
    equal, every Sha3 layer root is the hashlib tree over those rows, the remainder digest is sha3_256 of its canonical bytes."""
    field, ext, blowup, max_rem, n = F64, 2, 4, 3, 1 << 8
    rng = np.random.default_rng(folding)
    ev = rand_f64(rng, n * ext)
    n_layers = capi.fri_num_layers(folding, blowup, max_rem, n)
    assert n_layers >= 2
    alphas = [rand_f64(rng, ext) for _ in range(n_layers)]
    provers = [capi.FriProver(c, field, ext, folding, blowup, max_rem, 7) for c in (ctx, sctx)]
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
        nodes = S.merkle_nodes(S.hash_rows(field, rows))
        assert roots[1][i] == bytes(nodes[1]) == ls.root()
        assert roots[1][i] != roots[0][i]
        pos = np.array([0, size - 1], dtype=np.uint64)
        q_leaves, q_nodes, depth = ls.prove_batch(pos)
        assert S.verify_batch(bytes(nodes[1]), [0, size - 1], q_leaves, q_nodes, depth)
    rem_b, _ = provers[0].set_remainder(size)
    rem_s, digest = provers[1].set_remainder(size)
    assert np.array_equal(rem_b, rem_s)
    assert digest == hashlib.sha3_256(S.row_bytes(field, rem_s.reshape(-1))).digest()
    for pr in provers:
        pr.close()


# ---------------------------------------------------------------------------------------------------------- refusals
def test_inconsistent_pairs_and_sharded_entry_points_are_refused(capi):
    import torch
    from starkpack_winterfell_amd.shard import Comm
    c = capi.Context(0)
    try:
        c.set_hasher(capi.SHA3_256)
        with pytest.raises(capi.WfError) as e:
            c.set_digest_bytes(24)
        assert e.value.code == -31 and c.digest_bytes == 32
        rows = rand_f64(np.random.default_rng(1), 8 * 4).reshape(8, 4)
        assert np.array_equal(c.hash_rows(F64, rows, 8, 4), S.hash_rows(F64, rows))   # unchanged: still Sha3, 32 bytes
        with pytest.raises(capi.WfError) as e:
            c.set_hasher(2)
        assert e.value.code == -31 and c.hasher == capi.SHA3_256
        c.set_hasher(capi.BLAKE3)
        c.set_digest_bytes(24)
        with pytest.raises(capi.WfError) as e:
            c.set_hasher(capi.SHA3_256)
        assert e.value.code == -31 and c.hasher == capi.BLAKE3
        assert c.hash_rows(F64, rows, 8, 4).shape == (8, 24)                            # unchanged: still Blake3_192
        c.set_digest_bytes(32)

        # the multi-GPU entry points: WF_ERR_ARG before any collective (a loopback communicator of world 1)
        logR, logB, n_cols = 3, 1, 2
        p = capi.make_params(F64, 1, logR, logB, n_cols, 1, hasher=capi.SHA3_256)
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
        comm.close()
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------------------- graph
def test_commitment_replays_from_a_graph(capi, ctx):
    """The Sha3 device-buffer commitment of 2^10 x 8 captured and replayed as tests/test_gpu_graph.py does for BLAKE3: the
    tree is a pure kernel sequence (nodes[0] is written by the launch that produces the root)."""
    import torch
    dev = torch.device("cuda", 0)
    logR, logB, n_cols = 10, 3, 8
    R, N, rw = 1 << logR, 1 << (logR + logB), 8
    gen = torch.Generator(device=dev)
    gen.manual_seed(1008)
    trace = torch.randint(0, 2**62, (n_cols * R,), dtype=torch.int64, device=dev, generator=gen)
    polys = torch.empty_like(trace)
    lde = torch.empty(N * rw, dtype=torch.int64, device=dev)
    leaves = torch.empty((N, 32), dtype=torch.uint8, device=dev)
    nodes = torch.empty((N, 32), dtype=torch.uint8, device=dev)
    p = capi.make_params(F64, 1, logR, logB, n_cols, 1, hasher=capi.SHA3_256)
    s = torch.cuda.Stream(device=dev)

    def call(stream):
        ctx.trace_commit_dev(p, trace.data_ptr(), polys.data_ptr(), lde.data_ptr(), leaves.data_ptr(), nodes.data_ptr(), stream)

    with torch.cuda.stream(s):
        for _ in range(2):   # scratch buffers and tables exist before the capture
            call(s.cuda_stream)
        torch.cuda.synchronize()
    want = [t.clone() for t in (polys, lde, leaves, nodes)]
    # the direct call itself is right: leaves and tree from hashlib over the LDE it produced
    h_leaves = S.combined_leaves(F64, [lde.cpu().numpy().view(np.uint64).reshape(N, rw)], n_cols)
    assert np.array_equal(leaves.cpu().numpy(), h_leaves)
    assert np.array_equal(nodes.cpu().numpy(), S.merkle_nodes(h_leaves))
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
    for t in (polys, lde, leaves, nodes):
        t.fill_(-1 if t.dtype == torch.int64 else 255)
    call(0)
    torch.cuda.synchronize()
    assert torch.equal(nodes, want[3]) and torch.equal(lde, want[1])
