"""GPU: Rp64_256 and RpJive64_256 compared IN FULL -- every node, every leaf, every row digest -- with the plain C reference
of oracle/rescue_ref.c (orc.Rescue: canonical integers, 128-bit products reduced with %, square-and-multiply S-boxes; pinned
to the Python restatements by tests/test_oracle.py), at the sizes where the wide kernels first run and under the nonce
search's own window plan; and the directed operands of tests/rescue_edge_util.py for the closing addition of mds_row in
every product kernel that runs it.

The Python references of the other Rescue files cost milliseconds per permutation and keep those files to 2048 of them per
test; the C reference costs about 60 us (width 12) / 40 us (width 8) on one core and runs on up to 16, so a test here may
ask for about 2^19 permutations (`_budget`): a tree of n leaves is n - 1, a row of k elements ceil(k / rate).  A reference
nonce search may try 7 * 2^16 nonces and fails the test beyond that.  Every comparison is bit-exact; buffers are poisoned
behind the last element; every digest is asserted canonical."""
import hashlib

import numpy as np
import pytest

import rescue_edge_util as D
import rp64_util as RP
import rpjive_util as RJ
from conftest import rand_cols, rand_f64

pytestmark = pytest.mark.gpu
F64 = 1
P = RP.P
BUDGET = (1 << 19) + (1 << 16)   # "about 2^19": the largest case is the 2^19-leaf tree plus nothing else
GRIND_BUDGET = 7 << 16
W0 = 1 << 16                     # the first window of GRIND_PLAN_RP64 / GRIND_PLAN_RPJIVE; then 2 W0, 4 W0


class H:
    """One hasher: its id, references, the tree's level / sub-tree switch, row lengths on both sides of one rate block."""

    def __init__(self, capi, orc, name):
        self.name = name
        self.id = capi.RP64_256 if name == "rp64_256" else capi.RPJIVE64_256
        self.A = orc.Rescue(name)
        self.U = RP if name == "rp64_256" else RJ
        self.rate = 8 if name == "rp64_256" else 4
        self.switch = 17 if name == "rp64_256" else 18     # log2 leaves at which k_merkle_level first runs
        self.rows_entry = "rp_rows" if name == "rp64_256" else "rpj_rows"
        self.merge_entry = "rp_rows" if name == "rp64_256" else "rpj_merge"
        self.seed_entry = "rp_seed" if name == "rp64_256" else "rpj_seed"
        self.spent = 0

    def perms_of_row(self, k):
        return -(-k // self.rate)


@pytest.fixture(scope="module", params=["rp64_256", "rpjive64_256"])
def hs(request, capi, orc):
    """(hasher, a context of its own set to it, made with no WF_EXP_* tuning in force)."""
    import os
    assert not any(k.startswith("WF_EXP_GRIND") for k in os.environ), "this file runs the product's own window plan"
    h = H(capi, orc, request.param)
    c = capi.Context(0)
    c.set_hasher(h.id)
    yield h, c
    c.close()


@pytest.fixture(autouse=True)
def _budget(hs):
    """Every test counts the reference permutations it asks for (h.spent); none may ask for more than BUDGET.  (A nonce
    search is held to GRIND_BUDGET tries by expect().)"""
    h = hs[0]
    h.spent = 0
    yield
    assert h.spent <= BUDGET, f"{h.spent} reference permutations in one test"


def _canonical(digests):
    return (np.ascontiguousarray(digests).view(np.uint64) < np.uint64(P)).all()


def _ref_tree(h, leaves):
    h.spent += leaves.shape[0] - 1
    return h.A.merkle_nodes(leaves)


def _ref_rows(h, rows):
    h.spent += rows.shape[0] * h.perms_of_row(rows.shape[1])
    return h.A.hash_rows(rows)


# ---------------------------------------------------------------------------------------------------------- merkle_build_dev
def _leaves(log_n):
    """As _leaves() of tests/test_gpu_rp64.py: random u64 words, the words at and above p in the first and the last leaf."""
    n = 1 << log_n
    rng = np.random.default_rng(log_n)
    leaves = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)
    edge = np.array([P, P + 1, 2**64 - 1, 2**64 - 2**32], dtype=np.uint64)
    leaves[0] = edge
    leaves[n - 1] = edge[::-1]
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
    return got[:n]


def _check_tree(h, c, leaves):
    want = _ref_tree(h, leaves)
    got = _build_dev(c, leaves)
    assert not got[0].any()
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"{bad.size} nodes differ, the first at {bad[:8].tolist()}"
    assert bytes(got[1]) == bytes(want[1])
    assert _canonical(got)


@pytest.mark.parametrize("at", [-1, 0, 1])
def test_merkle_build_every_node(hs, at):
    """One size below the level / sub-tree switch (sub-tree launches only), the size at it (one lane-per-parent launch) and
    one above (two of them feed the sub-tree kernel): every node and the root."""
    h, c = hs
    _check_tree(h, c, _leaves(h.switch + at))


def _directed_pairs(h):
    """64 pairs of leaves whose merge meets a directed case in the first linear layer: every (row, case) of the merge's
    entry point, then a second draw; for RpJive64_256, whose merge controls every place, the two extreme states as well."""
    ins = D.inputs(h.merge_entry, 0)
    assert sorted(ins) == sorted(D.all_pairs(h.merge_entry))
    pairs = [ins[rc] for rc in D.all_pairs(h.merge_entry)]
    if h.merge_entry == "rpj_merge":
        pairs += [D.preimage(h.name, y) for y in D.extra_states(8)]
    more = D.inputs(h.merge_entry, 1)
    pairs += [more[rc] for rc in D.all_pairs(h.merge_entry) if rc[1] == "wrap"]
    pairs += [more[rc] for rc in D.all_pairs(h.merge_entry) if rc[1] != "wrap"]
    pairs = pairs[:64]
    assert len(pairs) == 64 and all(len(p) == 8 and max(p) < P for p in pairs)
    return np.array(pairs, dtype=np.uint64).reshape(128, 4).view(np.uint8).reshape(128, 32)


def test_merkle_subtree_on_directed_pairs(hs):
    """2^7 leaves, every pair a directed one: the bottom level runs in k_merkle_subtree_lanes<rp::Lanes> / <rpj::Lanes>, the
    lane form of the linear layer (lane_mds_ark).  Against the C reference and the Python one."""
    h, c = hs
    leaves = _directed_pairs(h)
    want = _ref_tree(h, leaves)
    assert np.array_equal(want, h.U.merkle_nodes(leaves))
    got = _build_dev(c, leaves)
    assert np.array_equal(got[64:], want[64:]), "the level above the directed pairs"
    assert np.array_equal(got, want) and _canonical(got)


def test_merkle_level_on_directed_pairs(hs):
    """The tree at the switch size whose first and last 64 leaves are the directed pairs: they go through
    k_merkle_level<Merge>, the one-lane form inside the wide kernel."""
    h, c = hs
    leaves = _leaves(h.switch).copy()
    d = _directed_pairs(h)
    leaves[:64] = d[:64]
    leaves[-64:] = d[64:]
    _check_tree(h, c, leaves)


# ---------------------------------------------------------------------------------------------------------- hash_rows
def _hash_rows(capi, c, rows, tail=5):
    a = np.ascontiguousarray(rows, dtype=np.uint64)
    n, k = a.shape
    out = np.full((n + tail, 32), 0xA5, dtype=np.uint8)
    rc = capi.load().wf_hash_rows(c._h, F64, a.ctypes.data, n, k, out.ctypes.data)
    assert rc == 0, capi.load().wf_last_error()
    assert (out[n:] == 0xA5).all(), "hash_rows wrote behind its last digest"
    return out[:n]


@pytest.mark.parametrize("side", [0, 1])
def test_hash_rows_many(capi, hs, side):
    """2^16 + 77 rows (257 work-groups, the last one a wave and 13 lanes) of one rate block and of one element more."""
    h, c = hs
    n, k = (1 << 16) + 77, h.rate + side
    rows = rand_f64(np.random.default_rng(1000 + k), n * k).reshape(n, k)
    rows[0, :] = 0
    rows[n - 1, :] = np.uint64(P - 1)
    got = _hash_rows(capi, c, rows)
    want = _ref_rows(h, rows)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"{bad.size} rows differ, the first at {bad[:8].tolist()}"
    assert _canonical(got)


def test_hash_rows_of_255_elements_all(capi, hs):
    """All 70 rows of the 255-element case of the per-hasher files (same seed, same rows)."""
    h, c = hs
    rows = rand_f64(np.random.default_rng(255), 70 * 255).reshape(70, 255)
    got = _hash_rows(capi, c, rows)
    assert np.array_equal(got, _ref_rows(h, rows)) and _canonical(got)


def test_hash_rows_directed(capi, hs):
    """Rows of exactly one rate block whose first S-box output is a directed state: every (row, case) the entry point reaches
    -- asserted to be all of them -- among uniform rows, ending in a partial wave."""
    h, c = hs
    assert D.reachable(h.rows_entry) == D.all_pairs(h.rows_entry)
    ins = D.inputs(h.rows_entry)
    directed = np.array([D.stored(ins[rc]) for rc in D.all_pairs(h.rows_entry)], dtype=np.uint64)
    assert directed.shape == (5 * h.A.width, h.rate)
    rng = np.random.default_rng(5)
    rows = np.concatenate([directed, rand_f64(rng, 141 * h.rate).reshape(141, h.rate)])
    order = rng.permutation(rows.shape[0])
    assert rows.shape[0] % 64 != 0
    rows = np.ascontiguousarray(rows[order])
    got = _hash_rows(capi, c, rows)
    want = _ref_rows(h, rows)
    assert np.array_equal(want, h.U.hash_rows(rows))
    for pos in np.flatnonzero(order < directed.shape[0]):
        assert bytes(got[pos]) == bytes(want[pos]), D.all_pairs(h.rows_entry)[order[pos]]
    assert np.array_equal(got, want) and _canonical(got)


# ---------------------------------------------------------------------------------------------------------- commitments
def _ref_commitment(h, orc, ext, logR, logB, n_cols, n_traces, seed):
    rng = np.random.default_rng(seed)
    traces = [rand_cols(rng, F64, n_cols, (1 << logR) * ext) for _ in range(n_traces)]
    want = orc.build_trace_commitment(F64, traces, ext, logR, logB, 7, threads=8)
    epr = n_cols * ext
    rows = np.ascontiguousarray(np.hstack([m[:, :epr] for m in want["lde"]]))
    leaves = _ref_rows(h, rows)
    nodes = _ref_tree(h, leaves)
    return traces, want, leaves, nodes


@pytest.mark.parametrize("shape", [(1, 12, 3, 8, 1), (1, 11, 2, 17, 2), (2, 11, 3, 3, 1)])
def test_trace_commit_dev_every_leaf_and_node(capi, orc, hs, shape):
    """wf_trace_commit_dev: 2^15 rows of 8; a multi-segment packed shape (two traces of 17 columns, 34 elements a row); a
    quadratic-extension one (6 base elements a row).  The oracle's LDE hashed with the C reference."""
    import torch
    h, c = hs
    ext, logR, logB, n_cols, n_traces = shape
    traces, want, leaves, nodes = _ref_commitment(h, orc, ext, logR, logB, n_cols, n_traces, sum(shape))
    p = capi.make_params(F64, ext, logR, logB, n_cols, n_traces, hasher=h.id)
    dev = torch.device("cuda", 0)
    N, rw = 1 << (logR + logB), orc.row_width(n_cols, ext)
    d_trace = torch.from_numpy(np.concatenate([col for t in traces for col in t]).view(np.int64)).to(dev)
    d_polys = torch.empty_like(d_trace)
    d_lde = torch.full((n_traces * N * rw,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device=dev)
    d_leaves = torch.full((N + 3, 32), 0xA5, dtype=torch.uint8, device=dev)
    d_nodes = torch.full((N + 3, 32), 0xA5, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    c.trace_commit_dev(p, d_trace.data_ptr(), d_polys.data_ptr(), d_lde.data_ptr(), d_leaves.data_ptr(), d_nodes.data_ptr())
    c.synchronize()
    lde = d_lde.cpu().numpy().view(np.uint64).reshape(n_traces, N, rw)
    for t in range(n_traces):
        assert np.array_equal(lde[t][:, :n_cols * ext], want["lde"][t][:, :n_cols * ext])
    g_leaves, g_nodes = d_leaves.cpu().numpy(), d_nodes.cpu().numpy()
    assert (g_leaves[N:] == 0xA5).all() and (g_nodes[N:] == 0xA5).all()
    assert np.array_equal(g_leaves[:N], leaves), "leaves"
    assert np.array_equal(g_nodes[:N], nodes), "nodes"
    assert not g_nodes[0].any() and _canonical(g_leaves[:N]) and _canonical(g_nodes[:N])


def test_resident_commitment_batch_query(capi, orc, hs):
    """The first shape through the resident form: the root, and a batch query of 40 positions against proofs cut from the
    reference tree."""
    h, c = hs
    ext, logR, logB, n_cols, n_traces = 1, 12, 3, 8, 1
    traces, want, leaves, nodes = _ref_commitment(h, orc, ext, logR, logB, n_cols, n_traces, 24)
    N = 1 << (logR + logB)
    p = capi.make_params(F64, ext, logR, logB, n_cols, n_traces, hasher=h.id)
    com, _ = c.trace_commit_resident(p, traces[0])
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
    finally:
        com.close()


@pytest.mark.parametrize("folding", [4, 2])
def test_fri_layer_commit_every_leaf_and_node(orc, hs, folding):
    """n = 2^16 evaluations of the quadratic extension: rows of folding * 2 base elements, 2^14 / 2^15 leaves."""
    h, c = hs
    ext, n = 2, 1 << 16
    ev = rand_f64(np.random.default_rng(16 + folding), n * ext)
    got = c.fri_layer_commit(F64, ext, ev, folding)
    tr = orc.transpose_slice(F64, ev, n, ext, folding)
    assert np.array_equal(got["transposed"], tr)
    leaves = _ref_rows(h, np.ascontiguousarray(tr.reshape(n // folding, folding * ext)))
    nodes = _ref_tree(h, leaves)
    assert np.array_equal(got["leaves"], leaves), "leaves"
    assert np.array_equal(got["nodes"], nodes), "nodes"
    assert got["root"] == bytes(nodes[1]) and _canonical(got["leaves"]) and _canonical(got["nodes"])


# ---------------------------------------------------------------------------------------------------------- wf_grind_seeds
# Seeds are SHA-256 of the ASCII text "grind seed <k>", searched on the CPU with the C reference; smallest qualifying nonce
# from nonce 1 at grinding factor 16.  The product's window plan from nonce 1: [1, 2^16], [2^16 + 1, 3 * 2^16],
# [3 * 2^16 + 1, 7 * 2^16].
GRIND_G = 16
GRIND_SEEDS = {   # hasher -> (k, answer) late in the first window, in the second, in the third
    "rp64_256": ((111, 51308), (105, 123507), (125, 210906)),
    "rpjive64_256": ((103, 50186), (100, 131243), (106, 231975)),
}
NOT_FOUND = (0, bytes(32), 0)


def K(k):
    return hashlib.sha256(b"grind seed %d" % k).digest()


def expect(h, seed, g, begin=1, max_nonces=2**64 - 1):
    """The reference search: the smallest qualifying nonce of the range with its digest.  It tries at most GRIND_BUDGET
    nonces and FAILS the test when a longer range has nothing within them: it never gives up silently."""
    span = min(max_nonces, 2**64 - begin)
    n, d = h.A.grind(seed, g, begin, min(span, GRIND_BUDGET))
    if n is None:
        if span > GRIND_BUDGET:
            pytest.fail(f"CPU search g={g} from {begin} went beyond its budget of {GRIND_BUDGET} tries: pick another seed")
        return NOT_FOUND
    return n, d, 1


def grind_one(c, seed, g, begin=1, max_nonces=2**64 - 1):
    nonces, new_seeds, found = c.grind(np.frombuffer(seed, dtype=np.uint8), g, begin, max_nonces)
    return int(nonces[0]), bytes(new_seeds[0]), int(found[0])


@pytest.mark.parametrize("window", [0, 1, 2])
def test_grind_in_each_production_window(hs, window):
    h, c = hs
    k, answer = GRIND_SEEDS[h.name][window]
    want = expect(h, K(k), GRIND_G)
    assert want[0] == answer and want[2] == 1
    assert (3 * W0 // 4, W0 + 1, 3 * W0 + 1)[window] <= answer <= (W0, 3 * W0, 7 * W0)[window]
    got = grind_one(c, K(k), GRIND_G)
    assert got == want
    assert int.from_bytes(got[1][:8], "little") % (1 << GRIND_G) == 0


def test_grind_range_ends_in_the_second_window(hs):
    """max_nonces one short of the second-window answer: not found; exactly at it: found."""
    h, c = hs
    k, answer = GRIND_SEEDS[h.name][1]
    want = expect(h, K(k), GRIND_G, 1, answer)
    assert want[0] == answer
    assert expect(h, K(k), GRIND_G, 1, answer - 1) == NOT_FOUND
    assert grind_one(c, K(k), GRIND_G, 1, answer - 1) == NOT_FOUND
    assert grind_one(c, K(k), GRIND_G, 1, answer) == want


def test_grind_batch_across_production_windows(capi, hs):
    """The three seeds in one call: each leaves the search in its own window; nothing is written behind n_seeds entries."""
    h, c = hs
    seeds = [K(k) for k, _ in GRIND_SEEDS[h.name]]
    want = [expect(h, s, GRIND_G) for s in seeds]
    assert [w[0] for w in want] == [a for _, a in GRIND_SEEDS[h.name]]
    n, tail = len(seeds), 3
    nonces = np.full(n + tail, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    new_seeds = np.full((n + tail, 32), 0xA5, dtype=np.uint8)
    found = np.full(n + tail, 0xA5, dtype=np.uint8)
    flat = np.frombuffer(b"".join(seeds), dtype=np.uint8)
    rc = capi.load().wf_grind_seeds(c._h, flat.ctypes.data, n, GRIND_G, 1, 2**64 - 1, nonces.ctypes.data,
                                    new_seeds.ctypes.data, found.ctypes.data)
    assert rc == 0, capi.load().wf_last_error()
    for i in range(n):
        assert (int(nonces[i]), bytes(new_seeds[i]), int(found[i])) == want[i], i
    assert (nonces[n:] == 0xA5A5A5A5A5A5A5A5).all() and (new_seeds[n:] == 0xA5).all() and (found[n:] == 0xA5).all()


def test_grind_on_directed_seeds(hs):
    """Factor 0 and max_nonces = 1 return merge_with_int(seed, nonce): directed seed words with a directed nonce, so that the
    first linear layer of k_grind / k_grind_finish meets every (row, case) its caller can reach -- asserted to be all."""
    h, c = hs
    assert D.reachable(h.seed_entry) == D.all_pairs(h.seed_entry)
    ins = D.inputs(h.seed_entry)
    for rc in D.all_pairs(h.seed_entry):
        *words, nonce = ins[rc]
        assert len(words) == 4 and nonce < P
        seed = b"".join(w.to_bytes(8, "little") for w in words)
        want = h.A.merge_with_int(seed, nonce)
        h.spent += 1
        if h.name == "rpjive64_256":
            assert want == RJ.merge_with_int(seed, nonce)
        else:
            assert want == RP.digest_bytes(RP.hash_elements(words + [nonce]))
        assert grind_one(c, seed, 0, nonce, 1) == (nonce, want, 1), rc
