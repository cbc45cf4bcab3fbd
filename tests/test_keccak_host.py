"""CPU: the SHA3-256 of csrc/keccak_dev.hpp (what the Sha3 row and tree kernels run) against hashlib.  Built with plain
g++: the functions are __host__ __device__.  Lengths around one and two rate blocks (136 bytes), a whole number of
blocks (136, 272, 2040 = 15 blocks, 4080 = 30 blocks: a further block holds only the padding), and the merge form."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = [0, 8, 64, 128, 135, 136, 137, 144, 264, 272, 280, 2040, 4080]


def _build(tmp_path, extra=()):
    exe = str(tmp_path / "test_keccak_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", *extra, "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_keccak_host.cpp")])
    return exe


def _requests():
    rng = np.random.default_rng(3)
    req, want = [], []
    for n in LENGTHS:
        msg = rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
        req.append("B " + msg.hex())
        want.append(hashlib.sha3_256(msg).hexdigest())
        if n % 8 == 0:  # the lane-granular absorber of the kernels
            req.append("L " + msg.hex())
            want.append(hashlib.sha3_256(msg).hexdigest())
    for _ in range(4):
        l, r = rng.integers(0, 256, size=32, dtype=np.uint8).tobytes(), rng.integers(0, 256, size=32, dtype=np.uint8).tobytes()
        req.append("M " + (l + r).hex())
        want.append(hashlib.sha3_256(l + r).hexdigest())
    req.append("M " + "00" * 64)
    want.append(hashlib.sha3_256(bytes(64)).hexdigest())
    return req, want


def _run(exe, env=None):
    req, want = _requests()
    out = subprocess.run([exe], input="\n".join(req) + "\n", capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    got = out.stdout.split()
    assert len(got) == len(want)
    for r, g, w in zip(req, got, want):
        assert g == w, f"{r[:1]} request of {(len(r) - 2) // 2} bytes: {g} != {w}"


def test_sha3_256_matches_hashlib(tmp_path):
    _run(_build(tmp_path))


def test_sha3_256_under_address_and_ub_sanitizers(tmp_path):
    """The same stand-alone program with -fsanitize=address,undefined (nothing is preloaded: it has its own main)."""
    try:
        exe = _build(tmp_path, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    except subprocess.CalledProcessError:
        pytest.skip("this g++ has no sanitizer runtime")
    # (the leak checker needs ptrace, which containers often deny; addresses and undefined behaviour are what is checked)
    _run(exe, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))


def test_params_check_knows_the_hasher(capi):
    lib = capi.load()
    assert capi.BLAKE3 == 0 and capi.SHA3_256 == 1
    ok = capi.make_params(capi.F64, 1, 10, 3, 8, 1, hasher=capi.SHA3_256)
    assert ok.hasher == 1 and ok.digest_bytes == 32
    assert lib.wf_params_check(ctypes.byref(ok), 0) == 0
    short = capi.make_params(capi.F64, 1, 10, 3, 8, 1, digest_bytes=24, hasher=capi.SHA3_256)
    assert lib.wf_params_check(ctypes.byref(short), 0) == -31
    assert b"Sha3" in lib.wf_last_error()
    unknown = capi.make_params(capi.F64, 1, 10, 3, 8, 1, hasher=2)
    assert lib.wf_params_check(ctypes.byref(unknown), 0) == -31
    assert b"hasher" in lib.wf_last_error()
    # hasher 0 is what every caller passed before (the field was `reserved`, must be zero): unchanged
    for db in (32, 24):
        assert lib.wf_params_check(ctypes.byref(capi.make_params(capi.F64, 1, 10, 3, 8, 1, digest_bytes=db)), 0) == 0
        assert lib.wf_params_check(ctypes.byref(capi.make_params(capi.F64, 1, 10, 3, 8, 1, digest_bytes=db, hasher=0)), 0) == 0
    assert lib.wf_params_check(ctypes.byref(capi.make_params(capi.F64, 1, 10, 3, 8, 1, digest_bytes=16)), 0) == -31
    assert capi.Params.hasher.offset == 28 and capi.Params.hasher.size == 4  # where `reserved` was


def test_python_helpers_agree_with_each_other(orc):
    """tests/sha3_util.py (the expected side of tests/test_gpu_sha3.py): its tree, single paths and batch proofs are
    consistent with the restated MerkleTree::prove / prove_batch of the oracle module (pure Python, hasher-agnostic)."""
    import sha3_util as S
    rng = np.random.default_rng(5)
    leaves = rng.integers(0, 256, size=(64, 32), dtype=np.uint8)
    nodes = S.merkle_nodes(leaves)
    assert not nodes[0].any()
    assert bytes(nodes[1]) == S.merge(S.merge(bytes(nodes[4]), bytes(nodes[5])), S.merge(bytes(nodes[6]), bytes(nodes[7])))
    assert bytes(nodes[32]) == hashlib.sha3_256(bytes(leaves[0]) + bytes(leaves[1])).digest()
    for idx in (0, 63, 21):
        assert S.verify_path(bytes(nodes[1]), idx, orc.merkle_prove(nodes, leaves, idx))
    for positions in ([0, 63], [5], [2, 3, 40, 41, 42, 17], list(range(64))):
        lv, vecs, depth = orc.merkle_prove_batch(nodes, leaves, positions)
        assert S.verify_batch(bytes(nodes[1]), positions, lv, vecs, depth)
        if vecs[0]:
            bad = [list(v) for v in vecs]
            bad[0][-1] = bytes(32)
            assert not S.verify_batch(bytes(nodes[1]), positions, lv, bad, depth)
    # f64: Montgomery residue -> canonical bytes (x * 2^-64 mod p); 2^64 mod p is the residue of one
    one = np.array([2**64 % S.F64_P], dtype=np.uint64)
    assert S.row_bytes(S.F64, one) == (1).to_bytes(8, "little")
    assert S.canonical_u64(orc.f64_new([0, 1, 12345, S.F64_P - 1])).tolist() == [0, 1, 12345, S.F64_P - 1]
