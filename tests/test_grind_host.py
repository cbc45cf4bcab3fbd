"""CPU: merge_with_int of csrc/keccak_dev.hpp and csrc/rescue_dev.hpp (what the nonce search kernels run per nonce) against
hashlib.sha3_256 and tests/rp64_util.py.  Built with plain g++: the functions are __host__ __device__.  Values: both nonce
words, and for Rp64_256 both branches of the function (value < p: five elements; value >= p: six, the sixth value / p),
on a seed of canonical words and on one with words >= p (read as BaseElement::new reads them)."""
import hashlib
import os
import subprocess

import pytest

import rp64_util as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = R.P
VALUES = [0, 1, 2**32 - 1, 2**32, P - 1, P, P + 1, 2**64 - 1]
SEEDS = [
    [0x0123456789ABCDEF, 0x0FEDCBA987654321, 0x00000000FFFFFFFF, 0x7FFFFFFF00000001],  # canonical words
    [P, 2**64 - 1, P + 1, 0],                                                           # words >= p, and zero
]


def _build(tmp_path, extra=()):
    exe = str(tmp_path / "test_grind_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", *extra, "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_grind_host.cpp")])
    return exe


_CASES = None


def _cases():
    """(request line, expected digest words): hashlib and Python integers only.  16 permutations."""
    global _CASES
    if _CASES is None:
        _CASES = []
        for seed in SEEDS:
            raw = b"".join(w.to_bytes(8, "little") for w in seed)
            for v in VALUES:
                want = hashlib.sha3_256(raw + v.to_bytes(8, "little")).digest()
                _CASES.append((f"S {' '.join(map(str, seed))} {v}", R.digest_words(want)))
                elems = [w % P for w in seed] + [v % P] + ([v // P] if v >= P else [])
                assert len(elems) == (6 if v >= P else 5)
                _CASES.append((f"R {' '.join(map(str, seed))} {v}", R.hash_elements(elems)))
    return _CASES


def _run(exe, env=None):
    cases = _cases()
    res = subprocess.run([exe], input="\n".join(line for line, _ in cases) + "\n", capture_output=True, text=True, timeout=120,
                         env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    got = [[int(x) for x in l.split()] for l in res.stdout.splitlines()]
    assert len(got) == len(cases)
    for (line, want), g in zip(cases, got):
        assert g == want, line
    # the two Rp64_256 branches differ in more than the sixth element: p and 0 are the same element, their digests differ
    by_line = {line: g for (line, _), g in zip(cases, got)}
    seed = " ".join(map(str, SEEDS[0]))
    assert by_line[f"R {seed} {P}"] != by_line[f"R {seed} 0"]


def test_merge_with_int_matches_hashlib_and_the_python_reference(tmp_path):
    _run(_build(tmp_path))


def test_merge_with_int_under_address_and_ub_sanitizers(tmp_path):
    """The same stand-alone program with -fsanitize=address,undefined (nothing is preloaded: it has its own main)."""
    try:
        exe = _build(tmp_path, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    except subprocess.CalledProcessError:
        pytest.skip("this g++ has no sanitizer runtime")
    _run(exe, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
