"""CPU: the launch sequence of the Merkle tree (merkle_next_launch, csrc/merkle_plan.hpp) is the one the three per-hasher
host loops produced before they became one.  tests/cpp/test_merkle_plan.cpp restates those loops and compares, launch
for launch (kind, grid, block, levels, children before and after), for every n_leaves = 2^1 .. 2^34, every hasher and
every merkle_l2_min in 10 .. 30.  Built with plain g++: the header needs no HIP."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path, extra=()):
    exe = str(tmp_path / "test_merkle_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O2", *extra, "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_merkle_plan.cpp")])
    return exe


def _run(exe, env=None):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok: ") and " 0 mismatches" in out.stdout, out.stdout
    # 34 sizes x 21 tuning values x 4 CU counts x 3 hashers
    assert f" {34 * 21 * 4 * 3} sequences compared" in out.stdout, out.stdout


def test_launch_sequences_match_the_former_loops(tmp_path):
    _run(_build(tmp_path))


def test_launch_sequences_under_address_and_ub_sanitizers(tmp_path):
    """The same stand-alone program with -fsanitize=address,undefined (nothing is preloaded: it has its own main)."""
    try:
        exe = _build(tmp_path, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    except subprocess.CalledProcessError:
        pytest.skip("this g++ has no sanitizer runtime")
    _run(exe, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
