"""CPU: the window schedule of the nonce search (grind_next_window, csrc/grind_plan.hpp).  tests/cpp/test_grind_plan.cpp
checks it from its statement -- contiguous windows from `begin`, sizes doubling from 2^first to 2^cap, the last one clipped,
their sum min(max_nonces, 2^64 - begin), nothing past 2^64 - 1 -- for every first <= cap in 2..12, begin in {0, 1, 2^32 - 1,
2^63, 2^64 - 70, 2^64 - 1} and max_nonces in {1, 2, 63, 64, 65, 1000, 2^40, 2^64 - 1}.  Built with plain g++: the header
needs no HIP."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path, extra=()):
    exe = str(tmp_path / "test_grind_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O2", *extra, "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_grind_plan.cpp")])
    return exe


def _run(exe, env=None):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok: ") and " 0 mismatches" in out.stdout, out.stdout
    # 66 (first, cap) pairs x 6 begins x 8 range lengths
    assert f"ok: {66 * 6 * 8} schedules checked" in out.stdout, out.stdout


def test_windows_tile_the_range_once(tmp_path):
    _run(_build(tmp_path))


def test_windows_under_address_and_ub_sanitizers(tmp_path):
    """The same stand-alone program with -fsanitize=address,undefined (nothing is preloaded: it has its own main)."""
    try:
        exe = _build(tmp_path, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    except subprocess.CalledProcessError:
        pytest.skip("this g++ has no sanitizer runtime")
    _run(exe, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
