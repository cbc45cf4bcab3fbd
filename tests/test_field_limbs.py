"""CPU: the limb arithmetic of csrc/field.hpp (what the device code runs) against wide unsigned __int128 arithmetic and a
bit-serial product.  Built with plain g++: the functions are __host__ __device__.  A plain build takes the host branches of
F64::mont_reduce / mul / sub (the unsigned __int128 forms) and reaches the f128 limb functions only by name;
-DWF_FIELD_LIMBS_ON_HOST sends the host compiler down the device branches, so the 32-bit carry and borrow chains
themselves run here, on operands built to make their rare branches fire (tests/cpp/test_field_edges.cpp)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path, source, name, *defines):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-D__HIP_PLATFORM_AMD__", *defines, "-I/opt/rocm/include", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", source)])
    return exe


def test_f128_limb_arithmetic(tmp_path):
    exe = _build(tmp_path, "test_field_limbs.cpp", "test_field_limbs")
    out = subprocess.run([exe, "400000"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ALL OK" in out.stdout


def test_limb_forms_on_host(tmp_path):
    """The same program with the device forms compiled for the host: the shift twiddles end in the 32-bit borrow chain of
    F64::sub, F128::add / sub / mul are the limb functions."""
    exe = _build(tmp_path, "test_field_limbs.cpp", "test_field_limbs_dev", "-DWF_FIELD_LIMBS_ON_HOST")
    out = subprocess.run([exe, "100000"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ALL OK" in out.stdout


def test_carry_edge_operands(tmp_path):
    """Limb-alphabet pairs, directed reduction inputs and every shift twiddle through the device forms; the operand sets must
    tell a wrong-mask copy of the reduction (c2 instead of c2 | c3) from the real one."""
    exe = _build(tmp_path, "test_field_edges.cpp", "test_field_edges", "-DWF_FIELD_LIMBS_ON_HOST")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ALL OK" in out.stdout
    m = re.search(r"f64 alphabet: 43 values, 1849 ordered pairs, wrong-mask copy differs on (\d+)", out.stdout)
    # the program is deterministic (its own xorshift, fixed seed): exact counts, so that a shrunken operand set cannot pass
    assert m and int(m.group(1)) == 92, out.stdout
    m = re.search(r"directed reduction: (\d+) \(lo, hi\) inputs, wrong-mask copy differs on (\d+)", out.stdout)
    assert m and (int(m.group(1)), int(m.group(2))) == (22481, 4076), out.stdout
    m = re.search(r"f128 alphabet: 6535 values, (\d+) pairs", out.stdout)
    assert m and int(m.group(1)) == 6100891, out.stdout
