"""zvec_amd/csrc/host/hole_bits.h without a GPU: the host half of both flat handles' hole bits is plain C++ that includes nothing of
HIP (tests/cpp/test_hole_bits_cpu.cc: set-range, clear and resize against a one-bit-at-a-time model, the dirty word range checked
after every step)."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hole_words_against_a_bit_at_a_time_model():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "test_hole_bits_cpu")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_hole_bits_cpu.cc")])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        assert out.stdout.strip().endswith("ok")
