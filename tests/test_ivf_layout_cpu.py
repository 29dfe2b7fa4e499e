"""zvec_amd/csrc/host/ivf_layout.h without a GPU: the host's share of an IVF build is plain C++ that includes nothing of HIP
(tests/cpp/test_ivf_layout_cpu.cc: the list -> shard map, the layout, the all-or-nothing placement of a chunk, the deal order and its
levels, and the position map against a row-at-a-time model of the per-list append, over fixed cases, the refusals and a few thousand
random builds)."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layout_placement_and_deal_order_against_a_row_at_a_time_model():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "test_ivf_layout_cpu")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_ivf_layout_cpu.cc")])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        assert out.stdout.strip().endswith("ok")
