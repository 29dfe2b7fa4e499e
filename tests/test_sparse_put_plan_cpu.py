"""zvec_amd/csrc/host/sparse_put_plan.h without a GPU: the host's share of both sparse add-with-id entries is plain C++ that includes
nothing of HIP (tests/cpp/test_sparse_put_plan_cpu.cc: the keep-last rule, the plan and its tables, the workspace layout and the hole
bits against a row-at-a-time model of add_vector_with_id, over fixed cases, the refusals and a few thousand random calls)."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_keep_plan_and_holes_against_a_row_at_a_time_model():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "test_sparse_put_plan_cpu")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_sparse_put_plan_cpu.cc")])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        assert out.stdout.strip().endswith("ok")
