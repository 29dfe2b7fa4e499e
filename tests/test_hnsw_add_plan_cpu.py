"""zvec_amd/csrc/host/hnsw_add_plan.h without a GPU: the host's share of the HNSW build and append is plain C++ that includes nothing of
HIP (tests/cpp/test_hnsw_add_plan_cpu.cc: the rounds from a base against a restatement, the request offsets of the new nodes, the
levels of a range, the capacity steps, the stride decision, the refusals and a few thousand random call sequences), compiled with
the address and undefined-behaviour sanitizers into a program of its own."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rounds_offsets_capacity_and_stride_against_a_restatement():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "test_hnsw_add_plan_cpu")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                               os.path.join(ROOT, "tests", "cpp", "test_hnsw_add_plan_cpu.cc")])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        assert out.stdout.strip().endswith("ok")
