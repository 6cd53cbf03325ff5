"""The descent rule of hdpm_trace_refine on the host (csrc/trace_refine.hpp, plain C++): the
selection, the new-class rule, the halving and the relabelling on small traces with a CPU
model of the gains, Binder's end state against brute force, and the run's end when a single
move is rejected, checked by tests/cpp/trace_refine_test.cpp.  No GPU."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_trace_refine_rule(tmp_path):
    exe = tmp_path / "trace_refine_test"
    src = os.path.join(HERE, "cpp", "trace_refine_test.cpp")
    # -ffp-contract=off as in csrc/Makefile: the losses are compared as doubles
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-o", str(exe), src],
                       capture_output=True, text=True)
    if r.returncode != 0:
        pytest.fail(r.stderr)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "trace refine ok" in r.stdout
