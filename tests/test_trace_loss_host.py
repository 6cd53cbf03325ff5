"""The host arithmetic of the posterior summaries (csrc/trace_loss.hpp, plain C++): cluster
sizes to log2 sizes, sum n log2 n and the pair count, the VI expressions, the block rule, the
label scan and the 63-bit bound, checked by tests/cpp/trace_loss_test.cpp.  No GPU."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_trace_loss_helpers(tmp_path):
    exe = tmp_path / "trace_loss_test"
    src = os.path.join(HERE, "cpp", "trace_loss_test.cpp")
    # -ffp-contract=off as in csrc/Makefile: the doubles are compared by bytes
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-o", str(exe), src],
                       capture_output=True, text=True)
    if r.returncode != 0:
        pytest.fail(r.stderr)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "trace loss ok" in r.stdout
