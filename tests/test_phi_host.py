"""The host side of a device update_phi's outcome (csrc/phi_host.hpp, plain C++): the output
layout, the view over an output buffer, the hand-back bit, the re-run ladder's table and the
log-likelihood fold, checked by tests/cpp/phi_host_test.cpp.  No GPU."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_phi_outcome_helpers(tmp_path):
    exe = tmp_path / "phi_host_test"
    src = os.path.join(HERE, "cpp", "phi_host_test.cpp")
    # -ffp-contract=off as in csrc/Makefile: the fold is compared bit for bit
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-o", str(exe), src],
                       capture_output=True, text=True)
    if r.returncode != 0:
        pytest.fail(r.stderr)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "phi host ok" in r.stdout
