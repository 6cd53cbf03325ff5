"""The host rules of hdpm_trace_merge_gains, hdpm_trace_merge_path and hdpm_trace_refine_merge
(csrc/trace_merge.hpp, plain C++): the tie order, empty classes, the path's labels, values and
step count, and the alternation of descent and merges with its bounds, on small traces with a
CPU model of gains and losses, checked by tests/cpp/trace_merge_test.cpp.  The program is host
code only and runs a second time built with the address and undefined-behaviour sanitizers.
No GPU."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_trace_merge_rules(tmp_path, flags):
    exe = tmp_path / "trace_merge_test"
    src = os.path.join(HERE, "cpp", "trace_merge_test.cpp")
    # -ffp-contract=off as in csrc/Makefile: the losses are compared as doubles
    r = subprocess.run(["g++", *flags, "-std=c++17", "-ffp-contract=off", "-Wall", "-o", str(exe), src],
                       capture_output=True, text=True)
    if r.returncode != 0:
        pytest.fail(r.stderr)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "trace merge ok" in r.stdout
