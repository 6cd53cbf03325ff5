"""The host tree of the matrix-free average-linkage search (csrc/trace_tree.hpp, plain C++):
its merge list against the greedy definition with the tie rule of include/hdpm.h, written
as an O(U^3) loop with __int128 fractions in tests/cpp/trace_tree_test.cpp.  No GPU."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_avg_linkage_is_the_greedy_sequence(tmp_path):
    exe = tmp_path / "trace_tree_test"
    src = os.path.join(HERE, "cpp", "trace_tree_test.cpp")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-o", str(exe), src], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.fail(r.stderr)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "trace tree ok" in r.stdout
