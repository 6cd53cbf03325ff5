"""The host side of the cluster profiles without a GPU (csrc/profile_host.hpp, plain C++;
tests/cpp/profile_host_test.cpp): the cuts of the attributes into blocks and of the draws into
chunks cover every item once for budgets from 1 byte up, the argument refusals are returned, and
the scalar fold gives the bytes of the restatement (tests/profile_ref.py) on a fixture written
here: a recorded chain of 5 draws with an empty class, the tables, the parameter rows with the
exps of their pairs, and the restatement's five outputs."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import profile_ref as pref  # noqa: E402


def write_fixture(path):
    Ks = [3, 1, 7, 2, 20]
    p = pref.problem(seed=5, N=45, d=9, Ks=Ks, att=[2, 3, 4, 6, 16, 17, 100, 255, 2])
    att, M, d, Ka, ld = p["att"], len(Ks), 9, 4, 255
    cl = np.where(np.arange(45) % 3 == 0, 0, np.where(np.arange(45) % 3 == 1, 1, 3)).astype(np.int32)   # class 2 is empty
    want = pref.profile(p["c_trace"], p["centers"], p["sigmas"], att, cl, Ka, ld)
    Kz = max(Ks)
    tab = np.zeros((M, Ka, Kz), np.uint32)
    for s, T in enumerate(pref.tables(p["c_trace"], cl, Ka)):
        tab[s, :, :T.shape[1]] = T
    cen = np.concatenate(p["centers"]).astype(np.uint8)
    sig = np.concatenate(p["sigmas"])
    emm = np.stack([np.concatenate(x) for x in zip(*[pref.exp_pairs(s, att) for s in p["sigmas"]])], axis=2)
    assert emm.shape == (sum(Ks), d, 2)
    parts = [np.array([M, Ka, Kz, d, ld, sum(Ks)], np.int32), att.astype(np.int32), np.array(Ks, np.int32), tab,
             want["sizes"].astype(np.uint64), cen, sig, emm, want["center_cnt"], want["code_pmf"], want["sigma_mean"],
             want["sigma_var"], want["sigma_trace"]]
    with open(path, "wb") as f:
        for a in parts:
            f.write(np.ascontiguousarray(a).tobytes())
    return want


def test_profile_host(tmp_path):
    exe = tmp_path / "profile_host_test"
    src = os.path.join(HERE, "cpp", "profile_host_test.cpp")
    # -ffp-contract=off as in csrc/Makefile: the doubles are compared by bytes
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-o", str(exe), src],
                       capture_output=True, text=True)
    if r.returncode != 0:
        pytest.fail(r.stderr)
    fixture = tmp_path / "profile_fixture.bin"
    want = write_fixture(fixture)
    assert want["sizes"][2] == 0 and want["sigma_var"].max() > 0
    r = subprocess.run([str(exe), str(fixture)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fold checked: M 5 Ka 4 d 9 ld 255" in r.stdout
    assert "profile host ok" in r.stdout
