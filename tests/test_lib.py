"""CPU checks of the product library: it builds, loads, exports every symbol that
include/hdpm.h declares, and refuses to run without a gfx950 device (no CPU fallback)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    src = open(os.path.join(ROOT, "include", "hdpm.h")).read()
    return sorted(set(re.findall(r"\b(hdpm_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from split_and_merge_gibbs_sampling_amd import _lib
    _lib.build()
    L = _lib.lib()
    decl = declared_symbols()
    assert len(decl) >= 20
    for name in decl:
        assert hasattr(L, name), name
    assert set(decl) == set(_lib.EXPORTS)


def test_no_cpu_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    from split_and_merge_gibbs_sampling_amd import Engine, HdpmError
    with pytest.raises(HdpmError) as e:
        Engine(0)
    assert e.value.status == 7


def test_product_does_not_import_oracle():
    pkg = os.path.join(ROOT, "split_and_merge_gibbs_sampling_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".hpp", ".inl", "Makefile")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "oracle_ffi" not in txt and "liboracle" not in txt and "oracle/src" not in txt, f


def test_tiled_layout_roundtrip():
    import numpy as np
    # mirror of tiled_offset() in csrc/kernels.hpp
    def off(i, j, nq):
        return (((i >> 6) * nq + (j >> 4)) * 64 + (i & 63)) * 16 + (j & 15)
    n, d = 130, 37
    nq = (d + 15) // 16
    seen = set()
    for i in range(n):
        for j in range(d):
            o = off(i, j, nq)
            assert o not in seen
            seen.add(o)
    assert max(seen) < ((n + 63) // 64) * 64 * nq * 16


def declared_debug_bits():
    """HDPM_DBG_* of include/hdpm.h: name -> value, from '#define HDPM_DBG_X (1u << n)'."""
    src = open(os.path.join(ROOT, "include", "hdpm.h")).read()
    defs = re.findall(r"^#define\s+HDPM_DBG_([A-Z0-9_]+)\s+\(1u << (\d+)\)\s*$", src, flags=re.M)
    assert len(defs) == len(re.findall(r"^#define\s+HDPM_DBG_", src, flags=re.M)), "a HDPM_DBG_ line of another form"
    assert len({n for n, _ in defs}) == len(defs), "a name defined twice"
    return {n: 1 << int(b) for n, b in defs}


# the values the engine and the tests used as literals before the bits had names
DEBUG_VALUES = {
    "EXACT_ALL": 1, "PHASE_TIMES": 2, "LL_PER_POINT": 4, "NO_SNAPSHOT": 8, "RECOUNT": 16, "TIMELINE": 32,
    "HOST_POOL": 64, "NO_SPEC_PHI": 128, "NO_PREPARE": 256, "KERNEL_EVENTS": 512, "NO_POOL_HEADS": 1024,
    "EXACT_WAVE": 2048, "NO_BLOCK_MODE": 4096, "BLOCK_MODE_ALWAYS": 8192, "NO_WIDE_PREPASS": 16384,
    "SWEEP_FIRST": 32768, "SM_HOST_DRAWS": 65536, "NO_PREPASS_AHEAD": 131072, "MARGIN_ONLY": 262144,
    "PHI_HOST": 524288, "NO_LOOKAHEAD": 1048576, "COMMIT_FIRST": 2097152, "NO_PIPE": 4194304,
    "ONE_WAVE_RESOLVER": 8388608, "FP_LIST_ALL_AFTER_EXACT": 16777216, "FP_ALWAYS": 33554432,
    "FP_FROM_STAY": 67108864, "PHI_WALKS": 134217728, "POOL_SERIAL_PARSE": 268435456, "FP_ONE_WG": 536870912,
    "FPG_ALWAYS": 1073741824,
}


def test_debug_bits_named_once_with_their_values():
    import split_and_merge_gibbs_sampling_amd as hd
    bits = declared_debug_bits()
    assert len(bits) == 31
    for name, v in bits.items():
        assert v > 0 and v & (v - 1) == 0, name                      # a single bit
    assert sorted(bits.values()) == [1 << b for b in range(31)]      # distinct, bits 0..30
    # the Python mirror: the same names and values, re-exported beside Engine
    assert {m.name: int(m) for m in hd.Debug} == bits
    from split_and_merge_gibbs_sampling_amd import _lib, sampler
    assert hd.Debug is _lib.Debug is sampler.Debug
    # no value moved (bench.py, profiles and A/B records pass the numbers)
    assert len(DEBUG_VALUES) == 31
    for name, v in DEBUG_VALUES.items():
        assert bits[name] == v, name
    assert int(hd.Debug.FP_ALWAYS | hd.Debug.FPG_ALWAYS) == 33554432 | 1073741824


def test_engine_steering_has_no_bare_numbers_or_stray_getenv():
    """Every debug test in csrc/ goes by name, and csrc/switches.hpp alone reads the environment."""
    csrc = os.path.join(ROOT, "split_and_merge_gibbs_sampling_amd", "csrc")
    for f in sorted(os.listdir(csrc)):
        p = os.path.join(csrc, f)
        if not os.path.isfile(p):
            continue
        txt = open(p).read()
        assert not re.search(r"debug\s*&\s*\(?\s*[0-9]", txt), f
        if f != "switches.hpp":
            assert "getenv" not in txt, f
