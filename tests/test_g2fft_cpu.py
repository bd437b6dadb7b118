"""The G2 group FFT at the C ABI and in the Python mirror: declared, exported, listed, typed as the
reference types it, and argument errors raised before any GPU call.  CPU only."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = ["bn128", "bls12_381"]
REF_NAMES = [f"{c}_G2_proj_fft_{d}" for c in CURVES for d in ("forward", "inverse")]
EXT_NAMES = ["zkg_g2_fft_device", "zkg_g2_fft_set_max_lanes"]


def header():
    return open(os.path.join(ROOT, "include", "zkalgebra_gpu.h")).read()


def test_header_declares_g2fft_symbols():
    declared = set(re.findall(r"ZKG_API\s+[\w\s\*]+?\b(\w+)\s*\(", header()))
    assert set(REF_NAMES + EXT_NAMES) <= declared, sorted(set(REF_NAMES + EXT_NAMES) - declared)


def test_library_exports_g2fft_symbols(zk):
    out = subprocess.check_output(["nm", "-D", "--defined-only", zk.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(REF_NAMES + EXT_NAMES) <= exported, sorted(set(REF_NAMES + EXT_NAMES) - exported)


def test_symbol_lists_name_g2fft(zk):
    assert set(REF_NAMES) <= set(zk.REFERENCE_SYMBOLS)
    assert set(EXT_NAMES) <= set(zk.EXTENSION_SYMBOLS)
    for f in ("g2_forward_fft", "g2_inverse_fft", "g2_fft_set_max_lanes"):
        assert callable(getattr(zk, f))
    lib = zk.load()
    for n in REF_NAMES:
        assert len(getattr(lib, n).argtypes) == 4, n
    assert len(lib.zkg_g2_fft_device.argtypes) == 6
    assert len(lib.zkg_g2_fft_set_max_lanes.argtypes) == 1


def _ptypes(s):
    return [re.sub(r"\w+$", "", a.strip()).replace(" ", "") for a in s[s.index("(") + 1:s.rindex(")")].split(",")]


def test_g2fft_prototypes_match_reference():
    """parameter types of the four reference symbols are the reference header's (names may differ)"""
    ref = "/root/reference/lib/cbits/curves/g2/proj"
    if not os.path.isdir(ref):
        pytest.skip("reference tree not present")
    ours = header().splitlines()
    for c in CURVES:
        protos = {}
        for line in open(os.path.join(ref, f"{c}_G2_proj.h")):
            m = re.search(r"(\w+_fft_(forward|inverse))\s*\(", line)
            if m and "noalloc" not in line:
                protos[m.group(1)] = line.replace("extern", "").strip().rstrip(";")
        assert sorted(protos) == sorted(n for n in REF_NAMES if n.startswith(c))
        for name, proto in protos.items():
            mine = [l for l in ours if re.search(r"\b" + name + r"\s*\(", l)]
            assert len(mine) == 1, name
            assert mine[0].split()[:2] == ["ZKG_API", "void"], name
            assert _ptypes(proto) == _ptypes(mine[0]), name


@pytest.fixture
def no_gpu_calls(zk, monkeypatch):
    """argument errors must be raised before the library or a device is touched"""
    def boom(*a, **k):
        raise AssertionError("reached the GPU path")
    monkeypatch.setattr(zk, "require_gpu", boom)
    monkeypatch.setattr(zk, "load", boom)
    return zk


@pytest.mark.parametrize("curve", CURVES)
def test_g2_fft_argument_errors(no_gpu_calls, curve):
    zk = no_gpu_calls
    NP = zk.NLIMBS_P[curve]
    sg = zk.FFTSubgroup(curve, (1, 2, 3, 4), 3)
    for f in (zk.g2_forward_fft, zk.g2_inverse_fft):
        for w in (3 * NP, 4 * NP, 6 * NP - 1, 6 * NP + 1):  # G1 projective, G2 affine, off by one
            with pytest.raises(ValueError):
                f(sg, np.zeros((8, w), np.uint64))
        with pytest.raises(ValueError):  # not 2-D
            f(sg, np.zeros(8 * 6 * NP, np.uint64))
        with pytest.raises(ValueError):
            f(sg, np.zeros((2, 4, 6 * NP), np.uint64))
        for n in (0, 4, 7, 9, 16):  # size differs from the subgroup's
            with pytest.raises(ValueError):
                f(sg, np.zeros((n, 6 * NP), np.uint64))
        with pytest.raises(AssertionError, match="reached the GPU path"):  # a well-formed call goes on
            f(sg, np.zeros((8, 6 * NP), np.uint64))
