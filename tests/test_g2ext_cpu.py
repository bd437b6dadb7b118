"""The G2 batch conversions and the G2 `_variable` MSM at the C ABI and in the Python mirror: declared,
exported, listed, typed as the reference types them, and argument errors raised before any GPU call.
CPU only."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = ["bn128", "bls12_381"]
REF_NAMES = [f"{c}_G2_proj_{f}" for c in CURVES
             for f in ("batch_from_affine", "batch_to_affine", "MSM_std_coeff_proj_out_variable")]
EXT_NAMES = ["zkg_g2_batch_to_affine_device"]


def header():
    return open(os.path.join(ROOT, "include", "zkalgebra_gpu.h")).read()


def test_header_declares_g2ext_symbols():
    declared = set(re.findall(r"ZKG_API\s+[\w\s\*]+?\b(\w+)\s*\(", header()))
    assert set(REF_NAMES + EXT_NAMES) <= declared, sorted(set(REF_NAMES + EXT_NAMES) - declared)


def test_library_exports_g2ext_symbols(zk):
    out = subprocess.check_output(["nm", "-D", "--defined-only", zk.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(REF_NAMES + EXT_NAMES) <= exported, sorted(set(REF_NAMES + EXT_NAMES) - exported)


def test_symbol_lists_name_g2ext(zk):
    assert set(REF_NAMES) <= set(zk.REFERENCE_SYMBOLS)
    assert set(EXT_NAMES) <= set(zk.EXTENSION_SYMBOLS)
    for f in ("g2_batch_from_affine", "g2_batch_to_affine", "g2_msm_variable", "g2_msm_proj", "g2_msm_device"):
        assert callable(getattr(zk, f))


def _ptypes(s):
    return [re.sub(r"\w+$", "", a.strip()).replace(" ", "") for a in s[s.index("(") + 1:s.rindex(")")].split(",")]


def test_g2ext_prototypes_match_reference():
    """parameter types of the three reference symbols are the reference's (names may differ)"""
    ref = "/root/reference/lib/cbits/curves/g2/proj"
    if not os.path.isdir(ref):
        pytest.skip("reference tree not present")
    ours = header().splitlines()
    for c in CURVES:
        protos = {}
        for line in open(os.path.join(ref, f"{c}_G2_proj.h")):
            m = re.search(r"(\w+_batch_(from|to)_affine)\s*\(", line)
            if m:
                protos[m.group(1)] = line.replace("extern", "").strip().rstrip(";")
        for line in open(os.path.join(ref, f"{c}_G2_proj.c")):
            m = re.match(r"void\s+(\w+_MSM_std_coeff_proj_out_variable)\s*\(", line)
            if m:
                protos[m.group(1)] = line[:line.rindex(")") + 1]
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
def test_g2_batch_row_width_errors(no_gpu_calls, curve):
    zk = no_gpu_calls
    NP = zk.NLIMBS_P[curve]
    for w in (2 * NP, 3 * NP, 4 * NP, 6 * NP + 1):
        with pytest.raises(ValueError):
            zk.g2_batch_to_affine(curve, np.zeros((3, w), np.uint64))
    for w in (2 * NP, 3 * NP, 6 * NP, 4 * NP - 1):
        with pytest.raises(ValueError):
            zk.g2_batch_from_affine(curve, np.zeros((3, w), np.uint64))
    with pytest.raises(ValueError):
        zk.g2_batch_to_affine(curve, np.zeros(6 * NP, np.uint64))
    with pytest.raises(ValueError):
        zk.g2_batch_from_affine(curve, np.zeros(4 * NP, np.uint64))


@pytest.mark.parametrize("curve", CURVES)
def test_g2_msm_proj_shape_errors(no_gpu_calls, curve):
    zk = no_gpu_calls
    NP = zk.NLIMBS_P[curve]
    sc = np.zeros((5, 4), np.uint64)
    with pytest.raises(ValueError):  # affine rows where projective ones are due
        zk.g2_msm_proj(curve, sc, np.zeros((5, 4 * NP), np.uint64))
    with pytest.raises(ValueError):  # G1 projective rows
        zk.g2_msm_proj(curve, sc, np.zeros((5, 3 * NP), np.uint64))
    with pytest.raises(ValueError):  # mismatched lengths
        zk.g2_msm_proj(curve, sc, np.zeros((4, 6 * NP), np.uint64))
    with pytest.raises(ValueError):
        zk.g2_msm_proj(curve, sc[0], np.zeros((1, 6 * NP), np.uint64))
    with pytest.raises(ValueError):
        zk.g2_msm_proj(curve, np.zeros((5, 0), np.uint64), np.zeros((5, 6 * NP), np.uint64))
    with pytest.raises(ValueError):
        zk.g2_msm_variable(curve, sc, np.zeros((4, 4 * NP), np.uint64), 8)
    with pytest.raises(ValueError):
        zk.g2_msm_variable(curve, sc, np.zeros((5, 6 * NP), np.uint64), 8)
