"""The pairing fixtures, the big-integer model and the host side of the pairing entry points.  CPU only.

tests/golden/pairing_<curve>.npz (tools/make_golden.py pairing) holds rows ([a] g1, [b] g2) with the
reference's <C>_pairing_affine of each, and random Fp12 rows with its <C>_pairing_final_expo."""
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import pairing_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = ("bn128", "bls12_381")
REF_NAMES = [f"{c}_pairing_{k}" for c in CURVES for k in ("affine", "projective")]
EXT_NAMES = [f"zkg_pairing_{k}{d}" for k in ("rows", "product", "final_expo") for d in ("", "_device")]


@pytest.fixture(scope="module")
def golden():
    return {c: np.load(os.path.join(ROOT, "tests", "golden", f"pairing_{c}.npz")) for c in CURVES}


def words(row):
    return [int(x) for x in row]


# ---------------------------------------------------------------------------- the fixtures themselves

@pytest.mark.parametrize("curve", CURVES)
def test_golden_bilinearity(golden, curve):
    g, T = golden[curve], pm.tower(curve)
    fam, out = g["family"], g["pairing"]
    assert out.shape[0] <= 48 and out.shape[1] == 12 * T.NP
    one = T.to_words(T.one())
    seen = {}
    for i in range(out.shape[0]):
        if fam[i] < 0:
            continue
        key = out[i].tobytes()
        assert seen.setdefault(key, fam[i]) == fam[i], "rows of different families differ"
        for j in range(i):
            if fam[j] == fam[i]:
                assert np.array_equal(out[i], out[j]), "rows of one family are bit-equal"
        assert words(out[i]) != one
    assert max(np.bincount(fam[fam >= 0])) >= 4
    for i in g["infinity"]:
        assert words(out[i]) == one
    a, b = (T.from_words(words(out[i])) for i in g["twin"])
    assert T.mul(a, b) == T.one()


# ---------------------------------------------------------------------------- the model

@pytest.mark.parametrize("curve", CURVES)
def test_model_equals_golden(golden, curve):
    g, T = golden[curve], pm.tower(curve)
    n = g["pairing"].shape[0]
    for i in (0, 4, n - 8, int(g["twin"][1]), int(g["infinity"][0])):
        assert T.pairing_words(words(g["P"][i]), words(g["Q"][i])) == words(g["pairing"][i]), i
    for i in (0, 7):
        assert T.to_words(T.final_expo(T.from_words(words(g["fe_src"][i])))) == words(g["fe_out"][i])


@pytest.mark.parametrize("curve", CURVES)
def test_kernel_programs_equal_golden(golden, curve):
    """the instruction streams the kernel interprets (zk_pairing_prog.inc), run on big integers"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_pairing_prog as gp
    with open(os.path.join(ROOT, "zikkurat-algebra_amd", "csrc", "zk_pairing_prog.inc")) as f:
        text = f.read()
    assert text == gp.render(), "zk_pairing_prog.inc is not what tools/gen_pairing_prog.py writes"
    progs = {}
    for kind in ("miller", "fexp"):
        m = re.search(r"ZK_PAIR_PROG_%s_%s\[\] = \{(.*?)\};" % (curve.upper(), kind.upper()), text, re.S)
        progs[kind] = [int(w.rstrip("u"), 16) for w in re.findall(r"0x[0-9a-f]+u", m.group(1))]
    g, T = golden[curve], pm.tower(curve)
    consts = pm.program_consts(T)
    for i in (1, 5, g["pairing"].shape[0] - 6, int(g["twin"][0])):
        P, Q = T.g1_from_words(words(g["P"][i])), T.g2_from_words(words(g["Q"][i]))
        cells = [(0, 0)] * gp.NCELL
        cells[gp.XP], cells[gp.YP], cells[gp.QX], cells[gp.QY] = (P[0], 0), (P[1], 0), Q[0], Q[1]
        pm.run_program(T, progs["miller"] + progs["fexp"], cells, gp.OPS, consts)
        assert T.to_words(cells[0:6]) == words(g["pairing"][i]), i
    for i in range(8):
        cells = [(0, 0)] * gp.NCELL
        cells[0:6] = T.from_words(words(g["fe_src"][i]))
        pm.run_program(T, progs["fexp"], cells, gp.OPS, consts)
        assert T.to_words(cells[0:6]) == words(g["fe_out"][i]), i


# ---------------------------------------------------------------------------- the host side

def test_names_are_declared_and_exported(zk):
    with open(os.path.join(ROOT, "include", "zkalgebra_gpu.h")) as f:
        header = f.read()
    lib = zk.load()
    for name in REF_NAMES + EXT_NAMES:
        assert name in (zk.REFERENCE_SYMBOLS if name in REF_NAMES else zk.EXTENSION_SYMBOLS), name
        assert re.search(r"ZKG_API\s+\w+\s+%s\(" % name, header), name
        assert hasattr(lib, name), name
    for name in ("pairing", "pairing_product", "final_expo"):
        assert callable(getattr(zk, name)) and callable(getattr(zk, name + "_device")), name
    for name in ("pairing_projective", "pairing_check", "kzg_verify"):
        assert callable(getattr(zk, name)), name


@pytest.mark.parametrize("curve", CURVES)
def test_shape_checks_raise_without_a_gpu(zk, curve):
    n1 = zk.NLIMBS_P[curve]
    z = lambda *s: np.zeros(s, dtype=np.uint64)
    with pytest.raises(ValueError):
        zk.pairing(curve, z(2 * n1), z(2 * n1))  # a G1 row where a G2 row belongs
    with pytest.raises(ValueError):
        zk.pairing(curve, z(3, 2 * n1), z(2, 4 * n1))
    with pytest.raises(ValueError):
        zk.pairing_product(curve, z(3, 3 * n1), z(3, 4 * n1))
    with pytest.raises(ValueError):
        zk.pairing_check(curve, z(2, 2 * n1), z(2, 6 * n1))
    with pytest.raises(ValueError):
        zk.pairing_projective(curve, z(2 * n1), z(6 * n1))
    with pytest.raises(ValueError):
        zk.final_expo(curve, z(2, 6 * n1))
    with pytest.raises(ValueError):
        zk.kzg_verify(curve, z(2 * n1), z(4 * n1), z(4 * n1), z(2 * n1), z(4), z(4), z(3 * n1))
    with pytest.raises(TypeError):
        zk.kzg_verify(curve, z(2 * n1), z(4 * n1), z(4 * n1), z(3 * n1), z(3), z(4), z(3 * n1))


@pytest.mark.parametrize("curve", CURVES)
def test_fp12_one(zk, curve):
    T = pm.tower(curve)
    assert words(zk.fp12_one(curve)) == T.to_words(T.one())
