"""The coset / batched NTT's surface without a GPU: the header declares zkg_ntt_ext_device and
zkg_ntt_ext with the stated parameter types, the library exports them, the Python mirror has the new
names, and the lazy-bound model of the shift paths (tools/lazy_bounds.py ntt_ext_paths) holds with
the constants the kernel source has.

What the model says about the forward shift: the loaded word times shift^j is a Montgomery product,
only known to be < 2p, and lds_dft does not take inputs that large -- with two inputs at 2p - 1 the
top limb of s23 in the first radix-4 round's fe_sub_lazy<4, 2> exceeds the borrowed top limb of 4p
by one, for every radix 2^2 .. 2^12 (2^1 has no such round and passes).  The kernel therefore
canonicalises the product before lds_put (the alternative the design allows), and the model checks
that step and the inverse shift's closing product for every radix instead."""
import importlib.util
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zkalgebra_gpu.h")
NTT_SRC = os.path.join(ROOT, "zikkurat-algebra_amd", "csrc", "zk_ntt.hip")
EXT_ARGS = ["int", "int", "int", "constuint64_t*", "constuint64_t*", "int", "constuint64_t*", "uint64_t*"]
FR_FIELDS = ["bn254_fr", "bls12_381_fr"]


def lazy_bounds():
    spec = importlib.util.spec_from_file_location("lazy_bounds", os.path.join(ROOT, "tools", "lazy_bounds.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def ptypes(proto):
    """parameter types of a prototype, names and spaces dropped"""
    args = proto[proto.index("(") + 1:proto.rindex(")")].split(",")
    return [re.sub(r"\w+$", "", a.strip()).replace(" ", "") for a in args]


def prototype(name):
    txt = open(HEADER).read()
    m = re.search(r"ZKG_API\s+([\w\s\*]+?)\b" + name + r"\s*(\([^;]*\));", txt)
    assert m, f"{name} is not declared in zkalgebra_gpu.h"
    return m.group(1).strip(), m.group(2)


@pytest.mark.parametrize("name", ["zkg_ntt_ext_device", "zkg_ntt_ext"])
def test_header_declares_ext_symbols(name):
    ret, args = prototype(name)
    assert ret == "int"
    assert ptypes(args) == EXT_ARGS


def test_library_exports_ext_symbols(zk):
    out = subprocess.check_output(["nm", "-D", "--defined-only", zk.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    want = {"zkg_ntt_ext_device", "zkg_ntt_ext", "zkg_ntt_ext_set_max_grid"}
    assert want <= exported, sorted(want - exported)
    assert want <= set(zk.EXTENSION_SYMBOLS)


def test_python_mirror_names(zk):
    for name in ("ntt_ext_device", "ntt_ext", "forward_ntt_batch", "inverse_ntt_batch", "coset_ntt", "coset_intt",
                 "ntt_ext_set_max_grid"):
        assert callable(getattr(zk, name)), name


def test_model_constants_are_the_kernels():
    lb = lazy_bounds()
    src = open(NTT_SRC).read()
    big = int(re.search(r"constexpr int NTT_TILE_BIG = (\d+);", src).group(1))
    assert big == 1 << lb.NTT_MAX_RADIX_LOG  # the largest DFT of one pass
    assert int(re.search(r"if \(m <= (\d+)\) \{ d\.push_back\(m\); return; \}", src).group(1)) == lb.NTT_ONE_PASS_MAX_LOG
    dft = src[src.index("void lds_dft("):src.index("struct PassArgs")]
    subs = re.findall(r"fe_sub_lazy<F, (\d+), (\d+)>", dft)
    assert subs == [tuple(str(v) for v in lb.NTT_DFT_SUB)]  # every other difference is the default <4, 1>
    hdr = open(os.path.join(ROOT, "zikkurat-algebra_amd", "csrc", "zk_field.hpp")).read()
    assert re.search(r"template <class F, int K = 4, int BW = 1>\s*__device__ __forceinline__ void fe_sub_lazy", hdr)
    # the pass body (shared by both kernels) canonicalises the shifted input and closes the inverse
    # shift through fe_store_ref
    ext = src[src.index("void ntt_pass_body("):src.index("k_sh_scale")]
    assert re.search(r"fe_mul\(y, x, w\);\s*fe_canon\(y\);", ext)
    assert re.search(r"tw2\(w, ext\.slo, ext\.shi, ext\.sh, \(uint32_t\)addr\);\s*fe_mul\(y, x, w\);\s*fe_store_ref", ext)
    # one body: one DFT call and one product-free closing loop in the file, behind both kernel names
    assert src.count("lds_dft<F, NT>(") == 1
    assert src.count("fe_reduce_small(x);") == 1
    for kernel in ("k_ntt_pass", "k_ntt_pass_ext"):
        assert re.search(r"__global__ void __launch_bounds__\(NT\)\s+" + kernel + r"\(", src), kernel


@pytest.mark.parametrize("field", FR_FIELDS)
def test_unreduced_product_is_not_a_dft_input(field):
    """< 2p inputs: accepted by the 2-point DFT only; every radix with a first radix-4 round rejects
    them, which is why the kernel reduces after the product"""
    lb = lazy_bounds()
    F = lb.Field(field)
    lb.ntt_lds_dft(F, 1, F.norm_val(2 * F.p))
    for r in range(2, lb.NTT_MAX_RADIX_LOG + 1):
        with pytest.raises(lb.BoundError, match="s23"):
            lb.ntt_lds_dft(F, r, F.norm_val(2 * F.p))
    for r in range(1, lb.NTT_MAX_RADIX_LOG + 1):  # what the kernel feeds it instead
        lb.ntt_lds_dft(F, r, F.norm_val(F.p))


@pytest.mark.parametrize("field", FR_FIELDS)
def test_shift_paths_hold(field):
    """the shifted input is < 2p (fe_canon's range) whatever 256-bit word was loaded, and the inverse
    shift's closing product is < 2p (fe_store_ref's range) after every DFT of 2^0 .. 2^12 points"""
    lb = lazy_bounds()
    F = lb.Field(field)
    xin, closing = lb.ntt_ext_paths(F)
    assert xin <= 2 * F.p and closing <= 2 * F.p
    assert F.checks > 1000
    assert lb.run_ext(verbose=False)


def test_model_rejects_a_twiddle_bounded_by_2p():
    """not vacuous: a shift power only known to be < 2p (instead of tw2's < 1.02p) after a
    2^12-point DFT would leave fe_store_ref's range"""
    lb = lazy_bounds()
    F = lb.Field("bls12_381_fr")
    out = lb.ntt_lds_dft(F, 12, F.norm_val(F.p))
    with pytest.raises(lb.BoundError):
        F.canon(F.mul(out, F.norm_val(2 * F.p)), "fe_store_ref")
