"""The G2 instantiation of the bucket pipeline (zk_msm_impl.hpp over Fp2: k_accum, the stitch levels,
k_ysum / k_ysum2 / k_ysum3<C,1>, k_jobsum_blk, k_fill_mark) against the reference's own C (oracle/_ref).

Default-window calls of at most BITS_MAX = 4096 pairs take the bit-job kernels and never run a
bucket, so every test here asserts `n > BITS_MAX or window` (bucket_path) before it calls the GPU.

Expected values.  The reference's G2 MSM costs 4 to 6 us per group addition on one host core, so a
test with many pairs runs them over FEW DISTINCT points: the GPU gets the whole list of n pairs
(idx[i] names the distinct row of pair i), the reference gets each distinct row once, with the sum
mod r (Python integers) of the scalars that the list pairs with it (ref_sum).  The points have order
r, so both are the same group element, and nothing the library under test computes enters the
expectation.  Repeated rows also make equal and opposite points meet inside the buckets, which
distinct points with random scalars never do."""
import numpy as np
import pytest

import golden_io

pytestmark = pytest.mark.gpu
CURVES = ["bn128", "bls12_381"]
NPS = {"bn128": 4, "bls12_381": 6}
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
BITS_MAX = 4096   # msm_bits_max(): the largest default-window n on the bit-job path
ND = 1 << 13      # distinct points per curve
REF_WINDOW_CAP = 12  # the reference's `_variable` above this window: see test_gpu_g2ext.py


def bucket_path(n, window=0):
    """the call about to be made runs the bucket pipeline: an explicit window (the `_variable` entry
    clamps any window into 4..24, the device entry any window >= 1), or more pairs than the bit jobs take"""
    assert n > BITS_MAX or window >= 1, (n, window)


# ---------------------------------------------------------------------------- reference side
def to_ints(a):
    b, w = np.ascontiguousarray(a).tobytes(), a.shape[1] * 8
    return [int.from_bytes(b[i * w:(i + 1) * w], "little") for i in range(a.shape[0])]


def from_ints(vals, nl=4):
    raw = b"".join(v.to_bytes(8 * nl, "little") for v in vals)
    return np.frombuffer(raw, dtype=np.uint64).reshape(len(vals), nl).copy()


def fr_convert(reference, curve, a, to_std):
    """<C>_arr_mont_to_std / _from_std of the reference"""
    out = np.zeros_like(a)
    reference.arr(curve, "arr_mont_to_std" if to_std else "arr_mont_from_std", a.shape[0], a, out)
    return out


def ref_entry(reference, curve, sc, pts, mont, affine):
    """<C>_G2_proj_MSM_{mont,std}_coeff_{affine,proj}_out on the rows as they are"""
    out = np.zeros((4 if affine else 6) * NPS[curve], np.uint64)
    name = f"G2_proj_MSM_{'mont' if mont else 'std'}_coeff_{'affine' if affine else 'proj'}_out"
    reference.arr(curve, name, sc.shape[0], sc, pts, out, sc.shape[1])
    return out


def ref_normalize(reference, curve, proj):
    out = np.zeros_like(proj)
    reference.arr(curve, "G2_proj_normalize", proj, out)
    return out


def ref_forms(reference, curve, proj):
    """(affine, normalised projective) of a raw projective result, by the reference's to_affine
    (what its `_affine_out` entries apply to the `_proj_out` value) and normalize"""
    aff = np.zeros(4 * NPS[curve], np.uint64)
    reference.arr(curve, "G2_proj_to_affine", proj, aff)
    return aff, ref_normalize(reference, curve, proj)


def aggregate(curve, std, idx, nbase):
    """scalar of distinct row j: the sum mod r of the std scalars std[i] with idx[i] == j"""
    r = golden_io.FR_ORDER[curve]
    agg = [0] * nbase
    for j, k in zip(idx.tolist(), to_ints(std)):
        agg[j] += k
    return from_ints([a % r for a in agg])


def ref_sum(reference, curve, std, base, idx, window=None):
    """sum_i std[i] * base[idx[i]] (raw projective): ONE reference MSM over the distinct rows `base`
    (its default std entry, or `_variable` at `window`)"""
    agg = aggregate(curve, std, idx, base.shape[0])
    if window is None:
        return ref_entry(reference, curve, agg, base, mont=False, affine=False)
    out = np.zeros(6 * NPS[curve], np.uint64)
    reference.arr(curve, "G2_proj_MSM_std_coeff_proj_out_variable", base.shape[0], agg, base, out, 4, window)
    return out


def ref_infinity(reference, curve):
    """(affine, projective) infinity as the reference sets them: all-0xFF and (0 : 1 : 0)"""
    aff, proj = np.zeros(4 * NPS[curve], np.uint64), np.zeros(6 * NPS[curve], np.uint64)
    reference.arr(curve, "G2_affine_set_infinity", aff)
    reference.arr(curve, "G2_proj_set_infinity", proj)
    NP = NPS[curve]
    assert np.all(aff == ONES) and not proj[:2 * NP].any() and proj[2 * NP:4 * NP].any() and not proj[4 * NP:].any()
    return aff, proj


# ---------------------------------------------------------------------------- inputs
@pytest.fixture(scope="module")
def points(reference):
    """2^13 distinct affine G2 points per curve, and the same rows with 1 in 97 at infinity"""
    out = {}
    for c in CURVES:
        p = golden_io.g2_points(reference.lib, c, ND)
        q = p.copy()
        q[::97] = ONES
        p.setflags(write=False)
        q.setflags(write=False)
        out[c] = (p, q)
    return out


def tiled(base, n, d):
    """n pairs over the first d rows of base: (rows, idx, the GPU's point list)"""
    rows = np.ascontiguousarray(base[:d])
    idx = np.arange(n) % d
    return rows, idx, np.ascontiguousarray(rows[idx])


def skewed_scalars(gpu, reference, curve, kind, n, seed):
    """(Montgomery, std) rows as _skewed_scalars of test_gpu_msm.py: "equal" one value, so one bucket
    per window holds every point; "binary" std 0 / 1; "mix3" three values and 5 % zeros; and "halves":
    three values in the first half, three others in the second, so the two splits of a host pipeline
    fill different buckets"""
    rng = np.random.default_rng(seed)
    if kind == "binary":
        std = np.zeros((n, 4), dtype=np.uint64)
        std[:, 0] = rng.integers(0, 2, n).astype(np.uint64)
        return fr_convert(reference, curve, std, to_std=False), std
    if kind == "equal":
        mont = np.tile(gpu.gen_fr(curve, seed, 1), (n, 1))
    elif kind == "mix3":
        mont = gpu.gen_fr(curve, seed, 3)[rng.integers(0, 3, n)].copy()
        mont[rng.random(n) < 0.05] = 0
    else:
        assert kind == "halves"
        vals = gpu.gen_fr(curve, seed, 6)
        pick = rng.integers(0, 3, n)
        pick[n // 2:] += 3
        mont = vals[pick].copy()
    return mont, fr_convert(reference, curve, mont, to_std=True)


def on_device(gpu, curve, sc, pts, **kw):
    ds, dp = gpu.DeviceBuffer(sc), gpu.DeviceBuffer(pts)
    try:
        return gpu.g2_msm_device(curve, sc.shape[0], ds, dp, nlimbs=sc.shape[1], **kw)
    finally:
        ds.free()
        dp.free()


# ---------------------------------------------------------------------------- 1. skewed scalars
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("kind", ["equal", "binary", "mix3"])
def test_g2_pipeline_skewed_default_window(gpu, reference, points, curve, kind):
    """20000 host pairs (c = 13) whose bucket runs cross chunk, wavefront, block and stitch-level
    boundaries, 1 point in 97 at infinity: all four host entries"""
    n, d = 20000, ND
    bucket_path(n)
    rows, idx, pts = tiled(points[curve][1], n, d)
    mont, std = skewed_scalars(gpu, reference, curve, kind, n, 1100)
    want_aff, want_proj = ref_forms(reference, curve, ref_sum(reference, curve, std, rows, idx))
    assert not np.all(want_aff == ONES)
    for sc, is_std in ((mont, False), (std, True)):
        assert np.array_equal(gpu.g2_msm(curve, sc, pts, std=is_std, affine=True), want_aff), is_std
        assert np.array_equal(gpu.g2_msm(curve, sc, pts, std=is_std, affine=False), want_proj), is_std


# ---------------------------------------------------------------------------- 2. equal and opposite points
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("kind", ["random", "random_runs", "equal", "equal_runs"])
def test_g2_pipeline_equal_and_opposite_points(gpu, reference, points, curve, kind):
    """2^15 pairs over 64 points and their negatives (rows P0, -P0, P1, -P1, ...): the doubling and the
    infinity branch of the Fp2 XYZZ additions.  With every scalar equal, P and -P share a bucket in
    every window and the sum is infinity: tiled, each bucket run goes P0, -P0 (infinity), P1, ...; as
    runs of two, P0, P0 (doubling), -P0, -P0 (infinity), P1, ...  "random_runs" gives each run of two
    equal rows one random scalar, so the two share a bucket in every window (neighbours wherever the
    sort keeps the input order, so a bucket run opens with a doubling), and the sum is a finite point"""
    n = 1 << 15
    bucket_path(n)
    NP = NPS[curve]
    rows = np.zeros((128, 4 * NP), np.uint64)
    rows[0::2] = points[curve][0][:64]
    for i in range(64):
        neg = np.zeros(4 * NP, np.uint64)
        reference.arr(curve, "G2_affine_neg", np.ascontiguousarray(rows[2 * i]), neg)
        rows[2 * i + 1] = neg
    assert np.array_equal(rows[0::2, :2 * NP], rows[1::2, :2 * NP]) and not np.array_equal(rows[0::2], rows[1::2])
    idx = (np.arange(n) // 2) % 128 if kind.endswith("_runs") else np.arange(n) % 128
    pts = np.ascontiguousarray(rows[idx])
    if kind == "random":
        mont = gpu.gen_fr(curve, 1200, n)
    elif kind == "random_runs":
        mont = np.ascontiguousarray(np.repeat(gpu.gen_fr(curve, 1202, n // 2), 2, axis=0))
    else:
        mont = np.tile(gpu.gen_fr(curve, 1201, 1), (n, 1))
    std = fr_convert(reference, curve, mont, to_std=True)
    agg = aggregate(curve, std, idx, 128)
    want_aff = ref_entry(reference, curve, fr_convert(reference, curve, agg, to_std=False), rows, True, True)
    want_proj = ref_normalize(reference, curve, ref_entry(reference, curve, agg, rows, False, False))
    if kind.startswith("equal"):
        inf_aff, inf_proj = ref_infinity(reference, curve)
        assert np.array_equal(want_aff, inf_aff) and np.array_equal(want_proj, inf_proj)
    else:
        assert not np.all(want_aff == ONES)
    assert np.array_equal(gpu.g2_msm(curve, mont, pts, affine=True), want_aff)
    assert np.array_equal(gpu.g2_msm(curve, mont, pts, affine=False), want_proj)
    assert np.array_equal(gpu.g2_msm(curve, std, pts, std=True, affine=True), want_aff)


# ---------------------------------------------------------------------------- 3. window sweep
@pytest.fixture(scope="module")
def sweep(gpu, reference, points):
    """one scalar set per curve for the window sweep (8192 pairs over 1024 rows, infinities among the
    rows, zero scalars) and the reference's `_variable` results by window, each computed once"""
    n, d = 8192, 1024
    out = {}
    for c in CURVES:
        rows, idx, pts = tiled(points[c][1], n, d)
        std = fr_convert(reference, c, gpu.gen_fr(c, 1300, n), to_std=True)
        std[::61] = 0
        out[c] = {"rows": rows, "idx": idx, "pts": pts, "std": std, "want": {}}
    return out


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("window", [1, 4, 9, 11, 12, 13, 16, 20, 24, 30])
def test_g2_pipeline_window_sweep(gpu, reference, sweep, curve, window):
    """8192 pairs, so the buckets of the small windows hold many points: k_ysum below c = 12, the
    block-level Y sums from 12 up, the mostly-empty large windows, and the clamp of 1 and 30"""
    s = sweep[curve]
    n = s["std"].shape[0]
    bucket_path(n, window)
    rw = min(window, REF_WINDOW_CAP)
    if rw not in s["want"]:
        s["want"][rw] = ref_normalize(reference, curve,
                                      ref_sum(reference, curve, s["std"], s["rows"], s["idx"], window=rw))
    got = gpu.g2_msm_variable(curve, s["std"], s["pts"], window)
    assert np.array_equal(ref_normalize(reference, curve, got), s["want"][rw])


# ---------------------------------------------------------------------------- 4. past the bit-job limit
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", [4096, 4097, 8191, 8192])
def test_g2_pipeline_default_window_past_bit_jobs(gpu, reference, points, curve, n):
    """the default entries on both sides of the bit-job limit: 4096 is the last bit-job size, 4097
    and 8191 run the buckets at c = 10, 8192 at c = 13"""
    if n > BITS_MAX:
        bucket_path(n)
    rows, idx, pts = tiled(points[curve][1], n, 2048)
    mont = gpu.gen_fr(curve, 1400 + n, n)
    mont[::53] = 0
    std = fr_convert(reference, curve, mont, to_std=True)
    want_aff, want_proj = ref_forms(reference, curve, ref_sum(reference, curve, std, rows, idx))
    assert np.array_equal(gpu.g2_msm(curve, mont, pts, affine=True), want_aff)
    assert np.array_equal(gpu.g2_msm(curve, std, pts, std=True, affine=False), want_proj)


# ---------------------------------------------------------------------------- 5. window groups
@pytest.fixture(scope="module")
def groups_case(gpu, reference, points):
    n, d = 4000, 1000
    out = {}
    for c in CURVES:
        rows, idx, pts = tiled(points[c][1], n, d)
        std = fr_convert(reference, c, gpu.gen_fr(c, 1500, n), to_std=True)
        out[c] = (std, pts, ref_normalize(reference, c, ref_sum(reference, c, std, rows, idx)))
    return out


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("window,limit", [(4, 3 * 4000), (9, 4000), (16, 1)])
def test_g2_pipeline_window_groups(gpu, reference, groups_case, curve, window, limit):
    """the windows in several pipeline passes (by default from W n >= 2^30 sorted entries)"""
    std, pts, want = groups_case[curve]
    bucket_path(std.shape[0], window)
    try:
        gpu.msm_set_group_limit(limit)
        got = gpu.g2_msm_variable(curve, std, pts, window)
        groups = gpu.msm_last_groups()
    finally:
        gpu.msm_set_group_limit(0)
    assert groups > 1
    assert np.array_equal(ref_normalize(reference, curve, got), want)


# ---------------------------------------------------------------------------- 6. sort-ahead
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("window,n", [(0, 5000), (13, 9001), (16, 20000)])
def test_g2_pipeline_sort_ahead(gpu, reference, points, curve, window, n):
    """two window groups sorted ahead on the sort stream (the test hook applies to every field),
    the plain pipeline and the default, device-resident: each equal to the reference"""
    bucket_path(n, window)
    rows, idx, pts = tiled(points[curve][1], n, 2048)
    mont = gpu.gen_fr(curve, 1600 + window, n)
    std = fr_convert(reference, curve, mont, to_std=True)
    want = ref_normalize(reference, curve, ref_sum(reference, curve, std, rows, idx))
    ds, dp = gpu.DeviceBuffer(mont), gpu.DeviceBuffer(pts)
    try:
        gpu.msm_set_ahead_min(12)
        two = gpu.g2_msm_device(curve, n, ds, dp, window=window)
        groups = gpu.msm_last_groups()
        gpu.msm_set_ahead_min(0)
        one = gpu.g2_msm_device(curve, n, ds, dp, window=window)
        gpu.msm_set_ahead_min(-1)
        dflt = gpu.g2_msm_device(curve, n, ds, dp, window=window)
    finally:
        gpu.msm_set_ahead_min(-1)
        ds.free()
        dp.free()
    assert groups == 2
    assert np.array_equal(two, want)
    assert np.array_equal(one, want)
    assert np.array_equal(dflt, want)
    assert np.array_equal(one, two) and np.array_equal(one, dflt)


# ---------------------------------------------------------------------------- 7. two-split host pipeline
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("kind", ["equal", "mix3", "halves"])
def test_g2_pipeline_two_host_splits(gpu, reference, points, curve, kind):
    """2^17 host pairs run as two splits: a bucket run of the second split starts from the first
    split's sum where that split filled the bucket (k_fill_mark / start_run), from infinity where
    it did not, and the Y sums take every bucket either split filled.  "halves" gives the splits
    disjoint buckets, and runs with the halves exchanged first -- the same sum, since half the
    length is a multiple of the 2^13 rows -- so the flags that call leaves in the workspace are wrong
    for the second"""
    n = 1 << 17
    bucket_path(n)
    rows, idx, pts = tiled(points[curve][1], n, ND)
    mont, std = skewed_scalars(gpu, reference, curve, kind, n, 1700)
    want_aff, want_proj = ref_forms(reference, curve, ref_sum(reference, curve, std, rows, idx))
    if kind == "halves":
        assert (n // 2) % ND == 0
        swapped = np.ascontiguousarray(np.roll(mont, n // 2, axis=0))
        assert np.array_equal(gpu.g2_msm(curve, swapped, pts, affine=True), want_aff)
    assert np.array_equal(gpu.g2_msm(curve, mont, pts, affine=True), want_aff)
    assert np.array_equal(on_device(gpu, curve, mont, pts), want_proj)  # one unsplit pass


# ---------------------------------------------------------------------------- 8. scalar widths
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("nl,high", [(5, "zero"), (5, "random"), (6, "random"), (9, "random")])
def test_g2_pipeline_std_wide_scalars(gpu, reference, points, curve, nl, high):
    """std rows of more than 4 limbs are used verbatim (one device MSM per 256-bit slice, Horner with
    the host's Fp2 xyzz_dbl), through the buckets (explicit window) and through the default entry"""
    n, window = 300, 7
    bucket_path(n, window)
    pts = np.ascontiguousarray(points[curve][1][:n])
    rng = np.random.default_rng(nl * 10 + (high == "random"))
    sc = np.zeros((n, nl), dtype=np.uint64)
    sc[:, :4] = gpu.gen_fr(curve, 1800 + nl, n)
    if high == "random":
        sc[:, 4:] = rng.integers(0, 1 << 64, size=(n, nl - 4), dtype=np.uint64)
    want_aff, want_proj = ref_forms(reference, curve, ref_entry(reference, curve, sc, pts, False, False))
    got = gpu.g2_msm_variable(curve, sc, pts, window)
    assert np.array_equal(ref_normalize(reference, curve, got), want_proj)
    assert np.array_equal(on_device(gpu, curve, sc, pts, mont=False, window=window), want_proj)
    assert np.array_equal(gpu.g2_msm(curve, sc, pts, std=True, affine=True), want_aff)
    if high == "zero":
        sc4 = np.ascontiguousarray(sc[:, :4])
        assert np.array_equal(ref_entry(reference, curve, sc4, pts, False, True), want_aff)
        got4 = gpu.g2_msm_variable(curve, sc4, pts, window)
        assert np.array_equal(ref_normalize(reference, curve, got4), want_proj)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("nl", [1, 2, 3, 5])
def test_g2_pipeline_mont_other_nlimbs(gpu, reference, points, curve, nl):
    """Montgomery rows with expo_nlimbs != 4 (undefined in the reference, which reads 4 limbs per
    row): the value of the row's first min(nl, 4) limbs, as for G1, and no abort.  Expected: the
    reference on the rows zero-extended or truncated to 4 limbs"""
    n, window = 300, 8
    bucket_path(n, window)
    pts = np.ascontiguousarray(points[curve][1][:n])
    base = gpu.gen_fr(curve, 1900, n)
    k = min(nl, 4)
    sc = np.zeros((n, nl), dtype=np.uint64)
    sc[:, :k] = base[:, :k]
    ext = np.zeros((n, 4), dtype=np.uint64)
    ext[:, :k] = base[:, :k]
    want_aff, want_proj = ref_forms(reference, curve, ref_entry(reference, curve, ext, pts, True, False))
    assert np.array_equal(on_device(gpu, curve, sc, pts, window=window), want_proj)
    assert np.array_equal(on_device(gpu, curve, ext, pts, window=window), want_proj)
    assert np.array_equal(gpu.g2_msm(curve, sc, pts, affine=True), want_aff)
    assert gpu.last_error() is None


# ---------------------------------------------------------------------------- 9. empty and all-infinity input
@pytest.mark.parametrize("curve", CURVES)
def test_g2_pipeline_empty_input(gpu, reference, curve):
    """n = 0 through the explicit-window entries and the default ones: infinity in the reference's form"""
    inf_aff, inf_proj = ref_infinity(reference, curve)
    sc, pts = np.zeros((0, 4), np.uint64), np.zeros((0, 4 * NPS[curve]), np.uint64)
    bucket_path(0, 8)
    got = gpu.g2_msm_variable(curve, sc, pts, 8)
    assert np.array_equal(ref_normalize(reference, curve, got), inf_proj)
    assert np.array_equal(on_device(gpu, curve, sc, pts, window=8), inf_proj)
    assert np.array_equal(gpu.g2_msm(curve, sc, pts, affine=True), inf_aff)
    assert np.array_equal(gpu.g2_msm(curve, sc, pts, affine=False), inf_proj)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n,window", [(300, 8), (300, 13), (4097, 0)])
def test_g2_pipeline_all_infinity_input(gpu, reference, curve, n, window):
    """every point at infinity: k_accum skips every entry, every bucket run stores infinity, and the
    stitch, the Y sums and the job sums add nothing but infinities"""
    bucket_path(n, window)
    inf_aff, inf_proj = ref_infinity(reference, curve)
    pts = np.full((n, 4 * NPS[curve]), ONES, np.uint64)
    mont = gpu.gen_fr(curve, 2000, n)
    std = fr_convert(reference, curve, mont, to_std=True)
    want_aff, want_proj = ref_forms(reference, curve,
                                    ref_sum(reference, curve, std, pts[:1], np.zeros(n, np.int64)))
    assert np.array_equal(want_aff, inf_aff) and np.array_equal(want_proj, inf_proj)
    if window:
        got = gpu.g2_msm_variable(curve, std, pts, window)
        assert np.array_equal(ref_normalize(reference, curve, got), want_proj)
        assert np.array_equal(on_device(gpu, curve, mont, pts, window=window), want_proj)
    else:
        assert np.array_equal(gpu.g2_msm(curve, mont, pts, affine=True), want_aff)
        assert np.array_equal(gpu.g2_msm(curve, std, pts, std=True, affine=False), want_proj)
