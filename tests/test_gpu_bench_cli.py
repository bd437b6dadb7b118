"""bench.py on the GPU at a small size: a plain run times the headline MSM alone and prints one
JSON line; --dump-outputs writes the last timed step's result; the secondary lines appear only
with --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG_N = 13  # above the small-input (bit-job) path's 4096 pairs: the bucket pipeline of the headline
SECONDARY = ("config5", "ntt", "config4", "end_to_end", "msm_sizes", "group_fft", "group_fft_kzg", "cpu_baseline")


def _bench(args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--log-n", str(LOG_N)] + args,
                       env=env, capture_output=True, text=True, timeout=100, cwd=ROOT)
    assert p.returncode == 0, p.stderr
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_times_the_headline_only_and_dumps_its_output(gpu, tmp_path):
    out = tmp_path / "dump"
    r = _bench(["--steps", "3", "--warmup", "1", "--dump-outputs", str(out)])
    assert r["steps"] == 3 and r["warmup"] == 1
    assert r["unit"] == "pairs/s" and r["higher_is_better"] is True
    assert r["ms_per_step"] > 0
    assert r["value"] == pytest.approx((1 << LOG_N) / (r["ms_per_step"] * 1e-3))
    assert not [k for k in SECONDARY if k in r]
    assert os.listdir(out) == ["msm_affine.npy"]
    words = np.load(out / "msm_affine.npy")
    assert words.dtype == np.float64 and words.shape == (2 * 2 * gpu.NLIMBS_P["bls12_381"],)
    w = words.astype(np.uint64)
    assert np.array_equal(w.astype(np.float64), words) and int(w.max()) < 1 << 32
    n = 1 << LOG_N
    want = gpu.msm_affine("bls12_381", gpu.gen_fr("bls12_381", 0x5A4B0002, n), gpu.gen_points("bls12_381", 0x5A4B0002, n))
    assert np.array_equal(w[0::2] | (w[1::2] << np.uint64(32)), want)


def test_full_adds_the_secondary_lines(gpu):
    r = _bench(["--steps", "2", "--warmup", "1", "--full", "--ntt-log", "12", "--ntt-steps", "1", "--no-config5",
                "--no-config4", "--no-e2e", "--no-extras", "--no-cpu-baseline"])
    assert r["steps"] == 2 and r["ms_per_step"] > 0
    assert r["ntt"]["parity_vs_reference"]["roundtrip_exact"] is True
    assert [k for k in SECONDARY if k in r] == ["ntt"]
