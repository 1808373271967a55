"""bench.py's command line: a plain run prints the headline line only and --dump-outputs writes
the last timed step's columns; --full adds the side measurements."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDE_KEYS = {"roofline", "hbm_copy_peak", "end_to_end", "reference_stream", "operator_ic", "cpu_baseline",
             "ppf_sweep", "kernels_standalone"}


def _bench(*args):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args],
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_is_lean_and_dumps_the_last_timed_step(gpu, tmp_path):
    """rows above the dump's row budget (131 072 at d = 32): the file holds the seeded row sample
    of the step with seed `--seed + warmup + steps - 1`, bit for bit what the same call gives
    in this process."""
    import bench
    from oracle.pipeline import cfg3_corr, cfg_dists
    from probabilit_amd.modeling import Distribution, NoOp

    rows, steps, warmup, seed = 150_001, 2, 1, 3
    line = _bench("--rows", str(rows), "--steps", str(steps), "--warmup", str(warmup), "--seed", str(seed),
                  "--dump-outputs", str(tmp_path))
    assert not SIDE_KEYS & set(line), sorted(line)
    assert line["steps"] == steps and line["warmup"] == warmup and line["config"]["rows"] == rows
    assert line["unit"] == "Msamples/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["ms_per_step"] > 0
    # value is N x d draws over the step time, both rounded in the line
    assert line["value"] == pytest.approx(rows * 32 / (line["ms_per_step"] / 1e3) / 1e6, rel=1e-3)
    assert line["kernels"]

    assert os.listdir(tmp_path) == ["samples.npy"]
    got = np.load(tmp_path / "samples.npy")
    keep = bench.DUMP_BYTES // (8 * 32)
    assert got.dtype == np.float64 and got.shape == (keep, 32) and got.nbytes <= 64_000_000
    ds = [Distribution(name, **kw) for name, kw in cfg_dists(32)]
    NoOp(*ds).correlate(*ds, corr_mat=cfg3_corr(32)).sample_device(rows, random_state=seed + warmup + steps - 1,
                                                                  method="lhs")
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(rows, size=keep, replace=False))
    want = np.stack([x.samples_device.cpu().numpy()[idx] for x in ds], axis=1)
    np.testing.assert_array_equal(got, want)


def test_full_run_adds_the_side_measurements(gpu):
    small = "100000"
    line = _bench("--full", "--rows", "150001", "--steps", "1", "--warmup", "1", "--cpu-n", "20000", "--ppf-rows", small,
                  "--operator-rows", small, "--refstream-rows", small)
    assert SIDE_KEYS <= set(line), sorted(line)
    for key in SIDE_KEYS:
        assert line[key], key
    assert line["roofline"]["kernel"] in line["kernels_standalone"]
    assert "kernel_time_ms_per_step" in line["pipeline_roofline"]
