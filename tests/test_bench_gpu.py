"""bench.py on the GPU, in process at a tiny shape: a plain run reports the headline figure alone
and --dump-outputs writes what its last timed step computed; --full adds the other measurements."""
import json
import os

import numpy as np
import pytest

import bench
from oracle import keras_ops as K

SHAPE = ["--size", "64", "--batch", "2", "--steps", "2", "--warmup", "1"]
MOVED = ("roofline", "op_breakdown", "encoder_blocks", "cpu_baseline", "data_parallel")


def _run(capsys, *extra):
    capsys.readouterr()
    bench.main(SHAPE + list(extra))
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_reports_the_headline_only_and_dumps_its_outputs(tmp_path, capsys):
    d = tmp_path / "dump"
    out = _run(capsys, "--dump-outputs", str(d))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup"):
        assert k in out, k
    assert not [k for k in MOVED if k in out], out
    assert out["steps"] == 2 and out["warmup"] == 1 and out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(2 * 2 / (2 * out["ms_per_step"] * 1e-3), rel=1e-3)
    files = sorted(os.listdir(d))
    assert files == ["bn_moving_stats.npy", "mean_io_u_confusion.npy", "prob.npy", "train_step.npy", "weights.npy"]
    arrs = {f[:-4]: np.load(d / f, allow_pickle=False) for f in files}
    assert sum(a.nbytes for a in arrs.values()) <= 64 * 10 ** 6
    for name, a in arrs.items():
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        assert np.isfinite(a).all(), name
    assert arrs["train_step"].shape == (3,) and arrs["prob"].shape == (2, 64, 64, 1)
    assert float(arrs["train_step"][0]) == pytest.approx(out["final_loss"], abs=1e-6)
    assert 0.0 <= arrs["prob"].min() and arrs["prob"].max() <= 1.0
    # every pixel of warm-up + timed steps is counted once
    assert arrs["mean_io_u_confusion"].sum() == 3 * 2 * 64 * 64
    # the loss of the dumped probabilities against the run's (seeded) masks is the dumped loss
    _, y = bench.synthetic_batch(2, 64, 64, 1, 2301, "cpu")
    # (float64 oracle; the kernel sums 64 x 64 float32 terms per image by tree reduction: a few ulp)
    dice = K.dice_coef(y.numpy().astype(np.float64), arrs["prob"].astype(np.float64))
    assert float(arrs["train_step"][1]) == pytest.approx(dice, abs=1e-5)


@pytest.mark.gpu
def test_full_run_adds_the_other_measurements(capsys):
    out = _run(capsys, "--full", "--no-cpu-baseline", "--encoder-batch", "2")
    for k in ("roofline", "op_breakdown", "encoder_blocks"):
        assert k in out, k
    assert out["ms_per_step"] > 0 and out["steps"] == 2
