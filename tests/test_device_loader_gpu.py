"""DevicePairLoader on the GPU (unet_amd/device_data.py): behind the Prefetcher its batches are
bitwise PairLoader's, a fit fed by it leaves the same history and the same weights (the train step
is bit-deterministic, test_carried_state_gpu.py), and scripts/train.py --device_loader trains."""
import os
import sys

import numpy as np
import pytest
from PIL import Image

torch = pytest.importorskip("torch")

from unet_amd.data import PairLoader  # noqa: E402
from unet_amd.device_data import DevicePairLoader  # noqa: E402
from unet_amd.prefetch import Prefetcher  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "unet-image-segmentation_amd", "scripts")
DEV = "cuda:0"
N, SIZE, BATCH = 12, (32, 32), 4
PAIR_BYTES = SIZE[0] * SIZE[1] * 4


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """12 PNG pairs of 40 x 30 (frames of noise, masks with every grey level), as test_data_host writes them."""
    root = str(tmp_path_factory.mktemp("pairs"))
    fr, mk = os.path.join(root, "frames"), os.path.join(root, "masks")
    os.makedirs(fr)
    os.makedirs(mk)
    rng = np.random.default_rng(0)
    for i in range(N):
        Image.fromarray(rng.integers(0, 256, (30, 40, 3), dtype=np.uint8)).save(os.path.join(fr, f"f{i:03d}.png"))
        m = np.zeros((30, 40), np.uint8)
        m[5:5 + i % 7 + 3, 4:20] = 255
        m[20:25, 2:30] = rng.integers(0, 256, (5, 28), dtype=np.uint8)
        Image.fromarray(m).save(os.path.join(mk, f"f{i:03d}.png"))
    return fr, mk


def _pair(tree, budget, **kw):
    kw = dict(dict(seed=2301, shuffle=True, horizontal_flip=True, workers=4), **kw)
    return (PairLoader(*tree, SIZE, BATCH, **kw),
            DevicePairLoader(*tree, SIZE, BATCH, device=DEV, device_cache_bytes=budget, **kw))


@pytest.mark.parametrize("budget", [None, 3 * PAIR_BYTES], ids=["full", "three"])
def test_prefetched_batches_equal_the_host_loaders(tree, budget):
    host, dev = _pair(tree, budget)
    assert dev.book.resident == (N if budget is None else 3)
    hp, dp = Prefetcher(host, DEV), Prefetcher(dev, DEV)
    hi, di = iter(hp), iter(dp)
    try:
        for k in range(3 * (N // BATCH)):
            a, b = next(hi), next(di)
            assert a.global_size == b.global_size == BATCH
            for u, v in zip(a, b):
                assert v.is_cuda and v.dtype == torch.float32 and v.is_contiguous()
                assert torch.equal(u, v), k
    finally:
        hp.close()
        dp.close()
    if budget is None:  # every sample went up once; later batches uploaded slot entries only
        assert dev.store.uploaded_bytes == N * PAIR_BYTES


def test_prefetcher_limit_restarts_the_pass(tree):
    """model.evaluate's use: Prefetcher(loader, limit=k) per call, each a fresh pass; the cache persists."""
    host, dev = _pair(tree, None, shuffle=False, horizontal_flip=False)
    want = [tuple(torch.from_numpy(a) for a in s) for s, _ in zip(iter(host), range(2))]
    for _ in range(2):
        got = list(Prefetcher(dev, DEV, limit=2))
        assert len(got) == 2
        for w, g in zip(want, got):
            assert torch.equal(w[0], g[0].cpu()) and torch.equal(w[1], g[1].cpu())
    assert dev.store.uploaded_bytes == 2 * BATCH * PAIR_BYTES


def test_fit_is_the_same_with_either_loader(tree):
    from helpers import trace_model
    cfg = (SIZE + (3,), 1, True, 0.0, {})
    out = []
    for which in (0, 1):
        model = trace_model(cfg)
        train = _pair(tree, None)[which]
        val = _pair(tree, None, shuffle=False, horizontal_flip=False)[which]
        hist = model.fit(train, epochs=2, steps_per_epoch=3, validation_data=val, validation_steps=2, verbose=0)
        out.append((hist.history, model.get_weights()))
    (h0, w0), (h1, w1) = out
    assert h0 == h1 and set(h0) >= {"loss", "val_loss"} and len(h0["loss"]) == 2
    assert len(w0) == len(w1)
    for a, b in zip(w0, w1):
        assert np.array_equal(a, b)


def test_train_cli_device_loader(tmp_path, capsys):
    sys.path[:0] = [p for p in (SCRIPTS, os.path.join(ROOT, "tools")) if p not in sys.path]
    from bench_loader import make_midv_tree
    make_midv_tree(str(tmp_path), 8, 4)
    import train
    out = tmp_path / "models" / "model.h5"
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        train.main(["--epochs", "1", "--batch-size", "4", "--model-out", str(out), "--dataset-root", str(tmp_path),
                    "--device_loader"])
    finally:
        os.chdir(cwd)
    text = capsys.readouterr().out
    assert "Found 8 training samples and 4 validation samples." in text
    assert "Steps per epoch: 2, Validation steps: 1" in text
    assert "Epoch 1/1" in text and os.path.isfile(out)
