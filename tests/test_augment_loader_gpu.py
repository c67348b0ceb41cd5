"""The augmented DevicePairLoader on the GPU (unet_amd/device_data.py with an augment.Augment): behind
the Prefetcher its batches are bitwise the augmented PairLoader's, a fit fed by it leaves the same
history and weights, the warp launches on the loader's side stream are ordered against the train
step by the shard's event alone (tests/hazards.py), and scripts/train.py takes the Keras flags."""
import os
import sys

import numpy as np
import pytest
from PIL import Image

torch = pytest.importorskip("torch")

import hazards as H  # noqa: E402
from unet_amd.augment import Augment  # noqa: E402
from unet_amd.data import PairLoader  # noqa: E402
from unet_amd.device_data import DevicePairLoader  # noqa: E402
from unet_amd.prefetch import Prefetcher  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "unet-image-segmentation_amd", "scripts")
DEV = "cuda:0"
N, SIZE, BATCH = 12, (32, 32), 4
PAIR_BYTES = SIZE[0] * SIZE[1] * 4
AUG = dict(rotation_range=30, width_shift_range=0.2, height_shift_range=0.2, shear_range=15, zoom_range=(0.7, 1.3))


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """12 PNG pairs of 40 x 30 (frames of noise, masks with every grey level), as test_device_loader_gpu writes them."""
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


def _pair(tree, budget, aug=None, **kw):
    kw = dict(dict(seed=2301, shuffle=True, horizontal_flip=True, workers=4), **kw)
    aug = AUG if aug is None else aug
    return (PairLoader(*tree, SIZE, BATCH, augment=Augment(**aug), **kw),
            DevicePairLoader(*tree, SIZE, BATCH, device=DEV, device_cache_bytes=budget, augment=Augment(**aug), **kw))


@pytest.mark.parametrize("aug", [AUG, dict(AUG, fill_mode="constant", cval=128.0, mask_order=0)], ids=["nearest", "constant"])
@pytest.mark.parametrize("budget", [None, 3 * PAIR_BYTES], ids=["full", "three"])
def test_prefetched_batches_equal_the_host_loaders(tree, budget, aug):
    host, dev = _pair(tree, budget, aug)
    assert dev.book.resident == (N if budget is None else 3)
    plain = iter(PairLoader(*tree, SIZE, BATCH, seed=2301, shuffle=True, horizontal_flip=True, workers=4))
    hp, dp = Prefetcher(host, DEV), Prefetcher(dev, DEV)
    hi, di = iter(hp), iter(dp)
    changed = 0
    try:
        for k in range(3 * (N // BATCH)):
            a, b = next(hi), next(di)
            assert a.global_size == b.global_size == BATCH
            for u, v in zip(a, b):
                assert v.is_cuda and v.dtype == torch.float32 and v.is_contiguous()
                assert torch.equal(u, v), k
            changed += not np.array_equal(next(plain)[0], b[0].cpu().numpy())
    finally:
        hp.close()
        dp.close()
    assert changed == 3 * (N // BATCH), "augmentation must change every batch"
    if budget is None:  # every sample went up once; later batches uploaded slot entries and records only
        assert dev.store.uploaded_bytes == N * PAIR_BYTES


def test_fit_is_the_same_with_either_loader(tree):
    from helpers import trace_model
    cfg = (SIZE + (3,), 1, True, 0.0, {})
    out = []
    for which in (0, 1):
        model = trace_model(cfg)
        train = _pair(tree, None, dict(AUG, mask_order=0))[which]
        hist = model.fit(train, epochs=2, steps_per_epoch=3, verbose=0)
        out.append((hist.history, model.get_weights()))
    (h0, w0), (h1, w1) = out
    assert h0 == h1 and "loss" in h0 and len(h0["loss"]) == 2
    assert len(w0) == len(w1)
    for a, b in zip(w0, w1):
        assert np.array_equal(a, b)


def test_augmented_device_loader_feeding_train_steps_has_no_hazard(tree):
    """The method of test_hazards_gpu's loader case: the loader iterated in this thread, the consumer
    protocol by hand, three train steps after a warm-up one inside one recording; 3 resident slots of
    12 samples, so every batch rewrites the transient slots the batch before it was warped from."""
    from helpers import trace_model
    loader = DevicePairLoader(*tree, SIZE, BATCH, seed=2301, shuffle=True, horizontal_flip=True, workers=1,
                              device=DEV, device_cache_bytes=3 * PAIR_BYTES, augment=Augment(**AUG))
    assert (loader.book.resident, loader.book.transient) == (3, 4)
    model = trace_model((SIZE + (3,), 1, True, 0.0, {}))
    it = iter(loader)
    keep = []  # (allocator reuse of a freed batch is outside what the recorder sees)

    def step():
        shard = next(it)
        cur = torch.cuda.current_stream(model.engine.device)
        cur.wait_event(shard.event)
        shard[0].record_stream(cur)
        shard[1].record_stream(cur)
        keep.append(shard)
        model.train_step(shard[0], shard[1])

    with H.record_accesses(model.engine) as rec:
        step()
        first = len(rec.events)
        for _ in range(3):
            step()
    torch.cuda.synchronize()
    events = rec.events[first:]
    ls = loader.store.stream.cuda_stream
    on_loader = [e for e in events if e["kind"] in H.ACCESS and e["stream"] == ls]
    names = [e["name"] for e in on_loader]
    assert names.count("unet_batch_affine_u8") == 6 and "unet_batch_gather_u8" not in names
    assert names.count("aten::copy_") >= 3 * 3
    warps = [e for e in on_loader if e["name"] == "unet_batch_affine_u8"]
    assert all([a for _, _, a in e["reads"]] == ["src", "slots", "xforms"] and [a for _, _, a in e["writes"]] == ["dst"]
               for e in warps)
    # entries and records went up in ONE copy: each warp's slots and xforms lie back to back in its table
    assert all(e["reads"][1][1] == e["reads"][2][0] for e in warps)
    an = H.Analysis(events, rec.names())
    hz = an.hazards()
    assert not hz, "\n".join(H.format_hazard(h) for h in hz[:12])
    # the consumer's wait on the shard's event is what orders the warps before the step's reads of x / y
    waits = [ed["index"] for ed in H.ordering_edges(events) if ed["producer"] == ls]
    assert len(waits) == 3
    hz = an.hazards(drop=waits)
    on_dst = [h for h in hz for me in ("a", "b") if h[me + "_name"] == "unet_batch_affine_u8" and h[me + "_arg"] == "dst"]
    assert on_dst, "without the consumer's waits the warps' outputs must race the step"


def test_train_cli_augmented_device_loader(tmp_path, capsys):
    sys.path[:0] = [p for p in (SCRIPTS, os.path.join(ROOT, "tools")) if p not in sys.path]
    from bench_loader import make_midv_tree
    make_midv_tree(str(tmp_path), 8, 4)
    import train
    out = tmp_path / "models" / "model.h5"
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        train.main(["--epochs", "1", "--batch-size", "4", "--model-out", str(out), "--dataset-root", str(tmp_path),
                    "--device_loader", "--rotation-range", "10", "--zoom-range", "0.1", "--mask-order", "0"])
    finally:
        os.chdir(cwd)
    text = capsys.readouterr().out
    assert "Found 8 training samples and 4 validation samples." in text
    assert "Steps per epoch: 2, Validation steps: 1" in text
    assert "Epoch 1/1" in text and os.path.isfile(out)
