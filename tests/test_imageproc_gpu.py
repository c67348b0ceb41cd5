"""The device image pipeline against the host functions of unet_amd/imageproc.py, BITWISE
(np.array_equal, no tolerance anywhere): ops.image_resize_u8, ops.mask_resize,
pipeline.predict_masks for the fp32, fp16 and int8 networks, and the two CLIs with and without
--device_imageproc.  Shapes are the smallest that reach every branch of the kernels: rows of a
packed uint8 image that are not 4-byte aligned, enlargement / shrink / identity / a single source
row or column, mask rows whose start is at every 16-byte phase with heads and tails of every
length, an output narrower than one thread's run."""
import functools
import io
import json
import os
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest
from PIL import Image

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SCRIPTS = os.path.join(ROOT, "unet-image-segmentation_amd", "scripts")
SAMPLES = os.path.join(HERE, "golden", "samples")
for _p in (os.path.join(HERE, "golden"), SCRIPTS):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import make_golden as MG  # noqa: E402
from unet_amd.imageproc import resize_linear  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = (64, 128, 256, 512)
F32 = np.float32


def _tab(n_out, n_in):
    from unet_amd.pipeline import coord_table
    return coord_table(n_out, n_in, DEV)


def _host_pre(img, oh, ow, reverse):
    """The CLIs' preprocessing: (channels reversed,) / 255, INTER_LINEAR."""
    src = img[..., ::-1] if reverse else img
    return resize_linear(src.astype(F32) / 255.0, oh, ow)


def _device_pre(img, oh, ow, reverse, out=None, slot=0):
    from unet_amd import ops
    src = torch.from_numpy(np.array(img)).to(DEV)
    if out is None:
        out = torch.empty((1, oh, ow, img.shape[2]), dtype=torch.float32, device=DEV)
    ops.image_resize_u8(src, _tab(oh, img.shape[0]), _tab(ow, img.shape[1]), out, slot, reverse_channels=reverse)
    return out


@functools.lru_cache(maxsize=None)
def _sample_rgb():
    return np.asarray(Image.open(os.path.join(SAMPLES, "brazil_passport.png")).convert("RGB"))


def _source(case, c):
    if case == "sample":
        img = _sample_rgb()
        assert img.shape == (960, 540, 3)
        return img if c == 3 else np.ascontiguousarray(img[..., 1:2])
    sh, sw = case
    return np.random.default_rng(1000 * sh + sw + c).integers(0, 256, (sh, sw, c), dtype=np.uint8)


RESIZE_CASES = [((37, 53), (16, 24)), ((5, 7), (16, 16)), ((16, 16), (16, 16)), ((1, 9), (4, 4)), ((9, 1), (4, 4)),
                ("sample", (256, 256))]


@pytest.mark.parametrize("c,reverse", [(3, True), (3, False), (1, False)])
@pytest.mark.parametrize("case,dst", RESIZE_CASES, ids=[f"{s}-{d}" for s, d in RESIZE_CASES])
def test_image_resize_u8_bitwise(case, dst, c, reverse):
    img = _source(case, c)
    oh, ow = dst
    got = _device_pre(img, oh, ow, reverse)[0].cpu().numpy()
    ref = _host_pre(img, oh, ow, reverse)
    assert got.shape == ref.shape == (oh, ow, c)
    assert np.array_equal(got, ref), np.abs(got - ref).max()


def test_image_resize_u8_writes_only_its_slot():
    img = _source((37, 53), 3)
    out = torch.full((3, 16, 24, 3), -7.0, dtype=torch.float32, device=DEV)
    _device_pre(img, 16, 24, True, out=out, slot=1)
    got = out.cpu().numpy()
    assert np.all(got[0] == -7.0) and np.all(got[2] == -7.0)
    assert np.array_equal(got[1], _host_pre(img, 16, 24, True))


def test_every_byte_value_over_255_is_correctly_rounded():
    """Decides between the kernel's fp32 divide and a host table: all 256 quotients, bitwise."""
    img = np.arange(256, dtype=np.uint8).reshape(1, 256, 1)
    got = _device_pre(img, 1, 256, False)[0].cpu().numpy().reshape(-1)
    assert np.array_equal(got, np.arange(256, dtype=F32) / F32(255))


def _device_mask(p, oh, ow, thr):
    """ops.mask_resize into the middle of a buffer with 64 sentinel bytes on either side."""
    from unet_amd import ops
    if p.ndim == 2:
        p = p[..., None]
    buf = torch.full((64 + oh * ow + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    out = buf[64:64 + oh * ow].view(oh, ow)
    ops.mask_resize(torch.from_numpy(np.ascontiguousarray(p)).to(DEV), _tab(oh, p.shape[0]), _tab(ow, p.shape[1]),
                    out, thr)
    host = buf.cpu().numpy()
    assert np.all(host[:64] == 0xA5), "bytes before the mask were written"
    assert np.all(host[-64:] == 0xA5), "bytes after the mask were written"
    return host[64:-64].reshape(oh, ow)


def _host_mask(p, oh, ow, thr):
    return (resize_linear(p, oh, ow) > thr).astype(np.uint8) * 255


@pytest.mark.parametrize("thr", [0.5, 0.3])
@pytest.mark.parametrize("dst", [(37, 53), (64, 64), (16, 16), (1, 5), (3, 131)])
def test_mask_resize_binary_bitwise(dst, thr):
    p = np.random.default_rng(16).random((16, 16), dtype=F32)
    got = _device_mask(p, *dst, thr)
    ref = _host_mask(p, *dst, thr)
    assert 0 < ref.mean() < 255 or dst == (1, 5)
    assert np.array_equal(got, ref), int((got != ref).sum())


def test_mask_resize_comparison_is_strict():
    p = np.full((8, 8), 0.5, F32)
    got = _device_mask(p, 19, 19, 0.5)
    assert np.array_equal(got, _host_mask(p, 19, 19, 0.5)) and not got.any()


def test_mask_resize_step_edge():
    p = np.empty((8, 8), F32)
    p[:, :4], p[:, 4:] = 0.25, 0.75
    got = _device_mask(p, 19, 19, 0.5)
    ref = _host_mask(p, 19, 19, 0.5)
    assert np.array_equal(got, ref) and 0 < ref.mean() < 255


@pytest.mark.parametrize("ncls", [3, 21])
def test_mask_resize_argmax_bitwise(ncls):
    e = np.random.default_rng(ncls).random((16, 16, ncls)) ** 4
    p = (e / e.sum(-1, keepdims=True)).astype(F32)
    got = _device_mask(p, 37, 53, 0.5)
    ref = np.argmax(resize_linear(p, 37, 53), -1).astype(np.uint8)
    assert len(np.unique(ref)) == ncls
    assert np.array_equal(got, ref), int((got != ref).sum())


@pytest.mark.parametrize("ncls", [3, 21])
def test_mask_resize_argmax_first_index_wins_a_tie(ncls):
    p = np.random.default_rng(ncls + 1).random((16, 16, ncls), dtype=F32) * F32(0.3)
    p[..., 1] = F32(0.4) + F32(0.5) * np.random.default_rng(5).random((16, 16), dtype=F32)
    p[..., 2] = p[..., 1]   # identical, and the largest everywhere
    got = _device_mask(p, 37, 53, 0.5)
    assert np.array_equal(got, np.argmax(resize_linear(p, 37, 53), -1).astype(np.uint8))
    assert np.all(got == 1)


def test_mask_resize_refuses_more_than_255_classes():
    from unet_amd import ops
    with pytest.raises(ValueError, match="ncls"):
        ops.mask_resize(torch.zeros((2, 2, 256), device=DEV), _tab(2, 2), _tab(2, 2),
                        torch.zeros((2, 2), dtype=torch.uint8, device=DEV))


# ------------------------------------------------------------------------------ end to end ---
@functools.lru_cache(maxsize=None)
def _models(h, w, ncls):
    from unet_amd.model import UNetModel
    m = UNetModel((h, w, 3), ncls, dropout_rate=0.0, device=DEV)
    m.engine.set_weights_dict({k: v.astype(F32) for k, v in MG.model_weights(ncls, F, 11).items()})
    calib = MG.U(21, (4, h, w, 3)).astype(F32)
    return {"float32": m, "float16": m.freeze(), "int8": m.freeze(dtype="int8", calibration=calib)}


@pytest.mark.parametrize("kind", ["float32", "float16", "int8"])
@pytest.mark.parametrize("h,w,ncls", [(32, 32, 1), (48, 32, 3)])
def test_predict_masks_end_to_end(h, w, ncls, kind):
    model = _models(h, w, ncls)[kind]
    rng = np.random.default_rng(7)
    images = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in ((37, 53), (64, 40), (32, 32))]
    masks, probs, inputs = model.predict_masks(images, batch_size=2, return_probs=True)
    assert len(masks) == 3 and tuple(probs.shape) == (3, h, w, ncls) and tuple(inputs.shape) == (3, h, w, 3)
    assert probs.is_cuda and inputs.is_cuda
    x, p = inputs.cpu().numpy(), probs.cpu().numpy()
    for i, img in enumerate(images):
        assert np.array_equal(x[i], _host_pre(img, h, w, True)), f"input {i}"
        ih, iw = img.shape[:2]
        if ncls == 1:
            ref = _host_mask(p[i, ..., 0], ih, iw, 0.5)
        else:
            ref = np.argmax(resize_linear(p[i], ih, iw), -1).astype(np.uint8)
        assert masks[i].dtype == np.uint8 and masks[i].shape == (ih, iw)
        assert np.array_equal(masks[i], ref), f"mask {i}: {int((masks[i] != ref).sum())} bytes differ"
    # device tensors are taken as images too, and plain (no return_probs) gives the masks alone
    again = model.predict_masks([torch.from_numpy(images[0]).to(DEV)], bgr=True)
    assert isinstance(again, list) and len(again) == 1 and again[0].shape == (37, 53)


# ------------------------------------------------------------------------------------ CLIs ---
@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """train.py --synthetic 48 --epochs 2 --batch-size 8 in a scratch directory."""
    import train
    d = tmp_path_factory.mktemp("train_imageproc")
    cwd = os.getcwd()
    os.chdir(d)
    try:
        out = os.path.join(str(d), "models", "model.h5")
        with redirect_stdout(io.StringIO()):
            train.main(["--synthetic", "48", "--epochs", "2", "--batch-size", "8", "--model-out", out])
    finally:
        os.chdir(cwd)
    return out


def test_inference_cli_device_imageproc_writes_the_same_files(trained, tmp_path):
    """If this pair ever differs: compare the two input tensors and the two probability maps
    first.  Should those differ, the network is not reproducible from call to call, which is a
    finding to report, not a tolerance to add here."""
    import inference
    src = os.path.join(SAMPLES, "chile_id_card.png")
    files = {}
    for tag, extra in (("host", []), ("device", ["--device_imageproc"])):
        om, oc = str(tmp_path / f"{tag}_mask.png"), str(tmp_path / f"{tag}_crop.png")
        inference.main([src, "--model", trained, "--output_mask", om, "--output_cropped", oc] + extra)
        files[tag] = (open(om, "rb").read(), open(oc, "rb").read() if os.path.isfile(oc) else None)
    assert np.asarray(Image.open(str(tmp_path / "device_mask.png"))).shape == (960, 540)
    assert files["host"][0] == files["device"][0], "mask files differ"
    assert files["host"][1] == files["device"][1], "crop files differ"


def test_benchmark_cli_device_imageproc_prints_the_same_metrics(trained, tmp_path, capsys):
    """A two-image tree in the layout benchmark.py reads (images/**/*.tif, ground_truth/**/*.json)."""
    import benchmark
    rng = np.random.default_rng(9)
    img_d, gt_d = tmp_path / "images" / "cardA", tmp_path / "ground_truth" / "cardA"
    os.makedirs(img_d)
    os.makedirs(gt_d)
    for i, (h, w) in enumerate(((300, 200), (211, 333))):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(str(img_d / f"f{i}.tif"))
        quad = [[int(0.2 * w), int(0.15 * h)], [int(0.8 * w), int(0.2 * h)], [int(0.85 * w), int(0.8 * h)],
                [int(0.1 * w), int(0.75 * h)]]
        with open(gt_d / f"f{i}.json", "w") as f:
            json.dump({"quad": quad}, f)
    metrics = {}
    for tag, extra in (("host", []), ("device", ["--device_imageproc"])):
        capsys.readouterr()
        benchmark.main([str(tmp_path), "--model", trained, "--iou_threshold", "1.0"] + extra)
        out = capsys.readouterr().out
        metrics[tag] = [l for l in out.splitlines() if l.startswith(("Overall Mean IoU:", "  - IoU:"))]
    assert len(metrics["host"]) == 3, metrics["host"]
    assert metrics["host"] == metrics["device"]
