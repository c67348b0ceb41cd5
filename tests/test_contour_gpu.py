"""The device contour kernels (csrc/contour.hip: ops.mask_largest_contour, and through it
predict_masks(..., return_boxes=True) and scripts/inference.py --device_contour) against the host
tracer imageproc.largest_external_contour, field by field of the 32-byte record and EXACTLY: every
value is an integer, so there is no tolerance anywhere.  Where the tracer is too slow (1080x1920)
the closed form's NumPy restatement is the oracle; tests/test_contour_host.py holds the two equal.
The masks come from that file: hand-built ones at the tile's edges (a tile is 32x32), topologies
that tell F from the foreground, ties, and seeded random and blob masks."""
import ctypes
import functools
import io
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
for _p in (HERE, os.path.join(HERE, "golden"), SCRIPTS):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import make_golden as MG  # noqa: E402
from test_contour_host import blob_masks, host_record, mask_cases, random_masks, sample_masks  # noqa: E402
from unet_amd.imageproc import largest_external_contour  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = (64, 128, 256, 512)
F32 = np.float32


def _fields(raw):
    from unet_amd._lib import UnetContourBox
    b = UnetContourBox.from_buffer_copy(bytes(raw))
    return (b.count, b.x, b.y, b.w, b.h, b.first, b.area2)


def device_record(mask, offset=0):
    """The record of `mask`, read by the kernels at byte `offset` inside a larger flat buffer."""
    from unet_amd import ops
    h, w = mask.shape
    flat = torch.full((offset + h * w + 5,), 0xFF, dtype=torch.uint8, device=DEV)
    flat[offset:offset + h * w] = torch.from_numpy(mask.reshape(-1).copy()).to(DEV)
    out = ops.mask_largest_contour(flat[offset:offset + h * w].view(h, w))
    assert out.dtype == torch.uint8 and out.numel() == 32 and out.is_cuda
    return _fields(out.cpu().numpy().tobytes())


@pytest.mark.parametrize("name", [n for n, _ in mask_cases()])
def test_hand_built_masks(name):
    mask = dict(mask_cases())[name]
    assert device_record(mask) == host_record(mask)


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_mask_at_every_byte_offset(offset):
    mask = dict(mask_cases())["29x37_random"]
    assert mask.shape[1] == 37
    assert device_record(mask, offset) == host_record(mask)


@pytest.mark.parametrize("shape", [(37, 53), (70, 150)])
def test_random_and_blob_masks(shape):
    masks = random_masks(6, 100 + shape[0], shape) + blob_masks(6, 200 + shape[0], shape)
    for i, m in enumerate(masks):
        assert m.shape == shape
        assert device_record(m) == host_record(m), i


@pytest.mark.parametrize("name", ["brazil_passport", "chile_id_card"])
def test_reference_sample_masks(name):
    mask = sample_masks()[name]
    rec = device_record(mask)
    assert rec == host_record(mask)
    area, rect = largest_external_contour(mask)
    assert rec[6] / 2.0 == area and rec[1:5] == rect


def test_1080x1920_blob_mask_against_the_closed_form():
    mask = blob_masks(2, 1080, (1080, 1920))[1]
    ref = host_record(mask, filled=True)
    assert ref[0] > 1
    assert device_record(mask) == ref


def _raw_call(mask_dev, h, w, out, ws, ws_bytes):
    from unet_amd import _lib
    _lib.call("unet_mask_largest_contour", ctypes.c_void_p(mask_dev.data_ptr()), h, w,
              ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(ws.data_ptr()), ws_bytes,
              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return _fields(out.cpu().numpy().tobytes())


def test_workspace_bounds_and_dirty_reuse():
    """Nothing beyond the reported workspace size is written, and neither the workspace's nor the
    record's earlier contents matter: another mask of the same size in between, then the first
    again."""
    from unet_amd import _lib
    cases = dict(mask_cases())
    a, b = cases["65x129_spiral"], cases["65x129_comb"]
    h, w = a.shape
    need = _lib.query("unet_mask_largest_contour_workspace", h, w)
    assert need > 0 and need % 256 == 0
    ws = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
    out = torch.full((32,), 0xA5, dtype=torch.uint8, device=DEV)
    da, db = (torch.from_numpy(m.copy()).to(DEV) for m in (a, b))
    first = _raw_call(da, h, w, out, ws, need)
    other = _raw_call(db, h, w, out, ws, need)
    again = _raw_call(da, h, w, out, ws, need)
    assert first == again == host_record(a)
    assert other == host_record(b)
    assert bool((ws[need:] == 0xA5).all()), "bytes beyond the reported workspace size were written"
    with pytest.raises(_lib.UnetHipError, match="workspace"):
        _raw_call(da, h, w, out, ws, need - 256)


def test_op_refuses_wrong_tensors():
    from unet_amd import ops
    with pytest.raises(ValueError, match="uint8"):
        ops.mask_largest_contour(torch.zeros((4, 4), dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError, match=r"\(h, w\)"):
        ops.mask_largest_contour(torch.zeros((4, 4, 1), dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="no CPU path"):
        ops.mask_largest_contour(torch.zeros((4, 4), dtype=torch.uint8))
    out = torch.zeros(32, dtype=torch.uint8, device=DEV)
    assert ops.mask_largest_contour(torch.zeros((4, 4), dtype=torch.uint8, device=DEV), out) is out
    assert _fields(out.cpu().numpy().tobytes()) == (0, 0, 0, 0, 0, 0, 0)


# ------------------------------------------------------------------------------ end to end ---
@functools.lru_cache(maxsize=None)
def _models(h, w, ncls, empty):
    """Random weights as tests/test_imageproc_gpu.py builds them.  empty: the output layer's bias
    puts every pixel in the background (class 0), so every mask comes out empty."""
    from unet_amd.model import UNetModel
    m = UNetModel((h, w, 3), ncls, dropout_rate=0.0, device=DEV)
    weights = {k: v.astype(F32) for k, v in MG.model_weights(ncls, F, 11).items()}
    if empty:
        bias = np.zeros_like(weights["output_mask/bias"])
        bias[0] = -30.0 if ncls == 1 else 30.0
        weights["output_mask/bias"] = bias
    m.engine.set_weights_dict(weights)
    calib = MG.U(21, (4, h, w, 3)).astype(F32)
    return {"float32": m, "float16": m.freeze(), "int8": m.freeze(dtype="int8", calibration=calib)}


@functools.lru_cache(maxsize=None)
def _images():
    rng = np.random.default_rng(7)
    samples = [np.asarray(Image.open(os.path.join(SAMPLES, n)).convert("RGB"))
               for n in ("brazil_passport.png", "chile_id_card.png")]
    return samples + [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in ((37, 53), (64, 40), (32, 32))]


@pytest.mark.parametrize("kind", ["float32", "float16", "int8"])
@pytest.mark.parametrize("h,w,ncls", [(32, 32, 1), (48, 32, 3)])
def test_predict_masks_return_boxes(h, w, ncls, kind):
    model = _models(h, w, ncls, False)[kind]
    images = _images()
    plain = model.predict_masks(images, batch_size=3)
    masks, boxes = model.predict_masks(images, batch_size=3, return_boxes=True)
    assert isinstance(plain, list) and len(masks) == len(boxes) == len(images)
    for i, (a, b) in enumerate(zip(plain, masks)):
        assert a.shape == images[i].shape[:2] and np.array_equal(a, b), f"mask {i} changed"
    assert any(m.any() for m in masks)
    for i, m in enumerate(masks):
        ref = largest_external_contour(m)
        assert boxes[i] == ref, (i, boxes[i], ref)
        if ref is not None:
            assert type(boxes[i][0]) is float and all(type(v) is int for v in boxes[i][1])
    # with the probabilities: boxes stay the last element
    m2, probs, inputs, b2 = model.predict_masks(images, batch_size=3, return_probs=True, return_boxes=True)
    assert tuple(probs.shape) == (len(images), h, w, ncls) and tuple(inputs.shape) == (len(images), h, w, 3)
    assert b2 == boxes and all(np.array_equal(a, b) for a, b in zip(m2, masks))
    # an image whose mask comes out empty has no box
    hollow = _models(h, w, ncls, True)[kind]
    m3, b3 = hollow.predict_masks(images[2:], return_boxes=True)
    assert not any(m.any() for m in m3) and b3 == [None] * len(m3)


# ------------------------------------------------------------------------------------- CLI ---
@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """train.py --synthetic 48 --epochs 2 --batch-size 8 in a scratch directory."""
    import train
    d = tmp_path_factory.mktemp("train_contour")
    cwd = os.getcwd()
    os.chdir(d)
    try:
        out = os.path.join(str(d), "models", "model.h5")
        with redirect_stdout(io.StringIO()):
            train.main(["--synthetic", "48", "--epochs", "2", "--batch-size", "8", "--model-out", out])
    finally:
        os.chdir(cwd)
    return out


_RESULT_LINES = ("Saving", "Finding", "Largest contour", "No contours")


def _run_cli(trained, workdir, extra):
    """inference.main in `workdir` with relative output paths -> (mask bytes, crop bytes or None,
    the lines about the result)."""
    import inference
    src = os.path.join(SAMPLES, "chile_id_card.png")
    os.makedirs(workdir)
    cwd = os.getcwd()
    os.chdir(workdir)
    buf = io.StringIO()
    try:
        with redirect_stdout(buf):
            inference.main([src, "--model", trained, "--output_mask", "mask.png", "--output_cropped", "crop.png"]
                           + extra)
        crop = open("crop.png", "rb").read() if os.path.isfile("crop.png") else None
        return open("mask.png", "rb").read(), crop, [l for l in buf.getvalue().splitlines()
                                                      if l.startswith(_RESULT_LINES)]
    finally:
        os.chdir(cwd)


def test_inference_cli_device_contour_writes_the_same_files(trained, tmp_path):
    mask = None
    for min_area in ("0", "1e9"):
        host = _run_cli(trained, str(tmp_path / f"host{min_area}"), ["--min_area", min_area])
        imgp = _run_cli(trained, str(tmp_path / f"imgp{min_area}"), ["--min_area", min_area, "--device_imageproc"])
        dev = _run_cli(trained, str(tmp_path / f"dev{min_area}"), ["--min_area", min_area, "--device_contour"])
        assert host[0] == dev[0], "mask files differ"
        assert host[1] == dev[1], "crop files differ"
        assert host[2] == dev[2] == imgp[2], (host[2], dev[2])
        if min_area == "1e9":
            assert dev[1] is None, "a crop was written below --min_area"
        mask = np.asarray(Image.open(str(tmp_path / f"dev{min_area}" / "mask.png")))
    assert mask.shape == (960, 540)
