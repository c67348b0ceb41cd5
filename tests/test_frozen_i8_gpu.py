"""The frozen int8 network end to end (quantize_weights -> FrozenUNetI8, UNetModel.freeze(dtype="int8")).

The gate is PER LAYER and bitwise: forward(x, keep_activations=True), then every block, pool and
upsample must equal the one-layer emulator of the contract (tests/i8_emulation.py) FED THAT LAYER'S
GPU INPUT BYTES.  Running every layer from the device's own inputs keeps one tie in the fp32 image
block from spreading into later layers.  The image block itself (fp32, one rounding to a byte) is
within one step of float64 with at most 0.1 % of elements different; prob is within the fp32 head
bound of its emulation, and within twice the emulator's whole-forward error of the float64 oracle.
Ranges come from the float64 oracle activations on the same input.
"""
import functools
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "unet-image-segmentation_amd", "scripts"))

import f16_emulation as E16  # noqa: E402
import i8_emulation as E  # noqa: E402
import make_golden as MG  # noqa: E402
from oracle import keras_ops as K  # noqa: E402
from unet_amd import frozen  # noqa: E402

pytestmark = pytest.mark.gpu

F = (64, 128, 256, 512)
# name -> (classes, input shape, weight seed, input seed, use_batch_norm, filters): test_frozen_gpu.py's cases
CASES = {
    "c1_2x32x32": (1, (2, 32, 32, 3), 11, 21, True, F),
    "c3_3x48x32": (3, (3, 48, 32, 3), 2301, 7, True, F),   # tile levels 48x32, 24x16; rows 12x8, 6x4, 3x2
    "c1_1x16x16": (1, (1, 16, 16, 3), 11, 21, True, F),    # the bottleneck is 1x1
    "nobn_2x32x32": (1, (2, 32, 32, 3), 11, 21, False, F),  # case 1 as a no-BN model: the bias route
    # two levels off the default widths: a 32-output image block on a non-square input ...
    "f3264_2x32x64": (1, (2, 32, 64, 3), 11, 21, True, (32, 64)),
    # ... and widths 96 and 192: N tails in the tile (48x32, 24x16) and rows (12x8) policies
    "f6496_3x48x32": (3, (3, 48, 32, 3), 2301, 7, True, (64, 96)),
}


def _weights(ncls, wseed, use_bn, F=F):
    w = MG.model_weights(ncls, F, wseed)
    if use_bn:
        return w
    ex = frozen.fold_exact(w, ncls, True, F)
    out = {k: v for k, v in w.items() if "_bn/" not in k}
    for b in frozen.block_names(F):
        out[f"{b}_sepconv/pointwise_kernel"] = ex[f"{b}_sepconv/pointwise_kernel"]
        out[f"{b}_sepconv/bias"] = ex[f"{b}_sepconv/bias"]
    return out


@functools.lru_cache(maxsize=None)
def _reference(case):
    """(x, float64 oracle activations, quantised operands, emulator forward), once per case."""
    ncls, shape, wseed, xseed, use_bn, F = CASES[case]
    w = _weights(ncls, wseed, use_bn, F)
    x = MG.U(xseed, shape)
    ref = E16.oracle_activations(w, x, ncls, F, use_bn)
    exact = frozen.fold_exact(w, ncls, use_bn, F)
    q = frozen.quantize_weights(exact, E.oracle_ranges(exact, ref, F), F)
    return x, ref, q, E.forward(q, x.astype(np.float32), ncls, F)


def _frozen(case):
    ncls, shape, _, _, _, F = CASES[case]
    x, _, q, _ = _reference(case)
    net = frozen.FrozenUNetI8(q, shape[1:], ncls, F, "cuda:0")
    return net, torch.as_tensor(x.astype(np.float32), device="cuda:0")


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if not np.array_equal(got, want):
        idx = tuple(int(i) for i in np.argwhere(got != want)[0])
        raise AssertionError(f"{what}: {int((got != want).sum())} of {want.size} bytes differ, first at {idx}: "
                             f"gpu {int(got[idx])}, emulator {int(want[idx])}")


@pytest.mark.parametrize("case", list(CASES))
def test_every_layer_is_the_emulator_on_the_device_inputs(case):
    ncls, F = CASES[case][0], CASES[case][5]
    net, xt = _frozen(case)
    x, ref, q, emu = _reference(case)
    assert net.dtype == "int8" and isinstance(net, frozen.FrozenUNet)
    prob = net.forward(xt, keep_activations=True)
    torch.cuda.synchronize()
    got = {name: net.activation(name).cpu().numpy() for name in frozen.activation_names(F)}
    n = len(F)
    # the image block: fp32 arithmetic against float64
    want, _ = E.image_block(x.astype(np.float32), q["enc1_block1/dw"], q["enc1_block1/pw"], q["enc1_block1/bias"],
                            q["scale/enc1_block1"])
    diff = np.abs(got["enc1_block1"].astype(np.int64) - want.astype(np.int64))
    print(case, "image block: elements differing", int((diff > 0).sum()), "of", diff.size)
    assert got["enc1_block1"].dtype == np.uint8 and diff.max() <= 1 and (diff > 0).sum() <= 1e-3 * diff.size
    # every other block from its own device input; pools; upsamples
    for b, srcs in frozen.block_inputs(F).items():
        a = np.concatenate([got[s].astype(np.int16) for s in srcs], axis=-1)
        _same(got[b], E.sepconv(a, *E.block_operands(q, b)), f"{case} {b}")
    for i in range(n):
        _same(got[f"enc{i + 1}_pool"], E.maxpool(got[f"enc{i + 1}_block2"]), f"{case} enc{i + 1}_pool")
        s = f"dec{i + 1}_upsample"
        src = "bneck_block2" if i == n - 1 else f"dec{i + 2}_block2"
        assert got[s].dtype == np.int8
        _same(got[s], E.conv_transpose(got[src], *E.upsample_operands(q, s)), f"{case} {s}")
    # the head: fp32 sums on the device, float64 here
    a = got["dec1_block2"]
    cin = a.shape[-1]
    p64 = prob.cpu().numpy().astype(np.float64)
    want = E.head(a, q["head/kernel"], q["head/bias"], ncls)
    hk = np.abs(np.asarray(q["head/kernel"], np.float64)).reshape(1, 1, cin, ncls)
    amp = (K.pointwise(a.astype(np.float64), hk) + np.abs(q["head/bias"])).max(axis=-1, keepdims=True)
    assert prob.dtype == torch.float32 and np.all(np.abs(p64 - want) <= (cin + 2) * 2.0 ** -24 * amp + 1e-6)
    # against the float64 oracle: within twice the emulator's own whole-forward error
    e_emu = float(np.abs(emu["prob"] - ref["prob"]).max())
    e_gpu = float(np.abs(p64 - ref["prob"]).max())
    print(case, "prob error: gpu", e_gpu, "emulator", e_emu)
    assert e_gpu <= 2.0 * e_emu
    # the ping-pong forward (no kept activations) computes the same probabilities
    assert torch.equal(net.forward(xt), prob)
    with pytest.raises(KeyError):
        net.activation("enc5_pool")
    # scales are quantize_weights'
    for name in frozen.activation_names(F):
        assert net.activation_scale(name) == float(q[f"scale/{name}"])
    assert net.activation_scale("enc2_pool") == net.activation_scale("enc2_block2")


def test_activation_needs_a_kept_forward():
    net, xt = _frozen("c1_1x16x16")
    net.forward(xt)
    with pytest.raises(RuntimeError, match="keep_activations"):
        net.activation("bneck_block2")
    with pytest.raises(ValueError, match="expected input"):
        net.forward(xt[:, :8])


def test_predict_in_chunks_equals_one_call():
    net, xt = _frozen("c3_3x48x32")
    x = xt.cpu().numpy()
    whole = net.predict(x)
    parts = net.predict(x, batch_size=2)
    assert isinstance(whole, np.ndarray) and whole.dtype == np.float32 and whole.shape == (3, 48, 32, 3)
    assert np.array_equal(whole.view(np.uint32), parts.view(np.uint32))
    dev = net.predict(xt)
    assert isinstance(dev, torch.Tensor) and dev.is_cuda and np.array_equal(dev.cpu().numpy(), whole)
    np.testing.assert_allclose(whole.sum(axis=-1), 1.0, atol=1e-5)
    net.release_buffers()
    assert np.array_equal(net.predict(x).view(np.uint32), whole.view(np.uint32))


@pytest.fixture(scope="module")
def model():
    from unet_amd.model import UNetModel
    m = UNetModel((32, 32, 3), 1, dropout_rate=0.0, device="cuda:0")
    m.engine.set_weights_dict({k: v.astype(np.float32) for k, v in MG.model_weights(1, F, 11).items()})
    return m


def test_freeze_int8_calibrates_and_snapshots_the_model(model, tmp_path):
    from unet_amd.optim import AdamW
    x = MG.U(21, (2, 32, 32, 3)).astype(np.float32)
    with pytest.raises(ValueError, match="calibration"):
        model.freeze(dtype="int8")
    with pytest.raises(ValueError, match="float16"):
        model.freeze(dtype="bfloat16", calibration=x)
    fz = model.freeze(dtype="int8", calibration=x, batch_size=1)
    assert isinstance(fz, frozen.FrozenUNetI8) and fz.dtype == "int8"
    # calibrated on the device: the ranges are those of the oracle's activations (fp16 network, fp32
    # weights: 1 % covers both), so the scales are those of the host-side reference
    _, ref, q, emu = _reference("c1_2x32x32")
    for name in frozen.calibration_names(F):
        np.testing.assert_allclose(fz.activation_scale(name), float(q[f"scale/{name}"]), rtol=1e-2, err_msg=name)
    before = fz.predict(x)
    p32 = model.predict(x)
    # (other scales than the reference's by a few 1e-4: the same scheme, so the same size of error)
    assert np.abs(before - ref["prob"]).max() <= 2.0 * np.abs(emu["prob"] - ref["prob"]).max()
    assert np.abs(before - p32).max() <= 3.0 * np.abs(emu["prob"] - ref["prob"]).max()
    # save / load reproduces predict bitwise, through FrozenUNet.load
    path = str(tmp_path / "frozen_i8.h5")
    fz.save(path)
    assert frozen.is_frozen_file(path)
    back = frozen.FrozenUNet.load(path, device="cuda:0")
    assert isinstance(back, frozen.FrozenUNetI8) and back.dtype == "int8"
    assert (back.h, back.w, back.c, back.num_classes, back.filters) == (32, 32, 3, 1, F)
    assert np.array_equal(back.predict(x).view(np.uint32), before.view(np.uint32))
    # a train step on the source model leaves the frozen copy bitwise unchanged
    model.compile(AdamW(learning_rate=1e-2), "dice_loss")
    y = (MG.U(22, (2, 32, 32, 1)) > 0.5).astype(np.float32)
    model.train_step(x, y)
    torch.cuda.synchronize()
    assert not np.array_equal(model.predict(x), p32)
    assert np.array_equal(fz.predict(x).view(np.uint32), before.view(np.uint32))


def test_collect_ranges_keeps_running_maxima(model):
    x = MG.U(21, (2, 32, 32, 3)).astype(np.float32)
    both = frozen.collect_ranges(model, x, batch_size=2)
    one = frozen.collect_ranges(model, x, batch_size=1)
    first = frozen.collect_ranges(model, x[:1])
    assert set(both) == set(frozen.calibration_names(F)) and both == one
    assert all(first[k] <= both[k] for k in both) and any(first[k] < both[k] for k in both)


def test_inference_cli_with_an_int8_model(tmp_path, capsys):
    """convert_to_frozen.py --int8 --calibration_data, then scripts/inference.py --model <int8 file>:
    the mask has the image's shape and the values 0 / 255, and is the mask of the int8 network's own
    predict at that threshold."""
    import convert_to_frozen
    import inference
    from PIL import Image
    from unet_amd.model import UNetModel
    m = UNetModel((256, 256, 3), 1, dropout_rate=0.0, device="cuda:0")
    w = {k: v.astype(np.float32) for k, v in MG.model_weights(1, F, 11).items()}
    w["output_mask/kernel"] = w["output_mask/kernel"] * 8.0  # spread the probabilities around 0.5
    w["output_mask/bias"] = np.full(1, -1.85, np.float32)
    m.engine.set_weights_dict(w)
    img = np.zeros((256, 256, 3), np.uint8)
    img[:, 128:] = 255
    png = str(tmp_path / "two_tone.png")
    Image.fromarray(img).save(png)
    x, _, _, _ = inference.load_and_preprocess_image(png, 256, 256)
    plain, frz, cal = str(tmp_path / "w.npz"), str(tmp_path / "w_i8.npz"), str(tmp_path / "cal.npy")
    m.save_weights(plain)
    np.save(cal, x.astype(np.float32))
    assert convert_to_frozen.main([plain, frz, "--int8", "--calibration_data", cal]) == 0
    assert "int8" in capsys.readouterr().out
    net = frozen.FrozenUNet.load(frz, device="cuda:0")
    assert net.dtype == "int8"
    p = net.predict(x)[0, ..., 0]
    s = np.sort(p.astype(np.float64).ravel())
    lo, hi = 16, s.size - 16  # at least 16 pixels on either side; the widest gap between them
    i = lo + int(np.argmax(np.diff(s[lo:hi])))
    thr = float(0.5 * (s[i] + s[i + 1]))
    assert 0.0 < thr < 1.0 and s[i + 1] - s[i] > 1e-4
    om = str(tmp_path / "mask.png")
    inference.main([png, "--model", frz, "--output_mask", om, "--output_cropped", str(tmp_path / "crop.png"),
                    "--threshold", repr(thr)])
    mask = np.asarray(Image.open(om))
    assert mask.shape == (256, 256) and set(np.unique(mask).tolist()) == {0, 255}
    assert np.array_equal(mask == 255, p > thr)
