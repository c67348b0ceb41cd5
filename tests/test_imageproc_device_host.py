"""Host side of the device image pipeline (no GPU): the sampling coordinates the kernels are fed
are those resize_linear always used, predict_masks refuses bad input before it touches a device,
and the two new ops have no CPU path."""
import numpy as np
import pytest

from unet_amd import imageproc


def _old_coords(n_out, n_in):
    """The inner coords() of resize_linear before linear_coords was factored out."""
    s = (np.arange(n_out) + 0.5) * (n_in / n_out) - 0.5
    s = np.clip(s, 0, n_in - 1)
    i0 = np.floor(s).astype(np.int64)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, (s - i0).astype(np.float32)


def _old_resize_linear(img, out_h, out_w):
    """resize_linear's body before the refactor."""
    h, w = img.shape[:2]
    y0, y1, fy = _old_coords(out_h, h)
    x0, x1, fx = _old_coords(out_w, w)
    a = img[y0][:, x0]
    b = img[y0][:, x1]
    c = img[y1][:, x0]
    d = img[y1][:, x1]
    fx = fx[None, :, None] if img.ndim == 3 else fx[None, :]
    fy = fy[:, None, None] if img.ndim == 3 else fy[:, None]
    top = a + (b - a) * fx
    bot = c + (d - c) * fx
    return (top + (bot - top) * fy).astype(np.float32)


@pytest.mark.parametrize("n_out,n_in", [(2, 4), (4, 2), (256, 960), (540, 256), (5, 5), (7, 1)])
def test_linear_coords_is_the_formula_resize_linear_used(n_out, n_in):
    i0, i1, f = imageproc.linear_coords(n_out, n_in)
    r0, r1, rf = _old_coords(n_out, n_in)
    assert i0.dtype == np.int64 and i1.dtype == np.int64 and f.dtype == np.float32
    assert i0.shape == i1.shape == f.shape == (n_out,)
    assert np.array_equal(i0, r0) and np.array_equal(i1, r1) and np.array_equal(f, rf)
    assert i0.min() >= 0 and i1.max() <= n_in - 1 and np.all(i1 - i0 <= 1) and np.all((f >= 0) & (f < 1))


def test_resize_linear_is_bitwise_unchanged():
    rng = np.random.default_rng(3)
    img = rng.random((9, 7, 3), dtype=np.float32)
    flat = rng.random((11, 6), dtype=np.float32)
    for a, sizes in ((img, [(16, 24), (4, 3), (9, 7)]), (flat, [(5, 13), (11, 6), (23, 2)])):
        for oh, ow in sizes:
            got = imageproc.resize_linear(a, oh, ow)
            assert got.dtype == np.float32 and np.array_equal(got, _old_resize_linear(a, oh, ow))


class _StubModel:
    """What predict_masks reads of a model before it touches the device."""
    h, w, c, num_classes, device = 32, 32, 3, 1, "cuda:0"

    def predict(self, x, batch_size=None):
        raise AssertionError("predict_masks reached the model with input it should have refused")


@pytest.mark.parametrize("images,threshold", [
    ([np.zeros((8, 8, 3), np.float32)], 0.5),                                   # float image
    ([np.zeros((8, 8, 3), np.uint8), np.zeros((8, 8, 4), np.uint8)], 0.5),       # 4 channels
    ([np.zeros((8, 8, 3), np.uint8), np.zeros((0, 8, 3), np.uint8)], 0.5),       # empty image
    ([np.zeros((8, 8, 3), np.uint8), None], 0.5),                               # empty list entry
    ([np.zeros((8, 8, 3), np.uint8)], 1.0),                                     # threshold outside (0, 1)
    ([np.zeros((8, 8, 3), np.uint8)], 0.0),
])
def test_predict_masks_refuses_bad_input_before_the_device(images, threshold):
    from unet_amd.pipeline import predict_masks
    with pytest.raises(ValueError):
        predict_masks(_StubModel(), images, threshold=threshold)


def test_model_classes_delegate_predict_masks():
    from unet_amd.frozen import FrozenUNet
    from unet_amd.model import UNetModel
    assert callable(UNetModel.predict_masks) and callable(FrozenUNet.predict_masks)


def test_image_ops_refuse_cpu_tensors():
    import torch
    from unet_amd import ops
    tab = torch.zeros((4, 4), dtype=torch.int32)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.image_resize_u8(torch.zeros((4, 4, 3), dtype=torch.uint8), tab, tab, torch.zeros((1, 4, 4, 3)))
    with pytest.raises(ValueError, match="no CPU path"):
        ops.mask_resize(torch.zeros((4, 4, 1)), tab, tab, torch.zeros((4, 4), dtype=torch.uint8))


def test_entry_points_refuse_bad_channel_counts():
    """c outside {1, 3} and ncls outside 1..255 are refused on the host side of the ABI (the
    pointers are never dereferenced: the refusal comes before any launch)."""
    import ctypes
    from unet_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(256)
    assert lib.unet_image_resize_u8(p, 4, 4, 2, p, p, 4, 4, 0, p, None) < 0
    assert b"c must be 1 or 3" in lib.unet_last_error()
    assert lib.unet_image_resize_u8(p, 4, 0, 3, p, p, 4, 4, 0, p, None) < 0
    assert lib.unet_mask_resize(p, 4, 4, 256, p, p, 4, 4, 0.5, p, None) < 0
    assert b"ncls must be 1..255" in lib.unet_last_error()
    assert lib.unet_mask_resize(p, 4, 4, 1, p, p, -1, 4, 0.5, p, None) < 0
