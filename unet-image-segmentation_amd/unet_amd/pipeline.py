"""Image in, mask out, with the image steps on the device.

The reference CLIs wrap the forward in host image processing (scripts/inference.py:105-108 and
:147-160, scripts/benchmark.py:105): the decoded uint8 image is scaled by 1/255 and resized
bilinearly to the model size, and the probability map is resized back to the image's size and
thresholded.  unet_amd/imageproc.py restates those steps in NumPy; this module runs the same
arithmetic in two kernels (ops.image_resize_u8, ops.mask_resize), bitwise equal to the NumPy
functions, so that a caller hands over images as decoded and gets masks at the images' sizes:

    masks = model.predict_masks([img0, img1, ...])      # UNetModel, FrozenUNet or FrozenUNetI8

Per chunk of images: one upload from pinned memory, one resize launch per image into one batch
tensor, one model.predict, one mask launch per image, one copy back, one synchronisation.
Everything is issued on the current stream.

    masks, boxes = model.predict_masks(images, return_boxes=True)

also runs the last step of scripts/inference.py on the device (ops.mask_largest_contour, after each
image's mask launch): boxes[i] is imageproc.largest_external_contour(masks[i]), the crop rectangle.
The 32-byte records ride in the chunk's one copy back.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import List, Sequence, Tuple

import numpy as np

from .imageproc import linear_coords

# A chunk's uint8 images are staged in one pinned buffer; a chunk ends at batch_size images or
# when the next image would take the staged bytes past this (32 images of 3000 x 4000 x 3 would pin
# 1.1 GB).  One image always fits a chunk, whatever its size.
STAGE_BYTES = 256 << 20
_TABLES_MAX = 512

_tables: "OrderedDict[tuple, object]" = OrderedDict()
_staging = {}  # (kind, device index) -> pinned uint8 tensor, grown on demand


def coord_table(n_out: int, n_in: int, device):
    """linear_coords(n_out, n_in) as the device table the kernels read: int32 (n_out, 4) holding
    i0, i1, the float32 weight's bits and 0 (`unet_lerp_coord`).  Cached per (device, n_out, n_in)."""
    import torch
    device = torch.device(device)
    key = (device.index if device.index is not None else torch.cuda.current_device(), int(n_out), int(n_in))
    t = _tables.get(key)
    if t is None:
        i0, i1, frac = linear_coords(int(n_out), int(n_in))
        host = np.zeros((int(n_out), 4), np.int32)
        host[:, 0] = i0
        host[:, 1] = i1
        host[:, 2] = frac.view(np.int32)
        t = torch.from_numpy(host).to(device)  # from pageable memory: complete when this returns
        _tables[key] = t
        if len(_tables) > _TABLES_MAX:
            _tables.popitem(last=False)
    else:
        _tables.move_to_end(key)
    return t


def model_geometry(model) -> Tuple[int, int, int, int, object]:
    """(h, w, c, num_classes, device) of a UNetModel or a FrozenUNet."""
    e = getattr(model, "engine", model)
    return int(e.h), int(e.w), int(e.c), int(e.num_classes), e.device


def _is_tensor(a) -> bool:
    return type(a).__module__.split(".")[0] == "torch"


def check_images(images: Sequence, channels: int) -> None:
    """ValueError for anything but non-empty uint8 (h, w, channels) images; touches no device."""
    if isinstance(images, np.ndarray) and images.ndim == 3 or _is_tensor(images) and images.dim() == 3:
        raise ValueError("images must be a list of (h, w, c) images, not one image")
    for i, a in enumerate(images):
        if a is None or not hasattr(a, "shape") or not hasattr(a, "dtype"):
            raise ValueError(f"images[{i}]: expected a uint8 (h, w, {channels}) array or device tensor, got {a!r}")
        if "uint8" not in str(a.dtype):
            raise ValueError(f"images[{i}]: expected uint8 as decoded, got {a.dtype}")
        shape = tuple(int(v) for v in a.shape)
        if len(shape) == 2 and channels == 1:
            shape = shape + (1,)
        if len(shape) != 3 or shape[2] != channels:
            raise ValueError(f"images[{i}]: expected (h, w, {channels}) for this model, got {tuple(a.shape)}")
        if shape[0] < 1 or shape[1] < 1:
            raise ValueError(f"images[{i}]: empty image {tuple(a.shape)}")


def _pinned(kind: str, nbytes: int, device):
    import torch
    key = (kind, device.index)
    buf = _staging.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = _staging[key] = torch.empty(max(int(nbytes * 1.25), 1 << 20), dtype=torch.uint8, pin_memory=True)
    return buf


def _chunks(images: Sequence, batch_size: int) -> List[Tuple[int, int]]:
    out, start, staged = [], 0, 0
    for i, a in enumerate(images):
        nb = 0 if _is_tensor(a) else int(np.prod(a.shape))
        if i > start and (i - start == batch_size or staged + nb > STAGE_BYTES):
            out.append((start, i))
            start, staged = i, 0
        staged += nb
    if len(images) > start:
        out.append((start, len(images)))
    return out


def _upload(images: Sequence, c: int, device) -> list:
    """Device uint8 (h, w, c) tensors of one chunk: the host arrays go through one pinned buffer
    and one asynchronous copy; device tensors are taken as they are."""
    import torch
    host = [(i, np.ascontiguousarray(a).reshape(a.shape[0], a.shape[1], c))
            for i, a in enumerate(images) if not _is_tensor(a)]
    out = [None if not _is_tensor(a) else a.to(device).contiguous().reshape(a.shape[0], a.shape[1], c)
           for a in images]
    total = sum(a.size for _, a in host)
    if total:
        stage = _pinned("in", total, device)
        view = stage.numpy()
        off = 0
        for _, a in host:
            view[off:off + a.size] = a.reshape(-1)
            off += a.size
        dev = torch.empty(total, dtype=torch.uint8, device=device)
        dev.copy_(stage[:total], non_blocking=True)
        off = 0
        for i, a in host:
            out[i] = dev[off:off + a.size].view(a.shape)
            off += a.size
    return out


def preprocess_images(images: Sequence, input_size, device, bgr: bool = True):
    """The fp32 device tensor (N, h, w, c) the network is fed for uint8 images of any sizes: each
    scaled by 1/255 and resized bilinearly to (h, w), bitwise
    resize_linear(img.astype(float32) / 255, h, w).  bgr=True reverses the channels first: the
    images are RGB as decoded and the network is fed BGR, as the reference CLIs feed it
    (cv2.imread order); bgr=False feeds the channels as given.  Issues no synchronisation: the
    caller must synchronise before the next call re-uses the staging buffer."""
    import torch

    from . import ops
    h, w, c = (int(v) for v in input_size)
    check_images(images, c)
    device = torch.device(device)
    x = torch.empty((len(images), h, w, c), dtype=torch.float32, device=device)
    for i, src in enumerate(_upload(images, c, device)):
        ops.image_resize_u8(src, coord_table(h, src.shape[0], device), coord_table(w, src.shape[1], device), x, i,
                            reverse_channels=bool(bgr) and c > 1)
    return x


def decode_contour_box(record):
    """32 bytes of a `unet_contour_box` (any buffer) -> what imageproc.largest_external_contour
    returns: None, or (area, (x, y, w, h)) with a float area and Python ints."""
    from ._lib import UnetContourBox
    b = UnetContourBox.from_buffer_copy(bytes(record))
    if b.count == 0:
        return None
    return b.area2 / 2.0, (int(b.x), int(b.y), int(b.w), int(b.h))


def predict_masks(model, images: Sequence, threshold: float = 0.5, batch_size: int = 32, bgr: bool = True,
                  return_probs: bool = False, return_boxes: bool = False):
    """uint8 images (h_i, w_i, c) of any, differing sizes -> a list of uint8 masks (h_i, w_i), each
    at its image's size: 255 where the probability, resized back bilinearly, is > threshold (one
    class), or the argmax class index (several classes; threshold is then unused).

    model: a UNetModel, FrozenUNet or FrozenUNetI8.  images: NumPy arrays or device tensors.  bgr: see
    preprocess_images.  return_probs=True returns (masks, probs, inputs): the device probabilities
    (N, H, W, classes) the masks were made from and the device tensor (N, H, W, c) the network was
    fed.  return_boxes=True appends boxes as the last element, (masks, boxes) or (masks, probs,
    inputs, boxes): boxes[i] is None (no foreground) or (area, (x, y, w, h)), the largest external
    contour of masks[i] found on the device, == imageproc.largest_external_contour(masks[i]);
    foreground is mask != 0, also for class-index masks.  ValueError, before the device is touched,
    for a non-uint8 image, a channel count other than the model's, an empty image and a threshold
    outside (0, 1)."""
    h, w, c, ncls, device = model_geometry(model)
    if not 0.0 < float(threshold) < 1.0:
        raise ValueError(f"threshold must be inside (0, 1), got {threshold}")
    if int(batch_size) < 1:
        raise ValueError(f"batch_size must be positive, got {batch_size}")
    images = list(images)
    check_images(images, c)
    import torch

    from . import ops
    device = torch.device(device)
    masks: List[np.ndarray] = []
    probs, inputs, boxes = [], [], []
    rec = ops.CONTOUR_BOX_BYTES
    with torch.cuda.device(device):
        for lo, hi in _chunks(images, int(batch_size)):
            chunk = images[lo:hi]
            x = preprocess_images(chunk, (h, w, c), device, bgr)
            prob = model.predict(x, batch_size=len(chunk))
            sizes = [(int(a.shape[0]), int(a.shape[1])) for a in chunk]
            npx = sum(a * b for a, b in sizes)
            box0 = -(-npx // rec) * rec  # the records follow the masks, aligned to their size
            total = box0 + rec * len(sizes) if return_boxes else npx
            dev = torch.empty(total, dtype=torch.uint8, device=device)
            off = 0
            for i, (ih, iw) in enumerate(sizes):
                m = dev[off:off + ih * iw].view(ih, iw)
                ops.mask_resize(prob[i], coord_table(ih, h, device), coord_table(iw, w, device), m, threshold)
                if return_boxes:
                    ops.mask_largest_contour(m, dev[box0 + rec * i:box0 + rec * (i + 1)])
                off += ih * iw
            stage = _pinned("out", total, device)
            stage[:total].copy_(dev, non_blocking=True)
            torch.cuda.current_stream(device).synchronize()  # the chunk's only wait
            flat = stage.numpy()
            off = 0
            for ih, iw in sizes:
                masks.append(flat[off:off + ih * iw].reshape(ih, iw).copy())
                off += ih * iw
            if return_boxes:
                boxes.extend(decode_contour_box(flat[box0 + rec * i:box0 + rec * (i + 1)]) for i in range(len(sizes)))
            if return_probs:
                probs.append(prob)
                inputs.append(x)
    if return_probs:
        cat = (lambda ts: ts[0] if len(ts) == 1 else torch.cat(ts, 0))
        empty = (lambda k: torch.empty((0, h, w, k), dtype=torch.float32, device=device))
        out = masks, (cat(probs) if probs else empty(ncls)), (cat(inputs) if inputs else empty(c))
        return out + (boxes,) if return_boxes else out
    return (masks, boxes) if return_boxes else masks
