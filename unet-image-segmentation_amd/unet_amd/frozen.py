"""Frozen inference: the engine's counterpart of the reference's deployment step
(scripts/tensorflow_lite/convert_to_tflite.py --float16, and the int8 mode with a representative
dataset that the converter names next).

`fold_weights` is pure NumPy (float64): BatchNormalization (model/u_net.py:22-23, eps 1e-3) folds
into the pointwise kernel and a bias, and the matrix-core operands are rounded to fp16.
`FrozenUNet` runs the folded network on the fp16 kernels of csrc/frozen.hip (the fp16 precision of
the kernel skeleton csrc/frozen_common.h): activations travel
as fp16, already activated (ReLU at the producer, max-pool written by the producer), the
pointwise GEMMs are one fp16 MFMA product per step with fp32 accumulation.

Rounding to fp16 (nearest even) happens at exactly four places: the folded pointwise / upsample
kernels (here), each block's depthwise output, each block's output after bias + ReLU, each
upsample's output after bias.  Everything else is fp32.

The int8 format (`quantize_weights`, `collect_ranges`, `FrozenUNetI8`, csrc/frozen_i8.hip) stores
activations as one byte with per-tensor scales from a calibration run and multiplies on the int8
MFMA; its arithmetic contract is written out in include/unet_hip.h ("Frozen int8 inference").
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np

BN_EPS = 1e-3  # keras.layers.BatchNormalization default
F16_MAX = 65504.0
FORMAT_VERSION = 1       # float16 archives
FORMAT_VERSION_INT8 = 2  # int8 archives
_FORMATS = {"float16": FORMAT_VERSION, "int8": FORMAT_VERSION_INT8}
MARKER = "__frozen_unet__"
IMAGE_BLOCK = "enc1_block1"


def block_names(filters: Sequence[int]):
    """The conv blocks in forward order."""
    n = len(filters)
    names = []
    for i in range(n):
        names += [f"enc{i + 1}_block1", f"enc{i + 1}_block2"]
    names += ["bneck_block1", "bneck_block2"]
    for i in range(n):
        names += [f"dec{n - i}_block1", f"dec{n - i}_block2"]
    return names


def activation_names(filters: Sequence[int]):
    """Every name FrozenUNet.activation() serves."""
    n = len(filters)
    return (block_names(filters) + [f"dec{n - i}_upsample" for i in range(n)]
            + [f"enc{i + 1}_pool" for i in range(n)])


def _checked(name: str, a: np.ndarray) -> np.ndarray:
    if not np.all(np.isfinite(a)):
        raise ValueError(f"{name}: folded values are not finite")
    if a.size and np.abs(a).max() > F16_MAX:
        raise ValueError(f"{name}: folded magnitude {np.abs(a).max():.6g} exceeds the fp16 range ({F16_MAX:g})")
    return a


def fold_exact(weights: Dict[str, np.ndarray], num_classes: int, use_batch_norm: bool,
               filters: Sequence[int]) -> Dict[str, np.ndarray]:
    """The frozen network's variables in float64, before any rounding: per block
    `depthwise_kernel`, `pointwise_kernel` (BatchNorm scale folded in) and `bias`; the upsample and
    head variables unchanged.  The same function as the source model's inference forward."""
    filters = tuple(int(f) for f in filters)
    out: Dict[str, np.ndarray] = {}

    def w64(name):
        if name not in weights:
            raise ValueError(f"missing variable {name}")
        return np.asarray(weights[name], np.float64)

    for b in block_names(filters):
        pk = w64(f"{b}_sepconv/pointwise_kernel")
        if use_batch_norm:
            scale = w64(f"{b}_bn/gamma") / np.sqrt(w64(f"{b}_bn/moving_variance") + BN_EPS)
            pw = pk * scale
            bias = w64(f"{b}_bn/beta") - w64(f"{b}_bn/moving_mean") * scale
        else:
            pw, bias = pk, w64(f"{b}_sepconv/bias")
        out[f"{b}_sepconv/depthwise_kernel"] = w64(f"{b}_sepconv/depthwise_kernel")
        out[f"{b}_sepconv/pointwise_kernel"] = pw
        out[f"{b}_sepconv/bias"] = bias
    for i in range(len(filters)):
        s = f"dec{len(filters) - i}_upsample"
        out[f"{s}/kernel"] = w64(f"{s}/kernel")
        out[f"{s}/bias"] = w64(f"{s}/bias")
    out["output_mask/kernel"] = w64("output_mask/kernel")
    out["output_mask/bias"] = w64("output_mask/bias")
    if out["output_mask/kernel"].shape[-1] != num_classes:
        raise ValueError(f"output_mask/kernel has {out['output_mask/kernel'].shape[-1]} classes, "
                         f"expected {num_classes}")
    return out


def fold_weights(weights: Dict[str, np.ndarray], num_classes: int, use_batch_norm: bool,
                 filters: Sequence[int]) -> Dict[str, np.ndarray]:
    """Fold a trained model's variables (Keras names and layouts) into the frozen network's:
    per block `depthwise_kernel` (fp32), `pointwise_kernel` (fp16; fp32 for the image block) and
    `bias` (fp32); `decN_upsample/kernel` fp16 with an fp32 bias; the head in fp32.  Computed in
    float64 (fold_exact), then rounded.  ValueError names the variable whose folded values are
    not finite or exceed the fp16 range, and refuses widths that are not multiples of 32."""
    filters = tuple(int(f) for f in filters)
    for f in filters:
        if f <= 0 or f % 32:
            raise ValueError(f"filters {filters}: the fp16 kernels need widths that are multiples of 32, got {f}")
    half = {f"{b}_sepconv/pointwise_kernel" for b in block_names(filters) if b != IMAGE_BLOCK}
    half |= {f"dec{i + 1}_upsample/kernel" for i in range(len(filters))}
    return {name: _checked(name, a).astype(np.float16 if name in half else np.float32)
            for name, a in fold_exact(weights, num_classes, use_batch_norm, filters).items()}


# ---------------------------------------------------------------------- the artefact ---
def to_archive(folded: Dict[str, np.ndarray], input_size, num_classes: int, filters,
               dtype: str = "float16") -> Dict[str, np.ndarray]:
    """The arrays of a frozen .npz: the folded variables in Keras layouts (':' for '/'), the
    geometry, the dtype, a format version (1 for float16, 2 for int8: the arrays are then those of
    quantize_weights) and the marker key."""
    if dtype not in _FORMATS:
        raise ValueError(f"frozen dtype {dtype!r}: float16 and int8 exist")
    arc = {k.replace("/", ":"): np.ascontiguousarray(v) if np.ndim(v) else np.asarray(v)  # (0-d: the int8 scales)
           for k, v in folded.items()}
    arc[MARKER] = np.asarray(1, np.int32)
    arc["format_version"] = np.asarray(_FORMATS[dtype], np.int32)
    arc["dtype"] = np.asarray(dtype)
    arc["input_size"] = np.asarray(tuple(int(v) for v in input_size), np.int32)
    arc["num_classes"] = np.asarray(int(num_classes), np.int32)
    arc["filters"] = np.asarray(tuple(int(f) for f in filters), np.int32)
    return arc


_META = (MARKER, "format_version", "dtype", "input_size", "num_classes", "filters")


def from_archive(arc) -> Tuple[Dict[str, np.ndarray], dict]:
    """Inverse of to_archive over any mapping of arrays (an open NpzFile included)."""
    keys = list(arc.files) if hasattr(arc, "files") else list(arc)
    if MARKER not in keys:
        raise ValueError("not a frozen U-Net file (marker key missing)")
    version = int(arc["format_version"])
    dtype = str(arc["dtype"])
    if dtype not in _FORMATS:
        raise ValueError(f"frozen file dtype {dtype!r}: this build reads float16 (format 1) and int8 (format 2)")
    if version != _FORMATS[dtype]:
        raise ValueError(f"frozen file format {version} with dtype {dtype!r}: this build reads "
                         f"format {_FORMATS[dtype]} for {dtype}")
    meta = {"input_size": tuple(int(v) for v in arc["input_size"]), "num_classes": int(arc["num_classes"]),
            "filters": tuple(int(v) for v in arc["filters"]), "dtype": dtype}
    folded = {k.replace(":", "/"): np.asarray(arc[k]) for k in keys if k not in _META}
    return folded, meta


def save_archive(path, arc: Dict[str, np.ndarray]) -> None:
    with open(path, "wb") as f:  # the exact path given (np.savez would append .npz to a name)
        np.savez(f, **arc)


def load_archive(path) -> Tuple[Dict[str, np.ndarray], dict]:
    with open(path, "rb") as f, np.load(f, allow_pickle=False) as z:
        return from_archive(z)


def is_frozen_file(path) -> bool:
    """True when `path` is an .npz carrying the frozen marker (any other file: False)."""
    try:
        with open(path, "rb") as f, np.load(f, allow_pickle=False) as z:
            return MARKER in z.files
    except Exception:  # unreadable, not a zip archive, a bare .npy, ...: the caller's loader reports it
        return False


# ------------------------------------------------------------------------ the network ---
class FrozenUNet:
    """A frozen fp16 copy of a U-Net: inference only, its own weights."""

    DTYPE = "float16"

    def __init__(self, folded: Dict[str, np.ndarray], input_size, num_classes: int, filters, device=None):
        import torch

        from . import _lib as L
        from .params import check_input_size
        if not torch.cuda.is_available():
            raise RuntimeError("FrozenUNet needs a HIP device (MI355X); there is no CPU execution path")
        L.load()
        self.filters = tuple(int(f) for f in filters)
        self.h, self.w, self.c = check_input_size(input_size, len(self.filters))
        if self.c > 4:
            raise ValueError(f"the image block takes at most 4 input channels, got {self.c}")
        self.num_classes = int(num_classes)
        self.dtype = self.DTYPE
        self.device = torch.device(device if device is not None else "cuda")
        self.folded = {k: np.array(v, copy=True) for k, v in folded.items()}  # Keras layouts, host
        self._dev: Dict[str, "torch.Tensor"] = {}
        self._pack()
        self._bufs: Dict[int, dict] = {}
        self._kept: Dict[str, "torch.Tensor"] = {}

    # ------------------------------------------------------------------ construction ---
    @classmethod
    def from_model(cls, model, dtype: str = "float16", calibration=None, batch_size=None) -> "FrozenUNet":
        if dtype not in _FORMATS:
            raise ValueError(f"freeze(dtype={dtype!r}): float16 and int8 are the frozen formats")
        if dtype == "int8" and calibration is None:
            raise ValueError("freeze(dtype='int8') needs calibration data (a representative dataset): "
                             "pass calibration=images (N, H, W, C)")
        e = model.engine
        weights = e.get_weights_dict()
        geom = ((e.h, e.w, e.c), e.num_classes, e.filters, e.device)
        half = FrozenUNet(fold_weights(weights, e.num_classes, e.use_bn, e.filters), *geom)
        if dtype == "float16":
            return half
        ranges = collect_ranges(half, calibration, batch_size)
        half.release_buffers()
        quant = quantize_weights(fold_exact(weights, e.num_classes, e.use_bn, e.filters), ranges, e.filters)
        return FrozenUNetI8(quant, *geom)

    def _pack(self):
        """Device operands: pointwise kernels as [cout][cin] fp16 (k contiguous, the MFMA B
        layout), everything else flat in its Keras layout."""
        import torch

        def put(a):
            return torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

        f = self.folded
        for b in block_names(self.filters):
            pk = f[f"{b}_sepconv/pointwise_kernel"][0, 0]
            self._dev[f"{b}/dw"] = put(f[f"{b}_sepconv/depthwise_kernel"].astype(np.float32).reshape(-1))
            self._dev[f"{b}/pw"] = put(pk.astype(np.float32) if b == IMAGE_BLOCK else pk.T.astype(np.float16))
            self._dev[f"{b}/bias"] = put(f[f"{b}_sepconv/bias"].astype(np.float32))
        for i in range(len(self.filters)):
            s = f"dec{i + 1}_upsample"
            self._dev[f"{s}/k"] = put(f[f"{s}/kernel"].astype(np.float16))
            self._dev[f"{s}/bias"] = put(f[f"{s}/bias"].astype(np.float32))
        self._dev["head/k"] = put(f["output_mask/kernel"].astype(np.float32).reshape(-1))
        self._dev["head/bias"] = put(f["output_mask/bias"].astype(np.float32))

    # ---------------------------------------------------------------------- file i/o ---
    def archive(self) -> Dict[str, np.ndarray]:
        return to_archive(self.folded, (self.h, self.w, self.c), self.num_classes, self.filters, self.dtype)

    def save(self, path) -> None:
        save_archive(path, self.archive())

    @classmethod
    def load(cls, path, device=None) -> "FrozenUNet":
        """The network of a frozen file, of the kind its dtype names (FrozenUNet or FrozenUNetI8)."""
        folded, meta = load_archive(path)
        kind = FrozenUNetI8 if meta["dtype"] == "int8" else FrozenUNet
        return kind(folded, meta["input_size"], meta["num_classes"], meta["filters"], device)

    # ----------------------------------------------------------------------- forward ---
    def _buffers(self, n: int) -> dict:
        """Per batch size: the four skips, their pooled copies and one pair of ping-pong buffers."""
        import torch
        b = self._bufs.get(n)
        if b is None:
            def e(*shape):
                return torch.empty(shape, dtype=self._act_dtype(), device=self.device)
            b = {"skip": [], "pool": []}
            h, w = self.h, self.w
            for f in self.filters:
                b["skip"].append(e(n, h, w, f))
                b["pool"].append(e(n, h // 2, w // 2, f))
                h, w = h // 2, w // 2
            big = n * self.h * self.w * self.filters[0]  # the largest activation (full resolution)
            b["ping"] = [e(big), e(big)]
            self._bufs[n] = b
        return b

    def _act_dtype(self, signed: bool = False):
        """dtype of an activation buffer (`signed`: an upsample's output)."""
        import torch
        return torch.float16

    def release_buffers(self):
        self._bufs.clear()
        self._kept.clear()

    # the per-layer launches: what a precision overrides
    def _view(self):
        from .ops import F16View
        return F16View

    def _image_block(self, name, x, n, h, w, cout, out):
        from . import ops
        d = self._dev
        ops.f16_image_block(x, n, h, w, self.c, d[f"{name}/dw"], cout, d[f"{name}/pw"], d[f"{name}/bias"], out)

    def _block(self, name, view, n, h, w, cout, out, pool=None):
        from . import ops
        d = self._dev
        ops.f16_sepconv(view, n, h, w, d[f"{name}/dw"], cout, d[f"{name}/pw"], d[f"{name}/bias"], out, pool)

    def _upsample(self, name, a, n, h, w, cin, cout, out):
        from . import ops
        d = self._dev
        ops.f16_conv_transpose2x2(a, n, h, w, cin, cout, d[f"{name}/k"], d[f"{name}/bias"], out)

    def _head(self, a, n, h, w, cin, prob):
        from . import ops
        d = self._dev
        ops.f16_head(a, n, h, w, cin, self.num_classes, d["head/k"], d["head/bias"], prob)

    def forward(self, x, keep_activations: bool = False):
        """x: fp32 device tensor (N, H, W, C).  Returns fp32 probabilities (N, H, W, classes) in a
        new tensor.  keep_activations: every layer's output (fp16; uint8 / int8 for the int8 network)
        stays readable by activation()."""
        import torch

        if x.dim() != 4 or tuple(x.shape[1:]) != (self.h, self.w, self.c):
            raise ValueError(f"expected input (N, {self.h}, {self.w}, {self.c}), got {tuple(x.shape)}")
        n = int(x.shape[0])
        fl, View = self.filters, self._view()
        self._kept = {}
        bufs = None if keep_activations else self._buffers(n)
        state = {"cur": 0}

        def new(name, h, w, c, fixed=None, signed=False):
            dt = self._act_dtype(signed)
            if keep_activations:
                t = torch.empty((n, h, w, c), dtype=dt, device=self.device)
                self._kept[name] = t
                return t
            if fixed is not None:
                return fixed
            state["cur"] ^= 1
            return bufs["ping"][state["cur"]][:n * h * w * c].view(dt).view(n, h, w, c)

        def block(name, view, h, w, cout, out, pool=None):
            self._block(name, view, n, h, w, cout, out, pool)
            return out

        h, w = self.h, self.w
        skips = []
        a = None
        for i, f in enumerate(fl):
            s = f"enc{i + 1}"
            out = new(f"{s}_block1", h, w, f)
            if i == 0:
                self._image_block(f"{s}_block1", x, n, h, w, f, out)
            else:
                block(f"{s}_block1", View.plain(a), h, w, f, out)
            skip = new(f"{s}_block2", h, w, f, None if bufs is None else bufs["skip"][i])
            pool = new(f"{s}_pool", h // 2, w // 2, f, None if bufs is None else bufs["pool"][i])
            block(f"{s}_block2", View.plain(out), h, w, f, skip, pool)
            skips.append(skip)
            a = pool
            h, w = h // 2, w // 2
        c = fl[-1] * 2
        a = block("bneck_block1", View.plain(a), h, w, c, new("bneck_block1", h, w, c))
        a = block("bneck_block2", View.plain(a), h, w, c, new("bneck_block2", h, w, c))
        for i in range(len(fl)):
            stage = len(fl) - i
            f = fl[stage - 1]
            s = f"dec{stage}"
            up = new(f"{s}_upsample", 2 * h, 2 * w, f, signed=True)
            self._upsample(f"{s}_upsample", a, n, h, w, c, f, up)
            h, w = 2 * h, 2 * w
            a = block(f"{s}_block1", View.concat(up, skips[stage - 1]), h, w, f, new(f"{s}_block1", h, w, f))
            a = block(f"{s}_block2", View.plain(a), h, w, f, new(f"{s}_block2", h, w, f))
            c = f
        prob = torch.empty((n, h, w, self.num_classes), dtype=torch.float32, device=self.device)
        self._head(a, n, h, w, c, prob)
        return prob

    __call__ = forward

    def activation(self, name: str):
        """The fp16 output of layer `name` from the last forward(x, keep_activations=True)."""
        if name not in activation_names(self.filters):
            raise KeyError(f"unknown activation {name!r}")
        if name not in self._kept:
            raise RuntimeError("run forward(x, keep_activations=True) first")
        return self._kept[name]

    def predict(self, x, batch_size: Optional[int] = None, verbose: int = 0):
        """UNetModel.predict's contract: numpy in -> numpy out, tensor in -> device tensor out."""
        import torch

        from .metrics import as_device_tensor
        is_np = not isinstance(x, torch.Tensor)
        xt = as_device_tensor(x, self.device)
        bs = batch_size or 32
        outs = [self.forward(xt[i:i + bs]) for i in range(0, xt.shape[0], bs)]
        out = torch.cat(outs, 0) if len(outs) > 1 else outs[0]
        return out.cpu().numpy() if is_np else out

    def predict_masks(self, images, threshold: float = 0.5, batch_size: int = 32, bgr: bool = True,
                      return_probs: bool = False, return_boxes: bool = False):
        """uint8 images as decoded, of any sizes -> uint8 masks at the images' sizes, the resizes on
        the device; return_boxes=True adds each mask's largest-contour crop rectangle, found on the
        device too (unet_amd.pipeline.predict_masks)."""
        from .pipeline import predict_masks
        return predict_masks(self, images, threshold, batch_size, bgr, return_probs, return_boxes)


# ------------------------------------------------------------------------ int8 format ---
def calibration_names(filters: Sequence[int]):
    """Every tensor whose range quantize_weights needs: the activations, and `<block>/y` (the
    depthwise output, the int8 MFMA's A operand) for each block but the image block."""
    return activation_names(filters) + [f"{b}/y" for b in block_names(filters) if b != IMAGE_BLOCK]


def block_inputs(filters: Sequence[int]) -> Dict[str, Tuple[str, ...]]:
    """{block: the activations its input is made of}: one name, or (upsample, skip) for a concat."""
    n = len(filters)
    src: Dict[str, Tuple[str, ...]] = {}
    for i in range(n):
        if i:
            src[f"enc{i + 1}_block1"] = (f"enc{i}_pool",)
        src[f"enc{i + 1}_block2"] = (f"enc{i + 1}_block1",)
    src["bneck_block1"] = (f"enc{n}_pool",)
    src["bneck_block2"] = ("bneck_block1",)
    for i in range(n, 0, -1):
        src[f"dec{i}_block1"] = (f"dec{i}_upsample", f"enc{i}_block2")
        src[f"dec{i}_block2"] = (f"dec{i}_block1",)
    return src


def _scale(name: str, ranges, levels: int) -> float:
    if name not in ranges:
        raise ValueError(f"{name}: no calibration range")
    r = float(ranges[name])
    if not np.isfinite(r) or r < 0.0:
        raise ValueError(f"{name}: calibration range {r!r} is negative or not finite")
    return r / levels if r > 0.0 else 1.0


def _quantize_rows(name: str, a: np.ndarray):
    """a (..., k) float64 -> (int8 of the same shape, scale per row = max|row| / 127, 1 for a zero row)."""
    if not np.all(np.isfinite(a)):
        raise ValueError(f"{name}: folded values are not finite")
    mx = np.abs(a).max(axis=-1)
    s = np.where(mx > 0.0, mx / 127.0, 1.0)
    q = np.clip(np.rint(a / s[..., None]), -127, 127).astype(np.int8)
    return q, s


def quantize_weights(exact: Dict[str, np.ndarray], ranges: Dict[str, float], filters: Sequence[int]
                     ) -> Dict[str, np.ndarray]:
    """The int8 network's operands from fold_exact(...) and the calibration ranges (max |.| of every
    calibration_names tensor).  Pure NumPy, float64, rounded once at the end.  Per block `<b>/taps`
    (fp32 [9][C] = dw s_in / s_y), `<b>/pw_q` (int8 [cout][C]), `<b>/mult`, `<b>/bias_q` (fp32 [cout]);
    the image block keeps `/dw`, `/pw`, `/bias` in fp32; per upsample `/kernel_q` (int8, Keras
    (2, 2, cout, cin)), `/colsum` (int32 [4 cout]), `/mult` (fp32 [4 cout]), `/bias_q` (fp32 [cout]);
    `head/kernel` (fp32, the input scale folded in) and `head/bias`; `scale/<name>` (float64) for
    every calibration_names tensor (uint8 max / 255 after a ReLU, int8 max / 127 for upsamples and
    `<b>/y`, 1 for an all-zero tensor; a pool shares its block's scale).  ValueError names the
    tensor whose range is missing, negative or not finite."""
    filters = tuple(int(f) for f in filters)
    for f in filters:
        if f <= 0 or f % 32:
            raise ValueError(f"filters {filters}: the int8 kernels need widths that are multiples of 32, got {f}")
    n = len(filters)
    ups = [f"dec{i + 1}_upsample" for i in range(n)]
    scale: Dict[str, float] = {}
    for name in calibration_names(filters):
        signed = name in ups or name.endswith("/y")
        scale[name] = _scale(name, ranges, 127 if signed else 255)
    for i in range(n):  # the pool is the max of the block's bytes: one scale
        scale[f"enc{i + 1}_pool"] = scale[f"enc{i + 1}_block2"]
    out: Dict[str, np.ndarray] = {}
    f32 = np.float32
    inputs = block_inputs(filters)
    for b in block_names(filters):
        dw = np.asarray(exact[f"{b}_sepconv/depthwise_kernel"], np.float64)
        pw = np.asarray(exact[f"{b}_sepconv/pointwise_kernel"], np.float64)[0, 0]  # (cin, cout)
        bias = np.asarray(exact[f"{b}_sepconv/bias"], np.float64)
        for nm, a in (("depthwise_kernel", dw), ("bias", bias)):
            if not np.all(np.isfinite(a)):
                raise ValueError(f"{b}_sepconv/{nm}: folded values are not finite")
        s_out = scale[b]
        if b == IMAGE_BLOCK:
            if not np.all(np.isfinite(pw)):
                raise ValueError(f"{b}_sepconv/pointwise_kernel: folded values are not finite")
            out[f"{b}/dw"], out[f"{b}/pw"], out[f"{b}/bias"] = dw.astype(f32), pw.astype(f32), bias.astype(f32)
            continue
        s_in = np.concatenate([np.full(ch, scale[src]) for src, ch in
                               zip(inputs[b], _split_channels(inputs[b], dw.shape[2]))])
        s_y = scale[f"{b}/y"]
        out[f"{b}/taps"] = (dw.reshape(9, -1) * s_in / s_y).astype(f32)
        q, s_w = _quantize_rows(f"{b}_sepconv/pointwise_kernel", pw.T)
        out[f"{b}/pw_q"] = np.ascontiguousarray(q)
        out[f"{b}/mult"] = (s_y * s_w / s_out).astype(f32)
        out[f"{b}/bias_q"] = (bias / s_out).astype(f32)
    for i in range(n):
        s = ups[i]
        src = "bneck_block2" if i == n - 1 else f"dec{i + 2}_block2"
        k = np.asarray(exact[f"{s}/kernel"], np.float64)  # (2, 2, cout, cin)
        bias = np.asarray(exact[f"{s}/bias"], np.float64)
        if not np.all(np.isfinite(bias)):
            raise ValueError(f"{s}/bias: values are not finite")
        q, s_w = _quantize_rows(f"{s}/kernel", k)
        out[f"{s}/kernel_q"] = q
        out[f"{s}/colsum"] = q.astype(np.int32).sum(axis=-1).reshape(-1).astype(np.int32)
        out[f"{s}/mult"] = (scale[src] * s_w / scale[s]).reshape(-1).astype(f32)
        out[f"{s}/bias_q"] = (bias / scale[s]).astype(f32)
    hk = np.asarray(exact["output_mask/kernel"], np.float64)[0, 0]  # (cin, classes)
    out["head/kernel"] = (hk * scale["dec1_block2"]).astype(f32)
    out["head/bias"] = np.asarray(exact["output_mask/bias"], np.float64).astype(f32)
    for name, v in scale.items():
        out[f"scale/{name}"] = np.asarray(v, np.float64)
    return out


def _split_channels(sources, channels: int):
    """Channel counts of a block input's sources: all of them, or (upsample, skip) halves."""
    return (channels,) if len(sources) == 1 else (channels // 2, channels - channels // 2)


def collect_ranges(model_or_frozen, x, batch_size: Optional[int] = None) -> Dict[str, float]:
    """Calibration: max |.| of every calibration_names tensor over the images x (numpy array or
    device tensor (N, H, W, C)).  Runs the fp16 FrozenUNet with keep_activations per batch and
    keeps running maxima; each `<block>/y` is the fp32 depthwise 3x3 of the kept block input.  The
    result does not depend on batch_size.  Needs the GPU; off the hot path."""
    import torch
    import torch.nn.functional as tf

    from .metrics import as_device_tensor
    net = model_or_frozen if isinstance(model_or_frozen, FrozenUNet) else FrozenUNet.from_model(model_or_frozen)
    if net.dtype != "float16":
        raise ValueError("collect_ranges runs the float16 frozen network")
    xt = as_device_tensor(x, net.device)
    if xt.dim() != 4 or xt.shape[0] == 0:
        raise ValueError(f"calibration data must be (N, H, W, C) with N > 0, got {tuple(xt.shape)}")
    bs = int(batch_size or 32)
    names = activation_names(net.filters)
    inputs = block_inputs(net.filters)
    best: Dict[str, "torch.Tensor"] = {}

    def track(name, t):
        m = t.abs().max().float()
        best[name] = m if name not in best else torch.maximum(best[name], m)

    for i in range(0, xt.shape[0], bs):
        net.forward(xt[i:i + bs], keep_activations=True)
        for name in names:
            track(name, net.activation(name))
        for b, srcs in inputs.items():
            a = torch.cat([net.activation(s) for s in srcs], dim=-1).float()
            n, h, w, c = a.shape
            dw = net._dev[f"{b}/dw"].view(3, 3, c).float()
            # nine taps summed in a fixed order, element by element: the value of a pixel does not
            # depend on the batch it is in (a library convolution may pick its algorithm, and with it
            # the summation order, from the batch size)
            ap = tf.pad(a, (0, 0, 1, 1, 1, 1))
            y = ap[:, 0:h, 0:w] * dw[0, 0]
            for t in range(1, 9):
                y = y + ap[:, t // 3:t // 3 + h, t % 3:t % 3 + w] * dw[t // 3, t % 3]
            track(f"{b}/y", y)
    net._kept = {}
    return {k: float(v.item()) for k, v in best.items()}


class FrozenUNetI8(FrozenUNet):
    """A frozen int8 copy of a U-Net (quantize_weights' operands on the kernels of
    csrc/frozen_i8.hip): FrozenUNet's interface and graph walk, one-byte activations.  activation(name) returns
    the uint8 / int8 bytes q, activation_scale(name) the s of x = s q."""

    DTYPE = "int8"

    def _act_dtype(self, signed: bool = False):
        import torch
        return torch.int8 if signed else torch.uint8

    def _pack(self):
        import torch

        def put(a):
            return torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

        f = self.folded
        for name in calibration_names(self.filters):
            if f"scale/{name}" not in f:
                raise ValueError(f"int8 frozen network: scale/{name} is missing")
        for k, v in f.items():
            if not k.startswith("scale/"):
                self._dev[k] = put(v.reshape(-1))

    def activation_scale(self, name: str) -> float:
        """s of x = s q for activation(name) (or for `<block>/y`)."""
        if name not in calibration_names(self.filters):
            raise KeyError(f"unknown activation {name!r}")
        return float(self.folded[f"scale/{name}"])

    def _view(self):
        from .ops import I8View
        return I8View

    def _image_block(self, name, x, n, h, w, cout, out):
        from . import ops
        d = self._dev
        ops.i8_image_block(x, n, h, w, self.c, d[f"{name}/dw"], cout, d[f"{name}/pw"], d[f"{name}/bias"],
                           float(np.float32(self.folded[f"scale/{name}"])), out)

    def _block(self, name, view, n, h, w, cout, out, pool=None):
        from . import ops
        d = self._dev
        ops.i8_sepconv(view, n, h, w, d[f"{name}/taps"], cout, d[f"{name}/pw_q"], d[f"{name}/mult"],
                       d[f"{name}/bias_q"], out, pool)

    def _upsample(self, name, a, n, h, w, cin, cout, out):
        from . import ops
        d = self._dev
        ops.i8_conv_transpose2x2(a, n, h, w, cin, cout, d[f"{name}/kernel_q"], d[f"{name}/colsum"], d[f"{name}/mult"],
                                 d[f"{name}/bias_q"], out)

    def _head(self, a, n, h, w, cin, prob):
        from . import ops
        d = self._dev
        ops.i8_head(a, n, h, w, cin, self.num_classes, d["head/kernel"], d["head/bias"], prob)
