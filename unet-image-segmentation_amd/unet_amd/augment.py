"""Random affine augmentation of the training input: the rotation / shift / shear / zoom arguments
of Keras' ImageDataGenerator (tf.keras 2.9 and later: `get_random_transform` and
`apply_affine_transform`), under Keras' names, for PairLoader and DevicePairLoader alike.

The host's part is small: per epoch one table of six parameters per sample, per batch position one
float64 matrix, rounded once to six fp32 numbers -- the transform record.  The warp itself is
`unet_batch_affine_u8` (csrc/batch.hip) on the device and `affine_u8_reference` below on the host,
the same fp32 arithmetic operation for operation, so the two loaders deliver the same bits.

    M = R(theta) @ T(tx, ty) @ S(shear) @ Z(zx, zy)        (Keras' matrices, axis 0 = rows)
    R = [[cos, -sin, 0], [sin, cos, 0], [0, 0, 1]]    T = [[1, 0, tx], [0, 1, ty], [0, 0, 1]]
    S = [[1, -sin(s), 0], [0, cos(s), 0], [0, 0, 1]]  Z = diag(zx, zy, 1)

conjugated about the centre (h/2 - 0.5, w/2 - 0.5); output pixel (r, q) samples the source at
M @ (r, q, 1).  Keras flips after the warp, so the horizontal flip is the substitution
q -> w - 1 - q in that map: the record carries it and the kernel knows no flips.

The exact TensorFlow / Keras random stream is not reproduced (data.py does not either)."""
from __future__ import annotations

import math

import numpy as np

FILL_MODES = ("nearest", "constant")
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def _range(name, v, below=None):
    v = float(v)
    if not math.isfinite(v) or v < 0:
        raise ValueError(f"{name} must be a finite number >= 0, got {v!r}")
    if below is not None and v >= below:
        raise ValueError(f"{name} must be a fraction of the image side in [0, {below}), got {v!r} "
                         f"(shifts in pixels are not supported)")
    return v


def _order(name, v):
    if isinstance(v, bool) or v not in (0, 1):
        raise ValueError(f"{name} must be 0 (nearest) or 1 (bilinear), got {v!r}")
    return int(v)


class Augment:
    """The settings of one augmented loader.  All ranges default to 0 = off; `active` is False then
    and a loader given such an object behaves exactly as one given none.

    rotation_range, shear_range: degrees.  height_shift_range, width_shift_range: fractions of the
    image side in [0, 1).  zoom_range: z for [1 - z, 1 + z], or (low, high).  fill_mode: "nearest"
    or "constant" with cval in 0..255 units.  frame_order / mask_order: the interpolation order of
    each (0 nearest, 1 bilinear; both 1 is what two Keras generators with equal arguments do,
    mask_order=0 keeps masks on their own grey levels)."""

    def __init__(self, rotation_range=0.0, width_shift_range=0.0, height_shift_range=0.0, shear_range=0.0,
                 zoom_range=0.0, fill_mode="nearest", cval=0.0, frame_order=1, mask_order=1):
        self.rotation_range = _range("rotation_range", rotation_range)
        self.width_shift_range = _range("width_shift_range", width_shift_range, below=1.0)
        self.height_shift_range = _range("height_shift_range", height_shift_range, below=1.0)
        self.shear_range = _range("shear_range", shear_range)
        if np.ndim(zoom_range) == 0:
            z = _range("zoom_range", zoom_range, below=1.0)
            self.zoom_range = (1.0 - z, 1.0 + z)
        else:
            if len(zoom_range) != 2:
                raise ValueError(f"zoom_range must be a float or a (low, high) pair, got {zoom_range!r}")
            lo, hi = (float(v) for v in zoom_range)
            if not (math.isfinite(lo) and math.isfinite(hi) and 0 < lo <= hi):
                raise ValueError(f"zoom_range must satisfy 0 < low <= high, got {zoom_range!r}")
            self.zoom_range = (lo, hi)
        if fill_mode not in FILL_MODES:
            raise ValueError(f"fill_mode must be one of {FILL_MODES}, got {fill_mode!r}")
        self.fill_mode = fill_mode
        self.cval = float(cval)
        if not math.isfinite(self.cval):
            raise ValueError(f"cval must be finite, got {cval!r}")
        self.frame_order = _order("frame_order", frame_order)
        self.mask_order = _order("mask_order", mask_order)

    @property
    def active(self) -> bool:
        return bool(self.rotation_range or self.width_shift_range or self.height_shift_range or self.shear_range
                    or self.zoom_range != (1.0, 1.0))

    @property
    def fill_constant(self) -> bool:
        return self.fill_mode == "constant"

    def draw(self, rng, samples: int) -> np.ndarray:
        """One epoch's parameter table, float64 (samples, 6): theta and shear in degrees, tx / ty as
        fractions of h / w, zx, zy -- from ONE rng.random((samples, 6)), indexed by sample."""
        u = rng.random((int(samples), 6))
        s = 2.0 * u - 1.0
        lo, hi = self.zoom_range
        t = np.empty_like(u)
        t[:, 0] = s[:, 0] * self.rotation_range
        t[:, 1] = s[:, 1] * self.height_shift_range
        t[:, 2] = s[:, 2] * self.width_shift_range
        t[:, 3] = s[:, 3] * self.shear_range
        t[:, 4] = lo + u[:, 4] * (hi - lo)
        t[:, 5] = lo + u[:, 5] * (hi - lo)
        return t

    @staticmethod
    def matrix(params, size) -> np.ndarray:
        """The float64 3x3 map output (r, q, 1) -> source (row, column, 1) of one parameter row."""
        theta, fy, fx, shear, zx, zy = (float(v) for v in params)
        h, w = size
        th, sh = math.radians(theta), math.radians(shear)
        rot = np.array([[math.cos(th), -math.sin(th), 0.0], [math.sin(th), math.cos(th), 0.0], [0.0, 0.0, 1.0]])
        shift = np.array([[1.0, 0.0, fy * h], [0.0, 1.0, fx * w], [0.0, 0.0, 1.0]])
        shr = np.array([[1.0, -math.sin(sh), 0.0], [0.0, math.cos(sh), 0.0], [0.0, 0.0, 1.0]])
        zoom = np.diag([zx, zy, 1.0])
        m = rot @ shift @ shr @ zoom
        oy, ox = h / 2.0 - 0.5, w / 2.0 - 0.5
        to_centre = np.array([[1.0, 0.0, oy], [0.0, 1.0, ox], [0.0, 0.0, 1.0]])
        back = np.array([[1.0, 0.0, -oy], [0.0, 1.0, -ox], [0.0, 0.0, 1.0]])
        return to_centre @ m @ back

    @staticmethod
    def record64(matrix, size, flip=False) -> np.ndarray:
        """[m00 m01 o0 m10 m11 o1] of a 3x3 map in float64, the flip (applied after the warp)
        folded in: q -> w - 1 - q."""
        m = np.asarray(matrix, np.float64)
        rec = np.array([m[0, 0], m[0, 1], m[0, 2], m[1, 0], m[1, 1], m[1, 2]])
        if flip:
            w1 = size[1] - 1
            rec[2], rec[1] = rec[2] + rec[1] * w1, -rec[1]
            rec[5], rec[4] = rec[5] + rec[4] * w1, -rec[4]
        return rec

    def records(self, table, idx, flips, size) -> np.ndarray:
        """fp32 (len(idx), 6): the transform records of a batch of samples idx, from the epoch's
        parameter table and flip flags (both indexed by sample), each number rounded once."""
        out = np.empty((len(idx), 6), np.float32)
        for k, i in enumerate(idx):
            i = int(i)
            out[k] = self.record64(self.matrix(table[i], size), size, bool(flips[i]))
        return out


def affine_u8_reference(src, slots, xforms, order=1, fill_constant=False, cval=0.0):
    """NumPy restatement of the warp kernel (unet_batch_affine_u8, csrc/batch.hip): uint8 samples
    src (n, h, w, c), b sample indices (clamped to [0, n-1]) and b fp32 records -> fp32 (b, h, w, c).
    Every operation is one fp32 rounding, in the kernel's order (include/unet_hip.h states it).  A
    NaN coordinate (a NaN in a record, or inf * 0) is not outside and clamps to 0, as the kernel's
    fmaxf / fminf have it; an infinite one is outside and clamps to the border."""
    src = np.asarray(src)
    if src.dtype != np.uint8 or src.ndim != 4:
        raise ValueError(f"src: expected uint8 (n, h, w, c), got {src.dtype} {src.shape}")
    if order not in (0, 1):
        raise ValueError(f"order must be 0 or 1, got {order!r}")
    slots = np.asarray(slots).reshape(-1)
    xforms = np.asarray(xforms, np.float32).reshape(-1, 6)
    if len(xforms) != len(slots):
        raise ValueError(f"{len(slots)} slots but {len(xforms)} records")
    n, h, w, _ = src.shape
    f32 = np.float32
    r = np.arange(h, dtype=np.int32).astype(f32)[:, None]
    q = np.arange(w, dtype=np.int32).astype(f32)[None, :]
    hm, wm, zero = f32(h - 1), f32(w - 1), f32(0)
    out = np.empty((len(slots),) + src.shape[1:], f32)
    for i, e in enumerate(slots):
        a = src[min(max(int(e), 0), n - 1)]
        m00, m01, o0, m10, m11, o1 = xforms[i]
        with np.errstate(invalid="ignore", over="ignore"):  # a non-finite record is an input like any other
            sy = (m00 * r + m01 * q) + o0
            sx = (m10 * r + m11 * q) + o1
        outside = (sy < zero) | (sy > hm) | (sx < zero) | (sx > wm)
        sy = np.fmin(np.fmax(sy, zero), hm)  # fmax / fmin return the other operand for a NaN
        sx = np.fmin(np.fmax(sx, zero), wm)
        if order == 0:
            y = np.minimum(np.floor(sy + f32(0.5)).astype(np.int32), h - 1)
            x = np.minimum(np.floor(sx + f32(0.5)).astype(np.int32), w - 1)
            v = a[y, x].astype(f32)
        else:
            y0 = np.minimum(np.floor(sy).astype(np.int32), max(h - 2, 0))
            x0 = np.minimum(np.floor(sx).astype(np.int32), max(w - 2, 0))
            y1, x1 = np.minimum(y0 + 1, h - 1), np.minimum(x0 + 1, w - 1)
            fy = (sy - y0.astype(f32))[..., None]
            fx = (sx - x0.astype(f32))[..., None]
            p00, p01 = a[y0, x0].astype(f32), a[y0, x1].astype(f32)
            p10, p11 = a[y1, x0].astype(f32), a[y1, x1].astype(f32)
            top = p00 + fx * (p01 - p00)
            bot = p10 + fx * (p11 - p10)
            v = top + fy * (bot - top)
        if fill_constant:
            v = np.where(outside[..., None], f32(cval), v)
        out[i] = v / f32(255.0)
    return out
