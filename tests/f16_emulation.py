"""NumPy float64 emulation of the frozen fp16 forward (unet_amd/frozen.py, csrc/frozen.hip), built
from oracle.keras_ops with rounding to nearest-even fp16 at exactly the four points the kernels
round at:

  1. the folded pointwise and upsample kernels (done by fold_weights, on the host);
  2. each block's depthwise output, before the pointwise product (not the image block's);
  3. each block's output, after bias and ReLU;
  4. each upsample output, after bias.

Everything else (the image, the image block up to its output, sums, biases, the head) is left in
float64 where the device uses fp32.  `forward` returns every layer's activation.  Test helper, not
a test module.
"""
from __future__ import annotations

import numpy as np

from oracle import keras_ops as K
from oracle.unet_ref import UNetOracle


def r16(a, on=True):
    return np.asarray(a, np.float64).astype(np.float16).astype(np.float64) if on else np.asarray(a, np.float64)


def U16(seed, shape, lo=0.0, hi=1.0):
    """Portable uniform draw, rounded to fp16 and returned as float64."""
    from unet_amd.params import portable_uniform
    n = int(np.prod(shape))
    return r16((lo + (hi - lo) * portable_uniform(seed, n)).reshape(shape))


def U32(seed, shape, lo=0.0, hi=1.0):
    """Portable uniform draw, rounded to fp32 and returned as float64 (make_golden.U)."""
    from unet_amd.params import portable_uniform
    n = int(np.prod(shape))
    return (lo + (hi - lo) * portable_uniform(seed, n)).reshape(shape).astype(np.float32).astype(np.float64)


def forward(folded, x, num_classes, filters, rounding=True):
    """folded: fold_weights(...) (rounding on) or fold_exact(...) (rounding off).  Returns
    {layer name: activation} for the 18 blocks, dec*_upsample, enc*_pool, and 'prob'."""
    fw = {k: np.asarray(v, np.float64) for k, v in folded.items()}
    acts = {}

    def block(name, a, image=False):
        y = K.depthwise3x3(a, fw[f"{name}_sepconv/depthwise_kernel"])
        if not image:
            y = r16(y, rounding)
        z = K.pointwise(y, fw[f"{name}_sepconv/pointwise_kernel"]) + fw[f"{name}_sepconv/bias"]
        acts[name] = r16(K.relu(z), rounding)
        return acts[name]

    a = np.asarray(x, np.float64)
    skips = []
    n = len(filters)
    for i in range(n):
        a = block(f"enc{i + 1}_block1", a, image=(i == 0))
        a = block(f"enc{i + 1}_block2", a)
        skips.append(a)
        a = acts[f"enc{i + 1}_pool"] = K.maxpool2(a)
    a = block("bneck_block1", a)
    a = block("bneck_block2", a)
    for i in range(n):
        s = f"dec{n - i}"
        u = K.conv_transpose2x2(a, fw[f"{s}_upsample/kernel"], fw[f"{s}_upsample/bias"])
        u = acts[f"{s}_upsample"] = r16(u, rounding)
        a = block(f"{s}_block1", np.concatenate([u, skips[n - 1 - i]], axis=-1))
        a = block(f"{s}_block2", a)
    acts["prob"] = K.head(a, fw["output_mask/kernel"], fw["output_mask/bias"], num_classes)
    return acts


def oracle_activations(weights, x, num_classes, filters, use_batch_norm=True):
    """The same layers from the float64 oracle's inference forward (UNetOracle.forward,
    training=False) on the UNFOLDED weights."""
    orc = UNetOracle(num_classes, 0.0, use_batch_norm, filters)
    p = {k: np.asarray(v, np.float64) for k, v in weights.items()}
    prob, cache, _ = orc.forward(p, np.asarray(x, np.float64), training=False)
    acts = {"prob": prob}
    n = len(filters)
    blocks = [f"enc{i + 1}_block{j}" for i in range(n) for j in (1, 2)] + ["bneck_block1", "bneck_block2"] \
        + [f"dec{n - i}_block{j}" for i in range(n) for j in (1, 2)]
    for b in blocks:
        z = cache[b]["z"]
        if use_batch_norm:
            pre = K.bn_infer(z, p[f"{b}_bn/gamma"], p[f"{b}_bn/beta"], p[f"{b}_bn/moving_mean"],
                             p[f"{b}_bn/moving_variance"])
        else:
            pre = z + p[f"{b}_sepconv/bias"]
        acts[b] = K.relu(pre)
    for i in range(n):
        acts[f"enc{i + 1}_pool"] = K.maxpool2(acts[f"enc{i + 1}_block2"])
        f = filters[i]
        acts[f"dec{i + 1}_upsample"] = cache[f"dec{i + 1}_block1"]["a_in"][..., :f]
    return acts


def layer_errors(acts, ref):
    """{name: (max |acts - ref|, max |ref|)} over the reference's layers."""
    return {k: (float(np.abs(acts[k] - ref[k]).max()), float(np.abs(ref[k]).max())) for k in ref}
