"""NumPy restatement of the frozen int8 arithmetic contract (include/unet_hip.h, "Frozen int8
inference"), written from the contract's text and not from the kernels:

  * integer GEMMs in int64 (exact);
  * fmaf(a, b, c) as float32(float64(a) * float64(b) + float64(c)) -- two roundings where the device
    has one, so a value could land on a tie the device resolves the other way: the GPU tests use
    fixed seeds and would show the element if that ever happened;
  * rintf as np.rint on float32; int32 -> fp32 as astype(np.float32) (nearest even).

One-layer functions (sepconv, maxpool, conv_transpose, image_block, head) on quantised bytes, and
`forward`, which returns every activation of the network; the image block and the head are taken
in float64.  Test helper, not a test module.
"""
from __future__ import annotations

import numpy as np

from oracle import keras_ops as K

F32, F64 = np.float32, np.float64


def fmaf(a, b, c):
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


def quant(v, lo, hi, dtype):
    """clamp(rintf(v), lo, hi) of float32 values."""
    v = np.asarray(v)
    assert v.dtype == F32
    return np.clip(np.rint(v), F32(lo), F32(hi)).astype(dtype)


def depthwise_q(x_q, taps):
    """y_q int8 = clamp(rint(sum_t x_q[t] taps[t]), -127, 127), taps fp32 (9, C), t row-major over
    (dy, dx); padding q = 0; the sum is the fmaf chain t = 0..8 from a = 0."""
    n, h, w, c = x_q.shape
    taps = np.asarray(taps, F32).reshape(9, c)
    xp = np.pad(x_q.astype(F32), ((0, 0), (1, 1), (1, 1), (0, 0)))
    a = np.zeros((n, h, w, c), F32)
    for t in range(9):
        a = fmaf(xp[:, t // 3:t // 3 + h, t % 3:t % 3 + w, :], taps[t], a)
    return quant(a, -127, 127, np.int8)


def gemm_i64(a_q, b_q):
    """a_q (..., k) x b_q (cols, k) -> (..., cols) in int64; must fit int32 (the accumulator)."""
    acc = a_q.astype(np.int64) @ b_q.astype(np.int64).T
    assert np.abs(acc).max(initial=0) < 2 ** 31
    return acc


def sepconv(x_q, taps, pw_q, mult, bias_q):
    """A quantised conv block: x_q uint8 / int8 bytes (a concat is np.concatenate of its halves,
    their scales are inside taps), pw_q int8 (cout, C); returns uint8 (n, h, w, cout)."""
    acc = gemm_i64(depthwise_q(x_q, taps), pw_q)
    v = fmaf(acc.astype(np.int32).astype(F32), np.asarray(mult, F32), np.asarray(bias_q, F32))
    return quant(v, 0, 255, np.uint8)


def maxpool(q):
    n, h, w, c = q.shape
    return q.reshape(n, h // 2, 2, w // 2, 2, c).max(axis=(2, 4))


def conv_transpose(x_q, kernel_q, colsum, mult, bias_q):
    """Conv2DTranspose 2x2: x_q uint8 (n, h, w, cin), kernel_q int8 (2, 2, cout, cin), colsum int32
    and mult fp32 per column (a, b, co), bias_q fp32 (cout); returns int8 (n, 2h, 2w, cout)."""
    assert x_q.dtype == np.uint8
    n, h, w, cin = x_q.shape
    cout = kernel_q.shape[2]
    a = (x_q ^ np.uint8(0x80)).view(np.int8)  # q - 128
    acc = gemm_i64(a, kernel_q.reshape(4 * cout, cin))
    acc32 = acc + 128 * np.asarray(colsum, np.int64).reshape(-1)
    assert np.abs(acc32).max(initial=0) < 2 ** 31
    v = fmaf(acc32.astype(np.int32).astype(F32), np.asarray(mult, F32).reshape(-1), np.tile(np.asarray(bias_q, F32), 4))
    q = quant(v, -127, 127, np.int8).reshape(n, h, w, 2, 2, cout)
    return np.ascontiguousarray(q.transpose(0, 1, 3, 2, 4, 5)).reshape(n, 2 * h, 2 * w, cout)


def image_block(x, dw, pw, bias, s_out):
    """enc1_block1 in float64 on the fp32 operands: q = clamp(rint(relu(z) / s_out), 0, 255), and
    the real-valued relu(z) / s_out it rounds."""
    cin = x.shape[-1]
    z = K.pointwise(K.depthwise3x3(np.asarray(x, F64), np.asarray(dw, F64).reshape(3, 3, cin, 1)),
                    np.asarray(pw, F64).reshape(1, 1, cin, -1)) + np.asarray(bias, F64)
    r = K.relu(z) / F64(F32(s_out))
    return np.clip(np.rint(r), 0, 255).astype(np.uint8), r


def head(x_q, kernel, bias, num_classes):
    """fp32 head operands (the input scale folded into kernel (cin, classes)) in float64."""
    cin = x_q.shape[-1]
    return K.head(x_q.astype(F64), np.asarray(kernel, F64).reshape(1, 1, cin, num_classes), np.asarray(bias, F64),
                  num_classes)


def block_operands(q, b):
    return q[f"{b}/taps"], q[f"{b}/pw_q"], q[f"{b}/mult"], q[f"{b}/bias_q"]


def upsample_operands(q, s):
    return q[f"{s}/kernel_q"], q[f"{s}/colsum"], q[f"{s}/mult"], q[f"{s}/bias_q"]


def forward(q, x, num_classes, filters):
    """q: frozen.quantize_weights(...).  Returns {name: bytes} for every activation, and 'prob'."""
    acts = {}
    n = len(filters)
    skips = []
    a = None
    for i in range(n):
        s = f"enc{i + 1}"
        if i == 0:
            a, _ = image_block(x, q[f"{s}_block1/dw"], q[f"{s}_block1/pw"], q[f"{s}_block1/bias"],
                               q[f"scale/{s}_block1"])
        else:
            a = sepconv(a, *block_operands(q, f"{s}_block1"))
        acts[f"{s}_block1"] = a
        a = acts[f"{s}_block2"] = sepconv(a, *block_operands(q, f"{s}_block2"))
        skips.append(a)
        a = acts[f"{s}_pool"] = maxpool(a)
    a = acts["bneck_block1"] = sepconv(a, *block_operands(q, "bneck_block1"))
    a = acts["bneck_block2"] = sepconv(a, *block_operands(q, "bneck_block2"))
    for i in range(n, 0, -1):
        s = f"dec{i}"
        u = acts[f"{s}_upsample"] = conv_transpose(a, *upsample_operands(q, f"{s}_upsample"))
        # int8 | uint8 halves side by side as integers (the taps carry each half's scale)
        cat = np.concatenate([u.astype(np.int16), skips[i - 1].astype(np.int16)], axis=-1)
        a = acts[f"{s}_block1"] = sepconv(cat, *block_operands(q, f"{s}_block1"))
        a = acts[f"{s}_block2"] = sepconv(a, *block_operands(q, f"{s}_block2"))
    acts["prob"] = head(a, q["head/kernel"], q["head/bias"], num_classes)
    return acts


def dequantize(acts, q):
    """The real values s q of forward's activations (prob as it is)."""
    return {k: (v if k == "prob" else v.astype(F64) * float(q[f"scale/{k}"])) for k, v in acts.items()}


def oracle_ranges(exact, ref, filters):
    """Calibration ranges (max |.| of every frozen.calibration_names tensor) from the float64 oracle
    activations `ref` and the exactly folded weights."""
    from unet_amd import frozen
    r = {k: float(np.abs(ref[k]).max()) for k in frozen.activation_names(filters)}
    for b, srcs in frozen.block_inputs(filters).items():
        a = np.concatenate([ref[s] for s in srcs], axis=-1)
        r[f"{b}/y"] = float(np.abs(K.depthwise3x3(a, np.asarray(exact[f"{b}_sepconv/depthwise_kernel"], F64))).max())
    return r
