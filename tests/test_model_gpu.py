"""Whole-model parity of the MI355X engine against the NumPy oracle (float64), through the
reference's builder API (model/u_net.py U_NET) and the train step of scripts/train.py.

Tolerances (north star: masks within 1e-3 on identical weights/inputs):
  * inference probabilities: max |p - p_ref| < 1e-3 (measured ~1e-6);
  * one train step: loss within 1e-5; every gradient tensor within relative L2 norm
    max(1e-3, 2 x e32) of the float64 oracle, where e32 is how far the SAME oracle run in
    float32 lands from float64 for that tensor (the network's own fp32 conditioning: BN over
    few samples at small test sizes amplifies rounding to ~1e-3..1e-2 in some gradients);
    post-AdamW weights within 1e-4 relative.
"""
import json
import os

import numpy as np
import pytest

from helpers import f32, train_step_parity
from helpers import weights_with_stats as _weights_with_stats
from oracle.unet_ref import UNetOracle

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _data(rng, n, h, w, ncls):
    x = rng.random((n, h, w, 3), dtype=np.float32)
    if ncls == 1:
        y = np.zeros((n, h, w, 1), np.float32)
        for i in range(n):  # ID-card-like axis-aligned quads (~30% foreground)
            y0, x0 = rng.integers(0, h // 3), rng.integers(0, w // 3)
            y[i, y0:y0 + h // 2, x0:x0 + w // 2] = 1.0
    else:
        y = np.eye(ncls, dtype=np.float32)[rng.integers(0, ncls, (n, h, w))]
    return x, y


def test_builder_api_and_inference_parity_cfg1():
    """configs[0]: U_NET((128,128,3), 1) forward on 2 images."""
    from model.u_net import U_NET, unet
    with pytest.raises(ValueError):
        U_NET((128, 128))
    model = unet(input_size=(128, 128, 3), num_classes=1)
    assert model.count_params() == 6000028
    rng = np.random.default_rng(2301)
    p = _weights_with_stats(model, rng)
    x, _ = _data(rng, 2, 128, 128, 1)
    prob = model.predict(x)
    ref, _, _ = UNetOracle(1).forward(p, x.astype(np.float64), training=False)
    assert prob.shape == (2, 128, 128, 1)
    assert np.abs(prob - ref).max() < 1e-3
    assert np.abs(prob - ref).max() < 2e-5  # in practice fp32 rounding only
    # binary masks at the reference's threshold (scripts/inference.py:160) agree pixelwise
    # except where |p - 0.5| is below the numeric noise
    far = np.abs(ref - 0.5) > 1e-4
    assert np.array_equal((prob > 0.5)[far], (ref > 0.5)[far])
    # the fused depthwise+pointwise kernel (used here at the 128x128 level) against the split path
    model.engine.fuse_sepconv = "never"
    prob_split = model.predict(x)
    model.engine.fuse_sepconv = "always"
    prob_fused = model.predict(x)
    assert np.abs(prob_split - ref).max() < 2e-5 and np.abs(prob_fused - ref).max() < 2e-5


@pytest.mark.parametrize("ncls,use_bn,drop,loss,fuse", [(1, True, 0.0, "dice_loss", "never"),
                                                        (1, True, 0.2, "dice_loss", "never"),
                                                        (21, True, 0.0, "dice_loss", "auto"),
                                                        (1, False, 0.0, "dice_loss", "auto"),
                                                        (1, True, 0.0, "iou_loss", "auto"),
                                                        (1, True, 0.0, "dice_loss", "always"),
                                                        (1, True, 0.2, "dice_loss", "always"),
                                                        (1, True, 0.2, "dice_loss", "always+r128")])
def test_train_step_parity(ncls, use_bn, drop, loss, fuse, record_property):
    """One train step against the oracle; fuse="always" runs the fused depthwise+pointwise
    forward on every level it supports (32x32 and 16x16 here), "never" the split kernels;
    "+r128": the 128-output blocks keep no y either (their weight gradients recompute it, through
    dec2_block1's dropout view)."""
    from unet_amd.model import UNetModel
    n, hw = 2, 32
    model = UNetModel((hw, hw, 3), ncls, dropout_rate=drop, use_batch_norm=use_bn, seed=11)
    if fuse.endswith("+r128"):
        fuse = fuse[:-5]
        model.engine.recompute_y_couts = (64, 128)
    model.engine.fuse_sepconv = fuse
    model.engine.fuse_bn_bwd = fuse != "never"  # "never": also the separate BN-backward dz pass
    orc = UNetOracle(ncls, drop, use_bn)

    def draw(attempt):
        rng = np.random.default_rng(ncls * 13 + int(drop * 10) + use_bn + 1000 * attempt)
        p = _weights_with_stats(model, rng)
        return (p,) + _data(rng, n, hw, hw, ncls)

    out = train_step_parity(model, orc, draw, loss)
    # how many input draws it took to find one whose discrete decisions all agree with fp64
    record_property("input_draws", out["input_draws"])
    print(f"train_step_parity[{ncls},{use_bn},{drop},{loss},{fuse}]: input draws = {out['input_draws']}")
    log = os.environ.get("UNET_PARITY_LOG")
    if log:
        with open(log, "a") as f:
            f.write(json.dumps({"test": f"train_step_parity[{ncls},{use_bn},{drop},{loss},{fuse}]",
                                "input_draws": out["input_draws"]}) + "\n")


def test_determinism_bitwise():
    """Fixed-order reductions: two identical train steps give identical bits."""
    from unet_amd.model import UNetModel
    rng = np.random.default_rng(3)
    x, y = _data(rng, 4, 64, 64, 1)
    outs = []
    for _ in range(2):
        m = UNetModel((64, 64, 3), 1, seed=5)
        m.compile(None, "dice_loss")
        m.train_step(x, y)
        m.train_step(x, y)
        torch.cuda.synchronize()
        outs.append((m.engine.params.cpu().clone(), m.engine.stats.cpu().clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_inplace_weight_edit_reaches_split_planes():
    """the split-precision (bf16 x 3) pointwise planes the fused forward reads are
    re-split on every forward, so an in-place write to engine.vars (a custom optimizer loop, a
    broadcast) changes predict() exactly as set_weights_dict of the same values does."""
    from unet_amd.model import UNetModel
    rng = np.random.default_rng(21)
    x, _ = _data(rng, 2, 64, 64, 1)
    m = UNetModel((64, 64, 3), 1, dropout_rate=0.0, seed=3)
    xd = torch.from_numpy(x).cuda()
    p0 = m.engine.predict(xd)
    name = "enc1_block2_sepconv/pointwise_kernel"  # a fused split-precision block (64 x 64 level)
    assert "enc1_block2" in m.engine.x3_off
    w = m.engine.vars[name]
    new = (w * -1.5 + 0.01).contiguous()
    w.copy_(new)  # in place: no set_weights_dict, no version bump
    p1 = m.engine.predict(xd)
    ref = UNetModel((64, 64, 3), 1, dropout_rate=0.0, seed=3)
    ref.engine.set_weights_dict({name: new.cpu().numpy()})
    p2 = ref.engine.predict(xd)
    torch.cuda.synchronize()
    assert not torch.equal(p0, p1)
    assert torch.equal(p1, p2)


def test_large_batch_fuses_the_32x32_level():
    """engine.block_fwd_choice fuses a level below 64 x 64 once the batch gives it >= 128 pixel
    tiles (FUSE_MIN_TOTAL_PIXELS: the 32 x 32 level from batch 16): on a 128 x 128
    input the 32 x 32 blocks (enc3 / dec3) then run the fused bf16x6 forward with their split
    planes (refreshed for that batch only), at batch 2 the split launches.  Against the all-split
    route (fuse="never": fp32 GEMMs): the training loss to 1e-5 and the batch-32 prediction to
    1e-5 relative L2.  (Gradients of this random-init net move by ~3e-3 between ANY two fp32
    summation orders -- ReLU decisions flip -- as fp32 vs the float64 oracle does in the
    train-geometry parity log; their parity is the op tests' and test_parity_sizes_gpu's.)"""
    from unet_amd.model import UNetModel
    rng = np.random.default_rng(23)
    x, y = _data(rng, 32, 128, 128, 1)
    xd = torch.from_numpy(x).cuda()
    res = {}
    for fuse in ("auto", "never"):
        m = UNetModel((128, 128, 3), 1, dropout_rate=0.0, seed=9)
        m.compile(None, "dice_loss")
        m.engine.fuse_sepconv = fuse
        p = m.engine.predict(xd).clone()
        live = set(m.engine.x3_live)
        loss = m.train_step(x, y)
        torch.cuda.synchronize()
        res[fuse] = (float(loss[0]), p)
        if fuse == "auto":
            assert {"enc3_block1", "enc3_block2", "dec3_block2"} <= live  # the 32 x 32 level at batch 32
            assert "enc4_block1" not in live  # 16 x 16 at batch 32: 8192 pixels, split launches
            m.engine.predict(xd[:2])
            assert "enc3_block2" not in m.engine.x3_live and "enc2_block2" in m.engine.x3_live
    (la, pa), (ln, pn) = res["auto"], res["never"]
    assert abs(la - ln) <= 1e-5 * max(1.0, abs(ln))
    assert float((pa - pn).double().norm() / pn.double().norm()) < 1e-5


def test_stream_schedules_bitwise_equal():
    """The schedule only orders launches: single-stream, two-stream with the weight gradients issued
    beside their data gradient, and two-stream with the fused 256x256-level weight gradient deferred
    past the next statistics launch give the same bits after two steps (with the MeanIoU update on
    the side stream).  128 x 128 input, batch 2: enc1's blocks take the fused y-recompute route."""
    from unet_amd.model import UNetModel
    from unet_amd.metrics import MeanIoU
    rng = np.random.default_rng(11)
    x, y = _data(rng, 2, 128, 128, 1)
    outs = []
    for overlap, defer in ((False, False), (True, False), (True, True)):
        m = UNetModel((128, 128, 3), 1, seed=7)
        m.engine.overlap, m.engine.defer_sw = overlap, defer
        miou = MeanIoU(2, threshold=0.5)
        m.compile(None, "dice_loss", [miou])
        m.train_step(x, y)
        m.train_step(x, y)
        torch.cuda.synchronize()
        outs.append((m.engine.params.cpu().clone(), m.engine.stats.cpu().clone(), miou.confusion_matrix()))
    for o in outs[1:]:
        assert torch.equal(outs[0][0], o[0]) and torch.equal(outs[0][1], o[1])
        assert (outs[0][2] == o[2]).all()


def test_full_size_train_steps_cfg2():
    """configs[1] shape (256x256x3, batch 16): loss decreases on a fixed batch, no NaNs, and
    size-independent properties hold (probabilities in [0,1], dice = 1 - loss)."""
    from unet_amd.model import UNetModel
    from unet_amd.metrics import MeanIoU
    rng = np.random.default_rng(0)
    x, y = _data(rng, 16, 256, 256, 1)
    m = UNetModel((256, 256, 3), 1)
    miou = MeanIoU(2)
    from unet_amd.optim import AdamW
    m.compile(AdamW(2e-3, 1e-4), "dice_loss", [miou, "dice_coef"])
    losses = []
    for _ in range(6):
        r = m.train_step(x, y).cpu().numpy()
        assert np.isfinite(r).all()
        assert abs(r[0] + r[1] - 1) < 1e-6
        losses.append(r[0])
    assert losses[-1] < losses[0]
    p = m.predict(x[:2])
    assert p.min() >= 0 and p.max() <= 1
    assert miou.confusion_matrix().sum() == 6 * 16 * 256 * 256


@pytest.mark.parametrize("size,batch,ncls", [(512, 8, 1),    # configs[3]: 512x512 binary, batch 8 per GPU
                                             (256, 8, 21)])  # configs[4]: 21 classes, batch 32 over 4 GPUs
def test_full_size_train_steps_other_configs(size, batch, ncls):
    """The per-GPU shapes of BASELINE configs[3] and configs[4]: finite steps whose loss falls on a
    fixed batch, dice = 1 - loss, probabilities a distribution, confusion counts cover every pixel."""
    from unet_amd.model import UNetModel
    from unet_amd.metrics import MeanIoU
    from unet_amd.optim import AdamW
    rng = np.random.default_rng(size + ncls)
    x, y = _data(rng, batch, size, size, ncls)
    m = UNetModel((size, size, 3), ncls)
    miou = MeanIoU(2)
    m.compile(AdamW(2e-3, 1e-4), "dice_loss", [miou, "dice_coef"] if ncls == 1 else ["dice_coef"])
    losses = []
    for _ in range(4):
        r = m.train_step(x, y).cpu().numpy()
        assert np.isfinite(r).all()
        assert abs(r[0] + r[1] - 1) < 1e-6
        losses.append(r[0])
    assert losses[-1] < losses[0]
    p = m.predict(x[:1])
    assert p.shape == (1, size, size, ncls) and p.min() >= 0 and p.max() <= 1
    if ncls > 1:
        assert np.abs(p.sum(-1) - 1).max() < 1e-5
    if ncls == 1:
        assert miou.confusion_matrix().sum() == 4 * batch * size * size
    del m
    torch.cuda.empty_cache()


def test_meaniou_metric_api():
    from unet_amd.metrics import MeanIoU
    from oracle import keras_ops as K
    rng = np.random.default_rng(1)
    yt = (rng.random((2, 16, 16, 1)) > 0.5).astype(np.float32)
    yp = rng.random((2, 16, 16, 1)).astype(np.float32)
    m = MeanIoU(2, threshold=0.5)
    m.update_state(yt, yp)
    cm = K.meaniou_confusion(yt, yp, 2, 0.5)
    assert abs(m.result() - K.meaniou_result(cm)) < 1e-12
    m2 = MeanIoU(2)  # training semantics: truncation of raw probabilities
    m2.update_state(yt, yp)
    assert abs(m2.result() - K.meaniou_result(K.meaniou_confusion(yt, yp, 2))) < 1e-12


def test_reference_loss_api():
    from utils.loss import dice_loss, iou_loss, jaccard_loss
    from utils.metrics import dice_coef, iou_coef
    from oracle import keras_ops as K
    rng = np.random.default_rng(2)
    yt = (rng.random((3, 8, 8, 2)) > 0.5).astype(np.float32)
    yp = rng.random((3, 8, 8, 2)).astype(np.float32)
    assert abs(float(dice_coef(yt, yp)) - K.dice_coef(f32(yt), f32(yp))) < 1e-6
    assert abs(float(iou_coef(yt, yp)) - K.iou_coef(f32(yt), f32(yp))) < 1e-6
    assert abs(float(dice_loss(yt, yp)) - K.dice_loss(f32(yt), f32(yp))) < 1e-6
    assert abs(float(iou_loss(yt, yp)) - K.iou_loss(f32(yt), f32(yp))) < 1e-6
    assert jaccard_loss is iou_loss
