"""The whole network on the data it exists for: decoded uint8 images with flat regions, exact 0 and 1.0
(helpers.poster_batch), and blob masks with an empty and a full one (helpers.blob_masks) -- every other
model-level GPU test feeds noise.  What such inputs contain, and the seed bases, are pinned without a device
in tests/test_structured_data_host.py; the ops' behaviour on them in tests/test_degenerate_ops_gpu.py.

  * train step: not4 (the scalar routes) and one_level (the fused MFMA route, the pool-selection epilogue,
    the tiled backward) with the dice and the IoU loss, and deep5 without BatchNorm and with zero biases
    (pre-activations exactly 0 on black pixels), through helpers.train_step_parity: loss and dice 1e-5,
    every gradient max(1e-3, 2 x the float32 oracle's own error), at most ten input draws.  Flat images are
    worse conditioned than noise -- the float32 NumPy oracle's own post-AdamW weights are up to 8.6e-5
    from float64's -- so the weight / statistics gate is max(1e-4, 2 x the float32 oracle's own error on
    that tensor), the rule the gradients already follow (oracle32_weight_gate).
  * inference and test_step with moving statistics: two64_nodrop and the default filters at (64, 64, 3),
    binary and 3-class.  Probabilities within max(2e-5, 2 x the float32 oracle's own max error) of float64;
    test_step's loss / dice / IoU within 1e-5; the MeanIoU confusion exactly that of the device's own
    probabilities, classes that never occur excluded from the mean as Keras does; on two64_nodrop predict
    through a captured graph bitwise equal to eager.

Every case's worst error / gate ratios and draw count are recorded as properties and, with UNET_PARITY_LOG
set, appended to that file (profiles/flat_data_parity.jsonl is such a run on an MI355X)."""
import json
import os

import numpy as np
import pytest

from helpers import (FLAT_BATCH, GEOMETRY_ENGINE_SEED, blob_masks, flat_draw, geometry_cfg, host, oracle_values,
                     poster_batch, randomised_stats, train_step_parity, trace_model)
from oracle import keras_ops as K
from oracle.unet_ref import FILTERS, UNetOracle

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PROB_FLOOR, VALUE_TOL = 2e-5, 1e-5


def _record(row, record_property):
    for k, v in row.items():
        if k != "test":
            record_property(k, v)
    print(json.dumps(row))
    log = os.environ.get("UNET_PARITY_LOG")
    if log:
        with open(log, "a") as f:
            f.write(json.dumps(row) + "\n")


@pytest.mark.parametrize("name,loss", [("not4", "dice_loss"), ("not4", "iou_loss"), ("one_level", "dice_loss"),
                                       ("one_level", "iou_loss"), ("deep5", "dice_loss")])
def test_flat_train_step_against_the_oracle(name, loss, record_property):
    cfg, filters, _ = geometry_cfg(name)
    size, ncls, use_bn, drop, _ = cfg
    model = trace_model(cfg, seed=GEOMETRY_ENGINE_SEED, filters=filters)
    eng = model.engine
    orc = UNetOracle(ncls, drop, use_bn, filters)
    seen = {}

    def draw(attempt):
        w32, x, y = flat_draw(name, attempt)
        eng.set_weights_dict(w32)
        seen.update(x=x, y=y)
        return {k: v.astype(np.float64) for k, v in w32.items()}, x, y

    row = {"test": f"flat_train_step[{name},{loss}]"}
    row.update(train_step_parity(model, orc, draw, loss=loss, oracle32_weight_gate=True))
    x, y = seen["x"], seen["y"]
    assert x.shape[0] == FLAT_BATCH.get(name, x.shape[0]) and not y[0].any() and y[1].any()
    assert (x == 0).any() and (x == 1).any()
    if not use_bn:  # the device's own pre-activation is exactly 0 wherever the neighbourhood is black
        bb = eng._acts_last.blocks["enc1_block1"]
        pre = bb.z.cpu().double() * bb.scale.cpu().double() + bb.shift.cpu().double()
        black = K.depthwise3x3((x != 0).any(-1, keepdims=True).astype(np.float64), np.ones((3, 3, 1, 1))) == 0
        zero = pre.numpy().reshape(x.shape[:3] + (-1,))[black[..., 0]]
        row["exact_zero_preactivations"] = int(zero.size)
        assert zero.size > 0 and not zero.any()
    _record(row, record_property)


def _inference_case(name):
    """(cfg, filters) of an inference network: a GEOMETRIES name, or default filters at (64, 64, 3)."""
    if name == "two64_nodrop":
        cfg, filters, _ = geometry_cfg(name)
        return cfg, filters
    return ((64, 64, 3), {"default_binary": 1, "default_3class": 3}[name], True, 0.2, {}), None


@pytest.mark.parametrize("name", ["two64_nodrop", "default_binary", "default_3class"])
def test_flat_inference_and_test_step(name, record_property):
    from unet_amd.metrics import MeanIoU
    from unet_amd.params import init_weights, unet_variables
    cfg, filters = _inference_case(name)
    size, ncls, use_bn, drop, _ = cfg
    n = 3
    thr = 0.5 if ncls == 1 else None
    metric = MeanIoU(max(ncls, 2), threshold=thr)
    model = trace_model(cfg, metrics=[metric], seed=GEOMETRY_ENGINE_SEED, filters=filters)
    eng = model.engine
    rng = np.random.default_rng(9100 + ncls + len(filters or FILTERS))
    w32 = randomised_stats(init_weights(unet_variables(size[2], ncls, use_bn, filters or FILTERS), GEOMETRY_ENGINE_SEED),
                           rng)
    eng.set_weights_dict(w32)
    x, y = poster_batch(rng, n, cfg), blob_masks(n, size, ncls)
    tx, ty = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    orc = UNetOracle(ncls, drop, use_bn, filters or FILTERS)
    ref = orc.forward({k: v.astype(np.float64) for k, v in w32.items()}, x.astype(np.float64), training=False)[0]
    p32 = orc.forward(w32, x, training=False)[0]
    assert p32.dtype == np.float32

    prob = host(eng.predict(tx))
    e, e32 = float(np.abs(prob - ref).max()), float(np.abs(p32.astype(np.float64) - ref).max())
    gate = max(PROB_FLOOR, 2.0 * e32)
    row = {"test": f"flat_inference[{name}]", "predict_err": e, "predict_err_oracle32": e32, "predict": e / gate}

    metric.reset_state()
    res = model.test_step(tx, ty).cpu().numpy().astype(np.float64)
    prob_dev = host(eng.acts(n).prob)
    want = oracle_values(y, ref)
    errs = np.abs(res - want)
    row.update(test_step_loss=errs[0] / VALUE_TOL, test_step_dice=errs[1] / VALUE_TOL, test_step_iou=errs[2] / VALUE_TOL,
               test_step_prob_err=float(np.abs(prob_dev - ref).max()))
    cm = K.meaniou_confusion(y, prob_dev, metric.num_classes, thr)
    absent = (cm.sum(0) + cm.sum(1)) == 0
    row["absent_classes"] = int(absent.sum())

    if name == "two64_nodrop":
        eager = eng.predict(tx)
        eng.graph_predict = True
        first, replay = eng.predict(tx), eng.predict(tx)  # the capture's call, then a replay of it
        eng.graph_predict = False
        torch.cuda.synchronize()
        row["graph_bitwise"] = bool(torch.equal(first, eager) and torch.equal(replay, eager))
    _record(row, record_property)

    assert np.isfinite(prob).all() and e <= gate, (e, gate, e32)
    assert np.abs(prob_dev - ref).max() <= gate
    assert (errs < VALUE_TOL).all(), (res, want)
    assert np.array_equal(metric.confusion_matrix(), cm)
    assert metric.result() == K.meaniou_result(cm)
    if ncls == 3:  # labels and truncated probabilities are 0 or 1: class 2 never occurs and leaves the mean
        assert absent[2] and not absent[0]
    assert row.get("graph_bitwise", True), f"{name}: predict through the captured graph differs from eager"
