"""What the flat-image GPU tests (test_flat_data_gpu.py, test_degenerate_ops_gpu.py) rely on, pinned
without a device, so that nobody can quietly swap their inputs for easier ones.

helpers.poster_batch / blob_masks build images as a decoder leaves them (flat cells, exact 0 and 1.0) and
masks as a labelled set has them (empty, one rectangle, full).  On such inputs:

  * exact ties at a POSITIVE value are common in the 2x2 pool windows of enc1, and in a good share of the
    windows the first element is not among the maxima, so first-maximum and last-maximum routing differ
    (measured: 45 % / 14 % of the windows for not4, 46 % / 16 % for one_level; gates 25 % and 5 %);
  * that tie-break is UNOBSERVABLE at model level: routing every window's gradient to its last maximum
    instead changes no weight gradient by more than 1e-12 relative (measured: 7e-15).  Tied positions of a
    flat region have identical neighbourhoods, so their contributions are interchangeable.  Only the
    op-level tests that compare dx itself (test_degenerate_ops_gpu.py) can hold the contract;
  * FLAT_SEEDS follows GEOMETRY_SEEDS' rule: the first base of 9000, 9001, ... at which the float32
    oracle's ReLU / max-pool decisions of draw 0 equal float64's.

Recorded, not asserted (16 bases 9000..9015, draw 0): not4 agrees on 14, one_level on 10; two64, gray3264
and mult8 agree on 0 of 16 and thin on 2 (9004, 9008).  Flat images are worse conditioned than noise
(BatchNorm over a low-variance channel amplifies rounding), and at 32 x 64 with 24+ channels some decision
always sits within float32 rounding of its boundary: those geometries cannot carry a flat-image train-step
case."""
import numpy as np
import pytest

from helpers import (FLAT_SEEDS, GEOMETRY_ENGINE_SEED, POSTER_COLOURS, blob_masks, flat_draw, geometry_cfg,
                     geometry_oracle32_agrees, norm_err, poster_batch, rel_err)
from oracle import keras_ops as K
from oracle.unet_ref import UNetOracle

FLAT_CASES = ("not4", "one_level")


def test_poster_batch_is_flat_uint8():
    cfg = ((16, 32, 3), 1, True, 0.0, {})
    x = poster_batch(np.random.default_rng(1), 4, cfg)
    assert x.dtype == np.float32 and x.shape == (4, 16, 32, 3)
    assert np.array_equal(x, np.round(x * 255).astype(np.float32) / np.float32(255))  # decoded uint8
    assert (x == 0).any() and (x == 1).any()
    cells = x.reshape(4, 2, 8, 4, 8, 3)
    assert np.array_equal(cells, np.broadcast_to(cells[:, :, :1, :, :1], cells.shape))  # flat 8x8 cells
    for img in x:
        assert len(np.unique(img.reshape(-1, 3), axis=0)) <= POSTER_COLOURS
    assert np.array_equal(x, poster_batch(np.random.default_rng(1), 4, cfg))


@pytest.mark.parametrize("ncls", [1, 5])
def test_blob_masks(ncls):
    y = blob_masks(3, (16, 32), ncls)
    assert y.dtype == np.float32 and y.shape == (3, 16, 32, ncls)
    lab = y[..., 0] if ncls == 1 else y.argmax(-1)
    if ncls > 1:
        assert np.array_equal(y.sum(-1), np.ones((3, 16, 32)))
    assert not lab[0].any()
    assert lab[1].sum() == 8 * 16 and lab[1, 4:12, 8:24].all() and set(np.unique(lab[1])) == {0, 1}
    assert (lab[2] == max(ncls - 1, 1)).all()
    assert blob_masks(2, (16, 32), ncls).shape[0] == 2


def _windows(a):
    N, H, W, C = a.shape
    return a.reshape(N, H // 2, 2, W // 2, 2, C).transpose(0, 1, 3, 5, 2, 4).reshape(-1, 4)


def _last_max_bwd(a, dout, first=K.maxpool2_bwd):
    """K.maxpool2_bwd with each window's gradient on its LAST maximum: the first one of the mirrored window."""
    return first(a[:, ::-1, ::-1], dout[:, ::-1, ::-1])[:, ::-1, ::-1]


@pytest.mark.parametrize("name", FLAT_CASES)
def test_flat_inputs_tie_and_the_tie_break_is_unobservable(name, monkeypatch):
    from unet_amd.engine import _mix64, drop_sites
    cfg, filters, _ = geometry_cfg(name)
    _, ncls, bn, drop, _ = cfg
    w32, x, y = flat_draw(name, 0)
    p = {k: v.astype(np.float64) for k, v in w32.items()}
    seeds = {s: _mix64(GEOMETRY_ENGINE_SEED, 1, i + 1) for i, s in enumerate(drop_sites(len(filters)))}
    orc = UNetOracle(ncls, drop, bn, filters)
    prob, cache, _ = orc.forward(p, x.astype(np.float64), training=True, drop_seeds=seeds if drop > 0 else None)
    win = _windows(cache["enc1_skip"])
    mx = win.max(1)
    tie = ((win == mx[:, None]).sum(1) > 1) & (mx > 0)
    first_loses = tie & (win[:, 0] < mx)
    print(f"{name}: positive ties in {tie.mean():.3f} of the enc1 windows, first element not a maximum in "
          f"{first_loses.mean():.3f}")
    assert tie.mean() >= 0.25 and first_loses.mean() >= 0.05
    for loss in ("dice", "iou"):
        _, dprob = orc.loss_and_dprob(y.astype(np.float64), prob, loss)
        g, _ = orc.backward(p, cache, dprob)
        with monkeypatch.context() as mp:
            mp.setattr(K, "maxpool2_bwd", _last_max_bwd)
            g_last, _ = orc.backward(p, cache, dprob)
        # (the routing itself does differ: the data gradient of the pooled block is another tensor)
        da = np.ones_like(K.maxpool2(cache["enc1_skip"]))
        assert not np.array_equal(K.maxpool2_bwd(cache["enc1_skip"], da), _last_max_bwd(cache["enc1_skip"], da))
        worst = max(max(norm_err(g_last[k], g[k]), rel_err(g_last[k], g[k])) for k in g)
        print(f"{name} {loss}: last-maximum routing changes the weight gradients by {worst:.2e}")
        assert worst <= 1e-12


@pytest.mark.parametrize("name", sorted(FLAT_SEEDS))
def test_flat_seed_bases_follow_the_rule(name):
    first = next(b for b in range(9000, 9016) if geometry_oracle32_agrees(name, 0, b, draw=flat_draw))
    assert FLAT_SEEDS[name] == first


def test_flat_draw_without_batchnorm_has_exact_zero_preactivations():
    """deep5's flat draw (no BatchNorm, every bias zero, as a fresh network): wherever a pixel's 3x3
    neighbourhood is black, the first block's z + b is exactly 0 in float64 and float32 alike -- the case a
    ReLU mask written `>= 0` gets wrong -- and both masks appear in the batch."""
    w32, x, y = flat_draw("deep5", 0)
    assert all(not v.any() for k, v in w32.items() if k.endswith("/bias"))
    assert y.shape[0] == 2 and not y[0].any() and y[1].any() and not y[1].all()
    z = K.pointwise(K.depthwise3x3(x, w32["enc1_block1_sepconv/depthwise_kernel"]),
                    w32["enc1_block1_sepconv/pointwise_kernel"])
    black = K.depthwise3x3((x != 0).any(-1, keepdims=True).astype(np.float32), np.ones((3, 3, 1, 1), np.float32)) == 0
    assert black.mean() >= 0.05 and not z[black[..., 0]].any()
