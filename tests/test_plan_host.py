"""unet_amd.plan on a host without a GPU: for every configuration of the launch-trace fixture
(tests/golden/step_traces.json, recorded on an MI355X) the step plan, built from shape-only views,
implies the recorded kernel launches -- entry point and stream, in order.  (Arguments need the
device: tests/test_step_trace_gpu.py.)  `implied` below is the schedule of engine.forward /
backward restated over plan fields alone; it names no kernel the plan's route enumerations do not.

Also: the two route combinations that cannot run raise when the plan is built, not mid-backward."""
import json
import os
from dataclasses import replace
from types import SimpleNamespace

import pytest

from helpers import TRACE_BATCH, TRACE_CONFIGS, TRACE_DEFAULTS
from unet_amd import _lib as L
from unet_amd import plan as P
from unet_amd.params import FILTERS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_traces.json")


def _setup(cid, **over):
    size, ncls, bn, drop, attrs = TRACE_CONFIGS[cid]
    eng = SimpleNamespace(**{**TRACE_DEFAULTS, **attrs}, use_bn=bn, sync_bn=False, sync_world=1, dropout_rate=drop,
                          num_classes=ncls)
    topo = P.build_topology(size[0], size[1], size[2], FILTERS, ncls, bn)
    return topo, replace(P.Knobs.of(eng), **over)


def implied(t, p):
    """[(entry point, on the side stream)] of one forward (+ loss, backward and AdamW when training)."""
    out, pending = [], []
    side = int(p.overlap)

    def main(*names):
        out.extend((nm, 0) for nm in names)

    def flush():
        out.extend((nm, 1) for nm in pending)
        del pending[:]

    if t.cpad != t.c:
        main("unet_copy_strided")
    if p.x3_segs:
        main("unet_split_x3_mixed")
    pooled = {b2.name for _, _, b2 in t.enc}

    def block_fwd(b):
        f = p.fwd[b.name]
        if b.wcin:
            main("unet_copy_strided", "unet_copy_strided")
        if f.fused:
            main("unet_sepconv_fwd")
        else:
            main("unet_dwconv3x3_fwd", "unet_pointwise_fwd_x3" if f.x3 else "unet_pointwise_fwd")
            if b.name in pooled:
                main("unet_pool_select")
        main("unet_bn_finalize" if p.batch_stats else "unet_bn_infer_params")

    for _, b1, b2 in t.enc:
        block_fwd(b1)
        block_fwd(b2)
    block_fwd(t.bneck[0])
    block_fwd(t.bneck[1])
    for stage, _fi, _cin, b1, b2 in t.dec:
        main("unet_conv_transpose2x2_fwd_x3" if p.x6 else "unet_conv_transpose2x2_fwd")
        block_fwd(b1)
        block_fwd(b2)
    main("unet_head_fwd")
    if not p.training:
        return out
    main("unet_dice_fwd")

    def block_bwd(b):
        r = p.bwd[b.name]
        if r.dz is P.Dz.UNFUSED:
            main("unet_bn_relu_bwd", "unet_pointwise_bwd_data")
        else:
            main("unet_bn_relu_bwd_stats_finish" if r.stats_slabs else "unet_bn_relu_bwd_stats")
            flush()
            main(r.dz.value + ("_x3" if r.x6 else ""))
        names = [nm for g in r.wgrads for nm in ([g.value] * (2 if g is P.WGrad.COPY_BACK else 1))]
        if r.wgrads_at is P.At.MAIN:
            main(*names)
        elif r.wgrads_at is not P.At.NONE:
            flush()
            if r.wgrads_at is P.At.DEFER:
                pending.extend(names)
            else:
                out.extend((nm, 1) for nm in names)
        if r.da is not P.Da.NONE:
            main(r.da.value)
        if r.da is P.Da.BNSTATS_DWF:
            out.append(("unet_reduce_slabs", side))

    main("unet_head_bwd_bnstats" if p.head.slabs else "unet_head_bwd")
    for stage, _fi, _cin, b1, b2 in reversed(t.dec):
        block_bwd(b2)
        block_bwd(b1)
        if p.convt[stage].slabs:
            main("unet_conv_transpose2x2_bwd_data_bnstats" + ("_x3" if p.x6 else ""))
        else:
            main("unet_conv_transpose2x2_bwd")
        out.append(("unet_conv_transpose2x2_bwd", side))
    block_bwd(t.bneck[1])
    block_bwd(t.bneck[0])
    for _, e1, e2 in reversed(t.enc):
        block_bwd(e2)
        block_bwd(e1)
    flush()
    main("unet_adamw_step")
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        d = json.load(f)
    assert d["batch"] == TRACE_BATCH
    return d["traces"]


@pytest.mark.parametrize("cid", list(TRACE_CONFIGS))
def test_plan_implies_the_recorded_launches(golden, cid):
    topo, knobs = _setup(cid)
    plan = P.plan_step(topo, TRACE_BATCH, cid != "P", knobs)
    want = [(name, side) for name, side, _args in golden[cid]]
    got = implied(topo, plan)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{cid}: launch {i}"
    assert len(got) == len(want)


def test_plans_are_values():
    """Equal inputs give equal plans (the engine caches them by (batch, training, Knobs)); a knob that
    routes gives another."""
    topo, knobs = _setup("A")
    a = P.plan_step(topo, 2, True, knobs)
    assert a == P.plan_step(topo, 2, True, replace(knobs)) and hash(knobs) == hash(replace(knobs))
    assert a != P.plan_step(topo, 2, True, replace(knobs, fuse_sepconv="never"))
    assert a.bwd["dec1_block2"].rank1 and a.head.rank1 and a.convt["dec4"].masked


def test_shape_view_is_the_views_struct():
    """A ShapeView puts to the library what a View of the same shape does, but for the pointers."""
    v = P.ShapeView(L.VIEW_CONCAT, 64, 128, True).c_struct()
    assert (v.mode, v.c0, v.c1, v.src0, v.src1) == (L.VIEW_CONCAT, 64, 128, None, None) and v.drop_rate > 0
    assert P.ShapeView(L.VIEW_BNRELU, 64, 7).c_struct().c1 == 0  # (c1 counts for a concat only)


def test_syncbn_off_the_fused_bn_backward_raises_at_plan_time():
    topo, knobs = _setup("A", sync_bn=True, fuse_bn_bwd=False)
    with pytest.raises(RuntimeError, match="SyncBN needs the fused BN-backward route"):
        P.plan_step(topo, 2, True, knobs)
    P.plan_step(topo, 2, False, knobs)  # (inference has no backward to route)


def test_rank_one_head_without_the_fused_block_backward_raises_at_plan_time():
    """plan_step derives the head's rank-one form and the last block's fused backward from one
    predicate, so no Knobs value separates them; forced at the block's route (rank1 with
    fuse_block_bwd off) it is refused there, where plan_step would meet it."""
    topo, knobs = _setup("A", fuse_block_bwd=False)
    plan = P.plan_step(topo, 2, True, knobs)
    assert not plan.head.rank1
    last = topo.dec[-1][4]
    v = P.ShapeView(L.VIEW_BNRELU, last.cin)
    with pytest.raises(RuntimeError, match="rank-one da without the fused block backward"):
        P.block_bwd_route(topo, knobs, last, plan.fwd[last.name], 2, topo.h, topo.w, v, v, True, True, False,
                          plan.head.slabs, False, True)
