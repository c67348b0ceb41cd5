"""Networks off the default filters, on a host without a GPU: for every entry of helpers.GEOMETRIES the
topology and the training and inference plans are built and held to what the library admits.

  * no block takes the fused block backward (unet_sepconv_bwd_fused) while the view it reads is dropped;
  * every route a plan names is one the library's pure `*_supported` / `*_slabs` queries admit for the
    view it will be launched on (the views are restated here from the network's structure alone);
  * the split-precision plane segments do not overlap, start on multiples of 8 elements and stay
    within their arenas, and read inside the flat weight buffer;
  * each geometry still reaches the routes it was chosen for (REACHES);
  * the dropout seed sites cover every stage of any depth, and are the historical tuple at depth 4;
  * filter tuples and class counts the head cannot run, and a depth whose split segments do not fit
    one refresh launch, are refused with a ValueError where the model is built.
"""
from types import SimpleNamespace

import pytest

from helpers import GEOMETRIES, TRACE_DEFAULTS
from unet_amd import _lib as L
from unet_amd import ops
from unet_amd import plan as P
from unet_amd.params import flat_layout, unet_variables


def _setup(name):
    size, filters, ncls, bn, drop, fuse, n = GEOMETRIES[name]
    eng = SimpleNamespace(**{**TRACE_DEFAULTS, "fuse_sepconv": fuse}, use_bn=bn, sync_bn=False, sync_world=1,
                          dropout_rate=drop, num_classes=ncls)
    topo = P.build_topology(size[0], size[1], size[2], filters, ncls, bn)
    return topo, P.Knobs.of(eng), n


def _plans(name):
    topo, knobs, n = _setup(name)
    return topo, n, P.plan_step(topo, n, True, knobs), P.plan_step(topo, n, False, knobs)


def input_views(t, drop):
    """block -> (the view its forward and weight gradients read, the view its data gradient reads),
    from the network's structure (model/u_net.py:55-112): the image, a block's output, a max-pool of
    one, or [upsample, skip] with the stage's dropout on every decoder stage but the last."""
    out = {}

    def pair(b1, b2, v, vd=None):
        out[b1.name] = (v, vd or v)
        o = P.ShapeView(L.VIEW_BNRELU, b1.cout)
        out[b2.name] = (o, o)

    v = P.ShapeView(L.VIEW_PLAIN, t.cpad)
    vd = None
    for _, b1, b2 in t.enc:
        pair(b1, b2, v, vd)
        v, vd = P.ShapeView(L.VIEW_BNRELU, b2.cout), P.ShapeView(L.VIEW_POOL_BNRELU, b2.cout)
    pair(t.bneck[0], t.bneck[1], v, vd)
    nd = len(t.dec)
    for i, (_stage, fi, _cin, b1, b2) in enumerate(t.dec):
        skip = t.enc[nd - 1 - i][2]
        pair(b1, b2, P.ShapeView(L.VIEW_CONCAT, fi, skip.cout, drop and i < nd - 1))
    return out


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_no_fused_block_backward_on_a_dropped_view(name):
    topo, n, train, _ = _plans(name)
    views = input_views(topo, train.drop)
    for b in topo.blocks:
        if train.bwd[b.name].dz is P.Dz.FUSED_BLOCK:
            assert not views[b.name][0].dropped, f"{name}: {b.name} takes unet_sepconv_bwd_fused on a dropped view"


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_every_route_is_admitted_by_the_library(name):
    topo, n, train, infer = _plans(name)
    views = input_views(topo, train.drop)
    iviews = input_views(topo, False)
    for b in topo.blocks:
        h, w = topo.dims(b.level)
        assert h > 0 and w > 0 and h * (1 << b.level) == topo.h and w * (1 << b.level) == topo.w
        vf, vd = views[b.name]
        what = f"{name}: {b.name}"
        assert vf.channels == b.cin, what
        for plan, v in ((train, vf), (infer, iviews[b.name][0])):
            f = plan.fwd[b.name]
            if f.fused:
                assert ops.sepconv_supported(v, n, h, w, b.cout), what
            if f.x3:
                assert b.name in topo.x3_off and b.cin % 16 == 0 and b.cin >= 64, what
            assert f.keep_y == plan.training or (f.fused and not f.keep_y), what
        assert not any(f.keep_y for f in infer.fwd.values())
        f, r = train.fwd[b.name], train.bwd[b.name]
        if f.fused and not f.keep_y:  # the weight gradients recompute y: some launch must do that
            assert ops.sepconv_bwd_filter_supported(vf, n, h, w, b.cout), what
            assert r.dz is P.Dz.FUSED_BLOCK or P.WGrad.RECOMPUTE_Y in r.wgrads, what
        if r.dz is P.Dz.FUSED_BLOCK:
            assert b.cout == 64 and not vf.dropped and ops.sepconv_bwd_filter_supported(vf, n, h, w, b.cout), what
            assert f.fused and not f.keep_y and r.wgrads == () and r.wgrads_at is P.At.NONE, what
        else:
            assert not r.rank1, what
        if P.WGrad.RECOMPUTE_Y in r.wgrads:
            assert ops.sepconv_bwd_filter_supported(vf, n, h, w, b.cout) and r.wgrads == (P.WGrad.RECOMPUTE_Y,), what
        elif r.dz not in (P.Dz.FUSED_BLOCK, P.Dz.IMAGE_ALL):
            assert f.keep_y, f"{what}: its weight gradients read a y the forward did not keep"
        if r.dz is not P.Dz.UNFUSED:
            assert b.cin % 4 == 0 and b.cout % 4 == 0, what
        if r.dz in (P.Dz.IMAGE_ALL, P.Dz.IMAGE_WGRAD):
            assert b.cin == 4 and b.cout in (32, 64), what
        if r.dz is P.Dz.IMAGE_ALL:
            assert vf == P.ShapeView(L.VIEW_PLAIN, 4) and r.da is P.Da.NONE, what
        if r.x6:
            assert r.dz is P.Dz.GEMM_BN and b.name in topo.x3d_off and b.cout % 32 == 0 and b.cin % 4 == 0, what
        if bool(b.wcin) and r.dz is not P.Dz.IMAGE_ALL:
            assert P.WGrad.COPY_BACK in r.wgrads, what
        # the data gradient: its slab count is the query's, on the view it is launched on
        want = ops.dwconv3x3_bwd_data_bnstats_slabs(vd, n, h, w) if r.da in (P.Da.BNSTATS, P.Da.BNSTATS_DWF) else 0
        assert r.da_slabs == want and (want > 0) == (r.da in (P.Da.BNSTATS, P.Da.BNSTATS_DWF)), what
        if r.da is P.Da.BNSTATS_DWF:
            assert vd.mode == L.VIEW_BNRELU and not vd.dropped and vd == vf, what
        assert (r.da is P.Da.NONE) == (b is topo.blocks[0]), what
    # the statistics a block finishes are the partials its da's producer emitted, slab for slab
    producer = {}
    last = topo.dec[-1][4]
    hv = P.ShapeView(L.VIEW_BNRELU, last.cout)
    assert train.head.slabs in (0, ops.head_bwd_bnstats_slabs(hv, n, topo.h, topo.w, GEOMETRIES[name][2]))
    producer[last.name] = train.head.slabs
    nd = len(topo.dec)
    for i, (stage, fi, _cin, b1, b2) in enumerate(topo.dec):
        producer[b1.name] = train.bwd[b2.name].da_slabs
        prev = topo.dec[i - 1][4] if i > 0 else topo.bneck[1]
        h, w = topo.dims(b1.level + 1)
        xv = P.ShapeView(L.VIEW_BNRELU, prev.cout, 0, i == 0 and train.drop)
        ct = train.convt[stage]
        assert ct.slabs in (0, ops.conv_transpose2x2_bwd_data_bnstats_slabs(xv, n, h, w, fi)), f"{name}: {stage}"
        assert ct.masked == (ct.slabs > 0 and xv.dropped), f"{name}: {stage}"
        producer[prev.name] = ct.slabs
    producer[topo.bneck[0].name] = train.bwd[topo.bneck[1].name].da_slabs
    for j, (_, e1, e2) in enumerate(topo.enc):
        producer[e1.name] = train.bwd[e2.name].da_slabs
        nxt = topo.enc[j + 1][1] if j + 1 < len(topo.enc) else topo.bneck[0]
        # (the skip half of an encoder stage's da is stored by the decoder, the pooled half added by this launch)
        producer[e2.name] = train.bwd[nxt.name].da_slabs
    for b in topo.blocks:
        r = train.bwd[b.name]
        assert r.stats_slabs in (0, producer[b.name]), f"{name}: {b.name} finishes {r.stats_slabs} slabs"
        if r.dz is P.Dz.UNFUSED:
            assert r.stats_slabs == 0, f"{name}: {b.name}"
    if train.head.rank1:
        assert GEOMETRIES[name][2] == 1 and train.bwd[last.name].dz is P.Dz.FUSED_BLOCK and train.bwd[last.name].rank1


def _disjoint(segs, size, what):
    """segs: (start, elements) in one arena of `size` elements."""
    end = 0
    for start, nel in sorted(segs):
        assert start % 8 == 0, f"{what}: a plane segment starts at element {start}"
        assert start >= end, f"{what}: plane segments overlap at element {start}"
        end = start + nel
    assert end <= size, f"{what}: plane segments end at {end} of {size}"


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_plane_segments_are_well_formed(name):
    topo, n, train, infer = _plans(name)
    size, filters, ncls, bn = GEOMETRIES[name][:4]
    lay = flat_layout(unet_variables(size[2], ncls, bn, filters), True)
    off, offd, offt = topo.x3_sizes
    _disjoint([(do, 3 * r * c) for _b, (_so, r, c, do) in topo.x3_cand], off, f"{name} pkx")
    _disjoint([(do, 3 * r * c) for _so, r, c, do in topo.x3d_segs], offd, f"{name} pkd")
    _disjoint([(o, nel) for _, o, nel in topo.x3u_off.values()], offt, f"{name} pkt")
    by_name = {b.name: b for b in topo.blocks}
    for bname, o in topo.x3_off.items():
        assert o + 3 * by_name[bname].cin * by_name[bname].cout <= off
    for bname, o in topo.x3d_off.items():
        assert o + 3 * by_name[bname].cin * by_name[bname].cout <= offd
    for stage, (od, ot, nel) in topo.x3u_off.items():
        assert od + nel <= offd and ot + nel <= offt and nel == 12 * dict((s, f * c) for s, f, c, *_ in topo.dec)[stage]
    for plan in (train, infer):
        assert len(plan.x3_segs) <= L.SPLIT_MAX_SEGS
        _disjoint([(do, 3 * r * c) for _so, r, c, do, _keep in plan.x3_segs], off + offd + offt, f"{name} arena")
        for so, r, c, _do, keep in plan.x3_segs:
            assert keep in (0, 1) and 0 <= so and so + r * c <= lay.total
        assert plan.x3_live == frozenset(b for b, f in plan.fwd.items() if f.x3)
    # the rows GEMMs' segments land in pkd / pkt, the fused forward's in pkx
    assert all(off <= s[3] < off + offd + offt for s in topo.x3_mixed)
    assert not infer.x6 and all(s[3] < off for s in infer.x3_segs)


def _count(plan, dz):
    return sorted(b for b, r in plan.bwd.items() if r.dz is dz)


def _reach_two64(t, p, q):
    assert t.dims(1) == (16, 32)
    fused = _count(p, P.Dz.FUSED_BLOCK)
    assert {"enc2_block1", "enc2_block2", "dec2_block2", "dec1_block1", "dec1_block2"} <= set(fused)
    r = p.bwd["dec2_block1"]  # the dropped concat into a 64-output block: the GEMM + the y-recomputing filter pass
    assert p.fwd["dec2_block1"].fused and not p.fwd["dec2_block1"].keep_y
    assert r.dz is P.Dz.GEMM_BN and r.x6 and r.wgrads == (P.WGrad.RECOMPUTE_Y,) and len(fused) == 6
    assert p.convt["dec2"].masked and p.convt["dec2"].slabs > 0 and p.head.rank1
    assert p.bwd["enc1_block1"].dz is P.Dz.IMAGE_ALL


def _reach_two64_nodrop(t, p, q):
    fused = _count(p, P.Dz.FUSED_BLOCK)
    assert len(fused) == 7 and {"enc2_block1", "enc2_block2", "dec2_block1", "dec2_block2"} <= set(fused)
    assert not p.drop and not p.convt["dec2"].masked and p.head.rank1


def _reach_two64_auto(t, p, q):
    assert t.dims(1) == (64, 64) and not p.fwd["bneck_block1"].fused  # the pixel rule: 64 x 64 fuses, 32 x 32 does not
    r = p.bwd["dec2_block1"]
    assert p.fwd["dec2_block1"].fused and not p.fwd["dec2_block1"].keep_y
    assert r.dz is P.Dz.GEMM_BN and r.wgrads == (P.WGrad.RECOMPUTE_Y,) and r.wgrads_at is P.At.DEFER
    assert len(_count(p, P.Dz.FUSED_BLOCK)) == 6 and p.head.rank1


def _reach_gray3264(t, p, q):
    assert (t.c, t.cpad) == (1, 4) and t.blocks[0].wcin == 1
    assert p.bwd["enc1_block1"].dz is P.Dz.IMAGE_ALL and t.blocks[0].cout == 32
    assert p.fwd["enc1_block2"].fused and not p.fwd["enc1_block2"].x3  # 32 channels: the LDS-tile fused kernel
    assert p.bwd["enc1_block2"].x6 and p.bwd["enc2_block1"].x6 and p.bwd["dec1_block1"].x6  # x6 at cout 32 and 64
    assert p.bwd["dec2_block1"].dz is P.Dz.GEMM_BN and p.bwd["dec2_block1"].wgrads == (P.WGrad.RECOMPUTE_Y,)
    assert _count(p, P.Dz.FUSED_BLOCK) == ["dec2_block2", "enc2_block2"] and not p.head.rank1


def _reach_thin(t, p, q):
    assert not any(f.fused for f in p.fwd.values()) and not any(f.fused for f in q.fwd.values())
    assert p.x3_live == {"bneck_block2", "dec2_block1"}  # no forward planes before the bottleneck
    r = p.bwd["enc1_block1"]
    assert t.blocks[0].cout == 16 and r.dz is P.Dz.GEMM_BN and P.WGrad.COPY_BACK in r.wgrads
    assert p.head.slabs > 0 and not p.head.rank1 and t.dims(1) == (16, 24)


def _reach_mult8(t, p, q):
    assert all(f.fused for f in p.fwd.values()) and all(b.cin % 8 == 0 and b.cout % 8 == 0 for b in t.blocks[1:])
    assert sum(b.cout % 16 != 0 for b in t.blocks) >= 8 and t.dec[-1][3].cin == 48
    # no depthwise data gradient and no head emits partials at these widths: own statistics passes
    assert all(r.da_slabs == 0 for r in p.bwd.values()) and p.head.slabs == 0
    assert sum(r.stats_slabs == 0 for r in p.bwd.values()) == 8
    assert p.x3_live == {"bneck_block2", "dec2_block1"} and t.bneck[1].cin == 80


def _reach_wide80(t, p, q):
    assert sorted({b.cin for b in t.blocks if p.fwd[b.name].x3}) == [80, 144, 160, 288]
    assert all(p.fwd[b.name].fused for b in t.blocks) and 80 % 32 == 144 % 32 == 16  # (the K loop's half step)
    assert sorted(b for b, r in p.bwd.items() if r.x6) == ["bneck_block1", "bneck_block2"] and t.bneck[0].cout == 288
    assert p.head.slabs == 0 and p.convt["dec2"].masked


def _reach_not4(t, p, q):
    unfused = _count(p, P.Dz.UNFUSED)
    assert unfused == ["bneck_block1", "dec2_block1", "dec2_block2", "enc2_block1", "enc2_block2"]
    assert t.dec[0][3].cin == 20 and t.dec[0][1] == 10  # CONCAT with c0 = 10
    # an UNFUSED block whose data gradient still emits the partials a % 4 block finishes
    assert p.bwd["enc2_block1"].da is P.Da.BNSTATS and p.bwd["enc1_block2"].stats_slabs == p.bwd["enc2_block1"].da_slabs > 0
    assert p.bwd["bneck_block2"].dz is P.Dz.GEMM_BN and p.bwd["bneck_block2"].stats_slabs == 0


def _reach_deep5(t, p, q):
    assert len(t.enc) == 5 and t.dims(5) == (2, 1) and not p.batch_stats
    assert set(p.convt) == {f"dec{s}" for s in range(1, 6)} and p.convt["dec5"].masked
    assert [p.fwd[b.name].fused for b in t.blocks[:4]] == [True] * 4 and not p.fwd["enc3_block1"].fused
    assert len(p.x3_segs) > 22  # more split segments than the default network's step


def _reach_one_level(t, p, q):
    assert len(t.enc) == 1 and (t.c, t.cpad) == (5, 8)
    assert not any(v[0].dropped for v in input_views(t, p.drop).values())  # no dropped concat ...
    assert p.drop and p.convt["dec1"].masked  # ... the masked ConvT gradient only
    assert P.WGrad.COPY_BACK in p.bwd["enc1_block1"].wgrads and p.bwd["enc1_block1"].dz is P.Dz.GEMM_BN
    assert _count(p, P.Dz.FUSED_BLOCK) == ["dec1_block1", "dec1_block2", "enc1_block2"] and p.head.rank1


REACHES = {"two64": _reach_two64, "two64_nodrop": _reach_two64_nodrop, "two64_auto": _reach_two64_auto,
           "gray3264": _reach_gray3264, "thin": _reach_thin, "mult8": _reach_mult8, "wide80": _reach_wide80,
           "not4": _reach_not4, "deep5": _reach_deep5, "one_level": _reach_one_level}


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_each_geometry_reaches_what_it_was_chosen_for(name):
    """Route counts under today's policy: a policy change that moves a geometry off the code it was
    chosen to reach must fail here, not quietly thin the GPU suite."""
    assert set(REACHES) == set(GEOMETRIES)
    topo, n, train, infer = _plans(name)
    REACHES[name](topo, train, infer)


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_dropout_sites_cover_every_stage(name):
    from unet_amd import engine as E
    topo, n, train, _ = _plans(name)
    depth = len(topo.enc)
    sites = E.drop_sites(depth)
    want = ["bneck_dropout"] + [f"{stage}_dropout" for stage, *_ in topo.dec[:-1]]
    assert list(sites) == want and len(set(sites)) == depth
    assert want[1:] == [f"dec{s}_dropout" for s in range(depth, 1, -1)]


def test_dropout_sites_of_the_default_depth_are_unchanged():
    from unet_amd import engine as E
    assert E.drop_sites(4) == ("bneck_dropout", "dec4_dropout", "dec3_dropout", "dec2_dropout") == E.DROP_SITES
    assert E.drop_sites(1) == ("bneck_dropout",)


@pytest.mark.parametrize("filters,ncls,limit", [((6, 10), 1, r"filters\[0\] % 4 == 0"),
                                                ((2,), 1, r"filters\[0\] % 4 == 0"),
                                                ((260, 8), 1, "at most 256 input channels"),
                                                ((64, 128), 33, "1 to 32 classes"),
                                                ((), 1, "non-empty"),
                                                ((8, 0), 1, "positive")])
def test_bad_tuples_are_refused_at_construction(filters, ncls, limit):
    from unet_amd.engine import UNetEngine
    from unet_amd.params import check_geometry
    with pytest.raises(ValueError, match=limit):
        check_geometry(filters, ncls)
    with pytest.raises(ValueError, match=limit):  # (before the constructor asks for a device)
        UNetEngine((32, 32, 3), ncls, filters=filters)


def test_good_tuples_pass_the_construction_check():
    from unet_amd.params import check_geometry
    for name, (_size, filters, ncls, *_rest) in GEOMETRIES.items():
        assert check_geometry(filters, ncls) == tuple(filters), name
    assert check_geometry([256, 7], 32) == (256, 7) and check_geometry((4,), 1) == (4,)


def test_a_depth_whose_split_segments_exceed_one_launch_is_refused_with_the_topology():
    """Eight 64-wide levels on a 4-channel input: 33 forward + 34 data-gradient + 8 + 8 upsample = 83 split
    segments against UNET_SPLIT_MAX_SEGS = 64.  Pinned: build_topology raises (and so does the model's
    constructor, which builds it); no plan lists more segments than one launch takes."""
    assert L.SPLIT_MAX_SEGS == 64
    with pytest.raises(ValueError, match="83 split-precision weight segments.*at most 64"):
        P.build_topology(256, 256, 4, (64,) * 8, 1, True)
    with pytest.raises(ValueError, match="73 split-precision weight segments"):
        P.build_topology(128, 128, 4, (64,) * 7, 1, True)
    from unet_amd.engine import UNetEngine
    with pytest.raises(ValueError, match="split-precision weight segments"):  # (before it asks for a device)
        UNetEngine((256, 256, 4), 1, filters=(64,) * 8)
    topo = P.build_topology(64, 64, 4, (64,) * 6, 1, True)  # 25 + 26 + 6 + 6 = 63: the deepest that fits
    assert len(topo.x3_cand) + len(topo.x3_mixed) == 63


@pytest.mark.parametrize("name", [g for g in GEOMETRIES if g != "two64_auto"])
def test_seed_bases_are_the_ones_the_float32_oracle_agrees_on(name):
    """helpers.GEOMETRY_SEEDS: draw 0 of every geometry is one whose ReLU / max-pool decisions the float32
    oracle shares with float64 (two64_auto has no such base: see the table's comment)."""
    from helpers import geometry_oracle32_agrees
    assert geometry_oracle32_agrees(name, 0)
