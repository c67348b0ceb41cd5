"""Which kernels a step launches: the engine's routing policy, resolved once per (batch, mode, knobs).

`plan_step` walks the network's topology with views described by shape only and returns a StepPlan:
per block the forward and backward routes, the head's and the Conv2DTranspose stages' routes, and
the split-plane refresh list.  The engine (engine.py) executes a StepPlan and decides nothing.

Nothing here touches a device: the policy needs channel counts, view modes, sizes and the
library's pure `*_supported` / `*_slabs` queries, which libunet_hip.so answers on any host.
A route that cannot run (SyncBN off the fused BN-backward route, a rank-one head gradient without
the fused block backward) raises here, before any launch of the step is issued.
"""
from __future__ import annotations

import enum
from dataclasses import dataclass
from typing import Dict, Tuple

from . import _lib as L
from . import ops
from .params import flat_layout, unet_variables

FUSE_MIN_PIXELS = 64 * 64  # fused conv forward from the 64 x 64 level up (tools/bench_sepconv.py sweeps)
# ... and on a smaller level once the batch gives it >= 128 pixel tiles: the 32 x 32 level from
# batch 16 (configs[1]; with the weight planes staged by LDS-DMA its bf16x6 launch 54.8 -> 47.3 us, and
# the step 10.44-10.47 -> 10.37-10.41 ms, profiles/r6h_fuse32_b16_ab.txt); at batch 8 (configs[4] per
# GPU) the split launches stay faster (6.05-6.07 vs 6.15-6.16 ms)
# (a fixed constant: every data-parallel rank takes the same route; an A/B sets the engine attributes
# fuse_min_pixels / fuse_min_total, bench.py --fuse-min-pixels / --fuse-min-total)
FUSE_MIN_TOTAL_PIXELS = 16 * 1024
# blocks whose weight gradients recompute y instead of the forward storing it: an output channel count
# (64: the fused block backward), or an (input, output) channel pair
RECOMPUTE_Y_COUTS = (64,)


# ------------------------------------------------------------------------ inputs ------
@dataclass(frozen=True)
class Knobs:
    """Every engine attribute that routing reads, frozen and hashable (a plan / graph cache key)."""

    fuse_sepconv: str
    fuse_min_pixels: int
    fuse_min_total: int
    recompute_y: bool
    recompute_y_couts: tuple
    fuse_bn_bwd: bool
    fuse_bn_stats: bool
    img_fused_wgrad: bool
    img_fused_dwf: bool
    fuse_block_bwd: bool
    dw_fused_filter: bool
    defer_sw: bool
    overlap: bool
    use_x3: bool
    x6_gemm: bool
    use_bn: bool
    sync_bn: bool  # SyncBN in effect (asked for, BatchNorm on, more than one replica)
    dropout: bool  # dropout_rate > 0
    num_classes: int

    @classmethod
    def of(cls, eng) -> "Knobs":
        """Snapshot of an engine's (or any object's) routing attributes."""
        return cls(eng.fuse_sepconv, eng.fuse_min_pixels, eng.fuse_min_total, bool(eng.recompute_y),
                   tuple(tuple(c) if isinstance(c, (tuple, list)) else c for c in eng.recompute_y_couts),
                   bool(eng.fuse_bn_bwd), bool(eng.fuse_bn_stats), bool(eng.img_fused_wgrad), bool(eng.img_fused_dwf),
                   bool(eng.fuse_block_bwd), bool(eng.dw_fused_filter), bool(eng.defer_sw), bool(eng.overlap),
                   bool(eng.use_x3), bool(eng.x6_gemm), bool(eng.use_bn),
                   bool(eng.sync_bn and eng.sync_world > 1 and eng.use_bn), eng.dropout_rate > 0.0, eng.num_classes)


@dataclass(frozen=True)
class ShapeView:
    """A unet_view by shape only: what the library's `*_supported` / `*_slabs` queries read."""

    mode: int
    c0: int
    c1: int = 0
    dropped: bool = False

    @property
    def channels(self) -> int:
        return self.c0 + (self.c1 if self.mode == L.VIEW_CONCAT else 0)

    def c_struct(self) -> L.UnetView:
        # null sources; the queries read the dropout rate only as zero / non-zero
        return ops.view_fields(self.mode, self.c0, self.c1, 0.5 if self.dropped else 0.0, 0)


@dataclass(frozen=True)
class Block:
    """One conv_block (SeparableConv2D -> BatchNormalization -> ReLU)."""

    name: str
    cin: int    # channels the kernels see (the image block is padded to a multiple of 4)
    cout: int
    level: int  # spatial size = input / 2**level
    wcin: int = 0  # channels of the Keras weights when they differ from cin (padded block)


@dataclass(frozen=True)
class Topology:
    """The network as the schedule walks it, and where its split-precision planes live."""

    h: int
    w: int
    c: int
    cpad: int  # the image block's input channels: c padded to a multiple of 4
    enc: tuple  # (stage, block1, block2)
    bneck: tuple  # (block1, block2)
    dec: tuple  # (stage, filters, upsample input channels, block1, block2)
    blocks: tuple
    # split-precision planes: element offsets per block / stage, and the split_x3 segments
    x3_off: Dict[str, int]  # fused-forward planes (pkx)
    x3_cand: tuple  # (block, (source, rows, cols, destination))
    x3d_off: Dict[str, int]  # BN-backward data-gradient planes (pkd)
    x3d_segs: tuple
    x3u_off: Dict[str, tuple]  # upsample kernels: (offset in pkd, offset in pkt, elements)
    x3_sizes: tuple  # elements of (pkx, pkd, pkt) in the one arena
    x3_mixed: tuple  # the rows GEMMs' segments (pkd, pkt) as unet_split_x3_mixed takes them

    def dims(self, level: int):
        return self.h >> level, self.w >> level


def build_topology(h: int, w: int, c: int, filters, num_classes: int, use_bn: bool) -> Topology:
    f = tuple(int(v) for v in filters)
    # The image block runs on a channel-padded copy of the input (3 -> 4 channels, zero
    # padding), so every kernel takes its vectorised / fused path; its Keras-shaped weights
    # are mirrored into padded buffers each forward and the gradients copied back.
    cpad = c if c % 4 == 0 else (c + 3) // 4 * 4
    enc, ci = [], c
    for i, fi in enumerate(f):
        b1 = Block(f"enc{i + 1}_block1", ci, fi, i) if i > 0 or cpad == c else \
            Block(f"enc{i + 1}_block1", cpad, fi, i, wcin=c)
        enc.append((f"enc{i + 1}", b1, Block(f"enc{i + 1}_block2", fi, fi, i)))
        ci = fi
    d, bn = len(f), 2 * f[-1]
    bneck = (Block("bneck_block1", ci, bn, d), Block("bneck_block2", bn, bn, d))
    dec, ci = [], bn
    for i, fi in enumerate(reversed(f)):
        stage = len(f) - i
        dec.append((f"dec{stage}", fi, ci, Block(f"dec{stage}_block1", 2 * fi, fi, stage - 1),
                    Block(f"dec{stage}_block2", fi, fi, stage - 1)))
        ci = fi
    blocks = tuple(b for _, b1, b2 in enc for b in (b1, b2)) + bneck + tuple(b for *_, b1, b2 in dec for b in (b1, b2))
    src = flat_layout(unet_variables(c, num_classes, use_bn, f), True).offsets
    # planes of the pointwise kernels of the blocks whose fused forward can run the bf16x6 register-A
    # kernel (channels % 16 == 0, >= 64), [3][Cout][Cin]
    x3_off, x3_cand, off = {}, [], 0
    for b in blocks:
        if b.cin % 16 == 0 and b.cin >= 64 and not b.wcin:
            x3_cand.append((b, (src[f"{b.name}_sepconv/pointwise_kernel"], b.cin, b.cout, off)))
            x3_off[b.name] = off
            off += (3 * b.cin * b.cout + 7) // 8 * 8
    # ... and the same kernels' planes in their own layout ([3][Cin][Cout], k = Cout contiguous)
    # for the split-precision BatchNorm-backward data gradient (unet_pointwise_bwd_data_bnrelu_x3):
    # every block but the padded image block (the 64-output blocks that take the fused block
    # backward do not read theirs)
    x3d_off, x3d_segs, offd = {}, [], 0
    for b in blocks:
        if b.cout % 32 == 0 and b.cin % 4 == 0 and not b.wcin:
            x3d_segs.append((src[f"{b.name}_sepconv/pointwise_kernel"], b.cin, b.cout, offd))
            x3d_off[b.name] = offd
            offd += (3 * b.cin * b.cout + 7) // 8 * 8
    # the Conv2DTranspose kernels (2, 2, f, cin) seen as (4 f, cin): planes in their own layout for
    # the forward (k = cin contiguous) and transposed ([3][cin][4 f]) for the data gradient
    x3u_off, x3t_segs, offt = {}, [], 0
    for stage, fi, cin, _b1, _b2 in dec:
        so = src[f"{stage}_upsample/kernel"]
        x3d_segs.append((so, 4 * fi, cin, offd))
        x3t_segs.append((so, 4 * fi, cin, offt))
        x3u_off[stage] = (offd, offt, 12 * fi * cin)
        offd += (12 * fi * cin + 7) // 8 * 8
        offt += (12 * fi * cin + 7) // 8 * 8
    # one arena, so a training forward refreshes all three plane sets in ONE unet_split_x3_mixed launch
    off, offd, offt = (max(v, 8) for v in (off, offd, offt))
    mixed = tuple((so, r, cc, do + off, 1) for so, r, cc, do in x3d_segs) + \
        tuple((so, r, cc, do + off + offd, 0) for so, r, cc, do in x3t_segs)
    # a step refreshes its live pkx planes and the rows GEMMs' in ONE launch: refuse here the depth
    # whose segments cannot fit one, not at the first forward (7 levels and up with wide channels)
    if len(x3_cand) + len(mixed) > L.SPLIT_MAX_SEGS:
        raise ValueError(f"filters {f}: {len(x3_cand) + len(mixed)} split-precision weight segments, the "
                         f"refresh launch takes at most {L.SPLIT_MAX_SEGS} (UNET_SPLIT_MAX_SEGS); use fewer levels")
    return Topology(h, w, c, cpad, tuple(enc), bneck, tuple(dec), blocks, x3_off, tuple(x3_cand), x3d_off,
                    tuple(x3d_segs), x3u_off, (off, offd, offt), mixed)


# ------------------------------------------------------------------------ routes ------
class Dz(enum.Enum):
    """How a block's backward forms dz (BN + ReLU backward) and dy (the pointwise data gradient)."""

    IMAGE_ALL = "unet_image_block_bwd_wgrad"  # image block: both weight gradients too, neither dz nor dy stored
    IMAGE_WGRAD = "unet_pointwise_bwd_data_bnrelu_wgrad"  # 4-channel block: dy + the pointwise weight gradient
    FUSED_BLOCK = "unet_sepconv_bwd_fused"  # dy and both weight gradients in one pass, dz never stored
    GEMM_BN = "unet_pointwise_bwd_data_bnrelu"  # dz formed inside the data-gradient GEMM's loads
    UNFUSED = "unet_bn_relu_bwd"  # a dz pass, then the plain GEMM


class WGrad(enum.Enum):
    """A weight-gradient launch a block's backward still issues after its dz / dy pass."""

    RECOMPUTE_Y = "unet_sepconv_bwd_filter"  # both kernels' gradients, y recomputed from the input view
    POINTWISE = "unet_pointwise_bwd_filter"
    DEPTHWISE = "unet_dwconv3x3_bwd_filter"
    COPY_BACK = "unet_copy_strided"  # padded image block: the Keras-shaped slices of both gradients


class At(enum.Enum):
    """Where those launches are issued."""

    NONE = 0  # there are none, and no deferred work is flushed (the fused block backward)
    MAIN = 1  # inline on the main stream
    SIDE = 2  # on the side stream beside the block's depthwise data gradient
    DEFER = 3  # on the side stream, after the main stream has issued the next block's statistics


class Da(enum.Enum):
    """The depthwise data gradient: the launch that completes the input block's da."""

    NONE = None  # the network's input: no data gradient
    PLAIN = "unet_dwconv3x3_bwd_data"
    BNSTATS = "unet_dwconv3x3_bwd_data_bnstats"  # ... emitting the input block's BN-backward partials
    BNSTATS_DWF = "unet_dwconv3x3_bwd_data_bnstats_dwf"  # ... and this block's depthwise filter-gradient slabs


@dataclass(frozen=True)
class BlockFwd:
    fused: bool  # one unet_sepconv_fwd launch (else depthwise + pointwise, which always store y)
    keep_y: bool  # the forward stores the depthwise output y for the weight gradients
    x3: bool  # its split-precision planes (pkx) are live for this step


@dataclass(frozen=True)
class BlockBwd:
    dz: Dz
    stats_slabs: int  # > 0: the BN-backward statistics finish the producer's partials of this many slabs; 0: own pass
    rank1: bool  # da is the binary head's dlogit (x) kernel, formed on load
    x6: bool  # the GEMM_BN launch reads the split-precision planes (pkd)
    wgrads: Tuple[WGrad, ...]
    wgrads_at: At
    da: Da
    da_slabs: int  # slabs of the BN partials (and filter-gradient slabs) the data gradient emits


@dataclass(frozen=True)
class HeadBwd:
    slabs: int  # > 0: unet_head_bwd_bnstats emits the last block's BN-backward partials
    rank1: bool  # ... and stores dlogit per pixel instead of the last block's da


@dataclass(frozen=True)
class ConvTBwd:
    slabs: int  # > 0: the data gradient emits the BN-backward partials of the block below
    masked: bool  # ... which carry the dropout mask between that block and the upsample


@dataclass(frozen=True)
class StepPlan:
    training: bool
    batch_stats: bool  # BatchNorm from the batch (training with BatchNorm), else the moving statistics / bias
    drop: bool  # dropout applied (training, rate > 0)
    x6: bool  # the rows GEMMs (upsample, BN-backward data gradient) read split-precision planes
    overlap: bool  # weight gradients on the side stream
    sync_bn: bool
    fwd: Dict[str, BlockFwd]
    bwd: Dict[str, BlockBwd]  # (training plans only)
    head: HeadBwd
    convt: Dict[str, ConvTBwd]  # per decoder stage
    x3_segs: tuple  # ops.split_x3 segments refreshed at the start of the forward
    x3_live: frozenset  # blocks whose pkx planes those segments refresh


def block_fwd_choice(view, n: int, h: int, w: int, cout: int, training: bool, fuse: str = "auto",
                     recompute_y: bool = True, recompute_couts=RECOMPUTE_Y_COUTS, min_total: int = FUSE_MIN_TOTAL_PIXELS,
                     min_pixels: int = FUSE_MIN_PIXELS):
    """The kernels a conv_block forward runs: (fused, keep_y).  fused: one unet_sepconv_fwd launch
    (else unet_dwconv3x3_fwd + unet_pointwise_fwd, which always store y); keep_y: the fused launch
    also stores the depthwise output y for the weight gradients (training blocks whose weight
    gradients do not recompute it).  view: an ops.View or a ShapeView.  Shared by plan_step and
    bench.py's encoder table."""
    want = fuse == "always" or (fuse == "auto" and (h * w >= min_pixels or n * h * w >= min_total))
    if not (want and ops.sepconv_supported(view, n, h, w, cout)):
        return False, training
    y_recompute = training and recompute_y and (cout in recompute_couts or (view.channels, cout) in recompute_couts) and \
        ops.sepconv_bwd_filter_supported(view, n, h, w, cout)
    return True, training and not y_recompute


def _fused_bwd(k: Knobs, b: Block, f: BlockFwd, drop: bool, vf: ShapeView) -> bool:
    """The block's backward runs as one unet_sepconv_bwd_fused pass (f: its training forward; vf: the
    view its weight gradients read).  That kernel refuses a view with dropout (a 64-output block1 of a
    decoder stage but the last): such a block takes the data-gradient GEMM plus
    unet_sepconv_bwd_filter, which admits it."""
    return (k.fuse_block_bwd and k.fuse_bn_bwd and f.fused and not f.keep_y and not drop and b.cout == 64
            and not vf.dropped)


def block_bwd_route(t: Topology, k: Knobs, b: Block, f: BlockFwd, n: int, h: int, w: int, vin: ShapeView, vf: ShapeView,
                    has_dx: bool, has_target: bool, drop: bool, slabs_in: int, masked_in: bool, rank1: bool) -> BlockBwd:
    """Backward route of one block.  vin: its input as the data gradient reads it; vf: as the weight
    gradients read it (vin itself unless the input is a max-pool); has_dx: it has a data gradient;
    has_target: that launch completes the da of the block vin reads; drop: dropout sits on this
    block's output; slabs_in / masked_in / rank1: what the producer of its da left for it."""
    y_recompute = f.fused and not f.keep_y
    fused = _fused_bwd(k, b, f, drop, vf)
    if rank1 and not fused:
        raise RuntimeError(f"{b.name}: rank-one da without the fused block backward")
    img_wg = img_all = False
    stats_slabs = 0
    if k.fuse_bn_bwd and b.cin % 4 == 0 and b.cout % 4 == 0:
        if slabs_in and (not drop or masked_in):
            stats_slabs = slabs_in
        img_wg = k.img_fused_wgrad and not drop and b.cin == 4 and b.cout in (32, 64)
        img_all = img_wg and k.img_fused_dwf and not has_dx and vf.mode == L.VIEW_PLAIN and vf.c0 == 4
        dz = Dz.IMAGE_ALL if img_all else Dz.IMAGE_WGRAD if img_wg else Dz.FUSED_BLOCK if fused else Dz.GEMM_BN
    else:
        if k.sync_bn:
            raise RuntimeError(f"{b.name}: SyncBN needs the fused BN-backward route (fuse_bn_bwd, channels % 4 == 0)")
        dz = Dz.UNFUSED
    producer = has_dx and has_target and k.fuse_bn_stats and k.fuse_bn_bwd
    da_slabs = ops.dwconv3x3_bwd_data_bnstats_slabs(vin, n, h, w) if producer else 0
    # the depthwise filter gradient from the data-gradient pass (unet_dwconv3x3_bwd_data_bnstats_dwf)
    dwf = (k.dw_fused_filter and da_slabs > 0 and vin.mode == L.VIEW_BNRELU and not vin.dropped and vf == vin
           and not fused and not img_all and not y_recompute and not b.wcin)
    if fused or img_all:  # (done by the fused pass)
        wgrads = ()
    elif y_recompute:
        wgrads = (WGrad.RECOMPUTE_Y,)
    else:  # (the image block's pointwise gradient is accumulated by its data-gradient pass)
        wgrads = ((() if img_wg else (WGrad.POINTWISE,)) + (() if dwf else (WGrad.DEPTHWISE,)) +
                  ((WGrad.COPY_BACK,) if b.wcin else ()))
    # the image block (no data gradient) runs its weight gradients on the otherwise idle main
    # stream, beside the side stream's enc1_block2 tail
    if fused:
        at = At.NONE
    elif k.overlap and has_dx:
        at = At.DEFER if k.defer_sw and y_recompute else At.SIDE
    else:
        at = At.MAIN
    da = Da.NONE if not has_dx else Da.BNSTATS_DWF if dwf else Da.BNSTATS if da_slabs > 0 else Da.PLAIN
    return BlockBwd(dz, stats_slabs, rank1, k.x6_gemm and dz is Dz.GEMM_BN and b.name in t.x3d_off,
                    wgrads, at, da, da_slabs)


def plan_step(t: Topology, n: int, training: bool, k: Knobs) -> StepPlan:
    """The routes of one forward (+ backward when training) of a batch of n images under knobs k."""
    drop = training and k.dropout
    six = training and k.x6_gemm
    fwd: Dict[str, BlockFwd] = {}
    vins: Dict[str, ShapeView] = {}

    def bnrelu(b: Block) -> ShapeView:  # a block's output, or its max-pool's window selections
        return ShapeView(L.VIEW_BNRELU, b.cout)

    def block(b: Block, v: ShapeView) -> ShapeView:
        h, w = t.dims(b.level)
        fused, keep_y = block_fwd_choice(v, n, h, w, b.cout, training, k.fuse_sepconv, k.recompute_y,
                                         k.recompute_y_couts, k.fuse_min_total, k.fuse_min_pixels)
        # (the split launches' pointwise GEMM reads the same planes: live under the pixel rule alone)
        x3 = k.use_x3 and b.name in t.x3_off and (six or h * w >= k.fuse_min_pixels or n * h * w >= k.fuse_min_total)
        fwd[b.name], vins[b.name] = BlockFwd(fused, keep_y, x3), v
        return bnrelu(b)

    v = ShapeView(L.VIEW_PLAIN, t.cpad)
    for _, b1, b2 in t.enc:
        v = block(b2, block(b1, v))
    v = block(t.bneck[1], block(t.bneck[0], v))
    nd = len(t.dec)
    for i, (stage, fi, cin, b1, b2) in enumerate(t.dec):
        skip = t.enc[nd - 1 - i][2]
        v = block(b2, block(b1, ShapeView(L.VIEW_CONCAT, fi, skip.cout, drop and i < nd - 1)))
    x3_live = frozenset(b.name for b in t.blocks if fwd[b.name].x3)
    segs = tuple(seg + (0,) for b, seg in t.x3_cand if b.name in x3_live) + (t.x3_mixed if six else ())
    plan = dict(training=training, batch_stats=training and k.use_bn, drop=drop, x6=six, overlap=k.overlap,
                sync_bn=k.sync_bn, fwd=fwd, x3_segs=segs, x3_live=x3_live)
    if not training:
        return StepPlan(bwd={}, head=HeadBwd(0, False), convt={}, **plan)

    # backward, in issue order: what each launch leaves for the block whose da it completes
    bwd: Dict[str, BlockBwd] = {}
    convt: Dict[str, ConvTBwd] = {}
    left: Dict[str, tuple] = {}  # block -> (BN partial slabs, they carry the dropout mask, da is rank one)
    producers = k.fuse_bn_stats and k.fuse_bn_bwd

    def block_bwd(b: Block, target=None, has_dx=True, drop_out=False, pooled=False):
        h, w = t.dims(b.level)
        vf = vins[b.name]  # the forward's view; the data gradient of a pooled input routes through the POOL view of z
        vin = ShapeView(L.VIEW_POOL_BNRELU, vf.c0) if pooled else vf
        r = bwd[b.name] = block_bwd_route(t, k, b, fwd[b.name], n, h, w, vin, vf, has_dx, target is not None,
                                          drop_out, *left.pop(b.name, (0, False, False)))
        if r.da_slabs:
            left[target.name] = (r.da_slabs, False, False)

    last = t.dec[-1][4]
    S = ops.head_bwd_bnstats_slabs(bnrelu(last), n, t.h, t.w, k.num_classes) if producers else 0
    # binary head feeding the fused block backward: da = dlogit (x) kernel stays rank one
    head = HeadBwd(S, S > 0 and k.num_classes == 1 and
                   _fused_bwd(k, last, fwd[last.name], False, vins[last.name]))
    if S:
        left[last.name] = (S, False, head.rank1)
    for i in reversed(range(nd)):
        stage, fi, cin, b1, b2 = t.dec[i]
        block_bwd(b2, target=b1)
        block_bwd(b1)
        prev = t.dec[i - 1][4] if i > 0 else t.bneck[1]
        h, w = t.dims(b1.level + 1)
        xv = ShapeView(L.VIEW_BNRELU, prev.cout, 0, i == 0 and drop)
        S = ops.conv_transpose2x2_bwd_data_bnstats_slabs(xv, n, h, w, fi) if producers else 0
        convt[stage] = ConvTBwd(S, S > 0 and xv.dropped)
        if S:
            left[prev.name] = (S, xv.dropped, False)
    block_bwd(t.bneck[1], target=t.bneck[0], drop_out=drop)
    block_bwd(t.bneck[0], target=t.enc[-1][2], pooled=True)
    for j in reversed(range(len(t.enc))):
        _, e1, e2 = t.enc[j]
        block_bwd(e2, target=e1)
        if j > 0:
            block_bwd(e1, target=t.enc[j - 1][2], pooled=True)
        else:
            block_bwd(e1, has_dx=False)
    return StepPlan(bwd=bwd, head=head, convt=convt, **plan)

