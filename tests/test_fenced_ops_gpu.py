"""Training ops inside guard bands (tests/fenced.py) at the edges the parity modules leave out:
reductions and BatchNorm finishes at row / column tails, every entry point that refuses a shape or a
misaligned operand (negative return, a message, nothing written), the scalar kernels behind the
`pointer % 16` predicates (operands 4 bytes past a 16-byte boundary, against the float64 oracle at
the aligned case's tolerance), and the engine under workspaces of exactly the queried size.

Every workspace here has exactly the bytes its `*_workspace()` query asked for and starts as 0xFF
bytes; every output starts as NaN; after each test no fence byte may have changed and no output
element may be left unwritten."""
import numpy as np
import pytest

import fenced
from helpers import TRACE_BATCH, TRACE_CONFIGS, TRACE_DEFAULTS, bn_affine, f32, host, rel_err, view_value
from oracle import keras_ops as K

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def ops():
    from unet_amd import ops as O
    return O


mem = None  # the running test's fenced.Arena, set by _fenced


@pytest.fixture(autouse=True)
def _fenced(ops):
    global mem
    mem = fenced.Arena("cuda")
    ws = fenced.FencedWorkspace("cuda")
    with ws.installed(ops):
        yield mem
        mem.check(extra=[ws])
    mem = None


def dev(a):
    return mem.inp(a)


def skew_if(t, yes):
    return mem.skewed(t) if yes else t


def refused(call, *untouched):
    """The call returns a negative status with a message (ops raises UnetHipError 'invalid argument'
    with unet_last_error's text) and leaves the given `mem.empty(..., output=False)` tensors alone."""
    from unet_amd._lib import UnetHipError
    with pytest.raises(UnetHipError, match=r"invalid argument\): \S"):
        call()
    for t in untouched:
        assert mem.is_untouched(t)


def test_arena_on_the_device(ops):
    """The allocator's own checks hold on device tensors (the overrun reports are proved on the CPU,
    test_fenced_host.py): poison is NaN / -1, an unwritten output is reported, a byte of a fence
    changed through the arena's own backing tensor (inside its allocation) is reported, skewed
    tensors sit 4 bytes past a 16-byte boundary, the workspace has exactly the bytes asked for."""
    own = fenced.Arena("cuda")
    out, cnt = own.empty((3, 5)), own.empty(4, dtype=torch.int64)
    assert out.is_cuda and bool(torch.isnan(out).all()) and bool((cnt == -1).all()) and out.data_ptr() % 256 == 0
    ops._check(out, "out", 15)
    with pytest.raises(AssertionError, match=r"out#1\[3, 5\]: output still holds 15 poison"):
        own.check()
    out.fill_(1.0)
    cnt.zero_()
    own.check()
    sk = own.skewed(out)
    assert sk.data_ptr() % 16 == 4 and torch.equal(sk, out)
    ops._check(sk, "skewed", 15)
    rec = own.bufs[0]
    rec.raw[rec.start + rec.nbytes + 8] = 0
    with pytest.raises(AssertionError, match=r"out#1\[3, 5\]: rear fence changed, first at byte offset 8 "):
        own.check()
    rec.raw[rec.start + rec.nbytes + 8] = 0xFF
    own.check()
    assert isinstance(ops.WORKSPACE, fenced.FencedWorkspace)
    ptr, nbytes = ops._ws(1000, "cuda")
    assert nbytes == 1000 and ptr.value % 256 == 0 and ops._ws(0, "cuda") == (None, 0)


# ------------------------------------------------------------------- reductions ---
@pytest.mark.parametrize("skew", [False, True])
@pytest.mark.parametrize("L", [1, 4, 7, 48, 68])
@pytest.mark.parametrize("S", [1, 127, 129, 300])  # 300 slabs of < 1024 quads: the in-place chunk level first
def test_reduce_slabs_tails(ops, S, L, skew):
    """unet_reduce_slabs = float64 column sums rounded once (2^-24 relative: 1e-6 holds with room);
    skew: the slabs 4 bytes past a 16-byte boundary take the scalar kernels."""
    rng = np.random.default_rng(S * 100 + L)
    slabs = f32(rng.standard_normal((S, L)))
    t = skew_if(mem.inp(slabs, fence=mem.out_fence), skew)  # scratch: the op may overwrite it
    out = mem.empty(L)
    ops.reduce_slabs(t, S, L, out)
    assert rel_err(host(out), slabs.sum(0)) < 1e-6


@pytest.mark.parametrize("n,h,w,c0,c1", [(1, 8, 512, 6, 2), (1, 3, 43, 34, 34)])
def test_dwconv_bwd_filter_concat_split_off_the_quads(ops, n, h, w, c0, c1):
    """unet_dwconv3x3_bwd_filter on a concat view with c0 % 4 != 0 and (c0 + c1) % 4 == 0: the scalar flat
    kernel under a workspace sized by the view-less query for c0 + c1 channels (here exactly that size, every
    byte 0xFF: NaN).  Its slabs stay inside it (6 + 2: the query sizes 4 slabs where the launch once wrote 16)
    and every channel is summed (34 + 34: two channel tiles of 64, not one of 17 quads), within
    test_dwconv_bwd's 1e-5 of float64."""
    rng = np.random.default_rng(n * h * w + c0)
    C = c0 + c1
    up, skip = f32(rng.standard_normal((n, h, w, c0))), f32(rng.standard_normal((n, h, w, c1)))
    sc, sh = bn_affine(rng, c1)
    dy = f32(rng.standard_normal((n, h, w, C)))
    v = ops.View.concat(dev(up), dev(skip), dev(sc), dev(sh))
    g = mem.empty((3, 3, C, 1))
    ops.dwconv3x3_bwd_filter(v, n, h, w, dev(dy), g)
    assert ops.WORKSPACE.sizes == [ops.L.query("unet_dwconv3x3_bwd_filter_workspace", n, h, w, C)]
    xv = view_value(3, up, None, None, skip, sc, sh, 0.0, 0)
    _, ddk = K.depthwise3x3_bwd(xv, np.zeros((3, 3, C, 1)), dy)
    assert rel_err(host(g), ddk) < 1e-5


@pytest.mark.parametrize("use_bn", [True, False])
@pytest.mark.parametrize("c", [4, 48, 68])
@pytest.mark.parametrize("m,S", [(1, 1), (127, 2), (129, 65)])  # 65 slabs: chunk rows + arrival counters
def test_bn_relu_bwd_stats_and_finish_tails(ops, m, S, c, use_bn):
    """unet_bn_relu_bwd_stats, and unet_bn_relu_bwd_stats_finish over host-made slabs of the same
    rows, against float64 sums (the tolerances of test_dwconv_bwd_data_bnstats) and each other."""
    rng = np.random.default_rng(m + 10 * c + use_bn)
    z = f32(rng.standard_normal((m, c)) * 2 + 0.3)
    da = f32(rng.standard_normal((m, c)))
    sc, sh = bn_affine(rng, c)
    mean, rstd = f32(rng.standard_normal(c) * 0.1), f32(1.0 + rng.random(c))
    g = np.where(z * sc + sh > 0, da, 0.0)
    xh = (z - mean) * rstd
    tm, tr = dev(mean), dev(rstd)
    mu, rs = (tm, tr) if use_bn else (None, None)
    numel = ops.bn_stats_partials_numel(S, c)
    part = np.zeros(numel)
    for s, rows in enumerate(np.array_split(np.arange(m), S)):
        part[s * 2 * c:s * 2 * c + c] = g[rows].sum(0)
        part[s * 2 * c + c:(s + 1) * 2 * c] = (g[rows] * xh[rows]).sum(0)
    tpart = mem.inp(part, fence=mem.out_fence)  # (the finish writes its chunk rows and counters)
    res = []
    for fused in (True, False):
        dg, db, coef = mem.zeros(c), mem.zeros(c), mem.empty(3 * c)
        if fused:
            ops.bn_relu_bwd_stats_finish(tpart, S, m, c, mu, rs, use_bn, dg if use_bn else None, db, coef)
            assert not torch.any(tpart[-((c + 63) // 64):].view(torch.int32))  # counters left zero
        else:
            ops.bn_relu_bwd_stats(dev(da), dev(z), m, c, mu, rs, dev(sc), dev(sh), use_bn, 0.0, 0,
                                  dg if use_bn else None, db, coef)
        res.append((host(dg), host(db), host(coef)))
    for x, y in zip(res[0], res[1]):
        assert rel_err(x, y) < 2e-5
    for r in res:
        assert rel_err(r[1], g.sum(0)) < 1e-5
        if use_bn:
            assert rel_err(r[0], (g * xh).sum(0)) < 1e-5


# -------------------------------------------------------------------- refusals ---
def test_refused_shapes_write_nothing(ops):
    """Shapes an entry point refuses (its `*_supported` query, a zero workspace answer or a zero slab
    count says so beforehand): negative return, a message, fences and outputs untouched."""
    sc64 = mem.full(64, 1.0)
    # fused sepconv forward: w % 16 != 0
    x = mem.zeros((1, 8, 8, 16))
    v = ops.View.plain(x)
    assert not ops.sepconv_supported(v, 1, 8, 8, 64)
    z = mem.empty((1, 8, 8, 64), output=False)
    refused(lambda: ops.sepconv_fwd(v, 1, 8, 8, mem.zeros(9 * 16), 64, mem.zeros(16 * 64), None, z), z)
    # fused filter gradients: 256 outputs; fused block backward: 128 outputs
    x64 = mem.zeros((1, 8, 16, 64))
    v64 = ops.View.bnrelu(x64, sc64, sc64)
    assert not ops.sepconv_bwd_filter_supported(v64, 1, 8, 16, 256)
    ddk, dpk = mem.empty(9 * 64, output=False), mem.empty(64 * 256, output=False)
    refused(lambda: ops.sepconv_bwd_filter(v64, 1, 8, 16, mem.zeros(9 * 64), mem.zeros(128 * 64), mem.zeros(128 * 256),
                                           256, ddk, dpk), ddk, dpk)
    dy, dpk2 = mem.empty((1, 8, 16, 64), output=False), mem.empty(64 * 128, output=False)
    refused(lambda: ops.sepconv_bwd_fused(v64, 1, 8, 16, mem.zeros(9 * 64), mem.zeros(64 * 128), mem.zeros(128 * 128),
                                          mem.zeros(128 * 128), mem.full(128, 1.0), mem.zeros(128), mem.zeros(3 * 128),
                                          128, dy, ddk, dpk2), dy, ddk, dpk2)
    # image-block gradients: 48 outputs (workspace answer 0)
    m, co = 128, 48
    assert ops.L.query("unet_pointwise_bwd_data_bnrelu_wgrad_workspace", m, 4, co) == 0
    assert ops.L.query("unet_image_block_bwd_wgrad_workspace", 1, 8, 16, co) == 0
    da, zz, pk, one, zero, coef, y = (mem.zeros((m, co)), mem.zeros((m, co)), mem.zeros(4 * co), mem.full(co, 1.0),
                                      mem.zeros(co), mem.zeros(3 * co), mem.zeros((m, 4)))
    dy4, dpk4 = mem.empty((m, 4), output=False), mem.empty(4 * co, output=False)
    refused(lambda: ops.pointwise_bwd_data_bnrelu_wgrad(da, zz, m, 4, co, pk, one, zero, coef, y, dy4, dpk4), dy4, dpk4)
    ddk3, dpk3 = mem.empty(9 * 3, output=False), mem.empty(3 * co, output=False)
    refused(lambda: ops.image_block_bwd_wgrad(mem.zeros((1, 8, 16, 4)), 1, 8, 16, 3, co, pk, one, zero, coef, da, zz, y,
                                              ddk3, dpk3), ddk3, dpk3)
    # ConvT data gradient with BN partials: cout % 4 != 0 (slab count 0)
    assert ops.conv_transpose2x2_bwd_data_bnstats_slabs(v64, 1, 8, 16, 17) == 0
    dx = mem.empty((1, 8, 16, 64), output=False)
    refused(lambda: ops.conv_transpose2x2_bwd_data_bnstats(v64, 1, 8, 16, 17, mem.zeros(4 * 17 * 64),
                                                           mem.zeros((1, 16, 32, 17)), dx, None, None, mem.zeros(0)), dx)
    # depthwise data gradient with BN partials: a concat view has no such path
    vc = ops.View.concat(x64, x64, sc64, sc64)
    assert ops.dwconv3x3_bwd_data_bnstats_slabs(vc, 1, 8, 16) == 0
    refused(lambda: ops.dwconv3x3_bwd_data_bnstats(vc, 1, 8, 16, mem.zeros(9 * 128), mem.zeros((1, 8, 16, 128)), dx,
                                                   None, None, mem.zeros(0)), dx)
    # head: 33 classes
    prob = mem.empty((1, 8, 16, 33), output=False)
    refused(lambda: ops.head_fwd(v64, 1, 8, 16, 33, mem.zeros(64 * 33), mem.zeros(33), prob), prob)


def _planes(ops, w2d, keep):
    rows, cols = w2d.shape
    t = mem.empty(3 * rows * cols, dtype=torch.int16)
    ops.split_x3(dev(f32(w2d)), [(0, rows, cols, 0)], t, keep=keep)
    return t


def test_refused_misaligned_operands_write_nothing(ops):
    """Entry points whose kernels have float4 accesses only: an operand 4 bytes past a 16-byte
    boundary is refused before any launch."""
    rng = np.random.default_rng(3)
    n, h, w, C, co = 1, 8, 16, 64, 64
    m = n * h * w
    r = lambda *s: f32(rng.standard_normal(s))  # noqa: E731
    sc, sh = bn_affine(rng, C)
    x, tsc, tsh = dev(r(n, h, w, C)), dev(sc), dev(sh)
    v = ops.View.bnrelu(x, tsc, tsh)
    dk, pk, z, da, dyi, coef = dev(r(9 * C)), dev(r(C * co)), dev(r(m, co)), dev(r(m, co)), dev(r(m, C)), dev(r(3 * co))
    # image block (cin 4): the data + weight gradient and the two-weight-gradient launch
    da4, z4, pk4, y4, x4 = dev(r(m, 64)), dev(r(m, 64)), dev(r(4 * 64)), dev(r(m, 4)), dev(r(n, h, w, 4))
    dy4, dpk4 = mem.empty((m, 4), output=False), mem.empty(4 * 64, output=False)
    refused(lambda: ops.pointwise_bwd_data_bnrelu_wgrad(mem.skewed(da4), z4, m, 4, 64, pk4, tsc, tsh, coef, y4, dy4, dpk4),
            dy4, dpk4)
    ddk3, dpk3 = mem.empty(9 * 3, output=False), mem.empty(3 * 64, output=False)
    refused(lambda: ops.image_block_bwd_wgrad(mem.skewed(x4), n, h, w, 3, 64, pk4, tsc, tsh, coef, da4, z4, y4, ddk3, dpk3),
            ddk3, dpk3)
    # fused filter gradients / fused block backward
    ddk, dpk, dy = mem.empty(9 * C, output=False), mem.empty(C * co, output=False), mem.empty((n, h, w, C), output=False)
    refused(lambda: ops.sepconv_bwd_filter(v, n, h, w, dk, mem.skewed(dyi), z, co, ddk, dpk), ddk, dpk)
    refused(lambda: ops.sepconv_bwd_filter(ops.View.bnrelu(mem.skewed(x), tsc, tsh), n, h, w, dk, dyi, z, co, ddk, dpk),
            ddk, dpk)
    refused(lambda: ops.sepconv_bwd_fused(v, n, h, w, dk, pk, da, mem.skewed(z), tsc, tsh, coef, co, dy, ddk, dpk),
            dy, ddk, dpk)
    # pooling selection, alone and as the fused forward's epilogue; split-precision planes
    sel = mem.empty((n, h // 2, w // 2, co), output=False)
    refused(lambda: ops.pool_select(mem.skewed(z), n, h, w, co, None, sel), sel)
    refused(lambda: ops.pool_select(z, n, h, w, co, None, mem.skewed(sel)))
    zo = mem.empty((n, h, w, co), output=False)
    for sch in (ops.SEPCONV_AUTO, ops.SEPCONV_TILE):
        old = ops.sepconv_set_schedule(sch)
        try:
            refused(lambda: ops.sepconv_fwd(v, n, h, w, dk, co, pk, None, zo, None, mem.skewed(sel), None), zo)
        finally:
            ops.sepconv_set_schedule(old)
    pkx = mem.skewed(_planes(ops, host(pk).reshape(C, co), keep=False))
    refused(lambda: ops.sepconv_fwd(v, n, h, w, dk, co, pk, None, zo, None, None, None, pkx=pkx), zo)
    refused(lambda: ops.pointwise_fwd(dyi, m, C, co, pk, zo, None, pkx=pkx), zo)  # check_planes
    # BatchNorm-backward data gradient: z (the float4 dz formation), and da (the vectorised GEMM only)
    dy2, dz2 = mem.empty((m, C), output=False), mem.empty((m, co), output=False)
    refused(lambda: ops.pointwise_bwd_data_bnrelu(da, mem.skewed(z), m, C, co, pk, tsc, tsh, coef, 0.0, 0, dy2, dz2),
            dy2, dz2)
    refused(lambda: ops.pointwise_bwd_data_bnrelu(mem.skewed(da), z, m, C, co, pk, tsc, tsh, coef, 0.0, 0, dy2, dz2),
            dy2, dz2)
    # depthwise data gradient that also writes filter-gradient slabs
    S = ops.dwconv3x3_bwd_data_bnstats_slabs(v, n, h, w)
    part = mem.zeros(ops.bn_stats_partials_numel(S, C))
    dwp = mem.skewed(mem.empty(S * 9 * C, output=False))
    refused(lambda: ops.dwconv3x3_bwd_data_bnstats_dwf(v, n, h, w, dk, dyi, dy, None, None, part, dwp), dy, dwp)
    assert not part.any()


# ------------------------------------------------- skewed operands, scalar kernels ---
M, CIN, COUT = 129, 64, 68  # a ragged row tile, one float4 past 64 columns


@pytest.mark.parametrize("stats", [True, False])
@pytest.mark.parametrize("which", ["y", "pk"])
def test_pointwise_fwd_skewed(ops, which, stats):
    rng = np.random.default_rng(41)
    y, pk = f32(rng.standard_normal((M, CIN))), f32(rng.standard_normal((CIN, COUT)) / np.sqrt(CIN))
    z = mem.empty((M, COUT))
    part = mem.zeros(ops.bn_partials_numel(M, COUT)) if stats else None
    ops.pointwise_fwd(skew_if(dev(y), which == "y"), M, CIN, COUT, skew_if(dev(pk), which == "pk"), z, part)
    assert rel_err(host(z), y @ pk) < 5e-6
    if stats:
        outs = [mem.empty(COUT) for _ in range(4)]
        gamma, beta = bn_affine(rng, COUT)
        ops.bn_finalize(part, M, COUT, dev(gamma), dev(beta), 1e-3, 0.99, None, None, False, *outs)
        _, mean, var = K.bn_train((y @ pk).reshape(M, 1, 1, COUT), gamma, beta)
        assert rel_err(host(outs[0]), mean) < 1e-4
        assert rel_err(host(outs[1]), 1 / np.sqrt(var + 1e-3)) < 1e-5


@pytest.mark.parametrize("which", ["dz", "pk"])
def test_pointwise_bwd_data_skewed(ops, which):
    rng = np.random.default_rng(42)
    dz, pk = f32(rng.standard_normal((M, COUT))), f32(rng.standard_normal((CIN, COUT)) / np.sqrt(CIN))
    dy = mem.empty((M, CIN))
    ops.pointwise_bwd_data(skew_if(dev(dz), which == "dz"), M, CIN, COUT, skew_if(dev(pk), which == "pk"), dy)
    assert rel_err(host(dy), dz @ pk.T) < 5e-6


@pytest.mark.parametrize("m", [M, 1033])  # 1033: two row slices, the last one ragged
@pytest.mark.parametrize("which", ["y", "dz"])
def test_pointwise_bwd_filter_skewed(ops, which, m):
    rng = np.random.default_rng(43 + m)
    y, dz = f32(rng.standard_normal((m, CIN))), f32(rng.standard_normal((m, COUT)))
    dpk, ref = mem.empty((CIN, COUT)), mem.empty((CIN, COUT))
    ops.pointwise_bwd_filter(skew_if(dev(y), which == "y"), skew_if(dev(dz), which == "dz"), m, CIN, COUT, dpk)
    ops.pointwise_bwd_filter(dev(y), dev(dz), m, CIN, COUT, ref)
    assert rel_err(host(dpk), y.T @ dz) < 5e-6
    assert rel_err(host(dpk), host(ref)) < 5e-6  # the vectorised kernel's answer


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("which", ["src0", "k", "dout"])
def test_conv_transpose_skewed(ops, which, mode):
    """ConvT forward, data gradient and kernel + bias gradients with one operand skewed: the scalar
    rows / weight-gradient kernels and the separate column-sum bias route, against the oracle and
    the aligned launch (fused-bias route)."""
    rng = np.random.default_rng(44 + mode)
    n, h, w, cin, cout = 1, 3, 43, 64, 17 if which == "k" else 16  # 129 pixels; 68 or 64 GEMM columns
    x = f32(rng.standard_normal((n, h, w, cin)))
    sc, sh = bn_affine(rng, cin)
    xv = view_value(mode, x, sc, sh)
    k, b = f32(rng.standard_normal((2, 2, cout, cin)) / np.sqrt(cin)), f32(rng.standard_normal(cout))
    dout = f32(rng.standard_normal((n, 2 * h, 2 * w, cout)))

    def view(skew):
        t = skew_if(dev(x), skew)
        return ops.View.plain(t) if mode == 0 else ops.View.bnrelu(t, dev(sc), dev(sh))
    v, tk, td = view(which == "src0"), skew_if(dev(k), which == "k"), skew_if(dev(dout), which == "dout")
    out = mem.empty((n, 2 * h, 2 * w, cout))
    ops.conv_transpose2x2_fwd(v, n, h, w, cout, tk, dev(b), out)
    assert rel_err(host(out), K.conv_transpose2x2(xv, k, b)) < 5e-6
    dx, dk, db = mem.empty((n, h, w, cin)), mem.empty((2, 2, cout, cin)), mem.empty(cout)
    ops.conv_transpose2x2_bwd(v, n, h, w, cout, tk, td, dx, dk, db)
    rdx, rdk, rdb = K.conv_transpose2x2_bwd(xv, k, dout)
    assert rel_err(host(dx), rdx) < 5e-6
    assert rel_err(host(dk), rdk) < 5e-6
    assert rel_err(host(db), rdb) < 5e-6
    dk2, db2 = mem.empty((2, 2, cout, cin)), mem.empty(cout)
    ops.conv_transpose2x2_bwd(view(False), n, h, w, cout, dev(k), dev(dout), None, dk2, db2)
    assert rel_err(host(dk), host(dk2)) < 5e-6 and rel_err(host(db), host(db2)) < 5e-6


@pytest.mark.parametrize("count,which", [(1027, None), (1024, "p"), (1024, "g"), (1024, "m"), (1024, "v")])
def test_adamw_skewed(ops, count, which):
    rng = np.random.default_rng(5 + count)
    p, g = f32(rng.standard_normal(count)), f32(rng.standard_normal(count) * 0.1)
    m, v = f32(rng.standard_normal(count) * 0.01), f32(rng.random(count) * 0.01)
    big = mem.out_fence  # p, m and v are updated in place
    tp, tg = skew_if(mem.inp(p, fence=big), which == "p"), skew_if(dev(g), which == "g")
    tm, tv = skew_if(mem.inp(m, fence=big), which == "m"), skew_if(mem.inp(v, fence=big), which == "v")
    step, lr, wd = 3, 2e-3, 1e-4
    alpha = lr * np.sqrt(1 - 0.999 ** step) / (1 - 0.9 ** step)
    ops.adamw_step(tp, tg, tm, tv, lr, wd, 0.9, 0.999, 1e-7, alpha, 0.5)
    rp, rm, rv = K.adamw_update(p, g * 0.5, m, v, step, lr, wd)
    assert rel_err(host(tp), rp) < 1e-6
    assert rel_err(host(tm), rm) < 1e-6
    assert rel_err(host(tv), rv) < 1e-6


@pytest.mark.parametrize("which", ["dst", "src"])
@pytest.mark.parametrize("rows", [1, 127, 129])
def test_copy_strided_pad4_skewed(ops, rows, which):
    """Channel padding 3 -> 4: a destination off the 16-byte grid takes the element kernel; pad
    channel untouched, bit-exact."""
    x = f32(np.random.default_rng(rows).standard_normal((rows, 3)))
    tx = skew_if(dev(x), which == "src")
    xp = skew_if(mem.full((rows, 4), 7.0), which == "dst")
    ops.copy_strided(tx, rows, 3, 3, xp, 4)
    assert torch.equal(xp[:, :3], tx) and bool((xp[:, 3] == 7.0).all())


@pytest.mark.parametrize("c0", [16, 64])
@pytest.mark.parametrize("ncls", [1, 3])
@pytest.mark.parametrize("mode", [0, 1])
def test_head_fwd_skewed_src(ops, mode, ncls, c0):
    """Head forward with its input 4 bytes past a 16-byte boundary: the general kernels, which then
    read the rows element by element."""
    rng = np.random.default_rng(c0 + ncls + mode)
    n, h, w = 1, 3, 43
    x = f32(rng.standard_normal((n, h, w, c0)))
    sc, sh = bn_affine(rng, c0)
    t = mem.skewed(dev(x))
    v = ops.View.plain(t) if mode == 0 else ops.View.bnrelu(t, dev(sc), dev(sh))
    k, b = f32(rng.standard_normal((1, 1, c0, ncls)) * 0.2), f32(rng.standard_normal(ncls) * 0.1)
    prob = mem.empty((n, h, w, ncls))
    ops.head_fwd(v, n, h, w, ncls, dev(k), dev(b), prob)
    assert rel_err(host(prob), K.head(view_value(mode, x, sc, sh), k, b, ncls)) < 2e-6


@pytest.mark.parametrize("which", ["prob", "y_true"])
@pytest.mark.parametrize("ncls", [1, 3, 21])
def test_head_bwd_skewed(ops, ncls, which):
    rng = np.random.default_rng(ncls)
    n, h, w, cin = 1, 3, 43, 64
    x = f32(rng.standard_normal((n, h, w, cin)))
    sc, sh = bn_affine(rng, cin)
    v = ops.View.bnrelu(dev(x), dev(sc), dev(sh))
    xv = view_value(1, x, sc, sh)
    k, b = f32(rng.standard_normal((1, 1, cin, ncls)) * 0.2), f32(rng.standard_normal(ncls) * 0.1)
    pp = f32(K.head(xv, k, b, ncls))
    yt = (rng.random((n, h, w, 1)) > 0.5).astype(np.float64) if ncls == 1 else np.eye(ncls)[rng.integers(0, ncls, (n, h, w))]
    prob, ytd = skew_if(dev(pp), which == "prob"), skew_if(dev(yt), which == "y_true")
    sums, res = mem.empty(n * ncls * 3), mem.empty(3)
    ops.dice_fwd(ytd, prob, n, h * w, ncls, 1e-7, sums, res)
    assert abs(host(res)[0] - K.dice_loss(yt, pp)) < 1e-6
    dx, dk, db = mem.empty((n, h, w, cin)), mem.empty((1, 1, cin, ncls)), mem.empty(ncls)
    ops.head_bwd(v, n, h, w, ncls, dev(k), prob, ytd, sums, 1e-7, 0, dx, dk, db)
    rdx, rdk, rdb = K.head_bwd(xv, k, pp, K.dice_loss_grad(yt, pp), ncls)
    assert rel_err(host(dx), rdx) < 1e-4
    assert rel_err(host(dk), rdk) < 1e-4
    assert rel_err(host(db), rdb) < 1e-4


# ------------------------------------------------------- the engine, exact workspaces ---
@pytest.mark.parametrize("cid", ["A", "L"])
def test_engine_under_exact_workspaces(ops, cid):
    """Two train steps and a predict with every workspace fenced, poisoned and of exactly the queried
    size, against an identically seeded model under the shared arena: loss, probabilities and all
    parameters bitwise equal (deterministic reductions; workspace contents and size do not matter)."""
    from unet_amd.model import UNetModel
    from unet_amd.optim import AdamW
    size, ncls, bn, drop, attrs = TRACE_CONFIGS[cid]
    rng = np.random.default_rng(7)
    x = rng.random((TRACE_BATCH,) + size, dtype=np.float32)
    y = (rng.random((TRACE_BATCH,) + size[:2] + (ncls,)) > 0.6).astype(np.float32)

    def run(workspace):
        model = UNetModel(size, ncls, dropout_rate=drop, use_batch_norm=bn, device="cuda:0")
        for k, v in {**TRACE_DEFAULTS, **attrs}.items():
            setattr(model.engine, k, v)
        model.compile(AdamW(learning_rate=2e-3, weight_decay=1e-4), "dice_loss")
        old, ops.WORKSPACE = ops.WORKSPACE, workspace
        try:
            tx, ty = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
            losses = [model.train_step(tx, ty).clone() for _ in range(2)]
            prob = model.engine.predict(tx).clone()
            torch.cuda.synchronize()
        finally:
            ops.WORKSPACE = old
        return losses, prob, model.engine.params.clone(), model.engine.stats.clone()

    ws = fenced.FencedWorkspace("cuda")
    got = run(ws)
    want = run(ops._Workspace())
    assert len(ws.bufs) > 0
    ws.check()
    for a, b in zip(got[0], want[0]):
        assert torch.equal(a, b)
    assert torch.equal(got[1], want[1])
    assert torch.equal(got[2], want[2]) and torch.equal(got[3], want[3])
    assert bool(torch.isfinite(got[1]).all()) and bool(torch.isfinite(got[2]).all())
