"""The kernels on the data that noise never produces, op by op against the float64 oracle
(oracle/keras_ops.py): exact ties in a 2x2 pool window at a positive value, channels that are exactly
constant or sit on a large offset, pre-activations that are exactly +-0, masks that are empty or full, classes
that are absent, heads that saturate.  Decoded images with flat backgrounds and blob masks produce all of
them (helpers.poster_batch / blob_masks, tests/test_structured_data_host.py); every other GPU test draws noise.

  a. pool-gradient routing under ties: MaxPoolGrad sends a window's gradient to its FIRST maximum in
     row-major order.  Weight gradients cannot see the tie-break (test_structured_data_host.py), so dx itself is
     compared, on every route of csrc/dw_plan.h, with and without the BN-backward statistics.
  b. same input, same output: a view that is constant over the pixels gives bitwise equal output pixels
     (one pixel in from the border).  This is what makes ties on the device coincide with ties in the oracle.
  c. BatchNorm statistics of constant and of offset channels from every producer of (mean, M2) partials.
  d. ReLU at exactly zero: the gradient there is 0 (mask `> 0`, never `>= 0`).
  e. loss and head edges: empty / full masks, an absent class, saturated logits.

Reference: model/u_net.py:14-25, 69, 105-112; utils/loss.py, utils/metrics.py."""
import itertools

import numpy as np
import pytest

import fenced
from helpers import blob_masks, bn_affine, f32, host, norm_err, rel_err
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
    """Every allocation of a test goes through `mem`; workspaces have exactly the queried size.
    After the body: no fence byte changed and every `mem.empty` output was written in full."""
    global mem
    mem = fenced.Arena("cuda")
    ws = fenced.FencedWorkspace("cuda")
    with ws.installed(ops):
        yield mem
        mem.check(extra=[ws])
    mem = None


def dev(a):
    return mem.inp(a)


class _schedule:
    """`with _schedule(ops, s):` runs sepconv_fwd under kernel schedule s."""

    def __init__(self, ops, schedule):
        self.ops, self.schedule = ops, schedule

    def __enter__(self):
        self.old = self.ops.sepconv_set_schedule(self.schedule)

    def __exit__(self, *exc):
        self.ops.sepconv_set_schedule(self.old)
        return False


def _sep_variants(ops):
    """name -> (schedule, split planes?) of every forward kernel of the fused separable conv at 64 / 128
    channels: the LDS-A-tile kernel, the register-A kernel in fp32 and in split precision (one tile per
    block), and the persistent split-precision kernel."""
    return {"tile": (ops.SEPCONV_TILE, False), "rk": (ops.SEPCONV_AUTO, False), "rk_x6": (ops.SEPCONV_RK1, True),
            "px": (ops.SEPCONV_RK, True)}


def _split(ops, pk, cin, cout):
    pkx = mem.empty(3 * cin * cout, dtype=torch.int16)
    ops.split_x3(pk, [(0, cin, cout, 0)], pkx)
    return pkx


# ------------------------------------------------------------------ a. ties in a pool window -----
TIE_SETS = [s for r in (2, 3, 4) for s in itertools.combinations(range(4), r)]  # 6 pairs, 4 triples, all four
N_PATTERNS = 2 * len(TIE_SETS) + 2


def _tie_affine(rng, c):
    """(scale, shift) of both signs: |scale| in [0.5, 1.5], every third channel negative, channels 0 and 1
    scale +0 and -0 (the activation is relu(shift) everywhere: one positive, one clipped); |shift| < 0.4."""
    sc = rng.uniform(0.5, 1.5, c)
    sc[2::3] *= -1.0
    sh = rng.uniform(-0.4, 0.4, c)
    sc[0], sc[1] = 0.0, -0.0
    sh[0], sh[1] = 0.3, -0.3
    return f32(sc), f32(sh)


def _tied_source(rng, n, h, w, sc):
    """The (n, 2h, 2w, c) source z of a max-pool view whose windows hold, in turn over the windows of every
    channel: each TIE_SETS pattern tied as the maximum of relu(fma(z, sc, sh)) at a positive value with the
    others lower; each pattern with all four clipped to 0 (the gradient lands on element 0); two windows
    without a tie.  The levels are exact in float32 and |level * sc| >= 0.25 apart, so equal z give equal
    activations and nothing else does.  With a negative scale the tie lives in the activation, not in z:
    the levels are mirrored (tied elements are the MINIMUM of z)."""
    c = sc.shape[0]
    lev = np.empty((n, h, w, c, 4))
    pid = (np.arange(n * h * w).reshape(n, h, w, 1) + 5 * np.arange(c)) % N_PATTERNS
    assert n * h * w >= N_PATTERNS
    for p in range(N_PATTERNS):
        sel = pid == p
        k = int(sel.sum())
        if p < len(TIE_SETS):  # tied at 2 |sc| + sh >= 0.6, the others at most |sc| + sh
            v = rng.choice([1.0, 0.5, -0.5, -1.0], (k, 4))
            v[:, TIE_SETS[p]] = 2.0
        elif p < 2 * len(TIE_SETS):  # all clipped: -|sc| + sh <= -0.1
            v = rng.choice([-1.5, -2.0, -3.0], (k, 4))
            v[:, TIE_SETS[p - len(TIE_SETS)]] = -1.0
        else:
            v = rng.standard_normal((k, 4)) * 2
        lev[sel] = v
    lev *= np.where(sc < 0, -1.0, 1.0)[:, None]
    return f32(lev.reshape(n, h, w, c, 2, 2).transpose(0, 1, 4, 2, 5, 3).reshape(n, 2 * h, 2 * w, c))


def _tie_census(act):
    """(windows with a positive tie, of those: first element not a maximum, windows all clipped)."""
    N, H, W, C = act.shape
    win = act.reshape(N, H // 2, 2, W // 2, 2, C).transpose(0, 1, 3, 5, 2, 4).reshape(-1, 4)
    mx = win.max(1)
    tie = ((win == mx[:, None]).sum(1) > 1) & (mx > 0)
    return int(tie.sum()), int((tie & (win[:, 0] < mx)).sum()), int((mx == 0).sum())


# (n, h, w, c) of the pooled view, route of csrc/dw_plan.h, tiles of the tiled route
TIE_CASES = [
    (2, 9, 17, 64, "tiled", 2 * 2 * 2),   # 16 quads x 16 columns: ragged tiles in both directions
    (3, 9, 5, 16, "tiled", 3 * 2 * 1),    # 4 quads x 64 columns
    (1, 5, 7, 8, "tiled", 1),             # 2 quads: one tile
    (2, 5, 7, 12, "flat_vec", 0),         # whole quads off the tiled widths
    (1, 3, 9, 20, "flat_vec", 0),
    (2, 5, 7, 10, "flat_scalar", 0),      # c % 4 != 0
    (1, 6, 5, 3, "flat_scalar", 0),
]


@pytest.mark.parametrize("use_bn", [True, False])
@pytest.mark.parametrize("n,h,w,c,route,tiles", TIE_CASES)
def test_pool_gradient_routing_under_ties(ops, n, h, w, c, route, tiles, use_bn):
    """dx0 of the max-pool view against init + K.maxpool2_bwd(act, dxv) (first maximum) within
    test_dwconv_bwd's 2e-6; bitwise equal between the plain and the statistics launch; the BN-backward
    statistics of the latter against float64 within test_dwconv_bwd_data_bnstats's 1e-5."""
    rng = np.random.default_rng(n * 1000 + h * 10 + w + c)
    sc, sh = _tie_affine(rng, c)
    z = _tied_source(rng, n, h, w, sc)
    act = K.relu(z * sc + sh)
    ties, first_loses, clipped = _tie_census(act)
    cycles = (n * h * w // N_PATTERNS) * (c - 2)  # every pattern at least this often (channels 0, 1: scale +-0)
    assert ties >= 11 * cycles and first_loses >= 4 * cycles and clipped >= 11 * cycles
    v = ops.View.pool_bnrelu(dev(z), dev(sc), dev(sh))
    S = ops.dwconv3x3_bwd_data_bnstats_slabs(v, n, h, w)
    assert S == tiles and (route == "tiled") == (S > 0) and (route == "flat_scalar") == (c % 4 != 0)
    dk = f32(rng.standard_normal((3, 3, c, 1)))
    dy = f32(rng.standard_normal((n, h, w, c)))
    init = f32(rng.standard_normal((n, 2 * h, 2 * w, c)))
    dxv, _ = K.depthwise3x3_bwd(K.maxpool2(act), dk, dy)
    ref = init + K.maxpool2_bwd(act, dxv)
    dx_p = mem.inp(init, fence=mem.out_fence)  # the pool route accumulates into dx0
    ops.dwconv3x3_bwd_data(v, n, h, w, dev(dk), dev(dy), dx_p)
    assert rel_err(host(dx_p), ref) < 2e-6
    # (what a last-maximum routing would give is far outside the gate: the test can see the tie-break)
    last = init + K.maxpool2_bwd(act[:, ::-1, ::-1], dxv[:, ::-1, ::-1])[:, ::-1, ::-1]
    assert rel_err(last, ref) > 1e-2
    if route != "tiled":
        return
    mean = dev(f32(rng.standard_normal(c) * 0.1))
    rstd = dev(f32(1.0 + rng.random(c)))
    mu, rs = (mean, rstd) if use_bn else (None, None)
    part = mem.zeros(ops.bn_stats_partials_numel(S, c))
    dx_f = mem.inp(init, fence=mem.out_fence)
    ops.dwconv3x3_bwd_data_bnstats(v, n, h, w, dev(dk), dev(dy), dx_f, mu, rs, part)
    assert torch.equal(dx_f, dx_p)
    m = n * 4 * h * w
    dg, db, coef = mem.zeros(c), mem.zeros(c), mem.empty(3 * c)
    ops.bn_relu_bwd_stats_finish(part, S, m, c, mean, rstd, use_bn, dg if use_bn else None, db, coef)
    da = host(dx_p).reshape(-1, c)
    zz = z.reshape(-1, c)
    g = np.where(zz * sc + sh > 0, da, 0.0)
    assert rel_err(host(db), g.sum(0)) < 1e-5
    if use_bn:
        xh = (zz - host(mean)) * host(rstd)
        assert rel_err(host(dg), (g * xh).sum(0)) < 1e-5


def _pool_of_view(z, sc, sh):
    """relu(fma(z, sc, sh)) pooled 2x2 on the device, as the views evaluate it (test_pool_select)."""
    n, h, w, c = z.shape
    return torch.relu(torch.addcmul(sh, z, sc)).reshape(n, h // 2, 2, w // 2, 2, c).amax((2, 4))


@pytest.mark.parametrize("n,h,w,c", [(2, 5, 7, 64), (1, 6, 5, 10), (3, 9, 5, 3), (1, 5, 7, 8)])
def test_pool_select_under_ties(ops, n, h, w, c):
    """unet_pool_select on the tied source: a BN+ReLU view of the selection is bitwise the pool of the view,
    for scales of both signs and +-0 (gamma carries the sign) and without BatchNorm."""
    rng = np.random.default_rng(n + h + c)
    sc, sh = _tie_affine(rng, c)
    z = _tied_source(rng, n, h, w, sc)
    out = mem.empty((n, h, w, c))
    for gamma, scale in ((sc, sc), (None, np.ones(c))):
        ops.pool_select(dev(z), n, 2 * h, 2 * w, c, None if gamma is None else dev(gamma), out)
        tsc, tsh = dev(scale), dev(sh)
        assert torch.equal(torch.relu(torch.addcmul(tsh, out, tsc)), _pool_of_view(dev(z), tsc, tsh))
        sel = host(out)  # and it is one of the window's own elements
        win = z.reshape(n, h, 2, w, 2, c)
        assert ((win == sel[:, :, None, :, None, :]).any((2, 4))).all()


@pytest.mark.parametrize("variant", ["tile", "rk", "rk_x6", "px"])
@pytest.mark.parametrize("cout", [64, 128])
def test_sepconv_pool_selection_epilogue_under_ties(ops, variant, cout):
    """The fused z_pool_sel epilogues (the separate pass after the LDS-A-tile kernel, the register-A
    epilogue in fp32 and split precision, the persistent kernel) on a z that holds the tie patterns: a
    centre-tap depthwise kernel of ones and a pointwise kernel that copies channel j % 64 to output j pass
    the tied input through.  zsel is bitwise unet_pool_select of the kernel's own z, and its BN+ReLU view
    is bitwise the pool of the view of z."""
    n, h, w, cin = 2, 8, 16, 64
    rng = np.random.default_rng(cout)
    sc, sh = _tie_affine(rng, cout)
    sc[cin:] = sc[:cout - cin]  # (output j carries input j % 64's tie pattern: the same sign there)
    x = _tied_source(rng, n, h // 2, w // 2, sc[:cin])
    dk = np.zeros((3, 3, cin, 1))
    dk[1, 1] = 1.0
    pk = np.zeros((1, 1, cin, cout))
    pk[0, 0, np.arange(cout) % cin, np.arange(cout)] = 1.0
    schedule, split = _sep_variants(ops)[variant]
    tpk = dev(pk)
    pkx = _split(ops, tpk, cin, cout) if split else None
    gamma = dev(sc)
    z = mem.empty((n, h, w, cout))
    zsel = mem.full((n, h // 2, w // 2, cout), 7.0)
    with _schedule(ops, schedule):
        ops.sepconv_fwd(ops.View.plain(dev(x)), n, h, w, dev(dk), cout, tpk, None, z, None, zsel, gamma, pkx=pkx)
    want = np.concatenate([x, x], -1)[..., :cout]
    assert _tie_census(K.relu(host(z) * sc + sh))[:2] == _tie_census(K.relu(want * sc + sh))[:2]
    ref = mem.empty(zsel.shape)
    ops.pool_select(z, n, h, w, cout, gamma, ref)
    assert torch.equal(zsel, ref)
    tsh = dev(sh)
    assert torch.equal(torch.relu(torch.addcmul(tsh, zsel, gamma)), _pool_of_view(z, gamma, tsh))


# ------------------------------------------------------------ b. same input, same output -----
def _const_rows(rng, c):
    """A non-trivial value per channel (both signs, no round numbers)."""
    return f32(rng.uniform(0.3, 1.7, c) * rng.choice([-1.0, 1.0], c))


def _assert_pixels_equal(out, what):
    """Every pixel of `out` (..., c) holds bitwise the same channel vector."""
    flat = out.reshape(-1, out.shape[-1])
    bad = (flat != flat[0]).any(1)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {flat.shape[0]} pixels differ from pixel 0, first {int(bad.nonzero()[0])}"


@pytest.mark.parametrize("n,h,w,c", [(1, 9, 21, 64), (2, 10, 70, 16), (1, 9, 21, 12), (1, 9, 21, 10), (2, 7, 9, 3)])
def test_constant_view_dwconv_fwd(ops, n, h, w, c):
    """dwconv3x3_fwd on the tiled, flat vector and flat scalar routes."""
    rng = np.random.default_rng(c)
    x = np.broadcast_to(_const_rows(rng, c), (n, h, w, c))
    y = mem.empty((n, h, w, c))
    ops.dwconv3x3_fwd(ops.View.plain(dev(x)), n, h, w, dev(f32(rng.standard_normal((3, 3, c, 1)))), y)
    _assert_pixels_equal(y[:, 1:-1, 1:-1], "dwconv3x3_fwd")


# the persistent kernel: 513 tiles of 8 x 16 pixels over 512 block slots = runs of 2 tiles, the last block one
PX_RAGGED = (1, 216, 304)


@pytest.mark.parametrize("variant,n,h,w,cin,cout", [("tile", 2, 16, 32, 16, 64), ("tile", 2, 16, 32, 64, 64),
                                                     ("rk", 2, 16, 32, 64, 128), ("rk_x6", 2, 16, 32, 64, 64),
                                                     ("rk_x6", 1, 16, 32, 128, 256), ("px", 2, 16, 32, 64, 128),
                                                     ("px",) + PX_RAGGED + (64, 64)])
def test_constant_view_sepconv_fwd(ops, variant, n, h, w, cin, cout):
    """sepconv_fwd in both schedules, in split precision and persistent (a ragged last run of tiles, more
    than one tile per block): y and z."""
    rng = np.random.default_rng(cin + cout)
    x = np.broadcast_to(_const_rows(rng, cin), (n, h, w, cin))
    dk = dev(f32(rng.standard_normal((3, 3, cin, 1))))
    pk = dev(f32(rng.standard_normal((1, 1, cin, cout)) / np.sqrt(cin)))
    schedule, split = _sep_variants(ops)[variant]
    pkx = _split(ops, pk, cin, cout) if split else None
    y, z = mem.empty((n, h, w, cin)), mem.empty((n, h, w, cout))
    part = mem.zeros(ops.bn_partials_numel(n * h * w, cout))
    with _schedule(ops, schedule):
        ops.sepconv_fwd(ops.View.plain(dev(x)), n, h, w, dk, cout, pk, y, z, part, pkx=pkx)
    _assert_pixels_equal(y[:, 1:-1, 1:-1], f"sepconv_fwd[{variant}] y")
    _assert_pixels_equal(z[:, 1:-1, 1:-1], f"sepconv_fwd[{variant}] z")


@pytest.mark.parametrize("m,cin,cout,split", [(129, 64, 64, False), (300, 64, 128, False), (300, 32, 96, False),
                                              (129, 64, 64, True), (300, 64, 128, True),
                                              (129, 4, 64, False), (300, 4, 32, False)])  # cin 4: the image block
def test_constant_view_pointwise_fwd(ops, m, cin, cout, split):
    """pointwise_fwd (rows GEMM, fp32 and split precision, and the image block's 4-channel one) at row
    counts with a tail tile."""
    rng = np.random.default_rng(m + cin + cout)
    y = np.broadcast_to(_const_rows(rng, cin), (m, cin))
    pk = dev(f32(rng.standard_normal((1, 1, cin, cout)) / np.sqrt(cin)))
    z = mem.empty((m, cout))
    part = mem.zeros(ops.bn_partials_numel(m, cout))
    ops.pointwise_fwd(dev(y), m, cin, cout, pk, z, part, pkx=_split(ops, pk, cin, cout) if split else None)
    _assert_pixels_equal(z, "pointwise_fwd")


def test_constant_view_image_block_fwd(ops):
    """The image block forward: the 3-channel image padded to 4, depthwise, then the 4 -> 64 pointwise."""
    n, h, w, cout = 2, 16, 32, 64
    rng = np.random.default_rng(3)
    x = np.zeros((n, h, w, 4))
    x[..., :3] = _const_rows(rng, 3)
    dk = f32(rng.standard_normal((3, 3, 4, 1)))
    pk = f32(rng.standard_normal((1, 1, 4, cout)))
    y, z = mem.empty((n, h, w, 4)), mem.empty((n, h, w, cout))
    ops.dwconv3x3_fwd(ops.View.plain(dev(x)), n, h, w, dev(dk), y)
    ops.pointwise_fwd(y, n * h * w, 4, cout, dev(pk), z, mem.zeros(ops.bn_partials_numel(n * h * w, cout)))
    _assert_pixels_equal(z[:, 1:-1, 1:-1], "image block forward")


@pytest.mark.parametrize("n,h,w,cin,cout,split", [(2, 5, 7, 128, 64, False), (1, 3, 43, 64, 32, False),
                                                  (1, 3, 43, 6, 12, False), (2, 5, 7, 128, 64, True)])
def test_constant_view_conv_transpose_fwd(ops, n, h, w, cin, cout, split):
    """conv_transpose2x2 forward: bitwise equal per channel and per (a, b) phase of the 2x2 upsampling."""
    rng = np.random.default_rng(cin + cout)
    x = np.broadcast_to(np.abs(_const_rows(rng, cin)), (n, h, w, cin))
    k = dev(f32(rng.standard_normal((2, 2, cout, cin)) / np.sqrt(cin)))
    b = dev(f32(rng.standard_normal(cout)))
    out = mem.empty((n, 2 * h, 2 * w, cout))
    kx = None
    if split:
        kx = mem.empty(3 * 4 * cout * cin, dtype=torch.int16)
        ops.split_x3(k, [(0, 4 * cout, cin, 0)], kx, keep=True)
    ops.conv_transpose2x2_fwd(ops.View.plain(dev(x)), n, h, w, cout, k, b, out, kx=kx)
    phases = out.reshape(n, h, 2, w, 2, cout).permute(0, 1, 3, 2, 4, 5).reshape(n * h * w, 4 * cout)
    _assert_pixels_equal(phases, "conv_transpose2x2_fwd")


# ------------------------------------------------- c. BatchNorm statistics on flat data -----
# Rows of the second input: base (1 + (0.5 r)) per channel times (1 + 1e-3 u), u one of FLAT_ROWS standard
# normal rows: std about 1e-3 of |mean| in every input channel and, through the GEMM, in z (|mean z| is a sum
# of ~N(0, 1) pointwise weights: up to ~4).  The gate on rstd is 1e-5 RELATIVE, so the honest error must stay
# below it: float32 rounding of z (~|z| 2^-24 times a small accumulation factor a) moves a variance of
# std^2 = 1e-6 z^2 by at most 2 std a |z| 2^-24 ~ 1.2e-10 a z^2, against var + eps >= 1e-3: with |z| <= 4 and
# a <= 4 that is 8e-9 / 1e-3 / 2 = 4e-6 in rstd.  (A larger offset would let the float64 reference itself
# disagree with ANY float32 z beyond the gate.)  Raw second moments lose 2^-24 z^2 a in E[x^2] - E[x]^2:
# ~5e-7 a against 1e-3, two orders of magnitude outside; on the constant channel var must be below 2e-8.
FLAT_ROWS = 5


def _flat_rows(rng, m, c, constant):
    base = f32(1.0 + 0.5 * rng.random(c))
    if constant:
        return np.broadcast_to(base, (m, c)).copy()
    u = rng.standard_normal((FLAT_ROWS, c))
    return f32(base * (1.0 + 1e-3 * u[rng.integers(0, FLAT_ROWS, m)]))


def _check_bn_finalize(ops, part, m, cout, zr, rng, constant):
    """test_pointwise_and_bn_stats' gates on bn_finalize of `part` against float64 statistics of zr (m, cout)."""
    gamma, beta = bn_affine(rng, cout)
    mm, mv = f32(rng.standard_normal(cout) * 0.1), f32(1 + rng.random(cout))
    tm, tv = dev(mm), dev(mv)
    outs = [mem.empty(cout) for _ in range(4)]
    ops.bn_finalize(part, m, cout, dev(gamma), dev(beta), 1e-3, 0.99, tm, tv, True, *outs)
    _, mean, var = K.bn_train(zr.reshape(m, 1, 1, cout), gamma, beta)
    mm2, mv2 = K.bn_moving_update(mm, mv, mean, var)
    inv = gamma / np.sqrt(var + 1e-3)
    got_rstd = host(outs[1])
    assert (got_rstd <= np.float32(1 / np.sqrt(1e-3)) * (1 + 1e-6)).all(), "a variance below zero"
    if constant:
        assert np.abs(var).max() < 1e-20  # (float64: exactly constant up to the rounding of its own mean)
    else:
        assert np.sqrt(var).max() < 5e-3 and np.abs(mean).max() > 1.0
    assert rel_err(host(outs[0]), mean) < 1e-4
    assert rel_err(got_rstd, 1 / np.sqrt(var + 1e-3)) < 1e-5
    assert rel_err(host(outs[2]), inv) < 1e-5
    assert rel_err(host(outs[3]), beta - mean * inv) < 1e-4
    assert rel_err(host(tm), mm2) < 1e-5 and rel_err(host(tv), mv2) < 1e-5


@pytest.mark.parametrize("constant", [True, False])
@pytest.mark.parametrize("m,cin,cout,split", [(300, 64, 64, False), (129, 32, 96, False), (8229, 64, 128, False),
                                              (300, 64, 128, True), (8229, 32, 64, True),
                                              (300, 4, 64, False), (8229, 4, 32, False)])  # cin 4: the image block
def test_bn_stats_flat_pointwise(ops, m, cin, cout, split, constant):
    """The rows GEMM's statistics epilogues (fp32 and split precision; 8229 rows = 65 partials: more than one
    finalize chunk) and the image block's 4-channel pointwise."""
    rng = np.random.default_rng(m + cin + cout)
    y = _flat_rows(rng, m, cin, constant)
    pk32 = f32(rng.standard_normal((1, 1, cin, cout)) / np.sqrt(cin))
    pk = dev(pk32)
    z = mem.empty((m, cout))
    part = mem.zeros(ops.bn_partials_numel(m, cout))
    ops.pointwise_fwd(dev(y), m, cin, cout, pk, z, part, pkx=_split(ops, pk, cin, cout) if split else None)
    zr = y @ pk32[0, 0]
    assert rel_err(host(z), zr) < 5e-6
    _check_bn_finalize(ops, part, m, cout, zr, rng, constant)


@pytest.mark.parametrize("constant", [True, False])
@pytest.mark.parametrize("variant,n,h,w,cin,cout", [("tile", 2, 16, 32, 16, 64), ("tile", 1, 16, 32, 64, 128),
                                                     ("rk", 2, 16, 32, 64, 128), ("rk_x6", 2, 16, 32, 64, 64),
                                                     ("rk_x6", 1, 16, 32, 128, 256), ("px", 2, 16, 32, 64, 128),
                                                     ("px",) + PX_RAGGED + (64, 64)])
def test_bn_stats_flat_sepconv(ops, variant, n, h, w, cin, cout, constant):
    """Every forward kernel of the fused separable conv.  The depthwise kernel has its centre tap only, so
    the zero padding does not put an edge into the flat channel."""
    rng = np.random.default_rng(n * h + cin + cout)
    m = n * h * w
    x = _flat_rows(rng, m, cin, constant).reshape(n, h, w, cin)
    dk32 = np.zeros((3, 3, cin, 1))
    dk32[1, 1, :, 0] = f32(0.5 + rng.random(cin))
    pk32 = f32(rng.standard_normal((1, 1, cin, cout)) / np.sqrt(cin))
    pk = dev(pk32)
    schedule, split = _sep_variants(ops)[variant]
    pkx = _split(ops, pk, cin, cout) if split else None
    y, z = mem.empty((n, h, w, cin)), mem.empty((n, h, w, cout))
    part = mem.zeros(ops.bn_partials_numel(m, cout))
    with _schedule(ops, schedule):
        ops.sepconv_fwd(ops.View.plain(dev(x)), n, h, w, dev(dk32), cout, pk, y, z, part, pkx=pkx)
    zr = K.pointwise(K.depthwise3x3(x, dk32), pk32).reshape(m, cout)
    assert rel_err(host(z).reshape(m, cout), zr) < 5e-6
    _check_bn_finalize(ops, part, m, cout, zr, rng, constant)


@pytest.mark.parametrize("m,cin,c", [(300, 16, 32), (1000, 64, 64), (129, 64, 68)])
def test_bn_backward_on_a_constant_channel(ops, m, cin, c):
    """bn_relu_bwd and pointwise_bwd_data_bnrelu where every other channel of z is exactly constant (batch
    variance 0, rstd = 1 / sqrt(eps), x-hat = 0 everywhere), against K.bn_relu_bwd at test_bn_relu_bwd's and
    test_pointwise_bwd_data_bnrelu's gates."""
    rng = np.random.default_rng(m + c)
    z = f32(rng.standard_normal((m, 1, 1, c)) * 2 + 0.3)
    z[..., ::2] = f32(_const_rows(rng, c)[::2] * 3.0)
    da = f32(rng.standard_normal((m, 1, 1, c)))
    gamma, beta = bn_affine(rng, c)
    beta[::2] = f32(np.where(np.arange(c)[::2] % 4 == 0, 0.3, -0.3))  # the constant channels: all on, all off
    _, mean, var = K.bn_train(z, gamma, beta)
    assert var[::2].max() < 1e-25  # (zero up to the rounding of the float64 mean)
    var[::2] = 0.0
    mean, var = f32(mean), f32(var)
    assert np.array_equal(mean[::2], z[0, 0, 0, ::2])
    rstd = 1 / np.sqrt(var + 1e-3)
    scale, shift = f32(gamma * rstd), f32(beta - mean * gamma * rstd)
    rz, rg, rb = K.bn_relu_bwd(da, z, gamma, beta, mean, var)
    assert (rg[::2] == 0).all()
    tmean, trstd, ts, th = dev(mean), dev(f32(rstd)), dev(scale), dev(shift)
    dg, db, dz = mem.zeros(c), mem.zeros(c), mem.empty((m, c))
    ops.bn_relu_bwd(dev(da), dev(z), m, c, tmean, trstd, ts, th, True, 0.0, 0, dg, db, dz)
    assert rel_err(host(dg), rg) < 1e-4
    assert rel_err(host(db), rb) < 1e-5
    assert rel_err(host(dz), rz.reshape(m, c)) < 1e-4
    pk = f32(rng.standard_normal((1, 1, cin, c)) / np.sqrt(c))
    dg2, db2, coef = mem.zeros(c), mem.zeros(c), mem.empty(3 * c)
    ops.bn_relu_bwd_stats(dev(da), dev(z), m, c, tmean, trstd, ts, th, True, 0.0, 0, dg2, db2, coef)
    dy, dz2 = mem.empty((m, cin)), mem.full((m, c), 7.0)
    ops.pointwise_bwd_data_bnrelu(dev(da), dev(z), m, cin, c, dev(pk), ts, th, coef, 0.0, 0, dy, dz2)
    assert rel_err(host(dg2), rg) < 1e-4
    assert rel_err(host(db2), rb) < 1e-5
    assert rel_err(host(dz2), rz.reshape(m, c)) < 1e-4
    assert rel_err(host(dy), rz.reshape(m, c) @ pk[0, 0].T) < 1e-4


# --------------------------------------------------------------- d. ReLU at exactly zero -----
def _zeroed(rng, shape):
    """Noise with about a quarter of the elements +0.0 or -0.0 (half each); (z, the mask of those)."""
    z = f32(rng.standard_normal(shape) * 2 + 0.3)
    u = rng.random(shape)
    z[u < 0.125] = 0.0
    z[(u >= 0.125) & (u < 0.25)] = -0.0
    zero = u < 0.25
    assert np.signbit(z[zero]).any() and not np.signbit(z[zero]).all()
    return z, zero


def _unit_bn(c, use_bn):
    """scale 1, shift 0: BatchNorm with mean 0, rstd 1, gamma 1, beta 0 (batch variance 1 - eps), or no
    BatchNorm and a zero bias, as a fresh network has it.  The pre-activation is z itself."""
    one, zero = np.ones(c), np.zeros(c)
    return dict(gamma=one, beta=zero, mean=zero, var=one - 1e-3, rstd=one if use_bn else zero, scale=one, shift=zero)


def _relu_bwd_ref(da, z, use_bn):
    """(dz, dgamma, dbeta) of the float64 oracle at scale 1, shift 0; da, z (m, c)."""
    m, c = z.shape
    if use_bn:
        b = _unit_bn(c, True)
        rz, rg, rb = K.bn_relu_bwd(da.reshape(m, 1, 1, c), z.reshape(m, 1, 1, c), b["gamma"], b["beta"], b["mean"], b["var"])
        return rz.reshape(m, c), rg, rb
    rz = np.where(z > 0, da, 0.0)
    return rz, None, rz.sum(0)


@pytest.mark.parametrize("use_bn", [True, False])
@pytest.mark.parametrize("m,c", [(300, 16), (129, 68), (96, 3)])
def test_relu_zero_bn_relu_bwd(ops, use_bn, m, c):
    rng = np.random.default_rng(m + c)
    z, zero = _zeroed(rng, (m, c))
    da = f32(rng.standard_normal((m, c)))
    b = {k: dev(v) for k, v in _unit_bn(c, use_bn).items()}
    dg, db, dz = mem.zeros(c), mem.zeros(c), mem.empty((m, c))
    ops.bn_relu_bwd(dev(da), dev(z), m, c, b["mean"], b["rstd"], b["scale"], b["shift"], use_bn, 0.0, 0,
                    dg if use_bn else None, db, dz)
    rz, rg, rb = _relu_bwd_ref(da, z, use_bn)
    if use_bn:
        assert rel_err(host(dg), rg) < 1e-4
    else:
        assert not host(dz)[zero].any()
    assert rel_err(host(db), rb) < 1e-5
    assert rel_err(host(dz), rz) < 1e-4


@pytest.mark.parametrize("use_bn", [True, False])
@pytest.mark.parametrize("m,cin,cout", [(300, 16, 32), (257, 128, 64), (129, 64, 68), (300, 4, 64), (1000, 4, 32)])
def test_relu_zero_pointwise_bwd_data_bnrelu(ops, use_bn, m, cin, cout):
    """pointwise_bwd_data_bnrelu, and at cin 4 its weight-gradient twin (dz never stored: seen through dW)."""
    rng = np.random.default_rng(m + cin + cout)
    c = cout
    z, zero = _zeroed(rng, (m, c))
    da = f32(rng.standard_normal((m, c)))
    pk = f32(rng.standard_normal((1, 1, cin, cout)) / np.sqrt(cout))
    b = {k: dev(v) for k, v in _unit_bn(c, use_bn).items()}
    dg, db, coef = mem.zeros(c), mem.zeros(c), mem.empty(3 * c)
    ops.bn_relu_bwd_stats(dev(da), dev(z), m, c, b["mean"], b["rstd"], b["scale"], b["shift"], use_bn, 0.0, 0,
                          dg if use_bn else None, db, coef)
    dy, dz = mem.empty((m, cin)), mem.full((m, c), 7.0)
    ops.pointwise_bwd_data_bnrelu(dev(da), dev(z), m, cin, cout, dev(pk), b["scale"], b["shift"], coef, 0.0, 0, dy, dz)
    rz, rg, rb = _relu_bwd_ref(da, z, use_bn)
    if use_bn:
        assert rel_err(host(dg), rg) < 1e-4
    else:
        assert not host(dz)[zero].any()
    assert rel_err(host(db), rb) < 1e-5
    assert rel_err(host(dz), rz) < 1e-4
    assert rel_err(host(dy), rz @ pk[0, 0].T) < 1e-4
    if cin == 4:
        y = f32(rng.standard_normal((m, cin)))
        dy_w, dpk = mem.empty((m, cin)), mem.full((1, 1, cin, cout), 7.0)
        ops.pointwise_bwd_data_bnrelu_wgrad(dev(da), dev(z), m, cin, cout, dev(pk), b["scale"], b["shift"], coef,
                                            dev(y), dy_w, dpk)
        assert rel_err(host(dy_w), rz @ pk[0, 0].T) < 1e-4
        assert rel_err(host(dpk).reshape(cin, cout), y.T @ rz) < 1e-5  # (test_pointwise_bwd_data_bnrelu_wgrad's)


@pytest.mark.parametrize("use_bn", [True, False])
@pytest.mark.parametrize("n,h,w,c", [(2, 9, 17, 64), (3, 9, 5, 16), (1, 3, 43, 32)])
def test_relu_zero_dwconv_bwd_data_bnstats(ops, use_bn, n, h, w, c):
    """dwconv3x3_bwd_data_bnstats through a BN+ReLU view whose z holds the zeros: the BN-backward statistics
    of the view's block see the mask (sum of g, sum of g x-hat) within test_dwconv_bwd_data_bnstats's 1e-5."""
    rng = np.random.default_rng(n * 100 + h + c)
    z, zero = _zeroed(rng, (n, h, w, c))
    b = _unit_bn(c, True)
    v = ops.View.bnrelu(dev(z), dev(b["scale"]), dev(b["shift"]))
    S = ops.dwconv3x3_bwd_data_bnstats_slabs(v, n, h, w)
    assert S > 0
    dk, dy = f32(rng.standard_normal((3, 3, c, 1))), f32(rng.standard_normal((n, h, w, c)))
    mean, rstd = dev(f32(rng.standard_normal(c) * 0.1)), dev(f32(1.0 + rng.random(c)))
    part = mem.zeros(ops.bn_stats_partials_numel(S, c))
    dx = mem.empty((n, h, w, c))
    ops.dwconv3x3_bwd_data_bnstats(v, n, h, w, dev(dk), dev(dy), dx, mean if use_bn else None,
                                   rstd if use_bn else None, part)
    dxv, _ = K.depthwise3x3_bwd(K.relu(z), dk, dy)
    assert rel_err(host(dx), dxv) < 2e-6
    m = n * h * w
    dg, db, coef = mem.zeros(c), mem.zeros(c), mem.empty(3 * c)
    ops.bn_relu_bwd_stats_finish(part, S, m, c, mean, rstd, use_bn, dg if use_bn else None, db, coef)
    g = np.where(z > 0, host(dx), 0.0).reshape(m, c)
    assert rel_err(host(db), g.sum(0)) < 1e-5
    if use_bn:
        assert rel_err(host(dg), (g * ((z.reshape(m, c) - host(mean)) * host(rstd))).sum(0)) < 1e-5


@pytest.mark.parametrize("use_bn", [True, False])
@pytest.mark.parametrize("n,h,w,cin", [(2, 8, 16, 64), (1, 16, 32, 128)])
def test_relu_zero_sepconv_bwd_fused(ops, use_bn, n, h, w, cin):
    """sepconv_bwd_fused: dy and both weight gradients against the float64 oracle at test_sepconv_bwd_fused's
    gates (the depthwise kernel gradient at the same 1e-4)."""
    rng = np.random.default_rng(n + cin)
    cout, m = 64, n * h * w
    x = f32(rng.standard_normal((n, h, w, cin)))
    dk = f32(rng.standard_normal((3, 3, cin, 1)))
    pk = f32(rng.standard_normal((1, 1, cin, cout)) / np.sqrt(cin))
    z, _ = _zeroed(rng, (m, cout))
    da = f32(rng.standard_normal((m, cout)))
    b = {k: dev(v) for k, v in _unit_bn(cout, use_bn).items()}
    tz, tda = dev(z), dev(da)
    dg, db, coef = mem.zeros(cout), mem.zeros(cout), mem.empty(3 * cout)
    ops.bn_relu_bwd_stats(tda, tz, m, cout, b["mean"], b["rstd"], b["scale"], b["shift"], use_bn, 0.0, 0,
                          dg if use_bn else None, db, coef)
    dy = mem.full((n, h, w, cin), 7.0)
    ddk, dpk = mem.empty((3, 3, cin, 1)), mem.empty((1, 1, cin, cout))
    ops.sepconv_bwd_fused(ops.View.plain(dev(x)), n, h, w, dev(dk), dev(pk), tda, tz, b["scale"], b["shift"], coef,
                          cout, dy, ddk, dpk)
    rz, _, rb = _relu_bwd_ref(da, z, use_bn)
    assert rel_err(host(db), rb) < 1e-5
    ry = rz @ pk[0, 0].T
    assert rel_err(host(dy).reshape(m, cin), ry) < 1e-4
    assert rel_err(host(dpk).reshape(cin, cout), K.depthwise3x3(x, dk).reshape(m, cin).T @ rz) < 1e-4
    _, rdk = K.depthwise3x3_bwd(x, dk, ry.reshape(n, h, w, cin))
    assert rel_err(host(ddk), rdk) < 1e-4


@pytest.mark.parametrize("use_bn", [True, False])
@pytest.mark.parametrize("loss_kind", [0, 1])
@pytest.mark.parametrize("ncls", [1, 5])
def test_relu_zero_head_bwd_bnstats(ops, use_bn, loss_kind, ncls):
    """head_bwd through a BN+ReLU view whose z holds the zeros, with its fused BN statistics: gradients at
    test_head_dice's 1e-4, statistics against float64 at the sibling producers' 1e-5."""
    rng = np.random.default_rng(ncls + loss_kind)
    n, h, w, c = 2, 16, 24, 64
    m = n * h * w
    z, zero = _zeroed(rng, (n, h, w, c))
    b = _unit_bn(c, True)
    v = ops.View.bnrelu(dev(z), dev(b["scale"]), dev(b["shift"]))
    k = f32(rng.standard_normal((1, 1, c, ncls)) * 0.2)
    bias = f32(rng.standard_normal(ncls) * 0.1)
    prob = mem.empty((n, h, w, ncls))
    ops.head_fwd(v, n, h, w, ncls, dev(k), dev(bias), prob)
    pp = host(prob)
    assert rel_err(pp, K.head(K.relu(z), k, bias, ncls)) < 2e-6
    yt = blob_masks(n, (h, w), ncls).astype(np.float64)
    sums, res = mem.empty(n * ncls * 3), mem.empty(3)
    ops.dice_fwd(dev(yt), prob, n, h * w, ncls, 1e-7, sums, res)
    S = ops.head_bwd_bnstats_slabs(v, n, h, w, ncls)
    assert S > 0
    mean, rstd = dev(f32(rng.standard_normal(c) * 0.1)), dev(f32(1.0 + rng.random(c)))
    part = mem.zeros(ops.bn_stats_partials_numel(S, c))
    dx, dkk, dbb = mem.empty((n, h, w, c)), mem.empty(c * ncls), mem.empty(ncls)
    ops.head_bwd_bnstats(v, n, h, w, ncls, dev(k), prob, dev(yt), sums, 1e-7, loss_kind, dx, dkk, dbb,
                         mean if use_bn else None, rstd if use_bn else None, part)
    dprob = K.dice_loss_grad(yt, pp) if loss_kind == 0 else K.iou_loss_grad(yt, pp)
    rdx, rdk, rdb = K.head_bwd(K.relu(z), k, pp, dprob, ncls)
    assert rel_err(host(dx), rdx) < 1e-4
    assert rel_err(host(dkk), rdk.reshape(-1)) < 1e-4
    assert rel_err(host(dbb), rdb) < 1e-4
    dg, db, coef = mem.zeros(c), mem.zeros(c), mem.empty(3 * c)
    ops.bn_relu_bwd_stats_finish(part, S, m, c, mean, rstd, use_bn, dg if use_bn else None, db, coef)
    g = np.where(z > 0, host(dx), 0.0).reshape(m, c)
    assert rel_err(host(db), g.sum(0)) < 1e-5
    if use_bn:
        assert rel_err(host(dg), (g * ((z.reshape(m, c) - host(mean)) * host(rstd))).sum(0)) < 1e-5


# -------------------------------------------------------------------- e. loss and head edges -----
HEAD_N, HEAD_H, HEAD_W, HEAD_CIN = 3, 16, 24, 64
SATURATED_LOGIT = 42.0


def _head_case(rng, ncls, saturated, xv):
    """(kernel, bias, masks) for the head input xv.  Binary: an empty, a rectangle and a full mask.  5
    classes: the masks hold classes 0, 1 and 4 only; class 3's bias is -30, so its probabilities sum to
    ~1e-10 an image (class 2 is absent from the masks alone).  saturated: test_head_dice's 0.2-scaled
    kernel scaled up until the largest |logit| (float64 oracle) is SATURATED_LOGIT: sigmoid(42) is exactly 1
    in float32 and sigmoid(-42) is 6e-19; softmax rows with such a gap are one-hot in float32."""
    k = rng.standard_normal((1, 1, HEAD_CIN, ncls)) * 0.2
    if saturated:
        k *= SATURATED_LOGIT / np.abs(K.pointwise(xv, k)).max()
    b = f32(rng.standard_normal(ncls) * 0.1)
    if ncls > 1:
        b[3] = -30.0
    return f32(k), b, blob_masks(HEAD_N, (HEAD_H, HEAD_W), ncls).astype(np.float64)


@pytest.mark.parametrize("saturated", [False, True])
@pytest.mark.parametrize("loss_kind", [0, 1])
@pytest.mark.parametrize("ncls", [1, 5])
def test_loss_and_head_edges(ops, ncls, loss_kind, saturated, record_property):
    """dice_fwd and head_bwd where the per-(image, class) terms reduce to smooth / (p + smooth) (t == 0,
    i == 0) and where the head saturates.  Loss, dice and IoU within test_head_dice's 1e-6 of the oracle on
    the device's own probabilities; probabilities within test_head_fwd_binary's 2e-6, all finite.

    Gradient gates: max(test_head_dice's 1e-4, 2 x the relative L2 error of the SAME float64 formulas
    (K.dice_loss_grad / K.iou_loss_grad, K.head_bwd) evaluated in float32 NumPy on the same float32 inputs).
    With t == 0 a term's gradient is (i + s) / (p + s)^2-like: p ~ 1e-10 puts 1e-7 / 1e-14 in front of float32
    sums, which no float32 implementation reproduces to 1e-4; the factor 2 is the margin train_step_parity
    allows for accumulation order.  Both numbers are recorded per case; none comes from the device."""
    rng = np.random.default_rng(10 * ncls + 2 * loss_kind + saturated)
    n, h, w, cin = HEAD_N, HEAD_H, HEAD_W, HEAD_CIN
    z = f32(rng.standard_normal((n, h, w, cin)))
    sc, sh = bn_affine(rng, cin)
    v = ops.View.bnrelu(dev(z), dev(sc), dev(sh))
    xv = K.relu(z * sc + sh)
    k, b, yt = _head_case(rng, ncls, saturated, xv)
    prob = mem.full((n, h, w, ncls), -1.0)
    ops.head_fwd(v, n, h, w, ncls, dev(k), dev(b), prob)
    pp = host(prob)
    rp = K.head(xv, k, b, ncls)
    assert np.isfinite(pp).all() and pp.min() >= 0.0 and pp.max() <= 1.0
    assert rel_err(pp, rp) < 2e-6
    if saturated:
        logits = K.pointwise(xv, k) + b
        assert np.abs(logits).max() > 40.0
        assert (pp == 1.0).any() and pp.min() < 1e-9
    elif ncls > 1:
        assert pp[..., 3].sum((1, 2)).max() < 1e-9 and not yt[..., 2].any() and not yt[..., 3].any()
    sums, res = mem.empty(n * ncls * 3), mem.empty(3)
    ops.dice_fwd(dev(yt), prob, n, h * w, ncls, 1e-7, sums, res)
    r = host(res)
    assert np.isfinite(r).all()
    assert abs(r[0] - K.dice_loss(yt, pp)) < 1e-6
    assert abs(r[1] - K.dice_coef(yt, pp)) < 1e-6
    assert abs(r[2] - K.iou_coef(yt, pp)) < 1e-6
    dx, dk, db = mem.empty((n, h, w, cin)), mem.empty((1, 1, cin, ncls)), mem.empty(ncls)
    ops.head_bwd(v, n, h, w, ncls, dev(k), prob, dev(yt), sums, 1e-7, loss_kind, dx, dk, db)
    grad = K.dice_loss_grad if loss_kind == 0 else K.iou_loss_grad
    ref = K.head_bwd(xv, k, pp, grad(yt, pp), ncls)
    t32 = np.float32
    x32, k32, p32, y32 = xv.astype(t32), k.astype(t32), pp.astype(t32), yt.astype(t32)
    got32 = K.head_bwd(x32, k32, p32, grad(y32, p32), ncls)
    assert all(a.dtype == t32 for a in got32)
    for name, got, g32, want in zip(("dx", "dk", "db"), (dx, dk, db), got32, ref):
        got = host(got)
        assert np.isfinite(got).all(), name
        e, e32 = norm_err(got, want), norm_err(g32, want)
        gate = max(1e-4, 2.0 * e32)
        record_property(f"{name}_err", e)
        record_property(f"{name}_err_float32_numpy", e32)
        print(f"head edges[{ncls}, {loss_kind}, {saturated}] {name}: device {e:.3e}, float32 NumPy {e32:.3e}, gate {gate:.3e}")
        assert e <= gate, (name, e, gate)


def test_meaniou_absent_class_and_threshold_ties(ops):
    """meaniou_update with a class that never occurs (labels and predictions) and with probabilities exactly
    equal to the threshold (`> threshold`: they count as class 0): the confusion matrix is K's, exactly."""
    rng = np.random.default_rng(5)
    count = 10007
    yt = rng.choice([0.0, 1.0, 2.0, 4.0], count)  # class 3 never occurs
    yp = rng.choice([0.0, 1.0, 2.0, 4.0], count) + rng.choice([0.0, 0.25, 0.999], count)
    conf = mem.zeros(25, dtype=torch.int64)
    ops.meaniou_update(dev(yt), dev(yp), 5, None, conf)
    ref = K.meaniou_confusion(f32(yt), f32(yp), 5)
    assert not ref[3].any() and not ref[:, 3].any()
    assert np.array_equal(conf.cpu().numpy().reshape(5, 5), ref)
    for thr in (0.5, 0.3):
        t32 = float(np.float32(thr))  # (the kernel's threshold argument is a float)
        yt = (rng.random(count) > 0.5).astype(np.float64)
        yp = f32(rng.random(count))
        yp[::3] = t32
        yp[1::7] = np.nextafter(np.float32(t32), np.float32(1.0))
        conf = mem.zeros(4, dtype=torch.int64)
        ops.meaniou_update(dev(yt), dev(yp), 2, t32, conf)
        ref = K.meaniou_confusion(yt, yp, 2, t32)
        assert np.array_equal(conf.cpu().numpy().reshape(2, 2), ref)
        conf.zero_()  # buffers not 16-byte aligned take the scalar kernel
        ops.meaniou_update(mem.skewed(f32(yt)[1:]), mem.skewed(yp[1:]), 2, t32, conf)
        assert np.array_equal(conf.cpu().numpy().reshape(2, 2), K.meaniou_confusion(yt[1:], yp[1:], 2, t32))
