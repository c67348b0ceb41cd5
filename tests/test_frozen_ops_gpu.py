"""Per-op parity of the frozen fp16 kernels (csrc/frozen.hip, through unet_amd.ops) against float64
NumPy on fp16-representable inputs.  Every bound is derived from the number formats, element by
element; none is measured:

  * depthwise output rounded to fp16: 2^-11 relative on each y, so 2^-11 (A @ |pw'|) with
    A = depthwise(|x|, |dw|);
  * fp32 summation, worst case: 9 depthwise terms and K product terms, (K + 9) 2^-24 (A @ |pw'|);
  * the fp16 output: 2^-11 |ref|, plus 2^-24 for the subnormal range.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from f16_emulation import U16, U32, r16  # noqa: E402
from oracle import keras_ops as K  # noqa: E402

pytestmark = pytest.mark.gpu

EPS16, EPS32 = 2.0 ** -11, 2.0 ** -24


def dev16(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float16))).cuda()


def dev32(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32))).cuda()


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _sep_inputs(seed, n, h, w, cin, cout):
    x = U16(seed, (n, h, w, cin), -1, 1)
    dk = U32(seed + 1, (3, 3, cin, 1), -0.5, 0.5)
    pw = U16(seed + 2, (1, 1, cin, cout), -0.25, 0.25)
    bias = U32(seed + 3, (cout,), -0.1, 0.1)
    return x, dk, pw, bias


def _sep_run(x, dk, pw, bias, split=None, route=0, pool=False):
    """Runs unet_f16_sepconv; split = c0 reads x as the concat of its first c0 and remaining channels."""
    from unet_amd import ops
    n, h, w, cin = x.shape
    cout = pw.shape[-1]
    if split is None:
        view = ops.F16View.plain(dev16(x))
    else:
        view = ops.F16View.concat(dev16(x[..., :split]), dev16(x[..., split:]))
    out = torch.full((n, h, w, cout), float("nan"), dtype=torch.float16, device="cuda")
    op = torch.full((n, h // 2, w // 2, cout), float("nan"), dtype=torch.float16, device="cuda") if pool else None
    ops.f16_sepconv(view, n, h, w, dev32(dk).reshape(-1), cout, dev16(pw[0, 0].T), dev32(bias), out, op, route)
    torch.cuda.synchronize()
    return out, op


def _sep_check(out, x, dk, pw, bias):
    cin = x.shape[-1]
    ref = K.relu(K.pointwise(K.depthwise3x3(x, dk), pw) + bias)
    amp = K.pointwise(K.depthwise3x3(np.abs(x), np.abs(dk)), np.abs(pw))
    bound = (EPS16 + (cin + 9) * EPS32) * amp + EPS16 * np.abs(ref) + EPS32
    err = np.abs(host(out) - ref)
    print("sepconv max err / bound", float((err / bound).max()))
    assert np.all(np.isfinite(host(out)))
    assert np.all(err <= bound), float((err / bound).max())
    assert float(np.abs(ref).max()) > 0.1  # the case is not vacuous


# (n, h, w), cin, cout, concat split, route -- the issue's shapes, then wider outputs and more
# K chunks; a launch of fewer than 512 blocks takes 32-column blocks, so the 64- and 128-column
# kernels are reached by the four cases of >= 512 pixel tiles at the end
SEP_CASES = [
    ((2, 8, 16), 16, 32, None, 2),    # one tile, one K stage
    ((2, 8, 16), 48, 96, None, 2),    # the LDS halo chunk tail, column count not a power of two
    ((1, 16, 32), 32, 64, None, 2),   # halo across tile edges
    ((1, 16, 32), 32, 32, 16, 2),     # CONCAT 16 + 16
    ((3, 6, 4), 32, 64, None, 1),     # rows policy, M tail
    ((1, 1, 1), 64, 64, None, 1),     # a single pixel
    ((1, 8, 16), 80, 128, None, 2),   # two halo chunks (64 + 16), four column blocks
    ((1, 5, 3), 144, 256, 64, 1),     # rows policy, odd sizes, CONCAT 64 + 80
    ((1, 8, 16), 32, 64, None, 0),    # auto route
    ((2, 128, 256), 16, 128, None, 2),  # 512 tiles: the 128-column kernel, tile policy
    ((2, 128, 256), 16, 64, None, 0),   # ... the 64-column kernel
    ((2, 130, 254), 16, 128, None, 1),  # 516 row blocks with an M tail: 128 columns, rows policy
    ((2, 130, 254), 16, 64, None, 0),   # ... 64 columns (auto falls to rows: 254 % 16 != 0)
]


@pytest.mark.parametrize("shape,cin,cout,split,route", SEP_CASES)
def test_f16_sepconv(shape, cin, cout, split, route):
    x, dk, pw, bias = _sep_inputs(100 + cin + cout, *shape, cin, cout)
    out, _ = _sep_run(x, dk, pw, bias, split, route)
    _sep_check(out, x, dk, pw, bias)


@pytest.mark.parametrize("shape,cin,cout,route", [((2, 8, 16), 32, 64, 2), ((3, 6, 4), 32, 64, 1),
                                                  ((2, 8, 16), 32, 256, 1), ((2, 128, 256), 16, 128, 2),
                                                  ((2, 130, 254), 16, 64, 1)])
def test_f16_sepconv_pool_is_the_max_of_out(shape, cin, cout, route):
    x, dk, pw, bias = _sep_inputs(300 + cout, *shape, cin, cout)
    out, pool = _sep_run(x, dk, pw, bias, None, route, pool=True)
    _sep_check(out, x, dk, pw, bias)
    n, h, w = shape
    o = out.cpu().numpy()
    want = o.reshape(n, h // 2, 2, w // 2, 2, cout).max(axis=(2, 4))
    assert np.array_equal(pool.cpu().numpy().view(np.uint16), want.view(np.uint16))
    # and the pooled launch computes the same `out` as the plain one
    plain, _ = _sep_run(x, dk, pw, bias, None, route)
    assert torch.equal(plain, out)


def test_f16_sepconv_routes_are_bitwise_equal():
    x, dk, pw, bias = _sep_inputs(400, 2, 16, 32, 32, 64)
    rows, _ = _sep_run(x, dk, pw, bias, None, 1)
    tile, _ = _sep_run(x, dk, pw, bias, None, 2)
    assert torch.equal(rows.view(torch.int16), tile.view(torch.int16))
    rows, prow = _sep_run(x, dk, pw, bias, None, 1, pool=True)
    tile2, ptile = _sep_run(x, dk, pw, bias, None, 2, pool=True)
    assert torch.equal(rows.view(torch.int16), tile.view(torch.int16)) and torch.equal(tile2, tile)
    assert torch.equal(prow.view(torch.int16), ptile.view(torch.int16))


def test_f16_sepconv_refuses_the_tile_route_on_other_shapes():
    from unet_amd import UnetHipError
    x, dk, pw, bias = _sep_inputs(500, 3, 6, 4, 32, 64)
    with pytest.raises(UnetHipError, match="route 2"):
        _sep_run(x, dk, pw, bias, None, 2)


@pytest.mark.parametrize("shape,cin,cout", [((2, 3, 2), 32, 16), ((1, 8, 8), 64, 32), ((1, 9, 15), 48, 40)])
def test_f16_conv_transpose2x2(shape, cin, cout):
    from unet_amd import ops
    n, h, w = shape
    x = U16(600 + cin, (n, h, w, cin), -1, 1)
    k = U16(601 + cin, (2, 2, cout, cin), -0.25, 0.25)
    b = U32(602 + cin, (cout,), -0.1, 0.1)
    out = torch.full((n, 2 * h, 2 * w, cout), float("nan"), dtype=torch.float16, device="cuda")
    ops.f16_conv_transpose2x2(dev16(x), n, h, w, cin, cout, dev16(k), dev32(b), out)
    torch.cuda.synchronize()
    ref = K.conv_transpose2x2(x, k, b)
    amp = K.conv_transpose2x2(np.abs(x), np.abs(k), np.zeros(cout))
    bound = cin * EPS32 * amp + EPS16 * np.abs(ref) + EPS32
    err = np.abs(host(out) - ref)
    print("convT max err / bound", float((err / bound).max()))
    assert np.all(err <= bound), float((err / bound).max())


# (2, 4, 4, 64): the issue's shape; (1, 3, 5, 32): a pixel tail inside a wave, half the lanes of a pixel idle
@pytest.mark.parametrize("shape", [(2, 4, 4, 64), (1, 3, 5, 32), (1, 2, 2, 136)])
@pytest.mark.parametrize("ncls", [1, 3])
def test_f16_head(ncls, shape):
    from unet_amd import ops
    n, h, w, cin = shape
    x = U16(700, (n, h, w, cin), 0, 2)
    k = U32(701 + ncls, (1, 1, cin, ncls), -0.5, 0.5)
    b = U32(702 + ncls, (ncls,), -0.5, 0.5)
    prob = torch.full((n, h, w, ncls), float("nan"), dtype=torch.float32, device="cuda")
    ops.f16_head(dev16(x), n, h, w, cin, ncls, dev32(k).reshape(-1), dev32(b), prob)
    torch.cuda.synchronize()
    ref = K.head(x, k, b, ncls)
    amp = (K.pointwise(np.abs(x), np.abs(k)) + np.abs(b)).max(axis=-1, keepdims=True)
    bound = (cin + 2) * EPS32 * amp + 1e-6
    err = np.abs(host(prob) - ref)
    print("head max err / bound", float((err / bound).max()))
    assert np.all(err <= bound), float((err / bound).max())
    assert ref.max() - ref.min() > 0.1


# (2, 8, 16, 3) -> 64: the issue's shape; -> 96: 12 channel groups (weights reloaded per round), odd sizes
@pytest.mark.parametrize("n,h,w,cin,cout", [(2, 8, 16, 3, 64), (1, 5, 7, 3, 96), (1, 40, 52, 4, 64)])
def test_f16_image_block(n, h, w, cin, cout):
    from unet_amd import ops
    x = U16(800, (n, h, w, cin), 0, 1)
    dk = U32(801, (3, 3, cin, 1), -0.5, 0.5)
    pw = U32(802, (1, 1, cin, cout), -0.5, 0.5)
    b = U32(803, (cout,), -0.1, 0.1)
    out = torch.full((n, h, w, cout), float("nan"), dtype=torch.float16, device="cuda")
    ops.f16_image_block(dev32(x), n, h, w, cin, dev32(dk).reshape(-1), cout, dev32(pw).reshape(-1), dev32(b), out)
    torch.cuda.synchronize()
    ref = K.relu(K.pointwise(K.depthwise3x3(x, dk), pw) + b)
    amp = K.pointwise(K.depthwise3x3(np.abs(x), np.abs(dk)), np.abs(pw))
    bound = EPS16 * np.abs(ref) + EPS32 + 12 * EPS32 * amp
    err = np.abs(host(out) - ref)
    print("image block max err / bound", float((err / bound).max()))
    assert np.all(err <= bound), float((err / bound).max())
    assert r16(ref).max() > 0.1
