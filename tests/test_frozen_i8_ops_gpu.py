"""Per-op checks of the frozen int8 kernels (csrc/frozen_i8.hip, through unet_amd.ops) against the
NumPy emulator of the arithmetic contract (tests/i8_emulation.py).  For the separable conv, its
pooled output and the upsample the gate is BITWISE EQUALITY of the quantised bytes: the contract
fixes every rounding, nothing is measured.  Seeds are fixed, so a run is deterministic; the
emulated fmaf rounds twice, so a value could land on a tie -- a failure prints the first differing
element, and the answer to a tie is another seed, never a looser gate.  Weights are asymmetric
random int8 matrices (a transposed or mirrored operand cannot pass).

The image block (fp32 arithmetic, then one rounding to a byte) is measured against float64: every
element within one quantisation step and at most 0.1 % of elements different at all.  A float32
NumPy restatement of the block (float32 fmaf chains in the kernel's order) against float64 on these
three cases and seeds differs in 0 / 0 / 2 of 16384 / 3360 / 133120 elements (0.0015 % at most),
never by more than one step, so the cap has almost two orders of magnitude of room.

The head is fp32 on uint8 input: the bound of test_f16_head, (cin + 2) 2^-24 amp + 1e-6.
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import i8_emulation as E  # noqa: E402
from f16_emulation import U32  # noqa: E402
from oracle import keras_ops as K  # noqa: E402

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -24


def dev(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).cuda()  # (the cached inputs are read-only)


def same_bytes(got, want, what):
    """Bitwise equality; a failure names the first differing element."""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    if not np.array_equal(got, want):
        idx = tuple(int(i) for i in np.argwhere(got != want)[0])
        raise AssertionError(f"{what}: {int((got != want).sum())} of {want.size} bytes differ, first at {idx}: "
                             f"gpu {int(got[idx])}, emulator {int(want[idx])}")


def non_vacuous(ref):
    assert ref.min() != ref.max() and not np.all(ref == 0) and not np.all(ref == 255)


# ------------------------------------------------------------------ separable conv ----
# name -> ((n, h, w), cin, cout, concat split).  A split reads the input as [int8 (split) | uint8]
# with the int8 half's taps carrying another scale.
SEP = {
    "tile_32_32": ((2, 8, 16), 32, 32, None),
    "tile_96_96": ((2, 8, 16), 96, 96, None),        # halo chunk tail (64 + 32), three column blocks
    "tile_edges": ((1, 16, 32), 32, 64, None),       # halo across tile edges
    "tile_concat": ((1, 16, 32), 64, 32, 32),        # concat int8 32 + uint8 32, different scales
    "rows_tail": ((3, 6, 4), 32, 64, None),          # rows, M tail
    "pixel": ((1, 1, 1), 64, 64, None),
    "rows_concat": ((1, 5, 3), 160, 256, 64),        # rows, concat 64 + 96, odd sizes
    "acc_max": ((1, 2, 2), 1024, 32, None),          # y_q = +-127 against +-127 columns: |acc| at its maximum
    "wide_128": ((2, 128, 256), 32, 128, None),      # >= 512 blocks: the 128-column kernels
    "wide_64": ((2, 128, 256), 32, 64, None),        # ... the 64-column kernels
    "rows_wide_tail": ((2, 130, 254), 32, 128, None),  # rows with an M tail, 128 columns
    "rows_wide_64": ((2, 130, 254), 32, 64, None),
    "routes": ((2, 16, 32), 32, 64, None),
    "pool_tile": ((2, 8, 16), 32, 64, None),
}


@functools.lru_cache(maxsize=None)
def _sep(name):
    """(input parts, taps, pw_q, mult, bias_q, emulator output), computed once per case."""
    (n, h, w), cin, cout, split = SEP[name]
    rng = np.random.default_rng(1000 + sorted(SEP).index(name))
    taps = rng.uniform(-0.02, 0.02, (9, cin)).astype(np.float32)
    pw_q = rng.integers(-127, 128, (cout, cin)).astype(np.int8)
    mult = (rng.uniform(0.5, 1.5, cout) / (8.0 * np.sqrt(cin))).astype(np.float32)
    bias_q = rng.uniform(-20.0, 100.0, cout).astype(np.float32)
    if name == "acc_max":
        # every tap of channel c has the sign sg[c] and saturates y_q; the first 16 columns are
        # +-127 sg (|acc| = 127 * 127 * 1024), the others stay random
        sg = rng.choice([-1.0, 1.0], cin)
        taps = (np.ones((9, 1)) * sg).astype(np.float32)
        parts = [np.full((n, h, w, cin), 255, np.uint8)]
        pw_q[:16] = (127 * sg[None, :] * rng.choice([-1, 1], (16, 1))).astype(np.int8)
        mult = np.full(cout, 1.2e-5, np.float32)
        bias_q = np.full(cout, 20.0, np.float32)
    elif split is None:
        parts = [rng.integers(0, 256, (n, h, w, cin)).astype(np.uint8)]
    else:
        parts = [rng.integers(-127, 128, (n, h, w, split)).astype(np.int8),
                 rng.integers(0, 256, (n, h, w, cin - split)).astype(np.uint8)]
        taps[:, :split] *= np.float32(2.0)
    x = np.concatenate([p.astype(np.int16) for p in parts], axis=-1)
    ref = E.sepconv(x, taps, pw_q, mult, bias_q)
    if name == "acc_max":
        acc = E.gemm_i64(E.depthwise_q(x, taps), pw_q)
        assert np.abs(acc).max() == 127 * 127 * 1024
    non_vacuous(ref)
    for a in (taps, pw_q, mult, bias_q, ref, *parts):
        a.setflags(write=False)
    return parts, taps, pw_q, mult, bias_q, ref


def _sep_run(name, route, pool=False):
    from unet_amd import ops
    parts, taps, pw_q, mult, bias_q, _ = _sep(name)
    n, h, w = parts[0].shape[:3]
    cout = pw_q.shape[0]
    view = ops.I8View.plain(dev(parts[0])) if len(parts) == 1 else ops.I8View.concat(dev(parts[0]), dev(parts[1]))
    out = torch.full((n, h, w, cout), 77, dtype=torch.uint8, device="cuda")
    op = torch.full((n, h // 2, w // 2, cout), 77, dtype=torch.uint8, device="cuda") if pool else None
    ops.i8_sepconv(view, n, h, w, dev(taps).reshape(-1), cout, dev(pw_q).reshape(-1), dev(mult), dev(bias_q), out, op,
                   route)
    torch.cuda.synchronize()
    return out, op


SEP_CASES = [("tile_32_32", 2), ("tile_96_96", 2), ("tile_edges", 2), ("tile_concat", 2), ("rows_tail", 1),
             ("pixel", 1), ("pixel", 0), ("rows_concat", 1), ("acc_max", 0), ("wide_128", 2), ("wide_128", 1),
             ("wide_64", 2), ("wide_64", 1), ("rows_wide_tail", 1), ("rows_wide_64", 0), ("tile_edges", 0)]


@pytest.mark.parametrize("name,route", SEP_CASES)
def test_i8_sepconv_is_the_emulator_bitwise(name, route):
    out, _ = _sep_run(name, route)
    same_bytes(out, _sep(name)[-1], f"sepconv {name} route {route}")


@pytest.mark.parametrize("name,route", [("pool_tile", 2), ("rows_tail", 1), ("wide_128", 2), ("rows_wide_64", 1)])
def test_i8_sepconv_pool_is_the_max_of_out(name, route):
    out, pool = _sep_run(name, route, pool=True)
    ref = _sep(name)[-1]
    same_bytes(out, ref, f"pooled launch out {name}")
    same_bytes(pool, E.maxpool(ref), f"pool {name}")
    plain, _ = _sep_run(name, route)
    assert torch.equal(plain, out)


def test_i8_sepconv_routes_are_bitwise_equal():
    rows, _ = _sep_run("routes", 1)
    tile, _ = _sep_run("routes", 2)
    assert torch.equal(rows, tile)
    same_bytes(rows, _sep("routes")[-1], "routes")
    rows2, prow = _sep_run("routes", 1, pool=True)
    tile2, ptile = _sep_run("routes", 2, pool=True)
    assert torch.equal(rows2, rows) and torch.equal(tile2, tile) and torch.equal(prow, ptile)


def test_i8_sepconv_refuses_the_tile_route_on_other_shapes():
    from unet_amd import UnetHipError
    with pytest.raises(UnetHipError, match="route 2"):
        _sep_run("rows_tail", 2)


# ---------------------------------------------------------------------- upsample ----
@pytest.mark.parametrize("shape,cin,cout", [((2, 3, 2), 32, 32), ((1, 8, 8), 64, 32), ((1, 9, 15), 96, 64),
                                            ((1, 2, 2), 1024, 32)])
def test_i8_conv_transpose2x2_is_the_emulator_bitwise(shape, cin, cout):
    from unet_amd import ops
    n, h, w = shape
    rng = np.random.default_rng(600 + cin + cout)
    x = rng.integers(0, 256, (n, h, w, cin)).astype(np.uint8)
    k = rng.integers(-127, 128, (2, 2, cout, cin)).astype(np.int8)
    mult = (rng.uniform(0.5, 1.5, 4 * cout) / (150.0 * np.sqrt(cin))).astype(np.float32)
    bias_q = rng.uniform(-30.0, 30.0, cout).astype(np.float32)
    if cin == 1024:  # inputs of 255 against +127 columns: acc32 = 255 * 127 * 1024 > 2^24
        x[:] = 255
        k[0, :, :16, :] = 127
        mult = (rng.uniform(0.5, 1.0, 4 * cout) * 3.5e-6).astype(np.float32)
    colsum = k.astype(np.int64).sum(axis=-1).reshape(-1).astype(np.int32)
    ref = E.conv_transpose(x, k, colsum, mult, bias_q)
    if cin == 1024:
        acc32 = E.gemm_i64(x, k.reshape(4 * cout, cin))
        assert acc32.max() == 255 * 127 * 1024 > 2 ** 24 and (acc32 % 2 == 1).any()
    assert ref.min() < -20 and ref.max() > 20 and not np.all(np.abs(ref) == 127)
    out = torch.full((n, 2 * h, 2 * w, cout), 77, dtype=torch.int8, device="cuda")
    ops.i8_conv_transpose2x2(dev(x), n, h, w, cin, cout, dev(k).reshape(-1), dev(colsum), dev(mult), dev(bias_q), out)
    torch.cuda.synchronize()
    same_bytes(out, ref, f"convT {shape} {cin}->{cout}")


# ------------------------------------------------------------------- image block ----
@pytest.mark.parametrize("n,h,w,cin,cout", [(2, 8, 16, 3, 64), (1, 5, 7, 3, 96), (1, 40, 52, 4, 64)])
def test_i8_image_block(n, h, w, cin, cout):
    from unet_amd import ops
    x = U32(800, (n, h, w, cin), 0, 1)
    dk = U32(801, (3, 3, cin, 1), -0.5, 0.5)
    pw = U32(802, (1, 1, cin, cout), -0.5, 0.5)
    b = U32(803, (cout,), -0.1, 0.1)
    z = K.relu(K.pointwise(K.depthwise3x3(x, dk), pw) + b)
    s_out = np.float32(z.max() / 255.0)
    ref, _ = E.image_block(x, dk, pw[0, 0], b, s_out)
    non_vacuous(ref)
    f32 = lambda a: dev(np.asarray(a, np.float32)).reshape(-1)  # noqa: E731
    out = torch.full((n, h, w, cout), 77, dtype=torch.uint8, device="cuda")
    ops.i8_image_block(dev(x.astype(np.float32)), n, h, w, cin, f32(dk), cout, f32(pw), f32(b), float(s_out), out)
    torch.cuda.synchronize()
    got = out.cpu().numpy().astype(np.int64)
    diff = np.abs(got - ref.astype(np.int64))
    print("image block: elements differing", int((diff > 0).sum()), "of", diff.size, "max", int(diff.max()))
    assert diff.max() <= 1
    assert (diff > 0).sum() <= 1e-3 * diff.size


# -------------------------------------------------------------------------- head ----
@pytest.mark.parametrize("shape", [(2, 4, 4, 64), (1, 3, 5, 32), (1, 2, 2, 136)])
@pytest.mark.parametrize("ncls", [1, 3])
def test_i8_head(ncls, shape):
    from unet_amd import ops
    n, h, w, cin = shape
    x = np.random.default_rng(700).integers(0, 256, shape).astype(np.uint8)
    k = U32(701 + ncls, (cin, ncls), -0.5, 0.5) * np.float64(np.float32(2.0 / 255.0))  # the input scale folded in
    k = k.astype(np.float32).astype(np.float64)
    b = U32(702 + ncls, (ncls,), -0.5, 0.5)
    prob = torch.full((n, h, w, ncls), float("nan"), dtype=torch.float32, device="cuda")
    ops.i8_head(dev(x), n, h, w, cin, ncls, dev(k.astype(np.float32)).reshape(-1), dev(b.astype(np.float32)), prob)
    torch.cuda.synchronize()
    ref = E.head(x, k, b, ncls)
    amp = (K.pointwise(x.astype(np.float64), np.abs(k).reshape(1, 1, cin, ncls)) + np.abs(b)).max(axis=-1, keepdims=True)
    bound = (cin + 2) * EPS32 * amp + 1e-6
    err = np.abs(prob.cpu().numpy().astype(np.float64) - ref)
    print("head max err / bound", float((err / bound).max()))
    assert np.all(err <= bound), float((err / bound).max())
    assert ref.max() - ref.min() > 0.1
