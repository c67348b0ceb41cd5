"""ops.batch_affine_u8 (unet_batch_affine_u8, csrc/batch.hip) against its NumPy restatement
augment.affine_u8_reference: bitwise, inside guard bands (tests/fenced.py) -- every output element
written, no byte outside the output touched.  The shapes take the 16-byte-store kernel (w % 4 == 0,
more than one block per sample), the one-float-per-thread one (any other w, or a destination off its
alignment) and images of one row / one column; the records are the identity, the pure flip, large
rotations, a zoom-out that leaves most pixels outside, and exact half-pixel shifts (ties)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from fenced import Arena  # noqa: E402
from unet_amd.augment import Augment, affine_u8_reference  # noqa: E402
from unet_amd.data import gather_u8_reference  # noqa: E402

pytestmark = pytest.mark.gpu

# (n, h, w): 5x32x32 is the quad path (c = 1: 256 groups per sample, c = 3 likewise; 64x64 below: more than one block)
SHAPES = [(5, 32, 32), (3, 17, 23), (2, 6, 10), (2, 1, 4), (2, 5, 1)]
FILLS = [(False, 0.0), (True, 0.0), (True, 128.0)]


def _source(n, h, w, c):
    rng = np.random.default_rng(n * 1000 + h * 100 + w * 10 + c)
    return rng.integers(0, 256, (n, h, w, c), dtype=np.uint8)


def _records(h, w):
    """fp32 (k, 6): identity, pure flip, rotations by 90 / 137 / 180 / -45 degrees about the centre,
    a 3x zoom-out (most pixels outside), half-pixel shifts on both axes (order-0 ties), a random draw
    of every parameter with and without the flip, a map that sends everything far outside, and records
    with NaN and infinite entries."""
    size = (h, w)
    recs = [Augment.record64(np.eye(3), size, False), Augment.record64(np.eye(3), size, True)]
    for theta in (90, 137, 180, -45):
        recs.append(Augment.record64(Augment.matrix([theta, 0, 0, 0, 1, 1], size), size, theta == 137))
    recs.append(Augment.record64(Augment.matrix([0, 0, 0, 0, 3, 3], size), size, False))
    recs += [np.array([1, 0, 0.5, 0, 1, 0.5]), np.array([1, 0, -0.5, 0, 1, 1.5]), np.array([1, 0, 0, 0, -1, w - 1.5])]
    a = Augment(rotation_range=30, width_shift_range=0.2, height_shift_range=0.2, shear_range=15, zoom_range=(0.7, 1.3))
    table = a.draw(np.random.default_rng(h * 100 + w), 2)
    recs += [Augment.record64(Augment.matrix(table[0], size), size, False),
             Augment.record64(Augment.matrix(table[1], size), size, True)]
    recs.append(np.array([1, 0, 1e6, 0, 1, -1e6]))
    recs = np.stack(recs).astype(np.float32)
    # non-finite records read inside the sample like any other: a NaN offset, inf * 0 at r = 0 / q = 0,
    # infinite offsets of either sign, everything NaN
    nan, inf = np.float32("nan"), np.float32("inf")
    return np.concatenate([recs, np.array([[1, 0, nan, 0, 1, 0], [inf, 0, 0, 0, -inf, 0], [1, 0, inf, 0, 1, -inf],
                                           [nan] * 6, [0, 1, 0, nan, 0, 0.5]], np.float32)])


def _slots(n, b):
    """Repeats, out of order, and entries outside the cache on both sides (clamped on the device)."""
    s = np.random.default_rng(n * 31 + b).integers(0, n, b)
    s[-1] = s[0]
    s[1] = n + 3
    s[2] = -1
    s[3] = 2 ** 31 - 1
    s[4] = -2 ** 31
    return s.astype(np.int32)


def _run(src, slots, recs, order, fill, cval, skew_src=0, skew_dst=0, skew_rec=0):
    from unet_amd import ops
    arena = Arena()
    s = arena.inp(src, torch.uint8, "src")
    if skew_src:
        s = arena.skewed(s, skew_src, "src")
    t = arena.inp(np.asarray(slots, np.int32), torch.int32, "slots")
    x = arena.inp(recs, torch.float32, "xforms")
    if skew_rec:
        x = arena.skewed(x, skew_rec, "xforms")
    out = arena.empty((len(slots),) + src.shape[1:], torch.float32, "dst")
    if skew_dst:
        out = arena.skewed(out, skew_dst, "dst")
    assert ops.batch_affine_u8(s, t, x, out, order, fill, cval) is out
    arena.check()
    return out


@pytest.mark.parametrize("fill,cval", FILLS, ids=["nearest", "constant0", "constant128"])
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_batch_affine_bitwise(shape, c, order, fill, cval):
    n, h, w = shape
    src = _source(n, h, w, c)
    recs = _records(h, w)
    slots = _slots(n, len(recs))
    got = _run(src, slots, recs, order, fill, cval)
    ref = affine_u8_reference(src, slots, recs, order, fill, cval)
    assert torch.equal(got.cpu(), torch.from_numpy(ref))
    # the two sharp consequences: identity = the plain gather, pure flip = the mirrored gather
    plain = np.clip(slots[:2].astype(np.int64), 0, n - 1)
    assert np.array_equal(got[:2].cpu().numpy(), gather_u8_reference(src, [plain[0], ~plain[1]]))
    if fill and h > 1 and w > 1:  # the zoom-out and the far-away map really leave pixels outside
        assert (got[6].cpu().numpy() == np.float32(cval) / np.float32(255)).mean() > 0.5
        assert np.all(got[12].cpu().numpy() == np.float32(cval) / np.float32(255))
    assert torch.isfinite(got).all(), "a non-finite record must still read inside the sample"


@pytest.mark.parametrize("c", [1, 3])
def test_more_than_one_block_per_sample(c):
    """64 x 64: 1024 groups of 4 pixels per sample on the quad path, 4 blocks."""
    src = _source(2, 64, 64, c)
    recs = _records(64, 64)[2:8]
    slots = np.array([0, 1, 1, 0, 5, 0], np.int32)
    got = _run(src, slots, recs, 1, True, 128.0)
    assert torch.equal(got.cpu(), torch.from_numpy(affine_u8_reference(src, slots, recs, 1, True, 128.0)))


@pytest.mark.parametrize("skew_src,skew_dst,skew_rec", [(1, 0, 0), (2, 0, 4), (3, 0, 0), (0, 4, 0), (0, 8, 8), (1, 12, 12)])
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("shape", [(5, 32, 32, 3), (5, 32, 32, 1), (2, 1, 4, 3)], ids=lambda s: "x".join(map(str, s)))
def test_batch_affine_skewed_pointers(shape, order, skew_src, skew_dst, skew_rec):
    """w % 4 == 0 with the destination off 16 bytes: the one-float-per-thread kernel; a source at any
    byte and records at any word leave the quad path as it is."""
    n, h, w, c = shape
    src = _source(n, h, w, c)
    recs = _records(h, w)
    slots = _slots(n, len(recs))
    got = _run(src, slots, recs, order, True, 128.0, skew_src, skew_dst, skew_rec)
    assert torch.equal(got.cpu(), torch.from_numpy(affine_u8_reference(src, slots, recs, order, True, 128.0)))


def test_wrapper_checks():
    from unet_amd import ops
    dev = "cuda:0"
    src = torch.zeros((2, 4, 8, 3), dtype=torch.uint8, device=dev)
    slots = torch.zeros(2, dtype=torch.int32, device=dev)
    xf = torch.zeros((2, 6), device=dev)
    out = torch.empty((2, 4, 8, 3), device=dev)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.batch_affine_u8(src.cpu(), slots, xf, out)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.batch_affine_u8(src, slots, xf.cpu(), out)
    with pytest.raises(TypeError):
        ops.batch_affine_u8(src.float(), slots, xf, out)
    with pytest.raises(TypeError):
        ops.batch_affine_u8(src, slots.long(), xf, out)
    with pytest.raises(TypeError):
        ops.batch_affine_u8(src, slots, xf.double(), out)
    with pytest.raises(ValueError, match="1 or 3"):
        ops.batch_affine_u8(src[..., :2].contiguous(), slots, xf, out)
    with pytest.raises(ValueError, match="xforms: expected"):
        ops.batch_affine_u8(src, slots, xf[:1], out)
    with pytest.raises(ValueError, match="xforms: expected"):
        ops.batch_affine_u8(src, slots, torch.zeros((2, 5), device=dev), out)
    with pytest.raises(ValueError, match="out: expected"):
        ops.batch_affine_u8(src, slots, xf, out[:1])
    with pytest.raises(ValueError, match="order"):
        ops.batch_affine_u8(src, slots, xf, out, order=2)
    with pytest.raises(ValueError, match="contiguous"):
        ops.batch_affine_u8(src, slots, xf, torch.empty((2, 4, 3, 8), device=dev).permute(0, 1, 3, 2))


def test_entry_point_refusals():
    """The C entry point refuses bad sizes, channel counts, orders and alignments with a message and
    writes nothing (real device buffers: were a check missing, the launch would stay inside them)."""
    from ctypes import c_void_p
    from unet_amd import _lib
    lib = _lib.load()
    f = lib.unet_batch_affine_u8
    f.restype, f.argtypes = _lib.SIGNATURES["unet_batch_affine_u8"]
    arena = Arena()
    src = arena.inp(np.zeros((2, 4, 8, 3), np.uint8), torch.uint8, "src")
    slots = arena.inp(np.zeros(4, np.int32), torch.int32, "slots")
    xf = arena.inp(np.tile(np.array([1, 0, 0, 0, 1, 0], np.float32), (4, 1)), torch.float32, "xforms")
    out = arena.empty((2, 4, 8, 3), torch.float32, "dst", output=False)
    s, t, x, d = (c_void_p(v.data_ptr()) for v in (src, slots, xf, out))
    st = c_void_p(torch.cuda.current_stream().cuda_stream)
    for args, msg in [((s, 2, 4, 8, 2, t, x, 2, 1, 0, 0.0, d, st), b"c must be 1 or 3"),
                      ((s, 2, 4, 8, 3, t, x, 2, 2, 0, 0.0, d, st), b"order must be 0 or 1"),
                      ((s, 2, 4, 8, 3, t, x, 2, -1, 0, 0.0, d, st), b"order must be 0 or 1"),
                      ((s, 2, 4, 8, 3, t, x, 2, 1, 0, 0.0, c_void_p(d.value + 2), st), b"4-byte aligned"),
                      ((s, 2, 4, 8, 3, c_void_p(t.value + 1), x, 2, 1, 0, 0.0, d, st), b"4-byte aligned"),
                      ((s, 2, 4, 8, 3, t, c_void_p(x.value + 2), 2, 1, 0, 0.0, d, st), b"4-byte aligned"),
                      ((s, 0, 4, 8, 3, t, x, 2, 1, 0, 0.0, d, st), b"positive"),
                      ((s, 2, 0, 8, 3, t, x, 2, 1, 0, 0.0, d, st), b"positive"),
                      ((s, 2, 4, 0, 3, t, x, 2, 1, 0, 0.0, d, st), b"positive"),
                      ((s, 2, 4, 8, 3, t, x, 0, 1, 0, 0.0, d, st), b"positive"),
                      ((s, 2, 65536, 32768, 1, t, x, 2, 1, 0, 0.0, d, st), b"exceeds 2^31"),
                      ((None, 2, 4, 8, 3, t, x, 2, 1, 0, 0.0, d, st), b"null pointer"),
                      ((s, 2, 4, 8, 3, None, x, 2, 1, 0, 0.0, d, st), b"null pointer"),
                      ((s, 2, 4, 8, 3, t, None, 2, 1, 0, 0.0, d, st), b"null pointer"),
                      ((s, 2, 4, 8, 3, t, x, 2, 1, 0, 0.0, None, st), b"null pointer")]:
        assert f(*args) < 0
        assert msg in lib.unet_last_error(), lib.unet_last_error()
    torch.cuda.synchronize()
    assert arena.is_untouched(out)
    arena.check()
