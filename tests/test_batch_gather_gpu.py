"""ops.batch_gather_u8 (unet_batch_gather_u8, csrc/batch.hip) against its NumPy restatement
data.gather_u8_reference: bitwise, inside guard bands (tests/fenced.py) -- every output element
written, no byte outside the output touched.  The shapes take the 16-byte-store kernel (w % 4 == 0),
the byte-wise one (any other w, or a source / destination off its alignment), sample sizes that are
no multiple of 4 bytes, and more than one block per sample."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from fenced import Arena  # noqa: E402
from unet_amd.data import gather_u8_reference  # noqa: E402

pytestmark = pytest.mark.gpu

# (n, h, w, c, b); 4x3x5x1: 15 bytes per sample, so sample bases lose their dword alignment; 3x8x64x3: two blocks
# per sample on the 16-byte-store kernel
SHAPES = [(5, 3, 5, 3, 7), (3, 4, 16, 1, 4), (4, 2, 37, 3, 5), (2, 16, 16, 3, 3), (6, 32, 32, 1, 6), (4, 3, 5, 1, 6),
          (3, 8, 64, 3, 4)]


def _source(n, h, w, c):
    rng = np.random.default_rng(n * 1000 + h * 100 + w * 10 + c)
    src = rng.integers(0, 256, (n, h, w, c), dtype=np.uint8)
    flat = src.reshape(-1)
    if flat.size >= 256:
        flat[:256] = rng.permutation(256).astype(np.uint8)
    return src


def _tables(n, b):
    """Mixed (repeated, out of order, flipped and not), all flipped, one entry, entries past the cache."""
    rng = np.random.default_rng(n * 31 + b)
    s = rng.integers(0, n, b)
    s[-1] = s[0]  # a repeat, whatever the draw
    mixed = np.where(np.arange(b) % 2 == 1, ~s, s)
    return {"mixed": mixed, "flipped": ~np.sort(s)[::-1], "one": np.array([~(n - 1)]), "first": np.array([0]),
            "clamped": np.array([n, ~n, 2 ** 31 - 1, -2 ** 31][:max(b, 2)])}


def _run(src, slots, skew_src=0, skew_dst=0):
    from unet_amd import ops
    arena = Arena()
    s = arena.inp(src, torch.uint8, "src")
    if skew_src:
        s = arena.skewed(s, skew_src, "src")
    t = arena.inp(np.asarray(slots, np.int32), torch.int32, "slots")
    out = arena.empty((len(slots),) + src.shape[1:], torch.float32, "dst")
    if skew_dst:
        out = arena.skewed(out, skew_dst, "dst")
    assert ops.batch_gather_u8(s, t, out) is out
    arena.check()
    return out


@pytest.mark.parametrize("table", ["mixed", "flipped", "one", "first", "clamped"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_batch_gather_bitwise(shape, table):
    n, h, w, c, b = shape
    src = _source(n, h, w, c)
    slots = _tables(n, b)[table]
    got = _run(src, slots)
    ref = torch.from_numpy(gather_u8_reference(src, slots))
    assert torch.equal(got.cpu(), ref)


@pytest.mark.parametrize("skew_src,skew_dst", [(1, 0), (2, 0), (3, 0), (0, 4), (0, 8), (1, 12)])
@pytest.mark.parametrize("shape", [(2, 16, 16, 3, 3), (3, 4, 16, 1, 4)], ids=lambda s: "x".join(map(str, s)))
def test_batch_gather_skewed_pointers(shape, skew_src, skew_dst):
    """w % 4 == 0 with the source off a dword or the destination off 16 bytes: the byte-wise kernel."""
    n, h, w, c, b = shape
    src = _source(n, h, w, c)
    slots = _tables(n, b)["mixed"]
    got = _run(src, slots, skew_src, skew_dst)
    assert torch.equal(got.cpu(), torch.from_numpy(gather_u8_reference(src, slots)))


@pytest.mark.parametrize("w", [64, 63])
def test_every_byte_value_is_correctly_rounded(w):
    src = np.zeros((1, 5, w, 1), np.uint8)
    src.reshape(-1)[:256] = np.arange(256, dtype=np.uint8)
    got = _run(src, [0, ~0]).cpu().numpy()
    want = np.arange(256, dtype=np.float32) / np.float32(255)
    assert np.array_equal(got[0].reshape(-1)[:256], want)
    assert np.array_equal(got[1][:, ::-1].reshape(-1)[:256], want)


def test_wrapper_checks():
    from unet_amd import ops
    dev = "cuda:0"
    src = torch.zeros((2, 4, 8, 3), dtype=torch.uint8, device=dev)
    slots = torch.zeros(2, dtype=torch.int32, device=dev)
    out = torch.empty((2, 4, 8, 3), device=dev)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.batch_gather_u8(src.cpu(), slots, out)
    with pytest.raises(TypeError):
        ops.batch_gather_u8(src.float(), slots, out)
    with pytest.raises(TypeError):
        ops.batch_gather_u8(src, slots.long(), out)
    with pytest.raises(ValueError, match="1 or 3"):
        ops.batch_gather_u8(src[..., :2].contiguous(), slots, out)
    with pytest.raises(ValueError, match="out: expected"):
        ops.batch_gather_u8(src, slots, out[:1])
    with pytest.raises(ValueError, match="contiguous"):
        ops.batch_gather_u8(src, slots, torch.empty((2, 4, 3, 8), device=dev).permute(0, 1, 3, 2))


def test_entry_point_refusals():
    """The C entry point refuses bad sizes, channel counts and alignments with a message and
    writes nothing (real device buffers: were a check missing, the launch would stay inside them)."""
    from ctypes import c_void_p
    from unet_amd import _lib
    lib = _lib.load()
    arena = Arena()
    src = arena.inp(np.zeros((2, 4, 8, 3), np.uint8), torch.uint8, "src")
    slots = arena.inp(np.zeros(4, np.int32), torch.int32, "slots")
    out = arena.empty((2, 4, 8, 3), torch.float32, "dst", output=False)
    s, t, d = (c_void_p(v.data_ptr()) for v in (src, slots, out))
    st = c_void_p(torch.cuda.current_stream().cuda_stream)
    for args, msg in [((s, 2, 4, 8, 2, t, 2, d, st), b"c must be 1 or 3"),
                      ((s, 2, 4, 8, 3, t, 2, c_void_p(d.value + 2), st), b"4-byte aligned"),
                      ((s, 2, 4, 8, 3, c_void_p(t.value + 1), 2, d, st), b"4-byte aligned"),
                      ((s, 0, 4, 8, 3, t, 2, d, st), b"positive"),
                      ((s, 2, 4, 0, 3, t, 2, d, st), b"positive"),
                      ((s, 2, 4, 8, 3, t, 0, d, st), b"positive"),
                      ((s, 2, 4, 8, 3, None, 2, d, st), b"null pointer"),
                      ((s, 2, 4, 8, 3, t, 2, None, st), b"null pointer")]:
        assert lib.unet_batch_gather_u8(*args) < 0
        assert msg in lib.unet_last_error(), lib.unet_last_error()
    torch.cuda.synchronize()
    assert arena.is_untouched(out)
    arena.check()
