"""Random affine augmentation on the host (unet_amd/augment.py): the settings object, the epoch's
draw, the transform records with the flip folded in, the NumPy restatement of the warp kernel held
to scipy.ndimage.affine_transform, and the two loaders' bitwise agreement with it in place of the
device."""
import os

import numpy as np
import pytest
import scipy.ndimage as ndi
from PIL import Image

from unet_amd.augment import Augment, affine_u8_reference
from unet_amd.data import PairLoader, gather_u8_reference, global_batches
from unet_amd.device_data import DevicePairLoader

IDENTITY = np.array([1, 0, 0, 0, 1, 0], np.float32)
EPS = 2.0 ** -24  # unit roundoff of fp32


def _flip_record(w):
    return np.array([1, 0, 0, 0, -1, w - 1], np.float32)


def _noise(n, h, w, c, seed=0):
    return np.random.default_rng(seed + 1000 * h + 10 * w + c).integers(0, 256, (n, h, w, c), dtype=np.uint8)


# ------------------------------------------------------------------------------- settings ---
def test_defaults_are_off():
    a = Augment()
    assert not a.active and a.fill_mode == "nearest" and a.cval == 0.0 and (a.frame_order, a.mask_order) == (1, 1)
    assert a.zoom_range == (1.0, 1.0) and not a.fill_constant
    assert Augment(zoom_range=(1.0, 1.0)).active is False
    for kw in (dict(rotation_range=1), dict(width_shift_range=0.1), dict(height_shift_range=0.1),
               dict(shear_range=2), dict(zoom_range=0.1), dict(zoom_range=(0.9, 1.0))):
        assert Augment(**kw).active, kw
    assert Augment(zoom_range=0.25).zoom_range == (0.75, 1.25)
    assert Augment(fill_mode="constant", cval=128).fill_constant


@pytest.mark.parametrize("kw", [
    dict(rotation_range=-1), dict(shear_range=-0.5), dict(width_shift_range=-0.1), dict(height_shift_range=-0.1),
    dict(width_shift_range=1.0), dict(height_shift_range=12), dict(width_shift_range=[-2, 0, 2]),
    dict(zoom_range=-0.1), dict(zoom_range=1.0), dict(zoom_range=(0.0, 1.0)), dict(zoom_range=(1.2, 0.8)),
    dict(zoom_range=(1.0, 1.1, 1.2)), dict(fill_mode="reflect"), dict(fill_mode="wrap"), dict(frame_order=2),
    dict(mask_order=3), dict(mask_order=-1), dict(frame_order=True), dict(rotation_range=float("nan")),
    dict(cval=float("inf"))])
def test_bad_arguments_are_refused(kw):
    with pytest.raises((ValueError, TypeError)):
        Augment(**kw)


# ----------------------------------------------------------------------------------- draws ---
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """12 PNG pairs of 40 x 30, frames of noise and masks with every grey level."""
    root = str(tmp_path_factory.mktemp("pairs"))
    fr, mk = os.path.join(root, "frames"), os.path.join(root, "masks")
    os.makedirs(fr)
    os.makedirs(mk)
    rng = np.random.default_rng(0)
    for i in range(12):
        Image.fromarray(rng.integers(0, 256, (30, 40, 3), dtype=np.uint8)).save(os.path.join(fr, f"f{i:03d}.png"))
        m = np.zeros((30, 40), np.uint8)
        m[5:5 + i % 7 + 3, 4:20] = 255
        m[20:25, 2:30] = rng.integers(0, 256, (5, 28), dtype=np.uint8)
        Image.fromarray(m).save(os.path.join(mk, f"f{i:03d}.png"))
    return fr, mk


AUG = dict(rotation_range=30, width_shift_range=0.2, height_shift_range=0.2, shear_range=15, zoom_range=(0.7, 1.3))


class _Spy(PairLoader):
    """Records what __iter__ hands to load(): the shard's indices, the epoch's flips, the records."""

    def load(self, idx, flips, records=None):
        self.seen.append((np.array(idx), np.array(flips), None if records is None else np.array(records)))
        z = np.zeros((len(idx), 1, 1, 1), np.float32)
        return z, z


def _seen(tree, batches, **kw):
    ld = _Spy(*tree, (16, 16), 4, seed=2301, shuffle=True, horizontal_flip=True, workers=1, **kw)
    ld.seen = []
    for _, _ in zip(range(batches), iter(ld)):
        pass
    return ld.seen


def test_the_draw_leaves_order_and_flips_alone(tree):
    plain = _seen(tree, 9)
    off = _seen(tree, 9, augment=Augment())
    on = _seen(tree, 9, augment=Augment(**AUG))
    for p, o, a in zip(plain, off, on):
        assert o[2] is None and p[2] is None, "all ranges 0 is today's path"
        assert np.array_equal(p[0], a[0]) and np.array_equal(p[1], a[1])
        assert np.array_equal(p[0], o[0]) and np.array_equal(p[1], o[1])
        assert a[2].dtype == np.float32 and a[2].shape == (4, 6)
    # epochs differ, a sample keeps its parameters within one
    assert not np.array_equal(on[0][2], on[3][2])


def test_the_table_is_one_draw_after_flips_and_indexed_by_sample(tree):
    a = Augment(**AUG)
    (idx, flips, recs), = _seen(tree, 1, augment=a)
    rng = np.random.default_rng(2301)
    order = rng.permutation(12)
    fl = rng.random(12) < 0.5
    u = rng.random((12, 6))
    assert np.array_equal(idx, order[:4]) and np.array_equal(flips, fl)
    table = a.draw(np.random.default_rng(5), 12)
    assert table.shape == (12, 6) and table.dtype == np.float64
    assert np.all(np.abs(table[:, 0]) <= 30) and np.all(np.abs(table[:, 1:3]) <= 0.2) and np.all(np.abs(table[:, 3]) <= 15)
    assert np.all((table[:, 4:] >= 0.7) & (table[:, 4:] <= 1.3))
    want = np.empty((12, 6))
    want[:, 0], want[:, 1], want[:, 2], want[:, 3] = ((2 * u[:, k] - 1) * r for k, r in enumerate((30, 0.2, 0.2, 15)))
    want[:, 4:] = 0.7 + u[:, 4:] * (1.3 - 0.7)
    assert np.array_equal(recs, a.records(want, idx, fl, (16, 16)))


def test_all_ranks_draw_the_same_table(tree):
    whole = _seen(tree, 3, augment=Augment(**AUG))
    for world in (2, 3):
        parts = [_seen(tree, 3, augment=Augment(**AUG), rank=r, world=world) for r in range(world)]
        for k in range(3):
            assert np.array_equal(np.concatenate([p[k][0] for p in parts]), whole[k][0])
            assert np.array_equal(np.concatenate([p[k][2] for p in parts]), whole[k][2])


def test_validation_style_loader_is_never_augmented(tree):
    for s in _seen(tree, 3):
        assert s[2] is None


# --------------------------------------------------------------------------------- records ---
def test_matrix_is_keras_composition():
    """Pure cases of R @ T @ S @ Z about the centre (h/2 - 0.5, w/2 - 0.5)."""
    h, w = 9, 14
    c = np.array([h / 2 - 0.5, w / 2 - 0.5, 1.0])
    for p in ([25, 0, 0, 0, 1, 1], [0, 0.1, -0.2, 0, 1, 1], [0, 0, 0, 10, 1, 1], [0, 0, 0, 0, 0.8, 1.25],
              [-17, 0.15, 0.05, 7, 1.1, 0.9]):
        m = Augment.matrix(p, (h, w))
        th, s = np.deg2rad(p[0]), np.deg2rad(p[3])
        rot = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]])
        sh = np.array([[1, 0, p[1] * h], [0, 1, p[2] * w], [0, 0, 1]])
        shear = np.array([[1, -np.sin(s), 0], [0, np.cos(s), 0], [0, 0, 1]])
        want = rot @ sh @ shear @ np.diag([p[4], p[5], 1.0])
        for pt in ([0, 0, 1], [3, 11, 1], [8, 13, 1]):
            v = np.array(pt, float)
            assert np.allclose(m @ v, want @ (v - c + [0, 0, 1]) + c - [0, 0, 1], atol=1e-12)
    assert np.allclose(Augment.matrix([0, 0, 0, 0, 1, 1], (h, w)), np.eye(3), atol=1e-15)
    # a pure shift moves the sampling point by tx rows, ty columns
    assert np.allclose(Augment.matrix([0, 0.5, 0.25, 0, 1, 1], (8, 16)) @ [0, 0, 1], [4, 4, 1])


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("fill", [False, True])
def test_folded_flip_is_warp_then_mirror(order, fill):
    h, w = 9, 14
    src = _noise(2, h, w, 3)
    rng = np.random.default_rng(4)
    a = Augment(**AUG)
    table = a.draw(rng, 6)
    for k in range(6):
        m = Augment.matrix(table[k], (h, w))
        plain = Augment.record64(m, (h, w), False).astype(np.float32)
        flipped = Augment.record64(m, (h, w), True).astype(np.float32)
        # the fold is exact in float64; in fp32 it is the SAME map only where plain's entries are
        # themselves folded from fp32, so the identity is stated on the float64 -> fp32 record of
        # the mirrored map: q -> w - 1 - q negates the column coefficients and moves the offsets
        assert np.array_equal(flipped[[1, 4]], -plain[[1, 4]]) and np.array_equal(flipped[[0, 3]], plain[[0, 3]])
        r64 = Augment.record64(m, (h, w), False)
        assert flipped[2] == np.float32(r64[2] + r64[1] * (w - 1)) and flipped[5] == np.float32(r64[5] + r64[4] * (w - 1))
    # bitwise warp-then-mirror where the fold loses nothing: records whose numbers are dyadic
    for rec in ([1, 0, 0.5, 0, 1, -1.25], [0.5, 0.25, 1, -0.25, 0.75, 3], [0, 1, 0, 1, 0, 0], [1.5, 0, -2, 0, 1.5, -3.5]):
        m = np.array([rec[:3], rec[3:], [0, 0, 1]], float)
        plain = Augment.record64(m, (h, w), False).astype(np.float32)
        flipped = Augment.record64(m, (h, w), True).astype(np.float32)
        warped = affine_u8_reference(src, [1], plain[None], order, fill, 77.0)
        folded = affine_u8_reference(src, [1], flipped[None], order, fill, 77.0)
        assert np.array_equal(folded, warped[:, :, ::-1])


@pytest.mark.parametrize("shape", [(1, 4), (5, 1), (17, 23), (8, 16), (1, 1)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("c", [1, 3])
def test_identity_and_flip_records_equal_the_gather(shape, c):
    h, w = shape
    src = _noise(3, h, w, c)
    slots = [2, 0, 1, 1, 7, -3]  # the last two are clamped into the cache
    plain = np.clip(slots, 0, 2)
    for order in (0, 1):
        for fill in (False, True):
            got = affine_u8_reference(src, slots, np.tile(IDENTITY, (6, 1)), order, fill, 200.0)
            assert got.dtype == np.float32
            assert np.array_equal(got, gather_u8_reference(src, plain))
            got = affine_u8_reference(src, slots, np.tile(_flip_record(w), (6, 1)), order, fill, 200.0)
            assert np.array_equal(got, gather_u8_reference(src, ~plain))
    assert np.array_equal(Augment.record64(np.eye(3), (h, w), True).astype(np.float32), _flip_record(w))


def test_half_pixel_ties_and_the_outside_rule():
    """A shift of exactly half a pixel: order 0 takes floor(s + 0.5), the later pixel; order 1 the
    mean of two neighbours.  A point exactly on the last row / column is inside."""
    src = np.arange(24, dtype=np.uint8).reshape(1, 4, 6, 1) * 10
    rec = np.array([[1, 0, 0.5, 0, 1, 0.5]], np.float32)
    f = src[0, :, :, 0].astype(np.float32)
    got0 = affine_u8_reference(src, [0], rec, 0)[0, :, :, 0] * 255
    assert np.allclose(got0[:3, :5], f[1:, 1:])
    assert np.allclose(got0[3, :5], f[3, 1:]) and np.allclose(got0[:3, 5], f[1:, 5])  # clamped border
    got1 = affine_u8_reference(src, [0], rec, 1)[0, :, :, 0] * 255
    assert np.allclose(got1[:3, :5], (f[:3, :5] + f[:3, 1:] + f[1:, :5] + f[1:, 1:]) / 4, atol=1e-4)
    fill = affine_u8_reference(src, [0], rec, 1, True, 255.0)[0, :, :, 0]
    assert np.all(fill[3, :] == 1.0) and np.all(fill[:, 5] == 1.0) and np.all(fill[:3, :5] < 1.0)
    on_edge = affine_u8_reference(src, [0], np.array([[1, 0, 1, 0, 1, 1]], np.float32), 1, True, 255.0)[0, :, :, 0]
    assert np.array_equal(on_edge[:3, :5] * 255, f[1:, 1:]) and np.all(on_edge[3, :] == 1.0)


# ----------------------------------------------------------------------- against scipy ---
SCIPY_SIZES = [(32, 32), (17, 23), (64, 48)]
TRANSFORMS = 40
LEFT_OUT_CAP = 0.01


def coordinate_bound(rec64, h, w):
    """How far the kernel's fp32 source coordinate can lie from the float64 one, per axis, from the
    float64 record alone.  With u = 2^-24 and the row coordinate sy = (m00 r + m01 q) + o0:
      the three record entries are rounded once each:      u (|m00| r + |m01| q + |o0|)
      the two products are rounded:                        u (|m00| r + |m01| q)
      their sum is rounded:                                u |m00 r + m01 q| <= u (|m00| r + |m01| q)
      the sum with o0 is rounded:                          u |sy|            <= u (|m00| r + |m01| q + |o0|)
    (r, q are integers below 2^24: their conversion is exact), in all
      u (4 (|m00| r + |m01| q) + 2 |o0|) <= u (4 (|m00| + |m01|) (max(h, w) - 1) + 2 |o0|),
    times 1.01 for the second-order terms.  |o| itself is at most about 2 max(h, w) max|m| here, so
    this is a small multiple (about 12) of 2^-24 max(h, w) max|m|.  The clamp to [0, n-1] moves both
    coordinates alike and does not widen it."""
    L = max(h, w) - 1
    rows = EPS * (4 * (abs(rec64[0]) + abs(rec64[1])) * L + 2 * abs(rec64[2]))
    cols = EPS * (4 * (abs(rec64[3]) + abs(rec64[4])) * L + 2 * abs(rec64[5]))
    return 1.01 * max(rows, cols)


def value_tolerance(cb, order):
    """Order 1: bilinear interpolation moves by at most one neighbour difference per unit of
    coordinate on each axis, and a neighbour difference is at most 1.0 of full scale: 2 axes x cb x
    1.0.  On top, the interpolation's own fp32 arithmetic (three lerps of two roundings each on
    values <= 255, and the division): 8 u of full scale.  Order 0 away from its decision points picks
    the same byte: what is left is the one fp32 rounding of byte / 255 <= 1, u."""
    return 2 * cb * 1.0 + 8 * EPS if order == 1 else EPS


@pytest.mark.parametrize("fill_mode", ["nearest", "constant"])
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("size", SCIPY_SIZES, ids=lambda s: "x".join(map(str, s)))
def test_restatement_against_scipy(size, c, order, fill_mode):
    """affine_u8_reference against scipy.ndimage.affine_transform fed the float64 matrix, per channel,
    then / 255, over 40 random transforms (+-30 degrees, shifts +-0.2, shear +-15 degrees, zoom
    [0.7, 1.3], half of them flipped) per case.  Tolerance: value_tolerance(coordinate_bound(...), order),
    derived in those two docstrings from the record rounding and the three fp32 roundings of a
    coordinate, about 1e-4 of full scale at 64 x 48; not tuned on the code's output.  Pixels are left
    out only where a float64 coordinate lies within coordinate_bound of a decision point (0 or n-1
    for fill_mode constant, k + 0.5 for order 0), decided from the float64 matrix alone; at most 1 %
    of a case's pixels may be."""
    h, w = size
    a = Augment(fill_mode=fill_mode, cval=37.0, **AUG)
    rng = np.random.default_rng(20 + h)
    src = rng.integers(0, 256, (TRANSFORMS, h, w, c), dtype=np.uint8)
    table = a.draw(rng, TRANSFORMS)
    flips = rng.random(TRANSFORMS) < 0.5
    recs = a.records(table, np.arange(TRANSFORMS), flips, size)
    got = affine_u8_reference(src, np.arange(TRANSFORMS), recs, order, a.fill_constant, a.cval)
    rr, qq = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    left_out = total = 0
    worst = 0.0
    for k in range(TRANSFORMS):
        r64 = Augment.record64(Augment.matrix(table[k], size), size, bool(flips[k]))
        cb = coordinate_bound(r64, h, w)
        tol = value_tolerance(cb, order)
        want = np.stack([ndi.affine_transform(src[k, :, :, ch].astype(np.float64), r64[[0, 1, 3, 4]].reshape(2, 2),
                                              offset=r64[[2, 5]], order=order, mode=fill_mode, cval=a.cval)
                         for ch in range(c)], -1) / 255.0
        sy = r64[0] * rr + r64[1] * qq + r64[2]
        sx = r64[3] * rr + r64[4] * qq + r64[5]
        skip = np.zeros((h, w), bool)
        for s, n in ((sy, h), (sx, w)):
            if fill_mode == "constant":
                skip |= (np.abs(s) <= cb) | (np.abs(s - (n - 1)) <= cb)
            if order == 0:
                t = np.clip(s, 0, n - 1)
                skip |= np.abs(t - np.floor(t) - 0.5) <= cb
        left_out += int(skip.sum())
        total += h * w
        err = np.abs(got[k].astype(np.float64) - want)[~skip]
        worst = max(worst, float(err.max(initial=0.0)))
        assert err.max(initial=0.0) <= tol, (k, float(err.max()), tol)
    print(f"{h}x{w}x{c} order {order} {fill_mode}: max error {worst:.3g}, left out {left_out} of {total}")
    assert left_out <= LEFT_OUT_CAP * total, (left_out, total)


# --------------------------------------------------------------------------------- loaders ---
N, SIZE, BATCH = 12, (16, 16), 4
PAIR_BYTES = SIZE[0] * SIZE[1] * 4


@pytest.mark.parametrize("budget", [N * PAIR_BYTES, 3 * PAIR_BYTES], ids=["full", "three"])
@pytest.mark.parametrize("kw", [dict(), dict(fill_mode="constant", cval=128.0, mask_order=0)], ids=["nearest", "constant"])
def test_device_loader_on_numpy_buffers_equals_pair_loader(tree, budget, kw):
    args = dict(seed=2301, shuffle=True, horizontal_flip=True, workers=2)
    host = PairLoader(*tree, SIZE, BATCH, augment=Augment(**AUG, **kw), **args)
    dev = DevicePairLoader(*tree, SIZE, BATCH, device=None, device_cache_bytes=budget, augment=Augment(**AUG, **kw), **args)
    plain = PairLoader(*tree, SIZE, BATCH, **args)
    assert dev.book.resident == min(N, budget // PAIR_BYTES)
    hi, di, pi = iter(host), iter(dev), iter(plain)
    changed = 0
    for k in range(2 * len(list(global_batches(N, BATCH, 1)))):
        a, b, p = next(hi), next(di), next(pi)
        assert a.global_size == b.global_size == BATCH
        assert b[0].dtype == np.float32 and b[0].shape == (BATCH,) + SIZE + (3,) and b[1].shape == (BATCH,) + SIZE + (1,)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), k
        changed += not np.array_equal(a[0], p[0])
    assert changed == 6, "augmentation must change the batches"
    # the slot table carries no flips: the flip is in the record
    assert all(e >= 0 for e in dev.book.plan(np.arange(4), [False] * 4).entries)


def test_mask_order_0_keeps_the_masks_grey_levels(tree):
    args = dict(seed=2301, shuffle=False, horizontal_flip=True, workers=1)
    levels = set()
    for _, s in zip(range(3), iter(PairLoader(*tree, SIZE, BATCH, **args))):
        levels |= set(np.unique(s[1]))
    ld = PairLoader(*tree, SIZE, BATCH, augment=Augment(mask_order=0, **AUG), **args)
    for _, s in zip(range(3), iter(ld)):
        assert set(np.unique(s[1])) <= levels
