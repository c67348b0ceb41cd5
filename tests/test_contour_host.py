"""The closed form behind the device contour kernels (include/unet_hip.h, "Device-side
largest-contour box") against the host tracer of unet_amd/imageproc.py, without a GPU:
imageproc.external_contour_stats_filled gives the same ordered list of (area, boundingRect) as
external_contours + contour_area + bounding_rect, and largest_external_contour_filled the same
answer as largest_external_contour.  Exact equality everywhere.

mask_cases(), random_masks() and blob_masks() are also what tests/test_contour_gpu.py feeds the
kernels: this file is the single source of the masks."""
import ctypes
import functools
import os

import numpy as np
import pytest
from PIL import Image
from scipy import ndimage

from unet_amd.imageproc import (bounding_rect, contour_area, external_contour_stats_filled, external_contours,
                                largest_external_contour, largest_external_contour_filled)

HERE = os.path.dirname(os.path.abspath(__file__))
USAGE = os.path.join(HERE, "golden", "samples", "usage")
TILE = 32  # csrc/contour.hip labels TILE x TILE tiles; the shapes below sit on, over and under it
TILE_SHAPES = ((64, 64), (65, 129), (63, 31))
SAMPLE_EXPECT = {"brazil_passport": (128961.0, (53, 274, 468, 378)), "chile_id_card": (128625.0, (38, 296, 466, 300))}


# ------------------------------------------------------------------------------- the masks ---
def _z(h, w):
    return np.zeros((h, w), np.uint8)


def _ring(m, y0, x0, y1, x1, v=255):
    """The one-pixel outline of rows y0..y1, columns x0..x1 (inclusive)."""
    m[y0, x0:x1 + 1] = v
    m[y1, x0:x1 + 1] = v
    m[y0:y1 + 1, x0] = v
    m[y0:y1 + 1, x1] = v
    return m


def _line(h, w, flip):
    n = max(h, w)
    ys = np.rint(np.linspace(0, h - 1, n)).astype(int)
    xs = np.rint(np.linspace(0, w - 1, n)).astype(int)
    m = _z(h, w)
    m[ys, (w - 1 - xs) if flip else xs] = 255
    return m


def _serpentine(h, w):
    m = _z(h, w)
    m[0::2, :] = 255
    for r in range(1, h, 2):
        m[r, w - 1 if (r // 2) % 2 == 0 else 0] = 255
    return m


def _spiral(h, w):
    """A one-pixel path that winds inwards from the top left corner, one pixel of gap between turns."""
    m = _z(h, w)
    dirs = ((0, 1), (1, 0), (0, -1), (-1, 0))
    y = x = d = 0
    m[0, 0] = 255
    while True:
        for _ in range(2):
            dy, dx = dirs[d]
            ny, nx, fy, fx = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if 0 <= ny < h and 0 <= nx < w and not m[ny, nx] and not (0 <= fy < h and 0 <= fx < w and m[fy, fx]):
                y, x = ny, nx
                m[y, x] = 255
                break
            d = (d + 1) % 4
        else:
            return m


def _comb(h, w):
    m = _z(h, w)
    m[0, :] = 255
    m[:, 0::2] = 255
    return m


def _plus(h, w):
    m = _z(h, w)
    m[h // 2, :] = 255
    m[:, w // 2] = 255
    return m


@functools.lru_cache(maxsize=None)
def mask_cases():
    """[(name, uint8 mask)]: the smallest shapes at which the kernels can go wrong."""
    c = []
    # degenerate sizes
    c.append(("1x1_fg", np.full((1, 1), 255, np.uint8)))
    c.append(("1x1_bg", _z(1, 1)))
    gaps = np.array([[255, 0, 255, 255, 0, 0, 255]], np.uint8)
    c.append(("1x7_gaps", gaps))
    c.append(("7x1_gaps", np.ascontiguousarray(gaps.T)))
    c.append(("2x2_full", np.full((2, 2), 255, np.uint8)))
    c.append(("33x65_zeros", _z(33, 65)))
    c.append(("33x65_full", np.full((33, 65), 255, np.uint8)))
    # tile boundaries in both directions: exact multiples, one over, one under
    for h, w in TILE_SHAPES:
        s = f"{h}x{w}"
        c.append((f"{s}_full", np.full((h, w), 255, np.uint8)))
        c.append((f"{s}_plus", _plus(h, w)))
        c.append((f"{s}_diagonal", _line(h, w, False)))
        c.append((f"{s}_antidiagonal", _line(h, w, True)))
        c.append((f"{s}_serpentine", _serpentine(h, w)))
        c.append((f"{s}_serpentine_t", np.ascontiguousarray(_serpentine(w, h).T)))
        c.append((f"{s}_spiral", _spiral(h, w)))
        c.append((f"{s}_comb", _comb(h, w)))
    # topology (40 x 44: every shape crosses the tile seams at 32)
    c.append(("ring", _ring(_z(40, 44), 4, 5, 36, 40)))
    c.append(("ring_on_frame", _ring(_z(40, 44), 4, 0, 36, 38)))
    m = _ring(_z(40, 44), 4, 5, 36, 40)
    m[15:22, 16:30] = 255
    c.append(("ring_blob_in_hole", m))
    m = _ring(_z(40, 44), 2, 2, 38, 41)
    _ring(m, 8, 8, 34, 36)
    m[18:24, 15:28] = 255
    c.append(("ring_ring_blob", m))
    yy, xx = np.mgrid[0:35, 0:37]
    c.append(("checkerboard", (((yy + xx) % 2) * 255).astype(np.uint8)))
    m = _z(40, 44)
    m[25:33, 24:33] = 255
    m[33:39, 33:42] = 255   # touches the first only through (32, 32) - (33, 33)
    c.append(("diagonal_joint", m))
    m = _ring(_z(40, 44), 4, 5, 36, 40)
    m[20, 40] = 0           # a one-pixel channel to the frame: the inside is no hole
    c.append(("channel_to_frame", m))
    m = _ring(_z(40, 44), 4, 5, 36, 40)
    m[36, 40] = 0           # the corner is closed by a diagonal pair only: still a hole
    c.append(("pocket_closed_diagonally", m))
    # selection
    m = _z(20, 40)
    m[2:8, 30:36] = 255     # first in raster order, further right
    m[10:16, 3:9] = 255     # the same area
    c.append(("tie_first_raster_wins", m))
    m = _z(12, 34)
    for y, x in ((3, 20), (5, 2), (9, 33), (11, 0)):
        m[y, x] = 255
    c.append(("all_areas_zero", m))
    m = _z(20, 50)
    m[2:4, 3:43] = 255      # 80 pixels, area 39
    m[8:16, 5:13] = 255     # 64 pixels, area 49
    c.append(("thin_large_vs_fat_small", m))
    # class-index masks: foreground is != 0
    m = _z(40, 44)
    m[3:20, 3:30] = 1
    m[10:30, 20:40] = 2
    m[34:38, 2:9] = 200
    c.append(("values_1_2_200", m))
    rng = np.random.default_rng(37)
    c.append(("29x37_random", ((ndimage.gaussian_filter(rng.standard_normal((29, 37)), 2.0) > 0) * 255).astype(np.uint8)))
    return tuple(c)


def random_masks(count, seed, shape=None):
    """Seeded random masks: sides 1..13 (or `shape`), five densities, a third opened or closed."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        h, w = shape if shape else (int(rng.integers(1, 14)), int(rng.integers(1, 14)))
        m = rng.random((h, w)) < (0.3, 0.5, 0.6, 0.75, 0.9)[i % 5]
        if i % 6 == 1:
            m = ndimage.binary_opening(m)
        elif i % 6 == 4:
            m = ndimage.binary_closing(m)
        out.append((m * 255).astype(np.uint8))
    return out


def blob_masks(count, seed, shape=None):
    """Seeded thresholded-Gaussian blobs, sides 20..69 (or `shape`): smooth noise above a quantile,
    or a band of it (rings, which nest components inside holes)."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        h, w = shape if shape else (int(rng.integers(20, 70)), int(rng.integers(20, 70)))
        g = ndimage.gaussian_filter(rng.standard_normal((h, w)), (1.5, 2.5, 4.0)[i % 3])
        if i % 2:
            lo, hi = np.quantile(g, (0.35, 0.6))
            m = (g > lo) & (g < hi)
        else:
            m = g > np.quantile(g, (0.4, 0.55, 0.7)[(i // 2) % 3])
        out.append((m * 255).astype(np.uint8))
    return out


@functools.lru_cache(maxsize=None)
def sample_masks():
    return {n: np.asarray(Image.open(os.path.join(USAGE, n + "_output_mask.png")).convert("L"))
            for n in ("brazil_passport", "chile_id_card")}


# ----------------------------------------------------------------------------- the oracles ---
def traced_stats(mask):
    """[(area2, rect, first)] of every external contour, in order, from the tracer."""
    w = mask.shape[1]
    out = []
    for pts in external_contours(mask):
        a2 = 2.0 * contour_area(pts)
        assert a2 == int(a2)
        out.append((int(a2), bounding_rect(pts), pts[0][1] * w + pts[0][0]))
    return out


def host_record(mask, filled=False):
    """The fields of `unet_contour_box` the device must give: (count, x, y, w, h, first, area2), from
    the tracer or (filled=True: large masks) from the closed form."""
    stats = external_contour_stats_filled(mask) if filled else traced_stats(mask)
    if not stats:
        return (0, 0, 0, 0, 0, 0, 0)
    best = stats[0]
    for s in stats[1:]:
        if s[0] > best[0]:
            best = s
    return (len(stats),) + tuple(best[1]) + (best[2], best[0])


def _assert_same_lists(mask, tag):
    assert external_contour_stats_filled(mask) == traced_stats(mask), tag


# ------------------------------------------------------------------------------- the tests ---
@pytest.mark.parametrize("name", [n for n, _ in mask_cases()])
def test_filled_equals_tracer_on_hand_built_masks(name):
    mask = dict(mask_cases())[name]
    got, ref = largest_external_contour_filled(mask), largest_external_contour(mask)
    assert got == ref
    if ref is not None:
        assert type(got[0]) is float and all(type(v) is int for v in got[1])
    _assert_same_lists(mask, name)


def test_hand_built_masks_hold_what_they_claim():
    c = dict(mask_cases())
    assert largest_external_contour(c["1x1_bg"]) is None and largest_external_contour(c["33x65_zeros"]) is None
    assert largest_external_contour(c["1x1_fg"]) == (0.0, (0, 0, 1, 1))
    assert largest_external_contour(c["33x65_full"]) == (32.0 * 64.0, (0, 0, 65, 33))
    for n in ("ring", "ring_on_frame", "ring_blob_in_hole", "ring_ring_blob", "pocket_closed_diagonally",
              "checkerboard", "diagonal_joint"):
        assert len(external_contours(c[n])) == 1, n
    assert largest_external_contour(c["ring_blob_in_hole"]) == largest_external_contour(c["ring"])
    assert largest_external_contour(c["pocket_closed_diagonally"])[0] == 32.0 * 35.0 - 0.5
    assert largest_external_contour(c["channel_to_frame"])[0] < 100.0
    assert largest_external_contour(c["tie_first_raster_wins"]) == (25.0, (30, 2, 6, 6))
    assert largest_external_contour(c["all_areas_zero"]) == (0.0, (20, 3, 1, 1))
    assert largest_external_contour(c["thin_large_vs_fat_small"]) == (49.0, (5, 8, 8, 8))
    for h, w in TILE_SHAPES:
        assert largest_external_contour(c[f"{h}x{w}_serpentine"])[1] == (0, 0, w, h)
        assert len(external_contours(c[f"{h}x{w}_spiral"])) == 1


def test_filled_lists_equal_tracer_on_random_masks():
    masks = random_masks(300, 2024)
    assert {m.shape[0] for m in masks} == set(range(1, 14))
    for i, m in enumerate(masks):
        _assert_same_lists(m, (i, m.tolist()))


def test_filled_lists_equal_tracer_on_blob_masks():
    nested = 0
    for i, m in enumerate(blob_masks(40, 7)):
        assert 20 <= min(m.shape) and max(m.shape) <= 69
        _assert_same_lists(m, i)
        components = ndimage.label(m != 0, structure=np.ones((3, 3), bool))[1]
        nested += components > len(external_contours(m))
    assert nested >= 1, "no blob mask has a component nested in a hole"


@pytest.mark.parametrize("name", sorted(SAMPLE_EXPECT))
def test_filled_equals_tracer_on_reference_sample_masks(name):
    mask = sample_masks()[name]
    assert mask.shape == (960, 540)
    assert largest_external_contour_filled(mask) == largest_external_contour(mask) == SAMPLE_EXPECT[name]
    _assert_same_lists(mask, name)


def test_contour_box_mirror_layout():
    from unet_amd._lib import UnetContourBox
    assert ctypes.sizeof(UnetContourBox) == 32
    assert UnetContourBox.count.offset == 0 and UnetContourBox.first.offset == 20
    assert UnetContourBox.area2.offset == 24


def test_contour_workspace_query():
    from unet_amd import _lib
    q = _lib.query
    b = q("unet_mask_largest_contour_workspace", 540, 960)
    assert b > 0 and b % 256 == 0
    assert b >= 9 * 540 * 960     # int32 labels, int32 area sums, one byte of kind per pixel
    assert q("unet_mask_largest_contour_workspace", 0, 960) == 0
    assert q("unet_mask_largest_contour_workspace", 540, 0) == 0
    assert q("unet_mask_largest_contour_workspace", 0, 0) == 0
    assert q("unet_mask_largest_contour_workspace", 1 << 15, (1 << 15) + 1) == 0   # more than 2^30 pixels


def test_contour_call_refuses_bad_arguments_without_gpu():
    from unet_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(256)   # never dereferenced: every refusal comes before a launch
    assert lib.unet_mask_largest_contour(None, 4, 4, one, one, 1 << 20, None) < 0
    assert b"null pointer" in lib.unet_last_error()
    assert lib.unet_mask_largest_contour(one, 0, 4, one, one, 1 << 20, None) < 0
    assert b"positive" in lib.unet_last_error()
    assert lib.unet_mask_largest_contour(one, 1 << 15, (1 << 15) + 1, one, one, 1 << 40, None) < 0
    assert b"2^30" in lib.unet_last_error()
    need = _lib.query("unet_mask_largest_contour_workspace", 4, 4)
    assert lib.unet_mask_largest_contour(one, 4, 4, one, one, need - 1, None) < 0
    assert b"workspace" in lib.unet_last_error()


def test_mask_largest_contour_refuses_cpu_and_wrong_tensors():
    import torch
    from unet_amd import ops
    with pytest.raises(ValueError, match="no CPU path"):
        ops.mask_largest_contour(torch.zeros((4, 4), dtype=torch.uint8))
