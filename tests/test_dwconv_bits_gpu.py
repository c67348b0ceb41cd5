"""Byte equality of the depthwise 3x3 entry points (unet_dwconv3x3_fwd, unet_view_materialize,
unet_dwconv3x3_bwd_data, unet_dwconv3x3_bwd_filter, unet_dwconv3x3_bwd_data_bnstats, its _dwf form, and
unet_reduce_slabs over their slabs) against tests/golden/dwconv_bits.json: the sha256 of every output buffer,
recorded from the library as it was before the family's host policy moved into csrc/dw_plan.h.  The views
take every route of dw_plan (flat scalar, flat vector off the tiled widths, tiled at every quad count and at
two channel chunks; tests/dw_plan_check.cpp pins the route of each) in all four view modes with and without
dropout, at one pixel, 1 x 1 x 127, 1 x 3 x 43 (ragged in both tile directions), 2 x 9 x 7, and at tile counts
that are and are not a multiple of 8 (the XCD tile order on and off); the tiled filter gradient's persistent
loop runs with more tiles than blocks.  These kernels reduce in a fixed order over a static assignment that
does not depend on the device's CU count, so the bytes are a function of the inputs alone.

Not recorded: unet_dwconv3x3_bwd_filter on a concat view split off the channel quads (c0 % 4 != 0,
(c0 + c1) % 4 == 0), which wrote past its workspace or left channels unsummed before dw_plan.h; it is held
by value in test_ops_gpu.py and test_fenced_ops_gpu.py.

Inputs come from seeded NumPy generators and live in guard bands (tests/fenced.py); workspaces have exactly
the queried size.  `python tests/test_dwconv_bits_gpu.py OUT.json` records a fixture (with the repository
root and the package directory on PYTHONPATH)."""
import hashlib
import json
import os
import sys
import zlib

import numpy as np
import pytest

import fenced

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dwconv_bits.json")

PLAIN, BNRELU, POOL, CONCAT = 0, 1, 2, 3
# name: (mode, n, h, w, c0, c1, dropout); each through forward, materialize, data and filter gradient
VIEWS = {
    "scalar-c3":          (PLAIN, 2, 9, 7, 3, 0, 0.0),
    "scalar-c3-1px":      (BNRELU, 1, 1, 1, 3, 0, 0.2),
    "scalar-pool-c3":     (POOL, 1, 3, 43, 3, 0, 0.2),
    "scalar-concat-5+6":  (CONCAT, 1, 1, 127, 5, 6, 0.0),
    "scalar-concat-6+2":  (CONCAT, 1, 3, 43, 6, 2, 0.2),    # split off the quads: no filter gradient recorded
    "vec-c12":            (BNRELU, 1, 3, 43, 12, 0, 0.2),
    "vec-pool-c12":       (POOL, 2, 9, 7, 12, 0, 0.0),
    "vec-concat-8+4":     (CONCAT, 1, 1, 127, 8, 4, 0.0),
    "vec-c68":            (PLAIN, 1, 3, 43, 68, 0, 0.2),     # 17 quads, one channel tile
    "vec-concat-32+36":   (CONCAT, 2, 9, 7, 32, 36, 0.2),
    "vec-c260":           (BNRELU, 1, 3, 43, 260, 0, 0.0),   # 65 quads, two channel tiles
    "vec-pool-c260-1px":  (POOL, 1, 1, 1, 260, 0, 0.2),
    "tile-qt1":           (PLAIN, 1, 3, 43, 4, 0, 0.0),
    "tile-qt2-pool":      (POOL, 1, 1, 127, 8, 0, 0.2),
    "tile-qt2-1px":       (BNRELU, 1, 1, 1, 8, 0, 0.0),
    "tile-qt4-concat":    (CONCAT, 2, 9, 7, 8, 8, 0.2),
    "tile-qt8":           (BNRELU, 1, 3, 43, 32, 0, 0.2),
    "tile-qt8-pool":      (POOL, 2, 9, 7, 32, 0, 0.0),
    "tile-qt16-8tiles":   (BNRELU, 1, 16, 64, 64, 0, 0.0),   # 8 tiles: XCD tile order
    "tile-qt16-6tiles":   (PLAIN, 1, 16, 48, 64, 0, 0.2),    # 6 tiles: plain order
    "tile-2chunks-concat": (CONCAT, 1, 3, 43, 64, 64, 0.0),
    "tile-2chunks-pool":  (POOL, 2, 9, 7, 128, 0, 0.2),
}
# the tiled filter gradient's persistent loop: 16 channel chunks, 32 blocks over 40 tiles (XCD-contiguous runs of
# 5 tiles over 4 blocks) and over 35 tiles (plain interleave)
FILTER_ONLY = {
    "persist-40tiles": (BNRELU, 1, 64, 80, 1024, 0, 0.0),
    "persist-35tiles": (BNRELU, 1, 56, 80, 1024, 0, 0.2),
}
# (mode, n, h, w, c, dropout, mean and rstd given)
BNSTATS = [(POOL, 2, 9, 7, 16, 0.0, True), (POOL, 1, 3, 43, 128, 0.2, True), (POOL, 1, 1, 127, 8, 0.0, False),
           (POOL, 1, 16, 64, 64, 0.2, False), (BNRELU, 1, 16, 64, 64, 0.0, True), (BNRELU, 2, 9, 7, 32, 0.2, True),
           (BNRELU, 1, 1, 1, 4, 0.0, False), (BNRELU, 1, 3, 43, 128, 0.2, False)]
# (n, h, w, c, mean and rstd given): BN+ReLU view, no dropout
DWF = [(1, 33, 17, 4, True), (2, 5, 7, 8, False), (2, 9, 7, 16, True), (1, 3, 43, 32, False), (1, 16, 64, 64, True),
       (1, 16, 48, 128, False), (1, 1, 127, 256, True)]


def _unrecorded_filter(mode, c0, c1):
    return mode == CONCAT and c0 % 4 != 0 and (c0 + c1) % 4 == 0


def _cases():
    out = {}
    for name, (mode, n, h, w, c0, c1, drop) in VIEWS.items():
        for kind in ("fwd", "materialize", "bwd_data", "bwd_filter"):
            if kind == "bwd_filter" and _unrecorded_filter(mode, c0, c1):
                continue
            out[f"{kind}-{name}"] = dict(kind=kind, mode=mode, nhw=[n, h, w], c0=c0, c1=c1, drop=drop)
    for name, (mode, n, h, w, c0, c1, drop) in FILTER_ONLY.items():
        out[f"bwd_filter-{name}"] = dict(kind="bwd_filter", mode=mode, nhw=[n, h, w], c0=c0, c1=c1, drop=drop)
    for mode, n, h, w, c, drop, bn in BNSTATS:
        out[f"bnstats-v{mode}-{n}x{h}x{w}-c{c}-d{drop}-bn{int(bn)}"] = dict(kind="bnstats", mode=mode, nhw=[n, h, w], c0=c,
                                                                         c1=0, drop=drop, bn=bn)
    for n, h, w, c, bn in DWF:
        out[f"dwf-{n}x{h}x{w}-c{c}-bn{int(bn)}"] = dict(kind="dwf", mode=BNRELU, nhw=[n, h, w], c0=c, c1=0, drop=0.0, bn=bn)
    return out


CASES = _cases()


def sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().contiguous().numpy())).hexdigest()


def _rand(rng, shape, scale=1.0):
    return (rng.random(shape, dtype=np.float32) - np.float32(0.5)) * np.float32(2 * scale)


def _view(ops, mem, rng, mode, n, h, w, c0, c1, drop):
    k = 2 if mode == POOL else 1
    x = mem.inp(_rand(rng, (n, k * h, k * w, c0)))
    if mode == PLAIN:
        v = ops.View.plain(x)
    elif mode == CONCAT:
        v = ops.View.concat(x, mem.inp(_rand(rng, (n, h, w, c1))), mem.inp(_rand(rng, c1) + 1.5), mem.inp(_rand(rng, c1, 0.3)))
    else:
        sc, sh = mem.inp(_rand(rng, c0) + 1.5), mem.inp(_rand(rng, c0, 0.3))
        v = ops.View.bnrelu(x, sc, sh) if mode == BNRELU else ops.View.pool_bnrelu(x, sc, sh)
    return v.dropout(drop, 29) if drop > 0 else v


def _run(ops, mem, case, cid):
    rng = np.random.default_rng(zlib.crc32(cid.encode()))
    (n, h, w), c0, c1, mode, kind = case["nhw"], case["c0"], case["c1"], case["mode"], case["kind"]
    C = c0 + c1
    v = _view(ops, mem, rng, mode, n, h, w, c0, c1, case["drop"])
    if kind == "materialize":
        return {"out": sha(ops.view_materialize(v, n, h, w, mem.empty((n, h, w, C))))}
    if kind == "fwd":
        return {"y": sha(ops.dwconv3x3_fwd(v, n, h, w, mem.inp(_rand(rng, (3, 3, C, 1))), mem.empty((n, h, w, C))))}
    if kind == "bwd_filter":
        ddk = mem.empty((3, 3, C, 1))
        ops.dwconv3x3_bwd_filter(v, n, h, w, mem.inp(_rand(rng, (n, h, w, C))), ddk)
        return {"d_dw_kernel": sha(ddk)}
    dk, dy = mem.inp(_rand(rng, (3, 3, C, 1))), mem.inp(_rand(rng, (n, h, w, C)))
    if mode == POOL:  # the pool route accumulates into the stored gradient of the 2 x 2 source
        dx0 = mem.inp(_rand(rng, (n, 2 * h, 2 * w, c0)), fence=mem.out_fence)
    else:
        dx0 = mem.empty((n, h, w, c0))
    if kind == "bwd_data":
        dx1 = mem.empty((n, h, w, c1)) if mode == CONCAT else None
        ops.dwconv3x3_bwd_data(v, n, h, w, dk, dy, dx0, dx1)
        return {"dx0": sha(dx0), "dx1": sha(dx1)} if mode == CONCAT else {"dx0": sha(dx0)}
    S = ops.dwconv3x3_bwd_data_bnstats_slabs(v, n, h, w)
    assert S > 0
    mean, rstd = (mem.inp(_rand(rng, C, 0.1)), mem.inp(_rand(rng, C, 0.5) + 1.5)) if case["bn"] else (None, None)
    part = mem.zeros(ops.bn_stats_partials_numel(S, C))
    got = {"slabs": S}
    if kind == "bnstats":
        ops.dwconv3x3_bwd_data_bnstats(v, n, h, w, dk, dy, dx0, mean, rstd, part)
    else:
        dwp = mem.empty(S * 9 * C)
        ops.dwconv3x3_bwd_data_bnstats_dwf(v, n, h, w, dk, dy, dx0, mean, rstd, part, dwp)
        got["dw_slabs"] = sha(dwp)
        ddk = mem.empty((3, 3, C, 1))
        ops.reduce_slabs(dwp, S, 9 * C, ddk)  # (the slabs are its scratch: hashed before)
        got["d_dw_kernel"] = sha(ddk)
    got.update(dx0=sha(dx0), bn_slabs=sha(part[:S * 2 * C]))
    sums = mem.empty(2 * C)
    ops.reduce_slabs(part[:S * 2 * C], S, 2 * C, sums)
    got["bn_sums"] = sha(sums)
    return got


def run_case(ops, cid):
    """Runs one case inside fresh guard bands; {buffer name: sha256}."""
    mem, ws = fenced.Arena("cuda"), fenced.FencedWorkspace("cuda")
    with ws.installed(ops):
        got = _run(ops, mem, CASES[cid], cid)
        mem.check(extra=[ws])
    return got


@pytest.fixture(scope="module")
def ops():
    from unet_amd import ops as O
    return O


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_fixture_lists_these_cases(golden):
    assert {k: v["params"] for k, v in golden["cases"].items()} == CASES


@pytest.mark.parametrize("cid", list(CASES))
def test_dwconv_bits(ops, golden, cid):
    got = run_case(ops, cid)
    want = golden["cases"][cid]["sha256"]
    assert got == want, sorted(k for k in want if got.get(k) != want[k])


if __name__ == "__main__":
    from unet_amd import ops as O
    rec = {cid: {"params": c, "sha256": run_case(O, cid)} for cid, c in CASES.items()}
    with open(sys.argv[1], "w") as f:
        json.dump({"cases": rec}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(rec)} cases to {sys.argv[1]}")
