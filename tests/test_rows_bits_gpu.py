"""Byte equality of the rows-GEMM entry points against tests/golden/rows_bits.json: the sha256 of
every output buffer (dy, the dz side store, the forward BN partials, the ConvT outputs, the ConvT data
gradient and its BN-backward partials), recorded by tools/record_rows_bits.py from the library as it
was before the split-precision k-loop of gemm_rows_vec (csrc/gemm_rows.hip) had its last stage peeled
off.  A change of that loop's schedule must not change one bit: each output element is one k-ordered
accumulation chain per MFMA tile, and every reduction of the epilogues runs in a fixed order.

Cases: the split-precision (x6 == true) rows of kOpRows in tests/gemm_plan_check.cpp, and the k-loop's
edges on the BatchNorm-backward route: one, two and three 32-deep stages (K = 32, 64, 96), a ragged
pixel count with N not a multiple of 128, N = 128 (every block writes the dz side store) and N = 256
(the blocks of the second column tile do not), dropout, no dz output, and the deepest K the route
takes (512).  The ConvT forward runs in the plain, BN + ReLU and dropout views; the ConvT data gradient
with BN partials at the smallest pixel count for which rows_x6 answers true with 68 input channels
(256 row tiles x 1 column tile, convt_bnpart_bm = 128).  One fp32 shape per tile of rows_cfg keeps the
fp32 k-loop, which this change leaves alone, under the same guard.

Inputs come from seeded NumPy generators and live in guard bands (tests/fenced.py); workspaces have
exactly the queried size."""
import hashlib
import json
import os
import zlib

import numpy as np
import pytest

import fenced
from helpers import bn_affine

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rows_bits.json")


def _bnbwd(m, cin, cout, drop=0.0, planes=True, dz=True):
    return dict(kind="bnbwd", m=m, cin=cin, cout=cout, drop=drop, planes=planes, dz=dz)


def _pwfwd(m, cin, cout, stats, planes=True):
    return dict(kind="pwfwd", m=m, cin=cin, cout=cout, stats=stats, planes=planes)


def _convt(n, h, w, cin, cout, view, drop=0.0, planes=True):
    return dict(kind="convt_fwd", nhw=[n, h, w], cin=cin, cout=cout, view=view, drop=drop, planes=planes)


def _convt_bwd(n, h, w, cin, cout, planes=True):
    return dict(kind="convt_bwd_bnstats", nhw=[n, h, w], cin=cin, cout=cout, planes=planes)


# GEMM shapes in the comments are M x K x N
CASES = {
    # BatchNorm-backward data gradient, split precision: K = cout, N = cin
    "bnbwd-k32": _bnbwd(33000, 96, 32),              # one stage: no k-loop iteration, the peeled stage only
    "bnbwd-k64": _bnbwd(33000, 96, 64),              # two stages
    "bnbwd-k96": _bnbwd(33000, 96, 96),              # an odd number of stages
    "bnbwd-33000x128x96": _bnbwd(33000, 96, 128),    # ragged M, N not a multiple of 128
    "bnbwd-n128": _bnbwd(33000, 128, 64),            # every block stores dz
    "bnbwd-n256": _bnbwd(16500, 256, 64),            # 129 x 2 tiles: the nt != 0 blocks store no dz
    "bnbwd-16384x256x256": _bnbwd(16384, 256, 256),  # whole row tiles
    "bnbwd-33000x64x512": _bnbwd(33000, 512, 64),    # four column tiles
    "bnbwd-k512": _bnbwd(33000, 96, 512),            # the deepest K of the route (coefficients fill their LDS)
    "bnbwd-drop": _bnbwd(33000, 96, 64, drop=0.2),
    "bnbwd-drop-n256": _bnbwd(16500, 256, 96, drop=0.2),
    "bnbwd-nodz": _bnbwd(33000, 96, 64, dz=False),
    # pointwise forward: K = cin, N = cout
    "pwfwd-stats-33000x96x160": _pwfwd(33000, 96, 160, True),  # the split route with statistics
    "pwfwd-33000x96x160": _pwfwd(33000, 96, 160, False),
    "pwfwd-stats-16384x512x1024": _pwfwd(16384, 512, 1024, True),
    "pwfwd-33000x1024x128": _pwfwd(33000, 1024, 128, False),   # the GEMM behind the 1024-channel dz pass
    # ConvT forward: K = cin, N = 4 cout
    "convt-33020x64x128": _convt(2, 130, 127, 64, 32, "bnrelu"),
    "convt-17589x96x160": _convt(13, 33, 41, 96, 40, "bnrelu"),
    "convt-17589x96x160-drop": _convt(13, 33, 41, 96, 40, "bnrelu", drop=0.2),
    "convt-17589x96x160-plain": _convt(13, 33, 41, 96, 40, "plain"),
    "convt-17589x96x160-plain-drop": _convt(13, 33, 41, 96, 40, "plain", drop=0.2),
    "convt-16384x256x512": _convt(4, 64, 64, 256, 128, "bnrelu"),
    # ConvT data gradient with BN partials: K = 4 cout, N = cin
    "convtbwd-32761x64x68": _convt_bwd(1, 181, 181, 68, 16),   # 256 x 1 tiles: the smallest split-route grid
    "convtbwd-16384x512x256": _convt_bwd(16, 32, 32, 256, 128),
    # fp32, one shape per tile (bn, bk, bm) of rows_cfg
    "f32-64-16": _pwfwd(300, 64, 128, True, planes=False),
    "f32-64-32": _pwfwd(512, 256, 512, True, planes=False),
    "f32-128-16": _pwfwd(33000, 96, 160, True, planes=False),
    "f32-128-32": _bnbwd(33000, 96, 128, planes=False),
    "f32-256-16": _bnbwd(33000, 512, 64, planes=False),
    "f32-128-32-bm64": _bnbwd(257, 128, 64, planes=False),
}


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _planes(ops, mem, w2d, keep):
    rows, cols = w2d.shape
    t = mem.empty(3 * rows * cols, dtype=torch.int16)
    ops.split_x3(mem.inp(_f32(w2d)), [(0, rows, cols, 0)], t, keep=keep)
    return t


def run_case(ops, cid):
    """Runs one case inside fresh guard bands; {buffer name: sha256}."""
    mem, ws = fenced.Arena("cuda"), fenced.FencedWorkspace("cuda")
    with ws.installed(ops):
        got = _run(ops, mem, np.random.default_rng(zlib.crc32(cid.encode())), CASES[cid])
        mem.check(extra=[ws])
    return got


def _run(ops, mem, rng, c):
    normal = lambda *s: rng.standard_normal(s, dtype=np.float32)  # noqa: E731
    if c["kind"] == "bnbwd":
        m, cin, cout = c["m"], c["cin"], c["cout"]
        da, z = mem.inp(normal(m, cout)), mem.inp(normal(m, cout) * 2 + 0.3)
        sc, sh = (mem.inp(a) for a in bn_affine(rng, cout))
        coef = mem.inp(normal(3 * cout) * 0.1)
        pk = _f32(normal(cin, cout) / np.sqrt(cout))
        pkd = _planes(ops, mem, pk, keep=True) if c["planes"] else None
        dy = mem.empty((m, cin))
        dz = mem.empty((m, cout)) if c["dz"] else None
        ops.pointwise_bwd_data_bnrelu(da, z, m, cin, cout, mem.inp(pk), sc, sh, coef, c["drop"], 55, dy, dz, pkd=pkd)
        return {"dy": sha(dy), **({"dz": sha(dz)} if c["dz"] else {})}
    if c["kind"] == "pwfwd":
        m, cin, cout = c["m"], c["cin"], c["cout"]
        y = mem.inp(normal(m, cin))
        pk = _f32(normal(cin, cout) / np.sqrt(cin))
        pkx = _planes(ops, mem, pk, keep=False) if c["planes"] else None
        zz = mem.empty((m, cout))
        part = mem.zeros(ops.bn_partials_numel(m, cout)) if c["stats"] else None
        ops.pointwise_fwd(y, m, cin, cout, mem.inp(pk), zz, part, pkx=pkx)
        return {"z": sha(zz), **({"partials": sha(part)} if c["stats"] else {})}
    (n, h, w), cin, cout = c["nhw"], c["cin"], c["cout"]
    x = mem.inp(normal(n, h, w, cin))
    sc, sh = (mem.inp(a) for a in bn_affine(rng, cin))
    k = _f32(normal(2, 2, cout, cin) / np.sqrt(cin))
    if c["kind"] == "convt_fwd":
        v = ops.View.plain(x) if c["view"] == "plain" else ops.View.bnrelu(x, sc, sh)
        if c["drop"] > 0:
            v = v.dropout(c["drop"], 4242)
        kx = _planes(ops, mem, k.reshape(4 * cout, cin), keep=True) if c["planes"] else None
        out = mem.empty((n, 2 * h, 2 * w, cout))
        ops.conv_transpose2x2_fwd(v, n, h, w, cout, mem.inp(k), mem.inp(normal(cout)), out, kx=kx)
        return {"out": sha(out)}
    assert c["kind"] == "convt_bwd_bnstats"
    v = ops.View.bnrelu(x, sc, sh)
    kxt = _planes(ops, mem, k.reshape(4 * cout, cin), keep=False) if c["planes"] else None
    dout = mem.inp(normal(n, 2 * h, 2 * w, cout))
    S = ops.conv_transpose2x2_bwd_data_bnstats_slabs(v, n, h, w, cout)
    assert S > 0
    mean, rstd = mem.inp(normal(cin) * 0.1), mem.inp(1.0 + rng.random(cin, dtype=np.float32))
    part = mem.zeros(ops.bn_stats_partials_numel(S, cin))
    dx = mem.empty((n, h, w, cin))
    ops.conv_transpose2x2_bwd_data_bnstats(v, n, h, w, cout, mem.inp(k), dout, dx, mean, rstd, part, kxt=kxt)
    return {"dx": sha(dx), "bnpart": sha(part)}


@pytest.fixture(scope="module")
def ops():
    from unet_amd import ops as O
    return O


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def test_fixture_lists_these_cases(golden):
    assert {k: v["params"] for k, v in golden.items()} == CASES


@pytest.mark.parametrize("cid", list(CASES))
def test_rows_bits(ops, golden, cid):
    got = run_case(ops, cid)
    want = golden[cid]["sha256"]
    assert got == want, sorted(k for k in want if got.get(k) != want[k])
