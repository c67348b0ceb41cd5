"""Byte equality of the head, dice and MeanIoU entry points against tests/golden/head_bits.json: the
sha256 of every output buffer, recorded from the library as it was before csrc/head.hip was split
into head_fwd.hip, head_bwd.hip and loss.hip.  Every route of csrc/head_plan.h is covered, in both
view modes, at 1, 127 and 129 pixels and at a two-image shape whose images are shorter than a tile
(143 pixels each).  The two heads whose src0 is 4 bytes off are hashed for the forward and the dice
sums only (the backward kernels read src0 as float4): that an unaligned src0 leaves the backward
route where it is, is pinned by tests/head_plan_check.cpp alone, not by bytes.  All reductions of
these kernels run in a fixed order, so the bytes are a function of the inputs alone.

Inputs come from seeded NumPy generators and live in guard bands (tests/fenced.py); workspaces have
exactly the queried size.  `python tests/test_head_bits_gpu.py OUT.json` records a fixture (with the
repository root and the package directory on PYTHONPATH)."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

import fenced
from helpers import bn_affine

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "head_bits.json")

# (Cin, classes, src0 16-byte aligned): one head per forward x backward route pair of head_plan.h
HEADS = [(64, 1, True),    # BIN / BIN_FUSED
         (64, 21, True),   # MFMA / MC_FUSED
         (64, 1, False),   # GENERAL (rows read by elements)
         (48, 1, True),    # GENERAL / GENERAL
         (48, 21, True),   # REG / GENERAL
         (128, 21, True),  # GENERAL / MC_REG
         (64, 32, True),   # MFMA / MC_REG
         (64, 21, False),  # REG
         (4, 3, True)]     # REG / MC_FUSED
SHAPES = [(1, 1, 1), (1, 1, 127), (1, 3, 43), (2, 13, 11)]  # 1, 127, 129 pixels; tiles that span two images
BNSTATS_HEADS = [(64, 1), (64, 21), (4, 3)]


def _cases():
    out = {}
    for cin, ncls, al in HEADS:
        for n, h, w in SHAPES:
            for mode in (0, 1):
                out[f"head-c{cin}-k{ncls}-{'al' if al else 'skew'}-{n}x{h}x{w}-v{mode}"] = dict(
                    kind="head", cin=cin, ncls=ncls, src_aligned=al, nhw=[n, h, w], mode=mode, io_skewed=False)
    out["head-c64-k21-ioskew-2x13x11-v1"] = dict(kind="head", cin=64, ncls=21, src_aligned=True, nhw=[2, 13, 11],
                                                 mode=1, io_skewed=True)  # prob, y_true 4 bytes off
    for cin, ncls in BNSTATS_HEADS:
        for n, h, w in SHAPES:
            out[f"bnstats-c{cin}-k{ncls}-{n}x{h}x{w}"] = dict(kind="bnstats", cin=cin, ncls=ncls, nhw=[n, h, w])
    for k, thr, count in [(2, None, 127), (2, 0.5, 286), (5, None, 127), (5, None, 286)]:
        out[f"meaniou-k{k}-t{thr}-{count}"] = dict(kind="meaniou", ncls=k, thr=thr, count=count)
    return out


CASES = _cases()


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _forward(ops, mem, rng, cin, ncls, nhw, mode, src_aligned=True, io_skewed=False):
    """Inputs, then unet_head_fwd and unet_dice_fwd: (aligned view, kernel, prob, y_true, sums, hashes)."""
    n, h, w = nhw
    x = mem.inp(rng.standard_normal((n, h, w, cin)).astype(np.float32))
    sc, sh = (mem.inp(a) for a in bn_affine(rng, cin))
    view = (lambda t: ops.View.plain(t)) if mode == 0 else (lambda t: ops.View.bnrelu(t, sc, sh))
    k = mem.inp((rng.standard_normal((1, 1, cin, ncls)) * 0.2).astype(np.float32))
    b = mem.inp((rng.standard_normal(ncls) * 0.1).astype(np.float32))
    if ncls == 1:
        yt = (rng.random((n, h, w, 1)) > 0.5).astype(np.float32)
    else:
        yt = np.eye(ncls, dtype=np.float32)[rng.integers(0, ncls, (n, h, w))]
    prob, yt = mem.empty((n, h, w, ncls)), mem.inp(yt)
    if io_skewed:
        prob, yt = mem.skewed(prob), mem.skewed(yt)
    ops.head_fwd(view(x if src_aligned else mem.skewed(x)), n, h, w, ncls, k, b, prob)
    sums, res = mem.empty(n * ncls * 3), mem.empty(3)
    ops.dice_fwd(yt, prob, n, h * w, ncls, 1e-7, sums, res)
    return view(x), k, prob, yt, sums, {"prob": sha(prob), "sums": sha(sums), "result": sha(res)}


def run_case(ops, case):
    """Runs one case inside fresh guard bands; {buffer name: sha256}."""
    mem, ws = fenced.Arena("cuda"), fenced.FencedWorkspace("cuda")
    with ws.installed(ops):
        got = _run(ops, mem, case)
        mem.check(extra=[ws])
    return got


def _run(ops, mem, case):
    if case["kind"] == "meaniou":
        k, count = case["ncls"], case["count"]
        rng = np.random.default_rng(1000 * k + count)
        yt = rng.integers(0, k if case["thr"] is None else 2, count).astype(np.float32)
        yp = (rng.random(count) * (k if case["thr"] is None else 1)).astype(np.float32)
        yp[::7] = np.floor(yp[::7])
        conf = mem.zeros(k * k, dtype=torch.int64)
        ops.meaniou_update(mem.inp(yt), mem.inp(yp), k, case["thr"], conf)
        return {"confusion": sha(conf)}
    cin, ncls, (n, h, w) = case["cin"], case["ncls"], case["nhw"]
    rng = np.random.default_rng(cin * 1000003 + ncls * 1009 + n * h * w * 7 + case.get("mode", 1))
    if case["kind"] == "head":
        v, k, prob, yt, sums, got = _forward(ops, mem, rng, cin, ncls, (n, h, w), case["mode"], case["src_aligned"],
                                             case["io_skewed"])
        if not case["src_aligned"]:
            return got  # the backward kernels read src0 as float4: forward and dice only
        for loss in (0, 1):
            dx, dk, db = mem.empty((n, h, w, cin)), mem.empty(cin * ncls), mem.empty(ncls)
            ops.head_bwd(v, n, h, w, ncls, k, prob, yt, sums, 1e-7, loss, dx, dk, db)
            got.update({f"dx{loss}": sha(dx), f"dkernel{loss}": sha(dk), f"dbias{loss}": sha(db)})
        return got
    v, k, prob, yt, sums, got = _forward(ops, mem, rng, cin, ncls, (n, h, w), 1)
    S = ops.head_bwd_bnstats_slabs(v, n, h, w, ncls)
    assert S > 0
    mean = mem.inp((rng.standard_normal(cin) * 0.1).astype(np.float32))
    rstd = mem.inp((1.0 + rng.random(cin)).astype(np.float32))
    for loss in (0, 1):
        for bn in (0, 1):
            for form in (("dx", "dlogit") if ncls == 1 else ("dx",)):  # the rank-one form is binary only
                out = mem.empty((n, h, w, cin)) if form == "dx" else mem.empty(n * h * w)
                dk, db = mem.empty(cin * ncls), mem.empty(ncls)
                part = mem.zeros(ops.bn_stats_partials_numel(S, cin))
                ops.head_bwd_bnstats(v, n, h, w, ncls, k, prob, yt, sums, 1e-7, loss, out if form == "dx" else None,
                                     dk, db, mean if bn else None, rstd if bn else None, part,
                                     dlogit=None if form == "dx" else out)
                tag = f"{loss}{'bn' if bn else ''}"
                got.update({f"{form}{tag}": sha(out), f"dkernel_{form}{tag}": sha(dk), f"dbias_{form}{tag}": sha(db),
                            f"bnpart_{form}{tag}": sha(part)})
    return got


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
def test_head_bits(ops, golden, cid):
    got = run_case(ops, CASES[cid])
    want = golden[cid]["sha256"]
    assert got == want, sorted(k for k in want if got.get(k) != want[k])


if __name__ == "__main__":
    from unet_amd import ops as O
    rec = {cid: {"params": c, "sha256": run_case(O, c)} for cid, c in CASES.items()}
    with open(sys.argv[1], "w") as f:
        json.dump({"cases": rec}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(rec)} cases to {sys.argv[1]}")
