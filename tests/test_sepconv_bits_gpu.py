"""Byte equality of the fused separable-conv entry points (unet_sepconv_fwd, unet_sepconv_bwd_fused,
unet_sepconv_bwd_filter) against tests/golden/sepconv_bits.json: the sha256 of every output buffer, recorded
from the library as it was before the family's host policy moved into csrc/sepconv_plan.h.  The forward
cases take every route and tile width of sep_fwd_plan (the pinned rows of tests/sepconv_plan_check.cpp) at
the smallest shape that reaches it, each in training form (y and BN partials) and in inference form
(neither); the backward cases are the shapes of SW_CASES in test_ops_gpu.py.  These kernels reduce in a
fixed order over a static tile assignment, so the bytes are a function of the inputs and, for the backward,
of the device's CU count (the slice count S of sep_bwd_plan): the fixture records it, and a device that
reports another count fails the test instead of skipping it.

Inputs come from seeded NumPy generators and live in guard bands (tests/fenced.py); workspaces have exactly
the queried size.  `python tests/test_sepconv_bits_gpu.py OUT.json` records a fixture (with the repository
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

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sepconv_bits.json")

AUTO, TILE, RK, RK1 = 0, 1, 2, 3
# name: (schedule, mode, n, h, w, c0, c1, cout, dropout, split planes given, pooling selection asked)
FWD = {
    "tile64":          (AUTO, 1, 1, 8, 16, 16, 0, 64, 0.0, False, False),
    "tile128":         (AUTO, 0, 3, 8, 16, 16, 0, 128, 0.0, False, False),
    "tile128x2":       (AUTO, 3, 1, 8, 16, 16, 16, 256, 0.2, False, False),   # 256 outputs, too few tiles for 256 columns
    "tile256":         (AUTO, 1, 1, 128, 256, 16, 0, 256, 0.0, False, False),  # 256 tiles
    "tile-poolpass":   (AUTO, 1, 3, 8, 16, 16, 0, 64, 0.0, False, True),
    "tile-forced":     (TILE, 1, 3, 8, 16, 64, 0, 128, 0.0, True, True),
    "tile-pool192":    (AUTO, 2, 1, 8, 16, 64, 0, 192, 0.0, False, True),     # max-pool view, N tail 192
    "tile-ktail":      (AUTO, 1, 1, 8, 16, 8, 0, 8, 0.0, False, False),
    "rk64":            (AUTO, 1, 1, 8, 16, 64, 0, 64, 0.0, False, False),
    "rk128":           (AUTO, 1, 3, 8, 16, 64, 0, 128, 0.0, False, True),
    "rk-ntail192":     (AUTO, 1, 2, 8, 32, 96, 0, 192, 0.0, False, False),
    "rk-pool128":      (AUTO, 2, 2, 8, 16, 64, 0, 128, 0.2, True, True),
    "rk-ktail68-100":  (AUTO, 0, 1, 8, 16, 68, 0, 100, 0.0, True, False),      # split planes, Cin % 16 != 0: fp32
    "x6-64":           (AUTO, 1, 3, 8, 16, 64, 0, 64, 0.0, True, True),
    "x6-128":          (AUTO, 1, 1, 8, 16, 128, 0, 128, 0.0, True, False),
    "x6-256":          (AUTO, 1, 1, 16, 32, 64, 0, 256, 0.0, True, True),
    "x6-concat72":     (RK, 3, 1, 8, 16, 72, 56, 128, 0.0, True, False),      # c0 % 16 != 0: no persistent kernel
    "x6-rk1":          (RK1, 1, 1, 8, 16, 64, 0, 128, 0.0, True, False),
    "px-auto-64-128":  (AUTO, 1, 3, 8, 16, 64, 0, 128, 0.0, True, False),
    "px-auto-zsel":    (AUTO, 1, 7, 88, 208, 128, 0, 128, 0.0, True, True),    # 1001 tiles: runs of 1 and 2 per block
    "px-rk-64-64":     (RK, 3, 1, 8, 16, 32, 32, 64, 0.2, True, False),
    "px-rk-64-128":    (RK, 0, 1, 8, 16, 64, 0, 128, 0.0, True, True),
    "px-rk-128-64":    (RK, 0, 3, 8, 16, 128, 0, 64, 0.0, True, True),
    "px-rk-128-128":   (RK, 3, 3, 8, 16, 64, 64, 128, 0.2, True, False),
}
# mode, n, h, w, c0, c1, cout, dropout: SW_CASES of test_ops_gpu.py
BWD = [(1, 2, 8, 16, 64, 0, 64, 0.0), (1, 1, 16, 32, 64, 0, 64, 0.2), (0, 2, 8, 32, 64, 0, 64, 0.0),
       (3, 1, 16, 16, 32, 32, 64, 0.2), (3, 2, 8, 16, 36, 28, 64, 0.0), (3, 1, 16, 32, 64, 64, 64, 0.0),
       (3, 1, 8, 16, 128, 128, 64, 0.2), (1, 3, 64, 96, 64, 0, 64, 0.0), (1, 2, 16, 32, 128, 0, 128, 0.0),
       (3, 1, 16, 32, 128, 128, 128, 0.2), (1, 1, 8, 16, 64, 0, 64, 0.0), (1, 3, 8, 16, 64, 0, 64, 0.0)]


def _cases():
    out = {}
    for name, (sch, mode, n, h, w, c0, c1, cout, drop, pkx, zsel) in FWD.items():
        for train in (True, False):
            out[f"fwd-{name}-{'train' if train else 'infer'}"] = dict(
                kind="fwd", schedule=sch, mode=mode, nhw=[n, h, w], c0=c0, c1=c1, cout=cout, drop=drop, pkx=pkx,
                zsel=zsel, train=train)
    for mode, n, h, w, c0, c1, cout, drop in BWD:
        shape = f"v{mode}-{n}x{h}x{w}-c{c0}+{c1}-o{cout}-d{drop}"
        out[f"filter-{shape}"] = dict(kind="filter", mode=mode, nhw=[n, h, w], c0=c0, c1=c1, cout=cout, drop=drop)
        if cout == 64 and drop == 0.0:  # the fused block backward: 64 outputs, no dropout on the input
            for form in ("da", "rank1"):
                out[f"fused-{form}-{shape}"] = dict(kind="fused", form=form, mode=mode, nhw=[n, h, w], c0=c0, c1=c1,
                                                    cout=cout, drop=drop)
    return out


CASES = _cases()


def sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().contiguous().numpy())).hexdigest()


def _rand(rng, shape, scale=1.0):
    return (rng.random(shape, dtype=np.float32) - np.float32(0.5)) * np.float32(2 * scale)


def _view(ops, mem, rng, mode, n, h, w, c0, c1, drop):
    k = 2 if mode == 2 else 1
    x = mem.inp(_rand(rng, (n, k * h, k * w, c0)))
    if mode == 0:
        v = ops.View.plain(x)
    elif mode == 3:
        v = ops.View.concat(x, mem.inp(_rand(rng, (n, h, w, c1))), mem.inp(_rand(rng, c1) + 1.5), mem.inp(_rand(rng, c1, 0.3)))
    else:
        sc, sh = mem.inp(_rand(rng, c0) + 1.5), mem.inp(_rand(rng, c0, 0.3))
        v = ops.View.bnrelu(x, sc, sh) if mode == 1 else ops.View.pool_bnrelu(x, sc, sh)
    return v.dropout(drop, 29) if drop > 0 else v


def _run(ops, mem, case, cid):
    rng = np.random.default_rng(zlib.crc32(cid.encode()))
    (n, h, w), c0, c1, cout, mode = case["nhw"], case["c0"], case["c1"], case["cout"], case["mode"]
    C, m = c0 + c1, n * h * w
    v = _view(ops, mem, rng, mode, n, h, w, c0, c1, case["drop"])
    dk = mem.inp(_rand(rng, (3, 3, C, 1)))
    if case["kind"] == "fwd":
        pk = mem.inp(_rand(rng, (1, 1, C, cout), 1.7 / np.sqrt(C)))
        pkx = None
        if case["pkx"]:
            pkx = mem.empty(3 * C * cout, dtype=torch.int16, output=False)
            ops.split_x3(pk, [(0, C, cout, 0)], pkx)
        train, zsel = case["train"], case["zsel"]
        y = mem.empty((n, h, w, C)) if train else None
        z = mem.empty((n, h, w, cout))
        part = mem.zeros(ops.bn_partials_numel(m, cout)) if train else None
        zs = mem.empty((n, h // 2, w // 2, cout)) if zsel else None
        gamma = mem.inp(_rand(rng, cout)) if zsel else None
        old = ops.sepconv_set_schedule(case["schedule"])
        try:
            ops.sepconv_fwd(v, n, h, w, dk, cout, pk, y, z, part, zs, gamma, pkx=pkx)
        finally:
            ops.sepconv_set_schedule(old)
        got = {"z": sha(z)}
        if train:
            got.update(y=sha(y), partials=sha(part[:m // 128 * cout * 2]))  # (mean, M2) per 128-pixel tile and column
        if zsel:
            got["z_pool_sel"] = sha(zs)
        return got
    ddk, dpk = mem.empty((3, 3, C, 1)), mem.empty((1, 1, C, cout))
    if case["kind"] == "filter":
        dy, dz = mem.inp(_rand(rng, (m, C))), mem.inp(_rand(rng, (m, cout)))
        ops.sepconv_bwd_filter(v, n, h, w, dk, dy, dz, cout, ddk, dpk)
        return {"d_dw_kernel": sha(ddk), "d_pw_kernel": sha(dpk)}
    pk = mem.inp(_rand(rng, (1, 1, C, cout), 1.7 / np.sqrt(C)))
    z = mem.inp(_rand(rng, (m, cout), 2.0))
    sc, sh, coef = mem.inp(_rand(rng, cout) + 1.5), mem.inp(_rand(rng, cout, 0.3)), mem.inp(_rand(rng, 3 * cout))
    dy = mem.empty((n, h, w, C))
    if case["form"] == "da":
        ops.sepconv_bwd_fused(v, n, h, w, dk, pk, mem.inp(_rand(rng, (m, cout))), z, sc, sh, coef, cout, dy, ddk, dpk)
    else:
        r1 = (mem.inp(_rand(rng, m)), mem.inp(_rand(rng, cout, 0.3)))
        ops.sepconv_bwd_fused(v, n, h, w, dk, pk, None, z, sc, sh, coef, cout, dy, ddk, dpk, da_rank1=r1)
    return {"dy": sha(dy), "d_dw_kernel": sha(ddk), "d_pw_kernel": sha(dpk)}


def run_case(ops, cid):
    """Runs one case inside fresh guard bands; {buffer name: sha256}."""
    mem, ws = fenced.Arena("cuda"), fenced.FencedWorkspace("cuda")
    with ws.installed(ops):
        got = _run(ops, mem, CASES[cid], cid)
        mem.check(extra=[ws])
    return got


def device_cus():
    return int(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count)


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


def test_device_has_the_recorded_cu_count(golden):
    """The backward's slice count, and so its summation order, follows the CU count."""
    assert device_cus() == golden["cus"]


@pytest.mark.parametrize("cid", list(CASES))
def test_sepconv_bits(ops, golden, cid):
    assert device_cus() == golden["cus"]
    got = run_case(ops, cid)
    want = golden["cases"][cid]["sha256"]
    assert got == want, sorted(k for k in want if got.get(k) != want[k])


if __name__ == "__main__":
    from unet_amd import ops as O
    rec = {cid: {"params": c, "sha256": run_case(O, cid)} for cid, c in CASES.items()}
    with open(sys.argv[1], "w") as f:
        json.dump({"cus": device_cus(), "cases": rec}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(rec)} cases to {sys.argv[1]}")
