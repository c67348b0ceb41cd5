"""Byte equality of the BatchNorm entry points (unet_bn_finalize, unet_bn_moments, unet_bn_finalize_moments,
unet_bn_infer_params, unet_bn_relu_bwd, unet_bn_relu_bwd_stats, unet_bn_relu_bwd_stats_finish, unet_bn_bwd_coef)
against tests/golden/bn_bits.json: the sha256 of every output buffer, recorded from the library as it was
before the family's host policy moved into csrc/bn_plan.h and bn.hip was split into bn_fwd.hip and bn_bwd.hip.

Forward partials are synthesised as (mean, M2) float pairs per 128-row tile, so no GEMM runs: m = 1 and 129 give
one ragged partial, 8192 one full chunk of 64 partials, 8193 two chunks (the second of one row), 40997 six
chunks and 524293 65 chunks, a second trip of the last block's 64-rows-in-flight loop.  Every m runs with and
without gamma, beta and moving statistics, with update_moving off, without the mean / rstd outputs, and with a
mean of 1e4 against a standard deviation of 1 (the shifted sums).  The backward shapes take scalar lanes and
the reduce_slabs + coefficient-kernel route (c = 3, 6), 17 quads in 15 row lanes (68), two column blocks
(260) and 65 slabs (8320 x 4: two finish rows and the last-arrival path); the finish runs on synthesised slabs
at S = 1, 63, 64, 65 and 2049 (33 chunk rows: the two-deep loop and its tail).  Two cases run twice on the same
workspace without zeroing it again: the arrival counters are left zero.  tests/bn_plan_check.cpp pins the
geometry of each shape.  These kernels reduce in a fixed order over a static assignment that does not depend
on the device's CU count, so the bytes are a function of the inputs alone.

Inputs come from seeded NumPy generators and live in guard bands (tests/fenced.py); workspaces have exactly
the queried size.  `python tests/test_bn_bits_gpu.py OUT.json` records a fixture (with the repository root
and the package directory on PYTHONPATH)."""
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

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bn_bits.json")

FWD_M = [1, 129, 8192, 8193, 40997, 524293]
# name: (gamma, beta, moving statistics, update_moving, mean / rstd outputs, mean of the data)
FWD_VARIANTS = {
    "bn":       (True, True, True, 1, True, 0.3),
    "nogamma":  (False, True, True, 1, True, 0.3),
    "nobeta":   (False, False, False, 1, True, 0.3),
    "nomoving": (True, True, False, 1, True, 0.3),
    "noupdate": (True, True, True, 0, True, 0.3),
    "nullout":  (True, True, True, 1, False, 0.3),
    "shifted":  (True, True, True, 1, True, 1e4),
}
BWD_SHAPES = [(1, 4), (300, 3), (300, 6), (300, 68), (300, 260), (8320, 4), (8320, 6)]
FINISH_S = [1, 63, 64, 65, 2049]


def _cases():
    out = {}
    for m in FWD_M:
        for c in (3, 64, 68):
            for v in FWD_VARIANTS:
                out[f"finalize-m{m}-c{c}-{v}"] = dict(kind="finalize", m=m, c=c, variant=v)
        out[f"moments-m{m}-c68"] = dict(kind="moments", m=m, c=68)
    # counts of the replicas' records; 0: a replica without rows (its mean and M2 are ignored)
    for name, counts in (("w1", [300]), ("w2", [300, 41]), ("w3", [128, 7, 4096]), ("w3-zero", [300, 0, 41])):
        for c in (3, 260):
            out[f"finalize_moments-{name}-c{c}"] = dict(kind="finalize_moments", counts=counts, c=c, variant="bn")
    out["finalize_moments-w2-c68-nogamma"] = dict(kind="finalize_moments", counts=[300, 41], c=68, variant="nogamma")
    out["finalize_moments-w3-c68-nomoving"] = dict(kind="finalize_moments", counts=[128, 7, 4096], c=68,
                                                   variant="nomoving")
    for c in (3, 260):
        for g in (1, 0):
            out[f"infer-c{c}-g{g}"] = dict(kind="infer", c=c, gamma=g)
    for m, c in BWD_SHAPES:
        for use_bn in (1, 0):
            for drop in (0.0, 0.2):
                for kind in ("bwd", "bwd_stats"):
                    out[f"{kind}-m{m}-c{c}-bn{use_bn}-d{drop}"] = dict(kind=kind, m=m, c=c, use_bn=use_bn, drop=drop,
                                                                       runs=1)
    out["bwd_stats-m8320-c4-bn1-d0.2-twice"] = dict(kind="bwd_stats", m=8320, c=4, use_bn=1, drop=0.2, runs=2)
    for S in FINISH_S:
        for c in (4, 64, 68):
            for name, use_bn, grads in (("bn1", 1, 1), ("bn0", 0, 1), ("bn1-nograds", 1, 0)):
                out[f"finish-S{S}-c{c}-{name}"] = dict(kind="finish", S=S, c=c, use_bn=use_bn, grads=grads, runs=1)
    out["finish-S2049-c68-bn1-twice"] = dict(kind="finish", S=2049, c=68, use_bn=1, grads=1, runs=2)
    for c in (3, 260):
        for use_bn in (1, 0):
            out[f"coef-c{c}-bn{use_bn}"] = dict(kind="coef", c=c, use_bn=use_bn)
    return out


CASES = _cases()


def sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().contiguous().numpy())).hexdigest()


def _rand(rng, shape, scale=1.0):
    return (rng.random(shape, dtype=np.float32) - np.float32(0.5)) * np.float32(2 * scale)


class _OneWorkspace(fenced.FencedWorkspace):
    """The same fenced buffer for every get() of one size: a second call finds what the first one left."""

    def get(self, nbytes, device=None):
        if not self.sizes:
            self._buf = super().get(nbytes, device)
        assert int(nbytes) == self.sizes[0]
        return self._buf


def _counters_zero(part, c):
    """The arrival counters, one per 64 channels, are the last words of either kind of partials buffer."""
    return not bool(part[part.numel() - (c + 63) // 64:].view(torch.int32).any())


def _affine(mem, rng, c, variant):
    """gamma, beta, moving mean, moving variance, update_moving and the (mean, rstd, scale, shift) outputs."""
    has_g, has_b, has_mov, upd, has_out, _ = FWD_VARIANTS[variant]
    gamma = mem.inp(_rand(rng, c, 0.5) + 1.5) if has_g else None
    beta = mem.inp(_rand(rng, c, 0.3)) if has_b else None
    mm = mem.inp(_rand(rng, c, 0.2), fence=mem.out_fence) if has_mov else None
    mv = mem.inp(_rand(rng, c, 0.2) + 1.0, fence=mem.out_fence) if has_mov else None
    mean, rstd = (mem.empty(c), mem.empty(c)) if has_out else (None, None)
    return gamma, beta, mm, mv, upd, (mean, rstd, mem.empty(c), mem.empty(c))


def _affine_shas(mm, mv, outs):
    got = {k: sha(t) for k, t in zip(("mean", "rstd", "scale", "shift"), outs) if t is not None}
    if mm is not None:
        got.update(moving_mean=sha(mm), moving_var=sha(mv))
    return got


def _partials(ops, mem, rng, m, c, center):
    """A zeroed partials buffer whose (mean, M2) pairs are those of tiles of unit-variance rows about `center`."""
    nblk = -(-m // 128)
    rows = np.minimum(128, m - 128 * np.arange(nblk)).astype(np.float32)[:, None]
    pairs = np.empty((nblk, c, 2), np.float32)
    pairs[..., 0] = np.float32(center) + _rand(rng, (nblk, c), 0.2)
    pairs[..., 1] = (rows - 1) * (np.float32(1.0) + _rand(rng, (nblk, c), 0.1))
    part = mem.zeros(ops.bn_partials_numel(m, c))
    part[:pairs.size].copy_(torch.from_numpy(pairs.reshape(-1)))
    return part


def _run(ops, mem, case, cid):
    rng = np.random.default_rng(zlib.crc32(cid.encode()))
    kind, c = case["kind"], case["c"]
    if kind in ("finalize", "moments"):
        m = case["m"]
        center = FWD_VARIANTS[case["variant"]][5] if kind == "finalize" else 0.3
        part = _partials(ops, mem, rng, m, c, center)
        if kind == "moments":
            rec = mem.empty(1 + 2 * c, torch.float64)
            ops.bn_moments(part, m, c, rec)
            got = {"record": sha(rec)}
        else:
            gamma, beta, mm, mv, upd, outs = _affine(mem, rng, c, case["variant"])
            ops.bn_finalize(part, m, c, gamma, beta, 1e-3, 0.99, mm, mv, upd, *outs)
            got = _affine_shas(mm, mv, outs)
        assert _counters_zero(part, c), "arrival counters left non-zero"
        return got
    if kind == "finalize_moments":
        counts = case["counts"]
        recs = np.empty((len(counts), 1 + 2 * c), np.float64)
        for r, n in enumerate(counts):
            recs[r, 0] = n
            recs[r, 1:1 + c] = 0.3 + _rand(rng, c, 0.2).astype(np.float64) + rng.random(c) * 1e-9
            recs[r, 1 + c:] = n * (1.0 + _rand(rng, c, 0.1).astype(np.float64)) if n else 7.0
        gamma, beta, mm, mv, upd, outs = _affine(mem, rng, c, case["variant"])
        ops.bn_finalize_moments(mem.inp(recs.reshape(-1), torch.float64), len(counts), c, gamma, beta, 1e-3, 0.99, mm,
                                mv, upd, *outs)
        return _affine_shas(mm, mv, outs)
    if kind == "infer":
        gamma = mem.inp(_rand(rng, c, 0.5) + 1.5) if case["gamma"] else None
        beta, mm, mv = mem.inp(_rand(rng, c, 0.3)), mem.inp(_rand(rng, c, 0.2)), mem.inp(_rand(rng, c, 0.2) + 1.0)
        scale, shift = mem.empty(c), mem.empty(c)
        ops.bn_infer_params(gamma, beta, mm, mv, c, 1e-3, scale, shift)
        return {"scale": sha(scale), "shift": sha(shift)}
    use_bn = bool(case["use_bn"])
    mean, rstd = (mem.inp(_rand(rng, c, 0.1)), mem.inp(_rand(rng, c, 0.5) + 1.5)) if use_bn else (None, None)
    if kind == "coef":
        coef = mem.empty(3 * c)
        ops.bn_bwd_coef(mem.inp(_rand(rng, 2 * c, 40.0)), 300, c, use_bn, mean, rstd, coef)
        return {"coef": sha(coef)}
    got = {}
    if kind == "finish":
        S = case["S"]
        part = mem.zeros(ops.bn_stats_partials_numel(S, c))  # counters zero
        part[:S * 2 * c].copy_(torch.from_numpy(_rand(rng, S * 2 * c, 3.0)))
        for run in range(case["runs"]):
            dg, db = (mem.empty(c) if use_bn else None, mem.empty(c)) if case["grads"] else (None, None)
            coef = mem.empty(3 * c)
            ops.bn_relu_bwd_stats_finish(part, S, 128 * S, c, mean, rstd, use_bn, dg, db, coef)
            got.update({f"{k}{run or ''}": sha(t) for k, t in (("dgamma", dg), ("dbeta", db), ("coef", coef))
                        if t is not None})
        assert _counters_zero(part, c), "arrival counters left non-zero"
        return got
    m, drop = case["m"], case["drop"]
    da, z = mem.inp(_rand(rng, (m, c))), mem.inp(_rand(rng, (m, c)))
    scale, shift = mem.inp(_rand(rng, c, 0.5) + 1.5), mem.inp(_rand(rng, c, 0.3))
    for run in range(case["runs"]):
        dg, db = mem.empty(c) if use_bn else None, mem.empty(c)
        if kind == "bwd":
            out = mem.empty((m, c))
            ops.bn_relu_bwd(da, z, m, c, mean, rstd, scale, shift, use_bn, drop, 55, dg, db, out)
        else:
            out = mem.empty(3 * c)
            ops.bn_relu_bwd_stats(da, z, m, c, mean, rstd, scale, shift, use_bn, drop, 55, dg, db, out)
        got.update({f"{k}{run or ''}": sha(t) for k, t in (("dgamma", dg), ("dbeta", db),
                                                           ("dz" if kind == "bwd" else "coef", out)) if t is not None})
    return got


def run_case(ops, cid):
    """Runs one case inside fresh guard bands; {buffer name: sha256}."""
    mem, ws = fenced.Arena("cuda"), _OneWorkspace("cuda")
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
def test_bn_bits(ops, golden, cid):
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
