"""Networks off the default filters (helpers.GEOMETRIES) on the device, through the C ABI like the rest:
the composition of plan.plan_step's routes, the split-plane arena and the kernels one after another at
channel counts, depths and non-square sizes the default (64, 128, 256, 512) network never visits.

Per geometry, one test:
  * one train step against the float64 oracle with the gates of test_train_step_parity
    (helpers.train_step_parity: loss and dice 1e-5, every gradient max(1e-3, 2 x the float32 oracle's
    own error), post-AdamW weights and moving statistics 1e-4, equal key sets), on inputs re-drawn until
    the ReLU / max-pool decisions agree with float64 (at most 10 draws);
  * a second step from the carried state, bitwise equal to the first step of a fresh engine that is
    given the visible state only (as tests/test_carried_state_gpu.py);
  * predict against the oracle's inference forward: within the README's 1e-3, and within
    max(2e-6, 2 x the float32 oracle forward's own max error against float64 on the same inputs).
On two64_nodrop and wide80, predict through a captured graph is bitwise equal to the eager one.

Every case's worst error / gate ratios are recorded as properties and, with UNET_PARITY_LOG set,
appended to that file (profiles/geometry_parity.jsonl is such a run on an MI355X).
"""
import json
import os

import numpy as np
import pytest

from helpers import (GEOMETRIES, GEOMETRY_ENGINE_SEED, engine_state, fresh_step, geometry_cfg, geometry_draw, host,
                     step_outputs, train_step_parity, trace_model)
from helpers import batch as _batch
from oracle.unet_ref import UNetOracle

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GRAPH_CASES = ("two64_nodrop", "wide80")
PREDICT_HARD, PREDICT_FLOOR = 1e-3, 2e-6


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_geometry_against_the_oracle(name, record_property):
    cfg, filters, n = geometry_cfg(name)
    size, ncls, use_bn, drop, attrs = cfg
    model = trace_model(cfg, seed=GEOMETRY_ENGINE_SEED, filters=filters)
    eng = model.engine
    assert eng.filters == tuple(filters) and eng.fuse_sepconv == GEOMETRIES[name][5]
    orc = UNetOracle(ncls, drop, use_bn, filters)

    def draw(attempt):
        w32, x, y = geometry_draw(name, attempt)
        eng.set_weights_dict(w32)
        return {k: v.astype(np.float64) for k, v in w32.items()}, x, y

    row = {"test": f"geometry[{name}]"}
    row.update(train_step_parity(model, orc, draw))

    # a second step from the carried state: the first step of a fresh engine, bit for bit
    rng = np.random.default_rng(77)
    x2, y2 = _batch(rng, n, cfg)
    state = engine_state(model)
    cont = step_outputs(model, model.train_step(x2, y2), n)
    fresh = fresh_step(cfg, state, x2, y2, seed=GEOMETRY_ENGINE_SEED, filters=filters)
    for k, a in cont.items():
        assert torch.equal(a, fresh[k]), (f"{name}: {k} of the second step differs from a fresh engine's in "
                                          f"{int((a != fresh[k]).sum())} of {a.numel()} elements")

    # predict (moving statistics, no dropout) on the twice-trained weights
    xp, _ = _batch(rng, n, cfg)
    w32 = eng.get_weights_dict()
    prob = host(model.engine.predict(xp))
    x64 = host(xp)
    ref = orc.forward({k: v.astype(np.float64) for k, v in w32.items()}, x64, training=False)[0]
    p32 = orc.forward(w32, x64.astype(np.float32), training=False)[0]
    assert p32.dtype == np.float32 and prob.shape == ref.shape == (n,) + tuple(size[:2]) + (ncls,)
    e, e32 = float(np.abs(prob - ref).max()), float(np.abs(p32.astype(np.float64) - ref).max())
    gate = max(PREDICT_FLOOR, 2.0 * e32)
    row.update(predict_err=e, predict_err_oracle32=e32, predict=e / gate)
    print(f"geometry[{name}]: predict max error {e:.3e} (float32 oracle {e32:.3e}, gate {gate:.3e})")

    if name in GRAPH_CASES:
        eager = eng.predict(xp)
        eng.graph_predict = True
        first, replay = eng.predict(xp), eng.predict(xp)  # the capture's call, then a replay of it
        eng.graph_predict = False
        torch.cuda.synchronize()
        row["graph_bitwise"] = bool(torch.equal(first, eager) and torch.equal(replay, eager))

    for k, v in row.items():
        if k != "test":
            record_property(k, v)
    print(json.dumps(row))
    log = os.environ.get("UNET_PARITY_LOG")
    if log:
        with open(log, "a") as f:
            f.write(json.dumps(row) + "\n")
    assert np.isfinite(prob).all() and e < PREDICT_HARD, (e, PREDICT_HARD)
    assert e <= gate, (e, gate, e32)
    assert row.get("graph_bitwise", True), f"{name}: predict through the captured graph differs from eager"
