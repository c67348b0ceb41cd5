"""Train steps 2..K: what a long-running engine carries from step to step, held two ways.

Bit for bit: the reductions are in fixed order and workspace contents do not matter, so a step of an
engine that has run before -- dirty activation buffers of several batch sizes, a cached plan, grown
workspaces, split planes of an earlier forward, an inference or a route change in between -- must
equal the first step of a fresh engine that is given only the visible state (helpers.engine_state:
weights, moving statistics, Adam moments, counters, learning rate).  No tolerance, no redraw.

Against the float64 oracle (model/u_net.py:28-116, keras.optimizers.AdamW of scripts/train.py:226),
restarted from the device's own state before every step ("teacher forcing"): the forward's loss, dice
and moving statistics; the AdamW update of the whole flat buffer elementwise within 2 x the rounding
bound of the kernel's operation sequence (oracle.keras_ops.adamw_update_bound); the MeanIoU confusion
matrix exactly.  Gradients of steps >= 2 are not compared with the oracle: the bitwise half makes
step k the first step of a fresh engine, which test_train_step_parity holds to the oracle where the
ReLU / max-pool decisions agree.
"""
import numpy as np
import pytest

from helpers import (TRACE_CONFIGS, bound_ratio, engine_state, fresh_model, fresh_step, host, record_launches, rel_err,
                     set_routes, step_outputs, trace_model)
from helpers import batch as _batch
from oracle import keras_ops as K
from oracle.unet_ref import UNetOracle

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _assert_same(cont, fresh, what):
    for k, a in cont.items():
        b = fresh[k]
        if not torch.equal(a, b):
            d = (a.double() - b.double()).abs()
            pytest.fail(f"{what}: {k} of the continued engine differs from the fresh engine's in "
                        f"{int((a != b).sum())} of {a.numel()} elements, max |diff| {float(d.max()):.3e}")


def _train_and_check(model, cfg, x, y, what, check=True, metrics=None, attrs=None):
    """One train step of the continued model; check: bit for bit against a fresh engine's step."""
    state = engine_state(model) if check else None
    res = model.train_step(x, y)
    if check:
        _assert_same(step_outputs(model, res, x.shape[0]), fresh_step(cfg, state, x, y, metrics, attrs=attrs), what)


@pytest.mark.parametrize("cid", ["A", "D", "E", "G", "I", "K", "L", "M"])
def test_steady_steps_equal_a_fresh_engine(cid):
    cfg = TRACE_CONFIGS[cid]
    model = trace_model(cfg)
    rng = np.random.default_rng(100 + ord(cid))
    for k in (1, 2, 3):
        x, y = _batch(rng, 2, cfg)
        _train_and_check(model, cfg, x, y, f"{cid} step {k}", check=k >= 2)


@pytest.mark.parametrize("cid", ["A", "L"])
def test_batch_size_changes_equal_a_fresh_engine(cid):
    """Batch 2, 3, 1, 2: step 3 is a new size beside two dirty Acts, step 4 returns to a dirty one."""
    cfg = TRACE_CONFIGS[cid]
    model = trace_model(cfg)
    rng = np.random.default_rng(200 + ord(cid))
    for k, n in enumerate((2, 3, 1, 2), 1):
        x, y = _batch(rng, n, cfg)
        _train_and_check(model, cfg, x, y, f"{cid} step {k} (batch {n})", check=k >= 3)


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("cid", ["A", "K"])
def test_inference_between_steps_equals_a_fresh_engine(cid, graph):
    """train, predict, test_step (MeanIoU), predict at another batch size, a training-mode forward,
    train: validation between epochs shares the Acts, the split planes and the workspaces with training."""
    from unet_amd.metrics import MeanIoU
    cfg = TRACE_CONFIGS[cid]
    model = trace_model(cfg, metrics=[MeanIoU(2, threshold=0.5)])
    model.engine.graph_predict = graph
    rng = np.random.default_rng(300 + ord(cid))

    def predict_and_check(n, what):
        x, _ = _batch(rng, n, cfg)
        state = engine_state(model)
        got = model.predict(x)
        want = fresh_model(cfg, state).predict(x)  # (eager: graph_predict is pinned off by the defaults)
        torch.cuda.synchronize()
        assert torch.equal(got, want), f"{cid} graph={graph}: {what} differs from a fresh engine's"

    _train_and_check(model, cfg, *_batch(rng, 2, cfg), "", check=False)
    predict_and_check(2, "predict (batch 2) after a train step")
    model.test_step(*_batch(rng, 2, cfg))
    predict_and_check(3, "predict (batch 3) after a test_step")
    model(_batch(rng, 2, cfg)[0], training=True)
    _train_and_check(model, cfg, *_batch(rng, 2, cfg), f"{cid} graph={graph}: the train step after inference",
                     metrics=[MeanIoU(2, threshold=0.5)])


def test_route_changes_equal_a_fresh_engine():
    """One model: two steps as A, one with E's attributes, one with I's, one as A again (the plan
    cache is keyed by the attributes; the split planes of I's step are not refreshed)."""
    cfg = TRACE_CONFIGS["A"]
    model = trace_model(cfg)
    rng = np.random.default_rng(400)
    for k, cid in enumerate(("A", "A", "E", "I", "A"), 1):
        attrs = TRACE_CONFIGS[cid][4]
        set_routes(model, attrs)
        x, y = _batch(rng, 2, cfg)
        _train_and_check(model, cfg, x, y, f"step {k} (routes of {cid})", check=k >= 3, attrs=attrs)


def test_learning_rate_change_equals_a_fresh_engine():
    """What ReduceLROnPlateau does between epochs: optimizer.learning_rate rewritten mid-run."""
    cfg = TRACE_CONFIGS["A"]
    model = trace_model(cfg)
    rng = np.random.default_rng(500)
    for k in (1, 2, 3):
        if k == 3:
            model.optimizer.learning_rate *= 0.2
        x, y = _batch(rng, 2, cfg)
        _train_and_check(model, cfg, x, y, f"step {k}", check=k == 3)
    assert model.optimizer.learning_rate == pytest.approx(4e-4)


def test_dropout_seeds_differ_from_step_to_step():
    """Two engines that both repeat a seed agree with each other, so the bitwise tests cannot see it:
    the seeds that the launches of consecutive steps receive must differ at every site."""
    from unet_amd.engine import DROP_SITES
    cfg = TRACE_CONFIGS["A"]
    model = trace_model(cfg)
    eng = model.engine
    rng = np.random.default_rng(600)
    used = []
    with record_launches(eng) as rec:
        for k in (1, 2, 3):
            first = len(rec.trace)
            model.train_step(*_batch(rng, 2, cfg))
            used.append({a["view"][4] for _, _, args in rec.trace[first:] for a in args
                         if isinstance(a, dict) and a["view"][3] > 0})
    torch.cuda.synchronize()
    for k, seen in enumerate(used, 1):
        want = eng.drop_seeds(k)
        assert len(set(want.values())) == len(DROP_SITES) and 0 not in want.values()
        assert seen == set(want.values()), f"step {k}: the launches' dropout seeds are not drop_seeds({k})"
        if k > 1:
            prev = eng.drop_seeds(k - 1)
            assert all(prev[s] != want[s] for s in DROP_SITES)
            assert not (seen & used[k - 2]), f"steps {k - 1} and {k} share a dropout seed"


ORACLE_BATCHES = (2, 3, 2, 2)


@pytest.mark.parametrize("ncls,use_bn,drop", [(1, True, 0.2), (3, True, 0.0), (1, False, 0.2)])
def test_steps_against_the_oracle_teacher_forced(ncls, use_bn, drop, record_property):
    """K = 4 steps at 64 x 64 (batch 2, 3, 2, 2; learning rate x 0.2 before step 3), the float64
    oracle restarted from the device's weights, statistics, moments and seeds before each step.

    The largest AdamW error / bound per buffer is recorded as `adamw_ratio_*` (measured on an
    MI355X: params 0.835, m 0.908, v 0.997; plain float32 NumPy reaches the same)."""
    from unet_amd.metrics import MeanIoU
    from unet_amd.model import UNetModel
    from unet_amd.optim import AdamW
    size = (64, 64, 3)
    cfg = (size, ncls, use_bn, drop, {})
    model = UNetModel(size, ncls, dropout_rate=drop, use_batch_norm=use_bn, device="cuda:0", seed=11)
    thr = 0.5 if ncls == 1 else None
    metric = MeanIoU(max(ncls, 2), threshold=thr)
    opt = AdamW(learning_rate=2e-3, weight_decay=1e-4)
    model.compile(opt, "dice_loss", [metric])
    eng = model.engine
    orc = UNetOracle(ncls, drop, use_bn)
    rng = np.random.default_rng(700 + ncls + 2 * use_bn)
    confusion = np.zeros((metric.num_classes,) * 2, np.int64)
    worst = {"param": 0.0, "m": 0.0, "v": 0.0}
    for k, n in enumerate(ORACLE_BATCHES, 1):
        if k == 3:
            opt.learning_rate *= 0.2
        x, y = _batch(rng, n, cfg)
        w = {name: a.astype(np.float64) for name, a in eng.get_weights_dict().items()}
        before = engine_state(model)
        seeds = eng.drop_seeds(eng.step_count + 1)
        res = model.train_step(x, y).cpu().numpy()
        torch.cuda.synchronize()
        prob_dev = host(eng.acts(n).prob)  # (synchronised and copied before the next step overwrites it)
        assert opt.iterations == k and eng.step_count == k
        # forward: loss, dice, moving statistics
        x64, y64 = host(x), host(y)
        prob, _, new_stats = orc.forward(w, x64, training=True, drop_seeds=seeds if drop > 0 else None)
        loss, dice = K.dice_loss(y64, prob), K.dice_coef(y64, prob)
        print(f"[{ncls},{use_bn},{drop}] step {k}: loss {res[0]:.7f} (oracle {loss:.7f}), dice {res[1]:.7f} ({dice:.7f})")
        assert abs(res[0] - loss) < 1e-5, (k, res[0], loss)
        assert abs(res[1] - dice) < 1e-5, (k, res[1], dice)
        after = eng.get_weights_dict()
        assert set(new_stats) == {s.name for s in eng.specs if not s.trainable}
        for name, ref in new_stats.items():
            assert rel_err(after[name], ref) < 1e-4, (k, name)
        # AdamW: the kernel's update restated in float64 from the pre-step state and the device's own gradient
        ref, bound = K.adamw_update_bound(host(before["params"]), host(eng.grads), host(before["m"]), host(before["v"]),
                                          lr=opt.learning_rate, wd=opt.weight_decay, beta1=opt.beta_1, beta2=opt.beta_2,
                                          eps=opt.epsilon, alpha=opt.alpha(k), grad_scale=1.0)
        ratios = {nm: bound_ratio(host(t), r, b)
                  for nm, t, r, b in zip(worst, (eng.params, opt._m, opt._v), ref, bound)}
        print(f"[{ncls},{use_bn},{drop}] step {k}: AdamW max error / bound = {ratios}")
        assert all(r <= 2.0 for r in ratios.values()), (k, ratios)
        worst = {nm: max(worst[nm], r) for nm, r in ratios.items()}
        confusion += K.meaniou_confusion(y64, prob_dev, metric.num_classes, thr)
    for nm, r in worst.items():
        record_property(f"adamw_ratio_{nm}", r)
    assert np.array_equal(metric.confusion_matrix(), confusion)
