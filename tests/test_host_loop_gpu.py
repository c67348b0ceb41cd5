"""The host loop around the train step: test_step, evaluate, fit's epoch logs and the callbacks that
act on them (scripts/train.py:273-316), held to the float64 oracle and to the loop they stand for.

val_mean_io_u decides which weights ModelCheckpoint writes, when EarlyStopping stops and what it
restores, and when ReduceLROnPlateau cuts the learning rate.  Everything here runs at 64 x 64 x 3 in
batches of 1 to 3 images with the default filters.

  * test_step: [loss, dice_coef, iou_coef] within 1e-5 and the probabilities within 2e-5 of
    UNetOracle.forward(training=False) on the device's own weights (the bounds of the train step's
    loss and of the inference forward in test_model_gpu.py), after a train step has dirtied every
    buffer; no launch carries a dropout rate, BatchNorm reads the moving statistics, and nothing a
    later step can see changes.
  * evaluate: the mean of the oracle's per-batch values within 1e-5; the confusion matrix exactly
    that of the device's own probabilities, and the device's decisions those of the oracle wherever
    the oracle's probability is further than 2e-5 from the threshold.  The threshold is the median of
    the oracle's probabilities (helpers.host_loop_case), so both columns of the matrix fill.
  * fit: History equals, float for float, a hand-run loop of train_step / test_step on a second model,
    and both models end bitwise equal.
  * callbacks: a scripted monitor (helpers.scripted_monitor_callback) makes the trajectory known
    without a device; the checkpoint file, the restored weights, the optimizer and a captured predict
    graph are the model's own and are compared with a hand-run model's snapshots bitwise.

With batches of unequal size only the per-batch values and the MeanIoU are asserted: evaluate takes
the unweighted mean of the batch means, and whether Keras weights by batch size is not pinned here.
"""
import numpy as np
import pytest

from helpers import (HOST_LOOP_SIZE, batch, engine_state, fresh_model, host, host_batch,
                     host_loop_case, oracle_values, record_launches, scripted_monitor_callback, set_routes,
                     trace_model, weights_with_stats)
from oracle import keras_ops as K
from oracle.unet_ref import UNetOracle

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

VALUE_TOL = 1e-5  # loss, dice_coef, iou_coef: the train step's bound (test_model_gpu.py, test_carried_state_gpu.py)
PROB_TOL = 2e-5   # inference probabilities (test_model_gpu.py: test_builder_api_and_inference_parity_cfg1)
NAMES = ("loss", "dice_coef", "iou_coef")


def _assert_state_equal(got, want, what, keys=None):
    """Two helpers.engine_state dicts: tensors bitwise, everything else ==."""
    for k in keys or want:
        a, b = got[k], want[k]
        same = torch.equal(a, b) if isinstance(b, torch.Tensor) else a == b
        assert same, f"{what}: {k} differs"


def _mean32(rows):
    """The float32 mean fit and evaluate log: the results summed in order, then divided by their number."""
    acc = np.asarray(rows[0], np.float32).copy()
    for r in rows[1:]:
        acc = acc + np.asarray(r, np.float32)
    return acc / np.float32(len(rows))


def _decisions(prob, thr):
    """(MeanIoU's predicted labels, distance of prob from the nearest decision boundary)."""
    if thr is None:  # truncation of raw probabilities: the boundary is 1
        return np.trunc(prob).astype(np.int64), np.abs(prob - 1.0)
    return (prob > thr).astype(np.int64), np.abs(prob - thr)


def _spy_test_step(model):
    """Record what every test_step of the model (evaluate's too) returns and the probabilities it left."""
    seen, inner = [], model.test_step

    def test_step(x, y):
        res = inner(x, y)
        seen.append((res.detach().cpu().numpy().copy(), host(model.engine.acts(x.shape[0]).prob)))
        return res

    model.test_step = test_step
    return seen


def _spy_result(metric):
    """Record the confusion matrix behind every result() (evaluate puts the training counts back afterwards)."""
    seen, inner = [], metric.result

    def result():
        seen.append(metric.confusion_matrix().copy())
        return inner()

    metric.result = result
    return seen


def _check_validation(logs, batches, oracle_probs, spied, matrix, metric, prefix, record=None):
    """Section "evaluate against the oracle": the logged values against the mean of the oracle's
    per-batch values, the matrix against the device's own probabilities, the decisions against the oracle's."""
    k, thr = metric.num_classes, metric.threshold
    assert len(spied) == len(batches)
    want = np.mean([oracle_values(y, p) for (_, y), p in zip(batches, oracle_probs)], axis=0)
    for i, nm in enumerate(NAMES):
        err = abs(logs[prefix + nm] - want[i])
        if record:
            record(f"{prefix}{nm}_err", err)
        assert err < VALUE_TOL, (nm, logs[prefix + nm], want[i])
    cm = np.zeros((k, k), np.int64)
    near = 0
    for (_, y), p_or, (_, p_dev) in zip(batches, oracle_probs, spied):
        assert np.abs(p_dev - p_or).max() < PROB_TOL
        cm += K.meaniou_confusion(y, p_dev, k, thr)
        d_or, margin = _decisions(p_or, thr)
        far = margin > PROB_TOL
        near += int((~far).sum())
        assert np.array_equal(_decisions(p_dev, thr)[0][far], d_or[far])
    if record:
        record(f"{prefix}near_threshold_pixels", near)
    assert np.array_equal(matrix, cm), (matrix, cm)
    assert logs[prefix + metric.name] == K.meaniou_result(cm)
    return cm


# ------------------------------------------------------------------------------ 1. test_step ---
@pytest.mark.parametrize("ncls,use_bn,loss", [(1, True, "dice_loss"), (1, True, "iou_loss"), (3, True, "dice_loss"),
                                              (1, False, "dice_loss")])
def test_test_step_against_the_oracle(ncls, use_bn, loss, record_property):
    """One train step (dropout 0.2, batch statistics) dirties the Acts, split planes and workspaces;
    then test_step on 2, 3 and 1 images against the inference oracle on the weights read back."""
    from unet_amd.metrics import MeanIoU
    from unet_amd.model import UNetModel
    from unet_amd.optim import AdamW
    cfg = (HOST_LOOP_SIZE, ncls, use_bn, 0.2, {})
    model = UNetModel(HOST_LOOP_SIZE, ncls, dropout_rate=0.2, use_batch_norm=use_bn, device="cuda:0", seed=11)
    set_routes(model, {})
    thr = 0.5 if ncls == 1 else None
    metric = MeanIoU(max(ncls, 2), threshold=thr)
    model.compile(AdamW(learning_rate=2e-3, weight_decay=1e-4), loss, [metric])
    eng = model.engine
    rng = np.random.default_rng(800 + 10 * ncls + use_bn)
    weights_with_stats(model, rng)
    orc = UNetOracle(ncls, 0.2, use_bn)
    worst = dict.fromkeys(NAMES + ("prob",), 0.0)
    confusion = np.zeros((metric.num_classes,) * 2, np.int64)
    with record_launches(eng) as rec:
        model.train_step(*batch(rng, 2, cfg))
        torch.cuda.synchronize()
        first = len(rec.trace)
        w = {name: a.astype(np.float64) for name, a in eng.get_weights_dict().items()}
        before = engine_state(model)
        seeds = eng.drop_seeds(eng.step_count + 1)
        metric.reset_state()
        for n in (2, 3, 1):
            x, y = batch(rng, n, cfg)
            res = model.test_step(x, y).cpu().numpy().astype(np.float64)
            prob_dev = host(eng.acts(n).prob)
            prob = orc.forward(w, host(x), training=False)[0]
            want = oracle_values(host(y), prob)
            if loss == "iou_loss":
                want[0] = 1.0 - want[2]
            errs = dict(zip(NAMES, np.abs(res - want)), prob=np.abs(prob_dev - prob).max())
            print(f"[{ncls},{use_bn},{loss}] batch {n}: test_step {res} (oracle {want}), errors {errs}")
            worst = {nm: max(worst[nm], float(e)) for nm, e in errs.items()}
            confusion += K.meaniou_confusion(host(y), prob_dev, metric.num_classes, thr)
        torch.cuda.synchronize()
    for nm, e in worst.items():
        record_property(f"test_step_{nm}_err", e)
    assert all(worst[nm] < VALUE_TOL for nm in NAMES), worst
    assert worst["prob"] < PROB_TOL, worst
    assert np.array_equal(metric.confusion_matrix(), confusion)
    # nothing a later step can see has changed
    _assert_state_equal(engine_state(model), before, "after three test_steps")
    assert eng.drop_seeds(eng.step_count + 1) == seeds
    # the launches: the train step's carry dropout and batch statistics (so the recording can see both) ...
    blocks = len(eng.blocks)

    def rates(trace):
        return [a["view"][3] for _, _, args in trace for a in args if isinstance(a, dict)]

    def count(trace, prefix):
        return sum(name.startswith(prefix) for name, _, _ in trace)

    train, test = rec.trace[:first], rec.trace[first:]
    assert max(rates(train)) == pytest.approx(0.2)
    assert count(train, "unet_bn_finalize") >= blocks if use_bn else count(train, "unet_bn_finalize") == 0
    # ... and no test_step's launch does
    assert len(rates(test)) >= 3 * blocks and max(rates(test)) == 0.0
    assert count(test, "unet_bn_infer_params") == 3 * blocks
    assert count(test, "unet_bn_finalize") == 0 and count(test, "unet_bn_moments") == 0


# -------------------------------------------------------------------------------- 2. evaluate ---
def _case_model(case, metrics, seed=None):
    """A model of the shared case's configuration holding its weights."""
    model = trace_model(case["cfg"], metrics=metrics, seed=case["seed"] if seed is None else seed)
    model.engine.set_weights_dict(case["w32"])
    got = model.engine.get_weights_dict()
    assert all(np.array_equal(got[k], v) for k, v in case["w32"].items())
    return model


def _case_metric(case):
    from unet_amd.metrics import MeanIoU
    ncls = case["cfg"][1]
    return MeanIoU(max(ncls, 2), threshold=case["threshold"])


def _foreground_share(case):
    return float(np.mean(np.concatenate([p.ravel() for p in case["probs"][:3]]) > case["threshold"]))


@pytest.mark.parametrize("ncls", [1, 3])
def test_evaluate_against_the_oracle(ncls, record_property):
    """evaluate(four batches, steps=3, prefix="val_") with known training counts in the metric."""
    case = host_loop_case(ncls)
    if ncls == 1:  # a condition on the input, not on the device: the threshold splits the oracle's predictions
        assert 0.3 <= _foreground_share(case) <= 0.7
    metric = _case_metric(case)
    model = _case_model(case, ["dice_coef", "iou_coef", metric])
    training_counts = torch.arange(3, 3 + metric.num_classes ** 2, dtype=torch.int64, device=metric.confusion.device) * 7
    metric.confusion.copy_(training_counts)
    spied, matrices = _spy_test_step(model), _spy_result(metric)
    before = engine_state(model)
    logs = model.evaluate(case["batches"], steps=3, prefix="val_")
    assert set(logs) == {"val_loss", "val_dice_coef", "val_iou_coef", "val_mean_io_u"}
    assert all(isinstance(v, float) for v in logs.values())
    assert len(matrices) == 1
    cm = _check_validation(logs, case["batches"][:3], case["probs"][:3], spied, matrices[0], metric, "val_",
                           record_property)
    if ncls == 1:
        assert cm.sum(axis=0).min() > 0.3 * cm.sum()  # both predicted columns are filled
    assert torch.equal(metric.confusion, training_counts), "evaluate did not put the training confusion back"
    _assert_state_equal(engine_state(model), before, "after evaluate")


def test_evaluate_reads_a_single_pass_generator_exactly():
    """A Keras-style flow shared across calls: evaluate(gen, steps=2) consumes exactly two batches, the
    next evaluate(gen, steps=1) sees the third, the one after it the fourth (of another size)."""
    case = host_loop_case(1)
    metric = _case_metric(case)
    model = _case_model(case, ["dice_coef", "iou_coef", metric])
    spied, matrices = _spy_test_step(model), _spy_result(metric)
    consumed = []

    def flow():
        for i, b in enumerate(case["batches"]):
            consumed.append(i)
            yield b

    gen = flow()
    taken = 0
    for steps in (2, 1, 1):
        del spied[:], matrices[:]
        logs = model.evaluate(gen, steps=steps)
        sel = slice(taken, taken + steps)
        taken += steps
        assert consumed == list(range(taken)), f"evaluate(steps={steps}) read batches {consumed}"
        assert set(logs) == {"loss", "dice_coef", "iou_coef", "mean_io_u"}
        _check_validation(logs, case["batches"][sel], case["probs"][sel], spied, matrices[0], metric, "")


def test_evaluate_batches_of_unequal_size():
    """Batches of 2 and 3 images: each batch's values and the MeanIoU over both; the mean of the two
    batch means is not asserted (unweighted here; Keras' weighting is not pinned)."""
    case = host_loop_case(1)
    metric = _case_metric(case)
    model = _case_model(case, ["dice_coef", "iou_coef", metric])
    spied, matrices = _spy_test_step(model), _spy_result(metric)
    batches, probs = case["batches"][2:4], case["probs"][2:4]
    assert batches[0][0].shape[0] != batches[1][0].shape[0]
    logs = model.evaluate(batches, steps=2)
    cm = np.zeros((2, 2), np.int64)
    for (_, y), p_or, (res, p_dev) in zip(batches, probs, spied):
        assert np.abs(res - oracle_values(y, p_or)).max() < VALUE_TOL
        assert np.abs(p_dev - p_or).max() < PROB_TOL
        cm += K.meaniou_confusion(y, p_dev, 2, metric.threshold)
    assert len(spied) == 2 and np.array_equal(matrices[0], cm)
    assert logs["mean_io_u"] == K.meaniou_result(cm)


def test_metric_is_summed_over_the_data_parallel_group():
    """fit and evaluate sum the confusion matrix over the group given to enable_data_parallel, the one
    the gradients and the moving statistics are reduced over, not over the default group (one process
    here: the group is a token and only the argument is looked at; tools/dp_eval_check.py runs two ranks)."""
    case = host_loop_case(1)
    metric = _case_metric(case)
    model = _case_model(case, [metric])
    group = object()
    model.enable_data_parallel(group=group)
    groups, inner = [], metric.all_reduce

    def all_reduce(group=None):
        groups.append(group)
        inner(group)

    metric.all_reduce = all_reduce
    model.evaluate(case["batches"], steps=1)
    assert groups == [group]
    model.fit(case["batches"], epochs=1, steps_per_epoch=1, validation_data=case["batches"], validation_steps=1,
              verbose=0)
    assert groups == [group] * 3  # (evaluate, fit's training metric, fit's validation)


# ------------------------------------------------------------------------------------- 3. fit ---
def _hand_epoch(model, train, val=()):
    """One epoch of the loop fit stands for: reset the metric, the train steps, the float32 mean of
    their results, the metric's result; then the validation steps with a reset metric, after which the
    training counts are put back.  Returns (logs, per-step device probabilities of training and of
    validation, the validation confusion matrix)."""
    metric = model.mean_iou
    metric.reset_state()
    rows, train_probs, val_probs = [], [], []
    for x, y in train:
        rows.append(model.train_step(x, y).cpu().numpy().copy())
        torch.cuda.synchronize()
        train_probs.append(host(model.engine.acts(x.shape[0]).prob))
    logs = dict(zip(NAMES, (float(v) for v in _mean32(rows))))
    logs[metric.name] = metric.result()
    val_matrix = None
    if val:
        saved = metric.confusion.clone()
        metric.reset_state()
        rows = []
        for x, y in val:
            rows.append(model.test_step(x, y).cpu().numpy().copy())
            val_probs.append(host(model.engine.acts(x.shape[0]).prob))
        logs.update(zip(("val_" + nm for nm in NAMES), (float(v) for v in _mean32(rows))))
        logs["val_" + metric.name] = metric.result()
        val_matrix = metric.confusion_matrix().copy()
        metric.confusion.copy_(saved)
    return logs, train_probs, val_probs, val_matrix


FIT_TRAIN_BATCHES = (2, 3, 1, 2, 1, 3)  # three epochs of two steps


def test_fit_equals_the_loop_it_stands_for(record_property):
    case = host_loop_case(1)
    cfg = case["cfg"]
    rng = np.random.default_rng(901)
    train = [host_batch(rng, n, cfg) for n in FIT_TRAIN_BATCHES]
    val = case["batches"][:2]
    a = _case_model(case, ["dice_coef", "iou_coef", _case_metric(case)])
    b = fresh_model(cfg, engine_state(a), ["dice_coef", "iou_coef", _case_metric(case)], seed=case["seed"])
    hist = a.fit(train, epochs=3, steps_per_epoch=2, validation_data=val, validation_steps=2, verbose=0)
    want = {}
    for epoch in range(3):
        logs, train_probs, val_probs, val_matrix = _hand_epoch(b, train[2 * epoch:2 * epoch + 2], val)
        for k, v in logs.items():
            want.setdefault(k, []).append(v)
    assert hist.epoch == [0, 1, 2]
    assert list(hist.history) == ["loss", "dice_coef", "iou_coef", "mean_io_u",
                                  "val_loss", "val_dice_coef", "val_iou_coef", "val_mean_io_u"]
    assert hist.history == want, (hist.history, want)
    torch.cuda.synchronize()
    _assert_state_equal(engine_state(a), engine_state(b), "fit against the hand-run loop")
    assert a.optimizer.iterations == 6 and a.engine.step_count == 6
    # the training metric of the last epoch counts that epoch's two steps alone
    cm = sum(K.meaniou_confusion(y, p, 2, case["threshold"]) for (_, y), p in zip(train[4:6], train_probs))
    assert np.array_equal(a.mean_iou.confusion_matrix(), cm) and np.array_equal(b.mean_iou.confusion_matrix(), cm)
    assert want["mean_io_u"][2] == K.meaniou_result(cm)
    # the last epoch's validation numbers against the oracle on the weights they were computed from
    w = {name: arr.astype(np.float64) for name, arr in b.engine.get_weights_dict().items()}
    orc = UNetOracle(1, 0.2, True)
    probs = [orc.forward(w, x.astype(np.float64), training=False)[0] for x, _ in val]
    record_property("val_oracle_foreground_share", float(np.mean(np.concatenate(probs) > case["threshold"])))
    spied = [(None, p) for p in val_probs]
    _check_validation({k: v[2] for k, v in want.items()}, val, probs, spied, val_matrix, b.mean_iou, "val_",
                      record_property)


# ------------------------------------------------------------------------------- 4. callbacks ---
@pytest.mark.parametrize("graph", [False, True])
def test_callbacks_act_on_the_device_model(graph, tmp_path):
    """Five epochs available, the monitor scripted to 0.5, 0.7, 0.6, 0.6, 0.6: the checkpoint is the
    end of epoch index 1 and is not rewritten, training stops after index 3 with those weights
    restored (the optimizer not rewound), the learning rate is cut after indices 2 and 3, and
    predict -- eager or a graph captured on the initial weights -- sees the restored weights."""
    from unet_amd.callbacks import EarlyStopping, ModelCheckpoint, ReduceLROnPlateau
    case = host_loop_case(1)
    cfg = case["cfg"]
    rng = np.random.default_rng(902)
    pair = [host_batch(rng, 2, cfg), host_batch(rng, 3, cfg)]
    val = case["batches"][:1]
    x = torch.from_numpy(case["batches"][1][0]).cuda()
    a = _case_model(case, ["dice_coef", _case_metric(case)])
    b = fresh_model(cfg, engine_state(a), ["dice_coef", _case_metric(case)], seed=case["seed"])
    a.engine.graph_predict = graph
    lr0 = a.optimizer.learning_rate
    before_fit = a.predict(x)  # graph: captured on the weights fit will replace
    saves, inner = [], a.save_weights

    def save_weights(path):
        saves.append(a.optimizer.iterations)
        inner(path)

    a.save_weights = save_weights
    path = str(tmp_path / "ckpt" / "best.weights.h5")
    hist = a.fit(pair * 5, epochs=5, steps_per_epoch=2, validation_data=val, validation_steps=1, verbose=0,
                 callbacks=[scripted_monitor_callback(),
                            ModelCheckpoint(path, "val_mean_io_u", "max", save_best_only=True),
                            EarlyStopping("val_mean_io_u", patience=2, mode="max", restore_best_weights=True),
                            ReduceLROnPlateau("val_mean_io_u", factor=0.2, patience=1, mode="max", min_lr=1e-6)])
    assert len(hist.epoch) == 4 and hist.epoch == [0, 1, 2, 3] and a.stop_training
    # the hand-run model: the same steps, the learning rate cut after epoch indices 2 and 3
    snapshots = []
    for epoch in range(4):
        for xb, yb in pair:
            b.train_step(xb, yb)
        snapshots.append(b.get_weights())
        if epoch >= 2:
            b.optimizer.learning_rate = max(float(b.optimizer.learning_rate) * 0.2, 1e-6)
    torch.cuda.synchronize()
    best = snapshots[1]
    assert not all(np.array_equal(u, v) for u, v in zip(best, snapshots[3]))
    # the checkpoint: written at the ends of epoch indices 0 and 1 (iterations 2 and 4), never after
    assert saves == [2, 4]
    loaded = trace_model(cfg, seed=case["seed"] + 1)
    loaded.load_weights(path)
    assert all(np.array_equal(u, v) for u, v in zip(loaded.get_weights(), best)), "checkpoint is not epoch index 1"
    assert all(np.array_equal(u, v) for u, v in zip(a.get_weights(), best)), "restored weights are not epoch index 1"
    # restoring weights does not rewind the optimizer
    _assert_state_equal(engine_state(a), engine_state(b), "optimizer after early stopping", ("m", "v", "iterations"))
    assert a.optimizer.iterations == 8
    assert a.optimizer.learning_rate == pytest.approx(lr0 * 0.04)
    assert b.optimizer.learning_rate == a.optimizer.learning_rate
    # set_weights reaches the split planes, the BN parameters and a replayed graph
    after_fit = a.predict(x)
    want = loaded.predict(x)
    torch.cuda.synchronize()
    assert not torch.equal(after_fit, before_fit)
    assert torch.equal(after_fit, want), "predict after fit differs from a fresh model loaded from the checkpoint"
