"""What tests/test_host_loop_gpu.py takes for granted, shown without a device: the callback timeline
that the scripted monitor implies, and that the validation threshold splits the oracle's predictions."""
import numpy as np

from helpers import SCRIPTED_MONITOR, host_loop_case, scripted_monitor_callback


def test_scripted_monitor_timeline_on_a_stub_model(tmp_path):
    """0.5, 0.7, 0.6, 0.6, 0.6 through unet_amd.callbacks as scripts/train.py wires them: the
    checkpoint is written after epoch indices 0 and 1 only, the learning rate is cut after indices 2
    and 3, training stops after index 3 and the weights of the end of index 1 come back."""
    from unet_amd.callbacks import CallbackList, EarlyStopping, ModelCheckpoint, ReduceLROnPlateau

    class Optimizer:
        learning_rate = 2e-3

    class Model:
        optimizer = Optimizer()
        stop_training = False
        weights = [np.full(1, -1.0)]
        saved = []

        def get_weights(self):
            return [w.copy() for w in self.weights]

        def set_weights(self, weights):
            self.weights = weights

        def save_weights(self, path):
            self.saved.append((path, float(self.weights[0][0])))

    model = Model()
    path = str(tmp_path / "best.weights.h5")
    cbs = CallbackList([scripted_monitor_callback(),
                        ModelCheckpoint(path, "val_mean_io_u", "max", save_best_only=True),
                        EarlyStopping("val_mean_io_u", patience=2, mode="max", restore_best_weights=True),
                        ReduceLROnPlateau("val_mean_io_u", factor=0.2, patience=1, mode="max", min_lr=1e-6)], model)
    cbs.on_train_begin()
    rates, ran = [], 0
    for epoch in range(len(SCRIPTED_MONITOR)):
        cbs.on_epoch_begin(epoch)
        model.weights = [np.full(1, float(epoch))]  # "training": the weights of the end of this epoch
        logs = {"val_mean_io_u": 0.123}  # what validation measured; the script replaces it
        cbs.on_epoch_end(epoch, logs)
        assert logs["val_mean_io_u"] == SCRIPTED_MONITOR[epoch]
        rates.append(model.optimizer.learning_rate)
        ran += 1
        if model.stop_training:
            break
    cbs.on_train_end()
    assert ran == 4
    assert model.saved == [(path, 0.0), (path, 1.0)]
    assert model.weights[0][0] == 1.0
    assert rates[:2] == [2e-3, 2e-3]
    assert np.allclose(rates[2:], [2e-3 * 0.2, 2e-3 * 0.04], rtol=1e-12, atol=0)


def test_validation_threshold_splits_the_oracle_predictions():
    """The binary validation case of the GPU tests: the oracle's probabilities lie in a narrow band
    (a MeanIoU at a threshold outside it fills one column of the confusion matrix), and the case's
    threshold, their median, puts between 30% and 70% of the pixels in the foreground -- of the three
    evaluated batches together and of each batch, the extra one included."""
    case = host_loop_case(1)
    t = case["threshold"]
    assert t == float(np.float32(t))  # the metric kernel's threshold argument is a float
    probs = case["probs"]
    flat = np.concatenate([p.ravel() for p in probs[:3]])
    print(f"oracle probabilities {flat.min():.6f}..{flat.max():.6f}, threshold {t:.8f}, "
          f"foreground share {np.mean(flat > t):.4f}, at 0.5: {np.mean(flat > 0.5):.4f}")
    assert flat.max() - flat.min() < 0.05
    assert 0.3 <= np.mean(flat > t) <= 0.7
    for p in probs:
        assert 0.3 <= np.mean(p > t) <= 0.7
    assert [b[0].shape[0] for b in case["batches"]] == [2, 2, 2, 3]
