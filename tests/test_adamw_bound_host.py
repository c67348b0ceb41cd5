"""The rounding-error bound that the device AdamW tests rest on (oracle.keras_ops.adamw_update_bound),
checked without a GPU: the kernel's update restated in float32 NumPy -- one rounding after every
operation, no contraction -- must stay within 1 x the bound of the float64 restatement, elementwise,
on the moment states of the device tests (zero, warm, cancelling, underflowing), 2 M elements each.
The device tests allow 2 x the bound."""
import numpy as np
import pytest

from helpers import ADAMW_STATES, adamw_case, adamw_f32, bound_ratio
from oracle import keras_ops as K

N = 2_000_000
HYPER = dict(lr=2e-3, wd=1e-4, beta1=0.9, beta2=0.999, eps=1e-7)


def _alpha(t):
    t = np.float32(t)
    return float(np.float32(HYPER["lr"]) * np.sqrt(np.float32(1) - np.float32(HYPER["beta2"]) ** t)
                 / (np.float32(1) - np.float32(HYPER["beta1"]) ** t))


@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
@pytest.mark.parametrize("state", sorted(ADAMW_STATES))
def test_float32_restatement_within_bound(state, grad_scale, record_property):
    rng = np.random.default_rng(sorted(ADAMW_STATES).index(state) + 10)
    p, g, m, v = adamw_case(rng, N, state, grad_scale)
    alpha = _alpha(ADAMW_STATES[state])
    ref, bound = K.adamw_update_bound(p, g, m, v, alpha=alpha, grad_scale=grad_scale, **HYPER)
    got = adamw_f32(p, g, m, v, alpha=alpha, grad_scale=grad_scale, **HYPER)
    for name, a, r, b in zip("pmv", got, ref, bound):
        assert np.isfinite(r).all() and np.isfinite(b).all(), name
        ratio = bound_ratio(a, r, b)
        record_property(f"ratio_{name}", ratio)
        print(f"adamw bound [{state}, gs {grad_scale}] {name}: max error / bound = {ratio:.3f}")
        assert ratio <= 1.0, (name, ratio)


def test_bound_agrees_with_the_keras_restatement():
    """The operation-by-operation float64 values are K.adamw_update's (same formula, float64 constants
    there, float32-rounded ones here), and a zero gradient on zero moments moves nothing but the decay."""
    rng = np.random.default_rng(3)
    p, g, m, v = adamw_case(rng, 4096, "warm")
    (rp, rm, rv), _ = K.adamw_update_bound(p, g, m, v, alpha=_alpha(7), **HYPER)
    kp, km, kv = K.adamw_update(p, g, m, v, 7, HYPER["lr"], HYPER["wd"])
    for a, b in ((rp, kp), (rm, km), (rv, kv)):
        assert np.abs(a - b).max() <= 1e-6 * np.abs(b).max()
    p, g, m, v = adamw_case(rng, 170, "zero")
    (rp, rm, rv), (bp, bm, bv) = K.adamw_update_bound(p, g, m, v, alpha=_alpha(1), **HYPER)
    z = slice(0, None, 17)
    assert not rm[z].any() and not rv[z].any() and bm[z].max() < 1e-37 and bv[z].max() < 1e-37  # (underflow terms only)
    lr_wd = np.float64(np.float32(HYPER["lr"]) * np.float32(HYPER["wd"]))
    assert np.array_equal(rp[z], p[z] - p[z] * lr_wd)
