"""Inference latency, eager vs the captured HIP graph (UNetEngine.graph_predict): ms per predict()
call at 256x256x3 (configs[1]'s network) for a few batch sizes, device-resident input, median of
timed calls after warm-up.  Usage: python tools/bench_predict.py [--frozen] [--int8] [sizes...]

--frozen also times the frozen fp16 network (UNetModel.freeze()): per batch size the three
variants alternate round by round in one process on the same device-resident input, and the JSON
line gains frozen_ms and frozen_speedup_vs_graph.

--int8 (beside --frozen) adds the frozen int8 network (UNetModel.freeze(dtype="int8"), calibrated
on 8 random images) as a fourth variant in the same alternation; the line gains int8_ms,
int8_over_f16 (int8_ms / frozen_ms, < 1 is faster) and int8_max_abs_diff against the graph."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "unet-image-segmentation_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from unet_amd.model import UNetModel  # noqa: E402


def _once(fn):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def timed(fn, reps=50):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    return 1e3 * float(np.median([_once(fn) for _ in range(reps)]))


def timed_alternating(fns, reps=50):
    """Median ms of each callable, one call of each per round (so drift hits all alike)."""
    for fn in fns:
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for t, fn in zip(ts, fns):
            t.append(_once(fn))
    return [1e3 * float(np.median(t)) for t in ts]


def main():
    args = sys.argv[1:]
    frozen = "--frozen" in args
    int8 = "--int8" in args
    if int8 and not frozen:
        sys.exit("--int8 is timed beside --frozen: pass both")
    batches = [int(a) for a in args if a not in ("--frozen", "--int8")] or [1, 4, 16]
    model = UNetModel((256, 256, 3), 1, dropout_rate=0.2, device="cuda:0")
    eng = model.engine
    fz = model.freeze() if frozen else None
    rng = np.random.default_rng(5)
    fq = model.freeze(dtype="int8", calibration=rng.random((8, 256, 256, 3), dtype=np.float32),
                      batch_size=4) if int8 else None

    def eager(x):
        eng.graph_predict = False
        return eng.predict(x)

    def graph(x):
        eng.graph_predict = True
        return eng.predict(x)

    for n in batches:
        x = torch.as_tensor(rng.random((n, 256, 256, 3), dtype=np.float32), device="cuda:0")
        if int8:
            t_e, t_g, t_f, t_q = timed_alternating([lambda: eager(x), lambda: graph(x), lambda: fz.predict(x),
                                                    lambda: fq.predict(x)])
        elif frozen:
            t_e, t_g, t_f = timed_alternating([lambda: eager(x), lambda: graph(x), lambda: fz.predict(x)])
        else:
            t_e = timed(lambda: eager(x))
            t_g = timed(lambda: graph(x))
        g = graph(x)
        same = bool(torch.equal(eager(x), g))
        rec = {"batch": n, "eager_ms": round(t_e, 3), "graph_ms": round(t_g, 3),
               "speedup": round(t_e / t_g, 3), "img_per_s_graph": round(n / t_g * 1e3, 1),
               "equal": same}
        if frozen:
            rec.update(frozen_ms=round(t_f, 3), frozen_speedup_vs_graph=round(t_g / t_f, 3),
                       img_per_s_frozen=round(n / t_f * 1e3, 1),
                       frozen_max_abs_diff=float((fz.predict(x) - g).abs().max()))
        if int8:
            rec.update(int8_ms=round(t_q, 3), int8_over_f16=round(t_q / t_f, 3),
                       img_per_s_int8=round(n / t_q * 1e3, 1),
                       int8_max_abs_diff=float((fq.predict(x) - g).abs().max()))
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
