"""uint8 images in host memory -> uint8 masks in host memory: the host image path (NumPy resizes
around model.predict, what scripts/inference.py does by default) against the device path
(model.predict_masks), end to end, in one process.  Usage:

    python tools/bench_imageproc.py [--reps 5] > profiles/imageproc_predict.txt

Rows: model (fp32 UNetModel with graph replay, and the int8 frozen network made from it) x image
size (the two 960x540 sample images; synthetic 1080x1920 and 3000x4000) x batch (1, 32).  A batch
repeats its one or two distinct images, so the host arrays stay small; every copy is still uploaded
and processed.  Each path is warmed up, then timed `reps` times with a host clock that stops after
the masks are in host memory, the two paths alternating; the median is reported.  A host run that
takes more than 5 s is timed once (the 3000x4000 batches take about a minute each).

Per row, ms per image:
  host    total, and its parts by host clock: pre (reverse, /255, resize), predict, post (resize
          back, threshold)
  device  total; resize / predict / mask are device-event times around the kernels (a second,
          instrumented pass; they exclude upload, copy-back and launch gaps, which is why they do
          not add up to the total)
  mask_GBps  the mask kernel's store bandwidth: mask bytes / its event time (one launch per image)

The last line times what stays on the host after either path, the contour / crop search
(imageproc.largest_external_contour), on the reference's two 960x540 sample masks
(--only-contour prints that line alone).

    python tools/bench_imageproc.py --contour [--reps 5] > profiles/contour_predict.txt

prints the device contour section instead (csrc/contour.hip, predict_masks(..., return_boxes=True)):
  per mask (the two 960x540 sample masks; one of them enlarged, nearest neighbour, to 1080x1920 and
  3000x4000): device_ms, HIP-event time around the ten launches of ops.mask_largest_contour alone
  (median); tracer_ms, imageproc.largest_external_contour on the host in the same run (timed once
  when it takes more than 2 s); filled_ms, the NumPy closed form, from 1080x1920 up; and whether
  the device record equals the host's answer;
  per size and batch: predict_masks end to end (host clock, masks and boxes in host memory), ms per
  image, without and with return_boxes, alternating; the host tracer (960x540 only: the network has
  random weights) and the closed form on the masks that came back, and whether the boxes equal the
  closed form's.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "unet-image-segmentation_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from unet_amd import ops  # noqa: E402
from unet_amd.imageproc import largest_external_contour, resize_linear  # noqa: E402
from unet_amd.model import UNetModel  # noqa: E402

H = W = 256
THR = 0.5
SAMPLES = os.path.join(ROOT, "tests", "golden", "samples")


def host_path(model, images, parts=None):
    """The default path of scripts/inference.py, a batch at a time."""
    t0 = time.perf_counter()
    x = np.concatenate([resize_linear(a[..., ::-1].copy().astype(np.float32) / 255.0, H, W)[None] for a in images])
    t1 = time.perf_counter()
    prob = model.predict(x, batch_size=len(images))
    t2 = time.perf_counter()
    masks = [(resize_linear(p[..., 0], a.shape[0], a.shape[1]) > THR).astype(np.uint8) * 255
             for p, a in zip(prob, images)]
    t3 = time.perf_counter()
    if parts is not None:
        parts.append((t1 - t0, t2 - t1, t3 - t2))
    return masks


def device_path(model, images):
    return model.predict_masks(images, threshold=THR, batch_size=len(images), bgr=True)


def _clock(fn):
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def device_parts(model, images, reps):
    """Median device-event ms of the resize launches, the predict and the mask launches of a batch."""
    res, msk, prd = [], [], []
    for _ in range(reps):
        ops.TIMER = ops.KernelTimer(names=("unet_image_resize_u8", "unet_mask_resize"))
        try:
            _, _, x = model.predict_masks(images, threshold=THR, batch_size=len(images), bgr=True, return_probs=True)
            s = ops.TIMER.summary()
        finally:
            ops.TIMER = None
        res.append(s["unet_image_resize_u8"]["ms"])
        msk.append(s["unet_mask_resize"]["ms"])
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        model.predict(x, batch_size=len(images))
        e1.record()
        torch.cuda.synchronize()
        prd.append(e0.elapsed_time(e1))
    return float(np.median(res)), float(np.median(prd)), float(np.median(msk))


def contour_remainder(reps):
    from PIL import Image
    rec = {"step": "largest_external_contour (host, after either path)", "size": "960x540"}
    for n in ("brazil_passport", "chile_id_card"):
        m = np.asarray(Image.open(os.path.join(SAMPLES, "usage", n + "_output_mask.png")).convert("L"))
        largest_external_contour(m)
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            largest_external_contour(m)
            ts.append(time.perf_counter() - t0)
        rec[n + "_ms"] = round(1e3 * float(np.median(ts)), 2)
    print(json.dumps(rec), flush=True)


def _median_ms(fn, reps, once_above=2.0):
    t0 = time.perf_counter()
    out = fn()
    first = time.perf_counter() - t0
    ts = [first]
    if first <= once_above:
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts)), out


def contour_section(reps, sizes, batches):
    from PIL import Image

    from unet_amd.imageproc import largest_external_contour_filled, resize_nearest
    from unet_amd.pipeline import decode_contour_box
    assert torch.cuda.is_available(), "bench_imageproc needs the MI355X"
    print(f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; reps {reps}", flush=True)
    print("# device contour step per mask: HIP-event ms of the launches alone | host tracer | NumPy closed form",
          flush=True)
    names = ("brazil_passport", "chile_id_card")
    sample = [np.asarray(Image.open(os.path.join(SAMPLES, "usage", n + "_output_mask.png")).convert("L"))
              for n in names]
    masks = [(f"960x540 {n}", m) for n, m in zip(names, sample)]
    big = [tuple(int(v) for v in s.split("x")) for s in sizes if s != "sample"]
    masks += [(f"{h}x{w} {names[0]} enlarged", np.ascontiguousarray(resize_nearest(sample[0], h, w))) for h, w in big]
    for name, m in masks:
        dm = torch.from_numpy(m.copy()).to("cuda:0")
        out = ops.mask_largest_contour(dm)
        for _ in range(3):
            ops.mask_largest_contour(dm, out)
        torch.cuda.synchronize()
        ts = []
        for _ in range(max(reps, 10)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.mask_largest_contour(dm, out)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        box = decode_contour_box(out.cpu().numpy().tobytes())
        tracer_ms, ref = _median_ms(lambda: largest_external_contour(m), reps)
        rec = {"mask": name, "device_ms": round(float(np.median(ts)), 4), "device_min_ms": round(float(min(ts)), 4),
               "tracer_ms": round(tracer_ms, 2)}
        if m.size >= 1080 * 1920:
            rec["filled_ms"] = round(_median_ms(lambda: largest_external_contour_filled(m), reps)[0], 2)
        rec["tracer_over_device"] = round(tracer_ms / float(np.median(ts)), 1)
        rec["box"] = box
        rec["same_as_tracer"] = bool(box == ref)
        print(json.dumps(rec), flush=True)

    print("# predict_masks end to end, ms per image (host clock): masks only | masks and boxes", flush=True)
    rng = np.random.default_rng(5)
    model = UNetModel((H, W, 3), 1, dropout_rate=0.2, device="cuda:0")
    model.engine.graph_predict = True
    sources = {"960x540": [np.asarray(Image.open(os.path.join(SAMPLES, n + ".png")).convert("RGB")) for n in names]}
    for h, w in big:
        sources[f"{h}x{w}"] = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8)]
    for size, src in sources.items():
        for n in batches:
            images = [src[i % len(src)] for i in range(n)]
            run = {False: (lambda: model.predict_masks(images, threshold=THR, batch_size=n, bgr=True)),
                   True: (lambda: model.predict_masks(images, threshold=THR, batch_size=n, bgr=True,
                                                      return_boxes=True))}
            for _ in range(2):
                run[False]()
                got_masks, got_boxes = run[True]()
            t = {False: [], True: []}
            for _ in range(reps):
                for k in (False, True):
                    t[k].append(_clock(run[k])[0])
            k = len(src)
            # the network has random weights: its masks can hold thousands of components, which the tracer
            # walks one by one, so it is timed on the 960x540 masks only
            tracer_ms = (_median_ms(lambda: [largest_external_contour(a) for a in got_masks[:k]], reps)[0]
                         if got_masks[0].size < 1080 * 1920 else None)
            filled_ms, ref = _median_ms(lambda: [largest_external_contour_filled(a) for a in got_masks[:k]], reps)
            same = got_boxes[:k] == ref
            plain, boxed = (1e3 * float(np.median(t[k_])) / n for k_ in (False, True))
            print(json.dumps({"size": size, "batch": n, "masks_ms": round(plain, 3), "masks_boxes_ms": round(boxed, 3),
                              "boxes_cost_ms": round(boxed - plain, 3),
                              "host_tracer_ms": None if tracer_ms is None else round(tracer_ms / k, 2),
                              "host_filled_ms": round(filled_ms / k, 2), "same_boxes": bool(same)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only-contour", action="store_true")
    ap.add_argument("--contour", action="store_true",
                    help="the device contour section (profiles/contour_predict.txt) instead of the resize rows")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="sample,1080x1920,3000x4000")
    ap.add_argument("--batches", default="1,32")
    args = ap.parse_args()
    if args.only_contour:
        return contour_remainder(args.reps)
    if args.contour:
        return contour_section(args.reps, args.sizes.split(","), [int(b) for b in args.batches.split(",")])
    assert torch.cuda.is_available(), "bench_imageproc needs the MI355X"
    from PIL import Image
    rng = np.random.default_rng(5)
    model = UNetModel((H, W, 3), 1, dropout_rate=0.2, device="cuda:0")
    model.engine.graph_predict = True
    quant = model.freeze(dtype="int8", calibration=rng.random((8, H, W, 3), dtype=np.float32), batch_size=4)
    sources = {}
    for size in args.sizes.split(","):
        if size == "sample":
            sources["960x540"] = [np.asarray(Image.open(os.path.join(SAMPLES, n)).convert("RGB"))
                                  for n in ("brazil_passport.png", "chile_id_card.png")]
        else:
            h, w = (int(v) for v in size.split("x"))
            sources[size] = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8)]
    print(f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; reps {args.reps}; ms per image", flush=True)
    print("# model size batch | host: total pre predict post (reps) | device: total resize predict mask | "
          "host/device mask_GBps same", flush=True)
    for name, m in (("fp32", model), ("int8", quant)):
        for size, src in sources.items():
            for n in (int(b) for b in args.batches.split(",")):
                images = [src[i % len(src)] for i in range(n)]
                first = _clock(lambda: host_path(m, images[:1]))[0]        # warm-up (one image: the host
                host_path(m, images[:1])                                   # path has no per-batch state)
                for _ in range(3):
                    got = device_path(m, images)
                torch.cuda.synchronize()
                host_reps = args.reps if first * n < 5.0 else 1
                parts, th, td = [], [], []
                for r in range(args.reps):
                    if r < host_reps:
                        th.append(_clock(lambda: host_path(m, images, parts))[0])
                    td.append(_clock(lambda: device_path(m, images))[0])
                same = all(np.array_equal(a, b) for a, b in zip(host_path(m, images[:2]), got[:2]))
                t_res, t_prd, t_msk = device_parts(m, images, args.reps)
                pre, prd, post = (1e3 * float(np.median([p[k] for p in parts])) / n for k in range(3))
                host_ms, dev_ms = 1e3 * float(np.median(th)) / n, 1e3 * float(np.median(td)) / n
                mask_bytes = sum(a.shape[0] * a.shape[1] for a in images)
                rec = {"model": name, "size": size, "batch": n, "host_ms": round(host_ms, 3), "host_pre_ms": round(pre, 3),
                       "host_predict_ms": round(prd, 3), "host_post_ms": round(post, 3), "host_reps": host_reps,
                       "device_ms": round(dev_ms, 3), "resize_kernel_ms": round(t_res / n, 4),
                       "predict_kernel_ms": round(t_prd / n, 4), "mask_kernel_ms": round(t_msk / n, 4),
                       "host_over_device": round(host_ms / dev_ms, 2),
                       "mask_store_GBps": round(mask_bytes / (t_msk * 1e-3) / 1e9, 1), "same_masks": bool(same)}
                print(json.dumps(rec), flush=True)
    contour_remainder(args.reps)


if __name__ == "__main__":
    main()
