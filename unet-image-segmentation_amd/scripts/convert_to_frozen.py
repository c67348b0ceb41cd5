#!/usr/bin/env python3
"""Freeze trained weights into the engine's inference artefact: the counterpart of the reference's
scripts/tensorflow_lite/convert_to_tflite.py (same positionals and flags).

    python scripts/convert_to_frozen.py <input_model> <output> [--float16] [--optimize]
    python scripts/convert_to_frozen.py <input_model> <output> --int8 --calibration_data PATH

input_model is an engine weight file (.npz, Keras variable names: what scripts/train.py saves).
The output is one .npz holding the BatchNorm-folded network with fp16 matrix operands, which
scripts/inference.py and scripts/benchmark.py load directly through --model.  float16 is the
default format, so --float16 and --optimize are accepted and change nothing; that conversion runs
on the host and needs no GPU.

--int8 writes the int8 format instead (one-byte activations, int8 matrix operands).  It needs a
representative dataset, --calibration_data: a .npy of float32 images in [0, 1], (N, H, W, C), or a
directory of images (read with scripts/inference.py's preprocessing).  The network's activation
ranges on those images set the quantisation scales; that calibration run needs the GPU.
"""
import argparse
import os
import sys

PROJECT_ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.append(PROJECT_ROOT)

import numpy as np  # noqa: E402

from unet_amd import frozen  # noqa: E402


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Freeze a trained U-Net into a float16 (default) or int8 inference file.")
    p.add_argument("input_model", type=str, help="Trained weights (engine .npz, Keras variable names).")
    p.add_argument("output", type=str, help="Where to write the frozen model (.npz, written to this exact path).")
    p.add_argument("--optimize", action="store_true", help="Accepted for compatibility; the frozen format is float16.")
    p.add_argument("--float16", action="store_true", help="Accepted for compatibility; the frozen format is float16.")
    p.add_argument("--input_size", type=int, nargs=3, default=(256, 256, 3), metavar=("H", "W", "C"),
                   help="Input size the model was trained for (default: 256 256 3).")
    p.add_argument("--num_classes", type=int, default=1, help="Number of output classes (default: 1).")
    p.add_argument("--int8", action="store_true",
                   help="Write the int8 format. Needs --calibration_data and a GPU (MI355X) for the calibration run.")
    p.add_argument("--calibration_data", type=str, default=None, metavar="PATH",
                   help="Representative dataset for --int8: a .npy of float32 images in [0, 1], (N, H, W, C), "
                        "or a directory of images.")
    return p


def parse_args(argv=None) -> argparse.Namespace:
    return build_parser().parse_args(argv)


IMAGE_EXTENSIONS = (".png", ".jpg", ".jpeg", ".bmp", ".tif", ".tiff", ".webp")


def read_calibration(path, input_size):
    """The representative dataset as float32 (N, H, W, C) in [0, 1]."""
    h, w, c = (int(v) for v in input_size)
    if os.path.isdir(path):
        import inference
        files = sorted(f for f in os.listdir(path) if f.lower().endswith(IMAGE_EXTENSIONS))
        if not files:
            raise ValueError(f"no images in {path}")
        x = np.concatenate([inference.load_and_preprocess_image(os.path.join(path, f), h, w)[0] for f in files], 0)
    else:
        x = np.load(path, allow_pickle=False)
    x = np.asarray(x, np.float32)
    if x.ndim != 4 or x.shape[0] == 0 or tuple(x.shape[1:]) != (h, w, c):
        raise ValueError(f"calibration data must be (N, {h}, {w}, {c}), got {x.shape}")
    if not np.all(np.isfinite(x)) or x.min() < 0.0 or x.max() > 1.0:
        raise ValueError("calibration images must be finite and lie in [0, 1]")
    return x


def quantize(weights, use_bn, filters, args):
    """The int8 operands: ranges from the fp16 frozen network on the calibration images (GPU)."""
    x = read_calibration(args.calibration_data, args.input_size)
    half = frozen.FrozenUNet(frozen.fold_weights(weights, args.num_classes, use_bn, filters), args.input_size,
                             args.num_classes, filters)
    ranges = frozen.collect_ranges(half, x)
    return frozen.quantize_weights(frozen.fold_exact(weights, args.num_classes, use_bn, filters), ranges, filters)


def read_weights(path):
    with open(path, "rb") as f, np.load(f, allow_pickle=False) as z:
        return {k.replace(":", "/"): z[k] for k in z.files}


def geometry(weights):
    """(use_batch_norm, filters) as the variable names and shapes tell them."""
    use_bn = "enc1_block1_bn/gamma" in weights
    filters = []
    while f"enc{len(filters) + 1}_block1_sepconv/pointwise_kernel" in weights:
        filters.append(int(weights[f"enc{len(filters) + 1}_block1_sepconv/pointwise_kernel"].shape[-1]))
    if not filters:
        raise ValueError("no encoder blocks found: not a U-Net weight file")
    return use_bn, tuple(filters)


def main(argv=None) -> int:
    args = parse_args(argv)
    if not os.path.isfile(args.input_model):
        print(f"Error: input model not found -> {args.input_model}")
        return 1
    if frozen.is_frozen_file(args.input_model):
        print(f"Error: {args.input_model} is already a frozen model")
        return 1
    if args.int8:
        if not args.calibration_data:
            print("Error: --int8 needs a representative dataset: pass --calibration_data PATH "
                  "(a .npy of images in [0, 1] or a directory of images)")
            return 1
        if not os.path.exists(args.calibration_data):
            print(f"Error: calibration data not found -> {args.calibration_data}")
            return 1
        print("Frozen format: int8 (scales from the representative dataset)")
    else:
        print("Frozen format: float16 (the default" + ("; --optimize changes nothing)" if args.optimize else ")"))
    try:
        weights = read_weights(args.input_model)
        use_bn, filters = geometry(weights)
        if args.int8:
            folded = quantize(weights, use_bn, filters, args)
        else:
            folded = frozen.fold_weights(weights, args.num_classes, use_bn, filters)
    except (ValueError, RuntimeError) as e:
        print(f"Error: cannot freeze {args.input_model}: {e}")
        return 1
    out_dir = os.path.dirname(args.output)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    frozen.save_archive(args.output, frozen.to_archive(folded, args.input_size, args.num_classes, filters,
                                                       "int8" if args.int8 else "float16"))
    size = os.path.getsize(args.output)
    print(f"Wrote {args.output}: {len(folded)} arrays, {size / 1e6:.2f} MB "
          f"({'BatchNorm folded' if use_bn else 'no BatchNorm'}, filters {filters})")
    return 0


if __name__ == "__main__":
    sys.exit(main())
