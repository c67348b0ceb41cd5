#!/usr/bin/env python3
"""Freeze trained weights into the engine's half-precision inference artefact: the counterpart of
the reference's scripts/tensorflow_lite/convert_to_tflite.py (same positionals and flags).

    python scripts/convert_to_frozen.py <input_model> <output> [--float16] [--optimize]

input_model is an engine weight file (.npz, Keras variable names: what scripts/train.py saves).
The output is one .npz holding the BatchNorm-folded network with fp16 matrix operands, which
scripts/inference.py and scripts/benchmark.py load directly through --model.  float16 is the only
frozen format, so --float16 and --optimize are accepted and change nothing.  The conversion runs
on the host; no GPU is needed.
"""
import argparse
import os
import sys

PROJECT_ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.append(PROJECT_ROOT)

import numpy as np  # noqa: E402

from unet_amd import frozen  # noqa: E402


def parse_args(argv=None) -> argparse.Namespace:
    p = argparse.ArgumentParser(description="Freeze a trained U-Net into a float16 inference file.")
    p.add_argument("input_model", type=str, help="Trained weights (engine .npz, Keras variable names).")
    p.add_argument("output", type=str, help="Where to write the frozen model (.npz, written to this exact path).")
    p.add_argument("--optimize", action="store_true", help="Accepted for compatibility; the frozen format is float16.")
    p.add_argument("--float16", action="store_true", help="Accepted for compatibility; the frozen format is float16.")
    p.add_argument("--input_size", type=int, nargs=3, default=(256, 256, 3), metavar=("H", "W", "C"),
                   help="Input size the model was trained for (default: 256 256 3).")
    p.add_argument("--num_classes", type=int, default=1, help="Number of output classes (default: 1).")
    return p.parse_args(argv)


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
    print("Frozen format: float16 (the only one" + ("; --optimize changes nothing)" if args.optimize else ")"))
    try:
        weights = read_weights(args.input_model)
        use_bn, filters = geometry(weights)
        folded = frozen.fold_weights(weights, args.num_classes, use_bn, filters)
    except ValueError as e:
        print(f"Error: cannot freeze {args.input_model}: {e}")
        return 1
    out_dir = os.path.dirname(args.output)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    frozen.save_archive(args.output, frozen.to_archive(folded, args.input_size, args.num_classes, filters))
    size = os.path.getsize(args.output)
    print(f"Wrote {args.output}: {len(folded)} arrays, {size / 1e6:.2f} MB "
          f"({'BatchNorm folded' if use_bn else 'no BatchNorm'}, filters {filters})")
    return 0


if __name__ == "__main__":
    sys.exit(main())
