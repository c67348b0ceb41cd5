"""Records tests/golden/rows_bits.json, the byte fixture of tests/test_rows_bits_gpu.py: the sha256 of
every output buffer of the rows-GEMM cases listed there, from the library that UNET_HIP_LIB names (the
one to hold later libraries to; default: the in-tree build).  Every case runs twice and must give the
same bytes both times, or nothing is written.  Needs the GPU.

    UNET_HIP_LIB=/path/to/reference/libunet_hip.so python tools/record_rows_bits.py [OUT.json]
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "unet-image-segmentation_amd"), ROOT, os.path.join(ROOT, "tests")]

import test_rows_bits_gpu as T  # noqa: E402
from unet_amd import _lib, ops  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    rec = {}
    for cid, params in T.CASES.items():
        first, second = T.run_case(ops, cid), T.run_case(ops, cid)
        if first != second:
            print(f"{cid}: two runs differ in {sorted(k for k in first if first[k] != second[k])}")
            return 1
        rec[cid] = {"params": params, "sha256": first}
    lib = hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()
    with open(out, "w") as f:
        json.dump({"library_sha256": lib, "cases": rec}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(rec)} cases (each twice, equal) from library {lib[:12]} to {out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
