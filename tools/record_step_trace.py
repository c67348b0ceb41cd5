"""Write tests/golden/step_traces.json: the kernel-launch trace of one train step (entry point, stream,
arguments) for every configuration of tests/helpers.py TRACE_CONFIGS, as tests/test_step_trace_gpu.py
replays and compares them.  Run it at the commit whose schedule is the reference and name that commit:

    python tools/record_step_trace.py --commit <hash> [--out FILE]

It drives the engine through its public attributes and the recorder only, so it runs at any commit."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "unet-image-segmentation_amd"), ROOT, os.path.join(ROOT, "tests")]

from helpers import TRACE_BATCH, TRACE_CONFIGS, step_trace  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="hash of the commit being recorded")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "step_traces.json"))
    args = ap.parse_args()
    traces = {}
    for cid in TRACE_CONFIGS:
        traces[cid] = step_trace(cid)
        print(f"{cid}: {len(traces[cid])} launches, {sum(e[1] for e in traces[cid])} on the side stream", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"recorded_at_commit": args.commit, "batch": TRACE_BATCH, "traces": traces}, f,
                  separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
