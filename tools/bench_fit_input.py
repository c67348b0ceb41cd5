"""What feeds model.fit: the host input path (PairLoader -> Prefetcher: uint8 -> fp32 on the host,
pinned copy, 16 bytes per pixel over PCIe) against the device-resident one (DevicePairLoader: uint8
cache on the device, one slot table up, two unet_batch_gather_u8 launches), both in ONE process,
alternating, median of RUNS timed runs after a warm-up.

    python tools/bench_fit_input.py [OUT.txt]        (default profiles/device_loader.txt)
    rocprofv3 --kernel-trace --stats ... -- python tools/bench_fit_input.py --gather-only
    python tools/bench_fit_input.py --augment [OUT.txt]   (default profiles/device_augment.txt)

--augment measures the random affine augmentation (unet_amd/augment.py) the same way: the warp kernel
unet_batch_affine_u8 beside the gather it replaces, the batches the augmented loaders deliver, and
model.fit with the augmented device loader against the unaugmented one of the same run.

The dataset is bench_loader.make_midv_tree (960x540 PNG frames and masks), resized to 256x256; after
the first epoch both loaders hold it decoded (host uint8 cache / device uint8 cache).  Sections:
  1  batches delivered to the device per second in cached epochs, the consumer only waiting on each
     batch's event (no step), batch 16 and 32; and the first, decode-bound epoch of each path;
  2  model.fit images/s at configs[1] (256x256x3, batch 16, dice loss, MeanIoU + dice_coef, dropout
     0.2) with each loader, against a train_step loop on one resident batch in the same process;
  3  the two gather launches in HIP-event time (a replayed graph of them) and their store rate;
  4  PCIe bytes per step of each path, computed from the shapes.
"""
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "unet-image-segmentation_amd"), ROOT, os.path.join(ROOT, "tools")]

SIZE = (256, 256)
N_TRAIN = 128
RUNS = 5
GRAPH_REPS = 100
SEED = 2301


def cpu_quota():
    q = f"{len(os.sched_getaffinity(0))} CPUs in the affinity mask of {os.cpu_count()}"
    for k in ("OMP_NUM_THREADS", "MAX_JOBS"):
        if os.environ.get(k):
            q += f", {k}={os.environ[k]}"
    try:
        q += ", cgroup cpu.max = " + open("/sys/fs/cgroup/cpu.max").read().strip()
    except OSError:
        pass
    return q


def gather_cases(frames, masks, dev):
    """(batch, c, cache, slot table, out) of the four launches a 256x256 step issues at batch 16 / 32,
    every other slot mirrored."""
    import torch
    for b in (16, 32):
        k = np.arange(b)
        entries = torch.from_numpy(np.where(k % 2, ~k, k).astype(np.int32)).to(dev)
        for src, c in ((frames, 3), (masks, 1)):
            yield b, c, src, entries, torch.empty((b,) + SIZE + (c,), dtype=torch.float32, device=dev)


def gather_section(say, med, frames, masks, dev):
    """Section 3.  A single launch between two events also times the events; back-to-back launches
    from Python are bounded by the host's call rate (~10 us), above the kernel's time.  So: GRAPH_REPS
    launches captured into one HIP graph (a linear chain), replayed between two events."""
    import torch
    from unet_amd import ops
    say(f"3. unet_batch_gather_u8 at 256x256: HIP-event time of a graph of {GRAPH_REPS} launches / {GRAPH_REPS}")
    for b, c, src, entries, out in gather_cases(frames, masks, dev):
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(3):
                ops.batch_gather_u8(src, entries, out)
        torch.cuda.current_stream(dev).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(GRAPH_REPS):
                ops.batch_gather_u8(src, entries, out)
        graph.replay()
        torch.cuda.synchronize()
        us = []
        for _ in range(RUNS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            graph.replay()
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / GRAPH_REPS)
        wr = 4.0 * out.numel()
        say(f"   batch {b:>2} c={c}: {med(us):6.2f} us per launch ({min(us):.2f}-{max(us):.2f}); stores {wr / 1e6:.1f} MB, "
            f"loads {out.numel() / 1e6:.1f} MB: {wr / med(us) / 1e3:.0f} GB/s stored, "
            f"{1.25 * wr / med(us) / 1e3:.0f} GB/s moved")
    say("   (the gap between two kernels of a graph is inside the figure; the source stays in L2 across the")
    say("    replays, the destination is rewritten; DESIGN 5's store calibration, 5.1-5.5 TB/s, is for buffers")
    say("    of hundreds of MB)")
    say()


def graph_launch_us(fn, dev):
    """HIP-event time of one launch of fn(), from a replayed graph of GRAPH_REPS of them: the RUNS samples."""
    import torch
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(GRAPH_REPS):
            fn()
    graph.replay()
    torch.cuda.synchronize()
    us = []
    for _ in range(RUNS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        graph.replay()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / GRAPH_REPS)
    return us


AUGMENT = dict(rotation_range=30, width_shift_range=0.2, height_shift_range=0.2, shear_range=15, zoom_range=(0.7, 1.3))
AUG_RUNS = 5        # alternating repeats of every --augment figure (the issue asks for at least three)
HOST_AUG_EPOCHS = 2  # the host warp is slow: fewer epochs per timed run than the 20 of the device paths


def augment_main(out_path):
    """`--augment`.  Sections:
      1  unet_batch_affine_u8 (order 1 and 0, both fill modes) and unet_batch_gather_u8 on the same cache and
         batch, HIP-event time per launch from a replayed graph, alternating within the run;
      2  images/s delivered in cached epochs by the augmented PairLoader, the augmented DevicePairLoader and
         the unaugmented DevicePairLoader, against a train_step loop on one resident batch;
      3  model.fit at configs[1] with the augmented and the unaugmented device loader, alternating."""
    import statistics as st
    import torch
    from bench_loader import make_midv_tree
    from unet_amd import ops
    from unet_amd.augment import Augment
    from unet_amd.data import PairLoader
    from unet_amd.device_data import DevicePairLoader
    from unet_amd.metrics import MeanIoU
    from unet_amd.model import UNetModel
    from unet_amd.optim import AdamW
    from unet_amd.prefetch import Prefetcher

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def flush():
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")

    def span(v, fmt="8.0f"):
        return f"{st.median(v):{fmt}}  ({min(v):.{fmt[-2]}f}-{max(v):.{fmt[-2]}f})"

    say("Random affine augmentation of model.fit's input (tools/bench_fit_input.py --augment)")
    say(f"device: {torch.cuda.get_device_name(dev)}; CPU quota: {cpu_quota()}; loader workers 16")
    say(f"augmentation: {AUGMENT}, fill_mode nearest, both orders 1, horizontal_flip; median (min-max) of "
        f"{AUG_RUNS} runs, the paths alternating")
    say()

    # ------------------------------------------------------------------ 1: kernel time ---
    say(f"1. one launch at 256x256, HIP-event time of a graph of {GRAPH_REPS} launches / {GRAPH_REPS}, us")
    say("   (random records of the ranges above, every other one flipped; the gather's slot table mirrors every other sample)")
    aug = Augment(**AUGMENT)
    frames = torch.randint(0, 256, (N_TRAIN,) + SIZE + (3,), dtype=torch.uint8, device=dev)
    masks = torch.randint(0, 256, (N_TRAIN,) + SIZE + (1,), dtype=torch.uint8, device=dev)
    for b, c, src, entries, out in gather_cases(frames, masks, dev):
        k = np.arange(b)
        recs = aug.records(aug.draw(np.random.default_rng(b), b), k, k % 2 == 1, SIZE)
        xf = torch.from_numpy(recs).to(dev)
        plain = torch.from_numpy(k.astype(np.int32)).to(dev)
        cases = {"gather": lambda: ops.batch_gather_u8(src, entries, out),
                 "affine order 1 nearest": lambda: ops.batch_affine_u8(src, plain, xf, out, 1, False, 0.0),
                 "affine order 1 constant": lambda: ops.batch_affine_u8(src, plain, xf, out, 1, True, 0.0),
                 "affine order 0 nearest": lambda: ops.batch_affine_u8(src, plain, xf, out, 0, False, 0.0)}
        wr = 4.0 * out.numel()
        for name, fn in cases.items():
            us = graph_launch_us(fn, dev)
            say(f"   batch {b:>2} c={c} {name:<24} {span(us, '6.2f')}   {wr / st.median(us) / 1e3:6.0f} GB/s stored")
    say("   the one-float-per-thread path (w % 4 != 0; the network itself admits w % 16 == 0 only), 256x254, batch 16:")
    odd = (SIZE[0], SIZE[1] - 2)
    k = np.arange(16)
    xf = torch.from_numpy(aug.records(aug.draw(np.random.default_rng(16), 16), k, k % 2 == 1, odd)).to(dev)
    plain = torch.from_numpy(k.astype(np.int32)).to(dev)
    mirrored = torch.from_numpy(np.where(k % 2, ~k, k).astype(np.int32)).to(dev)
    for c in (3, 1):
        src = torch.randint(0, 256, (N_TRAIN,) + odd + (c,), dtype=torch.uint8, device=dev)
        out = torch.empty((16,) + odd + (c,), dtype=torch.float32, device=dev)
        for name, fn in (("gather", lambda: ops.batch_gather_u8(src, mirrored, out)),
                         ("affine order 1 nearest", lambda: ops.batch_affine_u8(src, plain, xf, out, 1, False, 0.0))):
            us = graph_launch_us(fn, dev)
            say(f"   batch 16 c={c} {name:<24} {span(us, '6.2f')}   {4.0 * out.numel() / st.median(us) / 1e3:6.0f} GB/s stored")
    say("   (the gap between two kernels of a graph is inside every figure; source in L2, destination rewritten)")
    say()
    flush()

    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        base = make_midv_tree(d, N_TRAIN, 1)
        print(f"dataset written in {time.perf_counter() - t0:.1f} s", flush=True)
        fr, mk = os.path.join(base, "train_frames", "image"), os.path.join(base, "train_masks", "image")
        batch, per_epoch = 16, N_TRAIN // 16
        kw = dict(shuffle=True, horizontal_flip=True, workers=16)
        ld = {"host+aug": PairLoader(fr, mk, SIZE, batch, SEED, augment=Augment(**AUGMENT), **kw),
              "device+aug": DevicePairLoader(fr, mk, SIZE, batch, SEED, device=dev, augment=Augment(**AUGMENT), **kw),
              "device": DevicePairLoader(fr, mk, SIZE, batch, SEED, device=dev, **kw)}
        epochs_of = {"host+aug": HOST_AUG_EPOCHS, "device+aug": 20, "device": 20}

        def deliver(loader, nb):
            t = time.perf_counter()
            for _ in Prefetcher(loader, dev, limit=nb):
                pass
            torch.cuda.synchronize()
            return nb * batch / (time.perf_counter() - t)

        model = UNetModel(SIZE + (3,), 1, dropout_rate=0.2, device=dev)
        model.compile(AdamW(learning_rate=2e-3, weight_decay=1e-4), "dice_loss",
                      metrics=[MeanIoU(num_classes=2, name="mean_io_u", device=dev), "dice_coef"])
        for k in ld:  # first epoch (decode) + one cached epoch: caches, allocator, pinned areas, code objects
            deliver(ld[k], 2 * per_epoch)
        xb, yb = next(iter(Prefetcher(ld["device+aug"], dev, limit=1)))
        xb, yb = xb.clone(), yb.clone()
        epochs = 16

        def fit_rate(loader):
            t = time.perf_counter()
            model.fit(loader, epochs=epochs, steps_per_epoch=per_epoch, verbose=0)
            torch.cuda.synchronize()
            return epochs * per_epoch * batch / (time.perf_counter() - t)

        def step_rate():
            t = time.perf_counter()
            for _ in range(epochs * per_epoch):
                model.train_step(xb, yb)
            torch.cuda.synchronize()
            return epochs * per_epoch * batch / (time.perf_counter() - t)

        fit_rate(ld["device"])
        fit_rate(ld["device+aug"])
        step_rate()

        # ------------------------------------------------------------ 2: delivery rate ---
        rates = {k: [] for k in ld}
        steps = []
        for _ in range(AUG_RUNS):
            for k in ld:
                rates[k].append(deliver(ld[k], epochs_of[k] * per_epoch))
            steps.append(step_rate())
        say(f"2. batches delivered to the device in cached epochs, images/s (batch {batch}, no train step; consumer waits "
            f"on the batch's event)")
        for k in ld:
            say(f"   {k:<11} {span(rates[k])}   {st.median(rates[k]) / st.median(steps):5.2f} x the step rate   "
                f"({epochs_of[k]} epochs per run)")
        say(f"   train_step loop on one resident batch (what consumes them)  {span(steps)}")
        slow = st.median(rates["host+aug"]) < st.median(steps)
        say(f"   the host loader with augmentation delivers {'LESS' if slow else 'more'} than the step consumes"
            f"{': a fit fed by it waits for its input' if slow else ''}")
        say()
        flush()

        # ---------------------------------------------------------------------- 3: fit ---
        fits = {"device": [], "device+aug": [], "step": []}
        for _ in range(AUG_RUNS):
            fits["device"].append(fit_rate(ld["device"]))
            fits["device+aug"].append(fit_rate(ld["device+aug"]))
            fits["step"].append(step_rate())
        say(f"3. model.fit at configs[1] (batch 16, {epochs} epochs x {per_epoch} steps per run, cached epochs), images/s")
        for k, label in (("device", "fit, device loader"), ("device+aug", "fit, augmented device loader")):
            say(f"   {label:<30} {span(fits[k])}   {100 * st.median(fits[k]) / st.median(fits['step']):.1f} % of step-only")
        say(f"   {'train_step loop (the ceiling)':<30} {span(fits['step'])}")
        spread = max(fits["device"]) - min(fits["device"])
        cost = st.median(fits["device"]) - st.median(fits["device+aug"])
        say(f"   augmentation costs the fit {cost:+.0f} images/s (median - median); run-to-run spread of the unaugmented "
            f"fit {spread:.0f} images/s (max - min of {AUG_RUNS}): {'within' if cost <= spread else 'LARGER than'} the spread")
        say()
    flush()


def gather_only():
    """`--gather-only`: 50 launches of each of the four cases and nothing else, to be run under
    rocprofv3 --kernel-trace for the kernels' own durations."""
    import torch
    from unet_amd import ops
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    frames = torch.randint(0, 256, (N_TRAIN,) + SIZE + (3,), dtype=torch.uint8, device=dev)
    masks = torch.randint(0, 256, (N_TRAIN,) + SIZE + (1,), dtype=torch.uint8, device=dev)
    for b, c, src, entries, out in gather_cases(frames, masks, dev):
        for _ in range(50):
            ops.batch_gather_u8(src, entries, out)
        torch.cuda.synchronize()


def main():
    import torch
    from bench_loader import make_midv_tree
    from unet_amd.data import PairLoader
    from unet_amd.device_data import DevicePairLoader
    from unet_amd.metrics import MeanIoU
    from unet_amd.model import UNetModel
    from unet_amd.optim import AdamW
    from unet_amd.prefetch import Prefetcher

    if not torch.cuda.is_available():
        raise SystemExit("bench_fit_input.py needs the GPU: nothing here can be measured without it")
    if "--gather-only" in sys.argv[1:]:
        return gather_only()
    if "--augment" in sys.argv[1:]:
        rest = [a for a in sys.argv[1:] if a != "--augment"]
        return augment_main(rest[0] if rest else os.path.join(ROOT, "profiles", "device_augment.txt"))
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "device_loader.txt")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def med(v):
        return statistics.median(v)

    def span(v):
        return f"{med(v):8.0f}  ({min(v):.0f}-{max(v):.0f})"

    say("Input path of model.fit: host loader vs device-resident loader (tools/bench_fit_input.py)")
    say(f"device: {torch.cuda.get_device_name(dev)}; CPU quota: {cpu_quota()}; loader workers 16")
    say(f"dataset: make_midv_tree, {N_TRAIN} pairs of 960x540 PNG -> {SIZE[0]}x{SIZE[1]}; "
        f"median (min-max) of {RUNS} runs, the two paths alternating")
    say()
    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        base = make_midv_tree(d, N_TRAIN, 1)
        print(f"dataset written in {time.perf_counter() - t0:.1f} s", flush=True)
        fr, mk = os.path.join(base, "train_frames", "image"), os.path.join(base, "train_masks", "image")

        def loaders(batch):
            kw = dict(shuffle=True, horizontal_flip=True, workers=16)
            return {"host": PairLoader(fr, mk, SIZE, batch, SEED, **kw),
                    "device": DevicePairLoader(fr, mk, SIZE, batch, SEED, device=dev, **kw)}

        def deliver(loader, nb, batch):
            """nb batches through a fresh Prefetcher pass; the consumer waits on each event only."""
            t = time.perf_counter()
            for _ in Prefetcher(loader, dev, limit=nb):
                pass
            torch.cuda.synchronize()
            return nb * batch / (time.perf_counter() - t)

        # ---------------------------------------------------------------- 1: delivery rate ---
        say("1. batches delivered to the device, images/s (no train step; consumer waits on the batch's event)")
        say("   first epoch = PNG decode + resize on the host in both paths (decode-bound, not what the cache changes)")
        say(f"   {'batch':>5} {'path':>7} {'first epoch':>12} {'cached epochs: median (min-max)':>34}")
        for batch in (16, 32):
            ld = loaders(batch)
            per_epoch = N_TRAIN // batch
            first = {k: deliver(ld[k], per_epoch, batch) for k in ("host", "device")}
            for k in ld:
                deliver(ld[k], 2 * per_epoch, batch)  # warm-up: allocator, pinned areas, code objects
            rates = {"host": [], "device": []}
            for _ in range(RUNS):
                for k in ("host", "device"):
                    rates[k].append(deliver(ld[k], 20 * per_epoch, batch))
            for k in ("host", "device"):
                say(f"   {batch:>5} {k:>7} {first[k]:>12.0f} {span(rates[k]):>34}")
            if batch == 16:
                keep = ld
        say()

        # ------------------------------------------------------------------------ 2: fit ---
        model = UNetModel(SIZE + (3,), 1, dropout_rate=0.2, device=dev)
        model.compile(AdamW(learning_rate=2e-3, weight_decay=1e-4), "dice_loss",
                      metrics=[MeanIoU(num_classes=2, name="mean_io_u", device=dev), "dice_coef"])
        batch, per_epoch, epochs = 16, N_TRAIN // 16, 8
        xb, yb = next(iter(Prefetcher(keep["device"], dev, limit=1)))
        xb, yb = xb.clone(), yb.clone()

        def fit_rate(loader):
            t = time.perf_counter()
            model.fit(loader, epochs=epochs, steps_per_epoch=per_epoch, verbose=0)
            torch.cuda.synchronize()
            return epochs * per_epoch * batch / (time.perf_counter() - t)

        def step_rate():
            t = time.perf_counter()
            for _ in range(epochs * per_epoch):
                model.train_step(xb, yb)
            torch.cuda.synchronize()
            return epochs * per_epoch * batch / (time.perf_counter() - t)

        for k in keep:
            fit_rate(keep[k])
        step_rate()
        rates = {"host": [], "device": [], "step": []}
        for _ in range(RUNS):
            rates["host"].append(fit_rate(keep["host"]))
            rates["device"].append(fit_rate(keep["device"]))
            rates["step"].append(step_rate())
        say(f"2. model.fit at configs[1] (batch 16, {epochs} epochs x {per_epoch} steps per run, cached epochs), images/s")
        say(f"   fit, host loader       {span(rates['host'])}   {100 * med(rates['host']) / med(rates['step']):.1f} % of step-only")
        say(f"   fit, device loader     {span(rates['device'])}   {100 * med(rates['device']) / med(rates['step']):.1f} % of step-only")
        say(f"   train_step loop on one resident batch (the ceiling)  {span(rates['step'])}")
        say("   (fit also reads the epoch's logs back once per epoch; the step loop does not)")
        say()

        # ------------------------------------------------------------- 3: gather launches ---
        store = keep["device"].store
        gather_section(say, med, store.frames, store.masks, dev)

    # ------------------------------------------------------------------- 4: PCIe bytes ---
    say("4. PCIe bytes per step, computed from the shapes (256x256, frames + masks)")
    for b in (16, 32):
        px = b * SIZE[0] * SIZE[1]
        say(f"   batch {b:>2}: host path {16 * px / 1e6:.1f} MB of fp32 every step; device path {4 * b} B (the slot "
            f"table) once a sample is resident, {4 * px / 1e6:.1f} MB of uint8 + the table the first time")
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
