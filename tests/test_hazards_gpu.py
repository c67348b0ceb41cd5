"""Every cross-stream buffer hazard of a step, checked from its recorded trace (tests/hazards.py).

Each case records, inside one block, a warm-up step and then TWO consecutive steps (so the second
forward is checked against the first step's side-stream tail and AdamW), and asserts that no pair
of accesses on different streams to overlapping bytes, one of them a write, is left unordered by
the waits of the trace.  Nothing depends on timing, so the smallest shapes do (helpers.TRACE_CONFIGS).

That the check can fail is shown on the recorded trace alone -- ordering events are deleted from the
list and the analysis repeated; what runs on the device is never changed.

Out of scope (see hazards.py): the Prefetcher's producer thread (a dispatch mode is per thread; the
loader case iterates DevicePairLoader in the test's own thread and follows the consumer protocol by
hand), HIP-graph replay (its launches are invisible to the recorder), allocator reuse of freed
blocks, the internal streams of collectives.  Frozen, image-pipeline and contour entry points run
on one stream and have no case; test_recorder_takes_the_single_stream_entry_points only shows that
the recorder resolves their arguments.

UNET_HAZARD_REPORT=<file>: every case appends what it checked (profiles/launch_hazards.txt is such a file)."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import hazards as H  # noqa: E402
from helpers import TRACE_BATCH, TRACE_CONFIGS, batch, trace_model  # noqa: E402

pytestmark = pytest.mark.gpu

CFG_A = TRACE_CONFIGS["A"]


# ------------------------------------------------------------------------------ plumbing ---
def _labels(model, **extra):
    eng = model.engine
    out = {eng.main.cuda_stream: "main", eng.side.cuda_stream: "side",
           torch.cuda.default_stream(eng.device).cuda_stream: "caller"}
    out.update(extra)
    return out


def record_steps(model, steps):
    """Runs steps[0] (warm-up) and the others inside one recording; returns (the recorder, the events
    after the warm-up, the index in them at which each later step starts)."""
    starts = []
    with H.record_accesses(model.engine) as rec:
        steps[0]()
        first = len(rec.events)
        for s in steps[1:]:
            starts.append(len(rec.events) - first)
            s()
    torch.cuda.synchronize()
    return rec, rec.events[first:], starts


def report(case, events, an, hazards, labels, table=None, notes=()):
    path = os.environ.get("UNET_HAZARD_REPORT")
    if not path:
        return
    s = H.summarize(events, labels)
    lines = [f"== {case}",
             f"   launches per stream   {s['launches']}",
             f"   torch ops per stream  {s['torch_ops']}",
             f"   ordering edges        {s['edges']}",
             f"   conflicting pairs examined (overlap, two streams, a write)  {len(an.pairs)}",
             f"   hazards               {len(hazards)}"]
    lines += [f"      {H.format_hazard(h)}" for h in hazards[:20]]
    lines += [f"   {n}" for n in notes]
    if table is not None:
        lines.append("   single-edge deletion: hazards that appear when that wait alone is removed (0 = redundant);")
        lines.append("   equal rows are counted, with the trace index of the first")
        rows = {}
        for ed, n in table:
            nxt = next((x["name"] for x in events[ed["index"] + 1:] if x["kind"] in H.ACCESS
                        and x["stream"] == ed["waiter"]), "-")
            key = (f"{labels.get(ed['waiter'], hex(ed['waiter'])):>6s} waits for "
                   f"{labels.get(ed['producer'], hex(ed['producer'])):<6s} before its {nxt:<30s} hazards {n}")
            rows.setdefault(key, []).append(ed["index"])
        lines += [f"      {len(ix):3d} x {key}   (first #{ix[0]})" for key, ix in rows.items()]
        lines.append(f"   load-bearing edges: {sum(n > 0 for _, n in table)} of {len(table)}")
    with open(path, "a") as f:
        f.write("\n".join(lines) + "\n")


def check_clean(case, model, rec, events, labels=None, table=False, notes=()):
    labels = labels or _labels(model)
    an = H.Analysis(events, rec.names())
    hz = an.hazards()
    report(case, events, an, hz, labels, H.deletion_table(events) if table else None, notes)
    assert not hz, "\n".join(H.format_hazard(h) for h in hz[:12])
    return an


def side_launches(model, events):
    side = model.engine.side.cuda_stream
    return [e["name"] for e in events if e["kind"] == "launch" and e["stream"] == side]


def train_steps(model, rng, cfg, batches=(TRACE_BATCH,) * 3):
    data = [batch(rng, n, cfg) for n in batches]
    torch.cuda.synchronize()
    return [lambda x=x, y=y: model.train_step(x, y) for x, y in data], data


# ------------------------------------------------------------------ every TRACE_CONFIGS id ---
@pytest.mark.parametrize("cid", sorted(TRACE_CONFIGS))
def test_trace_config_has_no_hazard(cid):
    cfg = TRACE_CONFIGS[cid]
    model = trace_model(cfg)
    rng = np.random.default_rng(7)
    if cid == "P":
        x, _ = batch(rng, TRACE_BATCH, cfg)
        torch.cuda.synchronize()
        steps = [lambda: model.engine.predict(x)] * 3
    else:
        steps, _ = train_steps(model, rng, cfg)
    rec, events, _ = record_steps(model, steps)
    assert sum(e["kind"] == "launch" for e in events) > 40
    on_side = side_launches(model, events)
    if cid in ("B", "P"):  # single stream: trivially clean, and it must be single stream
        assert on_side == []
    else:
        assert on_side, "an overlapped train step with nothing on the side stream"
    check_clean(f"TRACE_CONFIGS[{cid}]  {cfg}", model, rec, events)


# ------------------------------------------- the routes that put most on the side stream ---
def _meaniou_model(cfg=CFG_A):
    from unet_amd.metrics import MeanIoU
    return trace_model(cfg, metrics=[MeanIoU(2, threshold=0.5)])


SIDE_CASES = {
    "meaniou": (CFG_A, None, "unet_meaniou_update"),
    "defer_sw": (CFG_A, {"fuse_block_bwd": False, "defer_sw": True}, "unet_sepconv_bwd_filter"),
    "no_defer_sw": (CFG_A, {"fuse_block_bwd": False, "defer_sw": False}, "unet_sepconv_bwd_filter"),
    "classes21": (((64, 64, 3), 21, True, 0.2, {}), None, "unet_conv_transpose2x2_bwd"),
    "no_batch_norm": (((64, 64, 3), 1, False, 0.2, {}), None, "unet_conv_transpose2x2_bwd"),
    "batch_2_then_3": (CFG_A, None, "unet_conv_transpose2x2_bwd"),
    "test_step_and_predict_between": (CFG_A, None, "unet_meaniou_update"),
    # the benchmark's two workloads at their own sizes: the routes of a step depend on the level sizes and
    # the batch (fusion thresholds, y recomputation, tile choices), and the hazards on the routes
    "bench_256_b16": (((256, 256, 3), 1, True, 0.2, {}), None, "unet_meaniou_update"),
    "bench_256_classes21_b8": (((256, 256, 3), 21, True, 0.2, {}), None, "unet_conv_transpose2x2_bwd"),
}
SIDE_BATCHES = {"batch_2_then_3": (2, 2, 3), "bench_256_b16": (16,) * 3, "bench_256_classes21_b8": (8,) * 3}


@pytest.mark.parametrize("case", sorted(SIDE_CASES))
def test_side_stream_route_has_no_hazard(case):
    cfg, attrs, must_be_on_side = SIDE_CASES[case]
    rng = np.random.default_rng(11)
    if must_be_on_side == "unet_meaniou_update":
        model = _meaniou_model(cfg)
    else:
        model = trace_model(cfg, attrs=attrs)
    steps, data = train_steps(model, rng, cfg, SIDE_BATCHES.get(case, (TRACE_BATCH,) * 3))
    if case == "test_step_and_predict_between":  # on the caller's stream, between the two train steps
        (x, y) = data[0]
        steps = [steps[0], steps[1], lambda: model.test_step(x, y), lambda: model.predict(x), steps[2]]
    rec, events, _ = record_steps(model, steps)
    assert must_be_on_side in side_launches(model, events)
    if case == "test_step_and_predict_between":
        caller = torch.cuda.default_stream(model.engine.device).cuda_stream
        assert sum(e["kind"] == "launch" and e["stream"] == caller for e in events) > 60
    check_clean(f"side-stream route: {case}", model, rec, events)


# ------------------------------------------------------------------------- gradient hook ---
@pytest.mark.parametrize("defer_sw", [True, False], ids=["defer_sw", "no_defer_sw"])
def test_gradient_hook_sees_final_gradients(defer_sw):
    """A pseudo-launch stands in for the bucketed all-reduce: issued on the stream the hook is called
    on, reading and writing grads[off:].  No hazard; and what _grads_ready promises: no launch issued
    after hook(off) in the same step writes a byte of grads[off:], on any stream, ordered or not."""
    model = trace_model(CFG_A, attrs={"fuse_block_bwd": False, "defer_sw": defer_sw})
    eng = model.engine
    hooks = []  # (index in rec.events, offset)
    holder = {}

    def hook(off):
        g = eng.grads[off:]
        hooks.append((holder["rec"].pseudo_launch("grad_hook", reads=[(g, "grads[off:]")], writes=[(g, "grads[off:]")]),
                      off))

    eng.grad_hook = hook
    steps, _ = train_steps(model, np.random.default_rng(13), CFG_A)
    starts = []
    with H.record_accesses(eng) as rec:
        holder["rec"] = rec
        for s in steps:
            starts.append(len(rec.events))
            s()
    torch.cuda.synchronize()
    first = starts[1]
    events = rec.events[first:]
    side = eng.side.cuda_stream
    assert all(rec.events[i]["stream"] == side for i, _ in hooks), "the hook is issued from the side stream"
    assert "unet_sepconv_bwd_filter" in side_launches(model, events)
    glo, ghi = H.Recorder.tensor_range(eng.grads)
    bounds = starts + [len(rec.events)]
    for k in range(len(steps)):
        mine = [(i, off) for i, off in hooks if bounds[k] <= i < bounds[k + 1]]
        assert len(mine) > 10 and min(off for _, off in mine) == 0, "the reports must cover the whole flat buffer"
        for i, off in mine:
            late = [(j, e["name"], a) for j, e in enumerate(rec.events[i + 1:bounds[k + 1]], i + 1)
                    if e["kind"] in H.ACCESS and e["name"] != "grad_hook"
                    for lo, hi, a in e["writes"] if hi > glo + 4 * off and lo < ghi]
            assert not late, f"step {k}: written after hook({off}) at #{i}: {late[:4]}"
    an = check_clean(f"gradient hook, defer_sw={defer_sw}", model, rec, events, table=True,
                     notes=[f"hook reports per step {len(hooks) // len(steps)}, offsets "
                            f"{sorted({off for _, off in hooks}, reverse=True)[:4]} ... 0"])
    _deletions_make_hazards(model, events, an)


# --------------------------------------------------------------------------- device loader ---
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """12 PNG pairs of 32 x 32, as test_device_loader_gpu.py writes them."""
    from PIL import Image
    root = str(tmp_path_factory.mktemp("pairs"))
    fr, mk = os.path.join(root, "frames"), os.path.join(root, "masks")
    os.makedirs(fr)
    os.makedirs(mk)
    rng = np.random.default_rng(0)
    for i in range(12):
        Image.fromarray(rng.integers(0, 256, (32, 32, 3), dtype=np.uint8)).save(os.path.join(fr, f"f{i:03d}.png"))
        m = np.zeros((32, 32), np.uint8)
        m[5:5 + i % 7 + 3, 4:20] = 255
        Image.fromarray(m).save(os.path.join(mk, f"f{i:03d}.png"))
    return fr, mk


def test_device_loader_feeding_train_steps_has_no_hazard(tree):
    """DevicePairLoader iterated in this thread (no Prefetcher), consumer protocol by hand, three
    train steps after a warm-up one; 3 resident slots of 12 samples, so every batch rewrites the
    4 transient slots the batch before it was gathered from."""
    from unet_amd.device_data import DevicePairLoader
    size, bs = (32, 32), 4
    loader = DevicePairLoader(*tree, size, bs, seed=2301, shuffle=True, horizontal_flip=True, workers=1,
                              device="cuda:0", device_cache_bytes=3 * size[0] * size[1] * 4)
    assert (loader.book.resident, loader.book.transient) == (3, 4)
    model = trace_model((size + (3,), 1, True, 0.0, {}))
    it = iter(loader)
    keep = []  # (a batch freed here could hand its block to the loader's next torch.empty: allocator reuse is out of scope)

    def step():
        shard = next(it)
        cur = torch.cuda.current_stream(model.engine.device)
        cur.wait_event(shard.event)
        shard[0].record_stream(cur)
        shard[1].record_stream(cur)
        keep.append(shard)
        model.train_step(shard[0], shard[1])

    rec, events, _ = record_steps(model, [step] * 4)
    ls = loader.store.stream.cuda_stream
    labels = _labels(model)
    labels[ls] = "loader"
    on_loader = [e for e in events if e["kind"] in H.ACCESS and e["stream"] == ls]
    names = [e["name"] for e in on_loader]
    assert names.count("unet_batch_gather_u8") == 6 and names.count("aten::copy_") >= 3 * 3
    slot3 = loader.store.frames.data_ptr() + loader.book.resident * loader.store.fbytes  # the first transient slot
    rewrites = sum(e["name"] == "aten::copy_" and any(lo == slot3 for lo, _, _ in e["writes"]) for e in on_loader)
    assert rewrites >= 2, "the transient slots must be rewritten inside the recorded steps"
    an = check_clean("device loader feeding three train steps", model, rec, events, labels, table=True)
    # the consumer's wait on the shard's event is what orders the gathers before the step's reads of x / y
    waits = [ed["index"] for ed in H.ordering_edges(events) if ed["producer"] == ls]
    assert len(waits) == 3
    hz = an.hazards(drop=waits)
    assert any("unet_batch_gather_u8" in (h["a_name"], h["b_name"]) for h in hz)


# ------------------------------------------------- the check can fail (on the trace only) ---
def _deletions_make_hazards(model, events, an):
    eng = model.engine
    main, side = eng.main.cuda_stream, eng.side.cuda_stream
    edges = H.ordering_edges(events)
    side_waits = [ed["index"] for ed in edges if (ed["waiter"], ed["producer"]) == (side, main)]
    main_waits = [ed["index"] for ed in edges if (ed["waiter"], ed["producer"]) == (main, side)]
    assert len(side_waits) > 10 and len(main_waits) == 2  # (one main-waits-for-side per step)
    assert an.hazards() == []
    assert an.hazards(drop=side_waits), "without any side-waits-for-main edge the trace must show hazards"
    glo, ghi = H.Recorder.tensor_range(eng.grads)
    hz = an.hazards(drop=main_waits[-1:])
    adamw = [h for h in hz for me, other in (("a", "b"), ("b", "a"))
             if h[me + "_name"] == "unet_adamw_step" and h[me + "_arg"] == "grad"
             and h[other + "_stream"] == side and h[other + "_write"] and glo <= h["lo"] and h["hi"] <= ghi]
    assert adamw, "without the final main-waits-for-side edge AdamW must race a side-stream weight-gradient write"
    assert any(n > 0 for _, n in H.deletion_table(events)), "no single ordering edge is load-bearing?"


@pytest.mark.parametrize("case", ["A", "meaniou"])
def test_deleting_waits_from_the_trace_yields_hazards(case):
    model = trace_model(CFG_A) if case == "A" else _meaniou_model()
    steps, _ = train_steps(model, np.random.default_rng(17), CFG_A)
    rec, events, _ = record_steps(model, steps)
    an = check_clean(f"deletions: {case}", model, rec, events, table=True)
    _deletions_make_hazards(model, events, an)
    if case == "meaniou":  # the metric's reads of prob are ordered by the run_beside wait alone
        upd = [i for i, e in enumerate(events) if e.get("name") == "unet_meaniou_update"]
        before = [ed["index"] for ed in H.ordering_edges(events) if ed["index"] < upd[0]
                  and ed["waiter"] == model.engine.side.cuda_stream]
        hz = an.hazards(drop=before[-1:])
        assert any("unet_meaniou_update" in (h["a_name"], h["b_name"]) for h in hz)


# ----------------------------------------------------- single-stream entry points resolve ---
def test_recorder_takes_the_single_stream_entry_points():
    """Frozen inference and the image pipeline: no hazard case (one stream), but every pointer of
    their launches must resolve (an offset destination, fp16 views, workspaces)."""
    model = trace_model(((64, 64, 3), 1, True, 0.0, {}))
    rng = np.random.default_rng(19)
    x, _ = batch(rng, 2, ((64, 64, 3), 1))
    frozen = model.freeze("float16")
    imgs = [rng.integers(0, 256, (40, 56, 3), dtype=np.uint8), rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)]
    with H.record_accesses(model.engine) as rec:
        frozen.predict(x)
        model.predict_masks(imgs, return_boxes=True)
    torch.cuda.synchronize()
    names = {e["name"] for e in rec.events if e["kind"] == "launch"}
    assert {"unet_f16_sepconv", "unet_image_resize_u8", "unet_mask_resize", "unet_mask_largest_contour"} <= names
    assert H.find_hazards(rec.events) == []


@pytest.mark.parametrize("outer", ["record_launches", "record_accesses"])
def test_recorder_works_beside_record_launches(outer):
    """Both recorders around the same steps, nested either way: the same launches on the same streams,
    and ops._call / L.call are the originals again afterwards."""
    import contextlib

    from helpers import record_launches
    from unet_amd import _lib, ops
    model = trace_model(CFG_A)
    steps, _ = train_steps(model, np.random.default_rng(23), CFG_A, (2, 2))
    before = (ops._call, ops._check, ops._check_dt, ops._ptr, _lib.call, ops.WORKSPACE)
    with contextlib.ExitStack() as stack:
        if outer == "record_launches":
            rl = stack.enter_context(record_launches(model.engine))
            rec = stack.enter_context(H.record_accesses(model.engine))
        else:
            rec = stack.enter_context(H.record_accesses(model.engine))
            rl = stack.enter_context(record_launches(model.engine))
        for s in steps:
            s()
    torch.cuda.synchronize()
    assert (ops._call, ops._check, ops._check_dt, ops._ptr, _lib.call, ops.WORKSPACE) == before
    side = model.engine.side.cuda_stream
    mine = [(e["name"], int(e["stream"] == side)) for e in rec.events if e["kind"] == "launch"]
    assert mine == [(t[0], t[1]) for t in rl.trace] and len(mine) > 200
    assert H.find_hazards(rec.events) == []
