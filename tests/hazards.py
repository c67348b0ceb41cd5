"""Cross-stream buffer hazards of a step, proved from its trace instead of hoped for from its timing.

The engine issues a train step on two HIP streams (engine.main, engine.side); DevicePairLoader and the
data-parallel hook add more.  Its results are right only if
  (1) no main-stream launch overwrites what a side-stream launch still reads, and
  (2) nothing touches the weight gradients before their last writer has been joined.
At test sizes every kernel has finished long before the next is issued, so a missing wait computes
the same bits.  This module does not run anything differently: it RECORDS, for every launch of the
block, its stream and the device byte ranges it reads and writes, and every ordering edge between
streams, and then PROVES on the host that every conflicting pair of accesses is ordered.

  parse_header()      include/unet_hip.h -> entry point -> [(argument, kind)]; the header is
                      const-correct, so `const T*` is a read and `T*` a write (no hand-kept table).
  record_accesses()   context manager (beside helpers.record_launches, not instead of it): launch
                      events through ops._call, ordering events through L.call and torch's Stream /
                      Event methods, torch-op events through a TorchDispatchMode.
  find_hazards()      pure Python (this module imports torch only inside the recorder): vector
                      clocks, one component per stream; every pair of accesses on different streams
                      whose byte ranges overlap, one of them a write, neither before the other.

A plain helper module like fenced.py: no conftest, no plugin, no pytest setting.

What the check does NOT cover:
  * the Prefetcher's producer thread: a dispatch mode and this recorder are per thread; the GPU
    tests iterate DevicePairLoader in their own thread and follow the consumer protocol by hand;
  * HIP-graph replay (engine.graph_predict): the launches inside a replayed graph go through
    neither ops._call nor the dispatcher;
  * the caching allocator handing a freed block to another stream (an address seen twice is taken
    for the same buffer; the tests keep their batches alive so that none is);
  * the internal streams of collectives (torch.distributed): the hook tests stand a pseudo-launch
    in for the all-reduce, on the stream the hook is called on.

Event records (dicts, so that a hand-built trace is a literal):
  {"kind": "launch" | "op", "name", "stream", "reads": [(lo, hi, arg)], "writes": [(lo, hi, arg)]}
  {"kind": "wait_stream", "stream": waiter, "producer"}     record on producer + wait, in one call
  {"kind": "record", "event": key, "stream"}                a later record of the same key rebinds it
  {"kind": "wait", "event": key, "stream": waiter}          ... for LATER waits only
  {"kind": "sync", "stream": handle or None}                host waits for one stream / for all
  {"kind": "sync_event", "event": key}                      host waits for what the event recorded
"""
from __future__ import annotations

import contextlib
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "unet_hip.h")

ACCESS = ("launch", "op")
HOST_ARRAYS = ("segs",)  # `const int64_t* segs`: read by the host side of the call, never by a kernel
VIEW_TYPES = ("unet_view", "unet_f16_view", "unet_i8_view")


# ------------------------------------------------------------------------------ the header ---
def parse_header(path=HEADER):
    """entry point -> [(argument name, kind)] for every prototype of the header, in argument order.
    kind: "read" (const T*), "write" (T*: plain and accumulating outputs alike), "view" (a const
    view struct: each non-null source pointer is a read), "ws" (void* followed by size_t ws_bytes:
    a write of ws_bytes bytes) and "ws_bytes", "host" (an array the host reads), "stream",
    "event" (the ordering handle), "value" (anything passed by value)."""
    with open(path) as f:
        txt = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    out = {}
    for name, params in re.findall(r"\b(unet_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", txt):
        plist = [" ".join(p.split()) for p in params.split(",")]
        if plist == ["void"] or plist == [""]:
            out[name] = []
            continue
        parsed = []
        for p in plist:
            m = re.match(r"^(.*?)(\w+)$", p)
            if m is None:
                raise ValueError(f"{name}: cannot parse parameter {p!r}")
            parsed.append((m.group(1).strip(), m.group(2)))
        args = []
        for i, (typ, arg) in enumerate(parsed):
            base = typ.replace("const", "").replace("*", "").strip()
            if "*" not in typ:
                if base == "unet_stream_t":
                    kind = "stream"
                elif base == "size_t" and i and args[-1][1] == "ws":
                    kind = "ws_bytes"
                else:
                    kind = "value"
            elif arg == "event":
                kind = "event"
            elif arg in HOST_ARRAYS:
                kind = "host"
            elif base in VIEW_TYPES:
                if not typ.startswith("const"):
                    raise ValueError(f"{name}: view argument {arg} is not const")
                kind = "view"
            elif base == "void" and i + 1 < len(parsed) and parsed[i + 1][0] == "size_t":
                kind = "ws"
            elif typ.startswith("const"):
                kind = "read"
            else:
                kind = "write"
            args.append((arg, kind))
        out[name] = args
    return out


# ------------------------------------------------------------------------------ the analyser ---
def _overlap_pairs(events):
    """[(i, j, arg_i, arg_j, lo, hi, write_i, write_j)], i < j: accesses of two events on different streams whose byte
    ranges overlap, at least one of them a write (a sweep over the ranges sorted by their start)."""
    ivs = []
    for i, e in enumerate(events):
        if e["kind"] not in ACCESS:
            continue
        for w, key in ((False, "reads"), (True, "writes")):
            for lo, hi, arg in e.get(key, ()):
                if hi > lo:
                    ivs.append((lo, hi, i, w, arg))
    ivs.sort(key=lambda t: (t[0], t[1], t[2]))
    active, seen, out = [], set(), []
    for lo, hi, i, w, arg in ivs:
        active = [a for a in active if a[1] > lo]
        for alo, ahi, j, aw, aarg in active:
            if i == j or not (w or aw) or events[i]["stream"] == events[j]["stream"]:
                continue
            a, b = ((j, aarg, aw), (i, arg, w)) if j < i else ((i, arg, w), (j, aarg, aw))
            key = (a[0], b[0], a[1], b[1], a[2], b[2])
            if key not in seen:
                seen.add(key)
                out.append((a[0], b[0], a[1], b[1], max(lo, alo), min(hi, ahi), a[2], b[2]))
        active.append((lo, hi, i, w, arg))
    out.sort()
    return out


def _clocks(events, drop=()):
    """index -> vector clock (tuple, one component per stream) of every access event.  Each stream's
    events are totally ordered; a wait joins the waiter with the producer's clock AT RECORD TIME; a
    synchronize joins the host with what it names, and everything issued later starts from the
    host's clock.  drop: indices of ordering events to leave out."""
    streams = []
    for e in events:
        for k in ("stream", "producer"):
            s = e.get(k)
            if s is not None and s not in streams:
                streams.append(s)
    idx = {s: k for k, s in enumerate(streams)}
    n = len(streams)
    clock = {s: [0] * n for s in streams}
    host = [0] * n
    recorded = {}
    stamps = {}

    def join(a, b):
        for k in range(n):
            if b[k] > a[k]:
                a[k] = b[k]

    for i, e in enumerate(events):
        kind = e["kind"]
        if i in drop:
            continue
        if kind in ACCESS:
            c = clock[e["stream"]]
            join(c, host)
            c[idx[e["stream"]]] += 1
            stamps[i] = tuple(c)
        elif kind == "wait_stream":
            join(clock[e["producer"]], host)  # (the record is issued by the host now)
            join(clock[e["stream"]], clock[e["producer"]])
        elif kind == "record":
            join(clock[e["stream"]], host)
            recorded[e["event"]] = list(clock[e["stream"]])
        elif kind == "wait":
            if e["event"] in recorded:
                join(clock[e["stream"]], recorded[e["event"]])
        elif kind == "sync":
            for s in (streams if e.get("stream") is None else [e["stream"]]):
                join(host, clock[s])
        elif kind == "sync_event":
            if e["event"] in recorded:
                join(host, recorded[e["event"]])
        else:
            raise ValueError(f"event {i}: unknown kind {kind!r}")
    return stamps, idx


def ordering_edges(events):
    """[{"index", "waiter", "producer"}] of every cross-stream wait of the trace (a wait on an event
    names the stream of the record it binds to; one that binds to nothing is left out)."""
    out, recorded = [], {}
    for i, e in enumerate(events):
        if e["kind"] == "record":
            recorded[e["event"]] = e["stream"]
        elif e["kind"] == "wait_stream":
            out.append({"index": i, "waiter": e["stream"], "producer": e["producer"]})
        elif e["kind"] == "wait" and e["event"] in recorded:
            out.append({"index": i, "waiter": e["stream"], "producer": recorded[e["event"]]})
    return [d for d in out if d["waiter"] != d["producer"]]


def _label(names, lo, hi):
    best = None
    for (nlo, nhi), nm in (names or {}).items():
        if nlo <= lo and hi <= nhi and (best is None or nhi - nlo < best[0]):
            best = (nhi - nlo, nm)
    return best[1] if best else None


class Analysis:
    """The conflicting pairs of a trace, found once; hazards(drop) re-orders them under the trace
    with some ordering events left out (the deletion tests ask that many times)."""

    def __init__(self, events, names=None):
        self.events, self.names = events, names
        self.pairs = _overlap_pairs(events)

    def hazards(self, drop=()):
        stamps, idx = _clocks(self.events, frozenset(drop))
        ev, out = self.events, []
        for i, j, ai, aj, lo, hi, wi, wj in self.pairs:
            si, sj = idx[ev[i]["stream"]], idx[ev[j]["stream"]]
            if stamps[i][si] <= stamps[j][si] or stamps[j][sj] <= stamps[i][sj]:
                continue
            out.append({"a": i, "b": j, "a_name": ev[i]["name"], "b_name": ev[j]["name"], "a_arg": ai, "b_arg": aj,
                        "a_stream": ev[i]["stream"], "b_stream": ev[j]["stream"],
                        "a_write": wi, "b_write": wj,
                        "lo": lo, "hi": hi, "buffer": _label(self.names, lo, hi)})
        return out


def find_hazards(events, names=None, drop=()):
    """Every unordered conflicting pair of the trace: [{"a", "b" (trace indices, a < b), "a_name",
    "b_name" (entry points), "a_arg", "b_arg" (the header's argument names), "a_stream", "b_stream",
    "a_write", "b_write", "lo", "hi" (the overlapping bytes), "buffer" (its name in `names`, a
    {(lo, hi): name} map, or None)}].  Empty: the trace is race-free whatever the timing."""
    return Analysis(events, names).hazards(drop)


def format_hazard(h):
    rw = lambda w: "W" if w else "R"  # noqa: E731
    return (f"#{h['a']} {h['a_name']}({h['a_arg']}) {rw(h['a_write'])} on stream {h['a_stream']:#x}  <->  "
            f"#{h['b']} {h['b_name']}({h['b_arg']}) {rw(h['b_write'])} on stream {h['b_stream']:#x}: "
            f"bytes [{h['lo']:#x}, {h['hi']:#x}) of {h['buffer'] or '?'}")


def reachability_hazards(events):
    """find_hazards' pairs {(a, b)} by brute force: a graph over the access events (program order per
    stream, one edge per wait from the producer's last access at record time to every later access
    of the waiter, host joins likewise) and a depth-first search per pair.  The host tests hold the
    vector clocks to it."""
    acc = [i for i, e in enumerate(events) if e["kind"] in ACCESS]
    succ = {i: set() for i in acc}
    last = {}          # stream -> its last access so far
    pending = {}       # stream -> accesses that must precede its NEXT access (edges not yet attached)
    recorded = {}      # event key -> the producer's last access at record time (or None)
    host = set()       # accesses the host has joined: they precede everything issued from now on
    streams = {e.get("stream") for e in events} | {e.get("producer") for e in events}
    streams.discard(None)
    for i, e in enumerate(events):
        kind = e["kind"]
        if kind in ACCESS:
            s = e["stream"]
            for p in pending.pop(s, set()) | host:
                succ[p].add(i)
            if s in last:
                succ[last[s]].add(i)
            last[s] = i
        elif kind == "wait_stream":
            if e["producer"] in last:
                pending.setdefault(e["stream"], set()).add(last[e["producer"]])
            # what the producer itself still waits for precedes the waiter too
            pending.setdefault(e["stream"], set()).update(pending.get(e["producer"], set()))
        elif kind == "record":
            recorded[e["event"]] = ({last[e["stream"]]} if e["stream"] in last else set()) | set(
                pending.get(e["stream"], set()))
        elif kind == "wait":
            pending.setdefault(e["stream"], set()).update(recorded.get(e["event"], set()))
        elif kind == "sync":
            for s in (streams if e.get("stream") is None else [e["stream"]]):
                if s in last:
                    host.add(last[s])
                host.update(pending.get(s, set()))
        elif kind == "sync_event":
            host.update(recorded.get(e["event"], set()))

    def reaches(a, b):
        stack, seen = [a], {a}
        while stack:
            for nx in succ[stack.pop()]:
                if nx == b:
                    return True
                if nx not in seen and nx < b:
                    seen.add(nx)
                    stack.append(nx)
        return False

    return {(i, j) for i, j, *_ in _overlap_pairs(events) if not reaches(i, j)}


# ------------------------------------------------------------------------------ the recorder ---
class UnresolvedPointer(RuntimeError):
    pass


class _Patches:
    """setattr with memory: undo() puts every attribute back exactly as it was found."""

    def __init__(self):
        self._saved = []

    def set(self, obj, name, value):
        own = name in vars(obj)  # (an inherited attribute is deleted again, not copied down)
        self._saved.append((obj, name, own, vars(obj)[name] if own else None))
        setattr(obj, name, value)

    def undo(self):
        while self._saved:
            obj, name, own, old = self._saved.pop()
            if own:
                setattr(obj, name, old)
            else:
                delattr(obj, name)


class Recorder:
    """What record_accesses yields: .events (the trace, in issue order) and helpers for the tests."""

    def __init__(self, engine=None, header=None):
        self.engine = engine
        self.events = []
        self.protos = header if header is not None else parse_header()
        self._pending = {}   # address -> bytes, tensors the running wrapper has checked since the last launch
        self._known = {}     # the same of earlier launches (a pointer that only they explain)
        self._keep = []      # event objects whose id() keys the trace: kept alive, so no id is reused
        self._depth = 0      # > 0 inside a patched torch method (wait_stream calls record_event + wait_event)

    # -- tensors -----------------------------------------------------------------------------
    def _note(self, t):
        try:
            if t is not None and t.is_cuda and t.numel():
                self._pending[t.data_ptr()] = max(self._pending.get(t.data_ptr(), 0), t.numel() * t.element_size())
        except AttributeError:
            pass  # (not a tensor: the wrapper's own check raises the TypeError)

    def _resolve(self, addr, name, arg):
        for table in (self._pending, self._known):
            nb = table.get(addr)
            if nb:
                return addr, addr + nb
            for lo, nb in table.items():  # inside a checked tensor: the rest of that tensor
                if lo < addr < lo + nb:
                    return addr, lo + nb
        raise UnresolvedPointer(f"{name}: argument {arg} = {addr:#x} lies in no tensor the wrapper was handed")

    @staticmethod
    def tensor_range(t):
        """[lo, hi) of the tensor's own elements (not of its storage)."""
        if t.numel() == 0:
            return None
        span = 1 + sum((s - 1) * st for s, st in zip(t.shape, t.stride()))
        return t.data_ptr(), t.data_ptr() + span * t.element_size()

    # -- launches ----------------------------------------------------------------------------
    def _launch(self, name, args):
        proto = self.protos.get(name)
        if proto is None:
            raise UnresolvedPointer(f"{name}: no prototype in the header")
        if len(proto) != len(args):
            raise UnresolvedPointer(f"{name}: {len(args)} arguments for {len(proto)} parameters")
        reads, writes, stream = [], [], 0
        for k, ((arg, kind), a) in enumerate(zip(proto, args)):
            if kind == "stream":
                stream = _addr(a)
            elif kind in ("read", "write"):
                addr = _addr(a)
                if not addr:
                    continue
                nb = getattr(a, "nbytes", None)
                lo, hi = (addr, addr + nb) if nb else self._resolve(addr, name, arg)
                (reads if kind == "read" else writes).append((lo, hi, arg))
            elif kind == "view":
                v = getattr(a, "_obj", None)
                if v is None:
                    raise UnresolvedPointer(f"{name}: argument {arg} is not a byref() of a view struct")
                for fname, ftype in v._fields_:
                    if ftype is ctypes.c_void_p and getattr(v, fname):
                        lo, hi = self._resolve(getattr(v, fname), name, f"{arg}.{fname}")
                        reads.append((lo, hi, f"{arg}.{fname}"))
            elif kind == "ws":
                addr = _addr(a)
                if addr:
                    writes.append((addr, addr + int(args[k + 1]), arg))
            elif kind == "host" and not (a is None or isinstance(a, ctypes.Array)):
                raise UnresolvedPointer(f"{name}: host array {arg} is {type(a).__name__}")
        self.events.append({"kind": "launch", "name": name, "stream": stream, "reads": reads, "writes": writes})
        self._known.update(self._pending)
        self._pending = {}

    def pseudo_launch(self, name, reads=(), writes=(), stream=None):
        """A stand-in launch on the current stream (or `stream`, a handle): reads / writes are
        [(tensor, argument name)].  What an all-reduce issued from a gradient hook could touch."""
        import torch
        if stream is None:
            stream = torch.cuda.current_stream().cuda_stream
        rng = lambda ts: [self.tensor_range(t) + (a,) for t, a in ts if t.numel()]  # noqa: E731
        self.events.append({"kind": "launch", "name": name, "stream": stream, "reads": rng(reads), "writes": rng(writes)})
        return len(self.events) - 1

    # -- torch ops ---------------------------------------------------------------------------
    def _torch_op(self, func, args, kwargs, out):
        import torch
        schema = func._schema
        if any(r.alias_info is not None and not r.alias_info.is_write for r in schema.returns):
            return  # a view: no byte is touched
        name = schema.name
        if name in ("aten::record_stream",):
            return  # allocator bookkeeping
        reads, writes = [], []

        def visit(v, written, arg):
            if isinstance(v, torch.Tensor):
                if v.is_cuda:
                    r = self.tensor_range(v)
                    if r is not None:
                        (writes if written else reads).append(r + (arg,))
            elif isinstance(v, (list, tuple)):
                for u in v:
                    visit(u, written, arg)

        for k, sa in enumerate(schema.arguments):
            v = args[k] if k < len(args) else kwargs.get(sa.name)
            visit(v, sa.alias_info is not None and sa.alias_info.is_write, sa.name)
        outs = out if isinstance(out, (list, tuple)) else (out,)
        for k, (r, v) in enumerate(zip(schema.returns, outs)):
            if r.alias_info is None:
                visit(v, True, f"out{k}")
        if reads or writes:
            self.events.append({"kind": "op", "name": name, "stream": torch.cuda.current_stream().cuda_stream,
                                "reads": reads, "writes": writes})

    # -- what the tests ask of a trace -------------------------------------------------------
    def names(self, *extra):
        """{(lo, hi): name} of the engine's flat buffers, variables, gradients and activation
        buffers (every Acts / BlockBufs attribute), plus extra (name, tensor) pairs."""
        out = {}

        def put(name, t):
            r = None if t is None or not hasattr(t, "data_ptr") or not t.is_cuda else self.tensor_range(t)
            if r is not None:
                out.setdefault(r, name)

        eng = self.engine
        if eng is not None:
            for k, v in eng.gvars.items():
                put(f"grads[{k}]", v)
            for k, v in eng.vars.items():
                put(f"vars[{k}]", v)
            for k in ("params", "grads", "stats", "x3buf"):
                put(k, getattr(eng, k, None))
            for n, A in eng._acts.items():
                for k, v in vars(A).items():
                    if isinstance(v, dict):
                        for kk, vv in v.items():
                            if hasattr(vv, "__dict__") and not hasattr(vv, "data_ptr"):
                                for k3, v3 in vars(vv).items():
                                    put(f"acts({n}).{k}[{kk}].{k3}", v3)
                            else:
                                put(f"acts({n}).{k}[{kk}]", vv)
                    else:
                        put(f"acts({n}).{k}", v)
        for name, t in extra:
            put(name, t)
        return out


def _addr(a):
    if a is None:
        return 0
    if isinstance(a, int):
        return a
    return a.value or 0


class _TrackedPtr(ctypes.c_void_p):
    """ops._ptr's c_void_p that remembers the bytes of the tensor it points into."""
    nbytes = 0


@contextlib.contextmanager
def record_accesses(engine=None, targets=None):
    """Collects the launch, ordering and torch-op events of the issuing thread while the block runs
    (Recorder.events).  targets (the host tests' stand-ins): {"ops", "lib", "Stream", "Event",
    "cuda", "dispatch"}; by default unet_amd.ops, unet_amd._lib, torch.cuda.Stream, torch.cuda.Event,
    torch.cuda and a TorchDispatchMode.  Everything patched is put back as it was found, also when
    the block raises."""
    rec = Recorder(engine)
    if targets is None:
        import torch
        from torch.utils._python_dispatch import TorchDispatchMode
        from unet_amd import _lib, ops

        class _Mode(TorchDispatchMode):
            def __torch_dispatch__(self, func, types, args=(), kwargs=None):
                out = func(*args, **(kwargs or {}))
                rec._torch_op(func, args, kwargs or {}, out)
                return out

        targets = {"ops": ops, "lib": _lib, "Stream": torch.cuda.Stream, "Event": torch.cuda.Event,
                   "cuda": torch.cuda, "dispatch": _Mode()}
    ops, lib, Stream, Event, cuda = (targets.get(k) for k in ("ops", "lib", "Stream", "Event", "cuda"))
    P = _Patches()

    def current():
        return cuda.current_stream().cuda_stream

    def outermost(fn):
        """Record only the outermost patched torch call: Stream.wait_stream is record_event + wait_event."""
        def wrapped(*a, **kw):
            top = rec._depth == 0
            rec._depth += 1
            try:
                return fn(top, *a, **kw)
            finally:
                rec._depth -= 1
        return wrapped

    def key(ev):
        rec._keep.append(ev)
        return id(ev)

    try:
        if ops is not None:
            o_call, o_check, o_check_dt, o_ptr = ops._call, ops._check, ops._check_dt, ops._ptr

            def call(name, work, *args, **kw):
                rec._launch(name, args)
                return o_call(name, work, *args, **kw)

            def check(t, *a, **kw):
                o_check(t, *a, **kw)
                rec._note(t)

            def check_dt(t, *a, **kw):
                o_check_dt(t, *a, **kw)
                rec._note(t)

            def ptr(t):
                p = o_ptr(t)
                if p is None:
                    return None
                rec._note(t)
                q = _TrackedPtr(p.value)
                q.nbytes = t.numel() * t.element_size()
                return q

            for name, fn in (("_call", call), ("_check", check), ("_check_dt", check_dt), ("_ptr", ptr)):
                P.set(ops, name, fn)
        if lib is not None:
            o_lcall = lib.call

            def lcall(name, *args):
                if name == "unet_stream_wait_stream":
                    rec.events.append({"kind": "wait_stream", "stream": _addr(args[0]), "producer": _addr(args[1]),
                                       "event": _addr(args[2])})
                return o_lcall(name, *args)

            P.set(lib, "call", lcall)
        if Stream is not None:
            o_ws, o_we, o_ss, o_re = Stream.wait_stream, Stream.wait_event, Stream.synchronize, Stream.record_event

            @outermost
            def wait_stream(top, self, other):
                if top:
                    rec.events.append({"kind": "wait_stream", "stream": self.cuda_stream, "producer": other.cuda_stream})
                return o_ws(self, other)

            @outermost
            def wait_event(top, self, event):
                if top:
                    rec.events.append({"kind": "wait", "event": key(event), "stream": self.cuda_stream})
                return o_we(self, event)

            @outermost
            def stream_sync(top, self):
                if top:
                    rec.events.append({"kind": "sync", "stream": self.cuda_stream})
                return o_ss(self)

            @outermost
            def record_event(top, self, event=None):
                out = o_re(self, event)
                if top:
                    rec.events.append({"kind": "record", "event": key(out), "stream": self.cuda_stream})
                return out

            for name, fn in (("wait_stream", wait_stream), ("wait_event", wait_event), ("synchronize", stream_sync),
                             ("record_event", record_event)):
                P.set(Stream, name, fn)
        if Event is not None:
            o_er, o_ew, o_es = Event.record, Event.wait, Event.synchronize

            @outermost
            def ev_record(top, self, stream=None):
                if top:
                    rec.events.append({"kind": "record", "event": key(self),
                                       "stream": current() if stream is None else stream.cuda_stream})
                return o_er(self) if stream is None else o_er(self, stream)

            @outermost
            def ev_wait(top, self, stream=None):
                if top:
                    rec.events.append({"kind": "wait", "event": key(self),
                                       "stream": current() if stream is None else stream.cuda_stream})
                return o_ew(self) if stream is None else o_ew(self, stream)

            @outermost
            def ev_sync(top, self):
                if top:
                    rec.events.append({"kind": "sync_event", "event": key(self)})
                return o_es(self)

            for name, fn in (("record", ev_record), ("wait", ev_wait), ("synchronize", ev_sync)):
                P.set(Event, name, fn)
        if cuda is not None:
            o_cs = cuda.synchronize

            @outermost
            def dev_sync(top, *a, **kw):
                if top:
                    rec.events.append({"kind": "sync", "stream": None})
                return o_cs(*a, **kw)

            P.set(cuda, "synchronize", dev_sync)
        mode = targets.get("dispatch")
        if mode is None:
            yield rec
        else:
            with mode:
                yield rec
    finally:
        P.undo()


# ------------------------------------------------------------------------------ reports ---
def summarize(events, streams=None):
    """{"launches": {stream label: count}, "torch_ops": {...}, "edges": count} of a trace; streams:
    {handle: label}."""
    lab = lambda s: (streams or {}).get(s, f"{s:#x}")  # noqa: E731
    out = {"launches": {}, "torch_ops": {}, "edges": len(ordering_edges(events))}
    for e in events:
        if e["kind"] in ACCESS:
            d = out["launches" if e["kind"] == "launch" else "torch_ops"]
            d[lab(e["stream"])] = d.get(lab(e["stream"]), 0) + 1
    return out


def deletion_table(events, names=None):
    """[(edge, hazards that appear when that ordering edge alone is deleted)] for every edge of the
    trace: an edge with 0 is redundant (another path orders everything it orders)."""
    an = Analysis(events, names)
    return [(ed, len(an.hazards(drop=(ed["index"],)))) for ed in ordering_edges(events)]
