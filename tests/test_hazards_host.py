"""tests/hazards.py without a device: the analyser on hand-built traces, the vector clocks against
brute-force reachability, the header parser against the binding table, and the recorder's promise
to leave what it patches exactly as it found it."""
import sys

import pytest
from hypothesis import HealthCheck, given, seed, settings
from hypothesis import strategies as st

import hazards as H
from hazards import find_hazards, ordering_edges, parse_header, reachability_hazards
from unet_amd import _lib

M, S, T = 0x10, 0x20, 0x30  # stream handles
BUF = (0x1000, 0x2000)


def launch(stream, reads=(), writes=(), name="k"):
    return {"kind": "launch", "name": name, "stream": stream,
            "reads": [(lo, hi, f"r{k}") for k, (lo, hi) in enumerate(reads)],
            "writes": [(lo, hi, f"w{k}") for k, (lo, hi) in enumerate(writes)]}


def wait_stream(waiter, producer):
    return {"kind": "wait_stream", "stream": waiter, "producer": producer}


def record(key, stream):
    return {"kind": "record", "event": key, "stream": stream}


def wait(key, stream):
    return {"kind": "wait", "event": key, "stream": stream}


def pairs(events, **kw):
    return [(h["a"], h["b"]) for h in find_hazards(events, **kw)]


def test_analyser_imports_no_torch():
    """(a fresh interpreter: this process has torch loaded already)"""
    import os
    import subprocess
    code = (f"import sys; sys.path.insert(0, {os.path.dirname(H.__file__)!r}); import hazards; "
            "hazards.find_hazards([]); hazards.parse_header(); assert 'torch' not in sys.modules")
    subprocess.run([sys.executable, "-c", code], check=True)


def test_same_stream_pairs_never_conflict():
    assert pairs([launch(M, writes=[BUF]), launch(M, reads=[BUF]), launch(M, writes=[BUF])]) == []


def test_read_read_pairs_never_conflict():
    assert pairs([launch(M, reads=[BUF]), launch(S, reads=[BUF])]) == []


def test_write_read_conflicts_without_an_edge_and_not_with_one():
    w, r = launch(M, writes=[BUF], name="producer"), launch(S, reads=[BUF], name="consumer")
    (h,) = find_hazards([w, r], names={(0x1000, 0x2000): "dz", (0x0, 0x10000): "arena"})
    assert (h["a"], h["b"], h["a_name"], h["b_name"], h["a_arg"], h["b_arg"]) == (0, 1, "producer", "consumer", "w0", "r0")
    assert (h["a_write"], h["b_write"], h["lo"], h["hi"], h["buffer"]) == (True, False, 0x1000, 0x2000, "dz")
    assert (h["a_stream"], h["b_stream"]) == (M, S)
    assert "producer(w0) W" in H.format_hazard(h) and "dz" in H.format_hazard(h)
    assert pairs([w, wait_stream(S, M), r]) == []
    assert pairs([w, wait_stream(M, S), r]) == [(0, 2)]  # the edge the other way round orders nothing
    assert pairs([r, w]) == [(0, 1)]  # read first, then overwritten: the same hazard
    assert pairs([launch(M, writes=[BUF]), launch(S, writes=[BUF])]) == [(0, 1)]


def test_ordering_is_transitive_over_three_streams():
    ev = [launch(M, writes=[BUF]), wait_stream(S, M), launch(S, writes=[(0x5000, 0x5100)]), wait_stream(T, S),
          launch(T, reads=[BUF])]
    assert pairs(ev) == []
    assert pairs(ev, drop=(1,)) == [(0, 4)]
    assert pairs(ev, drop=(3,)) == [(0, 4)]
    # ... also when the middle stream issues nothing between its wait and the next record
    assert pairs([launch(M, writes=[BUF]), wait_stream(S, M), wait_stream(T, S), launch(T, reads=[BUF])]) == []


def test_reused_event_handle_binds_each_wait_to_its_own_record():
    """record, wait, record again on one handle: the first wait covers the first record's prefix only."""
    a, b = (0x1000, 0x1100), (0x2000, 0x2100)
    ev = [launch(M, writes=[a]), record("e", M), wait("e", S), launch(M, writes=[b]), record("e", M),
          launch(S, reads=[a]), launch(S, reads=[b])]
    assert pairs(ev) == [(3, 6)]
    assert pairs(ev + [wait("e", S), launch(S, reads=[b])]) == [(3, 6)]  # the second wait sees the second record
    # unet_stream_wait_stream reuses its event in every call: each call is its own record + wait
    ev = [launch(M, writes=[a]), wait_stream(S, M), launch(M, writes=[b]), wait_stream(T, M), launch(S, reads=[b])]
    assert pairs(ev) == [(2, 4)]


def test_wait_before_the_write_does_not_order_it():
    assert pairs([wait_stream(S, M), launch(M, writes=[BUF]), launch(S, reads=[BUF])]) == [(1, 2)]
    assert pairs([record("e", M), launch(M, writes=[BUF]), wait("e", S), launch(S, reads=[BUF])]) == [(1, 3)]
    assert pairs([wait("never", S), launch(M, writes=[BUF]), launch(S, reads=[BUF])]) == [(1, 2)]


def test_overlap_is_by_bytes():
    flat = (0x1000, 0x3000)
    lo, hi = (0x1000, 0x2000), (0x2000, 0x3000)
    assert pairs([launch(M, writes=[lo]), launch(S, writes=[hi])]) == []  # disjoint slices of one buffer
    (h,) = find_hazards([launch(M, writes=[hi]), launch(S, reads=[flat])])  # a slice and its parent
    assert (h["lo"], h["hi"]) == hi
    assert pairs([launch(M, writes=[(0x1000, 0x2001)]), launch(S, reads=[hi])]) == [(0, 1)]  # one byte
    assert pairs([launch(M, writes=[(0x1000, 0x1000)]), launch(S, reads=[flat])]) == []  # empty range


def test_synchronize_joins():
    w, r = launch(M, writes=[BUF]), launch(S, reads=[BUF])
    assert pairs([w, {"kind": "sync", "stream": None}, r]) == []
    assert pairs([w, {"kind": "sync", "stream": M}, r]) == []
    assert pairs([w, {"kind": "sync", "stream": T}, r]) == [(0, 2)]  # another stream's: joins nothing of M
    assert pairs([w, record("e", M), {"kind": "sync_event", "event": "e"}, r]) == []
    assert pairs([record("e", M), w, {"kind": "sync_event", "event": "e"}, r]) == [(1, 3)]
    # the host's join holds for everything issued later, on every stream
    assert pairs([w, {"kind": "sync", "stream": None}, launch(T, reads=[BUF]), launch(S, writes=[BUF])]) == [(2, 3)]


def test_ordering_edges_names_waiter_and_producer():
    ev = [launch(M), wait_stream(S, M), record("e", S), wait("e", M), wait("unbound", T), wait_stream(M, M)]
    assert ordering_edges(ev) == [{"index": 1, "waiter": S, "producer": M}, {"index": 3, "waiter": M, "producer": S}]
    table = H.deletion_table([launch(M, writes=[BUF]), wait_stream(S, M), wait_stream(S, M), launch(S, reads=[BUF]),
                              launch(M, writes=[(0x9000, 0x9100)]), wait_stream(S, M), launch(S, reads=[(0x9000, 0x9100)])])
    assert [n for _, n in table] == [0, 0, 1]  # two redundant waits (each covers the other), one load-bearing


# ------------------------------------------------------------- vector clocks = reachability ---
STREAMS = [0x10, 0x20, 0x30, 0x40]
RANGES = [(0, 8), (4, 12), (8, 16), (16, 24), (0, 24)]


@st.composite
def traces(draw):
    n = draw(st.integers(1, 30))
    s = st.sampled_from(STREAMS)
    r = st.lists(st.sampled_from(RANGES), max_size=2)
    out = []
    for _ in range(n):
        kind = draw(st.sampled_from(["launch"] * 5 + ["wait_stream", "wait_stream", "record", "wait", "sync", "sync_event"]))
        if kind == "launch":
            out.append(launch(draw(s), draw(r), draw(r)))
        elif kind == "wait_stream":
            out.append(wait_stream(draw(s), draw(s)))
        elif kind in ("record", "wait"):
            out.append({"kind": kind, "event": draw(st.sampled_from(["e0", "e1"])), "stream": draw(s)})
        elif kind == "sync":
            out.append({"kind": "sync", "stream": draw(st.sampled_from(STREAMS + [None]))})
        else:
            out.append({"kind": "sync_event", "event": draw(st.sampled_from(["e0", "e1"]))})
    return out


@seed(2301)
@settings(max_examples=300, deadline=None, derandomize=True, database=None,
          suppress_health_check=[HealthCheck.too_slow])
@given(traces())
def test_vector_clocks_equal_brute_force_reachability(ev):
    assert {(h["a"], h["b"]) for h in find_hazards(ev)} == reachability_hazards(ev)


# --------------------------------------------------------------------- the header parser ---
def test_every_stream_entry_point_is_classified():
    protos = parse_header()
    kinds = {"read", "write", "view", "ws", "ws_bytes", "host", "stream", "event", "value"}
    for name, (_, argtypes) in _lib.SIGNATURES.items():
        args = protos[name]
        assert len(args) == len(argtypes), name
        assert {k for _, k in args} <= kinds, name
        if not any(k == "stream" for _, k in args):
            continue
        for (arg, kind), ct in zip(args, argtypes):
            pointer = ct is _lib.P or hasattr(ct, "contents")  # c_void_p or POINTER(struct)
            assert pointer == (kind in ("read", "write", "view", "ws", "host", "event", "stream")), (name, arg, kind)
            if hasattr(ct, "contents"):
                assert kind == "view", (name, arg)


def _rw(name):
    by = {}
    for arg, kind in parse_header()[name]:
        if kind not in ("value", "stream", "ws_bytes"):
            by.setdefault(kind, []).append(arg)
    return by


def test_classification_spelled_out():
    assert _rw("unet_pointwise_bwd_filter") == {"read": ["y", "dz"], "write": ["d_pw_kernel"], "ws": ["ws"]}
    assert _rw("unet_reduce_slabs") == {"write": ["slabs", "out"]}
    assert _rw("unet_dwconv3x3_bwd_data_bnstats_dwf") == {
        "view": ["x"], "read": ["dw_kernel", "dy", "mean", "rstd"], "write": ["dx0", "bn_partials", "dw_partials"]}
    assert _rw("unet_adamw_step") == {"write": ["param", "m", "v"], "read": ["grad"]}
    assert _rw("unet_meaniou_update") == {"read": ["y_true", "y_pred"], "write": ["confusion"]}
    assert _rw("unet_split_x3_mixed") == {"read": ["src"], "host": ["segs"], "write": ["dst"]}
    assert _rw("unet_dwconv3x3_bwd_data") == {"view": ["x"], "read": ["dw_kernel", "dy"], "write": ["dx0", "dx1"]}
    assert _rw("unet_batch_gather_u8") == {"read": ["src", "slots"], "write": ["dst"]}
    assert _rw("unet_stream_wait_stream") == {"event": ["event"]}
    assert [k for _, k in parse_header()["unet_stream_wait_stream"]] == ["stream", "stream", "event"]


# ----------------------------------------------------- the recorder on stand-in objects ---
class _Ptr:
    def __init__(self, value):
        self.value = value


class _Tensor:
    is_cuda = True

    def __init__(self, addr, n):
        self.addr, self.n = addr, n

    def data_ptr(self):
        return self.addr

    def numel(self):
        return self.n

    def element_size(self):
        return 4


def _stand_ins():
    import ctypes
    log = []

    class Ops:
        @staticmethod
        def _call(name, work, *args, route="main"):
            log.append(name)

        @staticmethod
        def _check(t, name, numel=None):
            pass

        @staticmethod
        def _check_dt(t, name, dtype, numel=None):
            pass

        @staticmethod
        def _ptr(t):
            return None if t is None else ctypes.c_void_p(t.data_ptr())

    class Lib:
        @staticmethod
        def call(name, *args):
            log.append(name)

    class StreamBase:
        def synchronize(self):
            log.append("sync")

    class Stream(StreamBase):  # (synchronize is inherited: it must not be left behind as a copy)
        def __init__(self, h):
            self.cuda_stream = h

        def wait_stream(self, other):
            self.wait_event(other.record_event())

        def wait_event(self, event):
            event.wait(self)

        def record_event(self, event=None):
            event = event or Event()
            event.record(self)
            return event

    class Event:
        def record(self, stream=None):
            log.append("record")

        def wait(self, stream=None):
            log.append("wait")

        def synchronize(self):
            log.append("esync")

    class Cuda:
        cur = Stream(M)

        @classmethod
        def current_stream(cls):
            return cls.cur

        @staticmethod
        def synchronize():
            log.append("dsync")

    return {"ops": Ops, "lib": Lib, "Stream": Stream, "Event": Event, "cuda": Cuda}, log


def _snapshot(t):
    return {(k, n): vars(o).get(n, "inherited") for k, o in t.items()
            for n in ("_call", "_check", "_check_dt", "_ptr", "call", "wait_stream", "wait_event", "record_event",
                      "synchronize", "record", "wait", "current_stream")}


HEADER_STANDIN = {"unet_k": [("x", "read"), ("n", "value"), ("out", "write"), ("ws", "ws"), ("ws_bytes", "ws_bytes"),
                             ("stream", "stream")],
                  "unet_stream_wait_stream": [("waiter", "stream"), ("producer", "stream"), ("event", "event")]}


def test_recorder_records_and_restores_on_stand_ins():
    t, log = _stand_ins()
    before = _snapshot(t)
    Ops, Lib, Stream, Event, Cuda = (t[k] for k in ("ops", "lib", "Stream", "Event", "cuda"))
    with H.record_accesses(targets=t) as rec:
        rec.protos = HEADER_STANDIN
        assert _snapshot(t) != before
        x, out, ws = _Tensor(0x1000, 64), _Tensor(0x2000, 16), _Tensor(0x9000, 1024)
        Ops._check(x, "x")
        Ops._call("unet_k", (0, 0), Ops._ptr(x), 3, Ops._ptr(out), Ops._ptr(ws), 100, _Ptr(M))
        Lib.call("unet_stream_wait_stream", _Ptr(S), _Ptr(M), _Ptr(0x77))
        side = Stream(S)
        side.wait_stream(Cuda.cur)  # one event, though it runs record_event + wait_event inside
        ev = Event()
        ev.record()
        side.wait_event(ev)
        ev.wait(side)
        ev.synchronize()
        side.synchronize()
        Cuda.synchronize()
        # a pointer at an offset inside a checked tensor: the rest of that tensor; into nothing: an error
        Ops._check(x, "x")
        Ops._call("unet_k", (0, 0), _Ptr(0x1010), 3, None, None, 0, None)
        with pytest.raises(H.UnresolvedPointer, match="unet_k: argument out = 0x5000"):
            Ops._call("unet_k", (0, 0), None, 3, _Ptr(0x5000), None, 0, None)
    assert _snapshot(t) == before
    ek = id(ev)
    assert rec.events == [
        {"kind": "launch", "name": "unet_k", "stream": M, "reads": [(0x1000, 0x1100, "x")],
         "writes": [(0x2000, 0x2040, "out"), (0x9000, 0x9064, "ws")]},
        {"kind": "wait_stream", "stream": S, "producer": M, "event": 0x77},
        {"kind": "wait_stream", "stream": S, "producer": M},
        {"kind": "record", "event": ek, "stream": M},
        {"kind": "wait", "event": ek, "stream": S},
        {"kind": "wait", "event": ek, "stream": S},
        {"kind": "sync_event", "event": ek},
        {"kind": "sync", "stream": S},
        {"kind": "sync", "stream": None},
        {"kind": "launch", "name": "unet_k", "stream": 0, "reads": [(0x1010, 0x1100, "x")], "writes": []},
    ]
    assert log.count("unet_k") == 2 and "record" in log and "dsync" in log  # the originals still ran


def test_recorder_restores_when_the_block_raises():
    t, _ = _stand_ins()
    before = _snapshot(t)
    with pytest.raises(KeyError):
        with H.record_accesses(targets=t):
            assert _snapshot(t) != before
            raise KeyError("boom")
    assert _snapshot(t) == before
    assert "synchronize" not in vars(t["Stream"])


def test_recorder_restores_the_real_modules():
    """The same on unet_amd.ops / _lib and torch's own classes (no device is touched)."""
    torch = pytest.importorskip("torch")
    from unet_amd import ops
    objs = {"ops": ops, "lib": _lib, "Stream": torch.cuda.Stream, "Event": torch.cuda.Event, "cuda": torch.cuda}
    before = _snapshot(objs)
    with pytest.raises(ZeroDivisionError):
        with H.record_accesses() as rec:
            assert ops._call is not before[("ops", "_call")] and _lib.call is not before[("lib", "call")]
            a = torch.zeros(4)
            a.add_(1)  # CPU tensors: ignored
            1 / 0
    assert _snapshot(objs) == before
    assert rec.events == []
