"""Guard-band allocator for the op tests: every tensor is its own allocation of
fence + body + fence bytes, fences and fresh outputs hold 0xFF bytes (NaN as fp32 / fp64 / fp16 /
bf16 bit patterns, -1 as integers), and Arena.check() fails when a fence byte changed (a store
past either end of a buffer) or when a tensor named as an output still holds a poison element
(an element the kernel never wrote).  Input fences are NaN on purpose: a read past the end that
reaches a result fails the oracle comparison.  A masked over-read that never reaches a result is
invisible to fences.

A plain helper module (no conftest, no plugin).  Works on "cpu" tensors too, which is how
test_fenced_host.py proves that the harness sees an overrun without running a GPU kernel."""
from __future__ import annotations

import contextlib

import numpy as np
import torch

POISON = 0xFF
OUT_FENCE = 256 * 1024  # one whole 128-row tile of 512 fp32 channels: the largest single-tile stray
IN_FENCE = 4 * 1024
ALIGN = 256             # bodies keep the alignment torch's device allocations have

_INT_OF_SIZE = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _np_dtype(dtype):
    return torch.empty(0, dtype=dtype).numpy().dtype


class _Buf:
    __slots__ = ("label", "raw", "start", "nbytes", "view", "output", "fence")

    def __init__(self, label, raw, start, nbytes, view, output, fence):
        self.label, self.raw, self.start, self.nbytes, self.view, self.output = label, raw, start, nbytes, view, output
        self.fence = fence

    def sides(self):
        return (("front", self.raw[:self.start]), ("rear", self.raw[self.start + self.nbytes:]))

    def elements(self):
        """The body as same-width integers: a poison element is -1 (0xFF for bytes)."""
        it = _INT_OF_SIZE[self.view.element_size()]
        return self.raw[self.start:self.start + self.nbytes].view(it)

    def poison_value(self):
        return POISON if self.view.element_size() == 1 else -1


class Arena:
    """Fenced tensors on one device ("cuda" or "cpu"), checked together by check()."""

    def __init__(self, device="cuda", out_fence=OUT_FENCE, in_fence=IN_FENCE):
        assert out_fence % ALIGN == 0 and in_fence % ALIGN == 0
        self.device = torch.device(device)
        self.out_fence, self.in_fence = out_fence, in_fence
        self.bufs = []
        self._n = 0

    # ------------------------------------------------------------------ allocation ---
    def _alloc(self, shape, dtype, fence, label, output, skew=0):
        if isinstance(shape, int):
            shape = (shape,)
        shape = tuple(int(s) for s in shape)
        esz = torch.empty(0, dtype=dtype).element_size()
        nbytes = int(np.prod(shape, dtype=np.int64)) * esz
        assert skew % esz == 0, "a skewed view must stay aligned to its element size"
        raw = torch.full((fence + ALIGN + skew + nbytes + fence,), POISON, dtype=torch.uint8, device=self.device)
        start = fence + (-(raw.data_ptr() + fence)) % ALIGN + skew
        view = raw[start:start + nbytes].view(dtype).view(shape)
        assert view.is_contiguous() and view.data_ptr() % ALIGN == skew
        self._n += 1
        buf = _Buf(f"{label or 'buf'}#{self._n}{list(shape)}", raw, start, nbytes, view, output, fence)
        self.bufs.append(buf)
        return view

    def inp(self, array, dtype=torch.float32, label="inp", fence=None):
        """Device copy of a host array (or tensor), inside 4 KiB NaN fences (fence=out_fence: a
        buffer with initial values that an op accumulates into)."""
        src = array.detach().cpu() if isinstance(array, torch.Tensor) else torch.from_numpy(
            np.ascontiguousarray(np.asarray(array, dtype=_np_dtype(dtype))))
        t = self._alloc(src.shape, dtype, self.in_fence if fence is None else fence, label, False)
        t.copy_(src.to(dtype))
        return t

    def empty(self, shape, dtype=torch.float32, label="out", output=True):
        """An output: the body is poisoned, and check() wants every element of it written
        (output=False: a buffer that a refused call must leave untouched)."""
        return self._alloc(shape, dtype, self.out_fence, label, output)

    def full(self, shape, value, dtype=torch.float32, label="full"):
        t = self._alloc(shape, dtype, self.out_fence, label, False)
        t.fill_(value)
        return t

    def zeros(self, shape, dtype=torch.float32, label="zeros"):
        return self.full(shape, 0, dtype, label)

    def skewed(self, src, nbytes=4, label="skewed"):
        """The same contents (and the same fence size and output flag, for a tensor of this arena)
        with the data pointer `nbytes` past a 16-byte boundary.  The fences start at the first byte
        before and the first byte after the contents."""
        if not isinstance(src, torch.Tensor):
            src = torch.from_numpy(np.ascontiguousarray(np.asarray(src, dtype=np.float32)))
        rec = next((b for b in self.bufs if b.view is src), None)
        output = rec.output if rec is not None else False
        fence = rec.fence if rec is not None else self.in_fence  # a host array: an input
        t = self._alloc(src.shape, src.dtype, fence, label, output, skew=nbytes)
        t.reshape(-1).view(torch.uint8).copy_(src.contiguous().reshape(-1).view(torch.uint8))  # bit copy: poison stays poison
        if output:  # the skewed copy is the output now
            rec.output = False
        assert t.data_ptr() % 16 == nbytes % 16
        return t

    def is_untouched(self, t):
        """True when every element of an `empty` tensor is still poison."""
        rec = next(b for b in self.bufs if b.view is t)
        return bool((rec.elements() == rec.poison_value()).all())

    # ------------------------------------------------------------------------ check ---
    def check(self, outputs=None, extra=()):
        """AssertionError when a fence byte changed (label, side, first changed offset) or when an
        output still holds a poison element (label, count).  outputs: the tensors to hold to the
        no-poison rule; None: every tensor from empty().  One synchronisation when all is well:
        every fence and output reduces to one device flag first."""
        bufs = list(self.bufs) + [b for a in extra for b in a.bufs]
        if outputs is None:
            outs = [b for b in bufs if b.output]
        else:
            ids = {id(t) for t in outputs}
            outs = [b for b in bufs if id(b.view) in ids]
            assert len(outs) == len(ids), "check(outputs=...): a tensor that this arena did not allocate"
        if not bufs:
            return
        flag = torch.zeros((), dtype=torch.bool, device=self.device)
        for b in bufs:
            for _, f in b.sides():
                flag |= (f != POISON).any()
        for b in outs:
            if b.nbytes:
                flag |= (b.elements() == b.poison_value()).any()
        if not bool(flag):  # the one synchronisation
            return
        msgs = []
        for b in bufs:
            for side, f in b.sides():
                bad = torch.nonzero(f != POISON)
                if bad.numel():
                    first = int(bad[0]) if side == "rear" else int(bad[0]) - f.numel()
                    msgs.append(f"{b.label}: {side} fence changed, first at byte offset {first} "
                                f"({'past the end' if side == 'rear' else 'relative to the start'}), "
                                f"{bad.numel()} bytes in all")
        for b in outs:
            if b.nbytes:
                cnt = int((b.elements() == b.poison_value()).sum())
                if cnt:
                    msgs.append(f"{b.label}: output still holds {cnt} poison elements of {b.view.numel()}")
        raise AssertionError("fenced check failed:\n  " + "\n  ".join(msgs))


class FencedWorkspace:
    """The interface of ops._Workspace.  Every get() returns a fresh fenced buffer of exactly
    `nbytes`, poisoned with 0xFF, allocated and filled on the current stream and kept alive until
    the check: nothing is freed mid-test, so a two-stream engine stays race-free."""

    def __init__(self, device="cuda", fence=OUT_FENCE):
        self.arena = Arena(device, out_fence=fence)
        self.sizes = []

    @property
    def bufs(self):
        return self.arena.bufs

    def get(self, nbytes, device=None):
        self.sizes.append(int(nbytes))
        if device is not None and torch.device(device).type != self.arena.device.type:
            raise ValueError("FencedWorkspace: wrong device")
        with (torch.cuda.device(device) if self.arena.device.type == "cuda" and device is not None
              else contextlib.nullcontext()):
            return self.arena.empty(int(nbytes), torch.uint8, label="workspace", output=False)

    def check(self):
        self.arena.check()

    @contextlib.contextmanager
    def installed(self, ops):
        """Installs this object as ops.WORKSPACE for the block and restores the old one."""
        old = ops.WORKSPACE
        ops.WORKSPACE = self
        try:
            yield self
        finally:
            ops.WORKSPACE = old
