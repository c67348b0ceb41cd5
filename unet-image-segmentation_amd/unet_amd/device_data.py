"""Device-resident training set: PairLoader's stream of batches, built on the device.

After its first decode a sample lives on the device as uint8 (a slot of two buffers, frames
(slots, H, W, 3) and masks (slots, H, W, 1)); from then on a batch that contains it costs the
upload of one int32 slot entry and its share of two `unet_batch_gather_u8` launches
(csrc/batch.hip), instead of a host uint8 -> fp32 conversion, a flip, a stack, a copy into pinned
memory and 4 bytes per value over PCIe.  For equal constructor arguments the k-th batch of
DevicePairLoader is bitwise the k-th batch of PairLoader: same listing, seed, shuffle order, flip
draws, sharding and `global_size` (the iteration is PairLoader's own; only `load` differs).

Three parts:
  SlotBook          the bookkeeping, pure Python: which slot a sample takes, which samples' bytes
                    must go up for a batch, the slot table with its flip encoding.  No device.
  _HostStore        the device's part restated in NumPy (data.gather_u8_reference): what the host
                    tests drive the bookkeeping with, and what DevicePairLoader(device=None) runs on.
  _DeviceStore      the device buffers, the pinned staging ring, the side stream and the launches.
"""
from __future__ import annotations

import os
from typing import List, NamedTuple, Tuple

import numpy as np

from .augment import affine_u8_reference
from .data import PairLoader, gather_u8_reference
from .dp import shard_bounds

STAGING_RING = 4  # pinned staging areas: Prefetcher keeps 3 batches in flight, one more is being filled


def encode_slot(slot: int, flip: bool) -> int:
    """A slot table entry: the slot as stored, or its complement for the mirrored sample (so slot
    0 mirrored is -1, distinct from slot 0)."""
    return ~int(slot) if flip else int(slot)


def decode_slot(entry: int) -> Tuple[int, bool]:
    entry = int(entry)
    return (~entry, True) if entry < 0 else (entry, False)


class BatchPlan(NamedTuple):
    entries: np.ndarray            # int32 (b,): encode_slot per batch position
    uploads: List[Tuple[int, int]]  # (sample, slot) whose bytes must go up before the gather, in batch order
    new_resident: List[Tuple[int, int]]  # the uploads that stay (SlotBook.commit)


class SlotBook:
    """Slots [0, resident) are given out once, in order of first use, and never taken back; slots
    [resident, resident + transient) are handed out anew for every batch, to the samples that found
    no resident slot.  A transient slot may be rewritten by the next batch only because uploads and
    gathers are ordered on one stream."""

    def __init__(self, resident: int, transient: int):
        if resident < 0 or transient < 0:
            raise ValueError("slot counts must be >= 0")
        self.resident, self.transient = int(resident), int(transient)
        self.slot_of = {}  # sample -> resident slot

    @property
    def slots(self) -> int:
        return self.resident + self.transient

    def plan(self, idx, flips) -> BatchPlan:
        """The slot table of the batch idx (flips: one flag per batch position) and the uploads it
        needs.  Changes nothing: commit() the plan once its uploads are issued."""
        entries = np.empty(len(idx), np.int32)
        uploads, new_resident, local = [], [], {}
        free = len(self.slot_of)
        for k, (i, f) in enumerate(zip(idx, flips)):
            i = int(i)
            slot = self.slot_of.get(i, local.get(i))
            if slot is None:
                if free < self.resident:
                    slot, free = free, free + 1
                    new_resident.append((i, slot))
                else:
                    slot = self.resident + len(uploads) - len(new_resident)
                    if slot >= self.slots:
                        raise ValueError(f"a batch of {len(idx)} samples needs more than {self.transient} "
                                         f"transient slots")
                local[i] = slot
                uploads.append((i, slot))
            entries[k] = encode_slot(slot, bool(f))
        return BatchPlan(entries, uploads, new_resident)

    def commit(self, plan: BatchPlan):
        for i, slot in plan.new_resident:
            self.slot_of[i] = slot


def upload_runs(uploads):
    """[(first upload, first slot, count)]: uploads whose slots are consecutive go up as one copy."""
    runs = []
    for p, (_, slot) in enumerate(uploads):
        if runs and runs[-1][1] + runs[-1][2] == slot:
            runs[-1][2] += 1
        else:
            runs.append([p, slot, 1])
    return [tuple(r) for r in runs]


class _HostStore:
    """The device's part in NumPy: two uint8 buffers and gather_u8_reference (affine_u8_reference
    for a batch that comes with transform records)."""

    def __init__(self, slots, size, augment=None):
        h, w = size
        self.augment = augment
        self.frames = np.zeros((max(slots, 1), h, w, 3), np.uint8)
        self.masks = np.zeros((max(slots, 1), h, w, 1), np.uint8)
        self.uploaded_bytes = 0

    def batch(self, plan: BatchPlan, pairs, records=None):
        for (_, slot), (f, m) in zip(plan.uploads, pairs):
            self.frames[slot], self.masks[slot] = f, m
            self.uploaded_bytes += f.nbytes + m.nbytes
        if records is not None:
            a = self.augment
            return (affine_u8_reference(self.frames, plan.entries, records, a.frame_order, a.fill_constant, a.cval),
                    affine_u8_reference(self.masks, plan.entries, records, a.mask_order, a.fill_constant, a.cval), None)
        return gather_u8_reference(self.frames, plan.entries), gather_u8_reference(self.masks, plan.entries), None


class _StagingArea:
    """One pinned buffer: the batch's new sample bytes and its table.  The table is `pairs` int32
    slot entries; for an augmented batch of b positions it is b entries followed at once by b
    transform records of 6 fp32 (room for 7 words per pair), so entries and records go up in one copy."""

    def __init__(self, torch, pairs, fbytes, mbytes, record_words=0):
        words = pairs * (1 + record_words)
        self.buf = torch.empty(pairs * (fbytes + mbytes) + 4 * words, dtype=torch.uint8, pin_memory=True)
        self.frames = self.buf[:pairs * fbytes].view(pairs, fbytes)
        self.masks = self.buf[pairs * fbytes:pairs * (fbytes + mbytes)].view(pairs, mbytes)
        self.table = self.buf[pairs * (fbytes + mbytes):].view(torch.int32)
        self.entries = self.table[:pairs]
        self.event = None  # recorded after the last copy that reads this area was issued


class _DeviceStore:
    """Uploads and gathers of one loader, all on one side stream of its own.  A staging area is
    rewritten only after the event behind its last copies has completed (a ring of STAGING_RING
    areas, so the wait is for a batch issued that many batches ago)."""

    def __init__(self, slots, size, pairs, device, augment=None):
        import torch
        self.augment = augment
        self.torch = torch
        self.device = torch.device(device)
        h, w = size
        self.size = (h, w)
        self.fbytes, self.mbytes = h * w * 3, h * w
        with torch.cuda.device(self.device):
            self.frames = torch.empty((max(slots, 1), h, w, 3), dtype=torch.uint8, device=self.device)
            self.masks = torch.empty((max(slots, 1), h, w, 1), dtype=torch.uint8, device=self.device)
            self.stream = torch.cuda.Stream(device=self.device)
        # the buffers were allocated on the constructing thread's stream and are only ever used on
        # self.stream: order the two once
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        self.frames.record_stream(self.stream)
        self.masks.record_stream(self.stream)
        self.ring = [_StagingArea(torch, pairs, self.fbytes, self.mbytes, 6 if augment else 0)
                     for _ in range(STAGING_RING)]
        self.turn = 0
        self.uploaded_bytes = 0

    def batch(self, plan: BatchPlan, pairs, records=None):
        from . import ops
        torch = self.torch
        area = self.ring[self.turn]
        self.turn = (self.turn + 1) % len(self.ring)
        if area.event is not None:
            area.event.synchronize()
        b, (h, w) = len(plan.entries), self.size
        fv, mv = area.frames.numpy(), area.masks.numpy()
        for p, (f, m) in enumerate(pairs):
            fv[p] = f.reshape(-1)
            mv[p] = m.reshape(-1)
        area.entries.numpy()[:b] = plan.entries
        if records is not None:
            area.table[b:7 * b].view(torch.float32).numpy()[:] = records.reshape(-1)
        fdev = self.frames.view(self.frames.shape[0], self.fbytes)
        mdev = self.masks.view(self.masks.shape[0], self.mbytes)
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            for p, slot, cnt in upload_runs(plan.uploads):
                fdev[slot:slot + cnt].copy_(area.frames[p:p + cnt], non_blocking=True)
                mdev[slot:slot + cnt].copy_(area.masks[p:p + cnt], non_blocking=True)
            words = b if records is None else 7 * b
            table = torch.empty(words, dtype=torch.int32, device=self.device)
            table.copy_(area.table[:words], non_blocking=True)
            entries = table[:b]
            x = torch.empty((b, h, w, 3), dtype=torch.float32, device=self.device)
            y = torch.empty((b, h, w, 1), dtype=torch.float32, device=self.device)
            if records is None:
                ops.batch_gather_u8(self.frames, entries, x)
                ops.batch_gather_u8(self.masks, entries, y)
            else:
                a, xf = self.augment, table[b:].view(torch.float32).view(b, 6)
                ops.batch_affine_u8(self.frames, entries, xf, x, a.frame_order, a.fill_constant, a.cval)
                ops.batch_affine_u8(self.masks, entries, xf, y, a.mask_order, a.fill_constant, a.cval)
            if area.event is None:
                area.event = torch.cuda.Event()
            area.event.record(self.stream)
            ready = torch.cuda.Event()
            ready.record(self.stream)
        self.uploaded_bytes += len(plan.uploads) * (self.fbytes + self.mbytes)
        return x, y, ready


def default_device_cache_bytes(dataset_bytes: int, device) -> int:
    """UNET_LOADER_CACHE_DEVICE_GB (per loader) when set; else the whole dataset if it fits in a
    quarter of the device memory free right now, else that quarter."""
    gb = os.environ.get("UNET_LOADER_CACHE_DEVICE_GB")
    if gb:
        return int(float(gb) * (1 << 30))
    if device is None:
        return dataset_bytes
    import torch
    free, _ = torch.cuda.mem_get_info(torch.device(device))
    return min(dataset_bytes, free // 4)


class DevicePairLoader(PairLoader):
    """PairLoader whose batches are built on `device` from a device-resident uint8 sample cache.
    It yields `Shard`s of fp32 device tensors with an `.event` (recorded on the loader's side stream
    after the two gather launches) that `Prefetcher` passes through, so model.fit / model.evaluate
    take it like a PairLoader.  device=None runs the same bookkeeping on NumPy buffers and yields
    host batches (the host tests' form).

    device_cache_bytes: the budget of resident samples (H*W*4 bytes per pair).  A sample gets a
    resident slot the first time it is decoded, while the budget lasts, and is not kept in the host
    uint8 cache; samples beyond the budget follow PairLoader's host cache rules (cache_bytes) and
    go through one local batch's worth of transient slots on every use, so any dataset size works
    with one kernel and one base pointer.  Default: UNET_LOADER_CACHE_DEVICE_GB (per loader) if set;
    otherwise the whole dataset when it fits in a quarter of the device memory
    torch.cuda.mem_get_info reports free at construction, else that quarter.  The default is a
    policy (train and validation loaders, the engine's activations and workspaces share the device),
    not a measured optimum.

    Decoding stays in PairLoader's thread pool, in the thread that iterates the loader (the
    Prefetcher's producer, ahead of the step).  Data parallel: each rank caches what its shards
    touch, within its own budget."""

    def __init__(self, frames_dir, masks_dir, size, batch_size, seed, shuffle=True, horizontal_flip=False, rank=0,
                 world=1, workers=16, cache_bytes=None, device="cuda", device_cache_bytes=None, augment=None):
        super().__init__(frames_dir, masks_dir, size, batch_size, seed, shuffle, horizontal_flip, rank, world,
                         workers, cache_bytes, augment)
        self.device = device
        self.pair_bytes = size[0] * size[1] * 4
        if device_cache_bytes is None:
            device_cache_bytes = default_device_cache_bytes(self.samples * self.pair_bytes, device)
        self.device_cache_bytes = int(device_cache_bytes)
        resident = min(self.samples, max(0, self.device_cache_bytes) // self.pair_bytes)
        lo, hi = shard_bounds(batch_size, world, 0)  # rank 0 holds the largest shard
        self.local_batch = hi - lo
        self.book = SlotBook(resident, 0 if resident >= self.samples else self.local_batch)
        self._store = None
        self._event = None

    @property
    def store(self):
        if self._store is None:
            if self.device is None:
                self._store = _HostStore(self.book.slots, self.size, self.augment)
            else:
                self._store = _DeviceStore(self.book.slots, self.size, self.local_batch, self.device, self.augment)
        return self._store

    def __iter__(self):
        for shard in super().__iter__():
            shard.event = self._event  # load() of this very batch set it
            yield shard

    def _decode(self, i, keep):
        f, m = self._sample_u8(i, keep=keep)
        if f.shape[:2] != tuple(self.size) or m.shape[:2] != tuple(self.size):
            raise ValueError(f"sample {i}: decoded to {f.shape}, {m.shape}, expected {tuple(self.size)}")
        return f, m

    def load(self, idx, flips, records=None):
        # with transform records the flip is in the record: the slot table is planned without flips
        plan = self.book.plan(idx, [records is None and bool(flips[i]) for i in idx])
        staying = {i for i, _ in plan.new_resident}
        jobs = [(i, i not in staying) for i, _ in plan.uploads]
        if self.workers > 1 and len(jobs) > 1:
            if self._pool is None:
                from concurrent.futures import ThreadPoolExecutor
                self._pool = ThreadPoolExecutor(self.workers, thread_name_prefix="unet-decode")
            pairs = list(self._pool.map(lambda j: self._decode(*j), jobs))
        else:
            pairs = [self._decode(*j) for j in jobs]
        x, y, self._event = self.store.batch(plan, pairs, records)
        self.book.commit(plan)
        return x, y
