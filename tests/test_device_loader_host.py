"""The device-resident loader's bookkeeping on the host (unet_amd/device_data.py): SlotBook with the
NumPy restatement of the batch-gather kernel (data.gather_u8_reference) in place of the device
reproduces PairLoader's batches bit for bit, whatever the resident budget."""
import os

import numpy as np
import pytest
from PIL import Image

from unet_amd.data import PairLoader, gather_u8_reference, global_batches
from unet_amd.device_data import DevicePairLoader, SlotBook, decode_slot, encode_slot, upload_runs

N, SIZE, BATCH, EPOCHS = 7, (16, 16), 3, 3
PAIR_BYTES = SIZE[0] * SIZE[1] * 4


def _write_dataset(root, n, size=(40, 30)):
    """As test_data_host._write_dataset, with masks of every grey level (not only 0 / 255)."""
    fr, mk = os.path.join(root, "frames"), os.path.join(root, "masks")
    os.makedirs(fr)
    os.makedirs(mk)
    rng = np.random.default_rng(0)
    for i in range(n):
        Image.fromarray(rng.integers(0, 256, (size[1], size[0], 3), dtype=np.uint8)).save(
            os.path.join(fr, f"f{i:03d}.png"))
        m = np.zeros((size[1], size[0]), np.uint8)
        m[5:5 + i % 7 + 3, 4:20] = 255
        m[20:25, 2:30] = rng.integers(0, 256, (5, 28), dtype=np.uint8)
        Image.fromarray(m).save(os.path.join(mk, f"f{i:03d}.png"))
    return fr, mk


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return _write_dataset(str(tmp_path_factory.mktemp("pairs")), N)


def _loaders(tree, rank, world, budget):
    kw = dict(seed=2301, shuffle=True, horizontal_flip=True, rank=rank, world=world, workers=2)
    return (PairLoader(*tree, SIZE, BATCH, **kw),
            DevicePairLoader(*tree, SIZE, BATCH, device=None, device_cache_bytes=budget, **kw))


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("budget", [N * PAIR_BYTES, 2 * PAIR_BYTES, 0], ids=["full", "two", "none"])
def test_bookkeeping_with_reference_gather_reproduces_pair_loader(tree, world, budget):
    per_epoch = len(list(global_batches(N, BATCH, world)))
    for rank in range(world):
        host, dev = _loaders(tree, rank, world, budget)
        assert dev.book.resident == min(N, budget // PAIR_BYTES)
        hi, di = iter(host), iter(dev)
        for k in range(EPOCHS * per_epoch):
            a, b = next(hi), next(di)
            assert a.global_size == b.global_size
            assert b[0].dtype == np.float32 and b[1].dtype == np.float32
            assert np.array_equal(a[0], b[0]), (rank, k)
            assert np.array_equal(a[1], b[1]), (rank, k)
        # resident samples are not held a second time on the host
        assert not set(dev._cache) & set(dev.book.slot_of)


def test_full_budget_uploads_nothing_after_the_first_epoch(tree):
    _, dev = _loaders(tree, 0, 1, N * PAIR_BYTES)
    it = iter(dev)
    per_epoch = len(list(global_batches(N, BATCH, 1)))
    for _ in range(per_epoch):
        next(it)
    assert dev.store.uploaded_bytes == N * PAIR_BYTES and len(dev.book.slot_of) == N
    for _ in range(2 * per_epoch):
        next(it)
    assert dev.store.uploaded_bytes == N * PAIR_BYTES
    order = np.random.default_rng(2301 + 1).permutation(N)
    plan = dev.book.plan(order[:BATCH], [False, True, False])
    assert plan.uploads == [] and plan.new_resident == []


def test_partial_budget_reuploads_only_the_overflow(tree):
    _, dev = _loaders(tree, 0, 1, 2 * PAIR_BYTES)
    it = iter(dev)
    per_epoch = len(list(global_batches(N, BATCH, 1)))
    for _ in range(2 * per_epoch):
        next(it)
    # 2 samples went up once; the other 5 go up in each of the two epochs
    assert dev.store.uploaded_bytes == (2 + 2 * (N - 2)) * PAIR_BYTES
    assert dev.book.slots == 2 + BATCH


def test_a_slot_is_never_assigned_to_two_live_samples():
    rng = np.random.default_rng(3)
    for resident in (0, 2, 5, 11):
        book = SlotBook(resident, 0 if resident >= 11 else 4)
        owner = {}
        for _ in range(40):
            idx = rng.permutation(11)[:rng.integers(1, 5)]
            plan = book.plan(idx, rng.random(len(idx)) < 0.5)
            live = {}  # slot -> sample within this batch
            for i, e in zip(idx, plan.entries):
                slot, _ = decode_slot(e)
                assert 0 <= slot < book.slots
                assert live.setdefault(slot, int(i)) == int(i)
                if slot < book.resident:  # resident: one owner for good
                    assert owner.setdefault(slot, int(i)) == int(i)
            for i, slot in plan.uploads:
                assert live[slot] == i
            assert all(slot >= book.resident for i, slot in plan.uploads if (i, slot) not in plan.new_resident)
            book.commit(plan)
        assert len(set(book.slot_of.values())) == len(book.slot_of) <= resident


def test_plan_changes_nothing_until_commit():
    book = SlotBook(3, 2)
    p1 = book.plan([4, 5], [False, True])
    assert book.slot_of == {} and book.plan([4, 5], [False, True]).uploads == p1.uploads
    book.commit(p1)
    assert book.slot_of == {4: 0, 5: 1}
    assert list(p1.entries) == [0, ~1]
    p2 = book.plan([5, 6, 7, 8], [False] * 4)
    assert p2.uploads == [(6, 2), (7, 3), (8, 4)] and p2.new_resident == [(6, 2)]
    with pytest.raises(ValueError, match="transient"):
        book.plan([6, 7, 8, 9], [False] * 4)
    assert upload_runs(p2.uploads) == [(0, 2, 3)]
    assert upload_runs([(1, 0), (2, 1), (3, 5), (4, 6), (9, 3)]) == [(0, 0, 2), (2, 5, 2), (4, 3, 1)]


def test_flip_encoding_round_trips():
    for slot in (0, 1, 7, 2 ** 31 - 1):
        for flip in (False, True):
            e = encode_slot(slot, flip)
            assert -2 ** 31 <= e < 2 ** 31 and decode_slot(e) == (slot, flip)
    assert encode_slot(0, True) == -1 and encode_slot(0, False) == 0
    assert decode_slot(np.int32(-1)) == (0, True)


def test_reference_gather_is_the_loaders_arithmetic_for_every_byte():
    src = np.arange(256, dtype=np.uint8).reshape(1, 4, 64, 1)
    want = src[0].astype(np.float32) / 255.0
    got = gather_u8_reference(src, [0, -1])
    assert got.dtype == np.float32
    assert np.array_equal(got[0], want) and np.array_equal(got[1], want[:, ::-1])
    rgb = np.random.default_rng(1).integers(0, 256, (3, 2, 5, 3), dtype=np.uint8)
    got = gather_u8_reference(rgb, [2, ~1, 0, 99, ~99])   # out-of-range entries clamp to the last sample
    assert np.array_equal(got[1], rgb[1][:, ::-1].astype(np.float32) / 255.0)   # pixels mirrored, channels kept
    assert np.array_equal(got[3], got[0]) and np.array_equal(got[4], got[0][:, ::-1])


def test_entry_point_refuses_before_any_launch():
    """unet_batch_gather_u8 validates on the host side of the ABI: no device is touched.  The
    pointers here are made-up addresses, so where a device is present the same refusals are held
    with real device buffers instead (test_batch_gather_gpu.py: test_entry_point_refusals)."""
    from ctypes import c_void_p
    import torch
    from unet_amd import _lib
    if torch.cuda.is_available():
        pytest.skip("device present: test_batch_gather_gpu.py holds the refusals with real buffers")
    lib = _lib.load()
    p = c_void_p(0x10000)
    for args, msg in [((p, 1, 4, 4, 2, p, 1, p, None), b"c must be 1 or 3"),
                      ((p, 1, 4, 4, 3, p, 1, c_void_p(0x10002), None), b"4-byte aligned"),
                      ((p, 1, 4, 4, 3, c_void_p(0x10001), 1, p, None), b"4-byte aligned"),
                      ((p, 0, 4, 4, 3, p, 1, p, None), b"positive"),
                      ((p, 1, 4, 4, 3, p, 0, p, None), b"positive"),
                      ((p, 1, 65536, 32768, 1, p, 1, p, None), b"2^31"),
                      ((p, 1, 4, 4, 3, None, 1, p, None), b"null pointer")]:
        assert lib.unet_batch_gather_u8(*args) < 0
        assert msg in lib.unet_last_error(), (args, lib.unet_last_error())
