"""The guard-band allocator (tests/fenced.py) proved on CPU tensors: a host write one element before
or after a body is reported with the right side and offset, an untouched output is reported, a
fully written one passes, skewed pointers land 4 bytes past a 16-byte boundary, and the fenced
workspace hands out exactly the bytes asked for."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import fenced  # noqa: E402


def _poke(t, elem_offset, value=1.0):
    """Writes one float at t.data_ptr() + 4 * elem_offset, as a stray host store would."""
    ctypes.c_float.from_address(t.data_ptr() + 4 * elem_offset).value = value


def test_write_after_body_is_reported():
    mem = fenced.Arena("cpu")
    out = mem.empty((3, 5))
    out.fill_(1.0)
    mem.check()
    _poke(out, out.numel())
    with pytest.raises(AssertionError, match=r"out#1\[3, 5\]: rear fence changed, first at byte offset [0-3] "):
        mem.check()


def test_write_before_body_is_reported():
    mem = fenced.Arena("cpu")
    mem.inp(np.ones(7))
    out = mem.empty(9)
    out.fill_(2.0)
    _poke(out, -1)
    with pytest.raises(AssertionError, match=r"out#2\[9\]: front fence changed, first at byte offset -[1-4] ") as e:
        mem.check()
    assert "rear" not in str(e.value) and "inp#1" not in str(e.value)


def test_input_fences_are_watched_too():
    mem = fenced.Arena("cpu")
    x = mem.inp(np.arange(6.0))
    assert x.dtype == torch.float32 and x.tolist() == [0, 1, 2, 3, 4, 5]
    _poke(x, 6 + 1000)  # still inside the 4 KiB fence
    with pytest.raises(AssertionError, match=r"inp#1\[6\]: rear fence changed, first at byte offset 400[0-3] "):
        mem.check()


def test_untouched_and_partly_written_outputs_are_reported():
    mem = fenced.Arena("cpu")
    out = mem.empty((4, 4))
    assert mem.is_untouched(out)
    with pytest.raises(AssertionError, match="output still holds 16 poison elements of 16"):
        mem.check()
    out.view(-1)[:13] = 0.5
    with pytest.raises(AssertionError, match="output still holds 3 poison elements of 16"):
        mem.check()
    with pytest.raises(AssertionError, match="poison"):
        mem.check(outputs=[out])
    out.fill_(float("nan"))  # a computed NaN is not the poison pattern
    mem.check()
    mem.check(outputs=[out])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.int16, torch.int32, torch.int64, torch.uint8])
def test_written_output_passes_in_every_dtype(dtype):
    mem = fenced.Arena("cpu")
    out = mem.empty((2, 3), dtype)
    assert out.dtype == dtype and out.shape == (2, 3) and out.is_contiguous()
    assert out.data_ptr() % 256 == 0
    if dtype.is_floating_point:
        assert bool(torch.isnan(out).all())
    elif dtype != torch.uint8:
        assert bool((out == -1).all())
    with pytest.raises(AssertionError, match="poison"):
        mem.check()
    out.zero_()
    mem.check()


def test_zeros_full_and_names_outputs():
    mem = fenced.Arena("cpu")
    z = mem.zeros(5)
    f = mem.full((2, 2), 7.0)
    s = mem.empty(3, output=False)
    assert not z.any() and bool((f == 7.0).all())
    mem.check()  # none of them is an output
    with pytest.raises(AssertionError, match="poison"):
        mem.check(outputs=[s])
    with pytest.raises(AssertionError, match="did not allocate"):
        mem.check(outputs=[torch.zeros(3)])


def test_skewed():
    mem = fenced.Arena("cpu")
    a = np.arange(10, dtype=np.float32)
    s = mem.skewed(a)
    assert s.data_ptr() % 16 == 4 and s.is_contiguous() and np.array_equal(s.numpy(), a)
    t = mem.inp(a)
    s2 = mem.skewed(t, 8)
    assert s2.data_ptr() % 16 == 8 and torch.equal(s2, t)
    mem.check()
    out = mem.skewed(mem.empty((2, 3)))  # a skewed output stays poisoned and stays an output
    assert out.data_ptr() % 16 == 4 and mem.is_untouched(out)
    with pytest.raises(AssertionError, match=r"skewed#5\[2, 3\]: output still holds 6 poison"):
        mem.check()
    out.fill_(0.0)
    mem.check()
    _poke(out, -1)  # the fence starts right at the skewed pointer
    with pytest.raises(AssertionError, match="front fence changed"):
        mem.check()


def test_fenced_workspace():
    class FakeOps:
        WORKSPACE = "old"

    ws = fenced.FencedWorkspace("cpu")
    with ws.installed(FakeOps):
        assert FakeOps.WORKSPACE is ws
        a = ws.get(1000, "cpu")
        b = ws.get(1000, "cpu")
    assert FakeOps.WORKSPACE == "old"
    assert a.numel() == 1000 and a.dtype == torch.uint8 and a.data_ptr() % 256 == 0
    assert a.data_ptr() != b.data_ptr() and bool((a == 0xFF).all())
    assert ws.sizes == [1000, 1000]
    ws.check()  # a workspace need not be written
    a.fill_(0)
    ws.check()
    ctypes.c_ubyte.from_address(b.data_ptr() + 1000).value = 0
    with pytest.raises(AssertionError, match=r"workspace#2\[1000\]: rear fence changed, first at byte offset 0 "):
        ws.check()
    mem = fenced.Arena("cpu")
    with pytest.raises(AssertionError, match="workspace#2"):  # an arena's check can cover the workspace as well
        mem.check(extra=[ws])
