"""tests/poison_utils.py on the CPU (devices=("cpu",)): the harness sees a leak of unwritten bytes, and only that."""
import pytest
import torch

import poison_utils as pu

CPU = ("cpu",)


def _leaks():
    return torch.empty(4)                           # returned as allocated


def _fills():
    t = torch.empty(4)
    t.copy_(torch.arange(4.0))
    return t


def test_an_unwritten_buffer_differs_between_the_two_fills():
    (a, _), (b, _) = pu.under_both(_leaks, CPU)
    assert not torch.equal(pu.raw(a), pu.raw(b))
    assert bool((pu.raw(a) == 0x00).all()) and bool((pu.raw(b) == 0xFF).all())
    assert bool(torch.isnan(b).all())               # 0xFF is NaN as fp32 ...
    with pytest.raises(AssertionError, match=r"1 of 1 fields differ.*\['\.'\]"):
        pu.assert_same_bytes(a, b, "leak")


@pytest.mark.parametrize("dtype,value", [(torch.float64, None), (torch.bfloat16, None), (torch.float16, None),
                                         (torch.int8, -1), (torch.int16, -1), (torch.int32, -1), (torch.int64, -1),
                                         (torch.uint8, 255)])
def test_what_0xff_reads_as(dtype, value):
    with pu.poisoned(pu.ONES, CPU):
        t = torch.empty(3, dtype=dtype)
    assert bool(torch.isnan(t).all()) if value is None else bool((t == value).all())


def test_a_written_buffer_is_the_same_under_both_fills():
    (a, ra), (b, rb) = pu.under_both(_fills, CPU)
    pu.assert_same_bytes(a, b, "filled")
    assert ra.count == rb.count == 1                # (the poison was live all the same)


def test_all_three_functions_are_patched_and_counted():
    with pu.poisoned(pu.ONES, CPU) as rec:
        a = torch.empty(4)                                           # 16 bytes
        b = torch.empty_like(torch.zeros(3, 5, dtype=torch.float64))   # 120
        c = a.new_empty((2, 3), dtype=torch.int16)                   # 12
        d = torch.empty((2, 2), dtype=torch.int64, device="cpu")     # 32
        e = torch.empty_like(torch.zeros(4, 6).t())                  # 96, strides kept
        z = torch.zeros(7)                                           # not an uninitialised buffer: untouched, uncounted
    assert (rec.count, rec.nbytes, rec.sizes) == (5, 276, [16, 120, 12, 32, 96])
    assert rec.byte == 0xFF
    for t in (a, b, c, d, e):
        assert bool((pu.raw(t) == 0xFF).all())
    assert e.shape == (6, 4) and e.stride() == (1, 6)
    assert bool((z == 0).all())


def test_other_devices_bool_and_empty_tensors_are_left_alone():
    with pu.poisoned(pu.ONES, CPU) as rec:
        m = torch.empty(5, dtype=torch.bool)
        n = torch.empty(0)
        o = torch.empty((3, 0, 2), dtype=torch.int32)
        p = torch.empty(6, device="meta")                            # a device that is not among `devices`
    assert (rec.count, rec.nbytes, rec.sizes) == (0, 0, [])
    assert m.dtype == torch.bool and n.numel() == 0 and o.shape == (3, 0, 2) and p.device.type == "meta"
    with pu.poisoned(pu.ONES) as rec:                                # default devices: CUDA only
        q = torch.empty(4)
    assert rec.count == 0 and q.shape == (4,)


def test_the_functions_are_restored_after_an_exception():
    before = (torch.empty, torch.empty_like, torch.Tensor.new_empty)
    with pytest.raises(KeyError):
        with pu.poisoned(pu.ZERO, CPU):
            assert torch.empty is not before[0] and torch.empty_like is not before[1]
            assert torch.Tensor.new_empty is not before[2]
            raise KeyError("inside")
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == before
    with pu.poisoned(pu.ONES, CPU) as rec:                           # and the helper can be entered again
        torch.empty(1)
    assert rec.count == 1
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == before


def test_nesting_is_refused():
    with pu.poisoned(pu.ZERO, CPU):
        patched = torch.empty
        with pytest.raises(RuntimeError, match="already active"):
            with pu.poisoned(pu.ONES, CPU):
                pass
        assert torch.empty is patched                                # the refused block changed nothing
        t = torch.empty(2)
    assert bool((pu.raw(t) == 0).all())
    with pytest.raises(ValueError):
        with pu.poisoned(256, CPU):
            pass


def test_results_are_compared_as_bytes_field_by_field():
    nan = float("nan")
    a = {"x": torch.tensor([1.0, nan]), "n": 3, "s": "ok", "none": None, "l": [torch.tensor([1, 2]), (nan, 2.5)]}
    b = {"x": torch.tensor([1.0, nan]), "n": 3, "s": "ok", "none": None, "l": [torch.tensor([1, 2]), (nan, 2.5)]}
    pu.assert_same_bytes(a, b, "equal, NaN included")
    b["l"][0] = torch.tensor([1, 3])
    b["x"] = torch.tensor([1.0, -nan])                               # another NaN: other bytes
    with pytest.raises(AssertionError, match=r"2 of 7 fields differ.*'x', 'l\[0\]'"):
        pu.assert_same_bytes(a, b, "differs")
    with pytest.raises(AssertionError):
        pu.assert_same_bytes({"x": torch.zeros(2)}, {"y": torch.zeros(2)}, "other fields")
    with pytest.raises(AssertionError):
        pu.assert_same_bytes({"x": torch.zeros(2)}, {"x": torch.zeros(2, dtype=torch.float64)}, "other dtype")
    with pytest.raises(AssertionError, match="holds no tensor"):
        pu.assert_same_bytes({"n": 1}, {"n": 1}, "nothing to compare")
