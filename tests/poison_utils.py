"""Helpers of tests/test_poison_host.py and tests/test_gpu_poison_*.py: fill every uninitialised buffer with a chosen byte.

A result of the package must not depend on the bytes of memory that no kernel of the call has written.  The suite cannot
see such a read by comparing two runs: a fresh process gets zeroed pages, and a second run gets the first run's block back
with the first run's values in it.  `poisoned(byte)` makes the bytes a parameter: while it is active, `torch.empty`,
`torch.empty_like` and `Tensor.new_empty` return their buffer with every byte set to `byte`.  The same call under two
fill bytes must then give the same result bytes; a difference is a read of unwritten memory, or an output cell that
nobody wrote.

Two fill bytes only:

* 0x00: what a fresh process sees;
* 0xFF: NaN as fp32, fp64 and bf16 (all exponent bits and a non-zero mantissa), -1 as every signed integer type.

No third "finite garbage" byte: a byte pattern that reads as a moderate float reads as an integer of about 1e9, and a
stray index read would then leave mapped memory; with 0xFF a stray integer is -1 and stays next to its buffer.  Integer
buffers are therefore checked by reading the code (each is written before it is read), the fills exist to find float reads.

What this leaves undetected:

* a stray float read that a select swallows: `x > 0 ? x : 0`, `fmaxf(x, 0)`, `isfinite(x) ? x : y` map NaN and 0.0 to
  the same value, and so does a comparison that only steers a branch whose two sides agree for the case at hand;
* a stray read whose value is multiplied into nothing: a product with a mask of exactly 0 still gives NaN (found), but a
  value that is loaded and never used is not a defect and is not found either;
* a stray integer read that lands on a valid entry under both fills (-1 and 0 are both clamped to row 0 by the gathers);
* a bool buffer (left alone: 0xFF is no bool) and a buffer that some other allocator call produces (`torch.zeros` is
  defined; `torch.empty_strided`, `resize_` and the C side's own allocations are not patched);
* memory that is written, but by the wrong call: a stale value of an earlier launch of the same step.  The decoy step of
  tests/stream_utils.py covers that.

Patching torch attributes for the length of a `with` block follows tests/stream_utils.py::skew.
"""
import contextlib

import torch

ZERO, ONES = 0x00, 0xFF
FILLS = (ZERO, ONES)

_ACTIVE = {"on": False}


class Fills:
    """What one `poisoned` block filled: `count` tensors, `nbytes` bytes, `sizes` (the byte size of every fill, in order)."""

    def __init__(self, byte, devices):
        self.byte, self.devices = byte, devices
        self.count, self.nbytes, self.sizes = 0, 0, []

    def __repr__(self):
        return f"Fills(byte=0x{self.byte:02X}, count={self.count}, nbytes={self.nbytes})"


@contextlib.contextmanager
def poisoned(byte, devices=("cuda",)):
    """While active, every tensor that `torch.empty`, `torch.empty_like` or `Tensor.new_empty` returns on a device whose
    type is in `devices` has all its bytes set to `byte` (tensors without elements and bool tensors are left alone).  After
    a fill on a GPU the device is synchronised, so no side stream of a step can run ahead of the fill.  Yields the `Fills`
    record.  Not re-entrant; the three functions are put back in a `finally`, after an exception too."""
    if not (isinstance(byte, int) and 0 <= byte <= 255):
        raise ValueError(f"poisoned: byte = {byte!r} is not in 0..255")
    if _ACTIVE["on"]:
        raise RuntimeError("poisoned: already active")
    rec = Fills(byte, tuple(devices))
    orig_empty, orig_like, orig_new = torch.empty, torch.empty_like, torch.Tensor.new_empty

    def fill(t):
        if not torch.is_tensor(t) or t.device.type not in rec.devices or t.numel() == 0 or t.dtype == torch.bool:
            return t
        flat = t.detach()
        if flat.is_contiguous():
            flat = flat.view(-1)
        else:       # empty_like of a permuted tensor keeps its strides: the fresh storage, whole
            flat = flat.as_strided((flat.untyped_storage().nbytes() // flat.element_size(),), (1,), 0)
        flat.view(torch.uint8).fill_(byte)
        if t.device.type == "cuda":
            torch.cuda.synchronize(t.device)
        n = flat.numel() * flat.element_size()
        rec.count += 1
        rec.nbytes += n
        rec.sizes.append(n)
        return t

    def empty(*a, **k):
        return fill(orig_empty(*a, **k))

    def empty_like(*a, **k):
        return fill(orig_like(*a, **k))

    def new_empty(self, *a, **k):
        return fill(orig_new(self, *a, **k))

    try:
        _ACTIVE["on"] = True
        torch.empty, torch.empty_like, torch.Tensor.new_empty = empty, empty_like, new_empty
        yield rec
    finally:
        torch.empty, torch.empty_like, torch.Tensor.new_empty = orig_empty, orig_like, orig_new
        _ACTIVE["on"] = False


def under_both(fn, devices=("cuda",)):
    """`fn()` once under each fill byte -> ((result under 0x00, its Fills), (result under 0xFF, its Fills))."""
    out = []
    for byte in FILLS:
        with poisoned(byte, devices) as rec:
            res = fn()
            if "cuda" in devices and torch.cuda.is_available():
                torch.cuda.synchronize()
        out.append((res, rec))
    return tuple(out)


@contextlib.contextmanager
def size_queries(*symbols):
    """While active, every value the library's size queries `symbols` (cartnet_workspace_bytes, ...) return is appended to
    the yielded list: the byte counts a liveness assertion looks for among `Fills.sizes`.  The wrappers sit on the loaded
    library object (cartnet_amd.lib.load()) and are taken off in a `finally`."""
    from cartnet_amd import lib
    cdll = lib.load()
    seen, orig = [], {s: getattr(cdll, s) for s in symbols}

    def wrap(fn):
        def query(*a):
            n = int(fn(*a))
            seen.append(n)
            return n
        return query

    try:
        for s, fn in orig.items():
            setattr(cdll, s, wrap(fn))
        yield seen
    finally:
        for s, fn in orig.items():
            setattr(cdll, s, fn)


def assert_live(rec, sizes, what, workspace=True):
    """The poison reached the call: at least one fill, and (with `workspace`) an allocation of exactly each queried
    workspace size among the fills."""
    assert rec.count > 0 and rec.nbytes > 0, f"{what}: nothing was filled with 0x{rec.byte:02X}"
    if workspace:
        assert sizes, f"{what}: no workspace size was queried"
        missing = [n for n in sizes if n not in rec.sizes]
        assert not missing, f"{what}: no fill of exactly the workspace size {missing} (fills: {sorted(set(rec.sizes))[-6:]})"


# --------------------------------------------------------------------------------------------------- results as bytes
def flatten(x, prefix="", out=None):
    """Every tensor, array, number, string and None inside a nested result (dict, list, tuple, an object with __dict__ or
    __slots__) as {path: leaf}; anything else by its `repr`.  What `assert_same_bytes` compares."""
    out = {} if out is None else out
    if torch.is_tensor(x) or x is None or isinstance(x, (bool, int, float, str, bytes)):
        out[prefix or "."] = x
    elif isinstance(x, dict):
        for k in x:
            flatten(x[k], f"{prefix}.{k}" if prefix else str(k), out)
    elif isinstance(x, (list, tuple)):
        for i, v in enumerate(x):
            flatten(v, f"{prefix}[{i}]", out)
    elif hasattr(x, "__dict__") or hasattr(x, "__slots__"):
        names = list(getattr(x, "__dict__", {})) + [s for s in getattr(type(x), "__slots__", ()) if hasattr(x, s)]
        for k in names:
            if not k.startswith("__"):
                flatten(getattr(x, k), f"{prefix}.{k}" if prefix else str(k), out)
    else:
        try:
            import numpy as np
            if isinstance(x, (np.ndarray, np.generic)):
                out[prefix or "."] = torch.as_tensor(np.ascontiguousarray(x))
                return out
        except ImportError:
            pass
        out[prefix or "."] = repr(x)        # (a torch.dtype, a device: compared as text)
    return out


def raw(t):
    """The bytes of a tensor (on the CPU), so that NaN compares equal to the same NaN."""
    t = t.detach().contiguous().cpu()
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    return t.reshape(-1).view(torch.uint8)


def assert_same_bytes(a, b, what):
    """Two nested results, leaf by leaf: the same paths, shapes and dtypes, the same bytes (several results hold NaN by
    contract); the message names the leaves that differ."""
    fa, fb = flatten(a), flatten(b)
    assert fa.keys() == fb.keys(), (what, sorted(set(fa) ^ set(fb)))
    assert any(torch.is_tensor(v) for v in fa.values()), f"{what}: the result holds no tensor"
    bad = []
    for k, x in fa.items():
        y = fb[k]
        if torch.is_tensor(x) != torch.is_tensor(y):
            bad.append(k)
        elif torch.is_tensor(x):
            if x.shape != y.shape or x.dtype != y.dtype or not torch.equal(raw(x), raw(y)):
                bad.append(k)
        elif isinstance(x, float) and isinstance(y, float):
            if torch.tensor(x, dtype=torch.float64).view(torch.int64) != torch.tensor(y, dtype=torch.float64).view(torch.int64):
                bad.append(k)
        elif x != y:
            bad.append(k)
    assert not bad, f"{what}: {len(bad)} of {len(fa)} fields differ between the fills 0x00 and 0xFF: {bad[:12]}"
