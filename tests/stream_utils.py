"""Helpers of tests/test_gpu_stream_order.py: make one of a step's two streams late, and run the step every comparison uses.

The training step runs on two HIP streams (csrc/model_common.h `Streams`; the Python-sequenced iComformer / eComformer
backward with `wait_stream`).  Its kernels sum in fixed orders without atomics, so a correct schedule gives the same bytes
whatever the relative speed of the two streams, and the bytes of the one-stream schedule.  `skew` makes one stream late at
the start of each of its concurrent sections (cartnet_debug_stream_skew, include/cartnet_hip.h); `step` runs a decoy step
first, so that memory a missing wait would read too early or overwrite too early holds another step's values.
"""
import contextlib
import threading

import torch

OFF, SIDE, MAIN = 0, 1, 2
SPIN_MAX_USEC = 5000          # cartnet_debug_spin refuses more

_ACTIVE = {"which": OFF, "usec": 0, "thread": None, "spins": 0}


def _backward_functions():
    from cartnet_amd import comformer, model
    return [model._CartNetFunction, comformer._IcfNativeFunction, comformer._IComformerFunction]


def _side_handles(models):
    from cartnet_amd import comformer
    streams = [comformer._SIDE["stream"]]
    for m in models:
        streams += [getattr(m, "_aux_stream", None), getattr(m, "_aux", None)]
    return {s.cuda_stream for s in streams if s is not None}


@contextlib.contextmanager
def skew(which, usec, *models):
    """While active, the side (SIDE) or the main (MAIN) stream of every two-stream call is late by `usec` microseconds at
    the start of each of its concurrent sections; OFF queues nothing.  `models`: whose `_aux_stream` / `_aux` is the side
    stream (comformer._SIDE["stream"] always counts as one).

    The C seam is a per-thread setting and autograd runs a backward function in a thread of its own, so the setting is also
    applied around every backward of the package's autograd functions, in the thread that runs it, and switched off there
    afterwards.  `torch.cuda.Stream.wait_stream` is patched for the sequences written in Python: after `a.wait_stream(b)` a
    spin is queued on whichever of the two is the late stream (a: it has just waited; b: the other one waits for what it
    has just recorded).  Everything is put back in a `finally`, after an exception too."""
    from cartnet_amd import ops
    if which not in (OFF, SIDE, MAIN):
        raise ValueError(f"skew: which = {which!r} is not OFF, SIDE or MAIN")
    if not 0 <= int(usec) <= SPIN_MAX_USEC:
        raise ValueError(f"skew: usec = {usec!r} is outside 0..{SPIN_MAX_USEC}")
    if _ACTIVE["which"] != OFF:
        raise RuntimeError("skew: already active")
    orig_wait = torch.cuda.Stream.wait_stream
    fns = _backward_functions()
    orig_bwd = [f.__dict__["backward"] for f in fns]

    def wait_stream(a, b):
        orig_wait(a, b)
        if _ACTIVE["which"] == OFF:
            return
        sides = _side_handles(models)
        a_side, b_side = a.cuda_stream in sides, b.cuda_stream in sides
        if a_side == b_side:               # not an ordering between the main and the side stream
            return
        late = (a if a_side else b) if _ACTIVE["which"] == SIDE else (b if a_side else a)
        _ACTIVE["spins"] += 1
        ops.debug_spin(_ACTIVE["usec"], late)

    def wrap(fn):
        def backward(ctx, *grads):
            ops.debug_stream_skew(_ACTIVE["which"], _ACTIVE["usec"])
            try:
                return fn(ctx, *grads)
            finally:
                if threading.get_ident() != _ACTIVE["thread"]:      # (the calling thread keeps it until the block ends)
                    ops.debug_stream_skew(OFF)
        return staticmethod(backward)

    try:
        _ACTIVE.update(which=which, usec=int(usec) if which != OFF else 0, thread=threading.get_ident(), spins=0)
        ops.debug_stream_skew(_ACTIVE["which"], _ACTIVE["usec"])
        if which != OFF:
            torch.cuda.Stream.wait_stream = wait_stream
            for f, b in zip(fns, orig_bwd):
                f.backward = wrap(b.__func__)
        yield _ACTIVE
    finally:
        torch.cuda.Stream.wait_stream = orig_wait
        for f, b in zip(fns, orig_bwd):
            f.backward = b
        _ACTIVE.update(which=OFF, usec=0, thread=None)
        ops.debug_stream_skew(OFF)


def clone_batch(b):
    c = b.clone()
    c.num_graphs = b.num_graphs
    return c


def make_decoy(batch):
    """The same graph with other numbers: every shape is the batch's, so the caching allocator hands a step on it the
    blocks it hands a step on the batch; distances, directions, cells, temperatures and targets differ."""
    d = clone_batch(batch)
    c, s = 0.8, 0.6
    rot = torch.tensor([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float32, device=d.cart_dist.device)
    d.cart_dist = d.cart_dist * 0.83 + 0.05
    if getattr(d, "cart_dir", None) is not None:
        d.cart_dir = (d.cart_dir @ rot).contiguous()
    if getattr(d, "cell", None) is not None:
        d.cell = (d.cell @ rot * 1.07).contiguous()
    if getattr(d, "temperature", None) is not None:
        d.temperature = d.temperature * -0.7 + 0.3
    d.y = d.y * 1.9 + 0.4
    return d


def _pass(model, sd, batch, mode, opt):
    model.load_state_dict(sd)
    b = clone_batch(batch)
    if mode in ("train", "dropped"):
        model.train()
        if opt is not None:
            opt.zero_grad()
        else:
            model.zero_grad(set_to_none=True)
        pred, true = model(b)
        if mode == "train":
            (pred - true).abs().mean().backward()
    else:
        model.train(mode == "train_nograd")
        with torch.no_grad():
            pred, true = model(b)
    return pred, b


def step(model, sd, batch, decoy_batch, decoy_sd, mode="train", opt=None, after_decoy=None, timer=None):
    """One checked step: a full step with the decoy weights on the decoy batch, a device synchronisation, then the step
    with `sd` on `batch` whose results are returned as clones: `pred`, `x_out` / `e_out` where the model leaves them in the
    batch, `grad.<name>` of every parameter that has one, `buf.<name>` of every BatchNorm running buffer.
    mode "train": forward and (pred - true).abs().mean().backward(); "eval" / "train_nograd": an eval-mode / a training-mode
    forward under no_grad, the decoy likewise; "dropped": the decoy pass is a training-mode forward whose outputs are
    dropped without a backward and WITHOUT the synchronisation (its workspace goes back to the allocator while the side
    stream may still hold work on it), the second pass a full training step.
    `opt`: a FlatAdam attached to the model (its zero_grad is used).  `after_decoy()` runs between the synchronisation and
    the second pass.  `timer`: a dict that receives the second pass's device time as `ms` (HIP events on the main stream)."""
    _pass(model, decoy_sd, decoy_batch, mode, opt)
    if mode != "dropped":
        torch.cuda.synchronize()
    if after_decoy is not None:
        after_decoy()
    if timer is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    pred, b = _pass(model, sd, batch, "train" if mode == "dropped" else mode, opt)
    if timer is not None:
        e1.record()
    torch.cuda.synchronize()
    if timer is not None:
        timer["ms"] = e0.elapsed_time(e1)
    return collect(model, pred, b, grads=mode in ("train", "dropped"))


def collect(model, pred, b, grads=True):
    """The results of one pass as clones (tests/test_gpu_poison_steps.py compares the same set): `pred`, `x_out` / `e_out`
    where the model leaves them in the batch `b`, `grad.<name>` of every parameter that has one (`grads`), `buf.<name>` of
    every BatchNorm running buffer."""
    out = {"pred": pred.detach().clone()}
    if torch.is_tensor(getattr(b, "x", None)) and b.x.is_floating_point():
        out["x_out"] = b.x.detach().clone()
    if torch.is_tensor(getattr(b, "edge_attr", None)):
        out["e_out"] = b.edge_attr.detach().clone()
    if grads:
        for n, p in model.named_parameters():
            if p.grad is not None:
                out["grad." + n] = p.grad.detach().clone()
    for n, t in model.named_buffers():
        if "running_" in n or "num_batches_tracked" in n:
            out["buf." + n] = t.detach().clone()
    return out


def assert_same(ref, got, what, than="the one-stream step"):
    """Bitwise equality of two `step` / `collect` results, tensor by tensor; the message names the tensors that differ."""
    assert ref.keys() == got.keys(), (what, sorted(set(ref) ^ set(got)))
    bad = [k for k in ref if not torch.equal(ref[k], got[k])]
    assert not bad, f"{what}: {len(bad)} of {len(ref)} tensors differ from {than}: {bad[:12]}"
