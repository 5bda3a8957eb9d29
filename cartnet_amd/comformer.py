"""iComformer (BASELINE.json configs[4]: the alternative, edge-attention message-passing path) on the gfx950 kernels.

Drop-in for ``models/comformer.py:iComformer`` of the reference (same constructor, ``forward(data) -> (pred, true)``,
``state_dict`` keys incl. the two parameters the reference declares but never uses, ``lemb`` and ``lin_edge_len``).
The sub-modules only hold parameters.  iComformer's forward and backward are ONE call into libcartnet_hip.so each
(``_IcfNativeFunction`` -> cartnet_icomformer_forward / _backward, csrc/icomformer.hip: round 4); the same kernels
sequenced launch by launch from Python (``_IComformerFunction``) remain as eComformer's path and as the cross-check of the
C++ sequence (``model.native_sequence = False``).

Mapping onto the kernels (C = dim_in, heads = 1):
  * every Linear = ``cartnet_gemm``; ``key_update`` / ``lin_msg_update`` on ``cat[k_i, k_j, e]`` use the same algebraic
    split as the CartNet layer: node halves once per atom, gathered in the edge GEMM's epilogue
    (comformer_conv.py:90-99);
  * ``alpha = q_i * key / sqrt(C)`` and its BatchNorm statistics = ``cartnet_rowmul_fwd`` over the CSR rows;
  * ``msg * sigmoid(bn_att(alpha))`` + scatter-add = ``cartnet_gate_scatter_fwd`` (no envelope, no edge residual);
  * ``softplus(x + bn(lin_concate(out)))`` = ``cartnet_softplus_update_fwd``;
  * the edge layer (comformer_conv.py:156-193) runs the same machinery on 3E rows (edge x lattice vector) with
    "segments" of three rows per edge; the lattice-length terms are per crystal (3 rows each) and are gathered, not
    expanded to E rows; ``lin_concate`` is applied after the sum over the three lattice vectors
    (sum_i (m_i W^T + b) = (sum_i m_i) W^T + 3 b).
"""
from __future__ import annotations

import math
from typing import Dict, List

import numpy as np
import torch
import torch.nn as nn

import ctypes as C

from . import ops
from . import lib as _l
from .model import BN_EPS, BN_MOMENTUM, Cholesky_head, N_ATOM_TYPES


class _RBF(nn.Module):
    def __init__(self, vmin, vmax, bins):
        super().__init__()
        self.vmin, self.vmax, self.bins = vmin, vmax, bins
        centers = torch.linspace(vmin, vmax, bins)
        self.register_buffer("centers", centers)
        # models/utils.py:118-119: gamma = 1 / np.diff(centers).mean(), evaluated in float32 like the reference does
        self.gamma = float(1 / np.diff(centers.numpy()).mean())


class _MLP(nn.Sequential):
    def __init__(self, c):
        super().__init__(nn.Linear(3 * c, c), nn.SiLU(), nn.Linear(c, c))


class ComformerConv(nn.Module):
    """Parameter container (reference: models/comformer_conv.py:24-69)."""

    def __init__(self, c):
        super().__init__()
        self.lin_key, self.lin_query, self.lin_value = nn.Linear(c, c), nn.Linear(c, c), nn.Linear(c, c)
        self.lin_edge, self.lin_concate = nn.Linear(c, c), nn.Linear(c, c)
        self.lin_msg_update, self.key_update = _MLP(c), _MLP(c)
        self.bn, self.bn_att = nn.BatchNorm1d(c), nn.BatchNorm1d(c)


class ComformerConv_edge(nn.Module):
    """Parameter container (reference: models/comformer_conv.py:103-154)."""

    def __init__(self, c):
        super().__init__()
        self.lemb = nn.Embedding(3, 32)                       # declared by the reference, never used
        self.lin_key, self.lin_query, self.lin_value = nn.Linear(c, c), nn.Linear(c, c), nn.Linear(c, c)
        self.lin_key_e1, self.lin_value_e1 = nn.Linear(c, c), nn.Linear(c, c)
        self.lin_key_e2, self.lin_value_e2 = nn.Linear(c, c), nn.Linear(c, c)
        self.lin_key_e3, self.lin_value_e3 = nn.Linear(c, c), nn.Linear(c, c)
        self.lin_edge = nn.Linear(c, c, bias=False)
        self.lin_edge_len = nn.Linear(c + 32, c)              # declared by the reference, never used
        self.lin_concate = nn.Linear(c, c)
        self.lin_msg_update, self.key_update = _MLP(c), _MLP(c)
        self.bn_att, self.bn = nn.BatchNorm1d(c), nn.BatchNorm1d(c)


_GEMM_PRECISION = [0]     # CartnetGemmArgs.precision of the running forward / backward (set from model.gemm_precision)


_IMAGE_CACHE: Dict[tuple, tuple] = {}     # weight view -> (transposed copy, pre-split image); rebuilt every forward

# Image plan.  A step needs ~190 weight images (every Linear in both orientations, column blocks of the [C, 3C] weights,
# folded K-segments) and ~60 transposed copies.  Built lazily they cost one tiny launch AND ~100 us of host time each
# (19 of the 32 ms of host enqueue per step in round 2).  The first step records which views were asked for -- as
# (parameter, row / column window) so that the record survives the optimiser moving the parameters into a flat buffer --
# and every later forward refills ALL images of the plan with one batched launch per 80 (cartnet_gemm_pack_b /
# _split_b) and one batched transpose per 40, into the buffers of the step before.
_ACTIVE: Dict[str, object] = {"plan": None, "ranges": None}


def _locate(w: torch.Tensor):
    """(parameter name, row0, col0) of a 2-D view into one of the model's parameters, or None."""
    ranges = _ACTIVE["ranges"]
    if ranges is None or w.dim() != 2 or w.stride(1) != 1:
        return None
    ptr = w.data_ptr()
    for lo, hi, name, ld in ranges:
        if lo <= ptr < hi and w.stride(0) == ld:
            off = (ptr - lo) // 4
            return name, off // ld, off % ld
    return None


def _record(key, kind, views, value):
    """Remember a lazily built image so that the next forward prefills it (no-op for views that are not parameters)."""
    plan = _ACTIVE["plan"]
    if plan is None:
        return
    locs = [_locate(v) for v in views]
    if any(l is None for l in locs):
        return
    ident = (kind, tuple(locs), tuple(views[0].shape))     # by parameter window, not by address
    if ident in plan["index"]:
        return
    ent = {"kind": kind, "locs": locs, "shape": tuple(views[0].shape), "value": value}
    plan["entries"].append(ent)
    plan["index"][ident] = ent


def _begin_forward(model, P, prec):
    """Clear the per-step cache; from the second step on refill every planned image in a few batched launches."""
    _IMAGE_CACHE.clear()
    ranges = []
    for name, t in P.items():
        if t.dim() == 2 and t.is_contiguous():
            ranges.append((t.data_ptr(), t.data_ptr() + 4 * t.numel(), name, t.stride(0)))
    _ACTIVE["ranges"] = ranges
    plans = model.__dict__.setdefault("_image_plans", {})      # lives and dies with the model
    plan = plans.setdefault(prec, {"entries": [], "index": {}})
    _ACTIVE["plan"] = plan
    if not plan["entries"]:
        return
    fp32_img = prec == 0
    srcs, dsts, tsrc, tdst, keys = [], [], [], [], []
    for ent in plan["entries"]:
        r, c = ent["shape"]
        views = [P[n][r0:r0 + r, c0:c0 + c] for n, r0, c0 in ent["locs"]]
        kind = ent["kind"]
        if kind == "fwd":        # forward operand W^T: image of w.t() + a contiguous transposed copy
            w = views[0]
            t, im = ent["value"]
            srcs.append(w.t()); dsts.append(im)
            tsrc.append(w); tdst.append(t)
            keys.append(((w.data_ptr(), tuple(w.shape), tuple(w.stride()), prec), (t, im)))
        elif kind == "k":        # backward operand W as [K = out, N = in]
            w = views[0]
            im = ent["value"][1]
            srcs.append(w); dsts.append(im)
            keys.append(((w.data_ptr(), tuple(w.shape), tuple(w.stride()), prec, "k"), (None, im)))
        else:                    # "fold": the segments' images back to back in one buffer
            big = ent["value"][1]
            per = big.numel() // len(views)
            for i, w in enumerate(views):
                srcs.append(w); dsts.append(big[i * per:(i + 1) * per])
            keys.append(((tuple((w.data_ptr(), tuple(w.stride())) for w in views), tuple(views[0].shape), prec, "fold"),
                         (None, big)))
    ops.split_b(srcs, _fp32=fp32_img, outs=dsts)
    if tsrc:
        ops.transpose(tsrc, outs=tdst)
    for k, v in keys:
        _IMAGE_CACHE[k] = v


def _gemm(A, B, C_out, **kw):
    """ops.gemm at the model's GEMM precision (0 fp32 MFMA, 1 bf16x3, 2 bf16; shapes without such a kernel run fp32).

    At precision 1 / 2 a product Y = X W^T with the weight given as W [out, in] is handed over as the k-strided operand
    W^T with its pre-split image (cartnet_gemm_split_b, once per weight per step): that is the form the bf16 kernels
    implement."""
    prec = _GEMM_PRECISION[0]
    kw.setdefault("tile_policy", 1)   # grouped C x C products on the 128-wide fp32 kernel (CartnetGemmArgs.tile_policy)
    fp32_img = prec == 0      # precision 0: fp32 rows packed for the DMA-fed fp32-MFMA kernel (cartnet_gemm_pack_b)
    if not kw.get("b_kstrided", False) and not kw.get("a_kstrided", False) and kw.get("splitk", 1) == 1:
        Bs = list(B) if isinstance(B, (list, tuple)) else [B]
        if all(w.shape[0] % 256 == 0 and w.shape[1] % 16 == 0 for w in Bs):
            Bt, imgs = [], []
            for w in Bs:
                key = (w.data_ptr(), tuple(w.shape), tuple(w.stride()), prec)
                if key not in _IMAGE_CACHE:
                    _IMAGE_CACHE[key] = (w.t().contiguous(), ops.split_b([w.t()], _fp32=fp32_img)[0])
                    _record(key, "fwd", [w], _IMAGE_CACHE[key])
                t, im = _IMAGE_CACHE[key]
                Bt.append(t)
                imgs.append(im)
            kw = dict(kw, b_kstrided=True, b_split=imgs)
            return ops.gemm(A, Bt if isinstance(B, (list, tuple)) else Bt[0], C_out, precision=prec, **kw)
    if kw.get("b_kstrided", False) and not kw.get("a_kstrided", False) and kw.get("splitk", 1) == 1 and \
            "b_split" not in kw and "b_split_folded" not in kw:
        # dX = dY W with the weight as the k-strided operand [K = out, N = in]: same kernels, image of that orientation
        Bs = list(B) if isinstance(B, (list, tuple)) else [B]
        if not kw.get("segments", False):
            if all(w.shape[1] % 256 == 0 and w.shape[0] % 16 == 0 for w in Bs):
                imgs = []
                for w in Bs:
                    key = (w.data_ptr(), tuple(w.shape), tuple(w.stride()), prec, "k")
                    if key not in _IMAGE_CACHE:
                        _IMAGE_CACHE[key] = (None, ops.split_b([w], _fp32=fp32_img)[0])
                        _record(key, "k", [w], _IMAGE_CACHE[key])
                    imgs.append(_IMAGE_CACHE[key][1])
                kw = dict(kw, b_split=imgs)
        elif len(Bs) > 1 and all(w.shape == Bs[0].shape and w.shape[1] == 256 and w.shape[0] % 16 == 0 for w in Bs):
            # K-segments: the images of the segments back to back are the image of the product over the concatenated K
            # (taken by the kernel when the A segments are adjacent column blocks of one matrix, csrc/gemm.hip)
            key = (tuple((w.data_ptr(), tuple(w.stride())) for w in Bs), tuple(Bs[0].shape), prec, "fold")
            if key not in _IMAGE_CACHE:
                _IMAGE_CACHE[key] = (None, torch.cat(ops.split_b(Bs, _fp32=fp32_img)))
                _record(key, "fold", Bs, _IMAGE_CACHE[key])
            kw = dict(kw, b_split_folded=_IMAGE_CACHE[key][1])
    return ops.gemm(A, B, C_out, precision=prec, **kw)


def _e(shape, dev, dtype=torch.float32):
    return torch.empty(shape, dtype=dtype, device=dev)


def _parts(n, dev):
    return torch.empty((n,), dtype=torch.float64, device=dev)


def _split_k(K, tiles):
    # 256 workgroups = one per CU, like csrc/model.hip (split_k): the weight-gradient stream must not take both slots of
    # every CU from the main chain
    return int(max(1, min((256 + tiles - 1) // tiles, K // 256)))


_SIDE: Dict[str, Optional[torch.cuda.Stream]] = {"stream": None, "on": True}   # weight-gradient stream of the running backward
# Tensors the second stream reads or writes are kept ALIVE until the streams are joined at the end of backward (a list of
# references) instead of being marked with `record_stream`: a marked tensor's block is freed through an event the caching
# allocator then polls on every later allocation -- torch.empty cost 21 us apiece in backward, 7 ms of host time per step.
# A block that is never returned before the join cannot be handed out while the other stream still uses it.
_KEEP: list = []


def _wgrad(dY: List[torch.Tensor], X: List[torch.Tensor], outs: List[torch.Tensor], b_act=False):
    """outs[g] = dY[g]^T @ (silu?)(X[g]) (row reduction split over workgroups, slabs summed in fixed order).

    Nothing inside backward reads a weight gradient (``_join_wgrads`` covers the one exception), so the product and its
    slab reduction are queued on a second stream, next to the chain of activation gradients -- what
    cartnet_model_backward does for CartNet.  Operands are never written again after this call (the callers keep
    in-place updates in front of it) and are kept alive until the streams join (``_KEEP``)."""
    side = _SIDE["stream"] if _SIDE["on"] else None
    if side is None:
        return _wgrad_now(dY, X, outs, b_act)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _wgrad_now(dY, X, outs, b_act)
    _KEEP.extend(dY)
    _KEEP.extend(X)
    _KEEP.extend(outs)


class _side_branch:
    """``with _side_branch(inputs) as sb:`` runs a branch of backward that nothing on the main chain waits for (until a
    later ``_join_wgrads``) on the weight-gradient stream: the stream first waits for what the main stream has queued,
    the tensors the branch reads are marked as in use there, and ``sb.keep(t)`` marks a result that a later main-stream
    kernel reads.  Without a second stream it is a no-op context."""

    def __init__(self, inputs):
        self.inputs = [t for t in inputs if t is not None]
        self.side = _SIDE["stream"] if _SIDE["on"] else None
        self.ctx = None

    def __enter__(self):
        if self.side is not None:
            self.main = torch.cuda.current_stream()
            self.side.wait_stream(self.main)
            self.ctx = torch.cuda.stream(self.side)
            self.ctx.__enter__()
        return self

    def keep(self, *tensors):
        if self.side is not None:
            _KEEP.extend(tensors)                  # allocated on the side stream, read on the main one after the join
        return tensors[0] if len(tensors) == 1 else tensors

    def __exit__(self, *exc):
        if self.side is not None:
            self.ctx.__exit__(*exc)
            _KEEP.extend(self.inputs)
        return False


def _join_wgrads():
    """The main stream waits for every weight gradient queued so far."""
    if _SIDE["stream"] is not None and _SIDE["on"]:
        torch.cuda.current_stream().wait_stream(_SIDE["stream"])


def _wgrad_now(dY: List[torch.Tensor], X: List[torch.Tensor], outs: List[torch.Tensor], b_act=False):
    K, M = dY[0].shape
    N = X[0].shape[1]
    if K == 0:
        for o in outs:
            o.zero_()
        return
    tiles = len(dY) * ((M + 127) // 128) * ((N + 255) // 256 if N > 128 else 1)
    S = _split_k(K, tiles)
    if S == 1:
        _gemm(dY, X, outs, a_kstrided=True, b_kstrided=True, b_act=b_act)
        return
    slabs = [_e((S * M, N), dY[0].device) for _ in dY]
    _gemm(dY, X, slabs, a_kstrided=True, b_kstrided=True, b_act=b_act, splitk=S)
    ops.splitk_reduce(slabs, S, outs)


class _Attention:
    """Shared forward/backward of the gated attention block on ``R`` rows grouped into ``S`` segments.

    ComformerConv: rows = edges, segments = target atoms (CSR), node terms gathered by (tgt, src).
    ComformerConv_edge: rows = (edge, lattice vector), segments = edges (3 rows each), "node" terms gathered by
    (edge id, crystal*3 + lattice vector)."""

    @staticmethod
    def forward(P, B, pre, q, term_i, term_j, idx_i, idx_j, ea, seg_layout, count, training, sv):
        """pre-activation GEMM of key_update / lin_msg_update on the per-row operand ``ea`` with gathered terms,
        second Linears, alpha = q*key/sqrt(C), bn_att statistics, gated sum per segment.  Returns aggr [S, C]."""
        dev = ea.device
        R, C = ea.shape
        S = seg_layout.N
        W1k, W1m = P[pre + ".key_update.0.weight"], P[pre + ".lin_msg_update.0.weight"]
        pr = _e((R, 2 * C), dev)
        _gemm([ea, ea], [W1k[:, 2 * C:], W1m[:, 2 * C:]], [pr[:, :C], pr[:, C:]],
                 gather_i=[term_i[:, :C], term_i[:, C:]], gather_j=[term_j[:, :C], term_j[:, C:]], tgt=idx_i, src=idx_j)
        keyb = _e((R, 2 * C), dev)      # key' in the first half (second half unused: groups share a leading dim)
        gs = _e((R, 2 * C), dev)        # [alpha | msg]
        # silu(pr) is not kept for the second Linears' weight gradients (a_act_out, which would let them read a plain operand
        # on the all-DMA kernel).  Measured in rounds 2 and 3: no gain (36.5-36.7 vs 36.2-36.4 ms) -- the cheaper product sits
        # on the weight-gradient stream, which has slack, while the costlier forward GEMM sits on the critical chain.
        _gemm([pr[:, :C], pr[:, C:]], [P[pre + ".key_update.2.weight"], P[pre + ".lin_msg_update.2.weight"]],
                 [keyb[:, :C], gs[:, C:]], a_act=True,
                 bias=[P[pre + ".key_update.2.bias"], P[pre + ".lin_msg_update.2.bias"]])
        npart = ops.segment_nparts(S)
        ps, pq = _parts(npart * C, dev), _parts(npart * C, dev)
        scale = 1.0 / math.sqrt(C)
        ops.rowmul_fwd(keyb[:, :C], q, seg_layout.rowptr, scale, gs[:, :C], ps, pq)
        mr1 = _e((2 * C,), dev)
        ops.bn_finalize(ps, pq, npart, count, C, BN_EPS, BN_MOMENTUM, training, B[pre + ".bn_att.running_mean"],
                        B[pre + ".bn_att.running_var"], B[pre + ".bn_att.num_batches_tracked"], mr1)
        aggr = _e((S, C), dev)
        gp = ops.gate_nparts(S)
        ops.gate_scatter_fwd(gs, None, None, seg_layout, mr1, P[pre + ".bn_att.weight"], P[pre + ".bn_att.bias"], None,
                             aggr, _parts(gp * C, dev), _parts(gp * C, dev))
        sv.update(pr=pr, keyb=keyb, gs=gs, mr1=mr1, aggr=aggr)
        return aggr

    @staticmethod
    def backward(P, G, pre, daggr, q, ea, seg_layout, count, training, sv, dq_out):
        """Consumes sv; returns dpre [R, 2C] (gradient at the first Linears' pre-activation, key | msg) after
        writing the parameter gradients of the second Linears / bn_att and dq into ``dq_out``."""
        dev = ea.device
        R, C = ea.shape
        S = seg_layout.N
        pr, keyb, gs, mr1 = sv["pr"], sv["keyb"], sv["gs"], sv["mr1"]
        gp = ops.gate_nparts(S)
        pa, pb = _parts(gp * C, dev), _parts(gp * C, dev)
        ga, gb = P[pre + ".bn_att.weight"], P[pre + ".bn_att.bias"]
        ops.gate_scatter_bwd_stats(gs, None, daggr, None, seg_layout, mr1, ga, gb, pa, pb)
        sums1 = _e((2 * C,), dev)
        ops.colsum_finalize([pa, pb], gp, [sums1[:C], sums1[C:]])
        G[pre + ".bn_att.bias"], G[pre + ".bn_att.weight"] = sums1[:C], sums1[C:]
        pdg, pds = _parts(gp * C, dev), _parts(gp * C, dev)
        ops.gate_scatter_bwd_apply(gs, None, daggr, None, seg_layout, mr1, ga, gb, sums1, training, pdg, pds)
        G[pre + ".lin_msg_update.2.bias"] = _e((C,), dev)
        ops.colsum_finalize(pds, gp, G[pre + ".lin_msg_update.2.bias"])
        ops.rowmul_bwd(gs[:, :C], keyb[:, :C], q, seg_layout.rowptr, 1.0 / math.sqrt(C), dq_out)   # gs = [dkey | dmsg]
        G[pre + ".key_update.2.bias"] = _e((C,), dev)
        ops.colsum(gs[:, :C], G[pre + ".key_update.2.bias"])
        G[pre + ".key_update.2.weight"], G[pre + ".lin_msg_update.2.weight"] = _e((C, C), dev), _e((C, C), dev)
        _wgrad([gs[:, :C], gs[:, C:]], [pr[:, :C], pr[:, C:]],
               [G[pre + ".key_update.2.weight"], G[pre + ".lin_msg_update.2.weight"]], b_act=True)
        tiles = ops.gemm_tiles_m(R)
        csk, csm = _parts(tiles * C, dev), _parts(tiles * C, dev)
        dpr = _e((R, 2 * C), dev)       # not in place over pr: the weight-gradient stream may still be reading silu(pr)
        _gemm([gs[:, :C], gs[:, C:]], [P[pre + ".key_update.2.weight"], P[pre + ".lin_msg_update.2.weight"]],
                 [dpr[:, :C], dpr[:, C:]], b_kstrided=True, dact=[pr[:, :C], pr[:, C:]], colsum=[csk, csm])
        pr = dpr
        G[pre + ".key_update.0.bias"], G[pre + ".lin_msg_update.0.bias"] = _e((C,), dev), _e((C,), dev)
        ops.colsum_finalize([csk, csm], tiles, [G[pre + ".key_update.0.bias"], G[pre + ".lin_msg_update.0.bias"]])
        dW1k, dW1m = _e((C, 3 * C), dev), _e((C, 3 * C), dev)
        G[pre + ".key_update.0.weight"], G[pre + ".lin_msg_update.0.weight"] = dW1k, dW1m
        _wgrad([pr[:, :C], pr[:, C:]], [ea, ea], [dW1k[:, 2 * C:], dW1m[:, 2 * C:]])
        return pr, dW1k, dW1m


class _IComformerFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model: "iComformer", batch, training: bool, *params):
        P: Dict[str, torch.Tensor] = dict(zip(model._param_names, params))
        B: Dict[str, torch.Tensor] = dict(model.named_buffers())
        need_grad = bool(getattr(model, "_grad_mode", True)) and any(ctx.needs_input_grad)
        ctx.gemm_precision = int(model.gemm_precision)
        _GEMM_PRECISION[0] = ctx.gemm_precision
        _begin_forward(model, P, ctx.gemm_precision)
        C = model.dim_in
        dev = params[0].device
        z = batch.x
        if not (torch.is_tensor(z) and z.dtype == torch.int64 and z.dim() == 1):
            raise ValueError("batch.x must hold int64 atomic numbers [N]")
        N, E, Bg = int(z.shape[0]), int(batch.edge_index.shape[1]), int(batch.num_graphs)
        gptr = batch.ptr.to(dev)
        lay = ops.GraphLayout(batch.edge_index, N, gptr)
        if model.validate_graph:
            lay.validate()
        sv = {"lay": lay, "N": N, "E": E, "Bg": Bg, "training": training}

        # ---- embeddings (comformer.py:116-124)
        x = _e((N, C), dev)
        T = batch.temperature.contiguous()
        ops.node_embed(z, batch.batch, T, P["embedding.weight"], P["temperature_proj_atom.weight"],
                       P["temperature_proj_atom.bias"], None, x)
        equi_model = getattr(model, "kind", "i") == "e"
        edge_feat, nl, nc = _e((max(E, 1),), dev), _e((Bg * 3,), dev), _e((max(E, 1) * 3,), dev)
        # edge_feat = -0.75 / dist for both models (comformer.py:59,117); the lattice terms are iComformer's only
        cell = batch.cell.contiguous()
        ops.lattice_features(cell, batch.batch, lay.src, batch.cart_dist.contiguous(), batch.cart_dir.contiguous(),
                             edge_feat, nl, nc)

        def rbf_branch(vals, n, rbf_mod, cbuf, lin, tag):
            r = _e((n, C), dev)
            ops.rbf_expand(vals, B[cbuf], rbf_mod.gamma, r)
            pre = _e((n, C), dev)
            _gemm(r, P[lin + ".weight"], pre, bias=P[lin + ".bias"])
            out = _e((n, C), dev)
            ops.eltwise(0, pre, None, out)
            sv[tag] = (r, pre)
            return out

        e = rbf_branch(edge_feat[:E], E, model.rbf[0], "rbf.0.centers", "rbf.1", "rbf_e")
        sv.update(z=z, gid=batch.batch, T=T, equi_model=equi_model)
        if not equi_model:
            NLt = rbf_branch(nl, Bg * 3, model.rbf[0], "rbf.0.centers", "rbf.1", "rbf_nl")           # [Bg*3, C]
            NA = rbf_branch(nc[:3 * E], 3 * E, model.rbf_angle[0], "rbf_angle.0.centers", "rbf_angle.1", "rbf_na")
            # index helpers for the edge layer: row r = 3*edge + lattice vector
            ar3 = torch.arange(3 * E, device=dev, dtype=torch.int32)
            idx_edge = torch.div(ar3, 3, rounding_mode="floor").to(torch.int32).contiguous()
            g_of_e = batch.batch[batch.edge_index[0]].to(torch.int32)
            idx_gl = (g_of_e.repeat_interleave(3) * 3 + ar3 % 3).to(torch.int32).contiguous()
            ptr3 = (3 * torch.arange(E + 1, device=dev, dtype=torch.int32)).contiguous()
            seg3 = ops.SegmentLayout(ptr3, 3 * E)
            gedge_ptr = lay.rowptr[gptr.long()].contiguous()          # edge range of every crystal
            sv.update(idx_edge=idx_edge, idx_gl=idx_gl, seg3=seg3, gedge_ptr=gedge_ptr)

        def conv(l, x, e):
            p = f"att_layers.{l}"
            s = {}
            QKV = _e((N, 3 * C), dev)
            _gemm([x, x, x], [P[p + ".lin_query.weight"], P[p + ".lin_key.weight"], P[p + ".lin_value.weight"]],
                     [QKV[:, :C], QKV[:, C:2 * C], QKV[:, 2 * C:]],
                     bias=[P[p + ".lin_query.bias"], P[p + ".lin_key.bias"], P[p + ".lin_value.bias"]])
            ea = _e((E, C), dev)
            _gemm(e, P[p + ".lin_edge.weight"], ea, bias=P[p + ".lin_edge.bias"])
            W1k, W1m = P[p + ".key_update.0.weight"], P[p + ".lin_msg_update.0.weight"]
            k, v = QKV[:, C:2 * C], QKV[:, 2 * C:]
            KPi, KPj = _e((N, 2 * C), dev), _e((N, 2 * C), dev)      # [key | msg] node terms for target / source
            _gemm([k, v, k, v], [W1k[:, :C], W1m[:, :C], W1k[:, C:2 * C], W1m[:, C:2 * C]],
                     [KPi[:, :C], KPi[:, C:], KPj[:, :C], KPj[:, C:]],
                     bias=[P[p + ".key_update.0.bias"], P[p + ".lin_msg_update.0.bias"], None, None])
            aggr = _Attention.forward(P, B, p, QKV[:, :C], KPi, KPj, lay.tgt, lay.src, ea, lay, E, training, s)
            tiles = ops.gemm_tiles_m(N)
            cs, cq = _parts(tiles * C, dev), _parts(tiles * C, dev)
            o = _e((N, C), dev)
            _gemm(aggr, P[p + ".lin_concate.weight"], o, bias=P[p + ".lin_concate.bias"], colsum=cs, colsq=cq)
            mr2 = _e((2 * C,), dev)
            ops.bn_finalize(cs, cq, tiles, N, C, BN_EPS, BN_MOMENTUM, training, B[p + ".bn.running_mean"],
                            B[p + ".bn.running_var"], B[p + ".bn.num_batches_tracked"], mr2)
            y = _e((N, C), dev)
            ops.softplus_update_fwd(o, x, mr2, P[p + ".bn.weight"], P[p + ".bn.bias"], y)
            s.update(x=x, e=e, QKV=QKV, ea=ea, o=o, mr2=mr2)
            sv[p] = s
            return y

        def conv_edge(e):
            p = "edge_update_layer"
            s = {}
            QKV = _e((E, 3 * C), dev)
            _gemm([e, e, e], [P[p + ".lin_query.weight"], P[p + ".lin_key.weight"], P[p + ".lin_value.weight"]],
                     [QKV[:, :C], QKV[:, C:2 * C], QKV[:, 2 * C:]],
                     bias=[P[p + ".lin_query.bias"], P[p + ".lin_key.bias"], P[p + ".lin_value.bias"]])
            NL3 = NLt.view(Bg, 3 * C)
            KY, VY = _e((Bg, 3 * C), dev), _e((Bg, 3 * C), dev)
            for out, kind in ((KY, "key"), (VY, "value")):
                _gemm([NL3[:, i * C:(i + 1) * C] for i in range(3)],
                         [P[p + f".lin_{kind}_e{i + 1}.weight"] for i in range(3)],
                         [out[:, i * C:(i + 1) * C] for i in range(3)],
                         bias=[P[p + f".lin_{kind}_e{i + 1}.bias"] for i in range(3)])
            exy = _e((3 * E, C), dev)
            _gemm(NA, P[p + ".lin_edge.weight"], exy)
            W1k, W1m = P[p + ".key_update.0.weight"], P[p + ".lin_msg_update.0.weight"]
            Ka = _e((E, 2 * C), dev)            # per-edge term   [key | msg]
            _gemm([QKV[:, C:2 * C], QKV[:, 2 * C:]], [W1k[:, :C], W1m[:, :C]], [Ka[:, :C], Ka[:, C:]],
                     bias=[P[p + ".key_update.0.bias"], P[p + ".lin_msg_update.0.bias"]])
            KYb = _e((Bg * 3, 2 * C), dev)      # per (crystal, lattice vector) term
            _gemm([KY.view(Bg * 3, C), VY.view(Bg * 3, C)], [W1k[:, C:2 * C], W1m[:, C:2 * C]],
                     [KYb[:, :C], KYb[:, C:]])
            aggr = _Attention.forward(P, B, p, QKV[:, :C], Ka, KYb, idx_edge, idx_gl, exy, seg3, 3 * E, training, s)
            bias3 = _e((1, C), dev)
            ops.eltwise(3, P[p + ".lin_concate.bias"].view(1, C), None, bias3, 3.0)
            tiles = ops.gemm_tiles_m(E)
            cs, cq = _parts(tiles * C, dev), _parts(tiles * C, dev)
            o = _e((E, C), dev)
            _gemm(aggr, P[p + ".lin_concate.weight"], o, bias=bias3.view(C), colsum=cs, colsq=cq)
            mr2 = _e((2 * C,), dev)
            ops.bn_finalize(cs, cq, tiles, E, C, BN_EPS, BN_MOMENTUM, training, B[p + ".bn.running_mean"],
                            B[p + ".bn.running_var"], B[p + ".bn.num_batches_tracked"], mr2)
            y = _e((E, C), dev)
            ops.softplus_update_fwd(o, e, mr2, P[p + ".bn.weight"], P[p + ".bn.bias"], y)
            s.update(e=e, QKV=QKV, KY=KY, VY=VY, exy=exy, o=o, mr2=mr2)
            sv[p] = s
            return y

        def equi(x, e):
            """ComformerConvEqui (comformer_conv.py:266-279) on the tensor-product kernels of csrc/equi_ops.hip."""
            p = "equi_update"
            s = {}
            ns = ops.EQUI_NS
            x0 = _e((N, ns), dev)
            _gemm(x, P[p + ".node_linear.weight"], x0, bias=P[p + ".node_linear.bias"])
            cdir = batch.cart_dir.contiguous()
            for li in (1, 2):       # the two edge MLPs: Linear, Softplus, Linear -> per-edge weights [E, 5120]
                q = f"{p}.nlayer_{li}"
                hpre, hact, w = _e((E, C), dev), _e((E, C), dev), _e((E, ops.EQUI_NW), dev)
                _gemm(e, P[q + ".fc.0.weight"], hpre, bias=P[q + ".fc.0.bias"])
                ops.eltwise(0, hpre, None, hact)
                _gemm(hact, P[q + ".fc.2.weight"], w, bias=P[q + ".fc.2.bias"])
                s[f"hpre{li}"], s[f"hact{li}"], s[f"w{li}"] = hpre, hact, w
            h1 = _e((N, ops.EQUI_H1), dev)
            ops.equi_tp1_fwd(x0, s["w1"], cdir, lay, h1)
            o2 = _e((N, ns), dev)
            ops.equi_tp2_fwd(h1, s["w2"], cdir, lay, o2)
            np_ = ops.colstats_nparts(N)
            ps, pq = _parts(np_ * ns, dev), _parts(np_ * ns, dev)
            ops.colstats_partial(o2, ps, pq)
            mr = _e((2 * ns,), dev)
            ops.bn_finalize(ps, pq, np_, N, ns, BN_EPS, BN_MOMENTUM, training, B[p + ".bn.running_mean"],
                            B[p + ".bn.running_var"], B[p + ".bn.num_batches_tracked"], mr)
            zero = torch.zeros(N, ns, device=dev)
            y1 = _e((N, ns), dev)
            ops.softplus_update_fwd(o2, zero, mr, P[p + ".bn.weight"], P[p + ".bn.bias"], y1)   # softplus(bn(o2))
            y2pre, y2, out = _e((N, C), dev), _e((N, C), dev), _e((N, C), dev)
            _gemm(y1, P[p + ".node_linear_2.weight"], y2pre, bias=P[p + ".node_linear_2.bias"])
            ops.eltwise(0, y2pre, None, y2)
            _gemm(x, P[p + ".skip_linear.weight"], out, bias=P[p + ".skip_linear.bias"], resid=y2)
            s.update(x=x, e=e, x0=x0, h1=h1, o2=o2, mr=mr, zero=zero, y1=y1, y2pre=y2pre, cdir=cdir)
            sv[p] = s
            return out

        x = conv(0, x, e)
        if equi_model:              # models/comformer.py:64-67
            x = equi(x, e)
            for l in (1, 2):
                x = conv(l, x, e)
        else:
            sv["NLt"], sv["NA"] = NLt, NA
            e = conv_edge(e)
            for l in (1, 2, 3):
                x = conv(l, x, e)

        # ---- Cholesky head (shared with CartNet)
        H = C // 2
        hid = _e((N, H), dev)
        _gemm(x, P["cholesky.MLP.0.weight"], hid, bias=P["cholesky.MLP.0.bias"])
        M = int(batch.y.shape[0])
        idx = torch.empty(N, dtype=torch.int32, device=dev)
        ops.mask_index(batch.non_H_mask.contiguous(), idx, None)
        p6, pred = _e((M, 6), dev), _e((M, 3, 3), dev)
        ops.cholesky_head_fwd(hid, idx, P["cholesky.MLP.2.weight"], P["cholesky.MLP.2.bias"], p6, pred)
        sv.update(hid=hid, idx=idx, p6=p6, x_final=x, P=P, model=model)
        ctx.sv = sv if need_grad else None
        ctx.mark_non_differentiable(x)
        return pred, x

    @staticmethod
    def backward(ctx, dpred, _dx_unused):
        sv = ctx.sv
        if sv is None:
            raise RuntimeError("iComformer backward called without saved state")
        _GEMM_PRECISION[0] = ctx.gemm_precision
        ctx.sv = None
        P, model, lay = sv["P"], sv["model"], sv["lay"]
        if _KEEP:                   # a previous backward raised before its join: the side stream may still read these
            if _SIDE["stream"] is not None:
                torch.cuda.current_stream().wait_stream(_SIDE["stream"])
            _KEEP.clear()
        _SIDE["on"] = bool(getattr(model, "overlap_weight_gradients", True))
        if _SIDE["on"] and (_SIDE["stream"] is None or _SIDE["stream"].device != dpred.device):
            _SIDE["stream"] = torch.cuda.Stream(device=dpred.device)
        N, E, Bg, training = sv["N"], sv["E"], sv["Bg"], sv["training"]
        C = model.dim_in
        H = C // 2
        dev = dpred.device
        G: Dict[str, torch.Tensor] = {}

        # ---- head
        nparts_n = ops.node_nparts(N)
        row = 7 * H + 8
        parts = _e((nparts_n * row,), dev)
        dhid = _e((N, H), dev)
        ops.cholesky_head_bwd(sv["hid"], sv["idx"], P["cholesky.MLP.2.weight"], sv["p6"], dpred.contiguous(), dhid, parts)
        tot = _e((row,), dev)
        ops.colsum_finalize(parts, nparts_n, tot)
        G["cholesky.MLP.2.weight"], G["cholesky.MLP.2.bias"] = tot[:6 * H].view(6, H), tot[6 * H:6 * H + 6]
        G["cholesky.MLP.0.bias"] = tot[6 * H + 8:]
        G["cholesky.MLP.0.weight"] = _e((H, C), dev)
        _wgrad([dhid], [sv["x_final"]], [G["cholesky.MLP.0.weight"]])
        dx = _e((N, C), dev)
        _gemm(dhid, P["cholesky.MLP.0.weight"], dx, b_kstrided=True)

        def softplus_bwd(p, s, dy, rows, x_in):
            """Backward of y = softplus(x_in + bn(o)): returns (d_o, d_residual)."""
            np_ = ops.segment_nparts(rows)
            pa, pb = _parts(np_ * C, dev), _parts(np_ * C, dev)
            ops.softplus_update_bwd_stats(s["o"], x_in, dy, s["mr2"], P[p + ".bn.weight"], P[p + ".bn.bias"], pa, pb)
            sums = _e((2 * C,), dev)
            ops.colsum_finalize([pa, pb], np_, [sums[:C], sums[C:]])
            G[p + ".bn.bias"], G[p + ".bn.weight"] = sums[:C], sums[C:]
            d_o, dres = _e((rows, C), dev), _e((rows, C), dev)
            ops.softplus_update_bwd_apply(s["o"], x_in, dy, s["mr2"], P[p + ".bn.weight"], P[p + ".bn.bias"], sums,
                                          training, d_o, None, dres)
            return d_o, dres

        def linear3_bwd(p, dQKV, inp, resid):
            """Backward of the query / key / value Linears that share the input ``inp``: returns d(inp) + resid."""
            for j, nm in enumerate(("query", "key", "value")):
                G[p + f".lin_{nm}.bias"] = _e((C,), dev)
                ops.colsum(dQKV[:, j * C:(j + 1) * C], G[p + f".lin_{nm}.bias"])
                G[p + f".lin_{nm}.weight"] = _e((C, C), dev)
            _wgrad([dQKV[:, :C], dQKV[:, C:2 * C], dQKV[:, 2 * C:]], [inp, inp, inp],
                   [G[p + ".lin_query.weight"], G[p + ".lin_key.weight"], G[p + ".lin_value.weight"]])
            d_in = _e(tuple(inp.shape), dev)
            _gemm([dQKV[:, :C], dQKV[:, C:2 * C], dQKV[:, 2 * C:]],
                     [P[p + ".lin_query.weight"], P[p + ".lin_key.weight"], P[p + ".lin_value.weight"]], d_in,
                     b_kstrided=True, segments=True, resid=resid)
            return d_in

        def conv_bwd(l, dy, de_acc=None):
            """Returns (dx, de) of att_layers[l]; ``de_acc`` (optional [E, C]) is added to de in the GEMM's epilogue."""
            p = f"att_layers.{l}"
            s = sv.pop(p)
            x_in, e_in, QKV, ea = s["x"], s["e"], s["QKV"], s["ea"]
            d_o, dres = softplus_bwd(p, s, dy, N, x_in)
            G[p + ".lin_concate.bias"] = _e((C,), dev)
            ops.colsum(d_o, G[p + ".lin_concate.bias"])
            G[p + ".lin_concate.weight"] = _e((C, C), dev)
            _wgrad([d_o], [s["aggr"]], [G[p + ".lin_concate.weight"]])
            daggr = _e((N, C), dev)
            _gemm(d_o, P[p + ".lin_concate.weight"], daggr, b_kstrided=True)
            dQKV = _e((N, 3 * C), dev)
            dpre, dW1k, dW1m = _Attention.backward(P, G, p, daggr, QKV[:, :C], ea, lay, E, training, s, dQKV[:, :C])
            W1k, W1m = P[p + ".key_update.0.weight"], P[p + ".lin_msg_update.0.weight"]
            # lin_edge: d(ea) = dpre @ W1[:, 2C:], then into e.  Nothing on the chain of atom gradients reads de before
            # the edge layer's backward (or the end), so this branch -- two edge-sized products -- runs on the
            # weight-gradient stream, which has the slack (round 3: main queue 34.7 of 35.4 ms busy, second queue 19.1)
            with _side_branch([dpre, e_in, de_acc]) as sb:
                dea = _e((E, C), dev)
                tiles = ops.gemm_tiles_m(E)
                cs = _parts(tiles * C, dev)
                _gemm([dpre[:, :C], dpre[:, C:]], [W1k[:, 2 * C:], W1m[:, 2 * C:]], dea, b_kstrided=True, segments=True,
                         colsum=cs)
                G[p + ".lin_edge.bias"] = _e((C,), dev)
                ops.colsum_finalize(cs, tiles, G[p + ".lin_edge.bias"])
                G[p + ".lin_edge.weight"] = _e((C, C), dev)
                _wgrad_now([dea], [e_in], [G[p + ".lin_edge.weight"]])
                de = _e((E, C), dev)
                _gemm(dea, P[p + ".lin_edge.weight"], de, b_kstrided=True, resid=de_acc)
                sb.keep(de, G[p + ".lin_edge.bias"], G[p + ".lin_edge.weight"])
            # node terms: reduce dpre over incoming (target) / outgoing (source) edges
            dKPi, dKPj = _e((N, 2 * C), dev), _e((N, 2 * C), dev)
            ops.segment_sum(dpre, lay.rowptr, None, dKPi)
            ops.segment_sum(dpre, lay.colptr, lay.perm, dKPj)
            k, v = QKV[:, C:2 * C], QKV[:, 2 * C:]
            _wgrad([dKPi[:, :C], dKPi[:, C:], dKPj[:, :C], dKPj[:, C:]], [k, v, k, v],
                   [dW1k[:, :C], dW1m[:, :C], dW1k[:, C:2 * C], dW1m[:, C:2 * C]])
            _gemm([dKPi[:, :C], dKPj[:, :C]], [W1k[:, :C], W1k[:, C:2 * C]], dQKV[:, C:2 * C], b_kstrided=True,
                     segments=True)
            _gemm([dKPi[:, C:], dKPj[:, C:]], [W1m[:, :C], W1m[:, C:2 * C]], dQKV[:, 2 * C:], b_kstrided=True,
                     segments=True)
            dx_in = linear3_bwd(p, dQKV, x_in, dres)
            return dx_in, de

        def conv_edge_bwd(dy):
            """Returns (de, dNLt [Bg*3, C], dNA [3E, C]) of the edge update layer."""
            p = "edge_update_layer"
            s = sv.pop(p)
            e_in, QKV, KY, VY, exy = s["e"], s["QKV"], s["KY"], s["VY"], s["exy"]
            seg3 = sv["seg3"]
            d_o, dres = softplus_bwd(p, s, dy, E, e_in)
            G[p + ".lin_concate.bias"] = _e((C,), dev)
            tmpb = _e((1, C), dev)
            ops.colsum(d_o, tmpb.view(C))
            ops.eltwise(3, tmpb, None, G[p + ".lin_concate.bias"].view(1, C), 3.0)
            G[p + ".lin_concate.weight"] = _e((C, C), dev)
            _wgrad([d_o], [s["aggr"]], [G[p + ".lin_concate.weight"]])
            daggr = _e((E, C), dev)
            _gemm(d_o, P[p + ".lin_concate.weight"], daggr, b_kstrided=True)
            dQKV = _e((E, 3 * C), dev)
            dpre, dW1k, dW1m = _Attention.backward(P, G, p, daggr, QKV[:, :C], exy, seg3, 3 * E, training, s,
                                                   dQKV[:, :C])
            W1k, W1m = P[p + ".key_update.0.weight"], P[p + ".lin_msg_update.0.weight"]
            # angle branch: d(exy) -> lin_edge (no bias) -> dNA; only the RBF backward at the very end reads dNA, so the
            # two 3E-row products run on the weight-gradient stream
            with _side_branch([dpre, sv["NA"]]) as sb:
                dexy = _e((3 * E, C), dev)
                _gemm([dpre[:, :C], dpre[:, C:]], [W1k[:, 2 * C:], W1m[:, 2 * C:]], dexy, b_kstrided=True, segments=True)
                G[p + ".lin_edge.weight"] = _e((C, C), dev)
                _wgrad_now([dexy], [sv["NA"]], [G[p + ".lin_edge.weight"]])
                dNA = _e((3 * E, C), dev)
                _gemm(dexy, P[p + ".lin_edge.weight"], dNA, b_kstrided=True)
                sb.keep(dNA, G[p + ".lin_edge.weight"])
            # per-edge term (sum over the three lattice vectors) and per-(crystal, lattice vector) term
            dKa = _e((E, 2 * C), dev)
            ops.segment_sum(dpre, seg3.rowptr, None, dKa)
            dKYb = _e((Bg * 3, 2 * C), dev)
            dpre6, dKYb6 = dpre.view(E, 6 * C), dKYb.view(Bg, 6 * C)
            for i in range(3):
                ops.segment_sum(dpre6[:, i * 2 * C:(i + 1) * 2 * C], sv["gedge_ptr"], None,
                                dKYb6[:, i * 2 * C:(i + 1) * 2 * C])
            kx, vx = QKV[:, C:2 * C], QKV[:, 2 * C:]
            KYf, VYf = KY.view(Bg * 3, C), VY.view(Bg * 3, C)
            _wgrad([dKa[:, :C], dKa[:, C:]], [kx, vx], [dW1k[:, :C], dW1m[:, :C]])
            _wgrad([dKYb[:, :C], dKYb[:, C:]], [KYf, VYf], [dW1k[:, C:2 * C], dW1m[:, C:2 * C]])
            _gemm(dKa[:, :C], W1k[:, :C], dQKV[:, C:2 * C], b_kstrided=True)
            _gemm(dKa[:, C:], W1m[:, :C], dQKV[:, 2 * C:], b_kstrided=True)
            dKY, dVY = _e((Bg, 3 * C), dev), _e((Bg, 3 * C), dev)
            _gemm(dKYb[:, :C], W1k[:, C:2 * C], dKY.view(Bg * 3, C), b_kstrided=True)
            _gemm(dKYb[:, C:], W1m[:, C:2 * C], dVY.view(Bg * 3, C), b_kstrided=True)
            # lin_key_e{i} / lin_value_e{i} on the lattice-length features
            NL3 = sv["NLt"].view(Bg, 3 * C)
            dNL3 = _e((Bg, 3 * C), dev)
            for i in range(3):
                sl = slice(i * C, (i + 1) * C)
                for dT, kind in ((dKY, "key"), (dVY, "value")):
                    nm = p + f".lin_{kind}_e{i + 1}"
                    G[nm + ".bias"] = _e((C,), dev)
                    ops.colsum(dT[:, sl], G[nm + ".bias"])
                    G[nm + ".weight"] = _e((C, C), dev)
                    _wgrad([dT[:, sl]], [NL3[:, sl]], [G[nm + ".weight"]])
                _gemm([dKY[:, sl], dVY[:, sl]], [P[p + f".lin_key_e{i + 1}.weight"], P[p + f".lin_value_e{i + 1}.weight"]],
                         dNL3[:, sl], b_kstrided=True, segments=True)
            de = linear3_bwd(p, dQKV, e_in, dres)
            return de, dNL3.view(Bg * 3, C), dNA

        def lin_bwd(wname, dY, X, d_in=None, resid=None):
            """Backward of Y = X W^T + b: bias / weight gradients into G, returns dX (+ resid) if ``d_in`` is given."""
            W = P[wname + ".weight"]
            G[wname + ".bias"] = _e((W.shape[0],), dev)
            ops.colsum(dY, G[wname + ".bias"])
            G[wname + ".weight"] = _e(tuple(W.shape), dev)
            _wgrad([dY], [X], [G[wname + ".weight"]])
            if d_in is not None:
                _gemm(dY, W, d_in, b_kstrided=True, resid=resid)
            return d_in

        def equi_bwd(dy):
            """Returns (dx, de) of equi_update."""
            p = "equi_update"
            s = sv.pop(p)
            ns = ops.EQUI_NS
            x_in, e_in, cdir = s["x"], s["e"], s["cdir"]
            dx = lin_bwd(p + ".skip_linear", dy, x_in, _e((N, C), dev))
            dy2pre = _e((N, C), dev)
            ops.eltwise(1, dy, s["y2pre"], dy2pre)
            dy1 = lin_bwd(p + ".node_linear_2", dy2pre, s["y1"], _e((N, ns), dev))
            # y1 = softplus(bn(o2)): the shared two-pass BatchNorm backward with a zero residual
            np_ = ops.segment_nparts(N)
            pa, pb = _parts(np_ * ns, dev), _parts(np_ * ns, dev)
            ops.softplus_update_bwd_stats(s["o2"], s["zero"], dy1, s["mr"], P[p + ".bn.weight"], P[p + ".bn.bias"], pa, pb)
            sums = _e((2 * ns,), dev)
            ops.colsum_finalize([pa, pb], np_, [sums[:ns], sums[ns:]])
            G[p + ".bn.bias"], G[p + ".bn.weight"] = sums[:ns], sums[ns:]
            do2, dres = _e((N, ns), dev), _e((N, ns), dev)
            ops.softplus_update_bwd_apply(s["o2"], s["zero"], dy1, s["mr"], P[p + ".bn.weight"], P[p + ".bn.bias"], sums,
                                          training, do2, None, dres)

            def edge_mlp_bwd(li, dw):
                q = f"{p}.nlayer_{li}"
                dhact = lin_bwd(q + ".fc.2", dw, s[f"hact{li}"], _e((E, C), dev))
                dhpre = _e((E, C), dev)
                ops.eltwise(1, dhact, s[f"hpre{li}"], dhpre)
                return lin_bwd(q + ".fc.0", dhpre, e_in, _e((E, C), dev))

            dw2, dhe = _e((E, ops.EQUI_NW), dev), _e((E, ops.EQUI_H1), dev)
            ops.equi_tp2_bwd(s["h1"], s["w2"], cdir, lay, do2, dw2, dhe)
            dh1 = _e((N, ops.EQUI_H1), dev)
            ops.segment_sum(dhe, lay.rowptr, None, dh1)
            de2 = edge_mlp_bwd(2, dw2)
            del dw2, dhe
            dw1, dxe = _e((E, ops.EQUI_NW), dev), _e((E, ns), dev)
            ops.equi_tp1_bwd(s["x0"], s["w1"], cdir, lay, dh1, dw1, dxe)
            dx0s, dx0 = _e((N, ns), dev), _e((N, ns), dev)
            ops.segment_sum(dxe, lay.rowptr, None, dx0s)
            ops.eltwise(2, dx0s, dh1[:, :ns], dx0)                  # + the residual pad(x0)
            de1 = edge_mlp_bwd(1, dw1)
            de = _e((E, C), dev)
            ops.eltwise(2, de1, de2, de)
            dx_tot = lin_bwd(p + ".node_linear", dx0, x_in, _e((N, C), dev), resid=dx)
            return dx_tot, de

        def add_e(a, b):
            if a is None:
                return b
            acc = _e((E, C), dev)
            ops.eltwise(2, a, b, acc)
            return acc

        if sv["equi_model"]:
            # ---- eComformer: att 2, att 1, equivariant update, att 0; the edge features are shared by all of them
            de_tot = None
            for l in (2, 1):
                dx, de_tot = conv_bwd(l, dx, de_tot)          # accumulated in the lin_edge backward's epilogue
            dx, de_q = equi_bwd(dx)
            _join_wgrads()                                    # de_tot was produced on the weight-gradient stream
            de_tot = add_e(de_tot, de_q)
            dx, de_tot = conv_bwd(0, dx, de_tot)
        else:
            # ---- layers in reverse: att 3, 2, 1 (all read the updated edge features), edge layer, att 0
            de_new = None
            for l in (3, 2, 1):
                dx, de_new = conv_bwd(l, dx, de_new)          # accumulated in the lin_edge backward's epilogue
            _join_wgrads()                                    # de_new was produced on the weight-gradient stream
            de_old, dNLt, dNA = conv_edge_bwd(de_new)
            dx, de_tot = conv_bwd(0, dx, de_old)

        # ---- RBF branches: out = softplus(pre), pre = rbf @ W^T + b ; rbf.1 is shared by the distance and the
        #      lattice-length features, so its gradients add up
        def rbf_bwd(tag, dout):
            r, pre = sv[tag]
            dpre = _e(tuple(pre.shape), dev)
            ops.eltwise(1, dout, pre, dpre)
            gw, gb = _e((C, C), dev), _e((C,), dev)
            _wgrad([dpre], [r], [gw])
            ops.colsum(dpre, gb)
            return gw, gb

        _join_wgrads()                                        # de_tot / dNA come from the weight-gradient stream
        gw1, gb1 = rbf_bwd("rbf_e", de_tot)
        if sv["equi_model"]:
            G["rbf.1.weight"], G["rbf.1.bias"] = gw1, gb1
        else:
            gw2, gb2 = rbf_bwd("rbf_nl", dNLt)
            _join_wgrads()                                   # gw1 / gw2 come from the weight-gradient stream
            G["rbf.1.weight"], G["rbf.1.bias"] = _e((C, C), dev), _e((C,), dev)
            ops.eltwise(2, gw1, gw2, G["rbf.1.weight"])
            ops.eltwise(2, gb1.view(1, C), gb2.view(1, C), G["rbf.1.bias"].view(1, C))
            G["rbf_angle.1.weight"], G["rbf_angle.1.bias"] = rbf_bwd("rbf_na", dNA)

        # ---- atom embedding and temperature projection
        pw, pb = _parts(nparts_n * C, dev), _parts(nparts_n * C, dev)
        ops.node_embed_bwd(sv["gid"], sv["T"], dx, pw, pb)
        gw, gb = _e((C,), dev), _e((C,), dev)
        ops.colsum_finalize([pw, pb], nparts_n, [gw, gb])
        G["temperature_proj_atom.weight"], G["temperature_proj_atom.bias"] = gw.view(C, 1), gb
        zperm, zptr, _ = ops.sort_by_key(sv["z"], N_ATOM_TYPES)
        G["embedding.weight"] = _e((N_ATOM_TYPES, C), dev)
        ops.segment_sum_long(dx, zptr, zperm, N, G["embedding.weight"])
        _join_wgrads()          # autograd accumulates the gradients on this stream
        _KEEP.clear()           # the streams are joined: what the second stream used may go back to the allocator
        sink = getattr(model, "_flat_grad", None)
        if sink is not None:
            # the optimiser's flat gradient buffer: one concatenation + one add instead of ~130 per-parameter adds
            flat = torch.cat([(G[n].reshape(-1) if G.get(n) is not None else
                               torch.zeros(P[n].numel(), dtype=torch.float32, device=dev)) for n in model._param_names])
            if flat.numel() == sink.numel():
                sink.add_(flat)
                return (None, None, None) + (None,) * len(model._param_names)
        return (None, None, None) + tuple(G.get(n) for n in model._param_names)


def _fill_icf_params(dst: "_l.IcfParams", T: Dict[str, torch.Tensor]) -> None:
    """Point a CartnetIcfParams struct at the tensors of a reference-layout name -> tensor mapping."""
    for field, key in _l.ICF_TOP_KEYS.items():
        setattr(dst, field, T[key].data_ptr())
    for l in range(5):
        conv = dst.att[l] if l < 4 else dst.edge
        pre = f"att_layers.{l}." if l < 4 else "edge_update_layer."
        for field, key in _l.ICF_CONV_KEYS.items():
            t = T.get(pre + key)
            setattr(conv, field, t.data_ptr() if t is not None else None)       # the edge layer's lin_edge has no bias
        if l == 4:
            for i in range(3):
                conv.key_e_w[i] = T[pre + f"lin_key_e{i + 1}.weight"].data_ptr()
                conv.key_e_b[i] = T[pre + f"lin_key_e{i + 1}.bias"].data_ptr()
                conv.value_e_w[i] = T[pre + f"lin_value_e{i + 1}.weight"].data_ptr()
                conv.value_e_b[i] = T[pre + f"lin_value_e{i + 1}.bias"].data_ptr()


class _IcfNativeFunction(torch.autograd.Function):
    """iComformer forward / backward as ONE call into libcartnet_hip.so each (cartnet_icomformer_forward / _backward,
    csrc/icomformer.hip): the sequence `_IComformerFunction` issues launch by launch from Python (still the eComformer
    path), in C++ over one workspace.  ``params`` follow ``model._param_names``."""

    @staticmethod
    def forward(ctx, model: "iComformer", batch, training: bool, *params):
        lib = _l.load()
        P: Dict[str, torch.Tensor] = dict(zip(model._param_names, params))
        B: Dict[str, torch.Tensor] = dict(model.named_buffers())
        need_grad = bool(getattr(model, "_grad_mode", True)) and any(ctx.needs_input_grad)
        C_ = model.dim_in
        dev = params[0].device
        z = batch.x
        if not (torch.is_tensor(z) and z.dtype == torch.int64 and z.dim() == 1):
            raise ValueError("batch.x must hold int64 atomic numbers [N]")
        N, E, Bg = int(z.shape[0]), int(batch.edge_index.shape[1]), int(batch.num_graphs)
        M = int(batch.y.shape[0])

        def dt(t, dtype, numel, name):
            if not (torch.is_tensor(t) and t.dtype == dtype and t.numel() == numel and t.device == dev):
                raise ValueError(f"batch.{name}: expected {dtype} with {numel} elements on {dev}")
            return t.contiguous()
        keep = [dt(z, torch.int64, N, "x"), dt(batch.batch, torch.int64, N, "batch"),
                dt(batch.ptr, torch.int64, Bg + 1, "ptr"), dt(batch.edge_index, torch.int64, 2 * E, "edge_index"),
                dt(batch.cart_dist, torch.float32, E, "cart_dist"), dt(batch.cart_dir, torch.float32, 3 * E, "cart_dir"),
                dt(batch.temperature, torch.float32, Bg, "temperature"), dt(batch.non_H_mask, torch.bool, N, "non_H_mask"),
                dt(batch.cell, torch.float32, 9 * Bg, "cell")]
        bd = _l.BatchDesc()
        (bd.z, bd.batch, bd.graph_ptr, bd.edge_index, bd.cart_dist, bd.cart_dir, bd.temperature, bd.non_h_mask) = \
            (t.data_ptr() for t in keep[:8])
        bd.N, bd.Bg, bd.M, bd.E = N, Bg, M, E
        for n, t in P.items():
            if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
                raise ValueError(f"parameter {n} must be a contiguous fp32 CUDA tensor")
        md = _l.IcfModel()
        md.C, md.n_types, md.gemm_precision = C_, N_ATOM_TYPES, int(model.gemm_precision)
        md.bn_group_size = int(model.bn_group_size)
        md.gamma_rbf, md.gamma_angle = float(model.rbf[0].gamma), float(model.rbf_angle[0].gamma)
        md.bn_eps, md.bn_momentum = BN_EPS, BN_MOMENTUM
        md.rbf_centers, md.rbf_angle_centers = B["rbf.0.centers"].data_ptr(), B["rbf_angle.0.centers"].data_ptr()
        _fill_icf_params(md.p, P)
        for l in range(5):
            pre = f"att_layers.{l}." if l < 4 else "edge_update_layer."
            for which, dst in (("bn", md.att_bn[l] if l < 4 else md.edge_bn),
                               ("bn_att", md.att_bn_att[l] if l < 4 else md.edge_bn_att)):
                dst.mean = B[pre + which + ".running_mean"].data_ptr()
                dst.var = B[pre + which + ".running_var"].data_ptr()
                dst.nbt = B[pre + which + ".num_batches_tracked"].data_ptr()
        nbytes = int(lib.cartnet_icomformer_workspace_bytes(C.byref(md), N, E, Bg, M))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        pred = torch.empty((M, 3, 3), dtype=torch.float32, device=dev)
        x_out = torch.empty((N, C_), dtype=torch.float32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        aux = model._aux_stream_ptr(dev)
        _l.check(lib.cartnet_icomformer_forward(C.byref(md), C.byref(bd), keep[8].data_ptr(), ws.data_ptr(), nbytes,
                                                int(training), pred.data_ptr(), x_out.data_ptr(), status.data_ptr(),
                                                _l.stream_ptr(), aux), "cartnet_icomformer_forward")
        if model.validate_graph:
            ops.raise_on_graph_status(int(status.item()))
        ctx.saved = (model, md, bd, ws, nbytes, keep, x_out, bool(training)) if need_grad else None
        ctx.mark_non_differentiable(x_out)
        return pred, x_out

    @staticmethod
    def backward(ctx, dpred, _dx_unused):
        if ctx.saved is None:
            raise RuntimeError("iComformer backward called without saved state")
        model, md, bd, ws, nbytes, keep, x_out, training = ctx.saved
        ctx.saved = None
        lib = _l.load()
        dpred = dpred.contiguous()
        dev = dpred.device
        cache = model.__dict__.get("_grad_cache")
        if cache is None or cache[0].flat.device != dev:
            from .model import _GradBuffer
            G = _GradBuffer(model, dev)
            gd = _l.IcfParams()
            _fill_icf_params(gd, G)
            cache = (G, gd)
            model.__dict__["_grad_cache"] = cache
        G, gd = cache
        # the staging buffer is reused every step: the slots no kernel writes (lemb / lin_edge_len) must stay zero and a
        # launch skipped for an empty batch must not leave last step's values behind -- one memset against a 29 ms step
        G.flat.zero_()
        _l.check(lib.cartnet_icomformer_backward(C.byref(md), C.byref(bd), ws.data_ptr(), nbytes, int(training),
                                                 dpred.data_ptr(), x_out.data_ptr(), C.byref(gd), _l.stream_ptr(),
                                                 model._aux_stream_ptr(dev)), "cartnet_icomformer_backward")
        sink = getattr(model, "_flat_grad", None)
        if sink is not None and sink.numel() == G.flat.numel():
            sink.add_(G.flat)
            return (None, None, None) + (None,) * len(model._param_names)
        # (lemb / lin_edge_len: declared by the reference, never used -- no gradient there either)
        return (None, None, None) + tuple(None if (".lemb." in n or ".lin_edge_len." in n) else G[n].clone()
                                          for n in model._param_names)


class iComformer(nn.Module):
    """iComformer (reference: models/comformer.py:75-132) on the gfx950 kernels.  ``forward(data)`` returns
    ``(pred [M,3,3], data.y)`` and, like the reference, replaces ``data.x`` with the final atom features."""

    def __init__(self, dim_in: int):
        super().__init__()
        if dim_in % 8 != 0 or dim_in // 2 > 512:
            raise ValueError("dim_in must be a multiple of 8 and at most 1024")
        c = dim_in
        self.dim_in = c
        self.embedding = nn.Embedding(N_ATOM_TYPES, c)
        self.temperature_proj_atom = nn.Linear(1, c, bias=True)
        self.rbf = nn.Sequential(_RBF(-4.0, 0.0, c), nn.Linear(c, c), nn.Softplus())
        self.rbf_angle = nn.Sequential(_RBF(-1.0, 1.0, c), nn.Linear(c, c), nn.Softplus())
        self.att_layers = nn.ModuleList([ComformerConv(c) for _ in range(4)])
        self.edge_update_layer = ComformerConv_edge(c)
        self.cholesky = Cholesky_head(c)
        self.validate_graph = False
        self.gemm_precision = 0         # 0: fp32 MFMA.  1: bf16x3 split-operand MFMA.  2: plain bf16 operands
        self.overlap_weight_gradients = True   # weight-gradient GEMMs on a second stream during backward
        self._flat_grad = None          # set by FlatAdam: backward adds all gradients there in one pass
        self._param_names = [n for n, _ in self.named_parameters()]
        self._param_shapes = {n: tuple(p.shape) for n, p in self.named_parameters()}
        self._aux = None
        # True (default): ONE C-ABI call per direction (csrc/icomformer.hip).  False: the same kernels sequenced from
        # Python (`_IComformerFunction`, what eComformer uses) -- kept as the cross-check of the C++ sequence
        self.native_sequence = True
        # > 0: consecutive crystals of a batch form BatchNorm groups of this size in training mode (CartnetIcfModel.
        # bn_group_size): the reference's recipe --batch 4 --batch_accumulation 16 (scripts/train_icomformer_adp.sh:3) as
        # ONE pass over 64 crystals with the statistics, the running-statistics updates and (train.grouped_loss) the loss
        # taken per micro-batch.  The C++ sequence only.
        self.bn_group_size = 0

    def _aux_stream_ptr(self, dev):
        if not getattr(self, "overlap_weight_gradients", True):
            return None
        if self._aux is None or self._aux.device != dev:
            self._aux = torch.cuda.Stream(device=dev)
        return self._aux.cuda_stream

    def forward(self, data):
        if int(self.bn_group_size) > 0 and not self.native_sequence:
            raise ValueError("bn_group_size > 0 needs native_sequence = True: the Python-sequenced path has one BatchNorm group")
        params = [p for _, p in self.named_parameters()]
        if not params[0].is_cuda:
            raise RuntimeError("cartnet_amd.iComformer runs only on an AMD GPU (HIP kernels); there is no CPU fallback")
        self._grad_mode = torch.is_grad_enabled()       # read by the Function's forward (grad mode is off in there)
        fn = _IcfNativeFunction if self.native_sequence else _IComformerFunction
        pred, x = fn.apply(self, data, self.training, *params)
        data.x = x
        return pred, data.y


class _EdgeMLP(nn.Module):
    """TensorProductConvLayer (comformer_conv.py:197-213): only its edge MLP ``fc`` holds parameters (the e3nn tensor
    product is weightless with shared_weights=False)."""

    def __init__(self, c: int):
        super().__init__()
        self.fc = nn.Sequential(nn.Linear(c, c), nn.Softplus(), nn.Linear(c, ops.EQUI_NW))


class ComformerConvEqui(nn.Module):
    """Parameter container of the reference's ComformerConvEqui (comformer_conv.py:226-264; ns = 64, nv = 8)."""

    def __init__(self, c: int):
        super().__init__()
        self.node_linear = nn.Linear(c, ops.EQUI_NS)
        self.skip_linear = nn.Linear(c, c)
        self.nlayer_1 = _EdgeMLP(c)
        self.nlayer_2 = _EdgeMLP(c)
        self.bn = nn.BatchNorm1d(ops.EQUI_NS)
        self.node_linear_2 = nn.Linear(ops.EQUI_NS, c)


class eComformer(nn.Module):
    """eComformer (reference: models/comformer.py:25-70) on the gfx950 kernels: three attention layers around the
    equivariant update.  The reference builds that update on e3nn, which is not available here; it is restated from
    e3nn's published algorithm (csrc/equi_ops.hip, oracle/ecomformer_ref.py) and its parity with e3nn is unpinned."""

    kind = "e"

    def __init__(self, dim_in: int):
        super().__init__()
        if dim_in % 8 != 0 or dim_in // 2 > 512:
            raise ValueError("dim_in must be a multiple of 8 and at most 1024")
        c = dim_in
        self.dim_in = c
        self.embedding = nn.Embedding(N_ATOM_TYPES, c)
        self.temperature_proj_atom = nn.Linear(1, c, bias=True)
        self.rbf = nn.Sequential(_RBF(-4.0, 0.0, c), nn.Linear(c, c), nn.Softplus())
        self.att_layers = nn.ModuleList([ComformerConv(c) for _ in range(3)])
        self.equi_update = ComformerConvEqui(c)
        self.cholesky = Cholesky_head(c)
        self._flat_grad = None          # set by FlatAdam: backward adds all gradients there in one pass
        self.validate_graph = False
        self.gemm_precision = 0
        self.overlap_weight_gradients = True
        self._param_names = [n for n, _ in self.named_parameters()]

    def forward(self, data):
        params = [p for _, p in self.named_parameters()]
        if not params[0].is_cuda:
            raise RuntimeError("cartnet_amd.eComformer runs only on an AMD GPU (HIP kernels); there is no CPU fallback")
        self._grad_mode = torch.is_grad_enabled()       # read by _IComformerFunction.forward (grad mode is off in there)
        pred, x = _IComformerFunction.apply(self, data, self.training, *params)
        data.x = x
        return pred, data.y


def make_ecomformer_state_dict(dim_in: int, seed: int = 0) -> Dict[str, torch.Tensor]:
    """Deterministic state_dict (CPU) for the eComformer tests; BatchNorm affine / running statistics randomised."""
    torch.manual_seed(seed)
    m = eComformer(dim_in)
    g = torch.Generator().manual_seed(seed + 1)
    sd = m.state_dict()
    for k, v in sd.items():
        if k.endswith("running_mean"):
            v.copy_(0.1 * torch.randn(v.shape, generator=g))
        elif k.endswith("running_var"):
            v.copy_(0.5 + torch.rand(v.shape, generator=g))
        elif (".bn." in k or ".bn_att." in k) and k.endswith(".weight"):
            v.copy_(1.0 + 0.2 * torch.randn(v.shape, generator=g))
        elif (".bn." in k or ".bn_att." in k) and k.endswith(".bias"):
            v.copy_(0.2 * torch.randn(v.shape, generator=g))
    return {k: v.clone() for k, v in sd.items()}


def make_icomformer_state_dict(dim_in: int, seed: int = 0) -> Dict[str, torch.Tensor]:
    """Deterministic reference-shaped state_dict (CPU) for the parity fixtures; BatchNorm affine / running statistics
    are randomised so that eval mode is exercised."""
    torch.manual_seed(seed)
    m = iComformer(dim_in)
    g = torch.Generator().manual_seed(seed + 1)
    sd = m.state_dict()
    for k, v in sd.items():
        if k.endswith("running_mean"):
            v.copy_(0.1 * torch.randn(v.shape, generator=g))
        elif k.endswith("running_var"):
            v.copy_(0.5 + torch.rand(v.shape, generator=g))
        elif (".bn." in k or ".bn_att." in k) and k.endswith(".weight"):
            v.copy_(1.0 + 0.2 * torch.randn(v.shape, generator=g))
        elif (".bn." in k or ".bn_att." in k) and k.endswith(".bias"):
            v.copy_(0.2 * torch.randn(v.shape, generator=g))
    return {k: v.clone() for k, v in sd.items()}
