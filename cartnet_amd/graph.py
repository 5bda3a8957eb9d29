"""Periodic radius graph on the GPU: the step right before the hot path.

``radius_graph_csr(pos, cell, atom_ptr, radius, max_neighbors)`` drives the library's one pass (csrc/radius_graph.hip:
count, read the sizes, cap if some row is too long, fill) over the crystals of a batch or of a whole resident shard and
returns the graph in the shard's format.  ``radius_graph_pbc(pos, cell, ptr, radius, max_neighbors)`` is the same pass
with the edges as a PyG ``edge_index`` in the reference's order (reference: dataset/utils.py:57-237 as called by
dataset/figshare_dataset.py:65-68), so the result can be fed straight to ``CartNet.forward`` / ``iComformer.forward``;
integers match the reference bit for bit, distances / directions to fp32 rounding (tests/test_gpu_radius_graph.py).
``max_neighbors`` is the reference's neighbour cap (dataset/utils.py:240-360; 25 for iComformer, off for CartNet --
main.py:141,176)."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import lib as _l


DEGENERACY_TOLERANCE = 0.01      # dataset/utils.py:245, in squared-distance units


def radius_graph_csr(pos: torch.Tensor, cell: torch.Tensor, atom_ptr: torch.Tensor, radius: float = 5.0,
                     max_neighbors: Optional[int] = None):
    """pos [N,3] fp32, cell [G,9] or [G,3,3] fp32 (rows = lattice vectors), atom_ptr [G+1] int64 atom offsets: contiguous
    tensors on one GPU, a batch's or a whole shard's.  ``max_neighbors`` None or <= 0: no cap.
    ``radius`` goes to the library as a double: the cutoff is fp32(radius * radius) with the product taken in double, as
    dataset/utils.py:202 takes it (the fp32 product of the rounded radius is one ulp larger for e.g. 3.7 and 4.3).
    Returns device tensors (edge_ptr [G+1] int64, edge_src [E], edge_tgt [E] int32 atom indices inside the crystal,
    cart_dist [E], cart_dir [E,3]), edges in the reference's order.  The host reads two sizes and a status word; with a
    cap that some atom exceeds the only transient edge-sized array is the uncapped rows' d^2 (4 B per edge).  Raises
    ``ValueError`` if ``atom_ptr`` is not an ascending offset array from 0 to N."""
    lib = _l.load()
    dev, G, N = pos.device, int(atom_ptr.numel()) - 1, int(pos.shape[0])
    cap = int(max_neighbors) if max_neighbors is not None and int(max_neighbors) > 0 else 0
    with torch.cuda.device(dev):
        args = (pos.data_ptr(), cell.data_ptr(), atom_ptr.data_ptr(), G, N, float(radius))
        ws_bytes = int(lib.cartnet_shard_regraph_workspace_bytes(G, N, 0))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        totals = torch.empty(4, dtype=torch.int64, device=dev)
        _l.check(lib.cartnet_shard_regraph_count(*args, cap, ws.data_ptr(), ws_bytes, totals.data_ptr(),
                                                 _l.stream_ptr()), "cartnet_shard_regraph_count")
        e_all, _, over, status = totals.tolist()            # device-to-host copy 1: the uncapped size
        if status != 0:
            raise ValueError("atom_ptr does not cover all atoms: it is not an ascending offset array from 0 to N")
        E = e_all
        if over:                                             # some atom has more than `cap` neighbours
            d2 = torch.empty(e_all, dtype=torch.float32, device=dev)
            _l.check(lib.cartnet_shard_regraph_cap(*args, cap, DEGENERACY_TOLERANCE, e_all, ws.data_ptr(), ws_bytes,
                                                   d2.data_ptr(), totals.data_ptr(), _l.stream_ptr()),
                     "cartnet_shard_regraph_cap")
            E = int(totals[1].item())                        # device-to-host copy 2: the capped size
        edge_ptr = torch.empty(G + 1, dtype=torch.int64, device=dev)
        src = torch.empty(E, dtype=torch.int32, device=dev)
        tgt = torch.empty(E, dtype=torch.int32, device=dev)
        dist = torch.empty(E, dtype=torch.float32, device=dev)
        dirs = torch.empty((E, 3), dtype=torch.float32, device=dev)
        _l.check(lib.cartnet_shard_regraph_fill(*args, int(bool(over)), ws.data_ptr(), ws_bytes, E, edge_ptr.data_ptr(),
                                                src.data_ptr(), tgt.data_ptr(), dist.data_ptr(), dirs.data_ptr(),
                                                _l.stream_ptr()), "cartnet_shard_regraph_fill")
    return edge_ptr, src, tgt, dist, dirs


def radius_graph_pbc(pos: torch.Tensor, cell: torch.Tensor, ptr: torch.Tensor, radius: float = 5.0,
                     max_neighbors: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """pos [N,3] fp32, cell [Bg,3,3] fp32 (rows = lattice vectors), ptr [Bg+1] int64 atom offsets -- all on the GPU.
    ``max_neighbors`` None or <= 0: no cap (what figshare_dataset.py:18 maps -1 to).  ``radius``: see ``radius_graph_csr``.
    Returns (edge_index [2,E] int64 = (source, target), cart_dist [E], cart_dir [E,3])."""
    if not (pos.is_cuda and pos.dtype == torch.float32 and pos.dim() == 2 and pos.shape[1] == 3):
        raise ValueError("pos must be a CUDA fp32 tensor [N,3]")
    if not (cell.is_cuda and cell.dtype == torch.float32 and cell.dim() == 3 and tuple(cell.shape[1:]) == (3, 3)):
        raise ValueError("cell must be a CUDA fp32 tensor [Bg,3,3]")
    if not (ptr.is_cuda and ptr.dtype == torch.int64 and ptr.dim() == 1 and ptr.numel() == cell.shape[0] + 1):
        raise ValueError("ptr must be a CUDA int64 tensor [Bg+1]")
    ptr = ptr.contiguous()
    edge_ptr, src, tgt, dist, dirs = radius_graph_csr(pos.contiguous(), cell.contiguous(), ptr, radius, max_neighbors)
    # in-crystal ends -> the batch's atom indices: + ptr[g], g = the crystal of the edge (device ops, no host read)
    off = torch.repeat_interleave(ptr[:-1], edge_ptr[1:] - edge_ptr[:-1], output_size=src.numel())
    return torch.stack((src + off, tgt + off)), dist, dirs
