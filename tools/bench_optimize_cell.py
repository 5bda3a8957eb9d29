"""Time DeviceShard.with_optimized_cell (csrc/lattice_ops.hip) on a resident shard against the same transform written
with torch device ops on the shard's own tensors: the selection through a batched ``sort`` of the 124 candidates, the
rotation as ``repeat_interleave`` of R over the edges (and target rows) and ``bmm``.

The two are taken alternately (HIP, torch, HIP, torch, ...) in one process, each call between two HIP events, after a
warm-up of both; the medians, the bytes the transform has to move and the rates they give are printed as one JSON line per
shard size and torch form of the rotation (``bmm`` -- up to BMM_MAX_BATCH edges, see there -- and the same products as
broadcast multiplies).  Both times include
everything a caller waits for: the allocations, the launches and the device-to-host read of the status word (the torch
form reads back whether a crystal was degenerate as well).

Every crystal's cell is first re-described by one of five unimodular matrices in turn (the lattice is the same, the graph
is unchanged): the synthetic cells are close to reduced already, and only a handful would change basis otherwise.

usage: python tools/bench_optimize_cell.py [--crystals 512 8192] [--atoms 194] [--rounds 9]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

UNIMODULAR = np.array([[[1, 1, 0], [0, 1, 0], [0, 0, 1]],            # a -> a + b
                       [[1, 0, 0], [0, 1, 0], [1, 0, 1]],            # c -> c + a
                       [[0, 1, 0], [0, 0, 1], [1, 0, 0]],            # cyclic permutation
                       [[-1, 0, 0], [0, -1, 0], [0, 0, 1]],          # two axes negated
                       [[1, 0, 0], [1, 1, 0], [0, 1, 1]]], dtype=np.float32)
HALF_PI = 1.5707963705062866                                         # fp32(pi / 2)
# torch.bmm with one batch per edge ran at 1.4 M edges and ended in an illegal memory access at 22.8 M (torch 2.10 on ROCm 7.2,
# inside the batched product, between two synchronisations of the torch form): the literal form is only taken up to here
BMM_MAX_BATCH = 2 ** 21


def _first(mask: torch.Tensor) -> torch.Tensor:
    """Index of the first True per row; the row length where there is none."""
    n = mask.shape[1]
    pos = torch.arange(n, device=mask.device).expand_as(mask)
    return torch.where(mask, pos, torch.full_like(pos, n)).min(dim=1).values


def torch_with_optimized_cell(shard, rotate: str = "bmm") -> dict:
    """dataset/datasetADP.py:75-80 with dataset/utils.py:366-452 for every crystal of a resident shard at once, in torch
    device ops: the arrays ``DeviceShard.with_optimized_cell`` replaces or adds.  ``rotate``: "bmm" multiplies every edge
    direction (and target) by its crystal's R with ``torch.bmm``, the literal batched form of the reference's ``@``;
    "broadcast" writes the same 3x3 products as broadcast multiplies and sums, which torch runs as a few element-wise
    kernels instead of E tiny matrix products."""
    t, G, dev = shard.t, shard.num_graphs, shard.device
    if rotate == "bmm" and int(shard.edge_ptr[-1]) > BMM_MAX_BATCH:
        raise ValueError(f"the bmm form is limited to {BMM_MAX_BATCH} edges (see BMM_MAX_BATCH); use rotate='broadcast'")
    from cartnet_amd.data import _LATTICE_COEFFS
    coef_i = _LATTICE_COEFFS.to(dev)
    coef = coef_i.to(torch.float32)
    cell = t["cell"].view(G, 3, 3)
    cand = (coef[None, :, 0:1] * cell[:, None, 0] + coef[None, :, 1:2] * cell[:, None, 1]) + coef[None, :, 2:3] * cell[:, None, 2]
    order = torch.sort(cand.norm(dim=2), dim=1, stable=True).indices
    v = torch.gather(cand, 1, order.unsqueeze(2).expand(-1, -1, 3))
    rows = torch.arange(G, device=dev)
    pos = torch.arange(v.shape[1], device=dev)
    v1 = v[:, 0]
    n1 = v1.norm(dim=1)

    def sign(w):
        cos = (v1 * w).sum(1) / (n1 * w.norm(dim=1))
        return torch.where(torch.acos(cos).abs() > HALF_PI, -1.0, 1.0)
    ok2 = ~(torch.linalg.cross(v1.unsqueeze(1).expand_as(v), v).norm(dim=2) <= 1e-3) & (pos > 0)
    r2 = _first(ok2)
    bad = r2 >= v.shape[1]
    r2c = r2.clamp(max=v.shape[1] - 1)
    s2 = sign(v[rows, r2c])
    v2 = v[rows, r2c] * s2.unsqueeze(1)
    n12 = torch.linalg.cross(v1, v2)
    ok3 = ~((n12.unsqueeze(1) * v).sum(2).abs() <= 1e-3) & (pos.unsqueeze(0) > r2.unsqueeze(1))
    r3 = _first(ok3)
    bad = bad | (r3 >= v.shape[1])
    r3c = r3.clamp(max=v.shape[1] - 1)
    s3 = sign(v[rows, r3c])
    v3 = v[rows, r3c] * s3.unsqueeze(1)
    h = torch.where((n12 * v3).sum(1) < 0, -1.0, 1.0)
    V = torch.stack((v1, v2, v3), dim=1) * h.view(G, 1, 1)
    sg = torch.stack((h, h * s2, h * s3), dim=1)
    picked = torch.stack((order[:, 0], order[rows, r2c], order[rows, r3c]), dim=1)
    basis = (coef_i[picked] * sg.to(torch.int64).unsqueeze(2)).to(torch.int8)
    x = V[:, 0] / V[:, 0].norm(dim=1, keepdim=True)
    p = V[:, 1] - (V[:, 1] * x).sum(1, keepdim=True) * x
    y = p / p.norm(dim=1, keepdim=True)
    R = torch.stack((x, y, torch.linalg.cross(x, y)), dim=1)
    if bool(bad.any()):                                                   # the read-back the HIP pass has as well
        raise ValueError(f"crystal {int(torch.nonzero(bad)[0])}: degenerate cell")
    out = {"cell": torch.bmm(V, R.transpose(1, 2)).reshape(G, 9), "rotation": R.reshape(G, 9), "basis": basis.reshape(G, 9)}
    edge_ptr = t["edge_ptr"]
    Re = torch.repeat_interleave(R, edge_ptr[1:] - edge_ptr[:-1], dim=0)
    if rotate == "bmm":
        out["cart_dir"] = torch.bmm(t["cart_dir"].unsqueeze(1), Re).squeeze(1)
    else:
        out["cart_dir"] = (t["cart_dir"].unsqueeze(2) * Re).sum(1)
    if shard.per_atom_target:
        y_ptr = t["y_ptr"]
        Ry = torch.repeat_interleave(R, y_ptr[1:] - y_ptr[:-1], dim=0)
        y3 = t["y"].view(-1, 3, 3)
        if rotate == "bmm":
            out["y"] = torch.bmm(torch.bmm(Ry.transpose(1, 2), y3), Ry).reshape(-1, 9)
        else:
            yr = (y3.unsqueeze(3) * Ry.unsqueeze(1)).sum(2)                                   # y R
            out["y"] = (Ry.unsqueeze(3) * yr.unsqueeze(2)).sum(1).reshape(-1, 9)              # R^T (y R)
    return out


def bytes_moved(shard) -> int:
    """What the transform has to read and write: 12 B in + 12 B out per edge, 36 B + 36 B per 3x3 target row, the cell in
    and cell / rotation / basis out per crystal, the offsets."""
    E, M, G = int(shard.edge_ptr[-1]), int(shard.y_ptr[-1]), shard.num_graphs
    return 24 * E + (72 * M if shard.per_atom_target else 0) + (36 + 36 + 36 + 9) * G + 2 * 8 * (G + 1)


def measure(shard, rounds: int = 9, warmup: int = 2, rotate: str = "bmm") -> dict:
    """Alternating timings (A B A B) of the HIP pass and the torch restatement on ``shard``; milliseconds."""
    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), r
    for _ in range(warmup):
        shard.with_optimized_cell()
        torch_with_optimized_cell(shard, rotate)
    torch.cuda.synchronize()
    hip, tor = [], []
    for _ in range(rounds):
        ms, _ = timed(shard.with_optimized_cell)
        hip.append(ms)
        ms, _ = timed(lambda: torch_with_optimized_cell(shard, rotate))
        tor.append(ms)
    nbytes = bytes_moved(shard)
    h, t = statistics.median(hip), statistics.median(tor)
    return {"torch_rotate": rotate, "crystals": shard.num_graphs, "edges": int(shard.edge_ptr[-1]),
            "target_rows": int(shard.y_ptr[-1]),
            "bytes_moved": nbytes, "hip_ms_median": round(h, 4), "torch_ms_median": round(t, 4),
            "hip_ms": [round(x, 4) for x in hip], "torch_ms": [round(x, 4) for x in tor],
            "hip_GBps": round(nbytes / h / 1e6, 1), "torch_GBps": round(nbytes / t / 1e6, 1)}


def redescribe(arrays: dict) -> dict:
    """The packed arrays with crystal g's cell replaced by UNIMODULAR[g % 5] @ cell (fp32): the same lattices."""
    out = dict(arrays)
    cell = np.asarray(arrays["cell"], dtype=np.float32).reshape(-1, 3, 3)
    u = UNIMODULAR[np.arange(cell.shape[0]) % len(UNIMODULAR)]
    out["cell"] = np.matmul(u, cell).astype(np.float32).reshape(-1, 9)
    return out


def large_shard(crystals: int = 512, atoms: int = 194, first: int = 5000):
    """``crystals`` synthetic crystals of ``atoms`` atoms, graphs built on the GPU (as tools/bench_no_hydrogens.py's
    ``large_shard``), cells re-described; returns (arrays, DeviceShard)."""
    from cartnet_amd.shard import DeviceShard, pack_with_gpu_graph
    from cartnet_amd.synthetic import make_geometry
    arrays = redescribe(pack_with_gpu_graph([make_geometry(first + g, atoms) for g in range(crystals)], 5.0, "cuda:0"))
    return arrays, DeviceShard(arrays, "cuda:0")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--crystals", type=int, nargs="+", default=[512, 8192])
    ap.add_argument("--atoms", type=int, default=194)
    ap.add_argument("--rounds", type=int, default=9)
    a = ap.parse_args()
    for n in a.crystals:
        _, sh = large_shard(n, a.atoms)
        for rotate in ("bmm", "broadcast") if int(sh.edge_ptr[-1]) <= BMM_MAX_BATCH else ("broadcast",):
            print(json.dumps(measure(sh, a.rounds, rotate=rotate)), flush=True)
        del sh
        torch.cuda.empty_cache()
