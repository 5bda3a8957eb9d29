"""Time DeviceShard.without_hydrogens (csrc/shard_ops.hip) on a resident shard against the same transform written
with torch device ops (boolean-mask indexing, cumsum) on the shard's own tensors.

The two are taken alternately (HIP, torch, HIP, torch, ...) in one process, each call between two HIP events, after a
warm-up of both; the medians, the bytes the transform has to move and the rates they give are printed as one JSON line.
Both times include everything a caller waits for: the allocations, the small launches, and the device-to-host read of
the new sizes (one in the HIP pass; the boolean-mask indexing of the torch form reads its sizes back as well).

usage: python tools/bench_no_hydrogens.py [--crystals 512] [--atoms 194] [--rounds 9]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch


def torch_without_hydrogens(shard) -> dict:
    """dataset/datasetADP.py:49-72 for every crystal of a resident shard at once, in torch device ops: the arrays
    ``DeviceShard.without_hydrogens`` replaces (the others are shared)."""
    t = shard.t
    G = shard.num_graphs
    z, atom_ptr, edge_ptr = t["z"], t["atom_ptr"], t["edge_ptr"]
    keep = z != 1
    incl = torch.cumsum(keep, 0)
    rank = incl - 1
    excl = torch.cat((incl.new_zeros(1), incl))
    atom_ptr_new = excl[atom_ptr]
    g_of_edge = torch.repeat_interleave(torch.arange(G, device=z.device), edge_ptr[1:] - edge_ptr[:-1])
    base = atom_ptr[g_of_edge]
    s, d = base + t["edge_src"], base + t["edge_tgt"]
    keep_e = keep[s] & keep[d]
    incl_e = torch.cumsum(keep_e, 0)
    new_base = atom_ptr_new[g_of_edge][keep_e]
    out = {"atom_ptr": atom_ptr_new, "edge_ptr": torch.cat((incl_e.new_zeros(1), incl_e))[edge_ptr], "z": z[keep],
           "edge_src": (rank[s[keep_e]] - new_base).to(torch.int32),
           "edge_tgt": (rank[d[keep_e]] - new_base).to(torch.int32),
           "cart_dist": t["cart_dist"][keep_e], "cart_dir": t["cart_dir"][keep_e]}
    if "pos" in t:
        out["pos"] = t["pos"][keep]
    if "non_h_mask" in t:
        out["non_h_mask"] = torch.ones_like(out["z"], dtype=torch.uint8)
    return out


def bytes_moved(shard, out) -> int:
    """What the transform has to read and write: 24 B per edge in, 24 B per kept edge out; z (+ pos, mask) of every
    atom in and of every kept atom out; the offsets."""
    N, E = int(shard.atom_ptr[-1]), int(shard.edge_ptr[-1])
    n, e = int(out.atom_ptr[-1]), int(out.edge_ptr[-1])
    per_atom = 4 + (12 if "pos" in shard.t else 0) + (1 if "non_h_mask" in shard.t else 0)
    return 24 * (E + e) + per_atom * (N + n) + 4 * 8 * (shard.num_graphs + 1)


def measure(shard, rounds: int = 9, warmup: int = 2) -> dict:
    """Alternating timings (A B A B) of the HIP pass and the torch restatement on ``shard``; milliseconds."""
    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), r
    for _ in range(warmup):
        shard.without_hydrogens()
        torch_without_hydrogens(shard)
    torch.cuda.synchronize()
    hip, tor, out = [], [], None
    for _ in range(rounds):
        ms, out = timed(shard.without_hydrogens)
        hip.append(ms)
        ms, _ = timed(lambda: torch_without_hydrogens(shard))
        tor.append(ms)
    nbytes = bytes_moved(shard, out)
    h, t = statistics.median(hip), statistics.median(tor)
    return {"atoms": int(shard.atom_ptr[-1]), "edges": int(shard.edge_ptr[-1]), "atoms_kept": int(out.atom_ptr[-1]),
            "edges_kept": int(out.edge_ptr[-1]), "bytes_moved": nbytes, "hip_ms_median": round(h, 4),
            "torch_ms_median": round(t, 4), "hip_ms": [round(x, 4) for x in hip], "torch_ms": [round(x, 4) for x in tor],
            "hip_GBps": round(nbytes / h / 1e6, 1), "torch_GBps": round(nbytes / t / 1e6, 1)}


def large_shard(crystals: int = 512, atoms: int = 194, first: int = 5000):
    """``crystals`` synthetic crystals of ``atoms`` atoms, graphs built on the GPU; returns (arrays, DeviceShard)."""
    from cartnet_amd.shard import DeviceShard, pack_with_gpu_graph
    from cartnet_amd.synthetic import make_geometry
    arrays = pack_with_gpu_graph([make_geometry(first + g, atoms) for g in range(crystals)], 5.0, "cuda:0")
    return arrays, DeviceShard(arrays, "cuda:0")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--crystals", type=int, default=512)
    ap.add_argument("--atoms", type=int, default=194)
    ap.add_argument("--rounds", type=int, default=9)
    a = ap.parse_args()
    _, sh = large_shard(a.crystals, a.atoms)
    print(json.dumps(measure(sh, a.rounds)))
