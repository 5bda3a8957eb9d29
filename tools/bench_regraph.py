"""Time the radius graph of a whole dataset split, three ways, on the ragged crystals of tools/bench_config4.py (20,283
crystals of 64-324 atoms, ~56 M edges at radius 5):

    regraph       ``DeviceShard.with_radius_graph(5.0)`` on the resident geometry
    regraph_cap   ``DeviceShard.with_radius_graph(5.0, 25)``
    from_lists    ``pack_with_gpu_graph`` on the Python ``Data`` lists (pack, upload, the same pass, every array copied
                  back to the host) followed by the upload of the packed arrays (``DeviceShard(arrays)``): the route from
                  Python lists to a resident shard with a graph

The three are taken alternately (A B C A B C ...) in one process after a warm-up round; each time is a host clock around
the call, ended by a device synchronise, so it holds everything a caller waits for (allocations, launches, the read-backs
of the sizes; for from_lists also the host concatenations and copies).  One JSON object goes to stdout and, with
``--out``, to a file.

usage: python tools/bench_regraph.py [--crystals 20283] [--rounds 5] [--cap 25] [--out profiles/exp_shard_regraph.json]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch

from cartnet_amd.shard import DeviceShard, pack, pack_with_gpu_graph
from cartnet_amd.synthetic import make_geometry


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--crystals", type=int, default=162270 // 8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--radius", type=float, default=5.0)
    ap.add_argument("--cap", type=int, default=25)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_regraph.py measures on the GPU; none found")
    dev = "cuda:0"
    geo = [make_geometry(30000 + i, None) for i in range(a.crystals)]          # the crystals of tools/bench_config4.py
    base = DeviceShard(pack(geo), dev)                                          # geometry only, resident

    runs = {"regraph": lambda: base.with_radius_graph(a.radius),
            "regraph_cap": lambda: base.with_radius_graph(a.radius, a.cap),
            "from_lists": lambda: DeviceShard(pack_with_gpu_graph(geo, a.radius, dev), dev)}
    warm = {k: fn() for k, fn in runs.items()}                                  # warm-up of all three
    edges, edges_cap = int(warm["regraph"].edge_ptr[-1]), int(warm["regraph_cap"].edge_ptr[-1])
    N, G = int(base.atom_ptr[-1]), base.num_graphs
    lib = base._lib
    del warm
    torch.cuda.empty_cache()
    ms = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, fn in runs.items():
            t, out = timed(fn)
            ms[k].append(round(t, 2))
            del out
    med = {k: statistics.median(v) for k, v in ms.items()}
    res = {"tool": "tools/bench_regraph.py", "device": torch.cuda.get_device_name(0), "crystals": G, "atoms": N,
           "radius": a.radius, "cap": a.cap, "edges": edges, "edges_capped": edges_cap,
           "rounds": a.rounds, "ms": ms, "ms_median": {k: round(v, 2) for k, v in med.items()},
           "transient_bytes_uncapped": int(lib.cartnet_shard_regraph_workspace_bytes(G, N, 0)),
           "transient_bytes_capped": int(lib.cartnet_shard_regraph_workspace_bytes(G, N, edges)),
           "output_bytes_uncapped": 24 * edges + 8 * (G + 1), "output_bytes_capped": 24 * edges_cap + 8 * (G + 1)}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
