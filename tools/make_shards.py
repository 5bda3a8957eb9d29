#!/usr/bin/env python3
"""Write a synthetic dataset split as shard files for ``main.py --shard_dir DIR``: DIR/train.cnshard, val.cnshard and
test.cnshard (cartnet_amd/shard.py), the crystals of ``--synthetic N --atoms lo hi`` split by the seed-123 80/10/10 rule of
``main.create_loaders`` (loader/loader.py:130-141).

    python tools/make_shards.py DIR --synthetic 2000 --atoms 30 70                  # uncapped radius-5 graphs
    python tools/make_shards.py DIR --synthetic 2000 --max_neighbours 25            # capped graphs (e/iComformer)
    python tools/make_shards.py DIR --synthetic 2000 --geometry_only                # no edges: graphed on the GPU at load
    python tools/make_shards.py DIR --synthetic 2000 --unlabeled                    # also DIR/predict.cnshard (see below)

Graphs are built on the host (the reference's edge order) and their radius / cap recorded in the header.  ADP temperatures
are stored in Kelvin, as the reference's files hold them (dataset/datasetADP.py:43-45 standardises at load, and so does
``--shard_dir``); ``--standardized_temperature`` stores the synthetic crystals' standardised values instead, for runs with
``--no_standarize_temp``.  ``--unlabeled`` (ADP) additionally writes DIR/predict.cnshard for ``main.py --predict``: the test
crystals once more, geometry only and without targets, named ``syn<k>`` after their synthetic index.  Runs on the host: no
GPU needed."""
from __future__ import annotations

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cartnet_amd.shard import write_shard                                       # noqa: E402
from cartnet_amd.synthetic import TEMP_MEAN, TEMP_STD, make_crystal, make_geometry   # noqa: E402

PARTS = ("train", "val", "test")


def split(items):
    """main.create_loaders' split: seed-123 permutation, 80 / 10 / 10, an empty part falls back to the first train item."""
    perm = torch.randperm(len(items), generator=torch.Generator().manual_seed(123)).tolist()
    n_tr, n_va = int(0.8 * len(items)), int(0.1 * len(items))
    tr = [items[i] for i in perm[:n_tr]]
    return tr, [items[i] for i in perm[n_tr:n_tr + n_va]] or tr[:1], [items[i] for i in perm[n_tr + n_va:]] or tr[:1]


def to_kelvin(d):
    d.temperature = d.temperature * TEMP_STD + TEMP_MEAN
    return d


def write_split(out_dir: str, n: int, atoms=(30, 70), adp: bool = True, radius: float = 5.0, max_neighbors=None,
                geometry_only: bool = False, kelvin: bool = True, unlabeled: bool = False):
    """Writes the three shard files and returns the three lists of crystals as they were stored.  ``unlabeled``: also
    predict.cnshard, the test crystals as geometry without ``y``, named ``syn<k>``."""
    cap = max_neighbors if max_neighbors is not None and max_neighbors > 0 else None
    if geometry_only:
        items = [make_geometry(g, None, tuple(atoms), adp) for g in range(n)]
    else:
        items = [make_crystal(g, None, radius, tuple(atoms), adp=adp, max_neighbors=cap) for g in range(n)]
    if adp and kelvin:
        items = [to_kelvin(d) for d in items]
    parts = split(items)
    os.makedirs(out_dir, exist_ok=True)
    graph = None if geometry_only else {"radius": radius, "max_neighbors": cap}
    for name, part in zip(PARTS, parts):
        write_shard(os.path.join(out_dir, name + ".cnshard"), part, graph=graph)
    if unlabeled:
        if not adp:
            raise ValueError("--unlabeled: only ADP shards are predicted for")
        ids = split(list(range(n)))[2]
        geo = [make_geometry(g, None, tuple(atoms), True) for g in ids]
        for d in geo:
            del d.y
        write_shard(os.path.join(out_dir, "predict.cnshard"), [to_kelvin(d) for d in geo] if kelvin else geo,
                    names=[f"syn{g}" for g in ids])
    return parts


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("out_dir")
    p.add_argument("--synthetic", type=int, default=32)
    p.add_argument("--atoms", type=int, nargs=2, default=(30, 70))
    p.add_argument("--dataset", type=str, default="ADP", help="ADP: per-atom 3x3 targets, mask, temperature; else scalar")
    p.add_argument("--radius", type=float, default=5.0)
    p.add_argument("--max_neighbours", type=int, default=-1)
    p.add_argument("--geometry_only", action="store_true")
    p.add_argument("--standardized_temperature", action="store_true")
    p.add_argument("--unlabeled", action="store_true",
                   help="also write DIR/predict.cnshard: the test crystals, geometry only, without targets, named syn<k>")
    a = p.parse_args(argv)
    parts = write_split(a.out_dir, a.synthetic, a.atoms, a.dataset == "ADP", a.radius, a.max_neighbours, a.geometry_only,
                        not a.standardized_temperature, a.unlabeled)
    print({name: len(part) for name, part in zip(PARTS, parts)})


if __name__ == "__main__":
    main()
