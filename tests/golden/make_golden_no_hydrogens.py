"""Generate tests/golden/no_hydrogens.npz from the REFERENCE ITSELF (build container only).

Runs the reference's own ``DatasetADP.get`` (dataset/datasetADP.py:41-86) with ``hydrogens=False``, imported read-only
from the reference checkout (``_ref_import.REFERENCE_ROOT``), on a handful of small synthetic crystals and stores its
inputs and outputs as plain arrays.  The reference's source never enters the repo; only tensors do.

    python tests/golden/make_golden_no_hydrogens.py          # rewrites tests/golden/no_hydrogens.npz

Beyond the stand-ins of _ref_import.py, ``get`` needs:
  * ``torch_geometric.data.Dataset``: a base class whose constructor takes (root, transform, pre_transform); the
    reference's ``len`` / ``get`` are called directly;
  * ``roma`` as an import (only ``augment_data`` calls it; augment stays off);
  * one ``<name>.pt`` per crystal in a temporary directory and a text file listing the names: ``get`` reads them with
    ``torch.load``.

``standarize_temp=False``, so the stored temperature is returned as it is.  Every crystal keeps at least one edge
between two non-hydrogen atoms (the reference's renumbering turns an empty edge list into a malformed tensor); crystal
2 has no hydrogen at all.  Per crystal i: ``in{i}_<key>`` what was pickled, ``out{i}_<key>`` what ``get`` returned.
"""
from __future__ import annotations

import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from _ref_import import REFERENCE_ROOT, install_standins  # noqa: E402

from cartnet_amd.data import Data  # noqa: E402
from cartnet_amd.synthetic import make_crystal  # noqa: E402

KEYS = ("x", "pos", "edge_index", "cart_dist", "cart_dir", "y", "cell", "temperature", "non_H_mask")
# (graph id, atoms): make_crystal(g, n) draws 45 % hydrogens
CRYSTALS = [(210, 7), (201, 12), (202, 9), (203, 24), (204, 40)]
NO_HYDROGEN = 2                                  # this one's hydrogens are turned into carbon before it is stored


class _Dataset:
    def __init__(self, root=None, transform=None, pre_transform=None):
        self.root = root


def import_dataset_adp():
    install_standins()
    sys.modules["torch_geometric.data"].Dataset = _Dataset
    sys.modules.setdefault("roma", types.ModuleType("roma"))
    if REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, REFERENCE_ROOT)
    import importlib
    return importlib.import_module("dataset.datasetADP").DatasetADP


def crystals():
    out = []
    for i, (g, n) in enumerate(CRYSTALS):
        d = make_crystal(g, n)
        if i == NO_HYDROGEN:
            d.x = torch.where(d.x == 1, torch.tensor(6), d.x)
            m = int(d.x.shape[0])
            gen = torch.Generator().manual_seed(77)
            A = torch.randn(m, 3, 3, generator=gen)
            d.y = 0.01 * A @ A.transpose(1, 2) + 0.005 * torch.eye(3)
            d.non_H_mask = d.x != 1
        keep = d.x != 1
        assert bool((keep[d.edge_index[0]] & keep[d.edge_index[1]]).any()), f"crystal {i} keeps no edge"
        del d.natoms                               # the reference's files carry no such attribute
        out.append(d)
    return out


def main():
    DatasetADP = import_dataset_adp()
    torch.serialization.add_safe_globals([Data])
    ds_in = crystals()
    arrays = {"n_crystals": np.int64(len(ds_in))}
    with tempfile.TemporaryDirectory() as tmp:
        names = [f"crystal{i}" for i in range(len(ds_in))]
        for name, d in zip(names, ds_in):
            torch.save(d, os.path.join(tmp, name + ".pt"))
        listing = os.path.join(tmp, "names.txt")
        with open(listing, "w") as f:
            f.write("\n".join(names) + "\n")
        ds = DatasetADP(root=tmp, file_names=listing, standarize_temp=False, hydrogens=False, augment=False,
                        optimize_cell=False)
        assert ds.len() == len(ds_in)
        for i, d in enumerate(ds_in):
            got = ds.get(i)
            for k in KEYS:
                arrays[f"in{i}_{k}"] = getattr(d, k).numpy()
                arrays[f"out{i}_{k}"] = getattr(got, k).numpy()
    np.savez_compressed(os.path.join(HERE, "no_hydrogens.npz"), **arrays)
    kept = [int(arrays[f"out{i}_x"].shape[0]) for i in range(len(ds_in))]
    print("atoms", [n for _, n in CRYSTALS], "->", kept, "edges",
          [arrays[f"in{i}_edge_index"].shape[1] for i in range(len(ds_in))], "->",
          [arrays[f"out{i}_edge_index"].shape[1] for i in range(len(ds_in))])


if __name__ == "__main__":
    main()
