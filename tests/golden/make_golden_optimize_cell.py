"""Generate tests/golden/optimize_cell.npz from the REFERENCE ITSELF (build container only).

Runs the reference's own ``DatasetADP.get`` (dataset/datasetADP.py:41-86) with ``optimize_cell=True`` -- and through it
``optmize_lattice`` (dataset/utils.py:366-452) -- imported read-only from the reference checkout
(``_ref_import.REFERENCE_ROOT``) with the stand-ins of make_golden_no_hydrogens.py, on small crystals, and stores its
inputs and outputs as plain arrays.  The reference's source never enters the repo; only tensors do.

    python tests/golden/make_golden_optimize_cell.py          # rewrites tests/golden/optimize_cell.npz

Per crystal i: ``in{i}_<key>`` what was pickled, ``out{i}_<key>`` what ``get`` returned (``cell_og`` too), ``hydrogens{i}``
the flag ``get`` ran with.  ``group`` [n] says what a crystal is there for:

  0  a generic synthetic crystal: in fp64 the norms of distinct candidates differ by more than 1e-3 (relative) up to the
     third chosen vector and |cos| between the first chosen vector and the other two exceeds 1e-2
     (``cartnet_amd.data.lattice_margins``; asserted below), so every fp32 evaluation of the rule picks the same basis;
  1  crystal ``partner[i]`` of group 0 once more, its cell re-described by the unimodular matrix ``unimodular[i]``
     (new rows = U @ old rows); positions and edges are unchanged: a radius graph depends on the lattice, not on its basis;
  2  special cells -- cubic, orthorhombic with permuted axes, hexagonal, fcc and bcc primitive, monoclinic with an obtuse
     angle, left-handed -- where candidates tie or are exactly orthogonal: the reference's result depends on its unstable
     ``argsort`` there, so the tests check validity on these, not equality;
  3  a group-0 crystal once more through ``hydrogens=False``.
"""
from __future__ import annotations

import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from make_golden_no_hydrogens import import_dataset_adp  # noqa: E402

from cartnet_amd.data import Data, lattice_margins  # noqa: E402
from cartnet_amd.synthetic import make_crystal, radius_graph_pbc_single  # noqa: E402

KEYS = ("x", "pos", "edge_index", "cart_dist", "cart_dir", "y", "cell", "temperature", "non_H_mask")
GENERIC = [(401, 12), (402, 12), (403, 12), (404, 12), (405, 12), (407, 12), (408, 12), (409, 12), (410, 12), (411, 12)]
UNIMODULAR = [[[1, 1, 0], [0, 1, 0], [0, 0, 1]],            # a -> a + b
              [[1, 0, 0], [0, 1, 0], [1, 0, 1]],            # c -> c + a
              [[0, 1, 0], [0, 0, 1], [1, 0, 0]],            # cyclic permutation
              [[-1, 0, 0], [0, -1, 0], [0, 0, 1]],          # two axes negated
              [[1, 0, 0], [1, 1, 0], [0, 1, 1]]]
S3 = 3.0 ** 0.5
SPECIAL = [("cubic", [[5.0, 0, 0], [0, 5.0, 0], [0, 0, 5.0]], 9),
           ("orthorhombic, axes permuted", [[0, 0, 7.0], [4.0, 0, 0], [0, 5.5, 0]], 10),
           ("hexagonal", [[4.0, 0, 0], [-2.0, 2.0 * S3, 0], [0, 0, 6.5]], 8),
           ("fcc primitive", [[0, 2.75, 2.75], [2.75, 0, 2.75], [2.75, 2.75, 0]], 7),
           ("bcc primitive", [[-2.5, 2.5, 2.5], [2.5, -2.5, 2.5], [2.5, 2.5, -2.5]], 7),
           ("monoclinic, obtuse", [[6.0, 0, 0], [0, 7.0, 0], [-3.0, 0, 8.0]], 12),
           ("left-handed", [[5.0, 0.3, 0], [0.2, 6.0, 0], [0.1, 0.4, -7.0]], 11)]
NO_HYDROGEN_OF = 1                                          # the group-0 crystal that is stored again for group 3


def crystal_in_cell(cell, n: int, seed: int) -> Data:
    """``n`` atoms at uniform fractional coordinates in ``cell``, with the attributes of make_crystal."""
    gen = torch.Generator().manual_seed(seed)
    cell = torch.tensor(cell, dtype=torch.float32)
    pos = torch.rand(n, 3, generator=gen) @ cell
    z = torch.where(torch.rand(n, generator=gen) < 0.4, torch.tensor(1), torch.tensor(6)).to(torch.int64)
    z[0] = 6
    edge_index, cart_dist, cart_dir = radius_graph_pbc_single(pos, cell, 5.0)
    m = int((z != 1).sum())
    A = torch.randn(m, 3, 3, generator=gen)
    return Data(x=z, pos=pos, cell=cell.unsqueeze(0), edge_index=edge_index, cart_dist=cart_dist, cart_dir=cart_dir,
                y=0.01 * A @ A.transpose(1, 2) + 0.005 * torch.eye(3), non_H_mask=z != 1,
                temperature=torch.tensor([0.5]))


def crystals():
    out, group, partner, uni, hydrogens = [], [], [], [], []

    def add(d, grp, par=-1, u=None, h=True):
        out.append(d)
        group.append(grp)
        partner.append(par)
        uni.append(np.eye(3, dtype=np.int64) if u is None else np.asarray(u, dtype=np.int64))
        hydrogens.append(h)
    for g, n in GENERIC:
        d = make_crystal(g, n)
        del d.natoms                               # the reference's files carry no such attribute
        gap, cos = lattice_margins(d.cell[0])
        assert gap > 1e-3 and cos > 1e-2, f"crystal {g} is not generic: gap {gap:.2e}, |cos| {cos:.2e}"
        add(d, 0)
    for i in range(len(GENERIC)):
        u = UNIMODULAR[i % len(UNIMODULAR)]
        d = out[i].clone()
        d.cell = (torch.tensor(u, dtype=torch.float32) @ out[i].cell[0]).unsqueeze(0)
        gap, cos = lattice_margins(d.cell[0])
        assert gap > 1e-3 and cos > 1e-2, f"re-described crystal {i} is not generic: gap {gap:.2e}, |cos| {cos:.2e}"
        add(d, 1, i, u)
    for s, (_, cell, n) in enumerate(SPECIAL):
        add(crystal_in_cell(cell, n, 900 + s), 2)
    keep = out[NO_HYDROGEN_OF].x != 1
    assert bool((keep[out[NO_HYDROGEN_OF].edge_index[0]] & keep[out[NO_HYDROGEN_OF].edge_index[1]]).any())
    add(out[NO_HYDROGEN_OF].clone(), 3, NO_HYDROGEN_OF, None, False)
    return out, group, partner, uni, hydrogens


def main():
    DatasetADP = import_dataset_adp()
    torch.serialization.add_safe_globals([Data])
    ds_in, group, partner, uni, hydrogens = crystals()
    arrays = {"n_crystals": np.int64(len(ds_in)), "group": np.asarray(group, dtype=np.int64),
              "partner": np.asarray(partner, dtype=np.int64), "unimodular": np.stack(uni),
              "hydrogens": np.asarray(hydrogens, dtype=bool)}
    with tempfile.TemporaryDirectory() as tmp:
        names = [f"crystal{i}" for i in range(len(ds_in))]
        for name, d in zip(names, ds_in):
            torch.save(d, os.path.join(tmp, name + ".pt"))
        listing = os.path.join(tmp, "names.txt")
        with open(listing, "w") as f:
            f.write("\n".join(names) + "\n")
        sets = {h: DatasetADP(root=tmp, file_names=listing, standarize_temp=False, hydrogens=h, augment=False,
                              optimize_cell=True) for h in (True, False)}
        for i, d in enumerate(ds_in):
            got = sets[hydrogens[i]].get(i)
            for k in KEYS:
                arrays[f"in{i}_{k}"] = getattr(d, k).numpy()
                arrays[f"out{i}_{k}"] = getattr(got, k).numpy()
            arrays[f"out{i}_cell_og"] = got.cell_og.numpy()
    path = os.path.join(HERE, "optimize_cell.npz")
    np.savez_compressed(path, **arrays)
    print(len(ds_in), "crystals, groups", np.bincount(group).tolist(), "atoms",
          [int(d.x.shape[0]) for d in ds_in], os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
