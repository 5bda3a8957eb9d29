"""Generate tests/golden/cif_expand.npz from the REFERENCE ITSELF (build container only).

Runs the reference's own ``delete_repeated`` and ``frac_to_cart_matrix`` (dataset/extract_csd_data.py:15-40), imported
read-only from the reference checkout (``_ref_import.REFERENCE_ROOT``), and stores their inputs and outputs as plain
arrays.  The reference's source never enters the repo; only tensors do.

    python tests/golden/make_golden_cif_expand.py          # rewrites tests/golden/cif_expand.npz

The module imports the CSD API, gemmi, pandas and its own ``utils`` at the top; none of them is touched by the two
functions, so empty stand-in modules are enough (``ccdc.io``, ``gemmi.cif``, ``pandas``, a bare ``utils`` with a
``radius_graph_pbc`` name, ``torch_geometric.data`` from _ref_import.py).

Stored: ``n_sets``, per coordinate set i ``coord{i}`` [r,3] fp32 and ``keep{i}`` [r] bool; ``cells`` [6,6] fp64
(a b c alpha beta gamma) and ``matrices`` [6,3,3] fp32 (rows = lattice vectors).  Two conditions keep bit-exactness
meaningful -- the answer must not hang on how a distance or a difference is rounded -- and are asserted here:
no pair distance lies in [5e-5, 2e-4], and no coordinate (after the first two steps of the normalisation) lies in
1 - [0.9e-4, 1.3e-4].
"""
from __future__ import annotations

import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from _ref_import import REFERENCE_ROOT, install_standins  # noqa: E402

CELLS = [(5.64, 5.64, 5.64, 90.0, 90.0, 90.0),            # cubic
         (5.812, 11.237, 7.446, 90.0, 104.31, 90.0),      # monoclinic
         (10.512, 10.512, 14.237, 90.0, 90.0, 120.0),     # hexagonal
         (7.123, 8.456, 9.789, 81.23, 77.45, 68.91),      # triclinic
         (5.1, 7.3, 11.9, 62.0, 104.0, 118.0),            # skewed triclinic
         (4.3, 7.9, 12.1, 90.0, 90.0, 90.0)]              # orthorhombic
SIZES = (1, 7, 64, 257, 300, 600)


def import_extract():
    install_standins()
    for name, attrs in (("ccdc", {"io": types.ModuleType("ccdc.io")}), ("gemmi", {"cif": types.ModuleType("gemmi.cif")}),
                        ("pandas", {}), ("utils", {"radius_graph_pbc": None})):
        m = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(m, k, v)
            if isinstance(v, types.ModuleType):
                sys.modules[v.__name__] = v
        sys.modules[name] = m
    sys.path.insert(0, os.path.join(REFERENCE_ROOT, "dataset"))
    return importlib.import_module("extract_csd_data")


def coordinate_set(n: int, seed: int) -> torch.Tensor:
    """n rows of fp32 fractions on a coarse grid (so that distinct atoms are far apart) with, where n allows: exact
    repeats, repeats shifted by 3e-5, negatives (a repeat minus 1), values above 1 (a repeat plus 1), and the triple
    0.99995 / 0.0 / 1.0 in one coordinate."""
    g = torch.Generator().manual_seed(seed)
    base = n if n < 7 else max(2, n // 2)
    pts = torch.randperm(40 ** 3, generator=g)[:base]
    x = torch.stack([pts // 1600, (pts // 40) % 40, pts % 40], 1).to(torch.float64) / 40.0 + 0.0123
    rows = [x]
    if n >= 7:
        extra = n - base
        src = x[torch.randint(0, base, (extra,), generator=g)].clone()
        kind = torch.arange(extra) % 4
        src[kind == 1, 2] += 3e-5
        src[kind == 2, 0] -= 1.0
        src[kind == 3, 1] += 1.0
        rows.append(src)
    out = torch.cat(rows).to(torch.float32)
    if n >= 7:
        out[0] = torch.tensor([0.99995, 0.25, 0.5])
        out[1] = torch.tensor([0.0, 0.25, 0.5])
        out[2] = torch.tensor([1.0, 0.25, 0.5])
    return out[torch.randperm(n, generator=g)] if n > 3 else out


def check_margins(coord: torch.Tensor) -> None:
    x = coord.clone()
    x = torch.where(x < 0, x + 1, x)
    x = torch.where(x > 1, x - 1, x)
    gap = (1.0 - x.double())
    assert not bool(((gap >= 0.9e-4) & (gap <= 1.3e-4)).any()), "a coordinate at the edge of the isclose window"
    x = torch.where((1.0 - x.double()).abs() < 1.1e-4, torch.zeros_like(x), x).double()
    d = torch.cdist(x, x)
    assert not bool(((d >= 5e-5) & (d <= 2e-4)).any()), "a pair distance at the edge of the threshold"


def main():
    ref = import_extract()
    arrays = {"n_sets": np.int64(len(SIZES))}
    for i, n in enumerate(SIZES):
        coord = coordinate_set(n, 500 + i)
        check_margins(coord)
        keep = ref.delete_repeated(coord.clone())
        arrays[f"coord{i}"] = coord.numpy()
        arrays[f"keep{i}"] = keep.numpy()
    arrays["cells"] = np.array(CELLS, dtype=np.float64)
    arrays["matrices"] = np.stack([ref.frac_to_cart_matrix(c[:3], c[3:]).numpy() for c in CELLS]).astype(np.float32)
    np.savez_compressed(os.path.join(HERE, "cif_expand.npz"), **arrays)
    print("rows", list(SIZES), "kept", [int(arrays[f"keep{i}"].sum()) for i in range(len(SIZES))])


if __name__ == "__main__":
    main()
