"""fp64 restatements and fixtures shared by the prediction / ADP-export tests."""
import numpy as np
import torch

from cartnet_amd.data import Data
from cartnet_amd.synthetic import make_geometry

CIF_ORDER = ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))          # U11 U22 U33 U23 U13 U12


def cell_from_parameters(a, b, c, alpha, beta, gamma) -> np.ndarray:
    """Rows = lattice vectors, a along x and b in the xy plane (the standard setting), fp64; angles in degrees."""
    al, be, ga = np.radians([alpha, beta, gamma])
    cx = c * np.cos(be)
    cy = c * (np.cos(al) - np.cos(be) * np.cos(ga)) / np.sin(ga)
    return np.array([[a, 0.0, 0.0], [b * np.cos(ga), b * np.sin(ga), 0.0], [cx, cy, np.sqrt(c * c - cx * cx - cy * cy)]])


def fixed_rotation() -> np.ndarray:
    """A generic proper rotation (no axis of it is a coordinate axis): Rodrigues about (1, 2, 3) by 0.83 rad."""
    k = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    t = 0.83
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


def cells() -> dict:
    """The four cells of the export tests (rows = lattice vectors), fp32."""
    tri = cell_from_parameters(5.1, 7.3, 11.9, 62.0, 104.0, 118.0)
    return {"cubic": np.float32(np.eye(3) * 6.2), "orthorhombic": np.float32(np.diag([4.3, 7.9, 12.1])),
            "triclinic": np.float32(tri), "triclinic_rotated": np.float32(tri @ fixed_rotation().T)}


def reciprocal_units(cell: np.ndarray) -> np.ndarray:
    """Rows = the unit vectors along the reciprocal vectors a*, b*, c* = the rows of inv(cell^T), fp64."""
    rec = np.linalg.inv(np.asarray(cell, dtype=np.float64).T)
    return rec / np.linalg.norm(rec, axis=1, keepdims=True)


def cart_from_cif(u_cif: np.ndarray, cell: np.ndarray) -> np.ndarray:
    """The reference's dataset/extract_csd_data.py:115-123 in fp64: with M = cell (rows a, b, c) and
    N = diag(row norms of inv(M^T)), y <- N^T y N, then y <- M^T y M.  u_cif [n,3,3] symmetric."""
    M = np.asarray(cell, dtype=np.float64)
    N = np.diag(np.linalg.norm(np.linalg.inv(M.T), axis=-1))
    return M.T @ (N.T @ np.asarray(u_cif, dtype=np.float64) @ N) @ M


def export_reference(u: np.ndarray, cell: np.ndarray):
    """fp64 (u_cif [n,6], u_eq [n], principal [n,3] ascending, U symmetrised [n,3,3]) of fp32 ``u`` [n,3,3] in ``cell``."""
    U = np.asarray(u, dtype=np.float64)
    U = 0.5 * (U + U.transpose(0, 2, 1))
    r = reciprocal_units(cell)
    full = np.einsum("ia,nab,jb->nij", r, U, r)
    cif = np.stack([full[:, i, j] for i, j in CIF_ORDER], axis=1) if len(U) else np.zeros((0, 6))
    return cif, np.trace(U, axis1=1, axis2=2) / 3.0, (np.linalg.eigvalsh(U) if len(U) else np.zeros((0, 3))), U


def spd_rows(n: int, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(n, 3, 3, generator=g)
    return 0.01 * a @ a.transpose(1, 2) + 0.005 * torch.eye(3)


SIX = ((11, 5, "single"), (12, 17, None), (13, 40, None), (14, 23, "no_h"), (15, 9, None), (16, 31, None))


def six_crystals(labeled: bool) -> list:
    """Six geometry-only crystals of 5 to 40 atoms: one with a single non-hydrogen atom, one without hydrogens.  Labeled:
    with ``y`` and ``non_H_mask``; unlabeled: with neither (the shard derives the mask from z)."""
    out = []
    for g, n, rule in SIX:
        d = make_geometry(g, n)
        x = d.x.clone()
        if rule == "single":
            x[:] = 1
            x[2] = 8
        elif rule == "no_h":
            x[x == 1] = 6
        new = Data(x=x, pos=d.pos, cell=d.cell, natoms=d.natoms, temperature=d.temperature)
        if labeled:
            new.non_H_mask = x != 1
            new.y = spd_rows(int((x != 1).sum()), 100 + g)
        out.append(new)
    return out


def non_h_counts() -> list:
    return [int((d.x != 1).sum()) for d in six_crystals(False)]
