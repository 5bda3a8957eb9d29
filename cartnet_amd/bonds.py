"""The bond rule of the rigid-bond test (``metrics.bond_test``, csrc/bond_ops.hip): covalent radii and the tolerance.

``COVALENT_RADII`` is indexed by the atomic number Z; index 0 is unused and holds 0.0, Z = 1 ... 96 are in Angstrom after
Cordero et al., Dalton Trans. 2008, 2832 (carbon: the sp3 value).  The table is this project's data: the tests pin it as
written here.

A directed edge ``e = (j -> i)`` of a batch's radius graph is a bond when ``i != j`` (an atom's own periodic image is
none), both atomic numbers are non-hydrogen and inside the table, and

    cart_dist[e] <= (r[z_i] + r[z_j]) + tol

evaluated in fp32 in exactly that order: additions only, so ``is_bond`` below (numpy fp32) and the kernel decide alike, bit
for bit.  ``BOND_TOLERANCE`` = 0.4 Angstrom is the usual ``r_i + r_j + 0.4`` connectivity rule.  Only edges the graph
holds are considered: a capped graph (``--max_neighbours``) or a ``--radius`` below a bond length sees fewer bonds.
"""
from __future__ import annotations

import numpy as np

BOND_TOLERANCE = 0.4           # Angstrom
RIGID_BOND_THRESHOLD = 1e-3    # Angstrom^2: well-refined organic structures stay below it (Hirshfeld 1976)

COVALENT_RADII = (
    0.0,
    0.31, 0.28, 1.28, 0.96, 0.84, 0.76, 0.71, 0.66, 0.57, 0.58, 1.66, 1.41, 1.21, 1.11, 1.07, 1.05,      # H  ... S
    1.02, 1.06, 2.03, 1.76, 1.70, 1.60, 1.53, 1.39, 1.39, 1.32, 1.26, 1.24, 1.32, 1.22,                  # Cl ... Zn
    1.22, 1.20, 1.19, 1.20, 1.20, 1.16, 2.20, 1.95, 1.90, 1.75, 1.64, 1.54, 1.47, 1.46,                  # Ga ... Ru
    1.42, 1.39, 1.45, 1.44, 1.42, 1.39, 1.39, 1.38, 1.39, 1.40, 2.44, 2.15, 2.07, 2.04,                  # Rh ... Ce
    2.03, 2.01, 1.99, 1.98, 1.98, 1.96, 1.94, 1.92, 1.92, 1.89, 1.90, 1.87, 1.87, 1.75,                  # Pr ... Hf
    1.70, 1.62, 1.51, 1.44, 1.41, 1.36, 1.36, 1.32, 1.45, 1.46, 1.48, 1.40, 1.50, 1.50,                  # Ta ... Rn
    2.60, 2.21, 2.15, 2.06, 2.00, 1.96, 1.90, 1.87, 1.80, 1.69,                                          # Fr ... Cm
)


def is_bond(dist, z_i, z_j, tol: float = BOND_TOLERANCE, same_atom=False) -> np.ndarray:
    """The bond rule in numpy fp32 for arrays (or scalars) of distances and atomic numbers of the two ends; ``same_atom``:
    where the edge joins an atom to its own image."""
    r = np.asarray(COVALENT_RADII, dtype=np.float32)
    zi, zj = np.asarray(z_i, dtype=np.int64), np.asarray(z_j, dtype=np.int64)
    ok = (zi > 1) & (zi < len(r)) & (zj > 1) & (zj < len(r)) & ~np.asarray(same_atom, dtype=bool)
    limit = (r[np.where(ok, zi, 0)] + r[np.where(ok, zj, 0)]) + np.float32(tol)
    return ok & (np.asarray(dist, dtype=np.float32) <= limit)
