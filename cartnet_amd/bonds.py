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

Riding hydrogens (``metrics.riding_h``, csrc/riding_ops.hip; ``riding_hydrogens_host`` below restates it in numpy).  The
model predicts no ADP for a hydrogen; the riding model gives it an isotropic U that is a fixed multiple of the equivalent
isotropic U of the atom it is bonded to (SHELXL: 1.5 for methyl, hydroxyl and water hydrogens, 1.2 for all others).
``is_h_bond`` is the bond rule with one end a hydrogen: the parent's Z is greater than 1 and inside the table, and
``cart_dist[e] <= (r[1] + r[z_parent]) + tol`` in fp32 in that order.

  parent      For a hydrogen ``i`` (Z == 1): among the edges ``j -> i`` with ``j != i``, ``j`` a non-hydrogen atom inside
              the table that has an ADP row, and ``is_h_bond``, the source of the edge with the smallest ``cart_dist``;
              a tie goes to the lowest edge index.  No such edge: an orphan, ``parent = -1``, ``mult = 0``,
              ``u_iso = NaN``.  Non-hydrogen atoms have ``parent = -1`` as well.
  count       For a non-hydrogen atom ``p``: the edges ``s -> p`` with ``z[s] == 1``, ``parent[s] == p`` and
              ``is_h_bond``.  Hydrogens have 0.
  multiplier  For a hydrogen with parent ``p`` and ``n = max(count[p], 1)`` (the maximum covers a capped, asymmetric graph
              that holds ``i <- p`` but not ``p <- i``): ``f_rot`` if ``z[p] == 8`` (hydroxyl, water) or ``z[p] == 6`` and
              ``n >= 3`` (methyl), else ``f``.  Non-hydrogen atoms have 0.
  value       ``u_iso[i] = fp32(fp64(mult) * fp64(u_eq[atom_row[p]]))`` with ``mult`` held as fp32: the product of two
              fp32 values is exact in fp64, so there is one rounding.  A non-hydrogen atom with a row has its own
              ``u_eq[atom_row[i]]`` (without a row: NaN), so the array fills ``_atom_site_U_iso_or_equiv`` for every
              atom.  A non-positive parent ``u_eq`` is passed through, not hidden.

Only edges the graph holds are seen, as with the rigid-bond test.  In a cell so small that one hydrogen reaches its parent
through two images inside the bond limit, both edges count: that hydrogen is counted twice.
"""
from __future__ import annotations

import numpy as np

BOND_TOLERANCE = 0.4           # Angstrom
RIGID_BOND_THRESHOLD = 1e-3    # Angstrom^2: well-refined organic structures stay below it (Hirshfeld 1976)
RIDING_FACTOR = 1.2            # U_iso(H) / U_eq(parent): SHELXL's convention
RIDING_FACTOR_ROTATING = 1.5   # ... for methyl, hydroxyl and water hydrogens

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


def is_h_bond(dist, z_parent, tol: float = BOND_TOLERANCE) -> np.ndarray:
    """The bond rule with one end a hydrogen, in numpy fp32: ``dist <= (r[1] + r[z_parent]) + tol`` for a parent whose Z is
    greater than 1 and inside the table.  A NaN distance is no bond."""
    r = np.asarray(COVALENT_RADII, dtype=np.float32)
    zp = np.asarray(z_parent, dtype=np.int64)
    ok = (zp > 1) & (zp < len(r))
    limit = (r[1] + r[np.where(ok, zp, 0)]) + np.float32(tol)
    return ok & (np.asarray(dist, dtype=np.float32) <= limit)


def riding_hydrogens_host(z, edge_index, cart_dist, atom_row, u_eq, tol: float = BOND_TOLERANCE, f: float = RIDING_FACTOR,
                          f_rot: float = RIDING_FACTOR_ROTATING):
    """The riding rule of the module docstring in plain numpy: ``(parent [N] int64, count [N] int32, mult [N] fp32,
    u_iso [N] fp32)``.  ``z`` [N] atomic numbers; ``edge_index`` [2,E] = (source, target); ``cart_dist`` [E]; ``atom_row``
    [N]: the row of an atom in ``u_eq`` [M], or -1.  An atom's segment is the edges that name it as their target, in edge
    order."""
    z = np.asarray(z, dtype=np.int64).reshape(-1)
    src, tgt = (np.asarray(a, dtype=np.int64).reshape(-1) for a in np.asarray(edge_index).reshape(2, -1))
    dist = np.asarray(cart_dist, dtype=np.float32).reshape(-1)
    atom_row = np.asarray(atom_row, dtype=np.int64).reshape(-1)
    u_eq = np.asarray(u_eq, dtype=np.float32).reshape(-1)
    N, M = z.shape[0], u_eq.shape[0]
    inside = (src >= 0) & (src < N) & (tgt >= 0) & (tgt < N)
    s, t = np.where(inside, src, 0), np.where(inside, tgt, 0)
    has_row = (atom_row >= 0) & (atom_row < M)
    parent = np.full(N, -1, dtype=np.int64)
    up = inside & (z[t] == 1) & (s != t) & has_row[s] & is_h_bond(dist, z[s], tol)     # heavy source, hydrogen target
    best = np.full(N, np.inf, dtype=np.float32)
    for e in np.nonzero(up)[0]:                                   # edge order: a tie keeps the lowest edge
        if dist[e] < best[t[e]] or parent[t[e]] < 0:
            best[t[e]], parent[t[e]] = dist[e], s[e]
    down = inside & (z[s] == 1) & (parent[s] == t) & is_h_bond(dist, z[t], tol)         # hydrogen source, its parent target
    count = np.bincount(t[down], minlength=N).astype(np.int32)
    mult = np.zeros(N, dtype=np.float32)
    u_iso = np.full(N, np.nan, dtype=np.float32)
    heavy = (z != 1) & has_row
    u_iso[heavy] = u_eq[atom_row[heavy]]
    for i in np.nonzero(parent >= 0)[0]:
        p = parent[i]
        n = max(int(count[p]), 1)
        mult[i] = np.float32(f_rot if z[p] == 8 or (z[p] == 6 and n >= 3) else f)
        u_iso[i] = np.float32(np.float64(mult[i]) * np.float64(u_eq[atom_row[p]]))
    return parent, count, mult, u_iso
