"""Crystals with hydrogens and the host chain shared by the anisotropic-hydrogen tests: a brute-force periodic radius graph
in numpy, the riding / molecule / TLS rules of ``cartnet_amd.bonds`` run one after the other on it, and the crystals of
the GPU tests."""
import numpy as np

import molecule_utils as mu
import tls_utils as tu

RADIUS = 5.0
FACE_START, FACE_CELL = (3.0, 12.0, 28.6), 30.0      # a helix of 7 whose hydrogens (1 A above) reach z = 30.4: two cross


def host_graph(pos, cell, radius=RADIUS):
    """``(edge_index [2,E], cart_dist [E] fp32, cart_dir [E,3] fp32)`` of one crystal: every pair (target i, source j, image
    n in {-1, 0, 1}^3) with ``0 < |pos_i - (pos_j + n @ cell)| <= radius``, the vector stored as the radius graph stores it,
    sorted by target.  Good for cells whose faces are ``radius`` or more apart."""
    pos, cell = np.asarray(pos, dtype=np.float64), np.asarray(cell, dtype=np.float64)
    n = np.stack(np.meshgrid(*[[-1, 0, 1]] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    vec = pos[:, None, None, :] - (pos[None, :, None, :] + (n @ cell)[None, None, :, :])      # [target, source, image, 3]
    dist = np.linalg.norm(vec, axis=-1)
    tgt, src, img = np.nonzero((dist > 0) & (dist <= radius))
    vec, dist = vec[tgt, src, img], dist[tgt, src, img]
    return np.stack([src, tgt]), dist.astype(np.float32), (vec / dist[:, None]).astype(np.float32)


def host_chain(pos, cell, z, rows, tls=True, stretch=0.0, bend=0.0):
    """The whole host chain on one crystal: the graph, the riding parents, the molecules, the TLS fit of the fp32 ``rows``
    [M,3,3] and ``aniso_hydrogens_host``; ``tls=False`` passes no TLS results.  Returns the rule's dict with ``parent``,
    ``atom_row``, ``rows`` (fp32) and ``fit`` (``tls_fit_host``'s) added."""
    from cartnet_amd import bonds
    z = np.asarray(z, dtype=np.int64)
    rows = np.asarray(rows, dtype=np.float32)
    ei, dist, dirs = host_graph(pos, cell)
    atom_row = mu.atom_rows(z != 1)
    u_eq = ((rows[:, 0, 0] + rows[:, 1, 1]) + rows[:, 2, 2]) / np.float32(3)
    parent = bonds.riding_hydrogens_host(z, ei, dist, atom_row, u_eq)[0]
    mo = bonds.molecules_host(z, ei, dist, dirs, atom_row)
    fit = bonds.tls_fit_host(rows, mo["label"], mo["x"], atom_row, mo["status"], mo["size"])
    extra = dict(x=mo["x"], params=fit["params"], rank=fit["rank"]) if tls else {}
    out = bonds.aniso_hydrogens_host(rows, z, ei, dist, dirs, atom_row, parent, stretch=stretch, bend=bend, **extra)
    out.update(parent=parent, atom_row=atom_row, rows=rows, fit=fit)
    return out


def mixed_crystal():
    """``(pos, cell, z, rows)``: a puckered ring of 6, a helix of 7, a planar chain of 8 and a chain of 3, every carbon with
    a hydrogen 1 A above it, and one lone hydrogen: sources 0 ... 4 number 1, 24, 3, 13 and 8."""
    molecules = [mu.ring((5, 5, 5)), tu.helix(7, (3, 12, 12)), tu.planar_chain(8, (3, 20, 20)), tu.planar_chain(3, (3, 30, 30))]
    pos, z = tu.with_hydrogens(np.concatenate(molecules))
    rows = np.concatenate([tu.rigid_rows(m, 700 + 7 * k, tu.NOISE) for k, m in enumerate(molecules)])
    return np.concatenate([pos, [[30.0, 5.0, 5.0]]]), mu.cubic(40.0), np.concatenate([z, [1]]), rows.astype(np.float32)


def polymer_crystal():
    """The polymer with a hydrogen on every carbon: periodic, so not fitted -- all 8 hydrogens are source 2."""
    pos, cell, _ = mu.polymer(8)
    both, z = tu.with_hydrogens(pos)
    return both, cell, z, tu.rigid_rows(pos, 710, tu.NOISE).astype(np.float32)


def face_crystal(wrap=True, seed=720, noise=0.0):
    """The helix of 7 at the face of its 30 A cell with its hydrogens, every atom wrapped into the cell or not."""
    carbons = tu.helix(7, FACE_START)
    pos, z = tu.with_hydrogens(carbons)
    cell = mu.cubic(FACE_CELL)
    return (np.mod(pos, FACE_CELL) if wrap else pos), cell, z, tu.rigid_rows(carbons, seed, noise).astype(np.float32)


def methyl_crystal():
    """A helix of 5 with three hydrogens on its third atom, 1 A away across the chain."""
    carbons = tu.helix(5, (3, 6, 6))
    h = carbons[2] + np.array([[0.0, 0.0, 1.0], [0.0, 0.866, -0.5], [0.0, -0.866, -0.5]])
    pos = mu.on_grid(np.concatenate([carbons[:3], h, carbons[3:]]))
    return pos, mu.cubic(20.0), np.array([6, 6, 6, 1, 1, 1, 6, 6]), tu.rigid_rows(carbons, 730, tu.NOISE).astype(np.float32)


def gpu_crystals():
    """Eight crystals ``(pos, cell, z)`` and the fp32 rows [M,3,3] of their non-hydrogen atoms in atom order:
      0  ``mixed_crystal``: every source code
      1  ``polymer_crystal``: periodic, source 2
      2  ``face_crystal``: two hydrogens through the cell face
      3  three lone hydrogens: no rows at all, in the middle of the batch
      4  ``methyl_crystal``: three hydrogens on one parent
      5  a helix of 5 without hydrogens
      6  a helix of 6 with hydrogens whose rows are negated: no tensor is positive definite
      7  helices of 130 and 65 atoms, interleaved by a fixed permutation, every carbon followed by its hydrogen"""
    crystals, rows = [], []
    for pos, cell, z, u in (mixed_crystal(), polymer_crystal(), face_crystal(noise=tu.NOISE)):
        crystals.append((pos, cell, z))
        rows.append(u)
    crystals.append((np.array([[1.0, 1.0, 1.0], [4.0, 4.0, 4.0], [7.0, 7.0, 7.0]]), mu.cubic(10.0), np.ones(3, dtype=np.int64)))
    rows.append(np.zeros((0, 3, 3), dtype=np.float32))
    pos, cell, z, u = methyl_crystal()
    crystals.append((pos, cell, z))
    rows.append(u)
    bare = tu.helix(5, (3, 6, 6))
    crystals.append((bare, mu.cubic(20.0), np.full(5, 6)))
    rows.append(tu.rigid_rows(bare, 740, tu.NOISE).astype(np.float32))
    six = tu.helix(6, (3, 6, 6))
    pos, z = tu.with_hydrogens(six)
    crystals.append((pos, mu.cubic(20.0), z))
    rows.append(-tu.rigid_rows(six, 750, tu.NOISE).astype(np.float32))
    long = [tu.helix(130, (2, 5, 5)), tu.helix(65, (2, 12, 12))]
    order = np.random.default_rng(5).permutation(195)
    pos, z = tu.with_hydrogens(np.concatenate(long)[order])
    crystals.append((pos, np.diag([180.0, 20.0, 20.0]), z))
    rows.append(np.concatenate([tu.rigid_rows(m, 760 + 7 * k, tu.NOISE) for k, m in enumerate(long)])[order].astype(np.float32))
    return crystals, np.concatenate(rows)


def entry_with_hydrogens():
    """A hand-made ``predict_adps`` entry of three atoms -- a carbon, its hydrogen with a tensor and an orphan hydrogen --
    with the keys of ``riding_h`` and ``aniso_h``, as torch tensors."""
    import torch
    nan = float("nan")
    return {"name": "pair", "temp": 120.0, "cell": torch.eye(3) * 10.0,
            "z": torch.tensor([6, 1, 1]), "atoms": torch.tensor([6]),
            "frac": torch.tensor([[0.1, 0.2, 0.3], [0.1, 0.2, 0.4], [0.7, 0.7, 0.7]]),
            "u_cif": torch.tensor([[0.02, 0.03, 0.04, 0.001, 0.002, 0.003]]), "u_eq": torch.tensor([0.03]),
            "u_iso": torch.tensor([0.03, 0.036, nan]),
            "h_u_cif": torch.tensor([[0.02, 0.03, 0.04, 0.001, 0.002, 0.003], [0.04, 0.05, 0.045, 0.001, 0.002, 0.003],
                                     [nan] * 6]),
            "h_u_eq": torch.tensor([0.03, 0.045, nan]), "h_source": torch.tensor([1, 2, 0], dtype=torch.int32)}
