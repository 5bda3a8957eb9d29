"""Geometries and synthetic rigid-body ADPs shared by the TLS tests: helices (the smallest shapes that determine all 20
parameters), the rank-deficient shapes, known T / L / S, and the crystals of the GPU test with their ADP rows."""
import numpy as np

import molecule_utils as mu

EPS22 = 2.0 ** -22
NOISE = 5e-4                     # A^2: symmetric noise on the rigid-body rows, so that resid and R are not trivially zero


def helix(n, start=(0.0, 0.0, 0.0)):
    """``n`` carbons on a helix along x: bonds of 1.80 A (C-C: up to 1.92 A), second neighbours 2.9 A apart, so one chain
    under the bond rule; no plane and no line holds it, so five atoms already determine all 20 parameters."""
    k = np.arange(n, dtype=np.float64)
    return mu.on_grid(np.asarray(start, dtype=np.float64)
                      + np.stack([1.25 * k, 0.8 * np.cos(1.9 * k), 0.8 * np.sin(1.9 * k)], axis=1))


def flat_circle(centre, radius=1.39, n=6):
    """``n`` atoms on a circle in a plane: the conic singularity, rank 19."""
    a = 2 * np.pi * np.arange(n) / n + 0.3
    return mu.on_grid(np.asarray(centre, dtype=np.float64) + radius * np.stack([np.cos(a), np.sin(a), 0 * a], axis=1))


def line(n, start, step=1.4):
    """``n`` collinear atoms along x: rank 14."""
    return mu.on_grid(np.asarray(start, dtype=np.float64) + np.stack([step * np.arange(n)] + [np.zeros(n)] * 2, axis=1))


def planar_chain(n, start=(3.0, 3.0, 3.0)):
    """``molecule_utils.chain`` unwrapped: a planar zig-zag, rank 19."""
    return mu.chain(n, start, mu.cubic(1000.0))[1]


def known_tls(seed):
    """``(T, L, S)``: T symmetric positive definite (A^2) and L positive semidefinite (rad^2) at the scales of
    ``molecule_utils.rigid_body_rows``, S traceless at 1e-4 (rad A)."""
    rng = np.random.default_rng(seed)
    a, b = rng.standard_normal((3, 3)), rng.standard_normal((3, 2))
    S = 1e-4 * rng.standard_normal((3, 3))
    return 0.01 * a @ a.T + 0.005 * np.eye(3), 1e-4 * b @ b.T, S - np.eye(3) * np.trace(S) / 3.0


def rigid_rows(pos, seed, noise=0.0):
    """fp64 [n,3,3]: ``U(r_i)`` of ``known_tls(seed)`` about the centroid of ``pos``, plus symmetric noise of that size."""
    from cartnet_amd.bonds import tls_model
    pos = np.asarray(pos, dtype=np.float64)
    U = tls_model(pos - pos.mean(axis=0), *known_tls(seed))
    if noise:
        e = noise * np.random.default_rng(seed + 1000).standard_normal(U.shape)
        U = U + 0.5 * (e + e.transpose(0, 2, 1))
    return U


def rotation(seed):
    q, r = np.linalg.qr(np.random.default_rng(seed).standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    return q * np.linalg.det(q)


def with_hydrogens(pos):
    """Every atom of ``pos`` followed by a hydrogen 1 A above it: ``(positions, Z)``, the hydrogens interleaved, so that an
    atom's index is not its row."""
    both = np.stack([pos, pos + [0.0, 0.0, 1.0]], axis=1).reshape(-1, 3)
    return mu.on_grid(both), np.tile([6, 1], len(pos))


def gpu_crystals():
    """Seven crystals ``(pos, cell, z)`` and the fp32 ADP rows ``u`` [M,3,3] of their non-hydrogen atoms in atom order:
    rigid-body rows of a TLS of its own per molecule plus noise.
      0  helices of 5, 17 and 4 atoms and a chain of 3: the 4 and the 3 are below the minimum
      1  helices of 130 and 65 atoms, interleaved by a fixed permutation: the ragged case, past one and two strides
      2  a planar chain of 8, a flat circle of 6 and a line of 5: rank 19, 19 and 14
      3  three hydrogens: no rows at all, in the middle of the batch
      4  the polymer: periodic, not fitted
      5  a puckered ring of 6 and a helix of 7, each atom with a hydrogen: rows are not atoms
      6  eleven helices of 5: more molecules than slots"""
    crystals, rows = [], []

    def add(molecules, cell, seed, permute=False, hydrogens=False):
        pos = np.concatenate(molecules)
        u = np.concatenate([rigid_rows(m, seed + 7 * k, NOISE) for k, m in enumerate(molecules)])
        z = np.full(len(pos), 6)
        if permute:
            order = np.random.default_rng(5).permutation(len(pos))
            pos, u = pos[order], u[order]
        if hydrogens:
            pos, z = with_hydrogens(pos)
        crystals.append((pos, cell, z))
        rows.append(u)

    add([helix(5, (3, 3, 3)), helix(17, (3, 12, 12)), helix(4, (3, 20, 20)), planar_chain(3, (3, 30, 30))],
        mu.cubic(40.0), 100)
    add([helix(130, (2, 5, 5)), helix(65, (2, 12, 12))], np.diag([180.0, 20.0, 20.0]), 200, permute=True)
    add([planar_chain(8, (3, 3, 3)), flat_circle((5, 12, 12)), line(5, (3, 20, 20))], mu.cubic(30.0), 300)
    crystals.append((np.array([[1.0, 1.0, 1.0], [4.0, 4.0, 4.0], [7.0, 7.0, 7.0]]), mu.cubic(10.0), np.ones(3, dtype=np.int64)))
    rows.append(np.zeros((0, 3, 3)))
    pos, cell, z = mu.polymer(8)
    crystals.append((pos, cell, z))
    rows.append(rigid_rows(pos, 400, NOISE))
    add([mu.ring((5, 5, 5)), helix(7, (3, 12, 12))], mu.cubic(30.0), 500, hydrogens=True)
    add([helix(5, (3 + 9 * (k % 4), 3 + 9 * (k // 4), 5)) for k in range(11)], mu.cubic(40.0), 600)
    return crystals, np.concatenate(rows).astype(np.float32)


def rel(a, b):
    """max |a - b| / max |b|"""
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())
