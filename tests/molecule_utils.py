"""Hand-built molecular crystals and the numpy references shared by the molecule tests: zig-zag chains, a ring, a polymer
through a cell face, ``bonds.molecules_host`` on a batch's arrays and the fp64 restatement of the pair test."""
import numpy as np

TOL, THRESHOLD = 0.4, 1e-3
STEP, ZIG = 1.25, 0.8            # a zig-zag chain: bonds of 1.484 A (C-C: up to 1.92 A), second neighbours at 2.5 A


def cubic(a):
    return np.eye(3) * a


def on_grid(pos):
    """Positions on a grid of 2^-10 A: with a cell of whole Angstroms every image and every difference of two of them is
    exact in fp32, so an edge and its reverse are exact negatives and a tree's closure gaps are rounding of fp64 sums."""
    return np.round(np.asarray(pos, dtype=np.float64) * 1024.0) / 1024.0


def chain(n, start, cell, drift=(0.0, 0.0), reverse=False):
    """``n`` carbons in a zig-zag along x from ``start``, drifting by ``drift`` (y, z) per atom, wrapped into the
    orthogonal ``cell``; numbered along the chain, or with ``reverse`` from its far end.  Returns ``(pos, true)``: the
    wrapped and the unwrapped positions."""
    k = np.arange(n, dtype=np.float64)
    true = on_grid(np.asarray(start, dtype=np.float64)
                   + np.stack([STEP * k, ZIG * (k % 2) + drift[0] * k, drift[1] * k], axis=1))
    if reverse:
        true = true[::-1].copy()
    return np.mod(true, np.diag(cell)), true


def ring(centre, radius=1.39, n=6):
    a = 2 * np.pi * np.arange(n) / n + 0.3
    return on_grid(np.asarray(centre, dtype=np.float64)
                   + radius * np.stack([np.cos(a), np.sin(a), 0.1 * np.cos(2 * a)], axis=1))


def polymer(n=8):
    """``n`` (even) carbons per cell in a zig-zag along a whose last atom bonds to the first atom's image."""
    cell = np.diag([STEP * n, 12.0, 12.0])
    return chain(n, (0.3, 5.0, 5.0), cell)[0], cell, np.full(n, 6)


def pair_test_crystals():
    """Four crystals for the pair test, all carbon: molecules of 17, 2 and 1 atoms in one cell; molecules of 130 and 65
    atoms in one cell, their atoms interleaved by a fixed permutation; the polymer; a chain of 5 (the test cuts one of its
    directions).  Sizes 1, 2, 17, 65, 130: untested, one pair, a ragged 16-lane pass, past one and two wave strides."""
    a = np.concatenate([chain(17, (3.0, 3.0, 3.0), cubic(30.0))[0], chain(2, (3.0, 12.0, 12.0), cubic(30.0))[0],
                        on_grid([[3.0, 20.0, 20.0]])])
    long_cell = np.diag([180.0, 20.0, 20.0])
    b = np.concatenate([chain(130, (2.0, 5.0, 5.0), long_cell)[0], chain(65, (2.0, 12.0, 12.0), long_cell)[0]])
    b = b[np.random.default_rng(5).permutation(len(b))]
    return [(a, cubic(30.0), np.full(len(a), 6)), (b, long_cell, np.full(len(b), 6)), polymer(8),
            (chain(5, (3.0, 3.0, 3.0), cubic(30.0))[0], cubic(30.0), np.full(5, 6))]


def rigid_body_rows(true, seed):
    """``U_i = T + [r_i]x L [r_i]x^T`` for the unwrapped positions ``true`` about their centroid: ``T`` symmetric positive
    definite (A^2), ``L`` positive semidefinite (rad^2), at the scale of ``predict_utils.spd_rows``; fp64 [n,3,3]."""
    rng = np.random.default_rng(seed)
    a, b = rng.standard_normal((3, 3)), rng.standard_normal((3, 2))
    T, L = 0.01 * a @ a.T + 0.005 * np.eye(3), 1e-4 * b @ b.T
    r = true - true.mean(axis=0)
    cross = np.zeros((len(r), 3, 3))
    cross[:, 0, 1], cross[:, 0, 2], cross[:, 1, 2] = -r[:, 2], r[:, 1], -r[:, 0]
    cross -= cross.transpose(0, 2, 1)
    return T + cross @ L @ cross.transpose(0, 2, 1)


def atom_rows(mask):
    mask = np.asarray(mask, dtype=bool)
    return np.where(mask, np.cumsum(mask) - 1, -1)


def host_molecules(batch, tol=TOL):
    """``bonds.molecules_host`` on the arrays of a dict batch (torch tensors on any device), with the margins of its two
    decisions: ``(result, bond distance margin, closure discrepancies of the bonds with equal labels)``."""
    from cartnet_amd.bonds import COVALENT_RADII, molecules_host
    z, mask = batch["x"].cpu().numpy(), batch["non_H_mask"].cpu().numpy()
    ei, ptr = batch["edge_index"].cpu().numpy(), batch["ptr"].cpu().numpy()
    dist, dirs = batch["cart_dist"].cpu().numpy(), batch["cart_dir"].cpu().numpy()
    row = atom_rows(mask)
    ref = molecules_host(z, ei, dist, dirs, row, ptr, tol)
    src, tgt = ei
    r = np.asarray(COVALENT_RADII, dtype=np.float32)
    can = (src != tgt) & (z[src] > 1) & (z[src] < len(r)) & (z[tgt] > 1) & (z[tgt] < len(r))
    limit = (r[np.where(can, z[tgt], 0)] + r[np.where(can, z[src], 0)]) + np.float32(tol)
    margin = np.abs(dist.astype(np.float64) - limit.astype(np.float64))[can].min() if can.any() else np.inf
    bond = can & (dist <= limit) & (row[src] >= 0) & (row[tgt] >= 0) & (ref["label"][src] == ref["label"][tgt])
    v = dist[bond].astype(np.float64)[:, None] * dirs[bond].astype(np.float64)
    gaps = np.linalg.norm(ref["x"][tgt[bond]] - (ref["x"][src[bond]] + v), axis=1)
    return ref, margin, gaps


def pair_reference(u, label, x, mask, size, status, threshold=THRESHOLD):
    """The pair test in fp64 numpy on the arrays the kernel reads (``u`` fp32 [M,3,3]; ``label``, ``x`` per atom;
    ``size``, ``status`` per row): the per-row figures and every counted ``|D|``."""
    U = np.asarray(u, dtype=np.float64)
    S = 0.5 * (U + U.transpose(0, 2, 1))
    row = atom_rows(mask)
    M = len(U)
    out = {"pairs": np.zeros(M, np.int32), "delta_sum": np.zeros(M), "delta_max": np.zeros(M),
           "worst": np.full(M, -1, np.int64), "over": np.zeros(M, np.int32)}
    deltas = []
    for i in np.nonzero(row >= 0)[0]:
        m = row[i]
        if status[m] != 0 or size[m] < 2:
            continue
        for j in np.nonzero(label == label[i])[0]:                            # atom order
            r = x[i] - x[j]
            rr = r @ r
            if j == i or rr == 0.0:
                continue
            a = abs(r @ (S[m] - S[row[j]]) @ r / rr)
            deltas.append(a)
            out["pairs"][m] += 1
            out["delta_sum"][m] += a
            out["over"][m] += a > threshold
            if out["worst"][m] < 0 or a > out["delta_max"][m]:                # a tie keeps the lower atom
                out["delta_max"][m], out["worst"][m] = a, j
    return out, np.asarray(deltas)
