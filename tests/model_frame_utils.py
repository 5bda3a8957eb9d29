"""Fixtures and host forms shared by tests/test_model_frame_host.py and tests/test_gpu_model_frame*.py: four small
triclinic crystals (stored reduced and unreduced, in standard and in rotated settings), the smallest iComformer of
tests/icomformer_utils.py, and ``cartnet_adp_stored_frame`` restated on the host with the kernel's own operations."""
import math
from fractions import Fraction

import numpy as np
import torch

import icomformer_utils as iu
from predict_utils import cell_from_parameters, fixed_rotation, spd_rows

from cartnet_amd.data import Data, lattice_basis, lattice_margins, optimize_lattice
from cartnet_amd.synthetic import radius_graph_pbc_single

RADIUS = 5.0
TEMP_MEAN, TEMP_STD = 180.0, 60.0                 # what the tests' loaders standardise the stored Kelvin values with

# (cell parameters of the reduced description: lengths pairwise >= 10 % apart, angles away from 90; the integer matrix the
#  stored cell is that description multiplied by, None = stored as it is; whether the stored cell is rotated out of the
#  standard setting; atomic numbers; Kelvin)
CRYSTALS = (
    ((6.0, 7.5, 9.2, 80.0, 75.0, 70.0), None, False, (6, 8, 7, 6, 16), 120.0),                       # reduced, R ~ I
    ((5.5, 6.8, 8.6, 78.0, 83.0, 72.0), ((1, 1, 0), (0, 1, 0), (0, 0, 1)), True,
     (6, 1, 1, 8, 6, 1, 7, 1, 6, 1, 1, 8), 200.0),                                                   # a' = a + b, hydrogens
    ((5.2, 6.4, 7.9, 74.0, 81.0, 67.0), ((1, 0, 0), (0, 1, 0), (-1, 1, 1)), True, (8, 6, 7), 290.0),  # c' = c - a + b
    ((6.3, 7.7, 9.6, 82.0, 73.0, 77.0), None, True, (6, 6, 6, 6, 6, 6, 9, 17), 150.0),               # reduced, rotated
)
HELIX = (3, 6)                # crystal 3: its first six atoms are one bonded chain (a molecule the TLS fit takes)
UNREDUCED = (1, 2)
REDUCED_IN_PLACE = 0


def second_rotation() -> np.ndarray:
    """Another generic proper rotation: Rodrigues about (-2, 1, 1.5) by 2.1 rad."""
    k = np.array([-2.0, 1.0, 1.5])
    k /= np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(2.1) * K + (1 - np.cos(2.1)) * K @ K


def crystals(labeled: bool, restored: bool = False, rotate: bool = True) -> list:
    """The four crystals with their radius graphs (built on the host, uncapped).  ``restored``: each one a second time,
    the same atoms and edges in a frame rotated by ``restore_rotations()[g]`` (``v' = v Q`` for ``pos``, ``cell`` and
    ``cart_dir``) and with another integer basis of the same lattice; with ``rotate=False`` only the basis changes
    (Q = I: the same Cartesian frame, as two CIF settings of one structure that share their axes' orientation)."""
    out = []
    for g, (par, basis, rotated, zs, kelvin) in enumerate(CRYSTALS):
        gen = torch.Generator().manual_seed(4100 + g)
        cell = cell_from_parameters(*par)
        frac = torch.rand(len(zs), 3, generator=gen, dtype=torch.float64).numpy()
        pos = frac @ cell
        last = 0
        for i, zi in enumerate(zs):                              # a hydrogen sits 1 A from the non-hydrogen atom before it
            if zi != 1:
                last = i
            else:
                v = torch.randn(3, generator=gen, dtype=torch.float64).numpy()
                pos[i] = pos[last] + v / np.linalg.norm(v)
        if g == HELIX[0]:                                        # 1.72 A between neighbours, 2.87 A between second ones
            k = np.arange(HELIX[1])
            turn = np.radians(100.0) * k
            pos[:HELIX[1]] = 0.5 * cell.sum(0) + np.stack([0.8 * np.cos(turn), 0.8 * np.sin(turn), 1.2 * (k - 2.5)], axis=1)
        if basis is not None:
            cell = np.array(basis, dtype=np.float64) @ cell
        if rotated:
            Q0 = fixed_rotation()
            cell, pos = cell @ Q0, pos @ Q0
        cell32, pos32 = torch.from_numpy(np.float32(cell)), torch.from_numpy(np.float32(pos))
        ei, dist, direction = radius_graph_pbc_single(pos32, cell32, RADIUS)
        x = torch.tensor(zs, dtype=torch.int64)
        d = Data(x=x, pos=pos32, cell=cell32.unsqueeze(0), edge_index=ei, cart_dist=dist, cart_dir=direction,
                 natoms=torch.tensor([len(zs)]), temperature=torch.tensor([kelvin], dtype=torch.float32))
        if restored:
            Q = torch.from_numpy(np.float32(restore_rotations()[g])) if rotate else torch.eye(3)
            T = torch.tensor(RESTORE_BASES[g], dtype=torch.float32)
            d.pos, d.cell, d.cart_dir = d.pos @ Q, ((T @ d.cell[0]) @ Q).unsqueeze(0), d.cart_dir @ Q
        if labeled:
            d.non_H_mask = x != 1
            d.y = spd_rows(int((x != 1).sum()), 4200 + g)
        out.append(d)
    return out


RESTORE_BASES = (((1, 0, 0), (1, 1, 0), (0, 0, 1)), ((1, 0, 0), (0, 1, 0), (0, 1, 1)), ((1, 0, 0), (0, 1, 0), (1, 0, 1)),
                 ((1, 0, 1), (0, 1, 0), (0, 0, 1)))              # unimodular, applied to the stored cell's rows


def restore_rotations() -> list:
    """One proper rotation per crystal for ``crystals(restored=True)``, fp64 (the fp32 rounding of it is what is applied)."""
    a, b = fixed_rotation(), second_rotation()
    return [np.float64(np.float32(q)) for q in (b, a @ b, b @ a, b @ b)]


def check_crystals(items: list) -> None:
    """What the issue asks of the fixture, on the CPU: no ties in the canonical choice (host and device then pick the same
    basis), one crystal stored reduced (basis and rotation the identity), two stored unreduced (neither is)."""
    eye = torch.eye(3, dtype=torch.int64)
    for g, d in enumerate(items):
        c = d.cell[0]
        gap, cos = lattice_margins(c)
        assert gap >= 1e-3 and cos >= 1e-3, (g, gap, cos)
        basis, (_, R) = lattice_basis(c), optimize_lattice(c)
        if g == REDUCED_IN_PLACE:
            assert torch.equal(basis, eye) and float((R - torch.eye(3)).abs().max()) <= 1e-6, (g, basis, R)
        if g in UNREDUCED:
            assert not torch.equal(basis.abs(), eye) and float((R - torch.eye(3)).abs().max()) > 0.1, (g, basis, R)


def model_and_weights():
    """(dim_in, state dict) of the smallest iComformer tests/icomformer_utils.py builds."""
    z, _, sd = iu.load("icomformer_tiny")
    return int(z["hp_dim_in"]), sd


# ---------------------------------------------------------------------------------------------- the kernel on the host
def _fma(a: float, b: float, c: float) -> float:
    """a * b + c with one rounding, exactly (Fraction is exact, float() of it rounds to nearest even); NaN and inf as fma."""
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    r = float(Fraction(a) * Fraction(b) + Fraction(c))
    return r if r != 0.0 else a * b + c                  # the sign of an exact zero: as the two-step form gives it


def member_host(p, r) -> list:
    """``fm_member`` of csrc/frame_ops.hip on nine fp32 values each: U = R P R^T in fp64 with its operations in its order --
    t = P R^T, then R t, each element a chain of two fma on the first product."""
    P, R = [float(v) for v in p], [float(v) for v in r]
    t = [_fma(P[a * 3 + 2], R[c * 3 + 2], _fma(P[a * 3 + 1], R[c * 3 + 1], P[a * 3] * R[c * 3]))
         for a in range(3) for c in range(3)]
    return [_fma(R[a * 3 + 2], t[6 + c], _fma(R[a * 3 + 1], t[3 + c], R[a * 3] * t[c])) for a in range(3) for c in range(3)]


def stored_frame_host(pred, rotation, row_ptr, slices: int = 1) -> np.ndarray:
    """``cartnet_adp_stored_frame`` on the host: pred [T*M,3,3] fp32, rotation [B,3,3] fp32, row_ptr [B+1] -> [T*M,3,3]
    fp32, every element the fp64 value of ``member_host`` rounded once."""
    pred = np.asarray(pred, dtype=np.float32).reshape(-1, 9)
    rot = np.asarray(rotation, dtype=np.float32).reshape(-1, 9)
    ptr = [int(v) for v in np.asarray(row_ptr).tolist()]
    M = pred.shape[0] // slices
    assert M * slices == pred.shape[0] and ptr[0] == 0 and ptr[-1] == M
    out = np.empty_like(pred)
    for t in range(slices):
        for g in range(len(ptr) - 1):
            for i in range(ptr[g], ptr[g + 1]):
                out[t * M + i] = np.array(member_host(pred[t * M + i], rot[g]), dtype=np.float64).astype(np.float32)
    return out.reshape(-1, 3, 3)


def bits(a) -> bytes:
    return np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a).tobytes()
