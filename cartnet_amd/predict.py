"""ADPs for crystals that have no targets, in the convention crystallographic tools read.

``predict_adps`` is the prediction-side counterpart of ``evaluate.inference``: per batch of a resident shard (labeled or
not) one forward, one ``adp_export`` (csrc/export_ops.hip: the predictions on the unit reciprocal axes -- the inverse of the
transform the reference applied to the dataset's targets, dataset/extract_csd_data.py:115-123 -- with U_eq and the
principal values / axes), the fractional coordinates, ONE device-to-host copy (``metrics.to_host``) and a split by row
counts on the host.  ``write_cif`` writes one crystal of the result as a P1 CIF.  For crystals that came from CIF files
(``cartnet_amd.symmetry.expand``) the same copy also brings one site-averaged ADP per atom of the asymmetric unit, and
``write_cif_symmetric`` writes the crystal in the file's own setting.  With ``rigid_bond`` the copy also brings Hirshfeld's
rigid-bond figures of the exported ADPs (``metrics.bond_test``, csrc/bond_ops.hip): a plausibility report that needs no truth.
With ``riding_h`` it brings an isotropic U for every hydrogen, a multiple of its parent's exported U_eq
(``metrics.riding_h``, csrc/riding_ops.hip), and both writers fill ``_atom_site_U_iso_or_equiv`` for every atom.
With ``temperatures`` every batch is predicted at T temperatures by one forward over a replica batch, the result has one
entry per crystal and temperature, and the copy also brings a least-squares line per row through the T exports
(``metrics.temp_series``, csrc/series_ops.hip).
With ``rigid_molecule`` the copy also brings the molecules of every crystal -- the components of its bond graph, found on
the GPU, with every atom's unwrapped position -- and the rigid-body test of the exported ADPs over all pairs of atoms of a
molecule (``metrics.molecules``, ``metrics.molecule_test``, csrc/molecule_ops.hip).
With ``tls_fit`` on top of that it brings the TLS fit of every molecule of five or more atoms: the rigid-body tensors T, L
and S that explain the molecule's exported ADPs best, the ADP that rigid body gives every atom and what is left over
(``metrics.tls_fit``, csrc/tls_ops.hip).
With ``aniso_h`` on top of ``riding_h`` it brings a full tensor for every hydrogen -- its parent's exported tensor, the change
of the molecule's fitted rigid-body motion from the parent to the hydrogen where ``tls_fit`` gave one, and a nominal internal
X-H motion (``metrics.aniso_h``, csrc/aniso_h_ops.hip) -- and both writers give such a hydrogen an anisotropic row.
Around the pass, for ``main.py --predict``: ``load_input`` (a shard file, or CIF files expanded in memory),
``parse_temperatures`` (the flag's SPEC) and ``pass_statistics`` (the result line).  ``frame_stage`` is the forward in K
frames that this pass and ``evaluate.inference`` share.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional

import torch

from .metrics import (adp_export, aniso_h as aniso_h_call, batch_graph, bond_test, check_export_status,
                      check_temperatures, edge_row_ptr, frame_mean, molecule_test, molecules as find_molecules, riding_h as riding_h_call,
                      rotate_rows, split_rows, target_row_ptr, temp_series, tls_fit as tls_fit_call, to_host)

KEYS = ("name", "atoms", "frac", "z", "cell", "temp", "u_cart", "u_cif", "u_eq", "principal", "axes", "stats")
SYM_KEYS = ("asym_labels", "asym_frac", "asym_z", "u_cif_asym", "spread", "symops")      # with a CifSymmetry only
ROT_KEYS = ("rot_spread", "frames", "rot_stats")                                          # with rotations > 1 only
BOND_KEYS = ("bond_count", "bond_delta_mean", "bond_delta_max", "bond_worst", "bond_over", "bond_ueq_ratio",
             "bond_stats")                                                                # with rigid_bond only
H_KEYS = ("u_iso", "h_parent", "h_count", "h_mult", "h_stats")                            # with riding_h only
H_SYM_KEYS = ("u_iso_asym", "h_parent_asym")                                              # ... and a CifSymmetry
MOL_KEYS = ("mol", "mol_size", "mol_status", "mol_pos", "mol_pairs", "mol_delta_mean", "mol_delta_max", "mol_worst",
            "mol_over", "mol_stats")                                                      # with rigid_molecule only
TLS_KEYS = ("tls_u", "tls_resid", "tls_T", "tls_L", "tls_S", "tls_origin", "tls_T_principal", "tls_L_principal",
            "tls_rank", "tls_r", "tls_stats")                                            # with tls_fit only
AH_KEYS = ("h_u_cart", "h_u_cif", "h_u_eq", "h_source", "h_aniso_stats")               # with aniso_h only
AH_SYM_KEYS = ("h_u_cif_asym",)                                                           # ... and a CifSymmetry
SERIES_KEYS = ("t_slope", "t_intercept", "t_ueq_slope", "t_ueq_intercept", "t_resid", "t_drops", "t_stats")
# with two or more temperatures the result has one more key, "series": a dict of lists, one entry per input crystal, with
# "name", "temps" and SERIES_KEYS

SYMBOLS = ("X H He Li Be B C N O F Ne Na Mg Al Si P S Cl Ar K Ca Sc Ti V Cr Mn Fe Co Ni Cu Zn Ga Ge As Se Br Kr Rb Sr Y Zr "
           "Nb Mo Tc Ru Rh Pd Ag Cd In Sn Sb Te I Xe Cs Ba La Ce Pr Nd Pm Sm Eu Gd Tb Dy Ho Er Tm Yb Lu Hf Ta W Re Os Ir Pt "
           "Au Hg Tl Pb Bi Po At Rn Fr Ra Ac Th Pa U Np Pu Am Cm Bk Cf Es Fm Md No Lr Rf Db Sg Bh Hs Mt Ds Rg Cn Nh Fl Mc "
           "Lv Ts Og").split()


def _inverse_cells(cell: torch.Tensor) -> torch.Tensor:
    """inv(cell) for [B,3,3] cells by the adjugate (its columns are the reciprocal vectors): plain torch on the device."""
    a, b, c = cell.unbind(1)
    adj = torch.stack((torch.linalg.cross(b, c), torch.linalg.cross(c, a), torch.linalg.cross(a, b)), dim=2)
    det = (a * torch.linalg.cross(b, c)).sum(1)
    return adj / det.view(-1, 1, 1)


def frames(B: int, K: int, gen: torch.Generator, device) -> torch.Tensor:
    """[K,B,3,3] fp32 on ``device``: the K frames of B crystals.  Frame 0 is the identity for every crystal (the frame the
    crystal is stored in); frames 1 ... K-1 come from ONE ``shard.random_rotations`` draw of ``(K-1)*B`` matrices."""
    from .shard import random_rotations
    if B < 1 or K < 1:
        raise ValueError("frames needs B >= 1 crystals and K >= 1 frames")
    out = torch.eye(3, dtype=torch.float32, device=device).repeat(K, B, 1, 1)
    if K > 1:
        out[1:] = random_rotations((K - 1) * B, gen, device).view(K - 1, B, 3, 3)
    return out


def replicate(batch, K: int, R: Optional[torch.Tensor]):
    """``batch`` (on the device, atomic numbers in ``x``) K times over as ONE batch of ``K*B`` crystals with PyG's offsets,
    replica-major: crystal ``k*B + g`` is crystal g with ``cart_dir @ R[k, g]`` (one ``rotate_rows`` over the replica
    batch's edge segments: the arithmetic of ``DeviceShard.collate(list(sel) * K, R.view(K*B,3,3))``).  Everything else
    (``x``, ``cart_dist``, ``pos``, ``non_H_mask``, ``cell``, ``temperature``, ``y``) is repeated.  ``R = None``: no frame
    but the stored one, ``cart_dir`` is repeated as well (its bits, no rotation by the identity).  Plain torch on the
    device; ``batch`` is not modified.  Works on a batch of either loader (``ShardLoader``, ``data.DataLoader``)."""
    B, N, E = int(batch.num_graphs), int(batch.x.shape[0]), int(batch.edge_index.shape[1])
    dev = batch.x.device
    if R is not None and not (torch.is_tensor(R) and tuple(R.shape) == (K, B, 3, 3)):
        raise ValueError("R must be a tensor [K,B,3,3]")
    if K < 1:
        raise ValueError("replicate needs K >= 1 replicas")
    if batch.x.dtype != torch.int64 or batch.x.dim() != 1:
        raise ValueError("replicate needs the atomic numbers in batch.x (a forward has overwritten them)")
    k = torch.arange(K, dtype=torch.int64, device=dev)
    out = batch.__class__()
    out.x = batch.x.repeat(K)
    out.batch = (batch.batch.unsqueeze(0) + (k * B).unsqueeze(1)).reshape(-1)
    zero = torch.zeros(1, dtype=torch.int64, device=dev)
    out.ptr = torch.cat([zero, (batch.ptr[1:].to(torch.int64).unsqueeze(0) + (k * N).unsqueeze(1)).reshape(-1)])
    out.edge_index = (batch.edge_index.unsqueeze(1) + (k * N).view(1, K, 1)).reshape(2, K * E)
    out.cart_dist = batch.cart_dist.repeat(K)
    if R is None:
        out.cart_dir = batch.cart_dir.repeat(K, 1)
    else:
        edge_ptr = torch.cat([zero, (edge_row_ptr(batch)[1:].unsqueeze(0) + (k * E).unsqueeze(1)).reshape(-1)])
        out.cart_dir = rotate_rows(batch.cart_dir.repeat(K, 1).contiguous(), edge_ptr,
                                   R.reshape(K * B, 3, 3).to(torch.float32))
    for name in ("pos", "non_H_mask", "cell", "temperature", "y"):
        t = getattr(batch, name, None)
        if torch.is_tensor(t):
            setattr(out, name, t.repeat(K, *([1] * (t.dim() - 1))))
    out.num_graphs = K * B
    return out


def frame_stage(model, batch, row_ptr: torch.Tensor, rotations: int, gen, stats: bool):
    """The prediction of ``batch`` (on the device, atomic numbers in ``x``) in ``rotations`` = K frames: K = 1 is the plain
    forward; K > 1 is ONE forward of ``replicate(batch, K, R)`` with ``R = frames(B, K, gen, device)`` and the members'
    ``metrics.frame_mean`` (``stats``: its per-crystal figures as well).  Returns ``(pred, R, FrameMean)``, the last two
    ``None`` for K = 1; ``batch`` comes back with its atomic numbers in ``x`` (a forward puts the features there: it
    replaces the tensor and writes into nothing, so no copy is taken)."""
    if rotations == 1:
        atoms = batch.x
        pred, _ = model(batch)
        batch.x = atoms
        return pred, None, None
    R = frames(int(batch.num_graphs), rotations, gen, batch.x.device)
    members, _ = model(replicate(batch, rotations, R))                        # batch.x stays: the replica's is overwritten
    fm = frame_mean(members, R, row_ptr, stats=stats)
    return fm.mean, R, fm


def parse_temperatures(spec: str) -> list:
    """``--predict_temperatures SPEC`` as a list of Kelvin values: ``100,150,200``, or ``A:B:STEP`` = A, A + STEP, ... up
    to and including B when STEP reaches it (``100:300:50`` is five values, ``100:290:50`` four).  Raises ``SystemExit``
    with a message for an empty spec, a value that is no number, one that is not finite or not > 0, a list that is not
    strictly increasing and a STEP that is not > 0.  On the host: no device is touched."""
    flag = "--predict_temperatures"

    def number(text: str) -> float:
        try:
            v = float(text)
        except ValueError:
            raise SystemExit(f"{flag}: {text.strip()!r} is no number") from None
        if not math.isfinite(v):
            raise SystemExit(f"{flag}: {text.strip()!r} is not finite")
        return v
    spec = (spec or "").strip()
    if not spec:
        raise SystemExit(f"{flag}: empty (a list 100,150,200 or a range A:B:STEP)")
    if ":" in spec:
        parts = spec.split(":")
        if len(parts) != 3:
            raise SystemExit(f"{flag}: a range is A:B:STEP, got {spec!r}")
        a, b, step = (number(p) for p in parts)
        if step <= 0:
            raise SystemExit(f"{flag}: STEP must be > 0, got {step:g}")
        count = math.floor((b - a) / step + 1e-9) + 1                        # B itself when STEP reaches it
        if count < 1:
            raise SystemExit(f"{flag}: the range {spec!r} is empty")
        values = [a + k * step for k in range(count)]
    else:
        values = [number(p) for p in spec.split(",")]
    if any(v <= 0 for v in values):
        raise SystemExit(f"{flag}: temperatures are Kelvin values > 0")
    if any(q <= p for p, q in zip(values, values[1:])):
        raise SystemExit(f"{flag}: the temperatures must be strictly increasing")
    return values


def standardised(temperatures, temp_mean: float, temp_std: float, device) -> torch.Tensor:
    """[T] fp32 on ``device``: ``(fp32(T_t) - fp32(mean)) / fp32(std)`` with both steps rounded to fp32, taken on the host:
    the bits the collation kernel gives a crystal stored at ``T_t`` (csrc/collate.hip: ``__fdiv_rn(__fsub_rn(...))``)."""
    import numpy as np
    t = (np.asarray(temperatures, dtype=np.float32) - np.float32(temp_mean)) / np.float32(temp_std)
    return torch.from_numpy(t.astype(np.float32)).to(device)


def replicate_temperatures(batch, temps: torch.Tensor, K: int = 1, R: Optional[torch.Tensor] = None):
    """``batch`` at the T model-side temperatures ``temps`` ([T] fp32 on the device: ``standardised``) and in K frames as
    ONE batch of ``T*K*B`` crystals, temperature-major, then frame, then crystal: crystal ``(t*K + k)*B + g`` is crystal g
    with ``cart_dir @ R[k, g]`` and ``temperature = temps[t]``.  The T temperatures share the K frames ``R`` [K,B,3,3];
    ``R = None`` (K = 1) rotates nothing.  ``replicate`` does the rest; ``batch`` is not modified."""
    T, B = int(temps.shape[0]), int(batch.num_graphs)
    if not (temps.dim() == 1 and T >= 1 and temps.dtype == torch.float32 and temps.device == batch.x.device):
        raise ValueError("temps must be an fp32 tensor [T], T >= 1, on the batch's device")
    if R is None and K != 1:
        raise ValueError("K frames need their rotations R [K,B,3,3]")
    out = replicate(batch, T * K, None if R is None else R.repeat(T, 1, 1, 1))
    out.temperature = temps.repeat_interleave(K * B)
    return out


def _in_crystal(index: torch.Tensor, batch) -> torch.Tensor:
    """Atom indices of the batch (a bond's partner, a hydrogen's parent: atoms of the crystal they are recorded in) as atom
    indices inside that crystal; -1 (no atom) is kept."""
    at = index.clamp(min=0)
    return torch.where(index >= 0, at - batch.ptr.to(torch.int64)[batch.batch[at]], index)


def bond_entries(bt, batch) -> dict:
    """The per-row keys of ``BOND_KEYS`` (and ``bond_stats`` per crystal) from a ``metrics.BondTest`` of ``batch``, on the
    device: ``bond_delta_mean`` = ``delta_sum / bonds`` (0 without bonds), ``bond_worst`` as an atom index inside its
    crystal (-1 without bonds).  Static-shape device ops: nothing is read back."""
    return {"bond_count": bt.bonds, "bond_delta_max": bt.delta_max, "bond_over": bt.over, "bond_ueq_ratio": bt.ueq_ratio,
            "bond_delta_mean": bt.delta_sum / bt.bonds.clamp(min=1).to(torch.float32),      # delta_sum is 0 without bonds
            "bond_worst": _in_crystal(bt.worst, batch), "bond_stats": bt.crystal_stats}


def riding_entries(rh, batch) -> dict:
    """The per-atom keys of ``H_KEYS`` (and ``h_stats`` per crystal) from a ``metrics.RidingH`` of ``batch``, on the device:
    ``h_parent`` as an atom index inside its crystal (-1 where there is none), converted as ``bond_entries`` converts
    ``bond_worst``.  Static-shape device ops: nothing is read back."""
    return {"u_iso": rh.u_iso, "h_parent": _in_crystal(rh.parent, batch), "h_count": rh.count, "h_mult": rh.mult,
            "h_stats": rh.crystal_stats}


def molecule_entries(mo, mt, batch) -> dict:
    """The keys of ``MOL_KEYS`` from the ``metrics.Molecules`` of ``batch`` and a ``metrics.MoleculeTest`` on them, on the
    device: ``mol_pos`` = ``fp32(x)`` of the row's atom, NaN where the molecule's status is not 0; ``mol_delta_mean`` =
    ``delta_sum / pairs`` (0 without pairs); ``mol_worst`` as an atom index inside its crystal (-1 without pairs);
    ``mol_stats`` [B,9] = the five counts of the molecules, then the four figures of the test.  Static-shape device ops:
    nothing is read back."""
    pos = mo.x[batch.non_H_mask].to(torch.float32)
    return {"mol": mo.mol, "mol_size": mo.size, "mol_status": mo.status,
            "mol_pos": torch.where((mo.status == 0).unsqueeze(1), pos, torch.full_like(pos, float("nan"))),
            "mol_pairs": mt.pairs, "mol_delta_mean": mt.delta_sum / mt.pairs.clamp(min=1).to(torch.float32),
            "mol_delta_max": mt.delta_max, "mol_worst": _in_crystal(mt.worst, batch), "mol_over": mt.over,
            "mol_stats": torch.cat([mo.crystal_counts, mt.crystal_stats], dim=1)}


_SYM6 = (0, 5, 4, 5, 1, 3, 4, 3, 2)               # a row-major symmetric 3x3 from its 11 22 33 23 13 12


def tls_entries(tf) -> dict:
    """The keys of ``TLS_KEYS`` from a ``metrics.TlsFit``, on the device: ``params`` cut into ``tls_T`` / ``tls_L`` /
    ``tls_S`` [M,3,3] and ``tls_origin`` [M,3], ``eig`` into the two triples of principal values.  Static-shape device ops:
    nothing is read back."""
    M = int(tf.params.shape[0])
    return {"tls_u": tf.u_tls, "tls_resid": tf.resid, "tls_T": tf.params[:, 0:6][:, _SYM6].reshape(M, 3, 3),
            "tls_L": tf.params[:, 6:12][:, _SYM6].reshape(M, 3, 3), "tls_S": tf.params[:, 12:21].reshape(M, 3, 3),
            "tls_origin": tf.params[:, 21:24], "tls_T_principal": tf.eig[:, 0:3], "tls_L_principal": tf.eig[:, 3:6],
            "tls_rank": tf.rank, "tls_r": tf.rfac, "tls_stats": tf.crystal_stats}


def aniso_entries(ah, batch) -> dict:
    """The keys of ``AH_KEYS`` from a ``metrics.AnisoH`` of ``batch``, on the device: one ``adp_export`` over ATOMS as rows
    (``batch.ptr`` as the row offsets) brings ``u_h`` into CIF convention with its equivalent isotropic value.  Rows without
    a tensor are NaN and stay NaN: the export's Jacobi has a fixed number of sweeps.  Nothing is read back."""
    ex = adp_export(ah.u_h, batch.ptr.to(torch.int64), batch.cell, axes=False, stats=False, check=False)
    return {"h_u_cart": ah.u_h, "h_u_cif": ex.u_cif, "h_u_eq": ex.u_eq, "h_source": ah.source,
            "h_aniso_stats": ah.crystal_stats}


def aniso_asym(asym_z, u_cif_asym, h_u_cif) -> torch.Tensor:
    """[a,6] fp32: the tensors of one crystal from a CIF per atom of its asymmetric unit, on the host.  A non-hydrogen atom
    gets its site's ``u_cif_asym`` (the orbit mean); hydrogen ``k`` gets expanded atom ``k``'s ``h_u_cif`` -- the first
    ``a`` expanded atoms are the asymmetric unit under the identity, which ``riding_asym`` has verified.  A hydrogen's
    tensor is NOT averaged over its orbit: it is the one of the image the file lists."""
    asym_z = torch.as_tensor(asym_z).to(torch.int64)
    heavy = asym_z != 1
    site = (torch.cumsum(heavy, 0) - 1).clamp(min=0)
    n = int(asym_z.shape[0])
    own = u_cif_asym[site] if int(u_cif_asym.shape[0]) else torch.full((n, 6), float("nan"))
    return torch.where(heavy.unsqueeze(1), own, h_u_cif[:n]).to(torch.float32)


def u_eq_of_cif(u_cif: torch.Tensor, cell: torch.Tensor) -> torch.Tensor:
    """[n] fp64: the equivalent isotropic U of ``u_cif`` [n,6] (U11 U22 U33 U23 U13 U12 on the unit reciprocal axes) in
    ``cell`` ([3,3], or [n,3,3] with one cell per row; rows = lattice vectors):
    ``(1/3) sum_ij U_ij |a*_i| |a*_j| (a_i . a_j)``, the trace of the Cartesian tensor ``sum_ij U_ij |a*_i| |a*_j| a_i a_j^T``
    over three (the inverse of ``adp_export``'s transform; in an orthogonal cell ``|a*_i| = 1 / |a_i|`` and it is the mean
    of the diagonal).  Plain torch, fp64."""
    u, c = u_cif.to(torch.float64), cell.to(torch.float64)
    if c.dim() == 2:
        c = c.unsqueeze(0).expand(u.shape[0], 3, 3)
    n = torch.linalg.norm(_inverse_cells(c), dim=1)                           # |a*_i|: the columns of inv(cell)
    g = (c @ c.transpose(1, 2)) * (n.unsqueeze(2) * n.unsqueeze(1))           # (a_i . a_j) |a*_i| |a*_j|
    return ((u[:, 0] * g[:, 0, 0] + u[:, 1] * g[:, 1, 1] + u[:, 2] * g[:, 2, 2])
            + 2.0 * (u[:, 3] * g[:, 1, 2] + u[:, 4] * g[:, 0, 2] + u[:, 5] * g[:, 0, 1])) / 3.0


def riding_asym(name: str, asym_z, z, h_parent, h_mult, parent_asym, u_eq_sites):
    """The riding hydrogens of one crystal from a CIF, per atom of its asymmetric unit, on the host:
    ``(u_iso_asym [a] fp32, h_parent_asym [a] int64)``.  Candidate ``s * n + a`` with operator 0 the identity
    (csrc/symmetry_ops.hip) makes the first ``a`` atoms of the expanded crystal the asymmetric unit in file order; that is
    checked against ``z`` here and a mismatch raises ``ValueError`` naming the crystal.  The asymmetric hydrogen ``k`` takes
    the parent and the multiplier of expanded atom ``k``; ``parent_asym`` [N] names the asymmetric atom every expanded
    atom's parent is an image of (-1 without a parent), and ``u_eq_sites`` [sites] fp64 is the U_eq of the site-averaged
    tensors, so ``u_iso_asym = mult * U_eq(site of the parent)`` agrees with the anisotropic rows of the same file.
    Non-hydrogen atoms get the U_eq of their own site."""
    asym_z = torch.as_tensor(asym_z).to(torch.int64)
    n = int(asym_z.shape[0])
    if int(z.shape[0]) < n or not torch.equal(z[:n].to(torch.int64), asym_z):
        raise ValueError(f"crystal {name}: the first {n} atoms of the expanded cell are not its asymmetric unit in file order")
    heavy = asym_z != 1
    site = torch.cumsum(heavy, 0) - 1                                         # the site of a non-hydrogen asymmetric atom
    pa = torch.where(heavy, torch.full_like(asym_z, -1), parent_asym[:n].to(torch.int64))
    pa = torch.where((h_parent[:n] >= 0) & (pa >= 0) & (pa < n), pa, torch.full_like(pa, -1))
    ueq = torch.cat([u_eq_sites.to(torch.float64), torch.full((1,), float("nan"), dtype=torch.float64)])
    own = ueq[torch.where(heavy, site, torch.full_like(site, -1))]
    of_parent = h_mult[:n].to(torch.float64) * ueq[torch.where(pa >= 0, site[pa.clamp(min=0)], torch.full_like(pa, -1))]
    return torch.where(heavy, own, of_parent).to(torch.float32), pa


# How every key of the result that travels to the host as a tensor is cut into the crystals' entries: one slice of dim 0
# per "crystal", or the pieces of dim 0 that hold a crystal's atoms ("atom"), its non-hydrogen rows ("row") or the
# non-hydrogen atoms of its asymmetric unit ("site").  The other keys of the result are assembled on the host.
SPLIT = {"atoms": "row", "frac": "atom", "z": "atom", "cell": "crystal", "u_cart": "row", "u_cif": "row", "u_eq": "row",
         "principal": "row", "axes": "row", "stats": "crystal",
         "u_cif_asym": "site", "spread": "site",
         "rot_spread": "row", "frames": "crystal", "rot_stats": "crystal",
         "bond_count": "row", "bond_delta_mean": "row", "bond_delta_max": "row", "bond_worst": "row", "bond_over": "row",
         "bond_ueq_ratio": "row", "bond_stats": "crystal",
         "u_iso": "atom", "h_parent": "atom", "h_count": "atom", "h_mult": "atom", "h_stats": "crystal"}
# The same for the keys of result["series"], which has one entry per input crystal: a table of its own, because SPLIT is
# exactly the tensor keys of an entry (tests/test_cif_writers_golden.py holds it to that).
SERIES_SPLIT = {"t_slope": "row", "t_intercept": "row", "t_ueq_slope": "row", "t_ueq_intercept": "row", "t_resid": "row",
                "t_drops": "row", "t_stats": "crystal"}
# ... and for MOL_KEYS: only "row" and "crystal" keys
MOL_SPLIT = {"mol": "row", "mol_size": "row", "mol_status": "row", "mol_pos": "row", "mol_pairs": "row",
             "mol_delta_mean": "row", "mol_delta_max": "row", "mol_worst": "row", "mol_over": "row", "mol_stats": "crystal"}
# ... and for TLS_KEYS
TLS_SPLIT = {**{k: "row" for k in TLS_KEYS}, "tls_stats": "crystal"}
# ... and for AH_KEYS: per atom, not per row
AH_SPLIT = {**{k: "atom" for k in AH_KEYS}, "h_aniso_stats": "crystal"}


def _check_pass(loader, rotations: int):
    """What ``predict_adps`` requires of its arguments; returns the loader's shard."""
    if rotations < 1:
        raise ValueError("rotations must be at least 1")
    shard = loader.shard
    if not shard.per_atom_target:
        raise ValueError("predict_adps needs an ADP shard (per-atom 3x3 rows)")
    if not all(k in shard.t for k in ("pos", "cell", "non_h_mask")):
        raise ValueError("predict_adps needs the shard's pos, cell and non_h_mask")
    return shard


def parent_asym(parent: torch.Tensor, batch, row_ptr: torch.Tensor, sym) -> torch.Tensor:
    """[N] int64 on the device: for every atom of ``batch`` the atom of the asymmetric unit that its riding parent
    (``RidingH.parent``, an atom index of the batch) is an image of, -1 without a parent: the parent's row in the batch,
    then in the expansion (``sym.y_ptr``), then ``sym.row_asym``."""
    n = int(sym.row_asym.shape[0])
    if not n:
        return torch.full_like(parent, -1)
    first = torch.from_numpy(sym.y_ptr[batch._sel]).to(parent.device)
    p = parent.clamp(min=0)
    row = (torch.cumsum(batch.non_H_mask.to(torch.int64), 0) - 1)[p]
    g = batch.batch[p]
    grow = (first[g] + (row - row_ptr[g])).clamp(0, n - 1)
    return torch.where(parent >= 0, sym.row_asym[grow].to(torch.int64), parent)


def _of_the_batch(batch, row_ptr: torch.Tensor) -> dict:
    """What a batch (on the device, before a forward) sends to the host whatever is predicted for it."""
    z = batch.x.clone()                                                       # forward overwrites x
    return {"z": z, "atoms": z[batch.non_H_mask], "cell": batch.cell, "_sel": batch._meta[:int(batch.num_graphs)],
            "_row_ptr": row_ptr, "_atom_ptr": batch.ptr,
            "frac": (batch.pos.unsqueeze(1) @ _inverse_cells(batch.cell)[batch.batch]).squeeze(1)}


def _device_stage(model, batch, shard, sym, rotations: int, gen, rigid_bond, riding_h, rigid_molecule=None,
                  tls_fit=None, aniso_h=None) -> dict:
    """One batch (on the device) through the forward and the kernels that follow it.  Returns what travels to the host in
    one ``to_host``: tensors under their key of ``SPLIT`` (``MOL_SPLIT``), and under names with a leading underscore what
    ``_host_stage`` needs to cut and check them."""
    row_ptr = target_row_ptr(batch)
    dev = _of_the_batch(batch, row_ptr)
    if "temperature" in shard.t:
        dev["_temp"] = shard.t["temperature"][dev["_sel"]]                    # the collated one is standardised
    pred, R, fm = frame_stage(model, batch, row_ptr, rotations, gen, stats=True)
    if fm is not None:
        dev.update(rot_spread=fm.spread, frames=R.transpose(0, 1), rot_stats=fm.crystal_spread)
    graph, mo = _of_the_graph(batch, row_ptr, int(pred.shape[0]), rigid_bond, riding_h, rigid_molecule)
    dev.update(_exported(pred, batch, row_ptr, sym, rigid_bond, riding_h, graph, mo, rigid_molecule, tls_fit, aniso_h))
    return dev


def _of_the_graph(batch, row_ptr: torch.Tensor, rows: int, rigid_bond, riding_h, rigid_molecule):
    """``(metrics.BatchGraph of the batch, its metrics.Molecules)``, each ``None`` unless a flag needs it: what the analyses
    of ``_exported`` share and what does not depend on U, so checked, built and found once per batch (its atomic numbers in
    ``x``), however many predictions of it follow."""
    if rigid_bond is None and riding_h is None and rigid_molecule is None:
        return None, None
    graph = batch_graph(batch, rows, "predict_adps")
    return graph, None if rigid_molecule is None else find_molecules(graph, row_ptr, rigid_molecule[0])


def _exported(pred: torch.Tensor, batch, row_ptr: torch.Tensor, sym, rigid_bond, riding_h, graph=None, mo=None,
              rigid_molecule=None, tls_fit=None, aniso_h=None) -> dict:
    """The kernels that follow the forward, on the prediction ``pred`` [M,3,3] of ``batch``: the export and, as asked for
    and on ``graph`` and ``mo`` (``_of_the_graph``), the rigid-bond test, the rigid-body test (and the TLS fit) on the
    molecules, the riding hydrogens (and their tensors, with the TLS fit if there is one) and the site average."""
    device = batch.x.device
    B = int(batch.num_graphs)
    sel = batch._meta[:B]
    ex = adp_export(pred, row_ptr, batch.cell, axes=True, stats=True, check=False)
    dev = dict(u_cart=pred, u_cif=ex.u_cif, u_eq=ex.u_eq, principal=ex.principal, axes=ex.axes,
               stats=ex.crystal_stats, _status=ex.status)
    if rigid_bond is not None:
        dev.update(bond_entries(bond_test(pred, graph, row_ptr, *rigid_bond), batch))
    tf = None
    if mo is not None:
        dev.update(molecule_entries(mo, molecule_test(pred, graph, row_ptr, mo, rigid_molecule[1]), batch))
        if tls_fit:
            tf = tls_fit_call(pred, graph, row_ptr, mo)
            dev.update(tls_entries(tf))
    if riding_h is not None:
        rh = riding_h_call(ex.u_eq, graph, *riding_h)
        dev.update(riding_entries(rh, batch))
        if aniso_h is not None:
            ah = aniso_h_call(pred, graph, row_ptr, rh, mo if tf is not None else None, tf, *aniso_h)
            dev.update(aniso_entries(ah, batch))
    if sym is not None:
        from .symmetry import site_average
        dev["u_cif_asym"], dev["spread"] = site_average(pred, row_ptr, batch._sel, sym)
        if riding_h is not None:                                              # what riding_asym takes, per site and per atom
            counts = torch.from_numpy(sym.site_count[batch._sel]).to(device)
            crystal = torch.repeat_interleave(torch.arange(B, device=device), counts,
                                              output_size=int(dev["u_cif_asym"].shape[0]))
            dev["_ueq_asym"] = u_eq_of_cif(dev["u_cif_asym"], sym.cell[sel].view(B, 3, 3)[crystal])
            dev["_parent_asym"] = parent_asym(rh.parent, batch, row_ptr, sym)
    return dev


def _device_stage_series(model, batch, sym, rotations: int, gen, rigid_bond, riding_h, kelvin: list,
                         temps: torch.Tensor, rigid_molecule=None, tls_fit=None, aniso_h=None) -> dict:
    """One batch (on the device) at the T temperatures ``kelvin`` (``temps``: their model-side values, ``standardised``)
    through ONE forward of ``replicate_temperatures`` and the kernels that follow it, those once per temperature on that
    temperature's rows.  Returns what travels to the host in one ``to_host``: what does not depend on the temperature
    under the names of ``_device_stage``, the keys of temperature t under ``"<key>@<t>"`` and, with T >= 2, the keys of
    ``SERIES_KEYS`` (one ``temp_series`` call on the T exports)."""
    B, T = int(batch.num_graphs), len(kelvin)
    row_ptr = target_row_ptr(batch)
    dev = _of_the_batch(batch, row_ptr)
    R = frames(B, rotations, gen, batch.x.device) if rotations > 1 else None
    members, _ = model(replicate_temperatures(batch, temps, rotations, R))    # batch.x stays: the replica's is overwritten
    if R is not None:
        dev["frames"] = R.transpose(0, 1)
    rows = int(members.shape[0]) // T                                         # K*M: one temperature's slice
    graph, mo = _of_the_graph(batch, row_ptr, rows // rotations, rigid_bond, riding_h, rigid_molecule)   # once for all T
    per = []
    for t in range(T):
        pred, d = members[t * rows:(t + 1) * rows], {}
        if R is not None:
            fm = frame_mean(pred, R, row_ptr, stats=True)
            pred = fm.mean
            d.update(rot_spread=fm.spread, rot_stats=fm.crystal_spread)
        d.update(_exported(pred, batch, row_ptr, sym, rigid_bond, riding_h, graph, mo, rigid_molecule, tls_fit, aniso_h))
        per.append(d)
        dev.update({f"{k}@{t}": v for k, v in d.items()})
    if T >= 2:
        ts = temp_series(torch.cat([d["u_cif"] for d in per]), torch.cat([d["u_eq"] for d in per]), kelvin, row_ptr)
        dev.update(t_slope=ts.slope, t_intercept=ts.intercept, t_ueq_slope=ts.ueq_slope,
                   t_ueq_intercept=ts.ueq_intercept, t_resid=ts.resid, t_drops=ts.drops, t_stats=ts.crystal_stats)
    return dev


def _host_stage_series(out: Dict[str, List], series: Dict[str, List], host: dict, shard, sym, kelvin: list) -> None:
    """Appends the entries of one batch to ``out``, crystal-major (crystal g at temperature t is entry ``g*T + t`` of the
    batch), and its crystals to ``series``, from the host copy of ``_device_stage_series``'s dict: one ``_host_stage`` per
    temperature on that temperature's keys."""
    T = len(kelvin)
    shared = {k: v for k, v in host.items() if "@" not in k and k not in SERIES_KEYS}
    B = int(shared["_sel"].shape[0])
    per = []
    for t, kt in enumerate(kelvin):
        mine = {k.rpartition("@")[0]: v for k, v in host.items() if k.endswith(f"@{t}")}
        mine["_temp"] = torch.full((B,), kt, dtype=torch.float64)             # .tolist(): the Kelvin value as given
        per.append({k: [] for k in out})
        names, counts = _host_stage(per[t], {**shared, **mine}, shard, sym)
    for g in range(B):
        for t, kt in enumerate(kelvin):
            for k in out:
                out[k].append(f"{per[t][k][g]}_{kt:g}K" if k == "name" else per[t][k][g])
    if T >= 2:
        _split(series, {k: host[k] for k in SERIES_KEYS}, counts, SERIES_SPLIT)
        series["name"] += names
        series["temps"] += [torch.tensor(kelvin, dtype=torch.float32) for _ in names]


def _split(out: Dict[str, List], host: dict, counts: dict, table: dict = SPLIT) -> None:
    """Appends to ``out[k]`` the crystals' pieces of every host tensor ``host[k]``, cut as ``table[k]`` says."""
    for k, t in host.items():
        kind = table[k]
        out[k] += [c.clone() for c in t.unbind(0)] if kind == "crystal" else split_rows(t, counts[kind])


def _host_stage(out: Dict[str, List], host: dict, shard, sym):
    """Appends the crystals of one batch to ``out`` from the host copy of ``_device_stage``'s dict.  Returns the crystals'
    names and their counts of rows, atoms and sites."""
    ids = host.pop("_sel").tolist()
    names = [shard.names[i] if shard.names is not None else f"crystal{i}" for i in ids]
    check_export_status(host.pop("_status"), names)
    rp, ap = host.pop("_row_ptr"), host.pop("_atom_ptr")
    counts = {"row": (rp[1:] - rp[:-1]).tolist(), "atom": (ap[1:] - ap[:-1]).tolist(),
              "site": [int(sym.site_count[i]) for i in ids] if sym is not None else None}
    out["name"] += names
    out["temp"] += host.pop("_temp").tolist() if "_temp" in host else [float("nan")] * len(ids)
    riding = "_ueq_asym" in host                                              # what riding_asym takes, per site and per atom
    ueq_sites = split_rows(host.pop("_ueq_asym"), counts["site"]) if riding else None
    parents = split_rows(host.pop("_parent_asym"), counts["atom"]) if riding else None
    _split(out, {k: host.pop(k) for k in MOL_KEYS if k in host}, counts, MOL_SPLIT)
    _split(out, {k: host.pop(k) for k in TLS_KEYS if k in host}, counts, TLS_SPLIT)
    _split(out, {k: host.pop(k) for k in AH_KEYS if k in host}, counts, AH_SPLIT)
    _split(out, host, counts)
    if sym is not None:
        out["asym_labels"] += [sym.labels[i] for i in ids]
        out["asym_frac"] += [torch.from_numpy(sym.frac[i]) for i in ids]
        out["asym_z"] += [torch.from_numpy(sym.z[i]) for i in ids]
        out["symops"] += [sym.symops[i] for i in ids]
    if riding:
        for g, i in enumerate(ids):
            k = len(out["z"]) - len(ids) + g
            u, pa = riding_asym(names[g], sym.z[i], out["z"][k], out["h_parent"][k], out["h_mult"][k], parents[g],
                                ueq_sites[g])
            out["u_iso_asym"].append(u)
            out["h_parent_asym"].append(pa)
            if "h_u_cif_asym" in out:
                out["h_u_cif_asym"].append(aniso_asym(sym.z[i], out["u_cif_asym"][k], out["h_u_cif"][k]))
    return names, counts


def predict_adps(model, loader, device, sym=None, rotations: int = 1, seed: int = 0, rigid_bond=None, riding_h=None,
                 temperatures=None, rigid_molecule=None, tls_fit=None, aniso_h=None) -> Dict[str, List]:
    """Predicted ADPs of every crystal of ``loader`` (a ``ShardLoader``; a labeled shard's ``y`` is ignored).  Returns a
    dict of lists with one entry per crystal, in the loader's order: ``name``; ``atoms`` [n] (Z of the n non-hydrogen atoms
    the rows belong to); ``frac`` [N,3] and ``z`` [N] (all atoms); ``cell`` [3,3]; ``temp`` (Kelvin, as stored; NaN if the
    shard has none); ``u_cart`` [n,3,3] (the model's output); ``u_cif`` [n,6] (U11 U22 U33 U23 U13 U12); ``u_eq`` [n];
    ``principal`` [n,3] ascending; ``axes`` [n,3,3]; ``stats`` [3] fp64 (sum of u_eq, smallest principal value, rows with a
    non-positive one).  A singular cell raises ``ValueError`` naming the crystal.  ``sym``: the ``CifSymmetry`` of a shard
    expanded from CIF files; the result then also has, per crystal, ``asym_labels`` / ``asym_frac`` [a,3] / ``asym_z`` [a]
    (the asymmetric unit as the file gives it), ``symops`` (strings, identity first), ``u_cif_asym`` [h,6] (one row per
    non-hydrogen atom of the asymmetric unit, the mean over its orbit, ``symmetry.site_average``) and ``spread`` [h].
    ``rotations`` = K > 1: every batch is predicted in K frames by ONE forward of ``replicate(batch, K, R)`` with
    ``R = frames(B, K, gen, device)`` (one generator seeded with ``seed`` for the whole pass), the members are brought back
    and averaged (``metrics.frame_mean``), and everything above derives from that mean: ``u_cart`` is the mean.  The result
    then also has, per crystal, ``rot_spread`` [n] (per row the largest deviation of a frame's prediction from the mean),
    ``frames`` [K,3,3] (the rotations used, the identity first) and ``rot_stats`` [2] fp64 (sum and maximum of
    ``rot_spread``).  ``rotations`` = 1 is the pass as it always was.  ``rigid_bond`` = ``(tol, threshold)``: one
    ``metrics.bond_test`` per batch on the ``u_cart`` that is exported (with rotations the frame mean; with CIF input the
    rows of the expanded cell, before site averaging), travelling in the same copy.  The result then also has, per crystal,
    ``bond_count`` [n], ``bond_delta_mean`` [n] (mean ``|D|`` over the atom's bonds, 0 without bonds), ``bond_delta_max``
    [n], ``bond_worst`` [n] (the partner of the worst bond as an atom index inside the crystal, -1 without bonds),
    ``bond_over`` [n], ``bond_ueq_ratio`` [n] and ``bond_stats`` [4] fp64 (directed bonds, sum of ``|D|``, largest ``|D|``,
    bonds over the threshold).  ``None`` is the pass as it always was.  ``riding_h`` = ``(tol, f, f_rot)``: one
    ``metrics.riding_h`` per batch on the ``u_eq`` that is exported (with rotations the frame mean's), travelling in the same
    copy.  The result then also has, per crystal, ``u_iso`` [N] (every atom: a hydrogen's ``mult * u_eq[parent]``, NaN for
    an orphan; a non-hydrogen atom's own ``u_eq``), ``h_parent`` [N] (an atom index inside the crystal, -1 where there is
    none), ``h_count`` [N] (hydrogens riding on a non-hydrogen atom), ``h_mult`` [N] and ``h_stats`` [4] fp64 (hydrogens,
    orphans, sum of the finite hydrogen ``u_iso``, hydrogens with a non-positive parent ``u_eq``); with ``sym`` also
    ``u_iso_asym`` [a] and ``h_parent_asym`` [a] per atom of the asymmetric unit (``riding_asym``).  ``None`` is the pass
    as it always was.  ``temperatures`` = T >= 1 Kelvin values (strictly increasing, finite, > 0; otherwise ``ValueError``):
    every batch is predicted at all of them by ONE forward of ``replicate_temperatures`` (with ``rotations`` = K that forward
    holds ``T*K*B`` crystals, and the T temperatures share the batch's K frames), the model-side value of ``T_t`` being
    ``standardised`` with the loader's ``temp_mean`` / ``temp_std``; the stored temperatures are not read.  The result then
    has one entry per (crystal, temperature), crystal-major -- entry ``g*T + t`` -- each with the keys and shapes above,
    ``temp`` = ``T_t`` as given and ``name`` = ``f"{name}_{T_t:g}K"``.  With T >= 2 it has one more key, ``series``: a dict
    of lists with one entry per input crystal, in the loader's order -- ``name`` (unsuffixed), ``temps`` [T] fp32 and, from
    one ``metrics.temp_series`` per batch on the exported ``u_cif`` / ``u_eq`` (with rotations the frame means'),
    ``t_slope`` [n,6] (A^2/K) and ``t_intercept`` [n,6] of ``u_cif``, ``t_ueq_slope`` [n], ``t_ueq_intercept`` [n],
    ``t_resid`` [n], ``t_drops`` [n] int32 and ``t_stats`` [4] fp64 (sum of ``t_ueq_slope``, rows whose U_eq slope is not
    > 0, rows with a drop, largest ``t_resid``).  ``None`` is the pass as it always was.  ``rigid_molecule`` =
    ``(tol, threshold)``: per batch one ``metrics.molecules`` (the components of the bond graph; they do not depend on U,
    so with temperatures they are found once for all T) and one ``metrics.molecule_test`` per exported ``u_cart`` (with
    rotations the frame mean, with the stored ``cart_dir``; with CIF input the rows of the expanded cell, before site
    averaging), travelling in the same copy.  The result then also has, per crystal, ``mol`` [n] (the row's molecule,
    numbered inside the crystal), ``mol_size`` [n], ``mol_status`` [n] (bit 1 periodic, bit 2 open), ``mol_pos`` [n,3] fp32
    (the atom's unwrapped position relative to its molecule's lowest atom; NaN where the status is not 0), ``mol_pairs``
    [n], ``mol_delta_mean`` [n], ``mol_delta_max`` [n], ``mol_worst`` [n] (an atom index inside the crystal, -1 without
    pairs), ``mol_over`` [n] and ``mol_stats`` [9] fp64 (molecules, tested, periodic, open, largest size; directed pairs,
    sum of ``|D|``, largest ``|D|``, pairs over the threshold).  ``None`` is the pass as it always was.  ``tls_fit`` = ``True``
    (with ``rigid_molecule`` only; otherwise ``ValueError``): one ``metrics.tls_fit`` wherever ``molecule_test`` runs, on the
    same ``u_cart`` and the same molecules, travelling in the same copy.  The result then also has, per crystal, ``tls_u``
    [n,3,3] (the ADP the fitted rigid body gives the atom), ``tls_resid`` [n] (``|Sym u_cart - tls_u|_F``) and, repeated on
    every row of a molecule, ``tls_T`` / ``tls_L`` / ``tls_S`` [n,3,3] (A^2, rad^2, rad A, about ``tls_origin``),
    ``tls_origin`` [n,3] (the centroid in the frame of ``mol_pos``), ``tls_T_principal`` / ``tls_L_principal`` [n,3]
    ascending, ``tls_rank`` [n] (20: all parameters determined; less: the minimum-norm representative; 0: not fitted;
    -1: no convergence) and ``tls_r`` [n] (the molecule's ``sqrt(sum resid^2 / sum |Sym U|^2)``), and ``tls_stats`` [6] fp64
    (fitted molecules, rank-deficient ones, ones with a negative principal value, sum of ``resid^2``, sum of
    ``|Sym U|^2`` over the fitted rows, largest ``resid``).  Rows of molecules that are not fitted (status not 0, fewer
    than five atoms) hold NaN, ``tls_resid`` / ``tls_rank`` / ``tls_r`` 0.  ``None`` is the pass as it always was.
    ``aniso_h`` = ``(stretch, bend)`` (with ``riding_h`` only; otherwise ``ValueError``): one ``metrics.aniso_h`` wherever
    ``riding_h`` runs -- on the frame mean with rotations, once per temperature, on the rows of the expanded cell with CIF
    input -- with the TLS fit of the same ``u_cart`` when ``tls_fit`` is on (without it every hydrogen with a parent has
    source 2), then one ``adp_export`` over atoms as rows, travelling in the same copy.  The result then also has, per
    crystal and per ATOM, ``h_u_cart`` [N,3,3] (a non-hydrogen atom's own row; a hydrogen's tensor: its parent's plus the
    change of the fitted rigid-body motion from the parent to the hydrogen plus ``stretch`` along and ``bend`` across the
    X-H bond; NaN without one), ``h_u_cif`` [N,6], ``h_u_eq`` [N], ``h_source`` [N] (0 none, 1 own row, 2 parent, 3 parent
    and TLS, 4 parent and a rank-deficient TLS) and ``h_aniso_stats`` [4] fp64 (hydrogens with a tensor, those with source
    >= 3, the sum of their ``trace / 3``, those not positive definite); with ``sym`` also ``h_u_cif_asym`` [a,6] per atom
    of the asymmetric unit (``aniso_asym``: a hydrogen's is the listed image's, not an orbit mean).  ``None`` is the pass
    as it always was."""
    rotations = int(rotations)
    if tls_fit and rigid_molecule is None:
        raise ValueError("tls_fit fits the molecules of rigid_molecule: it needs that keyword")
    if aniso_h is not None and riding_h is None:
        raise ValueError("aniso_h builds on the parents of riding_h: it needs that keyword")
    shard = _check_pass(loader, rotations)
    kelvin = None if temperatures is None else check_temperatures(temperatures, least=1, name="temperatures")
    model.eval()
    out: Dict[str, List] = {k: [] for k in KEYS + (SYM_KEYS if sym is not None else ())
                            + (ROT_KEYS if rotations > 1 else ()) + (BOND_KEYS if rigid_bond is not None else ())
                            + (H_KEYS if riding_h is not None else ())
                            + (H_SYM_KEYS if riding_h is not None and sym is not None else ())
                            + (MOL_KEYS if rigid_molecule is not None else ())
                            + (TLS_KEYS if tls_fit else ())
                            + (AH_KEYS if aniso_h is not None else ())
                            + (AH_SYM_KEYS if aniso_h is not None and sym is not None else ())}
    gen = torch.Generator(device=device).manual_seed(seed) if rotations > 1 else None
    if kelvin is not None:
        temps = standardised(kelvin, loader.temp_mean, loader.temp_std, device)
        series: Dict[str, List] = {k: [] for k in ("name", "temps") + SERIES_KEYS}
    with torch.no_grad():
        for batch in loader:
            if batch is None:
                continue
            batch.to(device)
            if kelvin is None:
                _host_stage(out, to_host(_device_stage(model, batch, shard, sym, rotations, gen, rigid_bond, riding_h,
                                                       rigid_molecule, tls_fit, aniso_h)), shard, sym)
            else:
                _host_stage_series(out, series, to_host(_device_stage_series(model, batch, sym, rotations, gen, rigid_bond,
                                                                             riding_h, kelvin, temps, rigid_molecule,
                                                                             tls_fit, aniso_h)),
                                   shard, sym, kelvin)
    if hasattr(model, "flush_graph_checks"):
        model.flush_graph_checks()
    if kelvin is not None and len(kelvin) >= 2:
        out["series"] = series
    return out


def load_input(path: str, device, temperature: Optional[float] = None):
    """What ``--predict_input`` names, as ``(shard, sym, rejected)``.  A shard file: the ``DeviceShard`` of it, ``None``,
    ``None``.  A CIF file or a directory of them: the crystals the reference's filters accept, expanded to their unit cells
    on the GPU in memory (``symmetry.expand``; no shard file is written), their ``CifSymmetry`` and the list of
    ``(name, reason)`` of the crystals that were not accepted, which also go to stderr one per line; ``temperature`` is
    the Kelvin value of a crystal whose file gives none.  No usable crystal raises ``SystemExit``."""
    import os
    from .shard import DeviceShard
    if not (os.path.isdir(path) or path.lower().endswith(".cif")):
        return DeviceShard.from_file(path, device), None, None
    import sys
    from .cif import load_crystals
    from .symmetry import expand
    crystals, rejected = load_crystals(path, False, temperature)
    for name, why in rejected:
        print(f"rejected\t{name}\t{why}", file=sys.stderr)
    if not crystals:
        raise SystemExit(f"--predict: no usable crystal in {path}")
    arrays, sym = expand(crystals, device, labeled=False, temperature=temperature)
    return DeviceShard(arrays, device, labeled=False, names=sym.names), sym, rejected


def pass_statistics(out: Dict[str, List], output: Optional[str] = None, cif_dir: Optional[str] = None, rejected=None,
                    rotations: int = 1, temperatures: Optional[list] = None) -> dict:
    """The result line of a whole ``predict_adps`` pass from its result ``out`` (``rotations`` and ``temperatures`` as the
    pass was given them), summed from the kernels' fp64 per-crystal statistics: ``crystals``, ``rows``, ``u_eq_mean`` and
    ``non_positive_rows``, then ``output`` and ``cif_dir`` as given and the number of ``rejected`` crystals if there is
    such a list (``load_input``); with ``temperatures`` ``entries`` and ``temperatures``, and from a ``series``
    ``ueq_slope_mean``, ``non_increasing_rows``, ``rows_with_drops`` and ``series_resid_max``; with frames ``rotations``,
    ``rot_spread_max`` and ``rot_spread_mean``; with the rigid-bond test ``bonds``, ``rigid_bond_mean`` / ``_max`` /
    ``_over``; with the rigid-body test ``molecules``, ``molecules_tested`` / ``_periodic`` / ``_open``,
    ``molecule_atoms_max`` and ``rigid_molecule_pairs`` / ``_mean`` / ``_max`` / ``_over`` (over the entries: with
    temperatures every crystal counts once per temperature); with the TLS fit ``tls_molecules``, ``tls_rank_deficient``,
    ``tls_nonphysical``, ``tls_r`` (over all fitted rows) and ``tls_resid_max``; with riding hydrogens ``hydrogens``, ``h_orphans``, ``h_uiso_mean`` (over the non-orphans) and
    ``h_non_positive``; with anisotropic hydrogens ``h_aniso`` (hydrogens with a tensor), ``h_aniso_tls`` (those with a
    libration term), ``h_aniso_ueq_mean`` (over ``h_aniso``) and ``h_aniso_non_positive``.  A pass without crystals gives
    zeros."""
    n = len(out["name"])                                  # entries: one per crystal, or per crystal and temperature
    rows = sum(int(t.shape[0]) for t in out["u_eq"])

    def stacked(key: str, width: int, of: dict = out) -> torch.Tensor:   # [n, width] fp64: one kernel's per-crystal figures
        return torch.stack(of[key]) if of[key] else torch.zeros(0, width, dtype=torch.float64)
    stats = stacked("stats", 3)
    res = {"crystals": n // len(temperatures) if temperatures else n, "rows": rows,
           "u_eq_mean": float(stats[:, 0].sum()) / max(rows, 1), "non_positive_rows": int(stats[:, 2].sum()),
           "output": output, "cif_dir": cif_dir}
    if rejected is not None:
        res["rejected"] = len(rejected)
    if temperatures is not None:
        res.update(entries=n, temperatures=temperatures)
    if "series" in out:                               # from the fp64 per-crystal stats of the lines; rows of ONE temperature
        ts = stacked("t_stats", 4, out["series"])
        res.update(ueq_slope_mean=float(ts[:, 0].sum()) / max(rows // len(temperatures), 1),
                   non_increasing_rows=int(ts[:, 1].sum()), rows_with_drops=int(ts[:, 2].sum()),
                   series_resid_max=float(ts[:, 3].max()) if len(ts) else 0.0)
    if rotations > 1:                                 # per row, from the fp64 per-crystal (sum, maximum) of rot_spread
        rot = stacked("rot_stats", 2)
        res.update(rotations=rotations, rot_spread_max=float(rot[:, 1].max()) if n else 0.0,
                   rot_spread_mean=float(rot[:, 0].sum()) / max(rows, 1))
    if "bond_stats" in out:                           # over the directed bonds of the pass, from the fp64 per-crystal stats
        bs = stacked("bond_stats", 4)
        count = int(bs[:, 0].sum())
        res.update(bonds=count, rigid_bond_mean=float(bs[:, 1].sum()) / count if count else 0.0,
                   rigid_bond_max=float(bs[:, 2].max()) if n else 0.0, rigid_bond_over=int(bs[:, 3].sum()))
    if "h_stats" in out:                              # from the fp64 per-crystal stats; the mean is over the non-orphans
        hs = stacked("h_stats", 4)
        hydrogens, orphans = int(hs[:, 0].sum()), int(hs[:, 1].sum())
        res.update(hydrogens=hydrogens, h_orphans=orphans,
                   h_uiso_mean=float(hs[:, 2].sum()) / (hydrogens - orphans) if hydrogens > orphans else 0.0,
                   h_non_positive=int(hs[:, 3].sum()))
    if "h_aniso_stats" in out:
        ah = stacked("h_aniso_stats", 4)
        count = int(ah[:, 0].sum())
        res.update(h_aniso=count, h_aniso_tls=int(ah[:, 1].sum()),
                   h_aniso_ueq_mean=float(ah[:, 2].sum()) / count if count else 0.0, h_aniso_non_positive=int(ah[:, 3].sum()))
    if "mol_stats" in out:                            # the sums over the entries, from the fp64 per-crystal figures
        ms = stacked("mol_stats", 9)
        count = int(ms[:, 5].sum())
        res.update(molecules=int(ms[:, 0].sum()), molecules_tested=int(ms[:, 1].sum()),
                   molecules_periodic=int(ms[:, 2].sum()), molecules_open=int(ms[:, 3].sum()),
                   molecule_atoms_max=int(ms[:, 4].max()) if n else 0, rigid_molecule_pairs=count,
                   rigid_molecule_mean=float(ms[:, 6].sum()) / count if count else 0.0,
                   rigid_molecule_max=float(ms[:, 7].max()) if n else 0.0, rigid_molecule_over=int(ms[:, 8].sum()))
    if "tls_stats" in out:                            # the same; tls_r over all fitted rows of the pass
        ts = stacked("tls_stats", 6)
        r2, s2 = float(ts[:, 3].sum()), float(ts[:, 4].sum())
        res.update(tls_molecules=int(ts[:, 0].sum()), tls_rank_deficient=int(ts[:, 1].sum()),
                   tls_nonphysical=int(ts[:, 2].sum()), tls_r=math.sqrt(r2 / s2) if s2 > 0 else 0.0,
                   tls_resid_max=float(ts[:, 5].max()) if n else 0.0)
    return res


def entry(result: Dict[str, List], k: int) -> dict:
    """Crystal ``k`` of a ``predict_adps`` result: what ``write_cif`` (and, with the keys of a ``CifSymmetry``,
    ``write_cif_symmetric``) takes."""
    return {key: result[key][k] for key in KEYS + SYM_KEYS + ROT_KEYS + BOND_KEYS + H_KEYS + H_SYM_KEYS + MOL_KEYS
            + TLS_KEYS + AH_KEYS + AH_SYM_KEYS if key in result}


def cell_parameters(cell) -> tuple:
    """(a, b, c, alpha, beta, gamma) in Angstrom and degrees of a cell whose rows are the lattice vectors."""
    v = [[float(x) for x in row] for row in (cell.tolist() if hasattr(cell, "tolist") else cell)]
    n = [math.sqrt(sum(x * x for x in r)) for r in v]

    def angle(i, j):
        c = sum(p * q for p, q in zip(v[i], v[j])) / (n[i] * n[j])
        return math.degrees(math.acos(max(-1.0, min(1.0, c))))
    return n[0], n[1], n[2], angle(1, 2), angle(0, 2), angle(0, 1)


def _iso_columns(u_iso, z):
    """Per atom the text of ``_atom_site_U_iso_or_equiv`` and ``_atom_site_adp_type`` (with a leading blank), or ``None``
    for an entry without riding hydrogens.  A value that is no number (an orphan) is written ``?``."""
    if u_iso is None:
        return None
    u = [float(v) for v in u_iso.tolist()]
    if len(u) != len(z):
        raise ValueError(f"{len(u)} isotropic values for {len(z)} atoms")
    return [f" {'?' if math.isnan(x) else format(x, '.6f')} {'Uani' if v != 1 else 'Uiso'}" for x, v in zip(u, z)]


def _hydrogen_tensors(h_cif, h_eq, z) -> dict:
    """``{atom: (U_eq, [U_11 U_22 U_33 U_23 U_13 U_12])}`` of the hydrogens of ``z`` whose tensor in ``h_cif`` [>= n,6]
    (with ``h_eq`` [>= n]) is finite; empty for an entry without anisotropic hydrogens (``h_cif`` is ``None``)."""
    if h_cif is None:
        return {}
    rows, eq = h_cif.tolist(), h_eq.tolist()
    if len(rows) < len(z) or len(eq) < len(z):
        raise ValueError(f"{len(rows)} hydrogen tensors for {len(z)} atoms")
    return {i: (float(eq[i]), rows[i]) for i, v in enumerate(z)
            if v == 1 and all(math.isfinite(x) for x in rows[i]) and math.isfinite(eq[i])}


def _write(path: str, entry: dict, z, labels, frac, u, whose: str, symmetry: list, iso, type_column: bool,
           h_cif=None, h_eq=None) -> None:
    """What the two writers share: the cell, the temperature, ``symmetry`` (the lines that state the setting), the atom loop
    (``labels``, ``z``, ``frac``) and the anisotropic loop of the non-hydrogen atoms (``u``: one row each, ``U_11 U_22 U_33
    U_23 U_13 U_12``).  ``iso``: the entry's isotropic values or ``None``; without them the atom loop has no further column,
    or with ``type_column`` the type alone (``Uani``, ``.`` for a hydrogen).  ``h_cif`` / ``h_eq``: per atom the tensors
    and equivalent values of an entry with anisotropic hydrogens; a hydrogen with a finite one is typed ``Uani`` with its
    own U_eq and gets a row of the anisotropic loop, which then runs in atom order over all atoms that have a tensor."""
    heavy = [i for i, v in enumerate(z) if v != 1]
    if len(heavy) != len(u):
        raise ValueError(f"{len(u)} ADP rows for {len(heavy)} non-hydrogen atoms{whose}")
    hydrogens = _hydrogen_tensors(h_cif, h_eq, z)
    a, b, c, al, be, ga = cell_parameters(entry["cell"])
    name = "".join(ch if ch.isalnum() or ch in "_-." else "_" for ch in str(entry["name"])) or "crystal"
    lines = [f"data_{name}",
             f"_cell_length_a {a:.6f}", f"_cell_length_b {b:.6f}", f"_cell_length_c {c:.6f}",
             f"_cell_angle_alpha {al:.5f}", f"_cell_angle_beta {be:.5f}", f"_cell_angle_gamma {ga:.5f}"]
    temp = float(entry["temp"])
    if not math.isnan(temp):
        lines.append(f"_diffrn_ambient_temperature {temp:.2f}")
    lines += symmetry
    lines += ["loop_", "_atom_site_label", "_atom_site_type_symbol", "_atom_site_fract_x", "_atom_site_fract_y",
              "_atom_site_fract_z"]
    tails = _iso_columns(iso, z)
    if tails is not None:
        lines += ["_atom_site_U_iso_or_equiv", "_atom_site_adp_type"]
    elif type_column:
        lines.append("_atom_site_adp_type")
        tails = [f" {'Uani' if v != 1 else '.'}" for v in z]
    else:
        tails = [""] * len(z)
    if iso is not None:
        for i, (eq, _) in hydrogens.items():
            tails[i] = f" {eq:.6f} Uani"
    for lab, v, f, tail in zip(labels, z, frac, tails):
        lines.append(f"{lab} {SYMBOLS[v] if 0 <= v < len(SYMBOLS) else 'X'} {f[0]:.6f} {f[1]:.6f} {f[2]:.6f}" + tail)
    lines += ["loop_", "_atom_site_aniso_label", "_atom_site_aniso_U_11", "_atom_site_aniso_U_22", "_atom_site_aniso_U_33",
              "_atom_site_aniso_U_23", "_atom_site_aniso_U_13", "_atom_site_aniso_U_12"]
    rows = dict(zip(heavy, u))
    rows.update({i: row for i, (_, row) in hydrogens.items()})
    for i in sorted(rows):
        lines.append(labels[i] + " " + " ".join(f"{x:.6f}" for x in rows[i]))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def write_cif(path: str, entry: dict) -> None:
    """One crystal as a P1 CIF: the cell, the temperature, every atom (label = element symbol + running number) and the
    anisotropic displacement parameters of the non-hydrogen atoms, ``U_11 U_22 U_33 U_23 U_13 U_12``.  An entry with
    ``u_iso`` (``predict_adps(riding_h=)``) also gets ``_atom_site_U_iso_or_equiv`` and ``_atom_site_adp_type`` in the atom
    loop: ``Uani`` with U_eq for a non-hydrogen atom, ``Uiso`` with the riding value for a hydrogen, ``?`` for an orphan.
    An entry with ``h_u_cif`` (``predict_adps(aniso_h=)``) gives every hydrogen with a finite tensor the type ``Uani``, its
    ``h_u_eq`` and a row of the anisotropic loop; an orphan stays ``?`` / ``Uiso``."""
    z = [int(v) for v in entry["z"].tolist()]
    labels = [f"{SYMBOLS[v] if 0 <= v < len(SYMBOLS) else 'X'}{i + 1}" for i, v in enumerate(z)]
    p1 = ["_symmetry_space_group_name_H-M 'P 1'", "_symmetry_Int_Tables_number 1",
          "loop_", "_symmetry_equiv_pos_as_xyz", "'x, y, z'"]
    _write(path, entry, z, labels, entry["frac"].tolist(), entry["u_cif"].tolist(), "", p1, entry.get("u_iso"), False,
           entry.get("h_u_cif"), entry.get("h_u_eq"))


def write_cif_symmetric(path: str, entry: dict) -> None:
    """One crystal in the setting of the file it came from: the cell, the temperature, the symmetry operators, the
    asymmetric unit with the input's labels and coordinates, and the site-averaged anisotropic displacement parameters of
    its non-hydrogen atoms (``u_cif_asym``: ``U_11 U_22 U_33 U_23 U_13 U_12``).  An entry with ``u_iso_asym``
    (``predict_adps(riding_h=)``) also gets ``_atom_site_U_iso_or_equiv``, and its hydrogens the type ``Uiso``.  An entry
    with ``h_u_cif_asym`` (``predict_adps(aniso_h=)``) gives every hydrogen with a finite tensor the type ``Uani``, the
    ``h_u_eq`` of the expanded atom it is (the first atoms of the expanded cell are the asymmetric unit) and a row of the
    anisotropic loop: the tensor of the listed image, not an orbit mean."""
    z = [int(v) for v in entry["asym_z"].tolist()]
    ops = ["loop_", "_space_group_symop_id", "_space_group_symop_operation_xyz"]
    ops += [f"{k + 1} '{op}'" for k, op in enumerate(entry["symops"])]
    _write(path, entry, z, list(entry["asym_labels"]), entry["asym_frac"].tolist(), entry["u_cif_asym"].tolist(),
           " of the asymmetric unit", ops, entry.get("u_iso_asym"), True, entry.get("h_u_cif_asym"),
           entry.get("h_u_eq") if "h_u_cif_asym" in entry else None)
