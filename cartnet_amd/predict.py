"""ADPs for crystals that have no targets, in the convention crystallographic tools read.

``predict_adps`` is the prediction-side counterpart of ``evaluate.inference``: per batch of a resident shard (labeled or
not) one forward, one ``adp_export`` (csrc/export_ops.hip: the predictions on the unit reciprocal axes -- the inverse of the
transform the reference applied to the dataset's targets, dataset/extract_csd_data.py:115-123 -- with U_eq and the
principal values / axes), the fractional coordinates, ONE device-to-host copy (``metrics.to_host``) and a split by row
counts on the host.  What else the copy brings -- for crystals from CIF files, in K frames, at T temperatures, and for
the five analyses of ``Analyses``, the bond table and the angle and torsion tables -- is stated once, in ``GROUPS``: a row
per group of keys with its documentation.  ``write_cif`` writes one crystal of the result as a P1 CIF, ``write_cif_symmetric`` one that came from a CIF file in the
file's own setting.  Around the pass, for ``main.py --predict``: ``load_input`` (a shard file, or CIF files expanded in
memory), ``parse_temperatures`` (the flag's SPEC) and ``pass_statistics`` (the result line).  ``frame_stage`` is the
forward in K frames that this pass and ``evaluate.inference`` share.  A model that reads crystals in another frame than the
stored one (iComformer: the reduced cell) gets it through ``model_frame``: only the forward sees that frame, its members
come back through ``metrics.stored_frame``, and every key keeps its meaning and its frame (row ``model_frame``).
"""
from __future__ import annotations

import math
from typing import Callable, Dict, List, NamedTuple, Optional

import torch

from .metrics import (adp_export, angle_index, angle_table as angle_table_call, aniso_h as aniso_h_call, batch_graph,
                      bond_index, bond_table as bond_table_call, bond_test, check_export_status, check_temperatures,
                      edge_row_ptr, frame_mean, molecule_test, molecules as find_molecules, riding_h as riding_h_call,
                      rotate_rows, split_rows, stored_frame, target_row_ptr, temp_series, tls_fit as tls_fit_call, to_host)


class Analyses(NamedTuple):
    """The analyses of a pass that run on the bond graph, as ``predict_adps`` and ``evaluate.inference`` take them by
    keyword; ``None`` is off.  Each one's row of ``GROUPS`` says what it adds."""
    rigid_bond: Optional[tuple] = None                    # (tol, threshold)
    riding_h: Optional[tuple] = None                      # (tol, f, f_rot)
    rigid_molecule: Optional[tuple] = None                # (tol, threshold)
    tls_fit: Optional[bool] = None                        # True, with rigid_molecule only
    aniso_h: Optional[tuple] = None                       # (stretch, bend), with riding_h only

    def checked(self) -> "Analyses":
        """Itself, or ``ValueError`` for an analysis without the one it builds on."""
        if self.tls_fit and self.rigid_molecule is None:
            raise ValueError("tls_fit fits the molecules of rigid_molecule: it needs that keyword")
        if self.aniso_h is not None and self.riding_h is None:
            raise ValueError("aniso_h builds on the parents of riding_h: it needs that keyword")
        return self


class Group(NamedTuple):
    """One group of keys of a result.  ``present(analyses, sym, rotations, temperatures, bond_table, angle_table,
    model_frame)``: whether a pass has it (``bond_table`` and ``angle_table``, ``None`` by default, are the analyses that
    are no field of ``Analyses``; ``model_frame``, ``False`` by default: whether the model reads another frame);
    ``cuts``: its keys in order, each with how it is cut into the crystals' entries -- a tensor that travels to the host
    as one slice of dim 0 per "crystal", or as the pieces of dim 0 that hold a crystal's atoms ("atom"), its non-hydrogen
    rows ("row"), the non-hydrogen atoms of its asymmetric unit ("site"), its listed bonds ("bond", counted from the
    batch's ``bond_ptr``), its angles ("angle") or its torsions ("torsion"; both counted from the batch's ``angle_ptr`` and
    ``torsion_ptr``);
    ``None``: assembled on the host; ``doc``: what the keys hold."""
    present: Callable
    cuts: Dict[str, Optional[str]]
    doc: str


# Every key of a result, stated once, in the key order of a result (it is in the pickle's bytes).  The keys of "series"
# live in result["series"], which has one entry per input crystal and is appended to a result last; the two rows after it
# came later and follow ``bonds_*`` in a result.
GROUPS: Dict[str, Group] = {
    "base": Group(lambda a, sym, K, T, bt=None, at=None, mf=False: True,
        {"name": None, "atoms": "row", "frac": "atom", "z": "atom", "cell": "crystal", "temp": None, "u_cart": "row",
         "u_cif": "row", "u_eq": "row", "principal": "row", "axes": "row", "stats": "crystal"},
        """``name``; ``atoms`` [n] (Z of the n non-hydrogen atoms the rows belong to); ``frac`` [N,3] and ``z`` [N]
        (all atoms); ``cell`` [3,3]; ``temp`` (Kelvin, as stored; NaN if the shard has none); ``u_cart`` [n,3,3] (the
        model's output); ``u_cif`` [n,6] (U11 U22 U33 U23 U13 U12); ``u_eq`` [n]; ``principal`` [n,3] ascending;
        ``axes`` [n,3,3]; ``stats`` [3] fp64 (sum of u_eq, smallest principal value, rows with a non-positive one)."""),
    "model_frame": Group(lambda a, sym, K, T, bt=None, at=None, mf=False: bool(mf),
        {"cell_rotation": "crystal", "cell_reduced": "crystal"},
        """``model_frame`` = the ``DeviceShard.with_optimized_cell()`` of the loader's shard (iComformer, whose recipe reads
        a crystal in the frame of its reduced cell): the forward runs on ``model_frame.frame_view(batch)``, the members
        come back once through ``metrics.stored_frame`` (``U = R P R^T``), and every other key keeps its meaning and its
        frame -- the stored cell and the stored ``cart_dir`` serve the export, the analyses, the site average and the
        writers.  ``cell_rotation`` [3,3] (R: the model read ``cart_dir @ R``) and ``cell_reduced`` [3,3] (the cell the
        model read, rows = lattice vectors in the rotated frame).  ``rotations`` > 1 raises ``ValueError``."""),
    "symmetry": Group(lambda a, sym, K, T, bt=None, at=None, mf=False: sym,
        {"asym_labels": None, "asym_frac": None, "asym_z": None, "u_cif_asym": "site", "spread": "site", "symops": None},
        """``sym``: the ``CifSymmetry`` of a shard expanded from CIF files.  ``asym_labels`` / ``asym_frac`` [a,3] /
        ``asym_z`` [a] (the asymmetric unit as the file gives it), ``symops`` (strings, identity first), ``u_cif_asym``
        [h,6] (one row per non-hydrogen atom of the asymmetric unit, the mean over its orbit,
        ``symmetry.site_average``) and ``spread`` [h]."""),
    "rotations": Group(lambda a, sym, K, T, bt=None, at=None, mf=False: K > 1,
        {"rot_spread": "row", "frames": "crystal", "rot_stats": "crystal"},
        """``rotations`` = K > 1: every batch is predicted in K frames by ONE forward of ``replicate(batch, K, R)``
        with ``R = frames(B, K, gen, device)`` (one generator seeded with ``seed`` for the whole pass), the members are
        brought back and averaged (``metrics.frame_mean``), and everything else derives from that mean: ``u_cart`` is
        the mean.  ``rot_spread`` [n] (per row the largest deviation of a frame's prediction from the mean), ``frames``
        [K,3,3] (the rotations used, the identity first) and ``rot_stats`` [2] fp64 (sum and maximum of
        ``rot_spread``)."""),
    "rigid_bond": Group(lambda a, sym, K, T, bt=None, at=None, mf=False: a.rigid_bond is not None,
        {"bond_count": "row", "bond_delta_mean": "row", "bond_delta_max": "row", "bond_worst": "row", "bond_over": "row",
         "bond_ueq_ratio": "row", "bond_stats": "crystal"},
        """``rigid_bond`` = ``(tol, threshold)``: Hirshfeld's rigid-bond test, one ``metrics.bond_test``
        (csrc/bond_ops.hip) per exported ``u_cart`` (with rotations the frame mean; with CIF input the rows of the
        expanded cell, before site averaging): a plausibility report that needs no truth.  ``bond_count`` [n],
        ``bond_delta_mean`` [n] (mean ``|D|`` over the atom's bonds, 0 without bonds), ``bond_delta_max`` [n],
        ``bond_worst`` [n] (the partner of the worst bond as an atom index inside the crystal, -1 without bonds),
        ``bond_over`` [n], ``bond_ueq_ratio`` [n] and ``bond_stats`` [4] fp64 (directed bonds, sum of ``|D|``, largest
        ``|D|``, bonds over the threshold)."""),
    "riding_h": Group(lambda a, sym, K, T, bt=None, at=None, mf=False: a.riding_h is not None,
        {"u_iso": "atom", "h_parent": "atom", "h_count": "atom", "h_mult": "atom", "h_stats": "crystal"},
        """``riding_h`` = ``(tol, f, f_rot)``: one ``metrics.riding_h`` (csrc/riding_ops.hip) per exported ``u_eq``
        (with rotations the frame mean's); both CIF writers then fill ``_atom_site_U_iso_or_equiv`` for every atom.
        ``u_iso`` [N] (every atom: a hydrogen's ``mult * u_eq[parent]``, NaN for an orphan; a non-hydrogen atom's own
        ``u_eq``), ``h_parent`` [N] (an atom index inside the crystal, -1 where there is none), ``h_count`` [N]
        (hydrogens riding on a non-hydrogen atom), ``h_mult`` [N] and ``h_stats`` [4] fp64 (hydrogens, orphans, sum of
        the finite hydrogen ``u_iso``, hydrogens with a non-positive parent ``u_eq``)."""),
    "riding_h_symmetry": Group(lambda a, sym, K, T, bt=None, at=None, mf=False: a.riding_h is not None and sym,
        {"u_iso_asym": None, "h_parent_asym": None},
        """``u_iso_asym`` [a] and ``h_parent_asym`` [a] per atom of the asymmetric unit (``riding_asym``)."""),
    "rigid_molecule": Group(lambda a, sym, K, T, bt=None, at=None, mf=False: a.rigid_molecule is not None,
        {"mol": "row", "mol_size": "row", "mol_status": "row", "mol_pos": "row", "mol_pairs": "row",
         "mol_delta_mean": "row", "mol_delta_max": "row", "mol_worst": "row", "mol_over": "row", "mol_stats": "crystal"},
        """``rigid_molecule`` = ``(tol, threshold)``: per batch one ``metrics.molecules`` (the components of the bond
        graph with every atom's unwrapped position; they do not depend on U, so they are found once for all T) and one
        ``metrics.molecule_test`` (csrc/molecule_ops.hip) per exported ``u_cart``, as for ``rigid_bond`` and with the
        stored ``cart_dir``: the rigid-body test over all pairs of atoms of a molecule.  ``mol`` [n] (the row's
        molecule, numbered inside the crystal), ``mol_size`` [n], ``mol_status`` [n] (bit 1 periodic, bit 2 open),
        ``mol_pos`` [n,3] fp32 (the atom's unwrapped position relative to its molecule's lowest atom; NaN where the
        status is not 0), ``mol_pairs`` [n], ``mol_delta_mean`` [n], ``mol_delta_max`` [n], ``mol_worst`` [n] (an atom
        index inside the crystal, -1 without pairs), ``mol_over`` [n] and ``mol_stats`` [9] fp64 (molecules, tested,
        periodic, open, largest size; directed pairs, sum of ``|D|``, largest ``|D|``, pairs over the threshold)."""),
    "tls_fit": Group(lambda a, sym, K, T, bt=None, at=None, mf=False: bool(a.tls_fit),
        {"tls_u": "row", "tls_resid": "row", "tls_T": "row", "tls_L": "row", "tls_S": "row", "tls_origin": "row",
         "tls_T_principal": "row", "tls_L_principal": "row", "tls_rank": "row", "tls_r": "row", "tls_stats": "crystal"},
        """``tls_fit`` = ``True`` (with ``rigid_molecule`` only): one ``metrics.tls_fit`` (csrc/tls_ops.hip) beside
        every ``molecule_test``: the rigid-body tensors T, L and S that explain the ADPs of a molecule of five or more
        atoms best.  ``tls_u`` [n,3,3] (the ADP the fitted rigid body gives the atom), ``tls_resid`` [n] (``|Sym u_cart
        - tls_u|_F``) and, repeated on every row of a molecule, ``tls_T`` / ``tls_L`` / ``tls_S`` [n,3,3] (A^2, rad^2,
        rad A, about ``tls_origin``), ``tls_origin`` [n,3] (the centroid in the frame of ``mol_pos``),
        ``tls_T_principal`` / ``tls_L_principal`` [n,3] ascending, ``tls_rank`` [n] (20: all parameters determined;
        less: the minimum-norm representative; 0: not fitted; -1: no convergence) and ``tls_r`` [n] (the molecule's
        ``sqrt(sum resid^2 / sum |Sym U|^2)``), and ``tls_stats`` [6] fp64 (fitted molecules, rank-deficient ones, ones
        with a negative principal value, sum of ``resid^2``, sum of ``|Sym U|^2`` over the fitted rows, largest
        ``resid``).  Rows of molecules that are not fitted (status not 0, fewer than five atoms) hold NaN, ``tls_resid``
        / ``tls_rank`` / ``tls_r`` 0."""),
    "aniso_h": Group(lambda a, sym, K, T, bt=None, at=None, mf=False: a.aniso_h is not None,
        {"h_u_cart": "atom", "h_u_cif": "atom", "h_u_eq": "atom", "h_source": "atom", "h_aniso_stats": "crystal"},
        """``aniso_h`` = ``(stretch, bend)`` (with ``riding_h`` only): one ``metrics.aniso_h`` (csrc/aniso_h_ops.hip)
        wherever ``riding_h`` runs, with the TLS fit of the same ``u_cart`` when ``tls_fit`` is on (without it every
        hydrogen with a parent has source 2), then one ``adp_export`` over atoms as rows; both CIF writers then give
        such a hydrogen an anisotropic row.  Per ATOM: ``h_u_cart`` [N,3,3] (a non-hydrogen atom's own row; a hydrogen's
        tensor: its parent's plus the change of the fitted rigid-body motion from the parent to the hydrogen plus
        ``stretch`` along and ``bend`` across the X-H bond; NaN without one), ``h_u_cif`` [N,6], ``h_u_eq`` [N],
        ``h_source`` [N] (0 none, 1 own row, 2 parent, 3 parent and TLS, 4 parent and a rank-deficient TLS) and
        ``h_aniso_stats`` [4] fp64 (hydrogens with a tensor, those with source >= 3, the sum of their ``trace / 3``,
        those not positive definite)."""),
    "aniso_h_symmetry": Group(lambda a, sym, K, T, bt=None, at=None, mf=False: a.aniso_h is not None and sym,
        {"h_u_cif_asym": None},
        """``h_u_cif_asym`` [a,6] per atom of the asymmetric unit (``aniso_asym``: a hydrogen's is the listed image's,
        not an orbit mean)."""),
    "bond_table": Group(lambda a, sym, K, T, bt=None, at=None, mf=False: bt is not None,
        {"bonds_a": "bond", "bonds_b": "bond", "bonds_dir": "bond", "bonds_length": "bond", "bonds_delta": "bond",
         "bonds_lower": "bond", "bonds_upper": "bond", "bonds_libration": "bond", "bonds_tls_rank": "bond",
         "bonds_stats": "crystal"},
        """``bond_table`` = the bond tolerance: per batch one ``metrics.bond_index`` (the bonds do not depend on U, so they
        are counted once for all T; its ``B + 1`` offsets are the one further device-to-host copy of a batch) and one
        ``metrics.bond_table`` (csrc/bond_table_ops.hip) per exported ``u_cart``, wherever ``rigid_bond`` runs, with the
        TLS fit of the same ``u_cart`` when ``tls_fit`` is on.  The only keys whose length is neither atoms nor rows: one
        entry per bond ``j -> i`` with ``j < i``, ``m`` of them, in target order and within a target in edge order.
        ``bonds_a`` / ``bonds_b`` [m] (``j`` and ``i`` as atom indices inside the crystal), ``bonds_dir`` [m,3] and
        ``bonds_length`` [m] (the edge as stored), ``bonds_delta`` [m] (Hirshfeld's ``D = d^T (U_b - U_a) d``, signed),
        ``bonds_lower`` / ``bonds_upper`` [m] (the Busing & Levy bounds on the thermally averaged length; NaN for a
        tensor that is not positive across the bond), ``bonds_libration`` [m] (the length corrected for the fitted
        libration ``L``; NaN without a fit), ``bonds_tls_rank`` [m] (that fit's rank, 0 without one) and ``bonds_stats``
        [9] fp64 (listed bonds, unlisted ``j > i`` bond edges -- a capped graph's differ --, sum of ``bonds_length``, sum
        of ``|D|``, largest ``|D|``, bonds with a libration, sum and largest of ``bonds_libration - bonds_length`` over
        those, bonds with a NaN bound).  X-H bonds and the riding-model correction are not here (angles and torsions:
        the rows ``angle_table`` and ``torsion_table``), and no CIF writer reads these keys."""),
    "series": Group(lambda a, sym, K, T, bt=None, at=None, mf=False: T is not None and len(T) >= 2,
        {"t_slope": "row", "t_intercept": "row", "t_ueq_slope": "row", "t_ueq_intercept": "row", "t_resid": "row",
         "t_drops": "row", "t_stats": "crystal"},
        """``temperatures`` = T >= 1 Kelvin values (strictly increasing, finite, > 0; otherwise ``ValueError``): every
        batch is predicted at all of them by ONE forward of ``replicate_temperatures`` (with ``rotations`` = K that
        forward holds ``T*K*B`` crystals, and the T temperatures share the batch's K frames), the model-side value of
        ``T_t`` being ``standardised`` with the loader's ``temp_mean`` / ``temp_std``; the stored temperatures are not
        read.  The result then has one entry per (crystal, temperature), crystal-major -- entry ``g*T + t`` -- with
        ``temp`` = ``T_t`` as given and ``name`` = ``f"{name}_{T_t:g}K"``; every analysis runs once per temperature.
        With T >= 2 it has one more key, ``series``: a dict of lists with one entry per input crystal, in the loader's
        order -- ``name`` (unsuffixed), ``temps`` [T] fp32 and, from one ``metrics.temp_series`` (csrc/series_ops.hip)
        per batch on the exported ``u_cif`` / ``u_eq`` (with rotations the frame means'), ``t_slope`` [n,6] (A^2/K) and
        ``t_intercept`` [n,6] of ``u_cif``, ``t_ueq_slope`` [n], ``t_ueq_intercept`` [n], ``t_resid`` [n], ``t_drops``
        [n] int32 and ``t_stats`` [4] fp64 (sum of ``t_ueq_slope``, rows whose U_eq slope is not > 0, rows with a drop,
        largest ``t_resid``)."""),
    "angle_table": Group(lambda a, sym, K, T, bt=None, at=None, mf=False: at is not None,
        {"angles_a": "angle", "angles_b": "angle", "angles_c": "angle", "angles_value": "angle",
         "angles_libration": "angle", "angles_tls_rank": "angle", "angles_stats": "crystal"},
        """``angle_table`` = the bond tolerance: per batch one ``metrics.angle_index`` (on the ``bond_index`` of
        ``bond_table`` if that is on with the same tolerance; nothing in it depends on U, so it is built once for all T;
        its two ``B + 1`` offsets travel in one further device-to-host copy of a batch) and one ``metrics.angle_table``
        (csrc/angle_table_ops.hip) per exported ``u_cart``, wherever ``bond_table`` runs, with the TLS fit of the same
        ``u_cart`` when ``tls_fit`` is on.  One entry per valence angle a-b-c of the bond graph, ``m`` of them: centres
        ``b`` in atom order, the pairs of a centre's bond edges by the first, then the second.  ``angles_a`` /
        ``angles_b`` / ``angles_c`` [m] (atom indices inside the crystal), ``angles_value`` [m] (degrees, from the stored
        edge directions: cell faces and images need no special case), ``angles_libration`` [m] (the angle after the
        fitted libration ``L`` of ``b``'s molecule; NaN without a fit), ``angles_tls_rank`` [m] (that fit's rank, 0
        without one) and ``angles_stats`` [5] fp64 (angles, sum of ``angles_value``, angles with a libration, sum and
        largest of ``|angles_libration - angles_value|`` over those).  No CIF writer reads these keys."""),
    "torsion_table": Group(lambda a, sym, K, T, bt=None, at=None, mf=False: at is not None,
        {"torsions_a": "torsion", "torsions_b": "torsion", "torsions_c": "torsion", "torsions_d": "torsion",
         "torsions_value": "torsion", "torsions_libration": "torsion", "torsions_tls_rank": "torsion",
         "torsions_stats": "crystal"},
        """With ``angle_table``, from the same two calls: one entry per torsion a-b-c-d, ``m`` of them, the central bonds
        b-c in the bond table's order (``b < c``), then the neighbours of ``b``, then those of ``c``.  ``torsions_a`` ...
        ``torsions_d`` [m] (atom indices inside the crystal; a three-membered ring gives entries with ``a == d``, which
        a user filters on the indices), ``torsions_value`` [m] (degrees in (-180, 180], the IUPAC sign; NaN for a
        collinear end), ``torsions_libration`` [m] and ``torsions_tls_rank`` [m] (as for the angles, read at ``c``) and
        ``torsions_stats`` [5] fp64 (torsions, those with a NaN value, those with a libration, sum and largest of the
        circular ``|torsions_libration - torsions_value|`` over those)."""),
}
(KEYS, MF_KEYS, SYM_KEYS, ROT_KEYS, BOND_KEYS, H_KEYS, H_SYM_KEYS, MOL_KEYS, TLS_KEYS, AH_KEYS, AH_SYM_KEYS, BT_KEYS,
 SERIES_KEYS, AT_KEYS, TT_KEYS) = (tuple(g.cuts) for g in GROUPS.values())


def _cuts(*names: str) -> Dict[str, str]:
    return {k: c for name in names or GROUPS for k, c in GROUPS[name].cuts.items() if c is not None}


# the cuts under the names they have always had (tests/test_cif_writers_golden.py holds SPLIT to these five); CUT: all
SPLIT, CUT = _cuts("base", "symmetry", "rotations", "rigid_bond", "riding_h"), _cuts()
SERIES_SPLIT, MOL_SPLIT, TLS_SPLIT, AH_SPLIT = _cuts("series"), _cuts("rigid_molecule"), _cuts("tls_fit"), _cuts("aniso_h")
BT_SPLIT, AT_SPLIT, TT_SPLIT = _cuts("bond_table"), _cuts("angle_table"), _cuts("torsion_table")


def result_keys(analyses: Analyses, sym: bool, rotations: int, bond_table: Optional[float] = None,
                angle_table: Optional[float] = None, model_frame: bool = False) -> tuple:
    """The keys of a ``predict_adps`` result in its order (``sym``: whether the pass has a ``CifSymmetry``; ``bond_table``
    and ``angle_table``: their tolerances, ``None`` without one; ``model_frame``: whether the pass has one); ``series``,
    which a pass at two or more temperatures adds at the end, is not among them."""
    return tuple(k for g in GROUPS.values()
                 if g.present(analyses, sym, rotations, None, bond_table, angle_table, model_frame) for k in g.cuts)


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
    members, R = _forward(model, batch, rotations, gen)
    pred, fm = _frame_mean(members, R, row_ptr, stats)
    return pred, R, fm


def _forward(model, batch, rotations: int, gen, temps: Optional[torch.Tensor] = None):
    """ONE forward of ``batch`` in ``rotations`` = K frames and, with ``temps`` (``standardised``), at its T temperatures:
    ``(members, R)``, the predictions of the ``T*K`` replicas (temperature-major, then frame) and the frames drawn from
    ``gen``, ``None`` for K = 1.  Without ``temps`` and at K = 1 it is the plain forward of the batch as collated."""
    R = frames(int(batch.num_graphs), rotations, gen, batch.x.device) if rotations > 1 else None
    if temps is None and R is None:
        atoms = batch.x
        members, _ = model(batch)
        batch.x = atoms
        return members, None
    replica = replicate(batch, rotations, R) if temps is None else replicate_temperatures(batch, temps, rotations, R)
    return model(replica)[0], R                                               # batch.x stays: the replica's is overwritten


def _frame_mean(members: torch.Tensor, R: Optional[torch.Tensor], row_ptr: torch.Tensor, stats: bool):
    """``(prediction, FrameMean)`` of one temperature's ``members`` in the frames ``R``: their ``metrics.frame_mean``, or
    the members themselves and ``None`` without frames."""
    if R is None:
        return members, None
    fm = frame_mean(members, R, row_ptr, stats=stats)
    return fm.mean, fm


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


def bond_table_entries(bt, batch) -> dict:
    """The keys of ``BT_KEYS`` from a ``metrics.BondTable`` of ``batch``, on the device: ``bonds_a`` and ``bonds_b`` as atom
    indices inside their crystal, converted as ``bond_entries`` converts ``bond_worst``.  Static-shape device ops: nothing
    is read back."""
    return {"bonds_a": _in_crystal(bt.a, batch), "bonds_b": _in_crystal(bt.b, batch), "bonds_dir": bt.dir,
            "bonds_length": bt.length, "bonds_delta": bt.delta, "bonds_lower": bt.lower, "bonds_upper": bt.upper,
            "bonds_libration": bt.libration, "bonds_tls_rank": bt.tls_rank, "bonds_stats": bt.crystal_stats}


def angle_table_entries(at, batch) -> dict:
    """The keys of ``AT_KEYS`` and ``TT_KEYS`` from a ``metrics.AngleTable`` of ``batch``, on the device: the atom indices
    brought inside their crystal as ``bond_table_entries`` does.  Static-shape device ops: nothing is read back."""
    return {"angles_a": _in_crystal(at.angle_a, batch), "angles_b": _in_crystal(at.angle_b, batch),
            "angles_c": _in_crystal(at.angle_c, batch), "angles_value": at.angle_value,
            "angles_libration": at.angle_libration, "angles_tls_rank": at.angle_tls_rank, "angles_stats": at.angle_stats,
            "torsions_a": _in_crystal(at.torsion_a, batch), "torsions_b": _in_crystal(at.torsion_b, batch),
            "torsions_c": _in_crystal(at.torsion_c, batch), "torsions_d": _in_crystal(at.torsion_d, batch),
            "torsions_value": at.torsion_value, "torsions_libration": at.torsion_libration,
            "torsions_tls_rank": at.torsion_tls_rank, "torsions_stats": at.torsion_stats}


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


def _device_stage(model, batch, shard, sym, rotations: int, gen, analyses: Analyses, kelvin: Optional[list] = None,
                  temps: Optional[torch.Tensor] = None, bond_table: Optional[float] = None,
                  angle_table: Optional[float] = None, model_frame=None) -> dict:
    """One batch (on the device) through ONE forward (``_forward``; with the T temperatures ``kelvin``, ``temps`` are their
    model-side values) and the kernels that follow it, those once per temperature on that temperature's rows.  With
    ``model_frame`` the forward -- and nothing else -- sees that shard's ``frame_view`` of the batch, and its members come
    back to the stored frame through one ``stored_frame`` before anything reads them.  Returns
    what travels to the host in one ``to_host``: what does not depend on the prediction under its key of ``CUT``, the
    keys of prediction t (the only one without temperatures) under ``"<key>@<t>"``, with T >= 2 the keys of
    ``SERIES_KEYS`` (one ``temp_series`` call on the T exports), and under names with a leading underscore what
    ``_host_stage`` needs to cut and check them."""
    T = 1 if kelvin is None else len(kelvin)
    row_ptr = target_row_ptr(batch)
    dev = _of_the_batch(batch, row_ptr)
    if kelvin is None and "temperature" in shard.t:
        dev["_temp"] = shard.t["temperature"][dev["_sel"]]                    # the collated one is standardised
    if model_frame is None:
        members, R = _forward(model, batch, rotations, gen, temps)
    else:                                                                     # K = 1: predict_adps has refused more
        view = model_frame.frame_view(batch)
        members, R = _forward(model, view, 1, None, temps)
        members = stored_frame(members, view.rotation, row_ptr, T)
        dev["cell_rotation"], dev["cell_reduced"] = view.rotation, view.cell
    if R is not None:
        dev["frames"] = R.transpose(0, 1)
    rows = int(members.shape[0]) // T                                         # K*M: one temperature's slice
    graph, mo, index, angles = _of_the_graph(batch, row_ptr, rows // rotations, analyses, bond_table, angle_table)
    if index is not None:                                                     # all four: once for all T
        dev["_bond_ptr"] = index.bond_ptr
    if angles is not None:
        dev["_angle_ptr"], dev["_torsion_ptr"] = angles.angle_ptr, angles.torsion_ptr
    per = []
    for t in range(T):
        pred, fm = _frame_mean(members[t * rows:(t + 1) * rows], R, row_ptr, stats=True)
        d = {} if fm is None else {"rot_spread": fm.spread, "rot_stats": fm.crystal_spread}
        d.update(_exported(pred, batch, row_ptr, sym, analyses, graph, mo, index, angles))
        per.append(d)
        dev.update({f"{k}@{t}": v for k, v in d.items()})
    if T >= 2:
        ts = temp_series(torch.cat([d["u_cif"] for d in per]), torch.cat([d["u_eq"] for d in per]), kelvin, row_ptr)
        dev.update(zip(SERIES_KEYS, ts))                                      # the fields of a TempSeries, in their order
    return dev


def _of_the_graph(batch, row_ptr: torch.Tensor, rows: int, analyses: Analyses, bond_table: Optional[float] = None,
                  angle_table: Optional[float] = None):
    """``(metrics.BatchGraph of the batch, its metrics.Molecules, its metrics.BondIndex, its metrics.AngleIndex)``, each
    ``None`` unless an analysis needs it: what the analyses of ``_exported`` share and what does not depend on U, so
    checked, built and found once per batch (its atomic numbers in ``x``), however many predictions of it follow.
    ``bond_table`` and ``angle_table``: their tolerances; at the same tolerance the angles build on the bond table's
    index."""
    if (analyses.rigid_bond is None and analyses.riding_h is None and analyses.rigid_molecule is None and bond_table is None
            and angle_table is None):
        return None, None, None, None
    graph = batch_graph(batch, rows, "predict_adps")
    index = None if bond_table is None else bond_index(graph, row_ptr, bond_table)
    return (graph, None if analyses.rigid_molecule is None else find_molecules(graph, row_ptr, analyses.rigid_molecule[0]),
            index, None if angle_table is None else angle_index(
                graph, row_ptr, angle_table, bonds=index if bond_table == angle_table else None))


def _exported(pred: torch.Tensor, batch, row_ptr: torch.Tensor, sym, analyses: Analyses, graph=None, mo=None,
              index=None, angles=None) -> dict:
    """The kernels that follow the forward, on the prediction ``pred`` [M,3,3] of ``batch``: the export and, as
    ``analyses`` asks and on ``graph``, ``mo``, ``index`` and ``angles`` (``_of_the_graph``), the rigid-bond test, the
    rigid-body test (and the TLS fit) on the molecules, the riding hydrogens (and their tensors, with the TLS fit if there
    is one), the bond table and the angle and torsion tables (with that fit as well) and the site average."""
    device = batch.x.device
    B = int(batch.num_graphs)
    sel = batch._meta[:B]
    ex = adp_export(pred, row_ptr, batch.cell, axes=True, stats=True, check=False)
    dev = dict(u_cart=pred, u_cif=ex.u_cif, u_eq=ex.u_eq, principal=ex.principal, axes=ex.axes,
               stats=ex.crystal_stats, _status=ex.status)
    if analyses.rigid_bond is not None:
        dev.update(bond_entries(bond_test(pred, graph, row_ptr, *analyses.rigid_bond), batch))
    tf = None
    if mo is not None:
        dev.update(molecule_entries(mo, molecule_test(pred, graph, row_ptr, mo, analyses.rigid_molecule[1]), batch))
        if analyses.tls_fit:
            tf = tls_fit_call(pred, graph, row_ptr, mo)
            dev.update(tls_entries(tf))
    if analyses.riding_h is not None:
        rh = riding_h_call(ex.u_eq, graph, *analyses.riding_h)
        dev.update(riding_entries(rh, batch))
        if analyses.aniso_h is not None:
            ah = aniso_h_call(pred, graph, row_ptr, rh, mo if tf is not None else None, tf, *analyses.aniso_h)
            dev.update(aniso_entries(ah, batch))
    if index is not None:
        dev.update(bond_table_entries(bond_table_call(pred, graph, row_ptr, index, tf), batch))
    if angles is not None:
        dev.update(angle_table_entries(angle_table_call(graph, row_ptr, angles, tf), batch))
    if sym is not None:
        from .symmetry import site_average
        dev["u_cif_asym"], dev["spread"] = site_average(pred, row_ptr, batch._sel, sym)
        if analyses.riding_h is not None:                                     # what riding_asym takes, per site and per atom
            counts = torch.from_numpy(sym.site_count[batch._sel]).to(device)
            crystal = torch.repeat_interleave(torch.arange(B, device=device), counts,
                                              output_size=int(dev["u_cif_asym"].shape[0]))
            dev["_ueq_asym"] = u_eq_of_cif(dev["u_cif_asym"], sym.cell[sel].view(B, 3, 3)[crystal])
            dev["_parent_asym"] = parent_asym(rh.parent, batch, row_ptr, sym)
    return dev


def _host_stage(out: Dict[str, List], series: Dict[str, List], host: dict, shard, sym, kelvin: Optional[list] = None) -> None:
    """Appends the entries of one batch to ``out`` from the host copy of ``_device_stage``'s dict: one ``_entries`` per
    prediction on its keys, the entries crystal-major (crystal g at temperature t is entry ``g*T + t`` of the batch), and
    with T >= 2 the batch's crystals to ``series``."""
    T = 1 if kelvin is None else len(kelvin)
    shared = {k: v for k, v in host.items() if "@" not in k and k not in SERIES_SPLIT}
    stage = [out] if T == 1 else [{k: [] for k in out} for _ in range(T)]
    for t in range(T):
        mine = {k.rpartition("@")[0]: v for k, v in host.items() if k.endswith(f"@{t}")}
        names, counts = _entries(stage[t], {**shared, **mine}, shard, sym, None if kelvin is None else kelvin[t])
    if T >= 2:
        for g in range(len(names)):
            for per in stage:
                for k in out:
                    out[k].append(per[k][g])
        _split(series, {k: host[k] for k in SERIES_KEYS}, counts)
        series["name"] += names
        series["temps"] += [torch.tensor(kelvin, dtype=torch.float32) for _ in names]


def _split(out: Dict[str, List], host: dict, counts: dict) -> None:
    """Appends to ``out[k]`` the crystals' pieces of every host tensor ``host[k]``, cut as ``CUT[k]`` says."""
    for k, t in host.items():
        kind = CUT[k]
        out[k] += [c.clone() for c in t.unbind(0)] if kind == "crystal" else split_rows(t, counts[kind])


def _entries(out: Dict[str, List], host: dict, shard, sym, kelvin: Optional[float] = None):
    """Appends the crystals of one batch to ``out`` from the host copy of one prediction of it; ``kelvin``: the
    temperature it was predicted at, which then is its ``temp`` and the suffix of its ``name``, instead of the stored
    one.  Returns the crystals' names (as stored) and their counts of rows, atoms, sites, listed bonds, angles and
    torsions."""
    ids = host.pop("_sel").tolist()
    names = [shard.names[i] if shard.names is not None else f"crystal{i}" for i in ids]
    check_export_status(host.pop("_status"), names)
    rp, ap = host.pop("_row_ptr"), host.pop("_atom_ptr")
    bp, gp, tp = (host.pop(k, None) for k in ("_bond_ptr", "_angle_ptr", "_torsion_ptr"))
    counts = {"row": (rp[1:] - rp[:-1]).tolist(), "atom": (ap[1:] - ap[:-1]).tolist(),
              "site": [int(sym.site_count[i]) for i in ids] if sym is not None else None,
              "bond": (bp[1:] - bp[:-1]).tolist() if bp is not None else None,
              "angle": (gp[1:] - gp[:-1]).tolist() if gp is not None else None,
              "torsion": (tp[1:] - tp[:-1]).tolist() if tp is not None else None}
    stored = host.pop("_temp").tolist() if "_temp" in host else [float("nan")] * len(ids)
    out["temp"] += stored if kelvin is None else [kelvin] * len(ids)          # the Kelvin value as given
    out["name"] += names if kelvin is None else [f"{name}_{kelvin:g}K" for name in names]
    riding = "_ueq_asym" in host                                              # what riding_asym takes, per site and per atom
    ueq_sites = split_rows(host.pop("_ueq_asym"), counts["site"]) if riding else None
    parents = split_rows(host.pop("_parent_asym"), counts["atom"]) if riding else None
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
                 temperatures=None, rigid_molecule=None, tls_fit=None, aniso_h=None, bond_table=None,
                 angle_table=None, model_frame=None) -> Dict[str, List]:
    """Predicted ADPs of every crystal of ``loader`` (a ``ShardLoader``; a labeled shard's ``y`` is ignored).  Returns a
    dict of lists with one entry per crystal, in the loader's order, under the keys of ``GROUPS["base"]``; a singular cell
    raises ``ValueError`` naming the crystal.  Every option adds what its row of ``GROUPS`` documents, all of it
    travelling in the batch's one copy, with the keys in the order of ``result_keys``; ``None`` (``rotations`` = 1) is the
    pass as it always was.  ``sym``: row ``symmetry``; ``rotations`` with ``seed``: ``rotations``; ``temperatures``:
    ``series`` (one entry per crystal and temperature, and the key ``series``); ``rigid_bond``, ``riding_h``,
    ``rigid_molecule``, ``tls_fit`` (``ValueError`` without ``rigid_molecule``) and ``aniso_h`` (``ValueError`` without
    ``riding_h``): the rows of their names, for the two hydrogen options with ``sym`` also the rows ``*_symmetry``;
    ``bond_table`` and ``angle_table`` (the bond tolerance): the row ``bond_table`` and the rows ``angle_table`` and
    ``torsion_table``, the analyses that are no field of ``Analyses``.  ``model_frame`` (the loader's shard
    ``.with_optimized_cell()``, for iComformer): the row ``model_frame``; it raises ``ValueError`` with ``rotations`` > 1,
    because iComformer's features are invariant and ``replicate`` rotates ``cart_dir`` but not ``cell``: K frames would
    feed it inconsistent inputs, and nothing would be averaged."""
    rotations = int(rotations)
    analyses = Analyses(rigid_bond, riding_h, rigid_molecule, tls_fit, aniso_h).checked()
    shard = _check_pass(loader, rotations)
    if model_frame is not None:
        if rotations > 1:
            raise ValueError("predict_adps: model_frame serves one frame only (rotations = 1): the model's features are "
                             "invariant, and the K frames rotate cart_dir but not cell, so they would feed it inconsistent "
                             "inputs and nothing would be averaged")
        import numpy as np
        if (model_frame.num_graphs != shard.num_graphs or "rotation" not in model_frame.t
                or not np.array_equal(model_frame.atom_ptr, shard.atom_ptr)
                or not np.array_equal(model_frame.edge_ptr, shard.edge_ptr)):
            raise ValueError("predict_adps: model_frame must be the with_optimized_cell() of the loader's shard (the same "
                             "crystals with the same graph)")
    kelvin = None if temperatures is None else check_temperatures(temperatures, least=1, name="temperatures")
    model.eval()
    out: Dict[str, List] = {k: [] for k in result_keys(analyses, sym is not None, rotations, bond_table, angle_table,
                                                          model_frame is not None)}
    series: Dict[str, List] = {k: [] for k in ("name", "temps") + SERIES_KEYS}
    gen = torch.Generator(device=device).manual_seed(seed) if rotations > 1 else None
    temps = None if kelvin is None else standardised(kelvin, loader.temp_mean, loader.temp_std, device)
    with torch.no_grad():
        for batch in loader:
            if batch is None:
                continue
            batch.to(device)
            dev = _device_stage(model, batch, shard, sym, rotations, gen, analyses, kelvin, temps, bond_table,
                                angle_table, model_frame)
            _host_stage(out, series, to_host(dev), shard, sym, kelvin)
    if hasattr(model, "flush_graph_checks"):
        model.flush_graph_checks()
    if GROUPS["series"].present(analyses, sym is not None, rotations, kelvin):
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


def _ratio(total: float, count: int) -> float:
    return total / count if count > 0 else 0.0


# The figures of a whole pass from one kernel's fp64 per-crystal statistics, each formula once and in the order of the
# result line (not the key order of a result): stats key -> (its width, ``figures(s, hi, rows)``), ``s`` the per-column
# sums and ``hi`` the per-column maxima as Python floats, 0 for a pass without crystals.  ``pass_statistics`` takes them
# from a result's stacked statistics, ``evaluate.inference`` from sums it accumulates on the device.
STATISTICS = {
    "t_stats": (4, lambda s, hi, rows: {                                      # rows: those of ONE temperature
        "ueq_slope_mean": s[0] / max(rows, 1), "non_increasing_rows": int(s[1]), "rows_with_drops": int(s[2]),
        "series_resid_max": hi[3]}),
    "rot_stats": (2, lambda s, hi, rows: {"rot_spread_max": hi[1], "rot_spread_mean": s[0] / max(rows, 1)}),
    "bond_stats": (4, lambda s, hi, rows=0: {                                 # over the directed bonds of the pass
        "bonds": int(s[0]), "rigid_bond_mean": _ratio(s[1], int(s[0])), "rigid_bond_max": hi[2],
        "rigid_bond_over": int(s[3])}),
    "h_stats": (4, lambda s, hi, rows=0: {                                    # the mean is over the non-orphans
        "hydrogens": int(s[0]), "h_orphans": int(s[1]), "h_uiso_mean": _ratio(s[2], int(s[0]) - int(s[1])),
        "h_non_positive": int(s[3])}),
    "h_aniso_stats": (4, lambda s, hi, rows=0: {
        "h_aniso": int(s[0]), "h_aniso_tls": int(s[1]), "h_aniso_ueq_mean": _ratio(s[2], int(s[0])),
        "h_aniso_non_positive": int(s[3])}),
    "mol_stats": (9, lambda s, hi, rows=0: {                                  # over the entries: once per temperature
        "molecules": int(s[0]), "molecules_tested": int(s[1]), "molecules_periodic": int(s[2]),
        "molecules_open": int(s[3]), "molecule_atoms_max": int(hi[4]), "rigid_molecule_pairs": int(s[5]),
        "rigid_molecule_mean": _ratio(s[6], int(s[5])), "rigid_molecule_max": hi[7], "rigid_molecule_over": int(s[8])}),
    "tls_stats": (6, lambda s, hi, rows=0: {                                  # tls_r over all fitted rows of the pass
        "tls_molecules": int(s[0]), "tls_rank_deficient": int(s[1]), "tls_nonphysical": int(s[2]),
        "tls_r": math.sqrt(s[3] / s[4]) if s[4] > 0 else 0.0, "tls_resid_max": hi[5]}),
    "bonds_stats": (9, lambda s, hi, rows=0: {                                # the libration figures: corrected - apparent
        "bonds_listed": int(s[0]), "bonds_unlisted": int(s[1]), "bond_length_mean": _ratio(s[2], int(s[0])),
        "bond_libration_bonds": int(s[5]), "bond_libration_mean": _ratio(s[6], int(s[5])), "bond_libration_max": hi[7],
        "bond_bounds_nan": int(s[8])}),
    "angles_stats": (5, lambda s, hi, rows=0: {                               # the libration figures: |corrected - apparent|
        "angles_listed": int(s[0]), "angle_mean": _ratio(s[1], int(s[0])), "angle_libration_angles": int(s[2]),
        "angle_libration_mean": _ratio(s[3], int(s[2])), "angle_libration_max": hi[4]}),
    "torsions_stats": (5, lambda s, hi, rows=0: {                             # ... on the circle
        "torsions_listed": int(s[0]), "torsions_undefined": int(s[1]), "torsion_libration_torsions": int(s[2]),
        "torsion_libration_mean": _ratio(s[3], int(s[2])), "torsion_libration_max": hi[4]}),
}


def _columns(stats: List[torch.Tensor], width: int):
    """``(sums, maxima)`` per column of a list of [width] fp64 per-crystal statistics, each column reduced on its own."""
    columns = (torch.stack(stats) if stats else torch.zeros(0, width, dtype=torch.float64)).unbind(1)
    return [float(c.sum()) for c in columns], [float(c.max()) if stats else 0.0 for c in columns]


def pass_statistics(out: Dict[str, List], output: Optional[str] = None, cif_dir: Optional[str] = None, rejected=None,
                    rotations: int = 1, temperatures: Optional[list] = None) -> dict:
    """The result line of a whole ``predict_adps`` pass from its result ``out`` (``rotations`` and ``temperatures`` as the
    pass was given them), summed from the kernels' fp64 per-crystal statistics: ``crystals``, ``rows``, ``u_eq_mean`` and
    ``non_positive_rows``, then ``output`` and ``cif_dir`` as given and the number of ``rejected`` crystals if there is
    such a list (``load_input``); with ``temperatures`` ``entries`` and ``temperatures``; then, for every statistics key
    of ``STATISTICS`` that the result (for ``t_stats`` its ``series``) has, that key's figures, with ``rotations`` in front
    of the frames'.  A pass without crystals gives zeros."""
    n = len(out["name"])                                  # entries: one per crystal, or per crystal and temperature
    rows = sum(int(t.shape[0]) for t in out["u_eq"])
    sums, _ = _columns(out["stats"], 3)
    res = {"crystals": n // len(temperatures) if temperatures else n, "rows": rows,
           "u_eq_mean": sums[0] / max(rows, 1), "non_positive_rows": int(sums[2]), "output": output, "cif_dir": cif_dir}
    if rejected is not None:
        res["rejected"] = len(rejected)
    if temperatures is not None:
        res.update(entries=n, temperatures=temperatures)
    for key, (width, figures) in STATISTICS.items():
        of = out.get("series", {}) if key == "t_stats" else out
        if key in of:
            if key == "rot_stats":
                res["rotations"] = rotations
            res.update(figures(*_columns(of[key], width), rows // len(temperatures) if key == "t_stats" else rows))
    return res


def entry(result: Dict[str, List], k: int) -> dict:
    """Crystal ``k`` of a ``predict_adps`` result: what ``write_cif`` (and, with the keys of a ``CifSymmetry``,
    ``write_cif_symmetric``) takes."""
    return {key: result[key][k] for g in GROUPS.values() for key in g.cuts if key in result}


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
