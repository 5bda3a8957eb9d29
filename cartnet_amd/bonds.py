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

Molecules (``metrics.molecules``, csrc/molecule_ops.hip; ``molecules_host`` below restates it in numpy).  The bond graph
has the directed edges of the rigid-bond test: ``e = (j -> i)`` is a bond when ``is_bond(cart_dist[e], z_i, z_j, tol,
same_atom = i == j)`` holds and both ends have an ADP row.  An atom's own image is no bond, as in the rigid-bond test: a
chain that bonds only to its own image (one atom per cell along the chain) is therefore seen as single atoms, not as a
polymer.  A molecule is a component of that graph, defined as the fixpoint of a Jacobi propagation per crystal:

  start       every atom with a row has ``label[i] = i`` and ``x[i] = 0`` (fp64, three components); an atom without a row
              has label -1 and takes no part.
  sweep       reads the previous sweep's values only.  Atom ``i`` takes the smallest label among the sources of its
              incoming bonds; if it is below its own, ``i`` adopts it together with
              ``x[i] = x[j] + fp64(cart_dist[e]) * fp64(cart_dir[e])`` along the edge that carries it -- the lowest edge
              index when several do.  The stored direction is ``pos_target - pos_source_image`` (synthetic.py:50), so the
              sum is the unwrapped position of ``i`` relative to the molecule's root, its lowest atom.
  end         when no label changes; the number of sweeps is bounded by the atoms of the crystal.
  status      one pass over all bonds ``j -> i`` after the fixpoint.  ``label[i] != label[j]``: the graph is asymmetric
              there (a capped graph can be: ``--max_neighbours``, eComformer) and both molecules get bit 2, *open*.
              Equal labels with ``|x[i] - (x[j] + v_e)|^2 > 0.25 A^2``: the molecule reaches its own image, as a polymer
              or a framework does, and gets bit 1, *periodic*.  0.5 A is far above the rounding of ``x`` and far below any
              lattice translation.  A molecule is *tested* when its status is 0 and it has two or more atoms.
  numbering   ``mol[m]``: the index of the row's molecule inside its crystal, molecules numbered in the order of their
              roots; ``mol_size[m]`` and ``mol_status[m]`` repeat the molecule's figures on each of its rows.

The rigid-body test on top of it (``metrics.molecule_test``; Rosenfield, Trueblood & Dunitz, Acta Cryst. A34 (1978) 828)
generalises Hirshfeld's test from bonds to all pairs of a tested molecule: for the row of atom ``i``, over the atoms
``j != i`` of its molecule in atom order and in fp64, ``r = x_i - x_j`` and ``D = r^T (S_i - S_j) r / (r . r)`` with ``S``
the symmetric part of ``U`` (the difference is taken first); a pair with ``r . r == 0`` is not counted.

The TLS fit (``metrics.tls_fit``, csrc/tls_ops.hip; ``tls_fit_host`` below restates it in numpy; Schomaker & Trueblood,
Acta Cryst. B24 (1968) 63): how much of a molecule's ADPs is rigid-body motion, which motion, and what is left per atom.

  fitted      a molecule whose status is 0 and that has at least ``TLS_MIN_ATOMS`` = 5 rows (the design matrix of any
              four points has rank <= 18); rows of other molecules get the neutral values ``u_tls`` / ``params`` /
              ``eig`` NaN, ``resid`` 0, ``rank`` 0, ``rfac`` 0.
  geometry    ``c``: the fp64 mean of ``x`` over the molecule's atoms, summed in atom order; ``r_i = x_i - c``;
              ``rho = sqrt(mean |r_i|^2)``, summed in atom order.  ``rho == 0``: not fitted, neutral rows.
  model       ``U(r) = T + A L A^T + A S + S^T A^T`` with ``A(r) = [[0, z, -y], [-z, 0, x], [y, -x, 0]]`` (``u = t +
              lambda x r``), ``T`` and ``L`` symmetric, ``S = <lambda t^T>`` a general 3x3 matrix with ``tr S = 0`` (the
              trace cannot be determined: ``A + A^T = 0``).  20 parameters: T (6) and L (6) in the order 11, 22, 33,
              23, 13, 12 (``u_cif``'s), then S (8) in the order 11, 22, 12, 13, 21, 23, 31, 32 with ``S33 = -(S11 +
              S22)``.  The fit is done in scaled units ``r / rho``, ``L rho^2``, ``S rho``: all columns are O(1).
  objective   minimise ``sum_i |Sym(U_i) - U(r_i)|_F^2``; ``Sym(U_i)`` in fp64 from the fp32 entries.  Six observations
              per atom in the order of T's parameters, the off-diagonal ones weighted sqrt(2): the row of ``J_i`` for the
              observation (p, q) holds ``w_pq dU_pq / dparam`` (``tls_design``).
  solve       ``N = J^T J`` (20 x 20) and ``b = J^T y``, fp64, summed over the atoms in atom order.  The eigenvalues of
              ``N`` by cyclic Jacobi (``jacobi_eigh``): a sweep is the 19 rounds of the round-robin ordering, ten
              disjoint rotations a round, all of a round taken from the matrix as the round found it.  Before every
              sweep: done when ``sum_{i != j} N_ij^2 <= TLS_JACOBI_TOL^2 sum_i N_ii^2`` with ``TLS_JACOBI_TOL`` = 1e-15;
              never more than ``TLS_MAX_SWEEPS`` = 30 sweeps.  The eigenvalues ``l_k > TLS_RANK_EPS l_max``
              (``TLS_RANK_EPS`` = 1e-10) are kept, ``rank`` is their number and
              ``p = V_kept diag(1 / l) V_kept^T b``: the minimum-norm solution in the scaled parameters.  A rank below
              20 is no error: a planar or a linear molecule has one.  The fitted ``U(r_i)`` and the residuals are
              unique all the same; T, L and S are then the minimum-norm representative.  Sweeps used up: ``rank = -1``
              and every other output NaN.
  molecule    ``T``, ``L``, ``S`` about ``c`` (unscaled: ``L / rho^2``, ``S / rho``); ``origin = c``, relative to the
              root atom as ``x`` is; ``rfac = sqrt(sum |resid_i|^2 / sum |Sym U_i|_F^2)`` (0 if the denominator is);
              the principal values of ``T`` and of ``L`` ascending, by the same Jacobi routine at n = 3.
  row         ``u_tls = U(r_i)`` and ``resid = |Sym U_i - u_tls|_F``.  fp64 throughout, one rounding to fp32 on store.
  crystal     fitted molecules (``rank != 0``, counted at their roots), those of them with ``rank < 20``, those whose
              smallest principal value of ``T`` or of ``L`` is negative, and over the rows of the fitted molecules the
              sum of ``resid^2`` as stored, the sum of ``|Sym U|_F^2`` and the largest ``resid`` (a NaN is kept).

Anisotropic hydrogens (``metrics.aniso_h``, csrc/aniso_h_ops.hip; ``aniso_hydrogens_host`` below restates it in numpy):
a full tensor for every hydrogen from what the three rules above give -- the decomposition of SHADE (Madsen, J. Appl.
Cryst. 39 (2006) 757) and of ADPH (Roversi & Destro, Chem. Phys. Lett. 386 (2004) 472): rigid-body motion plus internal
X-H motion.  Per atom ``i`` of a batch, ``u_h[i]`` [3,3] fp32 and ``source[i]`` int32:

  heavy       a non-hydrogen atom with a row: ``u_h[i] = u[atom_row[i]]`` copied bit for bit, ``source = 1``; without a
              row NaN, ``source = 0``.
  orphan      a hydrogen with ``parent[i] < 0`` (riding's orphans; also a parent out of range or without a row): NaN,
              ``source = 0``.
  edge        for a hydrogen with parent ``p``: among the edges ``p -> i`` of ``i``'s segment the one with the smallest
              ``cart_dist``, a tie going to the lowest edge index (a NaN distance is never taken) -- the edge the riding
              rule chose.  ``v = fp64(cart_dist[e]) * fp64(cart_dir[e])`` is the vector from the parent's image to the
              hydrogen: from the edge, never from ``pos``, so cell faces do not matter.  No such edge, or ``|v|^2`` not
              ``> 0``: NaN, ``source = 0``.  Otherwise ``d = v / |v|``.
  tensor      ``u_h[i] = Sym(U_p) + D_lib + U_int`` in fp64 with one rounding to fp32; the six components of the upper
              triangle are computed and stored on both sides of the diagonal, so the stored tensor is exactly symmetric.
  internal    ``U_int = stretch * d d^T + bend * (I - d d^T)``: ``stretch`` along the bond, ``bend`` in both directions
              across it.  ``ANISO_H_STRETCH`` = 0.005 A^2 and ``ANISO_H_BEND`` = 0.020 A^2, independent of the
              temperature, are this project's NOMINAL figures: of the order of the internal X-H mean-square displacements
              that neutron studies report, written from memory of that literature and not checked against a table;
              nothing here can verify them.  They are arguments so that a user can put in values of their choice.
  libration   ``D_lib = U_LS(r_p + v) - U_LS(r_p)`` with ``U_LS(r) = A(r) L A(r)^T + A(r) S + S^T A(r)^T`` and ``A`` =
              ``tls_cross``'s: how the fitted rigid-body motion of the parent's molecule grows from the parent's position
              to the hydrogen's (``T`` cancels).  ``L``, ``S`` and the origin ``c`` are read from the parent's row of
              ``tls_fit``'s ``params`` AS STORED in fp32, converted to fp64; ``r_p = x[p] - c`` with ``x`` the fp64
              positions of ``molecules``.  The term exists only when TLS results are passed and
              ``rank[atom_row[p]] > 0``: then ``source = 3`` for rank 20 and ``source = 4`` for a lower rank, where ``L``
              and ``S`` are the minimum-norm representative -- for a planar molecule the out-of-plane part of a
              hydrogen's libration is then the representative's, not a determined quantity.  Otherwise (no TLS passed, a
              molecule not fitted, rank 0 and rank -1) ``D_lib = 0`` and ``source = 2``.
  crystal     over the crystal's atoms in order, from the values as stored: the hydrogens with a tensor (``source >= 2``),
              those of them with ``source >= 3``, the sum of their ``trace / 3`` (fp64), and those whose tensor is not
              positive definite by Sylvester's criterion -- the three leading minors ``> 0`` in fp64 on the stored
              values; a NaN counts as not positive.

Using the parent's own tensor plus the CHANGE of the fitted motion keeps a hydrogen consistent with its parent even where
the fit is poor; SHADE uses the fitted tensor at the hydrogen instead.  For exactly rigid rows (``U_p = U_TLS(r_p)``) the
two coincide: ``u_h = U_TLS(r_p + v) + U_int``.

The bond table (``metrics.bond_index`` and ``metrics.bond_table``, csrc/bond_table_ops.hip; ``bond_table_host`` below
restates both in numpy): one entry per bond where the rules above give figures per atom -- Hirshfeld's ``D`` with its
sign, the model-free bounds of Busing & Levy (Acta Cryst. 17 (1964) 142) on the thermally averaged bond length, and the
length corrected for the libration of the fitted rigid body (Cruickshank, Acta Cryst. 9 (1956) 757; Schomaker &
Trueblood 1968), the geometric product of a TLS analysis that THMA11 and PLATON print.

  bonds       a directed edge ``e = (j -> i)`` is a bond exactly as for the rigid-bond test: ``is_bond`` and both ends with
              an ADP row, every atom of the batch admissible as a source.
  listed      the bonds with ``j < i`` (batch atom indices): a symmetric graph lists every bond once; a pair bonded
              through two different images is two entries.  Entries come in target order and within a target in edge
              order -- the graph's own order.
  unlisted    the bond edges with ``j > i`` are counted per atom ``i`` and per crystal and never listed.  A graph capped
              by ``--max_neighbours`` can hold a bond in one direction only: a crystal whose unlisted count differs from
              its listed count has an asymmetric graph.
  entry       ``a = j``, ``b = i``; ``dir = cart_dir[e]`` and ``length = cart_dist[e]`` as stored, ``d`` and ``l`` below.
              All arithmetic is fp64 from the fp32 inputs, and every stored value is rounded once.
  delta       ``d^T (Sym U_b - Sym U_a) d``, signed: the difference first, then ``_form`` (``bg_form`` of
              csrc/bond_graph.h).  ``|delta|`` is the ``|D|`` the rigid-bond test folds for row ``b``.
  bounds      ``w_x^2 = tr(U_x) - d^T Sym(U_x) d``, the mean-square displacement of atom ``x`` across the bond (the
              trace summed 11 + 22 + 33).  ``lower = l + (sqrt(w_b^2) - sqrt(w_a^2))^2 / (2 l)`` and ``upper = l +
              (sqrt(w_b^2) + sqrt(w_a^2))^2 / (2 l)``: fully correlated and fully anti-correlated motion across the bond.
              A negative ``w^2`` (a row that is not positive definite) or a NaN row gives NaN in both, the square root's
              own answer; such a bond is still listed, and counted.
  libration   ``| r + 1/2 (tr(L) I - L) r |`` with ``r = l d``: the bond between the mean positions of two atoms of a
              body that librates with ``L``.  ``L`` is ``params[atom_row[b], 6:12]`` (11 22 33 23 13 12) of the TLS fit AS
              STORED in fp32; filled where ``rank[atom_row[b]] > 0``, NaN otherwise and without TLS results.  It does not
              depend on ``S`` or on the origin.  A bond lies inside one molecule, so both ends share the fit.
  tls_rank    ``rank[atom_row[b]]``, 0 without TLS results: below 20, ``L`` is the minimum-norm representative (a planar
              or linear molecule), which a user may want to set aside as ``source`` 3 against 4 does for hydrogens.
  crystal     from the values as stored, a bond belonging to the crystal of ``b``: listed, unlisted, the sum of
              ``length``, the sum of ``|delta|``, the largest ``|delta|`` (a NaN is kept), the entries with a finite
              ``libration``, the sum and the largest of ``libration - length`` over those (0 without one), and the
              entries with a NaN bound.

Not in the table: X-H bonds (a hydrogen has no ADP row) and the riding-model correction, which needs a choice of which
atom rides on which.  Angles and torsions have tables of their own, below.

The angle and torsion tables (``metrics.angle_index`` and ``metrics.angle_table``, csrc/angle_table_ops.hip;
``angle_table_host`` below restates them in numpy): the valence angles and the torsions of the bond graph, each with the
value the fitted libration gives, as THMA11 and PLATON print them beside the corrected distances.  Both are built from
the edges of the radius graph alone (``cart_dir``, ``cart_dist``), never from ``pos``: cell faces and images need no
special case.

  adjacency   a directed edge ``e = (j -> i)`` is a bond exactly as for the bond table.  Atom ``i``'s adjacency is the
              bond edges that name it as their target, in edge order, sources ``j < i`` and ``j > i`` alike; its degree
              ``d_i`` is ``counts[i] + unlisted[i]`` of the bond table's index.
  angles      for a centre ``i`` every pair ``k1 < k2`` of positions in its adjacency, ordered by ``k1`` then ``k2``:
              ``d (d - 1) / 2`` entries, entry ``(k1, k2)`` in slot ``k1 (2 d - k1 - 1) / 2 + (k2 - k1 - 1)`` of the atom;
              centres in atom order.  ``a = src[e1]``, ``b = i``, ``c = src[e2]``.  ``value = atan2(|p x q|, p . q)`` in
              degrees with ``p, q = fp64(cart_dir[e1]), fp64(cart_dir[e2])`` as stored: both point into the centre, so the
              angle is that of the outward vectors; ``atan2`` and not ``acos``, which loses half its digits at 180.  A
              pair bonded through two images has two adjacency entries and therefore an angle, as it has two bonds.
  torsions    the central bond is a listed bond of the bond table, edge ``e0 = (b -> c)`` with ``b < c``, in the bond
              table's order.  The ``d`` side: the bond edges ``ed`` of ``c``'s adjacency other than ``e0``, in order.  The
              ``a`` side: the bond edges ``ea`` of ``b``'s adjacency other than the reverse of ``e0``, in order.  The
              entry is ``(a = src[ea], b, c, d = src[ed])`` in slot ``ia * n_d + id`` of the bond.  With ``b1 =
              dir[ea]``, ``b2 = dir[e0]``, ``b3 = -dir[ed]`` (fp64 of the stored fp32), ``n1 = b1 x b2`` and ``n2 = b2 x
              b3``: ``value = atan2(|b2| (b1 . n2), n1 . n2)`` in degrees, the IUPAC sign; an fp32 result of -180 is
              stored as +180; NaN when ``n1 . n1 == 0`` or ``n2 . n2 == 0`` (a collinear end).  A three-membered ring
              gives torsions with ``a == d``: they are listed, and a user who does not want them filters on the indices.
  reverse     the reverse of ``e0``: among the bond edges ``e'`` of ``b``'s adjacency with ``src[e'] == c`` the one with
              the smallest ``m = max_k |s_k|``, ``s_k = fp32(fp32(dist[e'] dir[e'][k]) + fp32(dist[e0] dir[e0][k]))`` --
              fp32, two products and their sum -- and the maximum taken as ``m = |s_0|``, then ``|s_1|`` and ``|s_2|`` in
              turn where they are greater (a NaN in ``s_0`` is never chosen).  Candidates in edge order with a strict
              ``<``: a tie keeps the lowest edge.  Accepted only if ``m < MOLECULE_CLOSURE`` (0.5 A).  Without one --
              a capped graph that holds the bond in one direction only -- nothing is excluded on the ``a`` side.
  libration   filled only with TLS results and where ``rank[row] > 0``, the row being ``b``'s for an angle and ``c``'s
              for a torsion (a fit is per molecule: the choice only fixes which copy is read).  Every vector ``v =
              fp64(cart_dist) fp64(cart_dir)`` is replaced by ``v' = v + 1/2 (tr(L) v - L v)`` with ``L = params[row,
              6:12]`` as stored and in the bond table's operation order, and the same two formulae run on the ``v'``
              (``b3' = -v'(ed)``; -180 is stored as +180 here too).  A torsion that is NaN by the raw criterion is NaN.
              Otherwise NaN; ``tls_rank`` is the row's rank, 0 without TLS results.
  arithmetic  cross products as ``p_y q_z - p_z q_y`` (cyclic), dot products and squares as ``(x x' + y y') + z z'``,
              all in fp64 without contraction; the degree factor is the fp64 constant 57.29577951308232; one rounding
              to fp32 on store.
  crystal     fp64, from the values as stored; an angle belongs to the crystal of ``b``, a torsion to that of ``c``.
              ``angle_stats`` [5]: entries, sum of ``value``, entries with a finite ``libration``, sum and largest of
              ``|libration - value|`` over those.  ``torsion_stats`` [5]: entries, entries with a NaN ``value``, entries
              with a finite ``libration``, sum and largest of the circular ``|libration - value|`` (``min(x, 360 - x)``)
              over those.

Not in these tables: X-H geometry, non-bonded contacts, standard uncertainties, and the S / origin part of the correction.
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


MOLECULE_PERIODIC, MOLECULE_OPEN = 1, 2        # the bits of a molecule's status
MOLECULE_CLOSURE = 0.5                         # Angstrom: a bond that disagrees with x by more reaches an image


def molecules_host(z, edge_index, cart_dist, cart_dir, atom_row, ptr=None, tol: float = BOND_TOLERANCE) -> dict:
    """The molecule rule of the module docstring in plain numpy: a dict with ``label`` [N] int64, ``x`` [N,3] fp64,
    ``mol`` / ``size`` / ``status`` [M] int32, ``crystal_counts`` [B,5] fp64 (molecules, tested, periodic, open, largest
    size) and ``sweeps`` [B] int64, the sweeps each crystal took including the last one that changed nothing.  ``z`` [N];
    ``edge_index`` [2,E] = (source, target); ``cart_dist`` [E] and ``cart_dir`` [E,3] fp32; ``atom_row`` [N]: an atom's row
    or -1 (M is the largest row plus one); ``ptr`` [B+1]: the crystals' atom offsets (``None``: one crystal).  An edge
    between atoms of different crystals is no bond."""
    z = np.asarray(z, dtype=np.int64).reshape(-1)
    src, tgt = (np.asarray(a, dtype=np.int64).reshape(-1) for a in np.asarray(edge_index).reshape(2, -1))
    dist = np.asarray(cart_dist, dtype=np.float32).reshape(-1)
    dirs = np.asarray(cart_dir, dtype=np.float32).reshape(-1, 3)
    atom_row = np.asarray(atom_row, dtype=np.int64).reshape(-1)
    N = z.shape[0]
    M = int(atom_row.max()) + 1 if N else 0
    ptr = np.asarray([0, N] if ptr is None else ptr, dtype=np.int64).reshape(-1)
    B = len(ptr) - 1
    crystal = np.searchsorted(ptr, np.arange(N), side="right") - 1
    inside = (src >= 0) & (src < N) & (tgt >= 0) & (tgt < N)
    s, t = np.where(inside, src, 0), np.where(inside, tgt, 0)
    has_row = atom_row >= 0
    bond = inside & (crystal[s] == crystal[t]) & has_row[s] & has_row[t] & is_bond(dist, z[t], z[s], tol, same_atom=s == t)
    be = np.nonzero(bond)[0]                                      # the bond edges, in edge order
    s, t = s[be], t[be]
    v = dist[be].astype(np.float64)[:, None] * dirs[be].astype(np.float64)
    label = np.where(has_row, np.arange(N, dtype=np.int64), -1)
    x = np.zeros((N, 3), dtype=np.float64)
    sweeps = np.ones(B, dtype=np.int64)
    for _ in range(N + 1):
        # per target the edge with the smallest source label, the lowest edge among equals
        order = np.lexsort((np.arange(len(be)), label[s], t))
        first = np.ones(len(order), dtype=bool)
        first[1:] = t[order][1:] != t[order][:-1]
        w = order[first]
        w = w[label[s[w]] < label[t[w]]]
        if not len(w):
            break
        new_label, new_x = label.copy(), x.copy()                # Jacobi: the sweep reads the previous values only
        new_label[t[w]] = label[s[w]]
        new_x[t[w]] = x[s[w]] + v[w]
        label, x = new_label, new_x
        sweeps[np.unique(crystal[t[w]])] += 1
    root = np.nonzero(label == np.arange(N))[0]                   # ascending: the order of the molecules
    open_, periodic = np.zeros(N, dtype=bool), np.zeros(N, dtype=bool)     # per root atom
    differ = label[s] != label[t]
    open_[label[s[differ]]] = True
    open_[label[t[differ]]] = True
    gap = x[t] - (x[s] + v)
    far = ~differ & ((gap * gap).sum(1) > MOLECULE_CLOSURE ** 2)
    periodic[label[t[far]]] = True
    status_of = periodic * MOLECULE_PERIODIC + open_ * MOLECULE_OPEN
    size_of = np.bincount(label[has_row], minlength=N) if N else np.zeros(0, dtype=np.int64)
    number_of = np.zeros(N, dtype=np.int64)
    number_of[root] = np.arange(len(root)) - np.searchsorted(root, ptr[crystal[root]])   # roots of the crystal below it
    rows = np.nonzero(has_row)[0]
    mol, size, status = (np.zeros(M, dtype=np.int32) for _ in range(3))
    mol[atom_row[rows]] = number_of[label[rows]]
    size[atom_row[rows]] = size_of[label[rows]]
    status[atom_row[rows]] = status_of[label[rows]]
    counts = np.zeros((B, 5), dtype=np.float64)
    for g in range(B):
        r = root[(root >= ptr[g]) & (root < ptr[g + 1])]
        st, sz = status_of[r], size_of[r]
        counts[g] = (len(r), ((st == 0) & (sz >= 2)).sum(), (st & MOLECULE_PERIODIC > 0).sum(),
                     (st & MOLECULE_OPEN > 0).sum(), sz.max() if len(r) else 0)
    return {"label": label, "x": x, "mol": mol, "size": size, "status": status, "crystal_counts": counts,
            "sweeps": sweeps}


TLS_MIN_ATOMS = 5              # four points never determine the model: their design matrix has rank <= 18
TLS_PARAMS = 20                # T (6), L (6), S (8: the trace is fixed at 0)
TLS_RANK_EPS = 1e-10           # eigenvalues of the normal matrix above this fraction of the largest are kept
TLS_JACOBI_TOL = 1e-15         # done when |off-diagonal|_F <= this * |diagonal|_F, looked at before every sweep
TLS_MAX_SWEEPS = 30            # the hard bound; the test molecules take 6 to 11
TLS_PAIRS = ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))                  # 11 22 33 23 13 12: T, L and the observations
TLS_S_ENTRIES = ((0, 0), (1, 1), (0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1))   # S's parameters; S33 = -(S11 + S22)


def tls_cross(r) -> np.ndarray:
    """``A(r)`` [n,3,3] for ``r`` [n,3]: ``A w = w x r``, so a libration ``lambda`` displaces the atom by ``A lambda``."""
    r = np.asarray(r, dtype=np.float64).reshape(-1, 3)
    A = np.zeros((len(r), 3, 3))
    A[:, 0, 1], A[:, 0, 2], A[:, 1, 2] = r[:, 2], -r[:, 1], r[:, 0]
    return A - A.transpose(0, 2, 1)


def tls_model(r, T, L, S) -> np.ndarray:
    """``U(r) = T + A L A^T + A S + S^T A^T`` [n,3,3] in fp64."""
    A = tls_cross(r)
    AS = A @ S
    return T + A @ L @ A.transpose(0, 2, 1) + AS + AS.transpose(0, 2, 1)


def tls_design(r) -> np.ndarray:
    """``J`` [n,6,20] for (scaled) positions ``r`` [n,3]: row o is the observation ``TLS_PAIRS[o]``, weighted sqrt(2) off
    the diagonal; the columns are T, L and S in the module docstring's order."""
    A = tls_cross(r)
    n = len(A)
    w = np.array([1.0, 1.0, 1.0] + [np.sqrt(2.0)] * 3)
    cols = []
    for m, k in TLS_PAIRS:                                                     # T: the observation itself
        E = np.zeros((3, 3))
        E[m, k] = E[k, m] = 1.0
        cols.append(np.broadcast_to(E, (n, 3, 3)))
    for m, k in TLS_PAIRS:                                                     # L: A E A^T
        E = np.zeros((3, 3))
        E[m, k] = E[k, m] = 1.0
        cols.append(A @ E @ A.transpose(0, 2, 1))
    for m, k in TLS_S_ENTRIES:                                                 # S: A E + (A E)^T, traceless
        E = np.zeros((3, 3))
        E[m, k] = 1.0
        if m == k:
            E[2, 2] = -1.0
        AE = A @ E
        cols.append(AE + AE.transpose(0, 2, 1))
    J = np.empty((n, 6, TLS_PARAMS))
    for o, (p, q) in enumerate(TLS_PAIRS):
        for a, Ua in enumerate(cols):
            J[:, o, a] = w[o] * Ua[:, p, q]
    return J


def jacobi_eigh(N, tol: float = TLS_JACOBI_TOL, max_sweeps: int = TLS_MAX_SWEEPS):
    """Eigenvalues and eigenvectors of the symmetric ``N`` [n,n] by cyclic Jacobi in the round-robin ordering, as the
    kernel runs it: ``(w [n] unsorted, V [n,n] with N V = V diag(w), sweeps)``; ``w`` is ``None`` when ``max_sweeps``
    sweeps did not reach ``|off-diagonal|_F <= tol |diagonal|_F``.  An odd n plays with a bye.  All rotations of a round are
    taken from the matrix as the round found it and applied together: ``N' = G^T N G``."""
    A = np.array(N, dtype=np.float64)
    n = A.shape[0]
    V = np.eye(n)
    even = n + (n & 1)
    m = even - 1
    idx = np.arange(n)
    for sweep in range(max_sweeps + 1):
        d = np.diag(A)
        off = A - np.diag(d)
        if (off * off).sum() <= tol * tol * (d * d).sum():
            return d.copy(), V, sweep
        if sweep == max_sweeps:
            break
        for r in range(m):
            partner = np.where(idx == r, m, np.where(idx == m, r, (2 * r - idx) % m))
            partner = np.where(partner >= n, idx, partner)                    # the bye
            p, q = np.minimum(idx, partner), np.maximum(idx, partner)
            app, aqq, apq = A[p, p], A[q, q], A[p, q]
            turn = (p != q) & (apq != 0.0)
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                theta = (aqq - app) / (2.0 * np.where(turn, apq, 1.0))
                t = np.where(theta < 0.0, -1.0, 1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
            c = np.where(turn, 1.0 / np.sqrt(t * t + 1.0), 1.0)
            s = np.where(turn, t * c, 0.0)
            s = np.where(idx == p, -s, s)                                     # column j of N G: c N_j + s_j N_j'
            B = A * c[None, :] + A[:, partner] * s[None, :]
            A = B * c[:, None] + B[partner, :] * s[:, None]
            A[idx[turn], partner[turn]] = 0.0                                 # the entry the rotation annihilates
            V = V * c[None, :] + V[:, partner] * s[None, :]
    return None, V, max_sweeps


def _in_order(a) -> np.ndarray:
    """The sum over dim 0, one addition after the other in index order."""
    return np.cumsum(a, axis=0)[-1]


def tls_solve_host(x, u) -> dict:
    """The TLS fit of ONE molecule whatever its size: ``x`` [n,3] fp64 and ``u`` [n,3,3] in atom order.  A dict with
    ``T``, ``L``, ``S`` [3,3], ``origin`` [3], ``rank``, ``eigenvalues`` [20] (of the normal matrix, ascending, relative
    to the largest), ``sweeps``, ``u_tls`` [n,3,3], ``resid`` [n], ``rfac``, ``T_principal`` / ``L_principal`` [3]
    ascending, ``sym2`` (the sum of ``|Sym U_i|_F^2``) -- fp64 all.  ``rank`` 0: ``rho == 0``; -1: the sweep bound."""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    U = np.asarray(u).astype(np.float64).reshape(-1, 3, 3)
    sym = 0.5 * (U + U.transpose(0, 2, 1))
    n = len(x)
    nan3 = np.full((3, 3), np.nan)
    out = {"T": nan3, "L": nan3, "S": nan3, "origin": np.full(3, np.nan), "rank": 0, "eigenvalues": np.zeros(TLS_PARAMS),
           "sweeps": 0, "u_tls": np.full((n, 3, 3), np.nan), "resid": np.zeros(n), "rfac": 0.0,
           "T_principal": np.full(3, np.nan), "L_principal": np.full(3, np.nan), "sym2": 0.0}
    c = _in_order(x) / n
    r = x - c
    rho = np.sqrt(_in_order((r * r).sum(1)) / n)
    if not rho > 0.0:
        return out
    w = np.array([1.0, 1.0, 1.0] + [np.sqrt(2.0)] * 3)
    J = tls_design(r / rho)
    y = np.stack([w[o] * sym[:, p, q] for o, (p, q) in enumerate(TLS_PAIRS)], axis=1)
    N = _in_order(np.einsum("ioa,iob->iab", J, J))
    b = _in_order(np.einsum("ioa,io->ia", J, y))
    out["sym2"] = float(_in_order((y * y).sum(1)))
    lam, V, out["sweeps"] = jacobi_eigh(N)
    if lam is None:
        out.update(rank=-1, resid=np.full(n, np.nan), rfac=np.nan)
        return out
    top = lam.max()
    keep = lam > TLS_RANK_EPS * top
    out["rank"], out["eigenvalues"] = int(keep.sum()), np.sort(lam) / top
    coef = np.where(keep, (V.T @ b) / np.where(keep, lam, 1.0), 0.0)
    p = V @ coef

    def full(v):
        return np.array([[v[0], v[5], v[4]], [v[5], v[1], v[3]], [v[4], v[3], v[2]]])
    T, L = full(p[0:6]), full(p[6:12]) / (rho * rho)
    S = np.zeros((3, 3))
    for (a, k), v in zip(TLS_S_ENTRIES, p[12:20]):
        S[a, k] = v
    S[2, 2] = -(S[0, 0] + S[1, 1])
    S = S / rho
    fit = tls_model(r, T, L, S)
    d = sym - fit
    resid = np.sqrt((d * d).sum((1, 2)))
    out.update(T=T, L=L, S=S, origin=c, u_tls=fit, resid=resid,
               rfac=float(np.sqrt(_in_order(resid * resid) / out["sym2"])) if out["sym2"] > 0.0 else 0.0)
    for key, mat in (("T_principal", T), ("L_principal", L)):
        vals, _, _ = jacobi_eigh(mat)
        out[key] = np.sort(vals) if vals is not None else np.full(3, np.nan)
    return out


def tls_fit_host(u, label, x, atom_row, status, size, ptr=None) -> dict:
    """The TLS rule of the module docstring in plain numpy, on what ``molecules_host`` (or ``metrics.molecules``) gives:
    ``u`` [M,3,3] fp32; ``label`` [N] and ``x`` [N,3] per atom; ``atom_row`` [N]; ``status`` and ``size`` [M] per row;
    ``ptr`` [B+1] (``None``: one crystal).  A dict with, per row and rounded once to fp32, ``u_tls`` [M,3,3], ``resid`` [M],
    ``params`` [M,24] (T6, L6, S9 row-major, origin3), ``eig`` [M,6] (the principal values of T, then of L) and ``rfac``
    [M]; ``rank`` [M] int32; ``crystal_stats`` [B,6] fp64; and ``molecules``: ``{root atom: tls_solve_host's dict}`` of
    the molecules that were fitted."""
    u = np.asarray(u, dtype=np.float32).reshape(-1, 3, 3)
    label = np.asarray(label, dtype=np.int64).reshape(-1)
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    atom_row = np.asarray(atom_row, dtype=np.int64).reshape(-1)
    status, size = np.asarray(status).reshape(-1), np.asarray(size).reshape(-1)
    N, M = len(label), len(u)
    ptr = np.asarray([0, N] if ptr is None else ptr, dtype=np.int64).reshape(-1)
    B = len(ptr) - 1
    u_tls = np.full((M, 3, 3), np.nan, dtype=np.float32)
    params = np.full((M, 24), np.nan, dtype=np.float32)
    eig = np.full((M, 6), np.nan, dtype=np.float32)
    resid, rfac = np.zeros(M, dtype=np.float32), np.zeros(M, dtype=np.float32)
    rank = np.zeros(M, dtype=np.int32)
    stats = np.zeros((B, 6), dtype=np.float64)
    fitted = {}
    pick = [0, 4, 8, 5, 2, 1]                                                 # 11 22 33 23 13 12 of a row-major 3x3
    for root in np.nonzero(label == np.arange(N))[0]:
        mr = atom_row[root]
        if status[mr] != 0 or size[mr] < TLS_MIN_ATOMS:
            continue
        atoms = np.nonzero(label == root)[0]
        rows = atom_row[atoms]
        fit = tls_solve_host(x[atoms], u[rows])
        if fit["rank"] == 0:
            continue
        fitted[int(root)] = fit
        u_tls[rows], resid[rows] = fit["u_tls"], fit["resid"]
        params[rows] = np.concatenate([fit["T"].reshape(-1)[pick], fit["L"].reshape(-1)[pick], fit["S"].reshape(-1),
                                       fit["origin"]])
        eig[rows] = np.concatenate([fit["T_principal"], fit["L_principal"]])
        rank[rows], rfac[rows] = fit["rank"], fit["rfac"]
        g = int(np.searchsorted(ptr, root, side="right") - 1)
        low = min(fit["T_principal"][0], fit["L_principal"][0])
        stored = resid[rows].astype(np.float64)
        stats[g, :5] += (1, fit["rank"] < TLS_PARAMS, low < 0.0, (stored * stored).sum(), fit["sym2"])
        stats[g, 5] = np.nan if np.isnan(stored).any() or np.isnan(stats[g, 5]) else max(stats[g, 5], stored.max())
    return {"u_tls": u_tls, "resid": resid, "params": params, "eig": eig, "rank": rank, "rfac": rfac,
            "crystal_stats": stats, "molecules": fitted}


ANISO_H_STRETCH = 0.005        # A^2 along X-H: a NOMINAL figure (see the module docstring), not a checked literature value
ANISO_H_BEND = 0.020           # A^2 across X-H, both directions alike: nominal as well
ANISO_H_NONE, ANISO_H_COPY, ANISO_H_PARENT, ANISO_H_TLS, ANISO_H_TLS_DEFICIENT = 0, 1, 2, 3, 4     # ``source``


def tls_libration(r, L, S) -> np.ndarray:
    """``U_LS(r) = A L A^T + A S + S^T A^T`` [3,3] in fp64 for one position ``r`` [3]: ``tls_model`` without ``T``."""
    A = tls_cross(r)[0]
    AS = A @ S
    return A @ L @ A.T + AS + AS.T


def positive_definite(u) -> np.ndarray:
    """Sylvester's criterion for ``u`` [n,3,3]: the three leading minors ``> 0``, in fp64; a NaN is not positive."""
    t = np.asarray(u).astype(np.float64).reshape(-1, 9).T
    m2 = t[0] * t[4] - t[1] * t[3]
    m3 = (t[0] * (t[4] * t[8] - t[5] * t[7]) - t[1] * (t[3] * t[8] - t[5] * t[6])) + t[2] * (t[3] * t[7] - t[4] * t[6])
    with np.errstate(invalid="ignore"):
        return (t[0] > 0.0) & (m2 > 0.0) & (m3 > 0.0)


def aniso_hydrogens_host(u, z, edge_index, cart_dist, cart_dir, atom_row, parent, x=None, params=None, rank=None,
                         stretch: float = ANISO_H_STRETCH, bend: float = ANISO_H_BEND, ptr=None) -> dict:
    """The anisotropic-hydrogen rule of the module docstring in plain numpy: a dict with ``u_h`` [N,3,3] fp32, ``source``
    [N] int32 and ``crystal_stats`` [B,4] fp64 and, for whoever wants the terms apart, ``bond`` [N,3] (``v``) and ``lib``
    [N,3,3] (``D_lib``) in fp64, NaN / 0 where there is none.  ``u`` [M,3,3] fp32; ``z``, ``edge_index``, ``cart_dist``,
    ``cart_dir``, ``atom_row`` as for ``molecules_host``; ``parent`` [N]: ``riding_hydrogens_host``'s; ``x`` [N,3] fp64
    (``molecules_host``), ``params`` [M,24] fp32 and ``rank`` [M] (``tls_fit_host``): all three or none; ``ptr`` [B+1]
    (``None``: one crystal)."""
    u = np.asarray(u, dtype=np.float32).reshape(-1, 3, 3)
    z = np.asarray(z, dtype=np.int64).reshape(-1)
    src, tgt = (np.asarray(a, dtype=np.int64).reshape(-1) for a in np.asarray(edge_index).reshape(2, -1))
    dist = np.asarray(cart_dist, dtype=np.float32).reshape(-1)
    dirs = np.asarray(cart_dir, dtype=np.float32).reshape(-1, 3)
    atom_row = np.asarray(atom_row, dtype=np.int64).reshape(-1)
    parent = np.asarray(parent, dtype=np.int64).reshape(-1)
    N, M = len(z), len(u)
    if (x is None) != (params is None) or (x is None) != (rank is None):
        raise ValueError("x, params and rank come together or not at all")
    if x is not None:
        x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
        params = np.asarray(params, dtype=np.float32).reshape(-1, 24).astype(np.float64)
        rank = np.asarray(rank).reshape(-1)
    ptr = np.asarray([0, N] if ptr is None else ptr, dtype=np.int64).reshape(-1)
    has_row = (atom_row >= 0) & (atom_row < M)
    u_h = np.full((N, 3, 3), np.nan, dtype=np.float32)
    source = np.zeros(N, dtype=np.int32)
    bond = np.full((N, 3), np.nan)
    lib = np.zeros((N, 3, 3))
    heavy = (z != 1) & has_row
    u_h[heavy], source[heavy] = u[atom_row[heavy]], ANISO_H_COPY
    upper = np.triu(np.ones((3, 3), dtype=bool))
    for i in np.nonzero((z == 1) & (parent >= 0) & (parent < N))[0]:
        p = parent[i]
        if not has_row[p]:
            continue
        best, at = np.float32(np.inf), -1
        for e in np.nonzero((tgt == i) & (src == p))[0]:                      # edge order: a tie keeps the lowest edge
            if dist[e] < best:
                best, at = dist[e], e
        if at < 0:
            continue
        v = np.float64(dist[at]) * dirs[at].astype(np.float64)
        n2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
        if not n2 > 0.0:
            continue
        d = v / np.sqrt(n2)
        mp = atom_row[p]
        Up = u[mp].astype(np.float64)
        source[i] = ANISO_H_PARENT
        if x is not None and rank[mp] > 0:
            L = params[mp, 6:12][[0, 5, 4, 5, 1, 3, 4, 3, 2]].reshape(3, 3)
            S = params[mp, 12:21].reshape(3, 3)
            rp = x[p] - params[mp, 21:24]
            lib[i] = tls_libration(rp + v, L, S) - tls_libration(rp, L, S)
            source[i] = ANISO_H_TLS if rank[mp] == TLS_PARAMS else ANISO_H_TLS_DEFICIENT
        dd = np.outer(d, d)
        full = (0.5 * (Up + Up.T) + lib[i]) + (stretch * dd + bend * (np.eye(3) - dd))
        tri = np.where(upper, full, 0.0).astype(np.float32)                  # the upper triangle, rounded once ...
        u_h[i] = tri + np.triu(tri, 1).T                                      # ... and stored on both sides
        bond[i] = v
    stats = np.zeros((len(ptr) - 1, 4), dtype=np.float64)
    stored = u_h.astype(np.float64)
    good = positive_definite(u_h)
    for g in range(len(ptr) - 1):
        a = np.arange(ptr[g], ptr[g + 1])
        a = a[source[a] >= ANISO_H_PARENT]
        tr = ((stored[a, 0, 0] + stored[a, 1, 1]) + stored[a, 2, 2]) / 3.0
        stats[g] = (len(a), (source[a] >= ANISO_H_TLS).sum(), tr.sum(), (~good[a]).sum())
    return {"u_h": u_h, "source": source, "crystal_stats": stats, "bond": bond, "lib": lib}


def _form(w, x, y, z) -> np.ndarray:
    """``v^T Sym(W) v`` for row-major ``w`` [n,9] and the components of ``v``, in the operation order of ``bg_form``
    (csrc/bond_graph.h): the off-diagonal pairs enter as ``(w_ab + w_ba)``."""
    return (w[:, 0] * x * x + w[:, 4] * y * y + w[:, 8] * z * z + (w[:, 1] + w[:, 3]) * x * y
            + (w[:, 2] + w[:, 6]) * x * z + (w[:, 5] + w[:, 7]) * y * z)


def bond_table_host(u, z, edge_index, cart_dist, cart_dir, atom_row, ptr=None, tol: float = BOND_TOLERANCE, params=None,
                    rank=None) -> dict:
    """The bond table of the module docstring in plain numpy, in the kernels' operation order: a dict with ``a``, ``b``
    [nb] int64, ``dir`` [nb,3], ``length``, ``delta``, ``lower``, ``upper``, ``libration`` [nb] fp32, ``tls_rank`` [nb]
    int32, ``counts`` and ``unlisted`` [N] int32 (per atom ``i``: its listed bonds, its bond edges with ``j > i``),
    ``bond_ptr`` [B+1] int64 (the crystals' offsets into the table) and ``crystal_stats`` [B,9] fp64.  ``u`` [M,3,3] fp32;
    ``z``, ``edge_index``, ``cart_dist``, ``cart_dir``, ``atom_row`` as for ``molecules_host``; ``ptr`` [B+1] (``None``:
    one crystal); ``params`` [M,24] fp32 and ``rank`` [M] (``tls_fit_host``): both or neither."""
    u = np.asarray(u, dtype=np.float32).reshape(-1, 9)
    z = np.asarray(z, dtype=np.int64).reshape(-1)
    src, tgt = (np.asarray(a, dtype=np.int64).reshape(-1) for a in np.asarray(edge_index).reshape(2, -1))
    dist = np.asarray(cart_dist, dtype=np.float32).reshape(-1)
    dirs = np.asarray(cart_dir, dtype=np.float32).reshape(-1, 3)
    atom_row = np.asarray(atom_row, dtype=np.int64).reshape(-1)
    N, M = len(z), len(u)
    if (params is None) != (rank is None):
        raise ValueError("params and rank come together or not at all")
    ptr = np.asarray([0, N] if ptr is None else ptr, dtype=np.int64).reshape(-1)
    B = len(ptr) - 1
    inside = (src >= 0) & (src < N) & (tgt >= 0) & (tgt < N)
    s, t = np.where(inside, src, 0), np.where(inside, tgt, 0)
    has_row = (atom_row >= 0) & (atom_row < M)
    bond = inside & has_row[s] & has_row[t] & is_bond(dist, z[t], z[s], tol, same_atom=s == t)
    counts = np.bincount(t[bond & (s < t)], minlength=N).astype(np.int32)
    unlisted = np.bincount(t[bond & (s > t)], minlength=N).astype(np.int32)
    offset = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)])
    e = np.nonzero(bond & (s < t))[0]
    e = e[np.argsort(t[e], kind="stable")]                                    # target order, then edge order
    a, b = s[e], t[e]
    nb = len(e)
    ub, ua = u[atom_row[b]].astype(np.float64), u[atom_row[a]].astype(np.float64)
    x, y, zz = (dirs[e, k].astype(np.float64) for k in range(3))
    l = dist[e].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        delta = _form(ub - ua, x, y, zz)
        wb = np.sqrt(((ub[:, 0] + ub[:, 4]) + ub[:, 8]) - _form(ub, x, y, zz))
        wa = np.sqrt(((ua[:, 0] + ua[:, 4]) + ua[:, 8]) - _form(ua, x, y, zz))
        lo, hi = wb - wa, wb + wa
        lower, upper = l + lo * lo / (2.0 * l), l + hi * hi / (2.0 * l)
    libration = np.full(nb, np.nan)
    tls_rank = np.zeros(nb, dtype=np.int32)
    if params is not None:
        p = np.asarray(params, dtype=np.float32).reshape(-1, 24).astype(np.float64)[atom_row[b]]
        tls_rank = np.asarray(rank).reshape(-1)[atom_row[b]].astype(np.int32)
        l11, l22, l33, l23, l13, l12 = (p[:, 6 + k] for k in range(6))
        rx, ry, rz, tr = l * x, l * y, l * zz, (l11 + l22) + l33
        with np.errstate(invalid="ignore", over="ignore"):
            vx = rx + 0.5 * (tr * rx - ((l11 * rx + l12 * ry) + l13 * rz))
            vy = ry + 0.5 * (tr * ry - ((l12 * rx + l22 * ry) + l23 * rz))
            vz = rz + 0.5 * (tr * rz - ((l13 * rx + l23 * ry) + l33 * rz))
            libration = np.where(tls_rank > 0, np.sqrt((vx * vx + vy * vy) + vz * vz), np.nan)
    out = {"a": a, "b": b, "dir": dirs[e], "length": dist[e], "delta": delta.astype(np.float32),
           "lower": lower.astype(np.float32), "upper": upper.astype(np.float32),
           "libration": libration.astype(np.float32), "tls_rank": tls_rank, "counts": counts, "unlisted": unlisted,
           "bond_ptr": offset[np.clip(ptr, 0, N)]}
    stats = np.zeros((B, 9), dtype=np.float64)
    for g in range(B):
        sl = slice(out["bond_ptr"][g], out["bond_ptr"][g + 1])
        ln, d, lib = (out[k][sl].astype(np.float64) for k in ("length", "delta", "libration"))
        d = np.abs(d)
        fin = np.isfinite(lib)
        grow = (lib - ln)[fin]
        nan_bound = np.isnan(out["lower"][sl]) | np.isnan(out["upper"][sl])
        stats[g] = (len(ln), unlisted[ptr[g]:ptr[g + 1]].sum(), ln.sum(), d.sum(),
                    (np.nan if np.isnan(d).any() else d.max()) if len(d) else 0.0, fin.sum(), grow.sum(),
                    grow.max() if len(grow) else 0.0, nan_bound.sum())
    out["crystal_stats"] = stats
    return out


ANGLE_DEGREES = 57.29577951308232   # 180 / pi as the kernels hold it (csrc/angle_table_ops.hip: AT_DEGREES)


def _cross(p, q) -> np.ndarray:
    return np.stack([p[..., 1] * q[..., 2] - p[..., 2] * q[..., 1], p[..., 2] * q[..., 0] - p[..., 0] * q[..., 2],
                     p[..., 0] * q[..., 1] - p[..., 1] * q[..., 0]], axis=-1)


def _dot(p, q) -> np.ndarray:
    return (p[..., 0] * q[..., 0] + p[..., 1] * q[..., 1]) + p[..., 2] * q[..., 2]


def _librated(v, p) -> np.ndarray:
    """``v + 1/2 (tr(L) v - L v)`` for vectors ``v`` [n,3] and their rows' parameters ``p`` [n,24] (fp64), in the bond
    table's operation order."""
    l11, l22, l33, l23, l13, l12 = (p[:, 6 + k] for k in range(6))
    rx, ry, rz, tr = v[:, 0], v[:, 1], v[:, 2], (l11 + l22) + l33
    return np.stack([rx + 0.5 * (tr * rx - ((l11 * rx + l12 * ry) + l13 * rz)),
                     ry + 0.5 * (tr * ry - ((l12 * rx + l22 * ry) + l23 * rz)),
                     rz + 0.5 * (tr * rz - ((l13 * rx + l23 * ry) + l33 * rz))], axis=1)


def _angle(p, q) -> np.ndarray:
    c = _cross(p, q)
    return (np.arctan2(np.sqrt(_dot(c, c)), _dot(p, q)) * ANGLE_DEGREES).astype(np.float32)


def _torsion(b1, b2, b3):
    """``(value fp32 with -180 stored as +180, defined)`` of the torsions of ``b1``, ``b2``, ``b3`` [n,3] fp64."""
    n1, n2 = _cross(b1, b2), _cross(b2, b3)
    defined = ~((_dot(n1, n1) == 0.0) | (_dot(n2, n2) == 0.0))
    v = (np.arctan2(np.sqrt(_dot(b2, b2)) * _dot(b1, n2), _dot(n1, n2)) * ANGLE_DEGREES).astype(np.float32)
    return np.where(v == np.float32(-180.0), np.float32(180.0), v), defined


def reverse_edge(e0: int, candidates, cart_dist, cart_dir):
    """``(edge or -1, m)``: the reverse of bond edge ``e0`` among ``candidates`` (edges in order) by the module
    docstring's fp32 rule, and the smallest ``m`` seen (``inf`` without a candidate), accepted or not."""
    best, at = np.float32(np.inf), -1
    for e in candidates:
        s = np.abs(cart_dist[e] * cart_dir[e] + cart_dist[e0] * cart_dir[e0])      # fp32: two products, one sum
        m = s[0]
        m = s[1] if s[1] > m else m
        m = s[2] if s[2] > m else m
        if m < best:
            best, at = m, int(e)
    return (at if best < np.float32(MOLECULE_CLOSURE) else -1), best


def angle_table_host(z, edge_index, cart_dist, cart_dir, atom_row, ptr=None, tol: float = BOND_TOLERANCE, params=None,
                     rank=None) -> dict:
    """The angle and torsion tables of the module docstring in plain numpy, in the kernels' operation order: a dict with
    ``degree`` [N] int64, ``nbr_ptr`` [N+1] int64 and ``adj`` (the bond edges, adjacency by adjacency); ``bond_edge``,
    ``reverse`` and ``torsion_counts`` [nb] int64 per listed bond of the bond table (its edge, its reverse edge or -1, its
    torsions) and ``reverse_m`` [nb] fp32 (the smallest closure value a candidate gave, ``inf`` without one);
    ``angle_counts`` [N] int64; ``angle_ptr`` and ``torsion_ptr`` [B+1] int64, the crystals' offsets into the two tables;
    ``angles``: a dict of ``a``, ``b``, ``c`` int64, ``value`` and ``libration`` fp32, ``tls_rank`` int32; ``torsions``:
    the same with ``d``; ``angle_stats`` and ``torsion_stats`` [B,5] fp64.  ``z``, ``edge_index``, ``cart_dist``,
    ``cart_dir``, ``atom_row`` and ``ptr`` as for ``molecules_host`` (an atom has a row where ``atom_row >= 0``);
    ``params`` [M,24] fp32 and ``rank`` [M] (``tls_fit_host``): both or neither."""
    z = np.asarray(z, dtype=np.int64).reshape(-1)
    src, tgt = (np.asarray(a, dtype=np.int64).reshape(-1) for a in np.asarray(edge_index).reshape(2, -1))
    dist = np.asarray(cart_dist, dtype=np.float32).reshape(-1)
    dirs = np.asarray(cart_dir, dtype=np.float32).reshape(-1, 3)
    atom_row = np.asarray(atom_row, dtype=np.int64).reshape(-1)
    N = len(z)
    if (params is None) != (rank is None):
        raise ValueError("params and rank come together or not at all")
    ptr = np.asarray([0, N] if ptr is None else ptr, dtype=np.int64).reshape(-1)
    B = len(ptr) - 1
    inside = (src >= 0) & (src < N) & (tgt >= 0) & (tgt < N)
    s, t = np.where(inside, src, 0), np.where(inside, tgt, 0)
    has_row = atom_row >= 0
    bond = inside & has_row[s] & has_row[t] & is_bond(dist, z[t], z[s], tol, same_atom=s == t)
    adj = np.nonzero(bond)[0]
    adj = adj[np.argsort(t[adj], kind="stable")]                              # target order, then edge order
    degree = np.bincount(t[adj], minlength=N).astype(np.int64)
    nbr_ptr = np.concatenate([[0], np.cumsum(degree)])
    bond_edge = adj[s[adj] < t[adj]]                                          # the bond table's rows
    nb = len(bond_edge)
    fit = params is not None
    if fit:
        par = np.asarray(params, dtype=np.float32).reshape(-1, 24).astype(np.float64)
        rk = np.asarray(rank).reshape(-1).astype(np.int32)
    d64, v64 = dirs.astype(np.float64), dist.astype(np.float64)[:, None] * dirs.astype(np.float64)

    def finish(cols, vectors, row_atom, formula):
        """The columns every table shares: ``tls_rank`` and ``libration`` of the entries whose edges are ``vectors`` (a
        list of (edge array, sign)) and whose fit is read at ``row_atom``."""
        n = len(row_atom)
        cols["tls_rank"] = rk[atom_row[row_atom]] if fit else np.zeros(n, dtype=np.int32)
        cols["libration"] = np.full(n, np.nan, dtype=np.float32)
        on = cols["tls_rank"] > 0
        if fit and on.any():
            p = par[atom_row[row_atom[on]]]
            with np.errstate(invalid="ignore", over="ignore"):
                cols["libration"][on] = formula(*[sign * _librated(v64[e[on]], p) for e, sign in vectors], on)
        return cols

    # ---- angles: per centre the pairs k1 < k2 of its adjacency, k1 first
    pairs = [(nbr_ptr[i] + k1, nbr_ptr[i] + k2) for i in range(N) for k1 in range(degree[i])
             for k2 in range(k1 + 1, degree[i])]
    k1, k2 = (np.asarray([p[c] for p in pairs], dtype=np.int64) for c in range(2))
    e1, e2 = adj[k1], adj[k2]
    angles = {"a": s[e1], "b": t[e1], "c": s[e2], "value": _angle(d64[e1], d64[e2])}
    finish(angles, [(e1, 1.0), (e2, 1.0)], t[e1], lambda p, q, on: _angle(p, q))
    angle_counts = degree * (degree - 1) // 2
    angle_off = np.concatenate([[0], np.cumsum(angle_counts)])

    # ---- torsions: per listed bond e0 = (b -> c) the edges into b without the reverse of e0, times those into c without e0
    reverse, reverse_m = np.full(nb, -1, dtype=np.int64), np.full(nb, np.inf, dtype=np.float32)
    counts = np.zeros(nb, dtype=np.int64)
    ea, e0s, ed = [], [], []
    for k, e0 in enumerate(bond_edge):
        b, c = s[e0], t[e0]
        into_b, into_c = adj[nbr_ptr[b]:nbr_ptr[b + 1]], adj[nbr_ptr[c]:nbr_ptr[c + 1]]
        reverse[k], reverse_m[k] = reverse_edge(e0, into_b[s[into_b] == c], dist, dirs)
        side_a, side_d = into_b[into_b != reverse[k]], into_c[into_c != e0]
        counts[k] = len(side_a) * len(side_d)
        for x in side_a:
            for y in side_d:
                ea.append(x), e0s.append(e0), ed.append(y)
    ea, e0s, ed = (np.asarray(x, dtype=np.int64) for x in (ea, e0s, ed))
    value, defined = _torsion(d64[ea], d64[e0s], -d64[ed])
    torsions = {"a": s[ea], "b": s[e0s], "c": t[e0s], "d": s[ed],
                "value": np.where(defined, value, np.float32(np.nan)).astype(np.float32)}
    finish(torsions, [(ea, 1.0), (e0s, 1.0), (ed, -1.0)], t[e0s],
           lambda b1, b2, b3, on: np.where(defined[on], _torsion(b1, b2, b3)[0], np.float32(np.nan)))
    torsion_off = np.concatenate([[0], np.cumsum(counts)])
    listed_off = np.concatenate([[0], np.cumsum(np.bincount(t[bond_edge], minlength=N))])

    at = np.clip(ptr, 0, N)
    out = {"degree": degree, "nbr_ptr": nbr_ptr, "adj": adj, "bond_edge": bond_edge, "reverse": reverse,
           "reverse_m": reverse_m, "torsion_counts": counts, "angle_counts": angle_counts, "angle_ptr": angle_off[at],
           "torsion_ptr": torsion_off[listed_off[at]], "angles": angles, "torsions": torsions}
    a_stats, t_stats = np.zeros((B, 5), dtype=np.float64), np.zeros((B, 5), dtype=np.float64)
    for g in range(B):
        for stats, table, cut, circular in ((a_stats, angles, out["angle_ptr"], False),
                                            (t_stats, torsions, out["torsion_ptr"], True)):
            v, lib = (table[k][cut[g]:cut[g + 1]].astype(np.float64) for k in ("value", "libration"))
            fin = np.isfinite(lib)
            x = np.abs(lib - v)[fin]
            if circular:
                x = np.minimum(x, 360.0 - x)
            stats[g] = (len(v), np.isnan(v).sum() if circular else v.sum(), fin.sum(), x.sum(), x.max() if len(x) else 0.0)
    out["angle_stats"], out["torsion_stats"] = a_stats, t_stats
    return out
