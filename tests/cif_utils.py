"""Hand-written CIF texts and fp64 numpy restatements shared by the CIF / symmetry tests.

The space groups are generated from generators by closure modulo lattice translations, not typed out.  The crystals are
the smallest shapes at which the expansion can go wrong:

  a  P1 triclinic, 5 atoms, one hydrogen, an esd on every number, no operator loop (P1 by name)
  b  P2_1/c, 4 operators, 6 atoms with a hydrogen, a negative coordinate and one atom on an inversion centre (orbit of 2)
  c  R-3 on hexagonal axes, 18 operators with x-y terms and translations of 1/3 and 2/3, one atom on the 3-fold axis
  d  Fm-3m NaCl, 192 operators, 2 atoms: 384 candidates cross a tile of 256 and leave 8 atoms
  e  one atom, one operator
"""
from fractions import Fraction

import numpy as np

CIF_ORDER = ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))          # U11 U22 U33 U23 U13 U12


# ------------------------------------------------------------------------------------------------ space groups
def _op(rows, trans=(0, 0, 0)):
    return (tuple(tuple(int(v) for v in r) for r in rows), tuple(Fraction(t) % 1 for t in trans))


def _mul(p, q):
    (W1, w1), (W2, w2) = p, q
    W = tuple(tuple(sum(W1[i][k] * W2[k][j] for k in range(3)) for j in range(3)) for i in range(3))
    w = tuple((sum(W1[i][k] * w2[k] for k in range(3)) + w1[i]) % 1 for i in range(3))
    return W, w


IDENTITY = _op(((1, 0, 0), (0, 1, 0), (0, 0, 1)))
INVERSION = _op(((-1, 0, 0), (0, -1, 0), (0, 0, -1)))


def close_group(generators):
    """Every product of the generators modulo lattice translations; the identity first, then in order of discovery."""
    ops = [IDENTITY]
    k = 0
    while k < len(ops):
        for g in generators:
            new = _mul(g, ops[k])
            if new not in ops:
                ops.append(new)
        k += 1
    return ops


def op_string(op) -> str:
    W, w = op
    out = []
    for r in range(3):
        s = ""
        for c in range(3):
            if W[r][c]:
                s += ("-" if W[r][c] < 0 else "+" if s else "") + "xyz"[c]
        if w[r]:
            s += f"+{w[r].numerator}/{w[r].denominator}"
        out.append(s)
    return ", ".join(out)


def op_arrays(ops):
    """(W [m,3,3] int64, w [m,3] float64)."""
    return (np.array([o[0] for o in ops], dtype=np.int64), np.array([[float(t) for t in o[1]] for o in ops]))


H = Fraction(1, 2)
P21C = close_group([_op(((-1, 0, 0), (0, 1, 0), (0, 0, -1)), (0, H, H)), INVERSION])
R3BAR = close_group([_op(((0, -1, 0), (1, -1, 0), (0, 0, 1))), INVERSION,
                     _op(IDENTITY[0], (Fraction(2, 3), Fraction(1, 3), Fraction(1, 3)))])
FM3M = close_group([_op(((0, -1, 0), (1, 0, 0), (0, 0, 1))), _op(((0, 0, 1), (1, 0, 0), (0, 1, 0))), INVERSION,
                    _op(IDENTITY[0], (0, H, H)), _op(IDENTITY[0], (H, 0, H))])
assert (len(P21C), len(R3BAR), len(FM3M)) == (4, 18, 192)


# ------------------------------------------------------------------------------------------------ the crystals
# name -> cell (a b c alpha beta gamma), operators (None: P1 by name), temperature, atoms (label, symbol, x, y, z, U6 or None)
CRYSTALS = {
    "a": dict(cell=(7.123, 8.456, 9.789, 81.23, 77.45, 68.91), ops=None, temp=150.0, atoms=[
        ("C1", "C", 0.1234, 0.2345, 0.3456, (0.0312, 0.0287, 0.0351, 0.0021, -0.0043, 0.0065)),
        ("N1", "N", 0.6543, 0.1287, 0.8712, (0.0254, 0.0331, 0.0298, -0.0034, 0.0027, 0.0012)),
        ("O1", "O", 0.3821, 0.7754, 0.5123, (0.0412, 0.0365, 0.0301, 0.0056, 0.0033, -0.0071)),
        ("S1", "S", 0.9012, 0.4433, 0.1357, (0.0223, 0.0251, 0.0267, 0.0011, -0.0025, 0.0038)),
        ("H1", "H", 0.2468, 0.5791, 0.7139, None)]),
    "b": dict(cell=(5.812, 11.237, 7.446, 90.0, 104.31, 90.0), ops=P21C, temp=100.0, atoms=[
        ("Fe1", "Fe", 0.5, 0.0, 0.5, (0.0187, 0.0212, 0.0165, 0.0014, 0.0031, -0.0009)),
        ("C1", "C", 0.2137, 0.1342, 0.4071, (0.0291, 0.0263, 0.0318, -0.0027, 0.0052, 0.0019)),
        ("C2", "C", -0.0312, 0.2718, 0.1564, (0.0334, 0.0279, 0.0246, 0.0041, -0.0018, 0.0063)),
        ("N1", "N", 0.3679, 0.4216, 0.0893, (0.0268, 0.0352, 0.0297, 0.0008, 0.0044, -0.0036)),
        ("O1", "O", 0.7421, 0.3187, 0.2865, (0.0401, 0.0317, 0.0372, -0.0062, 0.0029, 0.0047)),
        ("H1", "H", 0.1185, 0.0673, 0.3342, None)]),
    "c": dict(cell=(10.512, 10.512, 14.237, 90.0, 90.0, 120.0), ops=R3BAR, temp=293.0, atoms=[
        # on the 3-fold axis: U11 = U22 = 2 U12, U13 = U23 = 0
        ("Si1", "Si", 0.0, 0.0, 0.2134, (0.0242, 0.0242, 0.0318, 0.0, 0.0, 0.0121)),
        ("O1", "O", 0.1812, 0.0433, 0.1127, (0.0356, 0.0288, 0.0314, 0.0037, -0.0049, 0.0152)),
        ("C1", "C", 0.2671, 0.1893, 0.0418, (0.0279, 0.0341, 0.0263, -0.0022, 0.0035, 0.0118)),
        ("H1", "H", 0.3127, 0.2541, 0.0876, None)]),
    "d": dict(cell=(5.6402, 5.6402, 5.6402, 90.0, 90.0, 90.0), ops=FM3M, temp=295.0, atoms=[
        ("Na1", "Na", 0.0, 0.0, 0.0, (0.0173, 0.0173, 0.0173, 0.0, 0.0, 0.0)),
        ("Cl1", "Cl", 0.5, 0.5, 0.5, (0.0151, 0.0151, 0.0151, 0.0, 0.0, 0.0))]),
    "e": dict(cell=(4.05, 4.05, 4.05, 90.0, 90.0, 90.0), ops=[IDENTITY], temp=20.0, atoms=[
        ("Al1", "Al", 0.25, 0.25, 0.25, (0.0061, 0.0072, 0.0058, 0.0004, -0.0003, 0.0005))]),
}
# atoms in the cell, of which not hydrogen; (c) from the multiplicities: 6 on the axis, 18 general
ATOMS = {"a": (5, 4), "b": (22, 18), "c": (6 + 3 * 18, 6 + 2 * 18), "d": (8, 8), "e": (1, 1)}
# (crystal, atom, the operators of its stabiliser are those that map it onto itself)
SPECIAL = (("b", 0), ("c", 0))
BATCH = ("e", "b", "d", "c", "a", "d", "b", "e", "d")           # (d) again: a crystal that starts in the middle of a tile


def cif_text(key: str, name: str = None, esd: bool = None, labeled: bool = True) -> str:
    """The CIF of crystal ``key``; ``esd``: an esd on every number (default: only for (a))."""
    c = CRYSTALS[key]
    esd = (key == "a") if esd is None else esd

    def num(v, digits=4):
        return f"{v:.{digits}f}" + ("(3)" if esd else "")
    lines = ["# written by hand for the tests", f"data_{name or 'crystal_' + key}",
             "_publ_section_title", ";", f" Test crystal ({key}); a text field", " with two lines", ";"]
    for tag, v in zip(("length_a", "length_b", "length_c", "angle_alpha", "angle_beta", "angle_gamma"), c["cell"]):
        lines.append(f"_cell_{tag} {num(v)}")
    lines.append(f"_diffrn_ambient_temperature {c['temp']:.0f}" + ("(2)" if esd else ""))
    lines.append("_diffrn_ambient_pressure ?")
    if c["ops"] is None:
        lines.append("_symmetry_space_group_name_H-M 'P 1'")
    else:
        lines += ["_symmetry_space_group_name_H-M 'from the operators'", "loop_", "_space_group_symop_id",
                  "_space_group_symop_operation_xyz"]
        lines += [f"{k + 1} '{op_string(o)}'" for k, o in enumerate(c["ops"])]
    lines += ["loop_", "_atom_site_label", "_atom_site_type_symbol", "_atom_site_fract_x", "_atom_site_fract_y",
              "_atom_site_fract_z", "_atom_site_U_iso_or_equiv", "_atom_site_adp_type", "_atom_site_occupancy",
              "_atom_site_disorder_group"]
    for lab, sym, x, y, z, u in c["atoms"]:
        ueq = 0.05 if u is None else sum(u[:3]) / 3
        lines.append(f"{lab} {sym} {num(x)} {num(y)} {num(z)} {num(ueq)} {'Uiso' if u is None else 'Uani'} 1 .")
    if labeled:
        lines += ["loop_", "_atom_site_aniso_label"] + [f"_atom_site_aniso_U_{k}" for k in ("11", "22", "33", "23", "13", "12")]
        for lab, _, _, _, _, u in c["atoms"]:
            if u is not None:
                lines.append(lab + " " + " ".join(num(v) for v in u))
    return "\n".join(lines) + "\n"


def batch_text() -> str:
    """One file with the data blocks of BATCH, named ``<key><position>``."""
    return "".join(cif_text(k, f"{k}{i}") for i, k in enumerate(BATCH))


_HEAD = """data_{name}
_cell_length_a 6.1
_cell_length_b 7.2
_cell_length_c 8.3
_cell_angle_alpha 90
_cell_angle_beta 90
_cell_angle_gamma 90
_diffrn_ambient_temperature 120
"""
_P1 = "_symmetry_Int_Tables_number 1\n"
_SITES = "loop_\n_atom_site_label\n_atom_site_fract_x\n_atom_site_fract_y\n_atom_site_fract_z\n"
_ANISO = ("loop_\n_atom_site_aniso_label\n_atom_site_aniso_U_11\n_atom_site_aniso_U_22\n_atom_site_aniso_U_33\n"
          "_atom_site_aniso_U_23\n_atom_site_aniso_U_13\n_atom_site_aniso_U_12\n")
BAD = {
    "disordered": _HEAD.format(name="disordered") + _P1 + "loop_\n_atom_site_label\n_atom_site_fract_x\n_atom_site_fract_y\n"
    "_atom_site_fract_z\n_atom_site_occupancy\n_atom_site_disorder_group\nC1 0.1 0.2 0.3 1 .\nC2 0.4 0.5 0.6 0.5 1\n"
    + _ANISO + "C1 0.02 0.02 0.02 0 0 0\nC2 0.02 0.02 0.02 0 0 0\n",
    "isotropic_carbon": _HEAD.format(name="isotropic_carbon") + _P1 + _SITES + "C1 0.1 0.2 0.3\nC2 0.4 0.5 0.6\nH1 0.7 0.8 0.9\n"
    + _ANISO + "C1 0.02 0.02 0.02 0 0 0\n",
    "no_operators": _HEAD.format(name="no_operators") + "_symmetry_space_group_name_H-M 'P 21/c'\n" + _SITES
    + "C1 0.1 0.2 0.3\n" + _ANISO + "C1 0.02 0.02 0.02 0 0 0\n",
    # C1 and C3 are 1.5e-4 apart with C2 between them: C2 repeats C1 and C3 repeats C2, but C3 does not repeat C1
    "ambiguous": _HEAD.format(name="ambiguous") + _P1 + _SITES + "C1 0.3 0.2 0.1\nC2 0.300075 0.2 0.1\nC3 0.30015 0.2 0.1\n"
    + _ANISO + "C1 0.02 0.02 0.02 0 0 0\nC2 0.02 0.02 0.02 0 0 0\nC3 0.02 0.02 0.02 0 0 0\n",
    "pressure": _HEAD.format(name="pressure") + "_diffrn_ambient_pressure 250000\n" + _P1 + _SITES + "C1 0.1 0.2 0.3\n"
    + _ANISO + "C1 0.02 0.02 0.02 0 0 0\n",
    "aniso_in_b": _HEAD.format(name="aniso_in_b") + _P1 + _SITES + "C1 0.1 0.2 0.3\n"
    + _ANISO.replace("_U_", "_B_") + "C1 1.5 1.5 1.5 0 0 0\n",
    "no_temperature": _HEAD.format(name="no_temperature").replace("_diffrn_ambient_temperature 120\n", "") + _P1 + _SITES
    + "C1 0.1 0.2 0.3\n" + _ANISO + "C1 0.02 0.02 0.02 0 0 0\n",
    "singular": _HEAD.format(name="singular").replace("_cell_length_a 6.1", "_cell_length_a 0") + _P1 + _SITES
    + "C1 0.1 0.2 0.3\n" + _ANISO + "C1 0.02 0.02 0.02 0 0 0\n",
}


# ------------------------------------------------------------------------------------------------ fp64 numpy
def cell_reference(a, b, c, alpha, beta, gamma) -> np.ndarray:
    """The cell of the reference's convention (dataset/extract_csd_data.py:15-25) in fp64: rows = lattice vectors."""
    al, be, ga = np.radians([alpha, beta, gamma])
    v = np.sqrt(1 - np.cos(al) ** 2 - np.cos(be) ** 2 - np.cos(ga) ** 2 + 2 * np.cos(al) * np.cos(be) * np.cos(ga))
    cols = np.array([[a, b * np.cos(ga), c * np.cos(be)],
                     [0, b * np.sin(ga), c * (np.cos(al) - np.cos(be) * np.cos(ga)) / np.sin(ga)],
                     [0, 0, c * v / np.sin(ga)]])
    return cols.T


def full(u6: np.ndarray) -> np.ndarray:
    """[...,6] (U11 U22 U33 U23 U13 U12) -> symmetric [...,3,3]."""
    u6 = np.asarray(u6, dtype=np.float64)
    out = np.zeros(u6.shape[:-1] + (3, 3))
    for k, (i, j) in enumerate(CIF_ORDER):
        out[..., i, j] = out[..., j, i] = u6[..., k]
    return out


def six(u: np.ndarray) -> np.ndarray:
    return np.stack([np.asarray(u)[..., i, j] for i, j in CIF_ORDER], axis=-1)


def reciprocal_norms(cell: np.ndarray) -> np.ndarray:
    return np.linalg.norm(np.linalg.inv(np.asarray(cell, dtype=np.float64).T), axis=-1)


def cart_from_cif(u_cif: np.ndarray, cell: np.ndarray, W: np.ndarray = None) -> np.ndarray:
    """dataset/extract_csd_data.py:115-123 in fp64 for the image of an atom under the operator with rotation ``W``
    (None: the identity): with M = cell and N = diag(row norms of inv(M^T)), y = M^T (W (N U N) W^T) M."""
    M = np.asarray(cell, dtype=np.float64)
    n = reciprocal_norms(M)
    beta = n[:, None] * np.asarray(u_cif, dtype=np.float64) * n[None, :]
    if W is not None:
        W = np.asarray(W, dtype=np.float64)
        beta = W @ beta @ np.swapaxes(W, -1, -2)
    return M.T @ beta @ M


def cif_from_cart(y: np.ndarray, cell: np.ndarray) -> np.ndarray:
    """The inverse of ``cart_from_cif`` for the identity: U_cif = N^-1 M^-T y M^-1 N^-1, fp64."""
    M = np.asarray(cell, dtype=np.float64)
    Mi = np.linalg.inv(M)
    n = reciprocal_norms(M)
    return (Mi.T @ np.asarray(y, dtype=np.float64) @ Mi) / (n[:, None] * n[None, :])


def map6(cell: np.ndarray) -> np.ndarray:
    """T [6,6]: the 6 components of y (in CIF_ORDER) = T u6, for the identity operator."""
    T = np.zeros((6, 6))
    for k in range(6):
        e = np.zeros(6)
        e[k] = 1.0
        T[:, k] = six(cart_from_cif(full(e), cell))
    return T


def round_trip_bound(u6: np.ndarray, cell: np.ndarray) -> np.ndarray:
    """2^-23 (|T^-1| |T| |u|) componentwise, [...,6].  One fp32 rounding of every component of y = T u moves the u
    recovered from it by at most 2^-24 |T^-1| |T u| <= 2^-24 |T^-1| |T| |u|; the factor two covers the fp32 rounding of
    the result itself."""
    T = map6(cell)
    amp = np.abs(np.linalg.inv(T)) @ np.abs(T)
    return 2.0 ** -23 * np.abs(np.asarray(u6, dtype=np.float64)) @ amp.T


def fp64_floor(u6: np.ndarray, spread) -> np.ndarray:
    """[...,1]: what fp64 round-off can leave in a component of a site average whose members cancel.  A member is some
    hundred fp64 operations on values of its own size (at most |mean| + spread in the units of u), each with relative error
    2^-53, and the mean adds up to 192 of them: 2^-53 * 2^9 = 2^-44 of that size, 2^21 times below the fp32 bound."""
    size = np.abs(np.asarray(u6, dtype=np.float64)).max(axis=-1, keepdims=True) + np.asarray(spread, dtype=np.float64)[..., None]
    return 2.0 ** -44 * size


def crystal_from_coords(name: str, coord: np.ndarray):
    """A P1 crystal (one operator, the identity) in a cubic cell whose atoms sit at ``coord`` [n,3]; atom i has Z = i + 2,
    so the atoms that an expansion keeps can be read off its ``z``."""
    from cartnet_amd.cif import CifCrystal
    n = int(coord.shape[0])
    return CifCrystal(name=name, cell_parameters=(10.0, 10.0, 10.0, 90.0, 90.0, 90.0), temperature=100.0,
                      symops=[(np.eye(3, dtype=np.int64), np.zeros(3))], symop_strings=["x,y,z"],
                      labels=[f"X{i}" for i in range(n)], symbols=["X"] * n, z=[i + 2 for i in range(n)],
                      frac=[tuple(float(v) for v in row) for row in coord], occupancy=[1.0] * n, disorder_group=["."] * n,
                      u_iso=[None] * n, adp_type=[None] * n)


def kept_mask(z: np.ndarray, n: int) -> np.ndarray:
    """The atoms of a ``crystal_from_coords`` crystal that an expansion kept, from the ``z`` it returned."""
    mask = np.zeros(n, dtype=bool)
    mask[np.asarray(z, dtype=np.int64) - 2] = True
    return mask


def site_average_reference(pred: np.ndarray, orbit_rows: np.ndarray, W: np.ndarray, cell: np.ndarray):
    """fp64: (u6 [6], spread) of one site from ``pred`` [rows,3,3] of its crystal, ``orbit_rows`` [m], ``W`` [m,3,3]."""
    M = np.asarray(cell, dtype=np.float64)
    Mi = np.linalg.inv(M)
    n = reciprocal_norms(M)
    members = []
    for row, w in zip(orbit_rows, np.asarray(W, dtype=np.float64)):
        U = np.asarray(pred[row], dtype=np.float64)
        U = 0.5 * (U + U.T)
        L = np.rint(np.linalg.inv(w))
        members.append(L @ (Mi.T @ U @ Mi) @ L.T)
    members = np.array(members) / (n[:, None] * n[None, :])
    mean = members.mean(axis=0)
    return six(mean), float(np.abs(members - mean).max())
