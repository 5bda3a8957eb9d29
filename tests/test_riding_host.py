"""Riding hydrogens on the host: the flags and the refusal, the entry point's declaration, binding and returns that need no
launch, the rule in numpy (``bonds.riding_hydrogens_host``) on hand-built edge lists, the two CIF writers with and without
the new key, and U_eq of a tensor on the unit reciprocal axes (no GPU)."""
import os
import re

import numpy as np
import pytest
import torch

import predict_utils as pu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_parser_defaults_and_constants():
    import main as entry
    from cartnet_amd.bonds import RIDING_FACTOR, RIDING_FACTOR_ROTATING
    from cartnet_amd.predict import BOND_KEYS, H_KEYS, H_SYM_KEYS, KEYS, ROT_KEYS, SYM_KEYS
    assert (RIDING_FACTOR, RIDING_FACTOR_ROTATING) == (1.2, 1.5)
    p = entry.build_parser()
    d = p.parse_args([])
    assert (d.riding_h, d.riding_h_factor, d.riding_h_factor_rotating, d.bond_tolerance) == (False, 1.2, 1.5, 0.4)
    a = p.parse_args(["--riding_h", "--riding_h_factor", "1.3", "--riding_h_factor_rotating", "1.6"])
    assert (a.riding_h, a.riding_h_factor, a.riding_h_factor_rotating) == (True, 1.3, 1.6)
    assert H_KEYS == ("u_iso", "h_parent", "h_count", "h_mult", "h_stats") and H_SYM_KEYS == ("u_iso_asym", "h_parent_asym")
    assert not set(H_KEYS + H_SYM_KEYS) & set(KEYS + SYM_KEYS + ROT_KEYS + BOND_KEYS)


def test_riding_h_with_disable_h_is_refused_before_the_device_is_touched(monkeypatch):
    import main as entry

    def touched(*a, **k):
        raise AssertionError("--riding_h --disable_H went on past its argument check")
    monkeypatch.setattr(entry.cdist, "init_from_env", touched)
    monkeypatch.setattr(entry, "create_model", touched)
    with pytest.raises(SystemExit, match="--riding_h with --disable_H"):
        entry.main(["--predict", "--riding_h", "--disable_H", "--predict_input", "x.cnshard", "--checkpoint_path", "x.ckpt"])
    from cartnet_amd.config import set_cfg
    set_cfg()


def test_entry_point_is_declared_bound_and_built():
    from cartnet_amd import lib
    from cartnet_amd.build import SOURCES
    hdr = open(os.path.join(ROOT, "include", "cartnet_hip.h")).read()
    assert "Riding hydrogens" in hdr and "dataset/datasetADP.py:49" in hdr and "no counterpart" in hdr
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+cartnet_adp_riding_h\s*\(([^)]*)\)\s*;", hdr)
    assert m and len(m.group(1).split(",")) == 22 == len(lib.PROTOTYPES["cartnet_adp_riding_h"][1])
    assert "struct" not in m.group(1)                                         # plain arguments
    assert "riding_ops.hip" in SOURCES
    assert lib.ABI_VERSION == 16 == lib.load().cartnet_abi_version()          # no struct changed


def test_no_launch_and_refusal_returns():
    from cartnet_amd import lib
    l = lib.load()
    f = l.cartnet_adp_riding_h
    nul, out = [None] * 8, [None] * 6
    par = (97, 0.4, 1.2, 1.5)
    assert f(*nul, *par, 0, 10, 5, 50, *out) == 0                             # no crystals
    assert f(*nul, *par, 4, 0, 5, 50, *out) == 0                              # no atoms
    for bad in ((-1, 10, 5, 50), (4, -1, 5, 50), (4, 10, -1, 50), (4, 10, 5, -1)):
        assert f(*nul, *par, *bad, *out) != 0
        assert b"bad sizes" in l.cartnet_last_error()
    assert f(*nul, -1, 0.4, 1.2, 1.5, 4, 10, 5, 50, *out) != 0
    assert b"bad sizes" in l.cartnet_last_error()
    for k in range(3):
        p = [0.4, 1.2, 1.5]
        p[k] = float("nan")
        assert f(*nul, 97, *p, 4, 10, 5, 50, *out) != 0
        assert b"must be numbers" in l.cartnet_last_error()
    for sizes in ((4, 10, 5, 50), (4, 10, 0, 0)):                             # before any launch, also without rows and edges
        assert f(*nul, *par, *sizes, *out) != 0
        assert b"null pointer" in l.cartnet_last_error()


def test_is_h_bond_is_the_bond_rule_with_a_hydrogen_end():
    from cartnet_amd.bonds import COVALENT_RADII, is_h_bond
    r = np.asarray(COVALENT_RADII, dtype=np.float32)
    limit = (r[1] + r[6]) + np.float32(0.4)
    assert limit.dtype == np.float32 and abs(float(limit) - 1.47) < 1e-6
    assert bool(is_h_bond(limit, 6)) and not bool(is_h_bond(np.nextafter(limit, np.float32(9)), 6))
    got = is_h_bond(np.float32([1.09, 1.09, 1.09, 1.09, 1.6, np.nan]), [6, 1, 0, 97, 6, 6], 0.4)
    assert got.tolist() == [True, False, False, False, False, False]
    assert bool(is_h_bond(1.6, 6, 0.6))                                       # the tolerance is the caller's


# ---------------------------------------------------------------------------------------------------- the rule by hand
def _graph(z, bonds, extra=()):
    """(z, edge_index sorted by target, cart_dist, atom_row) of a molecule: ``bonds`` = (i, j, dist) held in both
    directions, ``extra`` = directed (source, target, dist)."""
    edges = [(i, j, d) for i, j, d in bonds] + [(j, i, d) for i, j, d in bonds] + list(extra)
    edges.sort(key=lambda e: e[1])
    z = np.asarray(z, dtype=np.int64)
    ei = np.array([[e[0] for e in edges], [e[1] for e in edges]], dtype=np.int64).reshape(2, -1)
    row = np.where(z != 1, np.cumsum(z != 1) - 1, -1)
    return z, ei, np.array([e[2] for e in edges], dtype=np.float32), row


def _u_eq(z, seed=0):
    return (0.02 + 0.03 * np.random.default_rng(seed).random(int((np.asarray(z) != 1).sum()))).astype(np.float32)


def _value(mult, u):
    return np.float32(np.float64(np.float32(mult)) * np.float64(u))


def test_methanol_by_hand():
    """C0 O1, H2 H3 H4 on the carbon, H5 on the oxygen; the carbon's hydrogens also see the oxygen at 2.0 A (no bond)."""
    from cartnet_amd.bonds import riding_hydrogens_host
    z, ei, dist, row = _graph([6, 8, 1, 1, 1, 1], [(0, 2, 1.09), (0, 3, 1.09), (0, 4, 1.09), (1, 5, 0.96), (0, 1, 1.43)],
                              [(1, 2, 2.0), (1, 3, 2.0), (0, 5, 1.95)])
    u = _u_eq(z)
    parent, count, mult, u_iso = riding_hydrogens_host(z, ei, dist, row, u, 0.4, 1.2, 1.5)
    assert parent.dtype == np.int64 and count.dtype == np.int32 and mult.dtype == u_iso.dtype == np.float32
    assert parent.tolist() == [-1, -1, 0, 0, 0, 1] and count.tolist() == [3, 1, 0, 0, 0, 0]
    assert mult.tolist() == [0.0, 0.0, 1.5, 1.5, 1.5, 1.5]                    # methyl and hydroxyl
    want = [u[0], u[1]] + [_value(1.5, u[0])] * 3 + [_value(1.5, u[1])]
    assert u_iso.tobytes() == np.array(want, dtype=np.float32).tobytes()


def test_aromatic_ch_nh3_ch2_and_an_orphan_by_hand():
    """C0-H1 (aromatic: one hydrogen), N2 with H3 H4 H5 (three on nitrogen: still 1.2), C6 with H7 H8 (CH2), H9 with no
    neighbour inside the limit, H10 whose only neighbour is another hydrogen."""
    from cartnet_amd.bonds import riding_hydrogens_host
    z, ei, dist, row = _graph([6, 1, 7, 1, 1, 1, 6, 1, 1, 1, 1],
                              [(0, 1, 0.95), (2, 3, 1.01), (2, 4, 1.01), (2, 5, 1.01), (6, 7, 0.99), (6, 8, 0.99), (0, 6, 1.5),
                               (0, 9, 2.6), (9, 10, 0.74)])
    u = _u_eq(z, 1)
    parent, count, mult, u_iso = riding_hydrogens_host(z, ei, dist, row, u)
    assert parent.tolist() == [-1, 0, -1, 2, 2, 2, -1, 6, 6, -1, -1]
    assert count.tolist() == [1, 0, 3, 0, 0, 0, 2, 0, 0, 0, 0]
    assert mult.tolist() == [0.0] + [np.float32(1.2)] * 1 + [0.0] + [np.float32(1.2)] * 3 + [0.0] + [np.float32(1.2)] * 2 + [0.0, 0.0]
    assert np.isnan(u_iso[9]) and np.isnan(u_iso[10]) and mult[9] == 0.0 and parent[9] == -1          # orphans
    assert u_iso[1] == _value(1.2, u[0]) and u_iso[3] == u_iso[4] == u_iso[5] == _value(1.2, u[1])
    assert u_iso[7] == u_iso[8] == _value(1.2, u[2]) and u_iso[[0, 2, 6]].tolist() == u.tolist()
    # other factors are the caller's; water: two hydrogens on oxygen take the rotating factor
    z, ei, dist, row = _graph([8, 1, 1], [(0, 1, 0.96), (0, 2, 0.96)])
    parent, count, mult, u_iso = riding_hydrogens_host(z, ei, dist, row, np.float32([-0.01]), 0.4, 1.3, 1.7)
    assert parent.tolist() == [-1, 0, 0] and count.tolist() == [2, 0, 0] and mult.tolist() == [0.0] + [np.float32(1.7)] * 2
    assert u_iso[1] == _value(1.7, np.float32(-0.01)) < 0                      # a negative parent is passed through


def test_ties_rows_and_asymmetric_graphs_by_hand():
    from cartnet_amd.bonds import riding_hydrogens_host
    # two carbons at the same distance: the lower edge wins; a nearer carbon without a row is skipped
    z = np.array([1, 6, 6, 6])
    ei = np.array([[3, 2, 1], [0, 0, 0]])
    dist = np.float32([1.0, 1.1, 1.1])
    parent, count, mult, _ = riding_hydrogens_host(z, ei, dist, [-1, 0, 1, -1], np.float32([0.02, 0.03]))
    assert parent.tolist() == [2, -1, -1, -1] and count.tolist() == [0, 0, 0, 0]     # the graph holds no edge 0 -> 2
    assert mult[0] == np.float32(1.2)                                         # n falls back to 1
    # the atom's own image and a hydrogen that reaches its parent through two images: counted twice
    z = np.array([6, 1])
    ei = np.array([[1, 1, 1, 0, 0], [0, 0, 1, 1, 1]])
    dist = np.float32([1.0, 1.2, 0.5, 1.2, 1.0])
    parent, count, mult, _ = riding_hydrogens_host(z, ei, dist, [0, -1], np.float32([0.02]))
    assert parent.tolist() == [-1, 0] and count.tolist() == [2, 0] and mult[1] == np.float32(1.2)


# ---------------------------------------------------------------------------------------------------- the CIF writers
def _entry(with_iso: bool) -> dict:
    z = torch.tensor([6, 8, 1, 1])
    e = {"name": "m", "z": z, "frac": torch.tensor([[0.1, 0.2, 0.3], [0.4, 0.5, 0.6], [0.15, 0.25, 0.35], [0.7, 0.8, 0.9]]),
         "cell": torch.eye(3) * 8.0, "temp": 100.0,
         "u_cif": torch.tensor([[0.03, 0.031, 0.032, 0.001, 0.002, 0.003], [0.04, 0.041, 0.042, -0.001, 0.0, 0.001]])}
    if with_iso:
        e["u_iso"] = torch.tensor([0.031, 0.041, 0.0465, float("nan")])
    return e


HEAD = ("data_m\n_cell_length_a 8.000000\n_cell_length_b 8.000000\n_cell_length_c 8.000000\n_cell_angle_alpha 90.00000\n"
        "_cell_angle_beta 90.00000\n_cell_angle_gamma 90.00000\n_diffrn_ambient_temperature 100.00\n")
ANISO = ("loop_\n_atom_site_aniso_label\n_atom_site_aniso_U_11\n_atom_site_aniso_U_22\n_atom_site_aniso_U_33\n"
         "_atom_site_aniso_U_23\n_atom_site_aniso_U_13\n_atom_site_aniso_U_12\n")
SITE = "loop_\n_atom_site_label\n_atom_site_type_symbol\n_atom_site_fract_x\n_atom_site_fract_y\n_atom_site_fract_z\n"
P1 = "_symmetry_space_group_name_H-M 'P 1'\n_symmetry_Int_Tables_number 1\nloop_\n_symmetry_equiv_pos_as_xyz\n'x, y, z'\n"
ROWS = "C1 0.030000 0.031000 0.032000 0.001000 0.002000 0.003000\nO2 0.040000 0.041000 0.042000 -0.001000 0.000000 0.001000\n"


def test_write_cif_without_the_key_writes_todays_bytes_and_with_it_the_new_columns(tmp_path):
    from cartnet_amd.predict import write_cif
    old = (HEAD + P1 + SITE + "C1 C 0.100000 0.200000 0.300000\nO2 O 0.400000 0.500000 0.600000\n"
           "H3 H 0.150000 0.250000 0.350000\nH4 H 0.700000 0.800000 0.900000\n" + ANISO + ROWS)
    write_cif(str(tmp_path / "old.cif"), _entry(False))
    assert (tmp_path / "old.cif").read_text() == old
    e = _entry(True)
    del e["u_iso"]                                                            # the key removed: the same bytes
    write_cif(str(tmp_path / "removed.cif"), e)
    assert (tmp_path / "removed.cif").read_text() == old
    write_cif(str(tmp_path / "new.cif"), _entry(True))
    new = (HEAD + P1 + SITE + "_atom_site_U_iso_or_equiv\n_atom_site_adp_type\n"
           "C1 C 0.100000 0.200000 0.300000 0.031000 Uani\nO2 O 0.400000 0.500000 0.600000 0.041000 Uani\n"
           "H3 H 0.150000 0.250000 0.350000 0.046500 Uiso\nH4 H 0.700000 0.800000 0.900000 ? Uiso\n" + ANISO + ROWS)
    assert (tmp_path / "new.cif").read_text() == new
    bad = _entry(True)
    bad["u_iso"] = bad["u_iso"][:3]
    with pytest.raises(ValueError, match="isotropic values"):
        write_cif(str(tmp_path / "bad.cif"), bad)


def test_write_cif_symmetric_without_the_key_writes_todays_bytes_and_with_it_the_new_column(tmp_path):
    from cartnet_amd.cif import read_cif
    from cartnet_amd.predict import write_cif_symmetric
    e = _entry(False)
    e.update(asym_z=e["z"], asym_labels=["C1", "O1", "H1", "H2"], asym_frac=e["frac"].double(), u_cif_asym=e["u_cif"],
             symops=["x, y, z", "-x, -y, -z"])
    ops = "loop_\n_space_group_symop_id\n_space_group_symop_operation_xyz\n1 'x, y, z'\n2 '-x, -y, -z'\n"
    rows = ROWS.replace("O2", "O1")
    old = (HEAD + ops + SITE + "_atom_site_adp_type\nC1 C 0.100000 0.200000 0.300000 Uani\nO1 O 0.400000 0.500000 0.600000 Uani\n"
           "H1 H 0.150000 0.250000 0.350000 .\nH2 H 0.700000 0.800000 0.900000 .\n" + ANISO + rows)
    write_cif_symmetric(str(tmp_path / "old.cif"), e)
    assert (tmp_path / "old.cif").read_text() == old
    e["u_iso_asym"] = torch.tensor([0.031, 0.041, 0.0465, float("nan")])
    write_cif_symmetric(str(tmp_path / "new.cif"), e)
    new = (HEAD + ops + SITE + "_atom_site_U_iso_or_equiv\n_atom_site_adp_type\n"
           "C1 C 0.100000 0.200000 0.300000 0.031000 Uani\nO1 O 0.400000 0.500000 0.600000 0.041000 Uani\n"
           "H1 H 0.150000 0.250000 0.350000 0.046500 Uiso\nH2 H 0.700000 0.800000 0.900000 ? Uiso\n" + ANISO + rows)
    assert (tmp_path / "new.cif").read_text() == new
    (back,) = read_cif(str(tmp_path / "new.cif"))                              # the project's own reader takes the file
    assert back.labels == ["C1", "O1", "H1", "H2"] and back.adp_type == ["Uani", "Uani", "Uiso", "Uiso"]
    assert back.u_iso[:3] == [0.031, 0.041, 0.0465] and back.u_iso[3] is None
    del e["u_iso_asym"]
    write_cif_symmetric(str(tmp_path / "removed.cif"), e)
    assert (tmp_path / "removed.cif").read_text() == old


# ---------------------------------------------------------------------------------------------------- U_eq on the CIF axes
def test_u_eq_of_a_cif_tensor_is_the_cartesian_trace_over_three_on_a_triclinic_cell():
    """Both sides fp64: only the few products of the transform separate them, so 1e-12 relative."""
    from cartnet_amd.predict import u_eq_of_cif
    cell = pu.cell_from_parameters(5.1, 7.3, 11.9, 62.0, 104.0, 118.0) @ pu.fixed_rotation().T
    rng = np.random.default_rng(3)
    a = rng.standard_normal((7, 3, 3))
    full = 0.01 * a @ a.transpose(0, 2, 1) + 0.005 * np.eye(3)                # symmetric positive definite, on the CIF axes
    u6 = np.stack([full[:, i, j] for i, j in pu.CIF_ORDER], axis=1)
    want = np.trace(pu.cart_from_cif(full, cell), axis1=1, axis2=2) / 3.0
    got = u_eq_of_cif(torch.from_numpy(u6), torch.from_numpy(cell)).numpy()
    assert got.dtype == np.float64 and got.shape == (7,)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    per_row = u_eq_of_cif(torch.from_numpy(u6), torch.from_numpy(cell).repeat(7, 1, 1)).numpy()       # one cell per row
    assert np.array_equal(per_row, got)
    # a cubic cell: the axes are orthogonal, so U_eq is the mean of the diagonal
    cubic = u_eq_of_cif(torch.from_numpy(u6), torch.eye(3, dtype=torch.float64) * 6.2).numpy()
    assert np.abs(cubic - u6[:, :3].mean(axis=1)).max() <= 1e-15


def test_riding_asym_maps_the_expanded_cell_back_and_refuses_another_order():
    from cartnet_amd.predict import riding_asym
    asym_z = np.array([6, 1, 8, 1], dtype=np.int32)                          # C1 H1 O1 H2; two operators: 8 atoms
    z = torch.tensor([6, 1, 8, 1, 6, 1, 8, 1])
    h_parent = torch.tensor([-1, 4, -1, -1, -1, 0, -1, 6])                    # H1 rides on the image of C1; H2 is an orphan
    h_mult = torch.tensor([0.0, 1.2, 0.0, 0.0, 0.0, 1.2, 0.0, 1.5])
    parent_asym = torch.tensor([-1, 0, -1, -1, -1, 0, -1, 2])
    ueq = torch.tensor([0.03, 0.05], dtype=torch.float64)
    u, pa = riding_asym("c", asym_z, z, h_parent, h_mult, parent_asym, ueq)
    assert u.dtype == torch.float32 and pa.tolist() == [-1, 0, -1, -1]
    assert u[:3].tolist() == [np.float32(0.03), np.float32(np.float64(np.float32(1.2)) * 0.03), np.float32(0.05)]
    assert bool(torch.isnan(u[3]))
    with pytest.raises(ValueError, match="crystal c: .*asymmetric unit"):
        riding_asym("c", asym_z, z.flip(0), h_parent, h_mult, parent_asym, ueq)


def test_riding_h_is_exported_from_metrics():
    from cartnet_amd import metrics
    assert metrics.RidingH._fields == ("parent", "count", "mult", "u_iso", "crystal_stats")
    with pytest.raises(ValueError, match="u_eq must be"):
        metrics.riding_h(torch.zeros(2), {})
