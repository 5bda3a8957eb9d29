"""CPU checks of the CIF reader, the host statement of the symmetry expansion and the symmetric CIF writer."""
import os
import re

import numpy as np
import pytest
import torch

import cif_utils as cu
from cartnet_amd import cif, symmetry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "cif_expand.npz"))
NEW_ENTRY_POINTS = ("cartnet_symmetry_expand_workspace_bytes", "cartnet_symmetry_expand_count",
                    "cartnet_symmetry_expand_fill", "cartnet_symmetry_targets", "cartnet_symmetry_average")


@pytest.mark.parametrize("key", sorted(cu.CRYSTALS))
def test_reader_understands_the_test_crystals(key):
    spec = cu.CRYSTALS[key]
    (c,) = cif.read_cif(cu.cif_text(key))
    assert c.name == "crystal_" + key and c.problem is None
    assert c.cell_parameters == spec["cell"] and c.temperature == spec["temp"] and c.pressure is None
    assert c.labels == [a[0] for a in spec["atoms"]] and c.symbols == [a[1] for a in spec["atoms"]]
    assert c.z == [cif._Z[a[1].upper()] for a in spec["atoms"]]
    assert c.frac == [tuple(float(f"{v:.4f}") for v in a[2:5]) for a in spec["atoms"]]         # esds dropped
    assert all(isinstance(v, float) for row in c.frac for v in row)
    assert c.occupancy == [1.0] * len(c.labels) and c.disorder_group == ["."] * len(c.labels)
    assert c.adp_type == ["Uiso" if a[5] is None else "Uani" for a in spec["atoms"]]
    assert c.u_aniso == {a[0]: a[5] for a in spec["atoms"] if a[5] is not None}
    assert np.isnan(c.u_cif()[[a[5] is None for a in spec["atoms"]]]).all()
    W, w = cu.op_arrays(spec["ops"] or [cu.IDENTITY])
    assert len(c.symops) == len(W)
    assert np.array_equal(np.stack([o[0] for o in c.symops]), W) and np.array_equal(np.stack([o[1] for o in c.symops]), w)
    assert c.symops[0][0].dtype == np.int64 and c.symops[0][1].dtype == np.float64
    assert c.reject_reason(True) is None and c.reject_reason(False) is None


def test_reader_syntax():
    text = ("# comment\ndata_one\n_cell_length_a 5.0(1) # trailing comment\n_symmetry_space_group_name_H-M 'P 1'\n"
            "_chemical_name_common \"it's quoted\"\n_exptl_special_details\n;\nfree text; with a ; inside\n_not_a_tag 1\n;\n"
            "_diffrn_ambient_temperature '293(2) K'\nloop_\n_atom_site_label\n_atom_site_fract_x\n_atom_site_fract_y\n"
            "_atom_site_fract_z\n_atom_site_U_iso_or_equiv\nCl1A .5 -0.25(3) 1.0E-1 ?\nHW1 0.1 0.2 0.3 .\n"
            "data_two\n_symmetry_Int_Tables_number 1\n")
    one, two = cif.read_cif(text)
    assert (one.name, two.name) == ("one", "two")
    assert one.temperature == 293.0                                    # the first number in the field
    assert one.labels == ["Cl1A", "HW1"] and one.symbols == ["Cl", "H"] and one.z == [17, 1]   # from the label's prefix
    assert one.frac == [(0.5, -0.25, 0.1), (0.1, 0.2, 0.3)] and one.u_iso == [None, None]
    assert one.cell_parameters is None and one.reject_reason(False) == "no cell"
    assert len(one.symops) == 1 and len(two.symops) == 1               # P1 by name, P1 by number
    assert two.reject_reason(False) == "no cell"
    assert cif.number("0.1234(5)") == 0.1234 and cif.number("-1.5e-3(2)") == -1.5e-3 and cif.number("?") is None
    with pytest.raises(cif.CifError):
        cif.read_cif("data_x\n_tag 'never closed\n")
    with pytest.raises(cif.CifError):
        cif.read_cif("data_x\nloop_\n_a\n_b\n1 2 3\n")


def test_parse_symop():
    W, w = cif.parse_symop("-x+1/2, y+1/2, -z")
    assert W.tolist() == [[-1, 0, 0], [0, 1, 0], [0, 0, -1]] and w.tolist() == [0.5, 0.5, 0.0]
    W, w = cif.parse_symop("2/3+X-Y,1/3+x,-Z+1/3")
    assert W.tolist() == [[1, -1, 0], [1, 0, 0], [0, 0, -1]] and w.tolist() == [2 / 3, 1 / 3, 1 / 3]
    assert cif.parse_symop("x,y,z+0.25")[1].tolist() == [0.0, 0.0, 0.25]
    for bad in ("2x, y, z", "x, y", "x, x, z", "x+y+z, y, q", "x+x, y, z"):
        with pytest.raises(cif.CifError):
            cif.parse_symop(bad)
    for ops in (cu.P21C, cu.R3BAR, cu.FM3M):                          # format_symop is parse_symop's inverse
        for op, (W, w) in zip(ops, zip(*cu.op_arrays(ops))):
            W2, w2 = cif.parse_symop(cif.format_symop(W, w))
            assert np.array_equal(W2, W) and np.array_equal(w2, w)


def test_identity_is_moved_to_the_front_and_must_be_there():
    text = cu.cif_text("b")
    first, second = "1 'x, y, z'", "2 '" + cu.op_string(cu.P21C[1]) + "'"
    swapped = text.replace(first, "@").replace(second, first.replace("1 ", "2 ")).replace("@", second.replace("2 ", "1 "))
    assert swapped != text
    (c,) = cif.read_cif(swapped)
    assert np.array_equal(c.symops[0][0], np.eye(3)) and not c.symops[0][1].any() and len(c.symops) == 4
    assert c.symop_strings[0].replace(" ", "") == "x,y,z"
    (c,) = cif.read_cif(text.replace(first, "1 'x, y, z+1/2'"))
    assert c.reject_reason(False) == "the identity is not among the operators"


def test_reject_reasons():
    want = {"disordered": ("disorder", "disorder"),
            "isotropic_carbon": ("non-hydrogen atom C2 without anisotropic ADPs", None),     # the hydrogen needs none
            "no_operators": ("no operators", "no operators"), "pressure": ("pressure given", "pressure given"),
            "aniso_in_b": ("aniso loop in B", None), "no_temperature": ("no temperature", "no temperature"),
            "ambiguous": (None, None), "singular": (None, None)}          # these two are the expansion's to refuse
    for key, (labeled, unlabeled) in want.items():
        (c,) = cif.read_cif(cu.BAD[key])
        assert (c.reject_reason(True), c.reject_reason(False)) == (labeled, unlabeled), key
    (c,) = cif.read_cif(cu.BAD["no_temperature"])
    assert c.reject_reason(True, temperature=150.0) is None
    (c,) = cif.read_cif(cu.BAD["disordered"].replace("0.5 1\n", "0.5 .\n"))
    assert c.reject_reason(False) == "disorder"                          # an occupancy below 1 alone


def test_cell_matrix_against_fp64_numpy():
    """A handful of fp64 operations per entry (the last one: four cosines, five products, a square root, a quotient): the
    two statements differ by a few units in the last place.  Bound: 8 * 2^-52 of the largest entry."""
    for c in GOLDEN["cells"]:
        got, want = cif.cell_matrix(*c), cu.cell_reference(*c)
        assert got.dtype == np.float64
        assert np.abs(got - want).max() <= 8 * 2.0 ** -52 * np.abs(want).max()
        assert got[0, 1] == 0.0 and got[0, 2] == 0.0 and got[1, 2] == 0.0       # rows = lattice vectors, a along x


def test_cell_matrix_against_the_reference():
    """The reference forms its cell in fp32 (dataset/extract_csd_data.py:15-25).  Its own error, measured here as the
    fixture against the fp64 formula, is 5.6e-7 to 1.5e-6 Angstrom over the six cells (printed); ``cell_matrix`` must
    agree with the fixture within twice that, per cell."""
    for c, ref in zip(GOLDEN["cells"], GOLDEN["matrices"]):
        own = np.abs(ref.astype(np.float64) - cu.cell_reference(*c)).max()
        got = np.abs(cif.cell_matrix(*c) - ref.astype(np.float64)).max()
        print(f"cell {[float(v) for v in c]}: reference fp32 error {own:.3e}, cell_matrix - reference {got:.3e}")
        assert got <= 2 * own
        assert own <= 2.0 ** -20 * np.abs(ref).max()                  # and the fixture is an fp32 statement of the formula


def test_kept_mask_equals_the_reference():
    crystals = [cu.crystal_from_coords(f"set{i}", GOLDEN[f"coord{i}"]) for i in range(int(GOLDEN["n_sets"]))]
    arrays, _ = symmetry.expand_host(crystals, labeled=False)
    for i, c in enumerate(crystals):
        coord, keep = GOLDEN[f"coord{i}"], GOLDEN[f"keep{i}"]
        x = symmetry.candidates_host(torch.from_numpy(coord), torch.eye(3)[None], torch.zeros(1, 3))
        rep = symmetry.first_duplicate_host(x)
        assert np.array_equal((rep == torch.arange(len(coord))).numpy(), keep)
        z = arrays["z"][arrays["atom_ptr"][i]:arrays["atom_ptr"][i + 1]]
        assert np.array_equal(cu.kept_mask(z, len(coord)), keep)
        assert list(z) == sorted(z)                                    # stable: kept atoms stay in candidate order


def test_expand_host_on_the_test_crystals():
    crystals = cif.read_cif(cu.batch_text())
    arrays, rows = symmetry.expand_host(crystals, labeled=True)
    assert np.diff(arrays["atom_ptr"]).tolist() == [cu.ATOMS[k][0] for k in cu.BATCH]
    assert np.diff(arrays["y_ptr"]).tolist() == [cu.ATOMS[k][1] for k in cu.BATCH]
    assert arrays["y"].shape == (arrays["y_ptr"][-1], 9) and arrays["pos"].dtype == np.float32
    assert arrays["temperature"].tolist() == [cu.CRYSTALS[k]["temp"] for k in cu.BATCH]
    assert (rows["orbit_row"] >= 0).all()
    for g, key in enumerate(cu.BATCH):                                  # identity rows carry the file's U, :115-123
        r0 = arrays["y_ptr"][g]
        u = np.array([a[5] for a in cu.CRYSTALS[key]["atoms"] if a[5] is not None])
        want = cu.cart_from_cif(cu.full(u), cu.cell_reference(*cu.CRYSTALS[key]["cell"]))
        got = arrays["y"][r0:r0 + len(u)].reshape(-1, 3, 3)
        assert np.abs(got - want).max() <= 2.0 ** -23 * np.abs(want).max()
    for key in ("ambiguous", "singular"):
        with pytest.raises(ValueError, match=f"crystal {key}:"):
            symmetry.expand_host(cif.read_cif(cu.BAD[key]), labeled=True)
    with pytest.raises(ValueError, match="crystal disordered: disorder"):
        symmetry.expand_host(cif.read_cif(cu.BAD["disordered"]), labeled=True)


def test_new_entry_points_are_declared_and_bound():
    from cartnet_amd import lib
    from cartnet_amd.build import EXTRA_FLAGS, SOURCES
    assert lib.ABI_VERSION == 16
    header = open(os.path.join(ROOT, "include", "cartnet_hip.h")).read()
    cdll = lib.load()
    assert cdll.cartnet_abi_version() == 16
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in lib.PROTOTYPES and hasattr(cdll, name), name
    assert "symmetry_ops.hip" in SOURCES and "-ffp-contract=off" in EXTRA_FLAGS["symmetry_ops.hip"]
    # argument validation runs before anything touches a device
    assert cdll.cartnet_symmetry_expand_workspace_bytes(3, 1000, 5) > 1000 * 40
    assert cdll.cartnet_symmetry_expand_count(*([None] * 10), 1, 1, 1, 1, 1, None, 0, None, None, None, None) == 1
    assert b"null array" in cdll.cartnet_last_error()
    assert cdll.cartnet_symmetry_average(None, None, None, None, 0, 0, 0, None, None, None, None, None, 1, 1, 0, None, None,
                                         None) == 0


def test_write_cif_symmetric_round_trips(tmp_path):
    from cartnet_amd.predict import write_cif_symmetric
    for key in ("b", "c"):
        (c,) = cif.read_cif(cu.cif_text(key, name=f"in_{key}"))
        heavy = [i for i, z in enumerate(c.z) if z != 1]
        gen = torch.Generator().manual_seed(5)
        u = (torch.rand(len(heavy), 6, generator=gen) - 0.3) * 0.05
        entry = {"name": c.name, "cell": torch.from_numpy(c.cell()).float(), "temp": c.temperature,
                 "asym_labels": c.labels, "asym_frac": torch.tensor(c.frac, dtype=torch.float64),
                 "asym_z": torch.tensor(c.z, dtype=torch.int32), "symops": c.symop_strings, "u_cif_asym": u,
                 "spread": torch.zeros(len(heavy))}
        path = str(tmp_path / f"{key}.cif")
        write_cif_symmetric(path, entry)
        (back,) = cif.read_cif(path)
        assert back.name == c.name and back.labels == c.labels and back.z == c.z and back.temperature == c.temperature
        assert back.reject_reason(True) is None
        assert len(back.symops) == len(c.symops)
        for (W1, w1), (W2, w2) in zip(back.symops, c.symops):
            assert np.array_equal(W1, W2) and np.array_equal(w1, w2)
        assert np.abs(np.array(back.frac) - np.array(c.frac)).max() <= 0.5e-6 + 1e-15          # six printed digits
        assert np.abs(np.array(back.cell_parameters) - np.array(c.cell_parameters)).max() <= 1e-5
        got = np.array([back.u_aniso[c.labels[i]] for i in heavy])
        assert np.abs(got - u.double().numpy()).max() <= 0.5e-6 + 1e-15
        assert sorted(back.u_aniso) == sorted(c.labels[i] for i in heavy)
    with pytest.raises(ValueError, match="ADP rows"):
        entry["u_cif_asym"] = u[:-1]
        write_cif_symmetric(path, entry)
