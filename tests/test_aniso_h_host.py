"""The anisotropic-hydrogen rule of ``cartnet_amd.bonds`` in numpy (``aniso_hydrogens_host``) on graphs built on the host:
exactly rigid rows give the known rigid body's tensor at the hydrogen, a cell face changes no bit, the source codes of
every kind of hydrogen, the internal motion in the bond frame, the rule without TLS results; then the surface around it:
the entry point's declaration and binding, the keys and their split table, the writers' text and ``main.py``'s refusals."""
import os
import re

import numpy as np
import pytest

import aniso_utils as au
import molecule_utils as mu
import tls_utils as tu

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def test_the_entry_point_is_declared_bound_and_built():
    from cartnet_amd import lib
    from cartnet_amd.build import EXTRA_FLAGS, SOURCES
    hdr = open(os.path.join(ROOT, "include", "cartnet_hip.h")).read()
    block = hdr[:hdr.index("int cartnet_adp_aniso_h(")].rsplit("/*", 1)[1]
    assert "Anisotropic hydrogens" in block and "dataset/datasetADP.py:49" in block and "no counterpart" in block
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+cartnet_adp_aniso_h\s*\(([^)]*)\)\s*;", hdr)
    assert m and len(m.group(1).split(",")) == 22 == len(lib.PROTOTYPES["cartnet_adp_aniso_h"][1])
    assert "struct" not in m.group(1)                                         # plain arguments
    assert "aniso_h_ops.hip" in SOURCES and os.path.exists(os.path.join(ROOT, "cartnet_amd", "csrc", "aniso_h_ops.hip"))
    assert {"-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage"} <= set(EXTRA_FLAGS["aniso_h_ops.hip"])
    assert lib.ABI_VERSION == 16 == lib.load().cartnet_abi_version()          # no struct changed
    f = lib.load().cartnet_adp_aniso_h
    nul, par, out = [None] * 12, (0.005, 0.02), [None] * 4
    assert f(*nul, *par, 0, 10, 5, 50, *out) == 0                             # no crystals
    assert f(*nul, *par, 4, 0, 5, 50, *out) == 0                              # no atoms
    assert f(*nul, *par, 4, 10, 5, 50, *out) == 1                             # null pointers are an error, not a fault
    assert f(*nul, *par, -1, 10, 5, 50, *out) == 1 and f(*nul, float("nan"), 0.02, 4, 10, 5, 50, *out) == 1


def test_rigid_rows_give_the_rigid_body_at_the_hydrogen():
    """Noise-free rigid rows of a known T, L, S on a helix of 7, stretch = bend = 0: the parent's tensor plus the change of
    the fitted motion is the known body's tensor at the hydrogen.  What separates them is the fp32 storage of the parent's
    row and of ``params`` and the final rounding."""
    from cartnet_amd.bonds import ANISO_H_TLS, tls_model
    carbons = tu.helix(7, (3, 12, 12))
    pos, z = tu.with_hydrogens(carbons)
    worst = 0.0
    for seed in (0, 1, 2, 3):
        rows = tu.rigid_rows(carbons, seed).astype(np.float32)
        got = host = au.host_chain(pos, mu.cubic(30.0), z, rows)
        h = np.nonzero(z == 1)[0]
        assert host["source"][h].tolist() == [ANISO_H_TLS] * 7 and host["parent"][h].tolist() == (h - 1).tolist()
        want = tls_model(pos[h] - carbons.mean(axis=0), *tu.known_tls(seed))
        err = np.abs(got["u_h"][h].astype(np.float64) - want).max() / np.abs(rows).max()
        worst = max(worst, err)
        assert err <= tu.EPS22, (seed, err)
        assert np.abs(host["bond"][h] - [0.0, 0.0, 1.0]).max() <= 2.0 ** -22    # the edge's vector: 1 A above
    print(f"largest |u_h - U_TLS(hydrogen)| / max |U|: {worst:.2e} (bound {tu.EPS22:.2e})")


def test_a_cell_face_changes_no_bit():
    wrapped, plain = (au.host_chain(*au.face_crystal(wrap), stretch=0.005, bend=0.02) for wrap in (True, False))
    pos = au.face_crystal(True)[0]
    moved = np.abs(pos - au.face_crystal(False)[0]).max(axis=1) > 1.0
    assert moved.sum() == 2 and (au.face_crystal(True)[2][moved] == 1).all()    # two hydrogens cross the face
    assert wrapped["source"].tolist() == plain["source"].tolist() == [1, 3] * 7
    assert wrapped["u_h"].tobytes() == plain["u_h"].tobytes()
    assert wrapped["fit"]["params"].tobytes() == plain["fit"]["params"].tobytes()


def test_source_codes():
    from cartnet_amd.bonds import ANISO_H_COPY, ANISO_H_NONE, ANISO_H_PARENT, ANISO_H_TLS, ANISO_H_TLS_DEFICIENT
    assert (ANISO_H_NONE, ANISO_H_COPY, ANISO_H_PARENT, ANISO_H_TLS, ANISO_H_TLS_DEFICIENT) == (0, 1, 2, 3, 4)
    pos, cell, z, rows = au.mixed_crystal()
    got = au.host_chain(pos, cell, z, rows, stretch=0.005, bend=0.02)
    assert np.bincount(got["source"], minlength=5).tolist() == [1, 24, 3, 13, 8]
    h = np.nonzero(z == 1)[0][:-1]
    assert got["parent"][h].tolist() == (h - 1).tolist() and got["parent"][-1] == -1
    rank = got["fit"]["rank"][got["atom_row"][h - 1]]
    assert got["source"][h].tolist() == [3 if r == 20 else 4 if r > 0 else 2 for r in rank]
    assert sorted(set(rank.tolist())) == [0, 19, 20]
    # copies bit for bit, NaN exactly where there is no tensor, symmetric everywhere else
    heavy = z != 1
    assert got["u_h"][heavy].tobytes() == rows.tobytes()
    assert np.isnan(got["u_h"][-1]).all() and not np.isnan(got["u_h"][:-1]).any()
    assert np.array_equal(got["u_h"][h], got["u_h"][h].transpose(0, 2, 1))
    assert got["u_h"].dtype == np.float32 and got["source"].dtype == np.int32
    stats = got["crystal_stats"]
    tr = got["u_h"][h].astype(np.float64)
    assert stats.shape == (1, 4) and stats[0, :2].tolist() == [24.0, 21.0] and stats[0, 3] == 0.0
    assert stats[0, 2] == pytest.approx(np.trace(tr, axis1=1, axis2=2).sum() / 3.0, rel=1e-12)
    # the polymer reaches its own image: not fitted, every hydrogen takes its parent's tensor alone
    pos, cell, z, rows = au.polymer_crystal()
    got = au.host_chain(pos, cell, z, rows, stretch=0.005, bend=0.02)
    assert got["source"].tolist() == [1, 2] * 8 and (got["fit"]["rank"] == 0).all() and not got["lib"].any()


def test_internal_motion_in_the_bond_frame():
    stretch, bend = 0.007, 0.031
    pos, cell, z, rows = au.mixed_crystal()
    got = au.host_chain(pos, cell, z, rows, stretch=stretch, bend=bend)
    bound = 3 * 2.0 ** -24 * float(np.nanmax(np.abs(got["u_h"])))            # one rounding per component, |d|_1^2 <= 3
    for i in np.nonzero(got["source"] >= 2)[0]:
        Up = got["rows"][got["atom_row"][got["parent"][i]]].astype(np.float64)
        rest = got["u_h"][i].astype(np.float64) - 0.5 * (Up + Up.T) - got["lib"][i]
        d = got["bond"][i] / np.linalg.norm(got["bond"][i])
        across = np.cross(d, [1.0, 0.0, 0.0])
        across /= np.linalg.norm(across)
        assert abs(d @ rest @ d - stretch) <= bound and abs(across @ rest @ across - bend) <= bound
        assert abs(d @ rest @ across) <= bound
    assert np.abs(got["lib"][got["source"] >= 3]).max() > 1e-5               # the libration term is there


def test_without_tls_every_hydrogen_takes_its_parent():
    pos, cell, z, rows = au.mixed_crystal()
    got = au.host_chain(pos, cell, z, rows, tls=False, stretch=0.005, bend=0.02)
    assert np.bincount(got["source"], minlength=5).tolist() == [1, 24, 24, 0, 0] and not got["lib"].any()
    assert got["crystal_stats"][0, :2].tolist() == [24.0, 0.0]
    from cartnet_amd.bonds import aniso_hydrogens_host
    with pytest.raises(ValueError, match="together"):
        aniso_hydrogens_host(rows, z, np.zeros((2, 0), dtype=np.int64), [], np.zeros((0, 3)), got["atom_row"], got["parent"],
                             x=np.zeros((len(z), 3)))


def test_not_positive_definite_and_nan_count():
    from cartnet_amd.bonds import positive_definite
    u = np.stack([np.eye(3), -np.eye(3), np.diag([1.0, 1.0, -1.0]), np.full((3, 3), np.nan),
                  np.array([[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]])]).astype(np.float32)
    assert positive_definite(u).tolist() == [True, False, False, False, False]


def test_keys_tables_and_pass_statistics():
    import torch
    from cartnet_amd import metrics, predict as p
    assert p.AH_KEYS == ("h_u_cart", "h_u_cif", "h_u_eq", "h_source", "h_aniso_stats") and p.AH_SYM_KEYS == ("h_u_cif_asym",)
    assert tuple(p.AH_SPLIT) == p.AH_KEYS and [p.AH_SPLIT[k] for k in p.AH_KEYS] == ["atom"] * 4 + ["crystal"]
    assert not set(p.AH_SPLIT) & (set(p.SPLIT) | set(p.MOL_SPLIT) | set(p.TLS_SPLIT) | set(p.SERIES_SPLIT))
    assert metrics.AnisoH._fields == ("u_h", "source", "crystal_stats")
    result = {k: [v] for k, v in au.entry_with_hydrogens().items()}
    result["stats"] = [torch.tensor([0.03, 0.02, 0.0], dtype=torch.float64)]
    result["h_aniso_stats"] = [torch.tensor([1.0, 0.0, 0.045, 0.0], dtype=torch.float64)]
    assert set(p.AH_KEYS) - {"h_u_cart"} <= set(p.entry(result, 0))           # entry() passes them on
    res = p.pass_statistics(result)
    assert (res["h_aniso"], res["h_aniso_tls"], res["h_aniso_non_positive"]) == (1, 0, 0) and res["h_aniso_ueq_mean"] == 0.045
    del result["h_aniso_stats"]
    assert not {"h_aniso", "h_aniso_tls", "h_aniso_ueq_mean", "h_aniso_non_positive"} & set(p.pass_statistics(result))
    with pytest.raises(ValueError, match="riding_h"):
        p.predict_adps(None, None, "cpu", aniso_h=(0.005, 0.02))


def test_writer_text(tmp_path):
    import torch
    from cartnet_amd import cif, predict as p
    e = au.entry_with_hydrogens()
    p.write_cif(str(tmp_path / "h.cif"), e)
    text = open(tmp_path / "h.cif").read().splitlines()
    assert "C1 C 0.100000 0.200000 0.300000 0.030000 Uani" in text
    assert "H2 H 0.100000 0.200000 0.400000 0.045000 Uani" in text            # its own U_eq, not the riding value
    assert "H3 H 0.700000 0.700000 0.700000 ? Uiso" in text                   # the orphan
    at = text.index("_atom_site_aniso_U_12")
    assert text[at + 1:] == ["C1 0.020000 0.030000 0.040000 0.001000 0.002000 0.003000",
                             "H2 0.040000 0.050000 0.045000 0.001000 0.002000 0.003000"]
    # without the new keys the file is what it was
    old = {k: v for k, v in e.items() if not k.startswith("h_u") and k != "h_source"}
    p.write_cif(str(tmp_path / "old.cif"), old)
    was = open(tmp_path / "old.cif").read().splitlines()
    assert "H2 H 0.100000 0.200000 0.400000 0.036000 Uiso" in was and was[was.index("_atom_site_aniso_U_12") + 1:] == text[at + 1:at + 2]
    # the file's own setting: the asymmetric unit is the first atoms of the expanded cell
    sym = dict(e, asym_labels=["Ca", "Ha", "Hb"], asym_frac=e["frac"], asym_z=e["z"], symops=["x, y, z"],
               u_cif_asym=e["u_cif"], u_iso_asym=e["u_iso"],
               h_u_cif_asym=p.aniso_asym(e["z"], e["u_cif"], e["h_u_cif"]))
    assert torch.equal(sym["h_u_cif_asym"][:2], e["h_u_cif"][:2]) and bool(torch.isnan(sym["h_u_cif_asym"][2]).all())
    p.write_cif_symmetric(str(tmp_path / "s.cif"), sym)
    text = open(tmp_path / "s.cif").read().splitlines()
    assert "Ha H 0.100000 0.200000 0.400000 0.045000 Uani" in text and "Hb H 0.700000 0.700000 0.700000 ? Uiso" in text
    assert text[text.index("_atom_site_aniso_U_12") + 1:] == ["Ca 0.020000 0.030000 0.040000 0.001000 0.002000 0.003000",
                                                               "Ha 0.040000 0.050000 0.045000 0.001000 0.002000 0.003000"]
    assert cif.__name__ == "cartnet_amd.cif"


def test_the_flag_is_refused_before_the_device_is_touched(monkeypatch):
    import main as entry
    from cartnet_amd.bonds import ANISO_H_BEND, ANISO_H_STRETCH

    def touched(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(entry.cdist, "init_from_env", touched)
    monkeypatch.setattr(entry, "create_model", touched)
    with pytest.raises(SystemExit, match="--aniso_h serves --predict only"):
        entry.main(["--aniso_h", "--riding_h"])
    with pytest.raises(SystemExit, match="--aniso_h serves --predict only"):
        entry.main(["--aniso_h", "--riding_h", "--inference"])
    with pytest.raises(SystemExit, match="--riding_h"):
        entry.main(["--predict", "--aniso_h", "--predict_input", "none.cnshard", "--checkpoint_path", "none.ckpt"])
    args = entry.build_parser().parse_args([])
    assert args.aniso_h is False and (args.aniso_h_stretch, args.aniso_h_bend) == (ANISO_H_STRETCH, ANISO_H_BEND) == (0.005, 0.020)
    assert entry.analysis_options(args) == {"rigid_bond": None, "riding_h": None}
    args = entry.build_parser().parse_args(["--aniso_h", "--aniso_h_stretch", "0.01", "--aniso_h_bend", "0.03"])
    assert entry.analysis_options(args) == {"rigid_bond": None, "riding_h": None, "aniso_h": (0.01, 0.03)}
    assert entry.analysis_options(args, inference=True) == {"rigid_bond": None}
    from cartnet_amd.config import set_cfg
    set_cfg()
