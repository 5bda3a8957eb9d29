"""``main.py --predict --riding_h --aniso_h`` end to end on three of the crystals of the kernel test (every source code,
the polymer, the helix at a cell face) with a small CartNet whose checkpoint the test saves: the JSON fields against the
pickle, the pickle against a direct ``metrics.aniso_h`` on its own ``u_cart``, the CIFs through the project's reader, the
flag without ``--tls_fit``, beside ``--predict_temperatures`` and ``--rotations``, with a CIF file as input, and nothing
changed without it."""
import json
import os

import numpy as np
import pytest
import torch

import aniso_utils as au
import cif_utils as cu
from test_gpu_main_rigid_molecule import MODEL, _graphed, _load, _same
from test_gpu_main_riding_h import METHANOL

pytestmark = pytest.mark.gpu

NAMES = ("mixed", "polymer", "face")
AH_JSON = {"h_aniso", "h_aniso_tls", "h_aniso_ueq_mean", "h_aniso_non_positive"}
ROWS, ATOMS = (24, 8, 7), (49, 16, 14)
SOURCES = ([1, 24, 3, 13, 8], [0, 8, 8, 0, 0], [0, 7, 0, 7, 0])             # per crystal: atoms with source 0 ... 4
SHAPES = {"h_u_cart": (3, 3), "h_u_cif": (6,), "h_u_eq": (), "h_source": ()}


def _crystals():
    from cartnet_amd.data import Data
    out = []
    for pos, cell, z, _ in (au.mixed_crystal(), au.polymer_crystal(), au.face_crystal()):
        out.append(Data(x=torch.tensor(z, dtype=torch.int64), pos=torch.tensor(pos, dtype=torch.float32),
                        cell=torch.tensor(cell, dtype=torch.float32).unsqueeze(0), natoms=torch.tensor([len(z)]),
                        temperature=torch.tensor([0.25])))
    return out


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """(directory, checkpoint of a fresh small CartNet, the unlabeled shard of the three crystals)."""
    import main as entry
    from cartnet_amd import shard
    from cartnet_amd.config import set_cfg
    from cartnet_amd.master import create_model
    d = tmp_path_factory.mktemp("aniso_h")
    entry.fill_cfg(entry.build_parser().parse_args(MODEL))
    torch.manual_seed(0)
    ckpt = str(d / "fresh.ckpt")
    torch.save({"model_state": create_model().state_dict()}, ckpt)
    src = str(d / "three.cnshard")
    shard.write_shard(src, _crystals(), names=list(NAMES))
    yield d, ckpt, src
    set_cfg()


def _check_entries(out, res, n_entries, sources=SOURCES):
    """What holds for every entry of a flag-on result: shapes and dtypes, NaN exactly where there is no tensor, the
    non-hydrogen atoms' rows, ``h_aniso_stats`` and the JSON line against sums over the pickle."""
    from cartnet_amd.bonds import positive_definite
    count = tls = bad = 0
    total = 0.0
    for k in range(n_entries):
        g = k * len(sources) // n_entries
        z, src = out["z"][k], out["h_source"][k]
        n = int(z.shape[0])
        for key, tail in SHAPES.items():
            t = out[key][k]
            assert t.dtype == (torch.int32 if key == "h_source" else torch.float32) and tuple(t.shape) == (n,) + tail, (key, k)
        assert np.bincount(src.numpy(), minlength=5).tolist() == sources[g], k
        assert bool(((src == 1) == (z != 1)).all())
        for key in ("h_u_cart", "h_u_cif", "h_u_eq"):
            t = out[key][k].reshape(n, -1)
            assert bool(torch.isnan(t[src == 0]).all()) and not bool(torch.isnan(t[src > 0]).any()), (key, k)
        heavy = z != 1
        assert _same(out["h_u_cart"][k][heavy], out["u_cart"][k]) and _same(out["h_u_cif"][k][heavy], out["u_cif"][k])
        assert _same(out["h_u_eq"][k][heavy], out["u_eq"][k])
        h = src >= 2
        t = out["h_u_cart"][k][h]
        assert torch.equal(t, t.transpose(1, 2))
        st = out["h_aniso_stats"][k]
        trace = float(t.double().diagonal(dim1=1, dim2=2).sum()) / 3.0
        assert st.dtype == torch.float64 and tuple(st.shape) == (4,)
        assert st[0] == int(h.sum()) and st[1] == int((src >= 3).sum()) and float(st[2]) == pytest.approx(trace, rel=1e-12)
        assert st[3] == int((~positive_definite(t.numpy())).sum())
        count, tls, bad, total = count + int(h.sum()), tls + int((src >= 3).sum()), bad + int(st[3]), total + float(st[2])
    assert (res["h_aniso"], res["h_aniso_tls"], res["h_aniso_non_positive"]) == (count, tls, bad)
    assert res["h_aniso_ueq_mean"] == pytest.approx(total / count, rel=1e-12)
    assert res["h_aniso"] == res["hydrogens"] - res["h_orphans"]


def test_predict_carries_the_direct_result(work, monkeypatch, capsys):
    import main as entry
    from cartnet_amd import metrics as gm
    from cartnet_amd.cif import read_cif
    from cartnet_amd.predict import AH_KEYS, H_KEYS, KEYS, MOL_KEYS, TLS_KEYS, aniso_entries
    d, ckpt, src = work
    monkeypatch.chdir(d)
    common = ["--predict", "--predict_input", src, "--checkpoint_path", ckpt, "--eval_batch", "2", "--riding_h",
              "--rigid_molecule", "--tls_fit"] + MODEL
    plain = entry.main(common + ["--predict_output", "plain.pkl", "--predict_cif_dir", "plain_cifs"])
    capsys.readouterr()
    res = entry.main(common + ["--predict_output", "aniso.pkl", "--predict_cif_dir", "aniso_cifs", "--aniso_h"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line == res
    old, out = _load("plain.pkl"), _load("aniso.pkl")
    assert not set(plain) & AH_JSON and tuple(old) == KEYS + H_KEYS + MOL_KEYS + TLS_KEYS      # without the flag: as it was
    assert set(res) == set(plain) | AH_JSON and list(out) == list(old) + list(AH_KEYS)
    skip = ("output", "cif_dir")
    assert {k: v for k, v in res.items() if k in plain and k not in skip} == {k: v for k, v in plain.items() if k not in skip}
    for k in old:                                                             # every shared key: the same bits
        assert len(old[k]) == len(out[k]) == 3 and all(_same(p, q) for p, q in zip(old[k], out[k])), k
    _check_entries(out, res, 3)
    assert (res["h_aniso"], res["h_aniso_tls"]) == (39, 28)
    s = _graphed(src)
    for k in range(3):                                                        # crystal k alone, from the pickle's own u_cart
        b = s.collate([k])
        rp = gm.target_row_ptr(b)
        u = out["u_cart"][k].cuda()
        ex = gm.adp_export(u, rp, b.cell, axes=False, stats=False, check=False)
        rh = gm.riding_h(ex.u_eq, b, 0.4, 1.2, 1.5)
        mo = gm.molecules(b, rp, 0.4, rows=ROWS[k])
        want = aniso_entries(gm.aniso_h(u, b, rp, rh, mo, gm.tls_fit(u, b, rp, mo), 0.005, 0.020), b)
        for key in AH_KEYS:
            t = want[key][0] if key == "h_aniso_stats" else want[key]
            assert _same(out[key][k], t.cpu().contiguous()), (key, k)
    # the CIFs: the project's reader takes them, the hydrogens are Uani with a row of their own
    for k, name in enumerate(NAMES):
        (back,) = read_cif(os.path.join("aniso_cifs", f"{name}.cif"))
        (was,) = read_cif(os.path.join("plain_cifs", f"{name}.cif"))
        src_k = out["h_source"][k]
        assert len(back.u_aniso) == ROWS[k] + int((src_k >= 2).sum()) and len(was.u_aniso) == ROWS[k]
        assert back.adp_type == ["Uani" if c > 0 else "Uiso" for c in src_k.tolist()]
        assert [v is None for v in back.u_iso] == [c == 0 for c in src_k.tolist()]
        text = open(os.path.join("aniso_cifs", f"{name}.cif")).read().splitlines()
        loop = text[text.index("_atom_site_aniso_U_12") + 1:]
        assert [row.split()[0] for row in loop] == [lab for lab, c in zip(back.labels, src_k.tolist()) if c > 0]   # atom order
        u6 = back.u_cif()
        assert np.abs(u6[src_k.numpy() > 0] - out["h_u_cif"][k][src_k > 0].double().numpy()).max() <= 0.5e-6 + 1e-12
        shown = np.array([np.nan if v is None else v for v in back.u_iso])
        assert np.nanmax(np.abs(shown - out["h_u_eq"][k].double().numpy())) <= 0.5e-6 + 1e-12
    # the libration term is in the tensors: the same pass without the fit gives other hydrogens, the same heavy atoms
    bare = entry.main([a for a in common if a != "--tls_fit"] + ["--predict_output", "bare.pkl", "--aniso_h"])
    low = _load("bare.pkl")
    assert "tls_u" not in low and bare["h_aniso_tls"] == 0 and bare["h_aniso"] == 39
    for k in range(3):
        src_k = low["h_source"][k]
        assert np.bincount(src_k.numpy(), minlength=5).tolist() == SOURCES[k][:2] + [sum(SOURCES[k][2:]), 0, 0]
        assert _same(low["h_u_cart"][k][src_k == 1], out["u_cart"][k])
        fitted = out["h_source"][k] >= 3
        assert bool(fitted.any()) == (k != 1)
        assert not bool((low["h_u_cart"][k][fitted] == out["h_u_cart"][k][fitted]).flatten(1).all(1).any())
        assert _same(low["h_u_cart"][k][~fitted], out["h_u_cart"][k][~fitted])


def test_the_flag_beside_temperatures_and_rotations(work, monkeypatch, capsys):
    import main as entry
    from cartnet_amd import predict as pr
    d, ckpt, src = work
    monkeypatch.chdir(d)
    calls = {"molecules": 0, "aniso_h": 0, "riding_h": 0}
    for name, key in (("find_molecules", "molecules"), ("aniso_h_call", "aniso_h"), ("riding_h_call", "riding_h")):
        def counted(*a, _f=getattr(pr, name), _k=key, **kw):
            calls[_k] += 1
            return _f(*a, **kw)
        monkeypatch.setattr(pr, name, counted)
    res = entry.main(["--predict", "--predict_input", src, "--checkpoint_path", ckpt, "--eval_batch", "2", "--riding_h",
                      "--rigid_molecule", "--tls_fit", "--aniso_h", "--predict_temperatures", "100:200:100", "--rotations", "2",
                      "--predict_output", "series.pkl"] + MODEL)
    out = _load("series.pkl")
    assert calls == {"molecules": 2, "aniso_h": 4, "riding_h": 4}             # two batches, two temperatures
    assert res["entries"] == 6 and res["crystals"] == 3 and out["name"][:2] == ["mixed_100K", "mixed_200K"]
    _check_entries(out, res, 6)
    assert (res["h_aniso"], res["h_aniso_tls"]) == (78, 56)
    for g in range(3):                                                        # the same sources, tensors of that temperature's U
        assert _same(out["h_source"][2 * g], out["h_source"][2 * g + 1])
        assert not _same(out["h_u_cart"][2 * g], out["h_u_cart"][2 * g + 1])


def test_a_cif_file_gets_a_tensor_per_atom_of_its_asymmetric_unit(work, monkeypatch, capsys):
    """P-1, the asymmetric unit a methanol molecule: six atoms in the file, twelve in the cell; four atoms per molecule
    with a row is below the TLS minimum, so every hydrogen is source 2."""
    import main as entry
    from cartnet_amd.cif import read_cif
    from cartnet_amd.predict import AH_KEYS, AH_SYM_KEYS
    d, ckpt, _ = work
    monkeypatch.chdir(d)
    cell = (8.1, 8.6, 9.2, 85.0, 95.0, 100.0)
    inv = np.linalg.inv(cu.cell_reference(*cell))
    atoms, sym = [], {1: "H", 6: "C", 8: "O"}
    for k, (z, pos, _, _) in enumerate(METHANOL):
        f = (np.array(pos) + np.array([2.0, 2.4, 1.9])) @ inv
        atoms.append((f"{sym[z]}{k + 1}", sym[z], float(f[0]), float(f[1]), float(f[2]),
                      None if z == 1 else (0.03, 0.03, 0.03, 0.0, 0.0, 0.0)))
    monkeypatch.setitem(cu.CRYSTALS, "aniso", dict(cell=cell, ops=cu.close_group([cu.INVERSION]), temp=120.0, atoms=atoms))
    os.makedirs("cif_in", exist_ok=True)
    with open(os.path.join("cif_in", "aniso.cif"), "w") as f:
        f.write(cu.cif_text("aniso", name="aniso", labeled=False))
    common = ["--predict", "--predict_input", os.path.join("cif_in", "aniso.cif"), "--checkpoint_path", ckpt, "--riding_h",
              "--rigid_molecule", "--tls_fit"] + MODEL
    plain = entry.main(common + ["--predict_output", "cif_plain.pkl"])
    res = entry.main(common + ["--predict_output", "cif_aniso.pkl", "--predict_cif_dir", "cif_out", "--aniso_h"])
    old, out = _load("cif_plain.pkl"), _load("cif_aniso.pkl")
    assert set(res) == set(plain) | AH_JSON and list(out) == list(old) + list(AH_KEYS) + list(AH_SYM_KEYS)
    for k in old:
        assert all(_same(p, q) for p, q in zip(old[k], out[k])), k
    _check_entries(out, res, 1, sources=([0, 4, 8, 0, 0],))
    z = [a[0] for a in METHANOL]
    asym = out["h_u_cif_asym"][0]
    assert asym.dtype == torch.float32 and tuple(asym.shape) == (6, 6) and not bool(torch.isnan(asym).any())
    site = np.cumsum(np.array(z) != 1) - 1
    for i, v in enumerate(z):                                                 # a site's orbit mean, or the listed hydrogen's own
        assert _same(asym[i], out["u_cif_asym"][0][site[i]] if v != 1 else out["h_u_cif"][0][i]), i
    (back,) = read_cif(os.path.join("cif_out", "aniso.cif"))
    (src,) = read_cif(os.path.join("cif_in", "aniso.cif"))
    assert back.labels == src.labels and len(back.symops) == len(src.symops) == 2      # the file's own setting
    assert back.adp_type == ["Uani"] * 6 and list(back.u_aniso) == back.labels
    assert np.abs(back.u_cif() - asym.double().numpy()).max() <= 0.5e-6 + 1e-12
    h = [i for i, v in enumerate(z) if v == 1]
    assert np.abs(np.array(back.u_iso)[h] - out["h_u_eq"][0][h].double().numpy()).max() <= 0.5e-6 + 1e-12


def test_without_the_flag_nothing_changes(work, monkeypatch, capsys):
    import main as entry
    d, ckpt, src = work
    monkeypatch.chdir(d)
    common = ["--predict", "--predict_input", src, "--checkpoint_path", ckpt, "--eval_batch", "2", "--riding_h",
              "--rigid_molecule", "--tls_fit"] + MODEL
    a = entry.main(common + ["--predict_output", "off_a.pkl", "--predict_cif_dir", "off_a"])
    b = entry.main(common + ["--predict_output", "off_b.pkl", "--predict_cif_dir", "off_b", "--aniso_h_stretch", "0.01",
                             "--aniso_h_bend", "0.03"])
    skip = ("output", "cif_dir")
    assert {k: v for k, v in a.items() if k not in skip} == {k: v for k, v in b.items() if k not in skip} and not set(a) & AH_JSON
    old, new = _load("off_a.pkl"), _load("off_b.pkl")
    assert list(old) == list(new) and not [k for k in new if k.startswith("h_u") or k in ("h_source", "h_aniso_stats")]
    for k in old:
        assert all(_same(p, q) for p, q in zip(old[k], new[k])), k
    for name in NAMES:
        with open(os.path.join("off_a", f"{name}.cif"), "rb") as f, open(os.path.join("off_b", f"{name}.cif"), "rb") as g:
            assert f.read() == g.read()
