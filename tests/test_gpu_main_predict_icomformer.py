"""``main.py --predict --model icomformer --model_frame reduced_cell`` end to end (without the new flag it exits as it
always did, and there was no flag to give): an unlabeled geometry-only shard file and a directory of two CIFs, one of them with a non-trivial operator;
the pickle, the JSON line with ``"model_frame": "reduced_cell"``, the CIFs of ``--predict_cif_dir`` read back with
``cartnet_amd.cif``, a temperature series, the analysis flags and ``--disable_H``."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

import cif_utils as cu
import model_frame_utils as mf

pytestmark = pytest.mark.gpu

CAP = "8"                                                                     # --max_neighbours: the cap bites on crystal 1
CIFS = ("a", "b")                                                             # P1 and P2_1/c
ANALYSIS_FLAGS = ["--rigid_bond", "--riding_h", "--rigid_molecule", "--tls_fit", "--aniso_h", "--bond_table", "--angle_table"]


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """(directory, checkpoint of the smallest iComformer, the model's flags, the shard file, the directory of CIFs)."""
    from cartnet_amd import shard
    from cartnet_amd.comformer import iComformer
    from cartnet_amd.data import Data
    root = tmp_path_factory.mktemp("icf_predict")
    dim, sd = mf.model_and_weights()
    model = iComformer(dim)
    model.load_state_dict(sd, strict=True)
    ckpt = str(root / "icf.ckpt")
    torch.save({"model_state": model.state_dict()}, ckpt)
    geometry = [Data(x=d.x, pos=d.pos, cell=d.cell, natoms=d.natoms, temperature=d.temperature) for d in mf.crystals(False)]
    src = str(root / "predict.cnshard")
    shard.write_shard(src, geometry, names=[f"m{g}" for g in range(4)])
    cifs = root / "cifs"
    cifs.mkdir()
    for k in CIFS:
        (cifs / f"{k}.cif").write_text(cu.cif_text(k, name=f"crystal_{k}", labeled=False))
    flags = ["--model", "icomformer", "--model_frame", "reduced_cell", "--dim_in", str(dim), "--max_neighbours", CAP]
    return root, ckpt, flags, src, str(cifs)


@pytest.fixture(autouse=True)
def _restore_cfg():
    yield
    from cartnet_amd.config import set_cfg
    set_cfg()


def _run(argv, capsys):
    import main as entry
    capsys.readouterr()
    res = entry.main(argv)
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line == res
    return res


def test_predict_a_shard_file(work, monkeypatch, capsys):
    from cartnet_amd import predict as p
    from cartnet_amd import shard
    from cartnet_amd.cif import read_cif
    from cartnet_amd.config import cfg
    from cartnet_amd.master import create_model
    from cartnet_amd.synthetic import TEMP_MEAN, TEMP_STD
    root, ckpt, model_flags, src, _ = work
    monkeypatch.chdir(root)
    base = ["--predict", "--predict_input", src, "--checkpoint_path", ckpt, "--eval_batch", "3"] + model_flags
    res = _run(base + ["--predict_output", "pred.pkl", "--predict_cif_dir", "out"], capsys)
    items = mf.crystals(False)
    rows = [int((d.x != 1).sum()) for d in items]
    assert res["model_frame"] == "reduced_cell" and list(res)[-1] == "model_frame"
    assert res["crystals"] == 4 and res["rows"] == sum(rows) and "rotations" not in res and "rejected" not in res
    with open("pred.pkl", "rb") as f:
        out = pickle.load(f)
    assert tuple(out) == p.KEYS + p.MF_KEYS and out["name"] == ["m0", "m1", "m2", "m3"]
    assert [int(t.shape[0]) for t in out["u_cart"]] == rows and all(bool(torch.isfinite(t).all()) for t in out["u_cart"])
    assert res["u_eq_mean"] == pytest.approx(torch.cat(out["u_eq"]).double().mean().item(), rel=1e-9)
    for g, d in enumerate(items):                                             # the stored cell, the stored temperature
        assert torch.equal(out["cell"][g], d.cell[0]) and out["temp"][g] == pytest.approx(float(d.temperature))
    # the pass main.py ran: the stored shard graphed with the cap, its reduced frame as the model's
    model = create_model()
    model.load_state_dict(torch.load(ckpt, map_location=cfg.device)["model_state"])
    stored = shard.DeviceShard.from_file(src, cfg.device).with_radius_graph(5.0, int(CAP))
    uncapped = shard.DeviceShard.from_file(src, cfg.device).with_radius_graph(5.0)
    assert int(stored.edge_ptr[-1]) < int(uncapped.edge_ptr[-1])
    want = p.predict_adps(model, shard.ShardLoader(stored, 3, temp_mean=TEMP_MEAN, temp_std=TEMP_STD), cfg.device,
                          model_frame=stored.with_optimized_cell())
    for k in ("u_cart", "u_cif", "cell_rotation", "cell_reduced", "frac"):
        for g in range(4):
            assert mf.bits(out[k][g]) == mf.bits(want[k][g]), (k, g)
    rot = torch.stack(out["cell_rotation"])
    assert float((rot[0] - torch.eye(3)).abs().max()) <= 1e-6 and float((rot[1] - torch.eye(3)).abs().max()) > 0.1
    # the CIFs: P1, the stored cell, the exported rows
    assert sorted(os.listdir("out")) == [f"m{g}.cif" for g in range(4)]
    for g, d in enumerate(items):
        (back,) = read_cif(os.path.join("out", f"m{g}.cif"))
        assert back.z == d.x.tolist() and len(back.symops) == 1
        heavy = [lab for lab, z in zip(back.labels, back.z) if z != 1]
        got = np.array([back.u_aniso[lab] for lab in heavy])
        assert np.abs(got - out["u_cif"][g].double().numpy()).max() <= 0.5e-6 + 1e-12       # the printed digits
        assert np.abs(np.array(back.frac) - out["frac"][g].double().numpy()).max() <= 0.5e-6 + 1e-12
    # every analysis flag, and --disable_H
    full = _run(base + ["--predict_output", "full.pkl"] + ANALYSIS_FLAGS, capsys)
    assert full["model_frame"] == "reduced_cell" and full["hydrogens"] == 6 and full["h_orphans"] == 0
    assert full["molecules"] > 0 and full["bonds_listed"] > 0 and full["angles_listed"] > 0
    with open("full.pkl", "rb") as f:
        fo = pickle.load(f)
    analyses = p.Analyses((0.4, 1e-3), (0.4, 1.2, 1.5), (0.4, 1e-3), True, (0.005, 0.020))
    assert tuple(fo) == p.result_keys(analyses, False, 1, 0.4, 0.4, True)
    for g in range(4):
        assert torch.equal(fo["u_cart"][g], out["u_cart"][g])
    bare = _run(base + ["--predict_output", "bare.pkl", "--disable_H"], capsys)
    assert bare["model_frame"] == "reduced_cell" and bare["rows"] == sum(rows)
    with open("bare.pkl", "rb") as f:
        bo = pickle.load(f)
    assert [int(t.shape[0]) for t in bo["z"]] == rows and all(bool(torch.isfinite(t).all()) for t in bo["u_cart"])
    # a temperature series: three entries per crystal and a series
    ser = _run(base + ["--predict_output", "series.pkl", "--predict_temperatures", "100,200,300", "--predict_cif_dir",
                       "series_out"], capsys)
    assert ser["model_frame"] == "reduced_cell" and ser["crystals"] == 4 and ser["entries"] == 12
    assert ser["temperatures"] == [100.0, 200.0, 300.0]
    with open("series.pkl", "rb") as f:
        so = pickle.load(f)
    assert len(so["name"]) == 12 and so["name"][3:6] == ["m1_100K", "m1_200K", "m1_300K"] and so["temp"][:3] == [100.0, 200.0, 300.0]
    assert so["series"]["name"] == ["m0", "m1", "m2", "m3"] and [int(t.shape[0]) for t in so["series"]["t_slope"]] == rows
    assert len(os.listdir("series_out")) == 12
    # the refusals
    with pytest.raises(SystemExit, match="--predict --model icomformer serves one frame only"):
        _run(base + ["--rotations", "2"], capsys)
    with pytest.raises(SystemExit, match="--predict does not serve --model icomformer in the stored frame"):
        _run([a for a in base if a not in ("--model_frame", "reduced_cell")], capsys)


def test_predict_a_directory_of_cifs(work, monkeypatch, capsys):
    from cartnet_amd.cif import read_cif
    root, ckpt, model_flags, _, cifs = work
    monkeypatch.chdir(root)
    res = _run(["--predict", "--predict_input", cifs, "--checkpoint_path", ckpt, "--predict_output", "cif.pkl",
                "--predict_cif_dir", "cif_out", "--eval_batch", "2", "--riding_h"] + model_flags, capsys)
    assert res["model_frame"] == "reduced_cell" and res["crystals"] == 2 and res["rejected"] == 0
    assert res["rows"] == sum(cu.ATOMS[k][1] for k in CIFS)
    with open("cif.pkl", "rb") as f:
        out = pickle.load(f)
    assert out["name"] == [f"crystal_{k}" for k in CIFS] and "cell_rotation" in out and "u_cif_asym" in out
    assert [int(t.shape[0]) for t in out["u_cart"]] == [cu.ATOMS[k][1] for k in CIFS]
    assert sorted(os.listdir("cif_out")) == sorted(f"crystal_{k}.cif" for k in CIFS)
    for i, k in enumerate(CIFS):
        (src,) = read_cif(cu.cif_text(k))
        (back,) = read_cif(os.path.join("cif_out", f"crystal_{k}.cif"))
        heavy = [lab for lab, z in zip(src.labels, src.z) if z != 1]
        assert back.labels == src.labels == out["asym_labels"][i] and back.z == src.z
        assert len(back.symops) == len(src.symops) == len(out["symops"][i])   # the file's operators, the file's setting
        for (W1, w1), (W2, w2) in zip(back.symops, src.symops):
            assert np.array_equal(W1, W2) and np.array_equal(w1, w2)
        assert np.abs(np.array(back.frac) - np.array(src.frac)).max() <= 1e-6
        u, spread = out["u_cif_asym"][i], out["spread"][i]
        assert tuple(u.shape) == (len(heavy), 6) and bool(torch.isfinite(u).all()) and bool((spread >= 0).all())
        got = np.array([back.u_aniso[lab] for lab in heavy])
        assert np.abs(got - u.double().numpy()).max() <= 0.5e-6 + 1e-12      # the same u_cif, to the printed digits
        # the stored cell is the file's, whatever frame the model read
        want = cu.cell_reference(*cu.CRYSTALS[k]["cell"])
        assert np.abs(out["cell"][i].double().numpy() - want).max() <= 1e-5 * np.abs(want).max()
    # P1: nothing to average over, so the site's ADP is the row's; P2_1/c: four images per site
    assert torch.allclose(out["u_cif_asym"][0], out["u_cif"][0], rtol=0, atol=2.0 ** -22 * float(out["u_cif"][0].abs().max()))
    assert float(out["spread"][0].max()) == 0.0
    assert len(out["symops"][1]) == 4 and int(out["u_cart"][1].shape[0]) > int(out["u_cif_asym"][1].shape[0])
    assert float(out["spread"][1].max()) > 0.0
