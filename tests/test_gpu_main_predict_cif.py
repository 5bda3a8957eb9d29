"""CIF files end to end: ``main.py --predict`` on a directory of CIFs (expanded in memory, one site-averaged ADP per
atom of the asymmetric unit, written back in the file's own setting), and ``tools/cif_to_shard.py`` shards for
``--shard_dir`` training and for ``--predict``."""
import importlib.util
import json
import os
import pickle

import numpy as np
import pytest
import torch

import cif_utils as cu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL = ["--dim_in", "32", "--num_layers", "2"]
KEYS = ("a", "b", "c", "d")


def _tool():
    spec = importlib.util.spec_from_file_location("cif_to_shard", os.path.join(ROOT, "tools", "cif_to_shard.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """One epoch on synthetic crystals, in a directory of its own: (directory, checkpoint, the directory of CIFs)."""
    import main as entry
    work = tmp_path_factory.mktemp("cif")
    old = os.getcwd()
    os.chdir(work)
    try:
        entry.main(["--synthetic", "24", "--atoms", "10", "30", "--epochs", "1", "--batch", "4", "--batch_accumulation", "1",
                    "--name", "c"] + MODEL)
    finally:
        os.chdir(old)
    ckpt = str(work / "results" / "c" / "0" / "ckpt" / "best.ckpt")
    assert os.path.exists(ckpt)
    cifs = work / "cifs"
    cifs.mkdir()
    for k in KEYS:
        (cifs / f"{k}.cif").write_text(cu.cif_text(k, name=f"crystal_{k}", labeled=False))
    (cifs / "z_disordered.cif").write_text(cu.BAD["disordered"])
    return work, ckpt, str(cifs)


def test_predict_a_directory_of_cifs(trained, monkeypatch, capsys):
    import main as entry
    from cartnet_amd.cif import read_cif
    work, ckpt, cifs = trained
    monkeypatch.chdir(work)
    capsys.readouterr()
    res = entry.main(["--predict", "--predict_input", cifs, "--checkpoint_path", ckpt, "--predict_output", "pred.pkl",
                      "--predict_cif_dir", "out", "--eval_batch", "2"] + MODEL)
    cap = capsys.readouterr()
    line = json.loads(cap.out.strip().splitlines()[-1])
    assert line == res and res["crystals"] == len(KEYS) and res["rejected"] == 1
    assert "rejected\tdisordered\tdisorder" in cap.err
    assert res["rows"] == sum(cu.ATOMS[k][1] for k in KEYS)             # the expanded non-hydrogen atoms
    with open("pred.pkl", "rb") as f:
        out = pickle.load(f)
    assert out["name"] == [f"crystal_{k}" for k in KEYS]
    assert [int(t.shape[0]) for t in out["u_cart"]] == [cu.ATOMS[k][1] for k in KEYS]
    assert [int(t.shape[0]) for t in out["z"]] == [cu.ATOMS[k][0] for k in KEYS]
    assert all(bool(torch.isfinite(p).all()) for p in out["principal"])
    assert sorted(os.listdir("out")) == sorted(f"crystal_{k}.cif" for k in KEYS)
    for i, k in enumerate(KEYS):
        (src,) = read_cif(cu.cif_text(k))
        (back,) = read_cif(os.path.join("out", f"crystal_{k}.cif"))
        heavy = [lab for lab, z in zip(src.labels, src.z) if z != 1]
        assert back.labels == src.labels == out["asym_labels"][i] and back.z == src.z
        assert len(back.symops) == len(src.symops) == len(out["symops"][i])
        for (W1, w1), (W2, w2) in zip(back.symops, src.symops):
            assert np.array_equal(W1, W2) and np.array_equal(w1, w2)
        assert np.abs(np.array(back.frac) - np.array(src.frac)).max() <= 1e-6
        assert np.array_equal(out["asym_frac"][i].numpy(), np.array(src.frac))
        assert sorted(back.u_aniso) == sorted(heavy) and back.reject_reason(True) is None
        u, spread = out["u_cif_asym"][i], out["spread"][i]
        assert tuple(u.shape) == (len(heavy), 6) and tuple(spread.shape) == (len(heavy),)
        assert bool(torch.isfinite(u).all()) and bool((spread >= 0).all())
        got = np.array([back.u_aniso[lab] for lab in heavy])
        assert np.abs(got - u.double().numpy()).max() <= 0.5e-6 + 1e-12  # the printed digits
    # P1: nothing to average over, so the site's ADP is the row's
    assert torch.allclose(out["u_cif_asym"][0], out["u_cif"][0], rtol=0, atol=2.0 ** -22 * float(out["u_cif"][0].abs().max()))
    assert float(out["spread"][0].max()) == 0.0
    # one CIF file as the input; a default temperature lets a crystal without one through
    bare = work / "bare.cif"
    bare.write_text(cu.BAD["no_temperature"])
    with pytest.raises(SystemExit, match="no usable crystal"):
        entry.main(["--predict", "--predict_input", str(bare), "--checkpoint_path", ckpt] + MODEL)
    one = entry.main(["--predict", "--predict_input", str(bare), "--predict_temperature", "150", "--checkpoint_path", ckpt,
                      "--predict_output", "one.pkl"] + MODEL)
    assert one["crystals"] == 1 and one["rows"] == 1 and one["rejected"] == 0
    with open("one.pkl", "rb") as f:
        assert pickle.load(f)["temp"] == [150.0]


def test_a_tool_written_shard_predicts_what_the_cifs_predict(trained, monkeypatch, capsys):
    import main as entry
    from cartnet_amd import shard
    work, ckpt, cifs = trained
    monkeypatch.chdir(work)
    res = _tool().main(["shards/predict.cnshard", cifs, "--unlabeled"])
    assert res["crystals"] == len(KEYS) and res["rejected"] == 1 and res["rows"] == sum(cu.ATOMS[k][1] for k in KEYS)
    assert open("shards/predict.rejected.txt").read() == "disordered\tdisorder\n"
    meta, arrays = shard.read_shard_meta("shards/predict.cnshard"), shard.read_shard("shards/predict.cnshard")
    assert meta["targets"] is False and meta["names"] == [f"crystal_{k}" for k in KEYS]
    assert "y" not in arrays and "edge_ptr" not in arrays and "graph" not in meta
    assert arrays["temperature"].tolist() == [cu.CRYSTALS[k]["temp"] for k in KEYS]
    entry.main(["--predict", "--predict_input", "shards/predict.cnshard", "--checkpoint_path", ckpt, "--predict_output",
                "from_shard.pkl", "--eval_batch", "2"] + MODEL)
    direct = entry.main(["--predict", "--predict_input", cifs, "--checkpoint_path", ckpt, "--predict_output",
                         "from_cifs.pkl", "--eval_batch", "2"] + MODEL)
    with open("from_shard.pkl", "rb") as f:
        a = pickle.load(f)
    with open("from_cifs.pkl", "rb") as f:
        b = pickle.load(f)
    assert "u_cif_asym" not in a and "rejected" in direct               # a shard takes the path it always took
    assert a["name"] == b["name"]
    for x, y in zip(a["u_cart"], b["u_cart"]):
        assert torch.equal(x, y)
    # with --radius the tool stores the graph and its provenance
    res = _tool().main(["shards/graphed.cnshard", cifs, "--unlabeled", "--radius", "4.0"])
    meta, arrays = shard.read_shard_meta("shards/graphed.cnshard"), shard.read_shard("shards/graphed.cnshard")
    assert meta["graph"] == {"radius": 4.0, "max_neighbors": None} and arrays["edge_ptr"][-1] == arrays["edge_src"].shape[0] > 0
    assert float(arrays["cart_dist"].max()) <= 4.0


def test_labeled_shards_from_cifs_train_under_shard_dir(trained, monkeypatch, capsys):
    import main as entry
    from cartnet_amd import shard
    work, _, _ = trained
    monkeypatch.chdir(work)
    src = work / "labeled"
    src.mkdir()
    (src / "train.cif").write_text(cu.batch_text())
    (src / "val.cif").write_text(cu.cif_text("a") + cu.cif_text("b"))
    (src / "test.cif").write_text(cu.cif_text("c") + cu.cif_text("e") + cu.BAD["isotropic_carbon"])
    for part in ("train", "val", "test"):
        res = _tool().main([f"set/{part}.cnshard", str(src / f"{part}.cif")])
        assert res["rejected"] == (1 if part == "test" else 0)
    assert "isotropic_carbon\tnon-hydrogen atom C2" in open("set/test.rejected.txt").read()
    arrays = shard.read_shard("set/train.cnshard")
    assert arrays["y"].shape == (sum(cu.ATOMS[k][1] for k in cu.BATCH), 9)
    capsys.readouterr()
    res = entry.main(["--shard_dir", "set", "--epochs", "1", "--batch", "4", "--batch_accumulation", "1", "--name", "fromcif"]
                     + MODEL)
    assert len(res["history"]) == 1 and np.isfinite(res["history"][0]["train_mae"]) and np.isfinite(res["test_mae"])
    assert res["test_metrics"]["mae"] > 0
