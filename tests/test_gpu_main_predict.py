"""``main.py --predict`` end to end: train one epoch, then predict the ADPs of the crystals of an unlabeled geometry-only
shard written by tools/make_shards.py --unlabeled, with one CIF per crystal."""
import importlib.util
import json
import os
import pickle
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL = ["--dim_in", "32", "--num_layers", "2"]


def _make_shards():
    spec = importlib.util.spec_from_file_location("make_shards", os.path.join(ROOT, "tools", "make_shards.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_train_then_predict_an_unlabeled_shard(tmp_path, monkeypatch, capsys):
    import main as entry
    from cartnet_amd import shard
    monkeypatch.chdir(tmp_path)
    entry.main(["--synthetic", "24", "--atoms", "10", "30", "--epochs", "1", "--batch", "4", "--batch_accumulation", "1",
                "--name", "p"] + MODEL)
    ckpt = os.path.join("results", "p", "0", "ckpt", "best.ckpt")
    assert os.path.exists(ckpt)
    _make_shards().main([str(tmp_path / "shards"), "--synthetic", "24", "--atoms", "10", "30", "--unlabeled"])
    src = str(tmp_path / "shards" / "predict.cnshard")
    meta, arrays = shard.read_shard_meta(src), shard.read_shard(src)
    assert meta["targets"] is False and "y" not in arrays and "edge_ptr" not in arrays
    names, rows = meta["names"], [int(r) for r in (arrays["y_ptr"][1:] - arrays["y_ptr"][:-1])]
    assert len(names) == 3                                                    # 24 crystals split 19 / 2 / 3
    assert all(re.fullmatch(r"syn\d+", n) for n in names)
    capsys.readouterr()
    res = entry.main(["--predict", "--predict_input", src, "--checkpoint_path", ckpt, "--predict_output", "pred.pkl",
                      "--predict_cif_dir", "cifs", "--eval_batch", "2"] + MODEL)
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line == res and line["crystals"] == len(names) and line["rows"] == sum(rows) and line["non_positive_rows"] == 0
    with open("pred.pkl", "rb") as f:
        out = pickle.load(f)
    assert out["name"] == names and [int(t.shape[0]) for t in out["u_cif"]] == rows
    assert all(bool((p > 0).all()) for p in out["principal"])
    assert line["u_eq_mean"] == pytest.approx(torch.cat(out["u_eq"]).double().mean().item(), rel=1e-9)
    assert all(80.0 < t < 310.0 for t in out["temp"])                         # Kelvin, as stored
    assert sorted(os.listdir("cifs")) == sorted(n + ".cif" for n in names)
    text = open(os.path.join("cifs", names[0] + ".cif")).read()
    assert len(re.findall(r"^[A-Z][a-z]?\d+ [A-Z][a-z]? ", text, flags=re.M)) == int(arrays["atom_ptr"][1])
    assert len(re.findall(r"^[A-Z][a-z]?\d+( -?\d+\.\d+){6}$", text, flags=re.M)) == rows[0]
    # a labeled shard is accepted too; its y is ignored
    lab = entry.main(["--predict", "--predict_input", str(tmp_path / "shards" / "test.cnshard"), "--checkpoint_path", ckpt,
                      "--predict_output", "pred_labeled.pkl", "--eval_batch", "2"] + MODEL)
    assert lab["crystals"] == len(names) and lab["rows"] == sum(rows)


def test_icomformer_is_refused_before_the_device_is_touched(monkeypatch):
    import main as entry

    def touched(*a, **k):
        raise AssertionError("--predict --model icomformer went on past its argument check")
    monkeypatch.setattr(entry.cdist, "init_from_env", touched)
    monkeypatch.setattr(entry, "create_model", touched)
    with pytest.raises(SystemExit, match="--predict does not serve --model icomformer"):
        entry.main(["--predict", "--model", "icomformer", "--predict_input", "x.cnshard", "--checkpoint_path", "x.ckpt"])
    from cartnet_amd.config import set_cfg
    set_cfg()
