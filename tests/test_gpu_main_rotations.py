"""``main.py --rotations K`` end to end: train one epoch, then ``--predict`` an unlabeled shard in three frames (JSON line,
pickle, CIFs), ``--inference`` in two frames at ``--eval_batch 1`` (the batched path, host loader and resident shard), and
``--rotations 1`` against the flag's absence."""
import importlib.util
import json
import math
import os
import pickle

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL = ["--dim_in", "32", "--num_layers", "2"]
DATA = ["--synthetic", "24", "--atoms", "10", "30"]


def _make_shards():
    spec = importlib.util.spec_from_file_location("make_shards", os.path.join(ROOT, "tools", "make_shards.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """One epoch on synthetic crystals in a directory of its own: (directory, checkpoint, the unlabeled shard)."""
    import main as entry
    work = tmp_path_factory.mktemp("rotations")
    old = os.getcwd()
    os.chdir(work)
    try:
        entry.main(DATA + ["--epochs", "1", "--batch", "4", "--batch_accumulation", "1", "--name", "r"] + MODEL)
        _make_shards().main([str(work / "shards")] + DATA + ["--unlabeled"])
    finally:
        os.chdir(old)
    ckpt = str(work / "results" / "r" / "0" / "ckpt" / "best.ckpt")
    assert os.path.exists(ckpt)
    yield work, ckpt, str(work / "shards" / "predict.cnshard")
    from cartnet_amd.config import set_cfg
    set_cfg()


def _load(path):
    with open(path, "rb") as f:
        return pickle.load(f)


def test_predict_in_three_frames(trained, monkeypatch, capsys):
    import main as entry
    from cartnet_amd import shard
    work, ckpt, src = trained
    monkeypatch.chdir(work)
    arrays = shard.read_shard(src)
    names, rows = shard.read_shard_meta(src)["names"], [int(r) for r in (arrays["y_ptr"][1:] - arrays["y_ptr"][:-1])]
    capsys.readouterr()
    res = entry.main(["--predict", "--predict_input", src, "--checkpoint_path", ckpt, "--predict_output", "rot.pkl",
                      "--predict_cif_dir", "rot_cifs", "--eval_batch", "2", "--rotations", "3"] + MODEL)
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line == res and line["rotations"] == 3 and line["crystals"] == len(names) and line["rows"] == sum(rows)
    assert math.isfinite(line["rot_spread_max"]) and math.isfinite(line["rot_spread_mean"])
    assert line["rot_spread_max"] >= line["rot_spread_mean"] >= 0
    out = _load("rot.pkl")
    assert out["name"] == names
    assert [tuple(t.shape) for t in out["rot_spread"]] == [(r,) for r in rows]           # one value per ADP row
    assert all(tuple(f.shape) == (3, 3, 3) and torch.equal(f[0], torch.eye(3)) for f in out["frames"])
    spread = torch.cat(out["rot_spread"]).double()
    assert line["rot_spread_max"] == spread.max().item()
    assert line["rot_spread_mean"] == pytest.approx(spread.mean().item(), rel=1e-9)
    assert [int(t.shape[0]) for t in out["u_cif"]] == rows
    assert sorted(os.listdir("rot_cifs")) == sorted(n + ".cif" for n in names)


def test_no_flag_is_rotations_one(trained, monkeypatch, capsys):
    import main as entry
    work, ckpt, src = trained
    monkeypatch.chdir(work)
    common = ["--predict", "--predict_input", src, "--checkpoint_path", ckpt, "--eval_batch", "2"] + MODEL
    a = entry.main(common + ["--predict_output", "plain.pkl"])
    b = entry.main(common + ["--predict_output", "one.pkl", "--rotations", "1"])
    assert "rotations" not in a and "rotations" not in b
    assert {k: v for k, v in a.items() if k != "output"} == {k: v for k, v in b.items() if k != "output"}
    x, y = _load("plain.pkl"), _load("one.pkl")
    assert list(x) == list(y) and "rot_spread" not in x
    for k in x:
        assert len(x[k]) == len(y[k])
        for p, q in zip(x[k], y[k]):
            assert torch.equal(p, q) if torch.is_tensor(p) else (p == q or (p != p and q != q)), k


@pytest.mark.parametrize("extra", [[], ["--resident_dataset"]])
def test_inference_in_two_frames_takes_the_batched_path(trained, monkeypatch, capsys, extra):
    import main as entry
    from cartnet_amd import evaluate
    work, ckpt, _ = trained
    monkeypatch.chdir(work)
    common = DATA + ["--inference", "--checkpoint_path", ckpt, "--eval_batch", "1"] + MODEL + extra
    plain = entry.main(common + ["--inference_output", "inf_plain.pkl"])
    calls = []
    one_loop = evaluate.inference                                             # there is no other pass to take

    def spy(*a, **k):
        calls.append(k)
        return one_loop(*a, **k)
    monkeypatch.setattr(evaluate, "inference", spy)
    capsys.readouterr()
    res = entry.main(common + ["--inference_output", "inf_rot.pkl", "--rotations", "2", "--seed", "4"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line == res and calls == [{"rotations": 2, "seed": 4, "rigid_bond": None}]
    assert set(res) == set(plain) | {"rotations", "rot_spread_max"} and res["rotations"] == 2
    assert all(math.isfinite(v) for k, v in res.items() if k != "output") and res["rot_spread_max"] >= 0
    out, ref = _load("inf_rot.pkl"), _load("inf_plain.pkl")
    assert set(out) == set(ref) | {"rot_spread"}
    n = len(ref["pred"])
    assert n == 3                                                             # 24 crystals split 19 / 2 / 3
    for k in ("pred", "true", "iou", "mae", "similarity_index", "atoms", "cell", "rot_spread"):
        assert len(out[k]) == n, k
    for c in range(n):
        assert out["pred"][c].shape == ref["pred"][c].shape and torch.equal(out["true"][c], ref["true"][c])
        assert tuple(out["rot_spread"][c].shape) == (int(ref["pred"][c].shape[0]),)
        assert torch.equal(out["atoms"][c], ref["atoms"][c])
        assert torch.equal(out["mae"][c], (out["pred"][c] - out["true"][c]).abs())      # evaluated on the mean
    assert res["rot_spread_max"] == float(torch.cat(out["rot_spread"]).max())
