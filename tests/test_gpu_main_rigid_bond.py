"""``main.py --rigid_bond`` end to end on the six crystals of ``predict_utils`` with a small CartNet whose checkpoint the
test saves: ``--predict`` (also in two frames) and ``--inference`` carry the rigid-bond figures of a direct
``metrics.bond_test`` call per crystal, bit for bit, and leave everything else as it is; without the flag nothing changes."""
import json
import math
import os
import pickle

import numpy as np
import pytest
import torch

import predict_utils as pu

pytestmark = pytest.mark.gpu

MODEL = ["--dim_in", "64", "--num_layers", "2"]
TOL, THRESHOLD = 0.4, 1e-3
PREDICT_JSON = {"crystals", "rows", "u_eq_mean", "non_positive_rows", "output", "cif_dir"}
INFERENCE_JSON = {"iou_mean", "iou_std", "mae_mean", "mae_std", "similarity_index_mean", "similarity_index_std", "output"}
INFERENCE_PICKLE = {"pred", "true", "temp", "cell", "refcode", "pos", "atoms", "iou", "mae", "similarity_index"}


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """(directory, checkpoint of a fresh small CartNet, the unlabeled shard, a --shard_dir whose splits are the six)."""
    import main as entry
    from cartnet_amd import shard
    from cartnet_amd.config import set_cfg
    from cartnet_amd.master import create_model
    d = tmp_path_factory.mktemp("rigid_bond")
    entry.fill_cfg(entry.build_parser().parse_args(MODEL))
    torch.manual_seed(0)
    ckpt = str(d / "fresh.ckpt")
    torch.save({"model_state": create_model().state_dict()}, ckpt)
    src = str(d / "six.cnshard")
    shard.write_shard(src, pu.six_crystals(False), names=[f"c{g}" for g, _, _ in pu.SIX])
    os.makedirs(d / "splits")
    for part in ("train", "val", "test"):
        shard.write_shard(str(d / "splits" / f"{part}.cnshard"), pu.six_crystals(True))
    yield d, ckpt, src, str(d / "splits")
    set_cfg()


def _load(path):
    with open(path, "rb") as f:
        return pickle.load(f)


def _same(p, q) -> bool:
    if torch.is_tensor(p):
        return p.dtype == q.dtype and p.shape == q.shape and p.numpy().tobytes() == q.numpy().tobytes()
    return p == q or (p != p and q != q)


def _graphed(path):
    """The shard of ``path`` as main.py's recipe leaves it (cfg is the one of the run before)."""
    import main as entry
    from cartnet_amd.shard import DeviceShard
    (s,), _ = entry.shard_recipe([DeviceShard.from_file(path, "cuda:0")])
    return s


def _shard_bonds(s) -> int:
    """Directed bonds of a graphed shard by the rule in numpy fp32: the reference side's count."""
    from cartnet_amd.bonds import is_bond
    z, src, tgt = (s.t[k].cpu().numpy().astype(np.int64) for k in ("z", "edge_src", "edge_tgt"))
    dist, n = s.t["cart_dist"].cpu().numpy(), 0
    for g in range(s.num_graphs):
        e, zg = slice(s.edge_ptr[g], s.edge_ptr[g + 1]), z[s.atom_ptr[g]:s.atom_ptr[g + 1]]
        n += int(is_bond(dist[e], zg[tgt[e]], zg[src[e]], TOL, same_atom=src[e] == tgt[e]).sum())
    return n


def _direct(s, k, u):
    """``bond_test`` on crystal k alone: its own batch, its own graph."""
    from cartnet_amd.metrics import bond_test, target_row_ptr
    b = s.collate([k])
    return bond_test(u.cuda(), b, target_row_ptr(b), TOL, THRESHOLD)


@pytest.mark.parametrize("rotations", [1, 2])
def test_predict_carries_the_direct_result_and_changes_nothing_else(work, monkeypatch, capsys, rotations):
    import main as entry
    from cartnet_amd.predict import BOND_KEYS, KEYS, ROT_KEYS
    d, ckpt, src, _ = work
    monkeypatch.chdir(d)
    common = ["--predict", "--predict_input", src, "--checkpoint_path", ckpt, "--eval_batch", "4"] + MODEL
    common += ["--rotations", str(rotations)] if rotations > 1 else []
    plain = entry.main(common + ["--predict_output", "plain.pkl"])
    capsys.readouterr()
    res = entry.main(common + ["--predict_output", "bond.pkl", "--rigid_bond"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line == res
    assert set(res) == set(plain) | {"bonds", "rigid_bond_mean", "rigid_bond_max", "rigid_bond_over"}
    assert {k: v for k, v in res.items() if k in plain and k != "output"} == {k: v for k, v in plain.items() if k != "output"}
    old, out = _load("plain.pkl"), _load("bond.pkl")
    assert set(old) == set(KEYS) | (set(ROT_KEYS) if rotations > 1 else set())
    assert list(out) == list(old) + list(BOND_KEYS)
    for k in old:                                                             # u_cart, u_cif and every old key: the same bits
        assert len(old[k]) == len(out[k]) == 6 and all(_same(p, q) for p, q in zip(old[k], out[k])), k
    s = _graphed(src)
    assert _shard_bonds(s) >= 1                                               # the shard has bonds to test
    counts = pu.non_h_counts()
    for k in range(6):
        bt = _direct(s, k, out["u_cart"][k])
        n = bt.bonds.cpu()
        assert tuple(n.shape) == (counts[k],)
        want = {"bond_count": n, "bond_delta_max": bt.delta_max.cpu(), "bond_worst": bt.worst.cpu(),
                "bond_over": bt.over.cpu(), "bond_ueq_ratio": bt.ueq_ratio.cpu(), "bond_stats": bt.crystal_stats[0].cpu(),
                "bond_delta_mean": torch.where(n > 0, bt.delta_sum.cpu() / n.clamp(min=1).float(), torch.zeros(len(n)))}
        for key, t in want.items():
            assert _same(out[key][k], t), (key, k)
        assert out["bond_stats"][k].dtype == torch.float64 and out["bond_worst"][k].dtype == torch.int64
        assert bool(((out["bond_worst"][k] >= 0) == (n > 0)).all()) and int(out["bond_worst"][k].max()) < len(out["z"][k])
    stats = torch.stack(out["bond_stats"])
    assert res["bonds"] == int(torch.cat(out["bond_count"]).sum()) == _shard_bonds(s) > 0
    assert res["rigid_bond_over"] == int(torch.cat(out["bond_over"]).sum())
    assert res["rigid_bond_max"] == float(torch.cat(out["bond_delta_max"]).max())
    assert res["rigid_bond_mean"] == pytest.approx(float(stats[:, 1].sum()) / res["bonds"], rel=1e-12)
    assert math.isfinite(res["rigid_bond_mean"]) and 0 < res["rigid_bond_mean"] <= res["rigid_bond_max"]


@pytest.mark.parametrize("eval_batch", [1, 4])
def test_inference_tests_prediction_and_truth_on_the_batched_path(work, monkeypatch, capsys, eval_batch):
    import main as entry
    from cartnet_amd import evaluate
    d, ckpt, _, splits = work
    monkeypatch.chdir(d)
    common = ["--inference", "--shard_dir", splits, "--checkpoint_path", ckpt, "--eval_batch", str(eval_batch)] + MODEL
    plain = entry.main(common + ["--inference_output", "inf_plain.pkl"])
    calls = []
    one_loop = evaluate.inference                                             # there is no other pass to take

    def spy(*a, **k):
        calls.append(k)
        return one_loop(*a, **k)
    monkeypatch.setattr(evaluate, "inference", spy)
    capsys.readouterr()
    res = entry.main(common + ["--inference_output", "inf_bond.pkl", "--rigid_bond"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert calls == [{"rotations": 1, "seed": 0, "rigid_bond": (TOL, THRESHOLD)}]
    assert line == res and set(res) == set(plain) | {"rigid_bond_mean", "rigid_bond_mean_true"}
    old, out = _load("inf_plain.pkl"), _load("inf_bond.pkl")
    assert set(out) == set(old) | {"bond_delta_max", "bond_delta_max_true"}
    for k in ("true", "atoms", "cell"):
        assert all(_same(p, q) for p, q in zip(old[k], out[k])), k
    s = _graphed(os.path.join(splits, "test.cnshard"))
    assert _shard_bonds(s) >= 1
    sums = {"bond_delta_max": [0.0, 0.0], "bond_delta_max_true": [0.0, 0.0]}
    for k in range(6):
        for key, u in (("bond_delta_max", out["pred"][k]), ("bond_delta_max_true", out["true"][k])):
            bt = _direct(s, k, u)
            assert _same(out[key][k], bt.delta_max.cpu()), (key, k)
            sums[key][0] += float(bt.crystal_stats[0, 0])
            sums[key][1] += float(bt.crystal_stats[0, 1])
    assert torch.equal(torch.cat(out["true"]), torch.cat([c.y for c in pu.six_crystals(True)]))     # the truth is y
    assert sums["bond_delta_max"][0] == sums["bond_delta_max_true"][0] == _shard_bonds(s)
    assert res["rigid_bond_mean"] == pytest.approx(sums["bond_delta_max"][1] / sums["bond_delta_max"][0], rel=1e-12)
    assert res["rigid_bond_mean_true"] == pytest.approx(sums["bond_delta_max_true"][1] / sums["bond_delta_max_true"][0],
                                                        rel=1e-12)
    assert res["rigid_bond_mean"] > 0 and res["rigid_bond_mean_true"] > 0


def test_without_the_flag_everything_is_as_it_was(work, monkeypatch, capsys):
    """The two figures alone switch nothing on: the key sets of both passes are the ones they have always had."""
    import main as entry
    from cartnet_amd import evaluate
    from cartnet_amd.predict import KEYS
    d, ckpt, src, splits = work
    monkeypatch.chdir(d)
    quiet = ["--bond_tolerance", "0.3", "--rigid_bond_threshold", "5e-4"]
    res = entry.main(["--predict", "--predict_input", src, "--checkpoint_path", ckpt, "--eval_batch", "4",
                      "--predict_output", "quiet.pkl"] + MODEL + quiet)
    assert set(res) == PREDICT_JSON and tuple(_load("quiet.pkl")) == KEYS
    calls = []
    one_loop = evaluate.inference

    def spy(*a, **k):
        calls.append(k)
        return one_loop(*a, **k)
    monkeypatch.setattr(evaluate, "inference", spy)
    res = entry.main(["--inference", "--shard_dir", splits, "--checkpoint_path", ckpt, "--eval_batch", "4",
                      "--inference_output", "inf_quiet.pkl"] + MODEL + quiet)
    assert calls == [{"rotations": 1, "seed": 0, "rigid_bond": None}]         # every option at its default: nothing switched on
    assert set(res) == INFERENCE_JSON and set(_load("inf_quiet.pkl")) == INFERENCE_PICKLE
