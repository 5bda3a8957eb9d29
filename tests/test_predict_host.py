"""Prediction on the host: unlabeled shards and names in the shard file, the CIF writer, the new flags and the new entry
point's declaration (no GPU)."""
import math
import os
import re

import numpy as np
import pytest
import torch

import predict_utils as pu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_unlabeled_shard_packs_writes_and_reads(tmp_path):
    from cartnet_amd import shard
    lab, unl = pu.six_crystals(True), pu.six_crystals(False)
    a, b = shard.pack(lab), shard.pack(unl)
    counts = pu.non_h_counts()
    assert counts[0] == 1 and counts[3] == pu.SIX[3][1]                      # the single non-H atom; the H-free crystal
    assert "y" not in b and b["y_ptr"].tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
    assert b["y_ptr"].dtype == np.int64 and b["non_h_mask"].dtype == np.uint8
    assert np.array_equal(b["non_h_mask"], (b["z"] != 1).astype(np.uint8))   # derived: these crystals carry no mask
    for k in b:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k    # everything but y is the labeled shard's
    assert set(a) - set(b) == {"y"} and a["y"].shape == (sum(counts), 9)
    names = [f"n{g}" for g in range(6)]
    path = str(tmp_path / "u.cnshard")
    shard.write_shard(path, unl, names=names)
    meta, back = shard.read_shard_meta(path), shard.read_shard(path)
    assert meta["targets"] is False and meta["names"] == names and meta["graphs"] == 6 and "y" not in back
    for k in b:
        assert np.array_equal(back[k], b[k]), k
    with pytest.raises(ValueError, match="with and without y"):
        shard.pack(lab[:2] + unl[2:])
    with pytest.raises(ValueError, match="5 names"):
        shard.write_shard(path, unl, names=names[:5])


def test_a_labeled_shard_is_written_as_before(tmp_path):
    """Key by key against ``pack()`` of the same crystals; the header gains nothing unless names are given."""
    from cartnet_amd import shard
    from cartnet_amd.synthetic import make_crystal
    items = [make_crystal(g, n) for g, n in ((0, 6), (1, 9))]
    packed = shard.pack(items)
    assert list(packed) == ["atom_ptr", "edge_ptr", "y_ptr", "z", "edge_src", "edge_tgt", "cart_dist", "cart_dir", "y", "pos",
                            "non_h_mask", "cell", "temperature"]
    assert packed["y_ptr"].tolist() == [0] + np.cumsum([int(d.non_H_mask.sum()) for d in items]).tolist()
    p1, p2 = str(tmp_path / "a.cnshard"), str(tmp_path / "b.cnshard")
    shard.write_shard(p1, items, graph={"radius": 5.0, "max_neighbors": None})
    meta, back = shard.read_shard_meta(p1), shard.read_shard(p1)
    assert sorted(meta) == ["arrays", "graph", "graphs"] and list(back) == list(packed)
    for k, v in packed.items():
        assert back[k].dtype == v.dtype and np.array_equal(back[k], v), k
    shard.write_shard(p2, items, graph={"radius": 5.0, "max_neighbors": None}, names=["a", "b"])
    assert shard.read_shard_meta(p2)["names"] == ["a", "b"] and "targets" not in shard.read_shard_meta(p2)
    for k, v in packed.items():
        assert np.array_equal(shard.read_shard(p2)[k], v), k


def test_make_shards_writes_the_unlabeled_test_crystals(tmp_path):
    import importlib.util
    from cartnet_amd import shard
    spec = importlib.util.spec_from_file_location("make_shards", os.path.join(ROOT, "tools", "make_shards.py"))
    ms = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ms)
    parts = ms.write_split(str(tmp_path), 20, (5, 9), unlabeled=True)
    meta, pred = shard.read_shard_meta(str(tmp_path / "predict.cnshard")), shard.read_shard(str(tmp_path / "predict.cnshard"))
    test = shard.read_shard(str(tmp_path / "test.cnshard"))
    assert meta["targets"] is False and meta["names"] == [f"syn{g}" for g in ms.split(list(range(20)))[2]]
    assert "y" not in pred and "edge_ptr" not in pred and len(parts[2]) == len(meta["names"]) == 2
    for k in ("atom_ptr", "y_ptr", "z", "pos", "non_h_mask", "cell", "temperature"):
        assert np.array_equal(pred[k], test[k]), k
    ms.write_split(str(tmp_path / "plain"), 20, (5, 9))
    assert not os.path.exists(str(tmp_path / "plain" / "predict.cnshard"))


def _entry(cell, z, seed=0):
    g = torch.Generator().manual_seed(seed)
    n = int((torch.tensor(z) != 1).sum())
    return {"name": "abc 1", "z": torch.tensor(z), "frac": torch.rand(len(z), 3, generator=g),
            "cell": torch.from_numpy(np.float32(cell)), "temp": 123.5, "u_cif": torch.rand(n, 6, generator=g) * 0.05 - 0.01}


def test_write_cif_round_trip(tmp_path):
    from cartnet_amd.predict import write_cif
    cell = pu.cells()["triclinic_rotated"]
    z = [6, 1, 8, 17, 1, 26, 118]
    e = _entry(cell, z)
    path = str(tmp_path / "x.cif")
    write_cif(path, e)
    text = open(path).read()
    assert text.startswith("data_abc_1\n") and "_symmetry_space_group_name_H-M 'P 1'" in text
    got = [float(re.search(rf"^_cell_{k} (\S+)$", text, flags=re.M).group(1))
           for k in ("length_a", "length_b", "length_c", "angle_alpha", "angle_beta", "angle_gamma")]
    c = np.float64(cell)
    n = np.linalg.norm(c, axis=1)
    ang = [math.degrees(math.acos(c[i] @ c[j] / (n[i] * n[j]))) for i, j in ((1, 2), (0, 2), (0, 1))]
    assert np.abs(np.array(got) - np.array(list(n) + ang)).max() <= 1e-4
    assert np.abs(np.array(got) - np.array([5.1, 7.3, 11.9, 62.0, 104.0, 118.0])).max() <= 1e-4   # a rotation changes none
    assert float(re.search(r"^_diffrn_ambient_temperature (\S+)$", text, flags=re.M).group(1)) == 123.5
    loops = text.split("loop_\n")[1:]
    assert [len(re.findall(r"^_", l, flags=re.M)) for l in loops[:1]] == [1]                 # the symmetry operator
    site = [l.split() for l in loops[1].splitlines() if not l.startswith("_")]
    aniso = [l.split() for l in loops[2].splitlines() if not l.startswith("_")]
    assert [l for l in loops[2].splitlines() if l.startswith("_")] == ["_atom_site_aniso_label"] + [
        f"_atom_site_aniso_U_{ij}" for ij in ("11", "22", "33", "23", "13", "12")]
    assert len(site) == 7 and len(aniso) == 5
    assert [r[0] for r in site] == ["C1", "H2", "O3", "Cl4", "H5", "Fe6", "Og7"]
    assert [r[1] for r in site] == ["C", "H", "O", "Cl", "H", "Fe", "Og"]
    assert [r[0] for r in aniso] == ["C1", "O3", "Cl4", "Fe6", "Og7"]                        # the non-hydrogen atoms
    assert np.abs(np.array([[float(v) for v in r[2:]] for r in site]) - e["frac"].numpy()).max() <= 5.1e-7
    assert np.abs(np.array([[float(v) for v in r[1:]] for r in aniso]) - e["u_cif"].numpy()).max() <= 5.1e-7   # same order
    e["u_cif"] = e["u_cif"][:4]
    with pytest.raises(ValueError, match="4 ADP rows for 5"):
        write_cif(path, e)


def test_new_flags_parse_and_old_defaults_stay():
    import main as entry
    from cartnet_amd.config import cfg, set_cfg
    p = entry.build_parser()
    d = p.parse_args([])
    assert (d.predict, d.predict_input, d.predict_output, d.predict_cif_dir) == (False, None, "./predictions.pkl", None)
    assert (d.inference, d.montecarlo, d.inference_output, d.eval_batch, d.model, d.radius, d.disable_H) == \
        (False, False, "./inference.pkl", 1, "CartNet", 5.0, True)
    a = p.parse_args(["--predict", "--predict_input", "in.cnshard", "--predict_output", "o.pkl", "--predict_cif_dir", "c",
                      "--checkpoint_path", "w.ckpt"])
    assert (a.predict, a.predict_input, a.predict_output, a.predict_cif_dir) == (True, "in.cnshard", "o.pkl", "c")
    try:
        entry.fill_cfg(a)
        entry.check_predict_args(a)                                          # CartNet on ADP with weights and an input
        assert cfg.eval_batch == 1 and cfg.model == "CartNet" and cfg.use_H is True
        for extra, msg in ((["--model", "icomformer"], "does not serve --model icomformer"), (["--dataset", "jarvis"], "ADP")):
            b = p.parse_args(["--predict", "--predict_input", "i", "--checkpoint_path", "w"] + extra)
            entry.fill_cfg(b)
            with pytest.raises(SystemExit, match=msg):
                entry.check_predict_args(b)
        b = p.parse_args(["--predict", "--predict_input", "i"])
        entry.fill_cfg(b)
        with pytest.raises(SystemExit, match="checkpoint_path"):
            entry.check_predict_args(b)
        entry.fill_cfg(p.parse_args(["--predict", "--model", "ecomformer", "--predict_input", "i", "--checkpoint_path", "w"]))
        entry.check_predict_args(p.parse_args(["--predict", "--predict_input", "i", "--checkpoint_path", "w"]))
    finally:
        set_cfg()


def test_export_entry_point_is_declared_bound_and_launches_nothing_without_rows():
    from cartnet_amd import lib
    hdr = open(os.path.join(ROOT, "include", "cartnet_hip.h")).read()
    assert "dataset/extract_csd_data.py:115-123" in hdr
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+cartnet_adp_export\s*\(([^)]*)\)\s*;", hdr)
    assert m and len(m.group(1).split(",")) == 12 == len(lib.PROTOTYPES["cartnet_adp_export"][1])
    l = lib.load()
    assert lib.ABI_VERSION == 16 == l.cartnet_abi_version()
    assert l.cartnet_adp_export(None, None, None, 4, 0, None, None, None, None, None, None, None) == 0
    assert l.cartnet_adp_export(None, None, None, 0, 0, None, None, None, None, None, None, None) == 0
    assert l.cartnet_adp_export(None, None, None, 1, -1, None, None, None, None, None, None, None) != 0
    assert b"bad sizes" in l.cartnet_last_error()
    assert l.cartnet_adp_export(None, None, None, 2, 5, None, None, None, None, None, None, None) != 0   # before any launch
    assert b"null pointer" in l.cartnet_last_error()


def test_to_host_is_shared_not_copied():
    from cartnet_amd import evaluate, metrics, predict
    assert evaluate.to_host is metrics.to_host is predict.to_host
    out = metrics.to_host({"a": torch.arange(6, dtype=torch.int64).reshape(2, 3), "b": torch.zeros(0, 3),
                           "c": torch.tensor([1.5, 2.5], dtype=torch.float64), "d": torch.tensor([True, False])})
    assert out["a"].tolist() == [[0, 1, 2], [3, 4, 5]] and tuple(out["b"].shape) == (0, 3)
    assert out["c"].tolist() == [1.5, 2.5] and out["d"].tolist() == [True, False]
