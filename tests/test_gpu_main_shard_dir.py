"""``main.py --shard_dir DIR``: training from shard files with the reference's dataset recipe applied on the resident
shards -- graph (main.graph_request), hydrogen removal, canonical cell, temperature standardisation."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from cartnet_amd import shard
from cartnet_amd.synthetic import TEMP_MEAN, TEMP_STD

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE_KEYS = ("edge_ptr", "edge_src", "edge_tgt", "cart_dist", "cart_dir")
TRAIN = ["--dim_in", "32", "--num_layers", "2", "--epochs", "2", "--batch", "4", "--batch_accumulation", "2"]


def _make_shards():
    spec = importlib.util.spec_from_file_location("make_shards", os.path.join(ROOT, "tools", "make_shards.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def dirs(tmp_path_factory):
    """The 20 crystals of ``--synthetic 20 --atoms 10 30`` as shard directories: uncapped radius-5 graphs with the synthetic
    (standardised) temperatures, the same in Kelvin, and geometry only."""
    ms, root = _make_shards(), tmp_path_factory.mktemp("shards")
    out = {}
    for name, kw in (("std", dict(kelvin=False)), ("kelvin", dict(kelvin=True)),
                     ("geometry", dict(kelvin=False, geometry_only=True))):
        out[name] = str(root / name)
        out[name + "_parts"] = ms.write_split(out[name], 20, (10, 30), **kw)
    return out


def _loaders(extra):
    import main
    args = main.build_parser().parse_args(extra)
    main.fill_cfg(args)
    return main.create_loaders(args, 0, 1)


def _finite(res):
    return (len(res["history"]) == 2 and torch.isfinite(torch.tensor(res["test_mae"])) and
            all(torch.isfinite(torch.tensor([h["train_mae"], h["val_mae"]])).all() for h in res["history"]))


def test_training_from_shard_files_reproduces_the_resident_synthetic_path(dirs, tmp_path, monkeypatch):
    import main as entry
    monkeypatch.chdir(tmp_path)
    a = entry.main(["--synthetic", "20", "--atoms", "10", "30", "--resident_dataset", "--no_standarize_temp",
                    "--name", "synthetic"] + TRAIN)
    b = entry.main(["--shard_dir", dirs["std"], "--no_standarize_temp", "--name", "files"] + TRAIN)
    assert [h["train_mae"] for h in a["history"]] == [h["train_mae"] for h in b["history"]]
    assert a["test_metrics"] == b["test_metrics"]


def test_kelvin_shards_are_standardised_in_the_collation(dirs, tmp_path, monkeypatch):
    import main as entry
    loaders = _loaders(["--shard_dir", dirs["kelvin"], "--batch", "4"])
    assert [len(l.shard.atom_ptr) - 1 for l in loaders] == [16, 2, 2]
    kelvin = torch.cat([d.temperature.reshape(1) for d in dirs["kelvin_parts"][2]])
    assert float(kelvin.min()) >= 89.0 and float(kelvin.max()) <= 301.0          # really Kelvin (90 .. 300)
    got = torch.cat([b.temperature.cpu() for b in loaders[2]])
    want = (kelvin - torch.tensor(TEMP_MEAN, dtype=torch.float32)) / torch.tensor(TEMP_STD, dtype=torch.float32)
    assert got.dtype == torch.float32 and torch.equal(got, want)                 # the kernel's own fp32 expression
    raw = _loaders(["--shard_dir", dirs["kelvin"], "--batch", "4", "--no_standarize_temp"])
    assert torch.equal(torch.cat([b.temperature.cpu() for b in raw[2]]), kelvin)
    monkeypatch.chdir(tmp_path)
    assert _finite(entry.main(["--shard_dir", dirs["kelvin"], "--name", "kelvin"] + TRAIN))


def _same_graph(a, b):
    return all(torch.equal(a.t[k], b.t[k]) for k in EDGE_KEYS) and np.array_equal(a.edge_ptr, b.edge_ptr)


def test_graph_order_rule_on_the_loaders(dirs):
    stored = shard.DeviceShard.from_file(os.path.join(dirs["std"], "train.cnshard"))
    assert stored.graph == {"radius": 5.0, "max_neighbors": None}
    e5 = int(stored.edge_ptr[-1])
    # ADP + CartNet reads the stored edges whatever --radius says
    s = _loaders(["--shard_dir", dirs["std"], "--radius", "6"])[0].shard
    assert int(s.edge_ptr[-1]) == e5 and _same_graph(s, stored)
    # any other dataset regraphs at --radius
    s = _loaders(["--shard_dir", dirs["std"], "--dataset", "jarvis", "--radius", "6"])[0].shard
    assert int(s.edge_ptr[-1]) > e5 and _same_graph(s, stored.with_radius_graph(6.0))
    assert s.graph == {"radius": 6.0, "max_neighbors": None}
    # iComformer on ADP: compute_knn's capped graph of the full crystal, then the canonical cell
    s = _loaders(["--shard_dir", dirs["std"], "--model", "icomformer", "--max_neighbours", "8"])[0].shard
    want = stored.with_radius_graph(5.0, 8)
    assert int(want.edge_ptr[-1]) < e5                                           # the cap bites
    want = want.with_optimized_cell()
    assert _same_graph(s, want) and torch.equal(s.t["cell"], want.t["cell"]) and torch.equal(s.t["y"], want.t["y"])
    s25 = _loaders(["--shard_dir", dirs["std"], "--model", "icomformer"])[0].shard
    assert _same_graph(s25, stored.with_radius_graph(5.0, 25).with_optimized_cell())
    # a geometry-only directory is graphed at (radius, uncapped) for CartNet: the stored graph again
    g = _loaders(["--shard_dir", dirs["geometry"]])[0].shard
    assert g.has_graph and g.graph == {"radius": 5.0, "max_neighbors": None}
    for k in ("edge_ptr", "edge_src", "edge_tgt"):
        assert torch.equal(g.t[k], stored.t[k]), k
    assert torch.allclose(g.t["cart_dist"], stored.t["cart_dist"], rtol=1e-6, atol=0)
    assert torch.allclose(g.t["cart_dir"], stored.t["cart_dir"], rtol=0, atol=1e-6)


def test_a_recorded_graph_equal_to_the_request_is_not_rebuilt(dirs, monkeypatch):
    """The reference's cached-directory test (dataset/utils.py:462-464): jarvis at --radius 5 on shards that record an
    uncapped radius-5 graph keeps the uploaded edge arrays (same data_ptr); --radius 6 allocates new ones."""
    made = []
    orig = shard.DeviceShard.from_file.__func__

    def spy(cls, path, device="cuda:0"):
        made.append(orig(cls, path, device))
        return made[-1]

    monkeypatch.setattr(shard.DeviceShard, "from_file", classmethod(spy))
    kept = _loaders(["--shard_dir", dirs["std"], "--dataset", "jarvis", "--radius", "5"])
    assert len(made) == 3
    for loader, up in zip(kept, made):
        assert all(loader.shard.t[k].data_ptr() == up.t[k].data_ptr() for k in EDGE_KEYS)
    rebuilt = _loaders(["--shard_dir", dirs["std"], "--dataset", "jarvis", "--radius", "6"])
    assert all(rebuilt[0].shard.t[k].data_ptr() != made[3].t[k].data_ptr() for k in EDGE_KEYS)


def test_main_trains_icomformer_and_geometry_only_directories(dirs, tmp_path, monkeypatch):
    import main as entry
    monkeypatch.chdir(tmp_path)
    icf = entry.main(["--shard_dir", dirs["std"], "--model", "icomformer", "--no_standarize_temp", "--dim_in", "32",
                      "--epochs", "2", "--batch", "3", "--batch_accumulation", "1", "--name", "icf_files"])
    assert _finite(icf)
    assert _finite(entry.main(["--shard_dir", dirs["geometry"], "--no_standarize_temp", "--name", "geometry"] + TRAIN))
