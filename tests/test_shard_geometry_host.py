"""Host side of the shard-wide radius graph: geometry-only shards, the graph provenance in the file header, the
``graph_request`` rule of ``main.py --shard_dir`` and the new C prototypes.  No GPU needed."""
import json
import re
import struct
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from cartnet_amd import shard
from cartnet_amd.synthetic import make_crystal, make_geometry


def _items(geometry: bool):
    make = make_geometry if geometry else make_crystal
    return [make(40 + g, n) for g, n in enumerate((5, 1, 12))]


def test_geometry_only_pack_write_read_round_trip(tmp_path):
    geo, full = _items(True), _items(False)
    arrays = shard.pack(geo)
    assert not any(k in arrays for k in ("edge_ptr", "edge_src", "edge_tgt", "cart_dist", "cart_dir"))
    want = shard.pack(full)
    assert set(arrays) == set(want) - {"edge_ptr", "edge_src", "edge_tgt", "cart_dist", "cart_dir"}
    for k, v in arrays.items():
        assert v.dtype == want[k].dtype and np.array_equal(v, want[k]), k
    path = str(tmp_path / "geo.cnshard")
    shard.write_shard(path, geo)
    back = shard.read_shard(path)
    assert set(back) == set(arrays)
    for k, v in arrays.items():
        assert back[k].dtype == v.dtype and np.array_equal(back[k], v), k
    meta = shard.read_shard_meta(path)
    assert meta["graphs"] == 3 and "graph" not in meta and "edge_src" not in meta["arrays"]
    with pytest.raises(ValueError, match="geometry-only"):
        shard.write_shard(path, geo, graph={"radius": 5.0, "max_neighbors": None})


def test_mixed_lists_and_bare_crystals_are_refused():
    geo, full = _items(True), _items(False)
    for mix in ([full[0], geo[1]], [geo[0], full[1], geo[2]]):
        with pytest.raises(ValueError, match="with and without"):
            shard.pack(mix)
    bare = geo[0].clone()
    del bare.__dict__["cell"]
    with pytest.raises(ValueError, match="pos and cell"):
        shard.pack([bare, geo[1]])


def test_header_graph_round_trip_and_old_format_files(tmp_path):
    full = _items(False)
    new, old = str(tmp_path / "new.cnshard"), str(tmp_path / "old.cnshard")
    shard.write_shard(new, full, graph={"radius": 5, "max_neighbors": -1})
    assert shard.read_shard_meta(new)["graph"] == {"radius": 5.0, "max_neighbors": None}
    shard.write_shard(new, full, graph={"radius": 6.5, "max_neighbors": 25})
    assert shard.read_shard_meta(new)["graph"] == {"radius": 6.5, "max_neighbors": 25}
    # a file as write_shard wrote it before the header knew about graphs: {"arrays", "graphs"} and nothing else
    shard.write_shard(old, full)
    with open(old, "rb") as f:
        assert f.read(8) == shard.MAGIC
        (hlen,) = struct.unpack("<Q", f.read(8))
        head = json.loads(f.read(hlen).decode())
    assert set(head) == {"arrays", "graphs"} and (16 + hlen) % 64 == 0
    assert shard.read_shard_meta(old).get("graph") is None
    a, b = shard.read_shard(old), shard.read_shard(new)
    assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)
    assert shard.graph_record(5.0, 0) == {"radius": 5.0, "max_neighbors": None}


def _cfg(dataset="ADP", model="CartNet", radius=5.0, max_neighbours=-1):
    return SimpleNamespace(dataset=SimpleNamespace(name=dataset), model=model, radius=radius, max_neighbours=max_neighbours)


def test_graph_request_table():
    from main import graph_request
    r5, r5k25 = {"radius": 5.0, "max_neighbors": None}, {"radius": 5.0, "max_neighbors": 25}
    # ADP + CartNet: the stored graph whatever --radius says; a geometry-only shard is graphed uncapped at --radius
    assert graph_request(_cfg(radius=6.0), r5, True) is None
    assert graph_request(_cfg(radius=6.0), None, True) is None
    assert graph_request(_cfg(radius=6.0), None, False) == (6.0, None)
    # ADP + e/iComformer: compute_knn(max_neighbours, radius)
    for model in ("icomformer", "ecomformer"):
        assert graph_request(_cfg(model=model, max_neighbours=25), r5, True) == (5.0, 25)
        assert graph_request(_cfg(model=model, max_neighbours=25), None, True) == (5.0, 25)
        assert graph_request(_cfg(model=model, max_neighbours=25), None, False) == (5.0, 25)
        assert graph_request(_cfg(model=model, max_neighbours=25), r5k25, True) is None        # already that graph
        assert graph_request(_cfg(model=model, max_neighbours=12), r5k25, True) == (5.0, 12)
        assert graph_request(_cfg(model=model, radius=4.0, max_neighbours=25), r5k25, True) == (4.0, 25)
    # any other dataset: (radius, cap or None)
    assert graph_request(_cfg("jarvis", radius=6.0), r5, True) == (6.0, None)
    assert graph_request(_cfg("jarvis"), r5, True) is None
    assert graph_request(_cfg("jarvis"), None, True) == (5.0, None)                            # provenance unknown
    assert graph_request(_cfg("jarvis"), r5, False) == (5.0, None)
    assert graph_request(_cfg("megnet", "icomformer", 5.0, 25), r5, True) == (5.0, 25)
    assert graph_request(_cfg("megnet", "icomformer", 5.0, 25), r5k25, True) is None
    assert graph_request(_cfg("megnet", "icomformer", 5.0, 0), r5, True) is None               # cap <= 0 is no cap


def test_shard_dir_flag_reaches_cfg():
    import main
    from cartnet_amd.config import cfg
    args = main.build_parser().parse_args(["--shard_dir", "some/dir", "--model", "icomformer"])
    assert args.shard_dir == "some/dir"
    main.fill_cfg(args)
    assert cfg.shard_dir == "some/dir" and cfg.max_neighbours == 25
    main.fill_cfg(main.build_parser().parse_args([]))
    assert cfg.shard_dir is None


def test_regraph_prototypes_are_declared_and_bound():
    import os
    from cartnet_amd import lib
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "cartnet_hip.h")).read()
    declared = set(re.findall(r"\b(cartnet_[a-z0-9_]+)\s*\(", hdr))
    names = {n for n in lib.PROTOTYPES if n.startswith("cartnet_shard_regraph_")}
    assert {"cartnet_shard_regraph_workspace_bytes", "cartnet_shard_regraph_count", "cartnet_shard_regraph_fill"} <= names
    assert names <= declared and lib.ABI_VERSION == 16
    for gone in ("cartnet_radius_graph_count", "cartnet_radius_graph_fill", "cartnet_neighbor_cap_count",
                 "cartnet_neighbor_cap_fill"):
        assert gone not in lib.PROTOTYPES and gone not in declared
    assert "dataset/utils.py:456-486" in hdr and "dataset/figshare_dataset.py:50-76" in hdr
