"""--disable_H on the GPU: ``DeviceShard.without_hydrogens`` (csrc/shard_ops.hip: the stable compaction of a whole
resident shard) holds, bit for bit, what packing the host-filtered crystals holds (``cartnet_amd.data.remove_hydrogens``:
the reference's dataset/datasetADP.py:49-72); and the flag reaches both loader paths of main.py."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from cartnet_amd import shard
from cartnet_amd.data import Batch, Data, remove_hydrogens
from cartnet_amd.model import CartNet, make_state_dict
from cartnet_amd.synthetic import make_crystal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARRAYS = ("atom_ptr", "edge_ptr", "y_ptr", "z", "pos", "non_h_mask", "edge_src", "edge_tgt", "cart_dist", "cart_dir", "cell",
          "temperature", "y")
BATCH_KEYS = ("x", "pos", "non_H_mask", "batch", "ptr", "edge_index", "cart_dist", "cart_dir", "cell", "temperature", "y")


def _bench_tool():
    spec = importlib.util.spec_from_file_location("bench_no_hydrogens", os.path.join(ROOT, "tools", "bench_no_hydrogens.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _edge_cases():
    """(all hydrogen, no edges at all, a kept atom that loses every neighbour) -- as tests/test_no_hydrogens_host.py."""
    base = make_crystal(310, 9)
    h_only = base.clone()
    h_only.x = torch.ones_like(base.x)
    h_only.non_H_mask = torch.zeros(9, dtype=torch.bool)
    h_only.y = torch.zeros(0, 3, 3)
    no_edges = make_crystal(311, 8)
    no_edges.edge_index = torch.zeros(2, 0, dtype=torch.int64)
    no_edges.cart_dist = torch.zeros(0)
    no_edges.cart_dir = torch.zeros(0, 3)
    lonely = Data(x=torch.tensor([6, 1, 1, 6, 8]), pos=torch.arange(15, dtype=torch.float32).reshape(5, 3),
                  cell=torch.eye(3).unsqueeze(0) * 9.0, natoms=torch.tensor([5]),
                  edge_index=torch.tensor([[1, 2, 0, 0, 4, 1, 3], [0, 0, 1, 2, 3, 3, 4]]),
                  cart_dist=torch.arange(1, 8, dtype=torch.float32),
                  cart_dir=torch.nn.functional.normalize(torch.arange(21, dtype=torch.float32).reshape(7, 3) + 1, dim=1),
                  y=torch.arange(27, dtype=torch.float32).reshape(3, 3, 3), non_H_mask=torch.tensor([1, 0, 0, 1, 1]).bool(),
                  temperature=torch.tensor([0.25]))
    return h_only, no_edges, lonely


def _assert_holds(ds: shard.DeviceShard, want: dict):
    """Every array of the resident shard equals the packed host arrays: names, dtypes, shapes, bytes."""
    assert set(ds.t) == set(want)
    for k in ARRAYS:
        if k not in want:
            continue
        got = ds.t[k].cpu().numpy()
        assert got.dtype == want[k].dtype and got.shape == want[k].shape, (k, got.dtype, got.shape, want[k].dtype,
                                                                          want[k].shape)
        assert got.tobytes() == np.ascontiguousarray(want[k]).tobytes(), k
    for k in ("atom_ptr", "edge_ptr", "y_ptr"):                          # the host copies the loaders read
        assert np.array_equal(getattr(ds, k), want[k]) and getattr(ds, k).dtype == np.int64, k
    assert ds.num_graphs == want["atom_ptr"].shape[0] - 1


def _check(items):
    full = shard.DeviceShard.from_data_list(items)
    before = {k: v.clone() for k, v in full.t.items()}
    out = full.without_hydrogens()
    _assert_holds(out, shard.pack([remove_hydrogens(d) for d in items]))
    for k, v in before.items():                                          # the original shard is untouched
        assert torch.equal(full.t[k], v), k
    return full, out


def _assert_same_batch(b, ref):
    for k in BATCH_KEYS:
        if not hasattr(ref, k):
            assert not hasattr(b, k), k
            continue
        got, want = getattr(b, k).cpu(), getattr(ref, k)
        assert got.dtype == want.dtype and got.shape == want.shape, (k, got.dtype, got.shape, want.dtype, want.shape)
        assert torch.equal(got, want), k


def test_ragged_crystals():
    sizes = (2, 324, 17, 64, 3, 200, 5, 129, 31, 2, 77)
    _check([make_crystal(500 + g, n) for g, n in enumerate(sizes)])


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_edge_cases_anywhere_in_the_shard(where):
    """A crystal of hydrogens only (zero atoms afterwards: equal consecutive offsets), a crystal without edges, a kept
    atom that loses all its neighbours -- at the start, in the middle and at the end of a shard."""
    plain = [make_crystal(520 + g, n) for g, n in enumerate((12, 40, 7, 90))]
    special = list(_edge_cases())
    items = {"first": special + plain, "middle": plain[:2] + special + plain[2:], "last": plain + special}[where]
    _, out = _check(items)
    g = {"first": 0, "middle": 2, "last": 4}[where]                      # the hydrogen-only crystal
    assert out.atom_ptr[g] == out.atom_ptr[g + 1] and out.edge_ptr[g] == out.edge_ptr[g + 1]
    # several empty crystals in a row, and a shard that ends in them
    _check(plain[:1] + [special[0]] * 3 + plain[1:2] + [special[0], special[1], special[0]])


def test_scalar_target_shard():
    items = [make_crystal(540 + g, n, adp=False) for g, n in enumerate((5, 9, 2, 14, 3, 64, 2))]
    full, out = _check(items)
    assert "non_h_mask" not in out.t and not out.per_atom_target and out.y_width == 1
    assert out.t["y"].data_ptr() == full.t["y"].data_ptr()              # shared, not copied
    sel = [3, 1, 6, 5]
    _assert_same_batch(out.collate(sel), Batch.from_data_list([remove_hydrogens(items[i]) for i in sel]))


def _unpack(a: dict):
    """The crystals of packed arrays as ``Data`` (the inverse of shard.pack for ADP-shaped crystals)."""
    out = []
    for g in range(a["atom_ptr"].shape[0] - 1):
        n0, n1, e0, e1, y0, y1 = (int(a[k][g + j]) for k in ("atom_ptr", "edge_ptr", "y_ptr") for j in (0, 1))
        out.append(Data(x=torch.from_numpy(a["z"][n0:n1].astype(np.int64)), pos=torch.from_numpy(a["pos"][n0:n1]),
                        cell=torch.from_numpy(a["cell"][g].reshape(1, 3, 3)),
                        edge_index=torch.from_numpy(np.stack((a["edge_src"][e0:e1], a["edge_tgt"][e0:e1])).astype(np.int64)),
                        cart_dist=torch.from_numpy(a["cart_dist"][e0:e1]), cart_dir=torch.from_numpy(a["cart_dir"][e0:e1]),
                        y=torch.from_numpy(a["y"][y0:y1].reshape(-1, 3, 3)),
                        non_H_mask=torch.from_numpy(a["non_h_mask"][n0:n1].astype(bool)),
                        temperature=torch.from_numpy(a["temperature"][g:g + 1])))
    return out


@pytest.fixture(scope="module")
def large():
    """512 crystals of 194 atoms with GPU-built graphs: ~1.4 M edges, so both prefix sums cross many 1024-item tiles, and
    the edge total is not a multiple of the tile."""
    arrays, full = _bench_tool().large_shard(512, 194)
    return arrays, full


def test_large_shard_crosses_many_tiles_with_a_ragged_tail(large):
    arrays, full = large
    N, E = int(arrays["atom_ptr"][-1]), int(arrays["edge_ptr"][-1])
    assert E >= 2 ** 20 and E % 1024 != 0 and (E + 1) % 1024 != 0
    assert N == 97 * 1024                 # the atoms fill their tiles exactly: the one-past-the-end item opens a tile
    out = full.without_hydrogens()
    want = shard.pack([remove_hydrogens(d) for d in _unpack(arrays)])
    assert int(want["edge_ptr"][-1]) % 1024 != 0 and int(want["edge_ptr"][-1]) > 2 ** 18
    assert int(want["atom_ptr"][-1]) % 1024 != 0
    _assert_holds(out, want)
    # the same transform in torch device ops (tools/bench_no_hydrogens.py) agrees as well
    for k, v in _bench_tool().torch_without_hydrogens(full).items():
        assert torch.equal(v, out.t[k]), k


def test_two_runs_give_identical_bytes(large):
    _, full = large
    a, b = full.without_hydrogens(), full.without_hydrogens()
    for k in a.t:
        assert a.t[k].cpu().numpy().tobytes() == b.t[k].cpu().numpy().tobytes(), k
    small = shard.DeviceShard.from_data_list([make_crystal(560 + g, n) for g, n in enumerate((9, 33, 2, 120))])
    a, b = small.without_hydrogens(), small.without_hydrogens()
    for k in a.t:
        assert a.t[k].cpu().numpy().tobytes() == b.t[k].cpu().numpy().tobytes(), k


def test_hip_pass_is_not_slower_than_the_torch_restatement(large):
    """HIP events around ``without_hydrogens()`` and around the same transform in torch device ops on the same shard,
    taken alternately in this process (A B A B), warm, medians of 9.  The figures are printed; the only condition is that
    the HIP pass is not the slower one."""
    _, full = large
    r = _bench_tool().measure(full, rounds=9)
    print("\nwithout_hydrogens:", r)
    assert r["hip_ms_median"] <= r["torch_ms_median"], r


def test_mask_that_contradicts_the_atomic_numbers_raises_value_error():
    items = [make_crystal(570 + g, n) for g, n in enumerate((12, 30, 8))]
    arrays = shard.pack(items)
    arrays["non_h_mask"] = arrays["non_h_mask"].copy()
    i = int(np.flatnonzero(arrays["z"] == 1)[-1])
    arrays["non_h_mask"][i] = 1                                          # a hydrogen the mask calls a non-hydrogen
    with pytest.raises(ValueError):
        shard.DeviceShard(arrays).without_hydrogens()
    arrays["non_h_mask"][i] = 0
    j = int(np.flatnonzero(arrays["z"] != 1)[0])
    arrays["non_h_mask"][j] = 0                                          # and the other way round
    with pytest.raises(ValueError):
        shard.DeviceShard(arrays).without_hydrogens()
    arrays["non_h_mask"][j] = 1
    shard.DeviceShard(arrays).without_hydrogens()


def test_collate_and_model_agree_with_the_host_filtered_crystals():
    """tests/test_gpu_shard.py's comparison on the compacted shard; CartNet forward + backward on the device-built and the
    host-built batch agree bit for bit (same inputs, same kernels).  The zero-atom crystal stays out of the selections."""
    special = list(_edge_cases())
    items = [make_crystal(580 + g, n) for g, n in enumerate((5, 9, 14, 3, 64, 30))] + special
    out = shard.DeviceShard.from_data_list(items).without_hydrogens()
    host = [remove_hydrogens(d) for d in items]
    for sel in ([0, 1, 2, 3, 4, 5, 7, 8], [4], [8, 0, 4, 4, 7], [7, 7]):
        b = out.collate(sel)
        _assert_same_batch(b, Batch.from_data_list([host[i] for i in sel]))
        assert b.num_graphs == len(sel)
    sel = [4, 8, 0, 5, 2, 7, 1]
    grads = []
    for make in (lambda: out.collate(sel), lambda: Batch.from_data_list([host[i] for i in sel]).to("cuda:0")):
        m = CartNet(32, 16, 2)
        m.load_state_dict(make_state_dict(32, 16, 2, seed=4))
        m = m.cuda().train()
        pred, true = m(make())
        (pred - true).abs().mean().backward()
        grads.append((pred.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters()}))
    assert torch.isfinite(grads[0][0]).all()
    assert torch.equal(grads[0][0], grads[1][0])
    for k in grads[0][1]:
        assert torch.equal(grads[0][1][k], grads[1][1][k]), k


@pytest.mark.parametrize("resident", [False, True])
def test_disable_h_reaches_every_batch_of_the_three_loaders(resident):
    import main
    argv = ["--synthetic", "20", "--atoms", "10", "30", "--batch", "4", "--disable_H"]
    args = main.build_parser().parse_args(argv + (["--resident_dataset"] if resident else []))
    main.fill_cfg(args)
    loaders = main.create_loaders(args, 0, 1)
    assert len(loaders) == 3
    seen = 0
    for loader in loaders:
        for b in loader:
            assert not bool((b.x == 1).any())
            assert b.non_H_mask.dtype == torch.bool and bool(b.non_H_mask.all())
            assert b.y.shape[0] == b.x.shape[0]
            seen += b.num_graphs
    assert seen == 20


def test_main_with_disable_h_trains_on_other_data_and_both_loader_paths_agree(tmp_path, monkeypatch):
    """tests/test_gpu_main.py::test_main_with_resident_dataset_matches_host_loader with --disable_H: the host-loader run
    and the --resident_dataset run agree exactly, and differ from the run that keeps the hydrogens."""
    import main as entry
    monkeypatch.chdir(tmp_path)
    common = ["--synthetic", "20", "--atoms", "10", "30", "--dim_in", "32", "--num_layers", "2", "--epochs", "2",
              "--batch", "4", "--batch_accumulation", "2"]
    a = entry.main(common + ["--name", "host_noh", "--disable_H"])
    b = entry.main(common + ["--name", "resident_noh", "--resident_dataset", "--disable_H"])
    assert [h["train_mae"] for h in a["history"]] == [h["train_mae"] for h in b["history"]]
    assert a["test_metrics"] == b["test_metrics"]
    c = entry.main(common + ["--name", "host_h"])
    assert [h["train_mae"] for h in a["history"]] != [h["train_mae"] for h in c["history"]]
    assert all(torch.isfinite(torch.tensor(h["train_mae"])) for h in a["history"])


def test_main_runs_icomformer_with_disable_h(tmp_path, monkeypatch):
    """The transform is per dataset, not per model (loader/loader.py:29-32)."""
    import main as entry
    monkeypatch.chdir(tmp_path)
    res = entry.main(["--synthetic", "12", "--atoms", "10", "20", "--dim_in", "32", "--epochs", "2", "--batch", "3",
                      "--batch_accumulation", "1", "--name", "icf_noh", "--model", "icomformer", "--disable_H"])
    assert len(res["history"]) == 2
    assert all(torch.isfinite(torch.tensor(h["train_mae"])) for h in res["history"])
