"""The iComformer dataset recipe on the GPU: ``DeviceShard.with_optimized_cell`` (csrc/lattice_ops.hip: one wavefront per
crystal picks the canonical reduced lattice, one memory-bound pass rotates every edge direction and every 3x3 target)
against the host rule (``cartnet_amd.data.optimize_cell``: the reference's dataset/datasetADP.py:75-80 and
dataset/utils.py:366-452) and the reference's own outputs (tests/golden/optimize_cell.npz); and the recipe's way through
both loader paths of main.py.

What is exact and what is not: the integer selection (``basis``) must equal the host rule's wherever the candidates do not
tie within rounding; floats are compared with an fp64 evaluation of that selection within 1e-5 * max|reference| per array,
the project's fp32 parity budget."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from cartnet_amd import shard
from cartnet_amd.data import (Batch, Data, lattice_basis, lattice_frame, lattice_margins, optimize_cell, optimize_lattice,
                              remove_hydrogens)
from cartnet_amd.synthetic import make_crystal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "optimize_cell.npz")
KEYS = ("x", "pos", "edge_index", "cart_dist", "cart_dir", "y", "cell", "temperature", "non_H_mask")
OWNED = ("cell", "cart_dir", "y", "rotation", "basis")
BATCH_INTS = ("x", "non_H_mask", "batch", "ptr", "edge_index")
BATCH_FLOATS = ("pos", "cart_dist", "cart_dir", "cell", "temperature", "y")
BUDGET = 1e-5
PRED_TOL = 1e-5                                   # tests/test_gpu_model.py: the project's prediction budget


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _golden():
    z = np.load(GOLDEN)
    n = int(z["n_crystals"])
    ins = [Data(**{k: torch.from_numpy(z[f"in{i}_{k}"]) for k in KEYS}) for i in range(n)]
    outs = [{k: z[f"out{i}_{k}"] for k in KEYS} for i in range(n)]
    ins = [d if h else remove_hydrogens(d) for d, h in zip(ins, z["hydrogens"])]     # what get() canonicalises
    return ins, outs, z["group"]


def _close(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if want.size == 0:
        return
    err, bound = float(np.abs(got - want).max()), BUDGET * float(np.abs(want).max())
    assert err <= bound, f"{what}: max deviation {err:.3e} > {bound:.3e}"


def _valid(old_cell, new_cell, R, basis, what):
    """``new_cell`` is a canonical description of the lattice of ``old_cell`` in the frame ``R`` (the checks of
    tests/test_optimize_cell_host.py), and ``basis`` is the integer matrix between the two."""
    old, new, R = (np.asarray(a, dtype=np.float64).reshape(3, 3) for a in (old_cell, new_cell, R))
    T = (new @ R) @ np.linalg.inv(old)
    assert np.abs(T - np.round(T)).max() < 1e-3, (what, T)
    assert abs(abs(np.linalg.det(np.round(T))) - 1.0) < 1e-9, (what, T)
    assert np.array_equal(np.round(T).astype(np.int64), np.asarray(basis, dtype=np.int64).reshape(3, 3)), (what, T, basis)
    assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-5 and np.linalg.det(R) > 0, (what, R)
    assert max(abs(new[0, 1]), abs(new[0, 2]), abs(new[1, 2])) <= 1e-5 * np.abs(new).max(), (what, new)
    assert (np.diag(new) > 0).all(), (what, new)
    norms = np.linalg.norm(new, axis=1)
    assert norms[0] <= norms[1] * (1 + 1e-6) and norms[1] <= norms[2] * (1 + 1e-6), (what, norms)
    for r in (1, 2):
        assert new[0] @ new[r] >= -1e-5 * norms[r] ** 2, (what, r, new)


def _fp64(cell, basis, cart_dir, y=None):
    """The transform of one crystal evaluated in fp64 for a given integer selection; ``y``: per-atom targets [m,9]."""
    V = torch.as_tensor(np.asarray(basis, dtype=np.float64).reshape(3, 3)) @ torch.as_tensor(cell).double().reshape(3, 3)
    new_cell, R = lattice_frame(V)
    if y is not None:
        y = (R.T @ torch.as_tensor(y).double().reshape(-1, 3, 3) @ R).reshape(-1, 9)
    return new_cell, R, torch.as_tensor(cart_dir).double() @ R, y


def _arrays(ds: shard.DeviceShard):
    return {k: v.cpu().numpy() for k, v in ds.t.items()}


def _check_shard(arrays: dict, out: shard.DeviceShard, exact=None, per_atom=True, what=""):
    """Every crystal of the transformed shard ``out`` against the host rule on the packed input ``arrays``.  ``exact[g]``:
    the basis must be the host rule's (default: wherever the fp64 margins are clear: gap >= 1e-4 and |cos| >= 1e-4).
    Returns the number of crystals whose basis was compared exactly."""
    got = _arrays(out)
    G = arrays["atom_ptr"].shape[0] - 1
    assert got["basis"].dtype == np.int8 and got["basis"].shape == (G, 9)
    assert got["rotation"].dtype == np.float32 and got["rotation"].shape == (G, 9)
    assert got["cell"].dtype == np.float32 and got["cell"].shape == (G, 9)
    assert got["cart_dir"].dtype == np.float32 and got["cart_dir"].shape == arrays["cart_dir"].shape
    assert got["y"].dtype == np.float32 and got["y"].shape == arrays["y"].shape
    n_exact = 0
    for g in range(G):
        cell = torch.from_numpy(np.asarray(arrays["cell"][g])).reshape(3, 3)
        e0, e1, y0, y1 = (int(arrays[k][g + j]) for k in ("edge_ptr", "y_ptr") for j in (0, 1))
        if exact is None:
            gap, cos = lattice_margins(cell)
            must = gap >= 1e-4 and cos >= 1e-4
        else:
            must = bool(exact[g])
        if must:
            assert np.array_equal(got["basis"][g].reshape(3, 3), lattice_basis(cell).numpy()), (what, g)
            n_exact += 1
        _valid(cell, got["cell"][g], got["rotation"][g], got["basis"][g], (what, g))
        new_cell, R, dirs, y = _fp64(cell, got["basis"][g], arrays["cart_dir"][e0:e1],
                                     arrays["y"][y0:y1] if per_atom else None)
        _close(got["cell"][g].reshape(3, 3), new_cell, (what, g, "cell"))
        _close(got["rotation"][g].reshape(3, 3), R, (what, g, "rotation"))
        _close(got["cart_dir"][e0:e1], dirs, (what, g, "cart_dir"))
        if per_atom:
            _close(got["y"][y0:y1], y, (what, g, "y"))
    return n_exact


def _transform(items):
    full = shard.DeviceShard.from_data_list(items)
    before = {k: v.clone() for k, v in full.t.items()}
    out = full.with_optimized_cell()
    for k, v in before.items():                                          # the original shard is untouched
        assert torch.equal(full.t[k], v), k
    assert set(out.t) == set(full.t) | {"rotation", "basis"}
    owned = set(OWNED) if full.per_atom_target else set(OWNED) - {"y"}
    for k in full.t:                                                     # owns what it changed, shares the rest
        assert (out.t[k].data_ptr() != full.t[k].data_ptr()) == (k in owned), k
    for k in ("atom_ptr", "edge_ptr", "y_ptr"):
        assert np.array_equal(getattr(out, k), getattr(full, k))
    assert out.num_graphs == full.num_graphs and out.y_width == full.y_width
    return full, out


def test_golden_crystals_as_a_shard():
    ins, outs, group = _golden()
    full, out = _transform(ins)
    arrays = shard.pack(ins)
    n = _check_shard(arrays, out, exact=group != 2, what="golden")
    assert n == int((group != 2).sum()) >= 17
    got = _arrays(out)
    for i in np.flatnonzero(group != 2):                                 # and the reference's own outputs
        e0, e1, y0, y1 = (int(arrays[k][i + j]) for k in ("edge_ptr", "y_ptr") for j in (0, 1))
        _close(got["cell"][i].reshape(1, 3, 3), outs[i]["cell"], (i, "cell"))
        _close(got["cart_dir"][e0:e1], outs[i]["cart_dir"], (i, "cart_dir"))
        _close(got["y"][y0:y1].reshape(-1, 3, 3), outs[i]["y"], (i, "y"))


def test_ragged_shard_with_tiny_crystals_first_in_the_middle_and_last():
    sizes = (2, 324, 17, 64, 3, 2, 200, 129, 31, 77, 2)
    items = [make_crystal(700 + g, n) for g, n in enumerate(sizes)]
    _, out = _transform(items)
    assert _check_shard(shard.pack(items), out, what="ragged") >= len(sizes) - 1
    # a crystal without edges and one without targets in the shard
    bare = make_crystal(720, 6)
    bare.edge_index, bare.cart_dist, bare.cart_dir = torch.zeros(2, 0, dtype=torch.int64), torch.zeros(0), torch.zeros(0, 3)
    h_only = make_crystal(721, 5)
    h_only.x, h_only.non_H_mask, h_only.y = torch.ones_like(h_only.x), torch.zeros(5, dtype=torch.bool), torch.zeros(0, 3, 3)
    for items2 in ([bare, h_only] + items[:3], items[:2] + [h_only, bare, h_only] + items[2:4], items[:3] + [bare, h_only]):
        _, out = _transform(items2)
        _check_shard(shard.pack(items2), out, what="empty")


def test_scalar_targets_are_untouched():
    items = [make_crystal(740 + g, n, adp=False) for g, n in enumerate((5, 9, 2, 14, 3, 64, 2))]
    full, out = _transform(items)
    assert not out.per_atom_target and out.y_width == 1
    assert out.t["y"].data_ptr() == full.t["y"].data_ptr()              # shared, not copied
    _check_shard(shard.pack(items), out, per_atom=False, what="scalar")


@pytest.fixture(scope="module")
def large():
    """512 crystals of 194 atoms with GPU-built graphs (the constructor of tools/bench_no_hydrogens.py), every cell
    re-described by one of five unimodular matrices in turn: ~1.4 M edges."""
    tool = _tool("bench_optimize_cell")
    arrays, full = tool.large_shard(512, 194)
    return tool, arrays, full


def test_large_shard_crosses_many_tiles_with_a_ragged_tail(large):
    tool, arrays, full = large
    E, M, G = int(arrays["edge_ptr"][-1]), int(arrays["y_ptr"][-1]), 512
    assert E >= 2 ** 20 and E % 1024 != 0                # many edge tiles, the last one partly filled
    assert M > 2 ** 15 and M % 1024 != 0                 # and the same for the target rows
    out = full.with_optimized_cell()
    # fp64 classes: the re-description changes the basis, not the lattice
    cells = torch.from_numpy(np.asarray(arrays["cell"])).reshape(G, 3, 3)
    inv_u = np.linalg.inv(tool.UNIMODULAR.astype(np.float64))
    clear = np.zeros(G, dtype=bool)
    changed = 0
    for g in range(G):
        gap, cos = lattice_margins(cells[g])
        clear[g] = gap >= 1e-4 and cos >= 1e-4
        original = torch.from_numpy(inv_u[g % 5] @ cells[g].double().numpy()).to(torch.float32)
        gap0, cos0 = lattice_margins(original)
        if clear[g] and gap0 >= 1e-4 and cos0 >= 1e-4:                   # the same lattice: the same canonical cell
            _close(optimize_lattice(cells[g])[0], optimize_lattice(original)[0], (g, "re-description"))
        changed += not np.array_equal(np.abs(lattice_basis(cells[g]).numpy()), np.eye(3, dtype=np.int64))
    print(f"\nlarge shard: {int((~clear).sum())} of {G} crystals unclear, {changed} change basis")
    assert int((~clear).sum()) <= G // 100
    assert changed >= G // 2
    assert _check_shard(arrays, out, exact=clear, what="large") == int(clear.sum())
    # the same transform in torch device ops (tools/bench_optimize_cell.py) agrees as well
    ref = tool.torch_with_optimized_cell(full)
    same = (ref["basis"] == out.t["basis"]).all(dim=1).cpu().numpy()
    assert same[clear].all()
    for k in ("cell", "rotation"):
        _close(out.t[k][torch.from_numpy(same).to(out.device)].cpu(), ref[k][torch.from_numpy(same).to(out.device)].cpu(), k)
    if same.all():
        _close(out.t["cart_dir"].cpu(), ref["cart_dir"].cpu(), "cart_dir")
        _close(out.t["y"].cpu(), ref["y"].cpu(), "y")


def test_two_runs_give_identical_bytes(large):
    _, _, full = large
    a, b = full.with_optimized_cell(), full.with_optimized_cell()
    for k in a.t:
        assert a.t[k].cpu().numpy().tobytes() == b.t[k].cpu().numpy().tobytes(), k
    small = shard.DeviceShard.from_data_list([make_crystal(760 + g, n) for g, n in enumerate((9, 33, 2, 120))])
    a, b = small.with_optimized_cell(), small.with_optimized_cell()
    for k in a.t:
        assert a.t[k].cpu().numpy().tobytes() == b.t[k].cpu().numpy().tobytes(), k


def test_composes_with_hydrogen_removal_in_either_order():
    items = [make_crystal(770 + g, n) for g, n in enumerate((12, 40, 7, 90, 3, 31))]
    full = shard.DeviceShard.from_data_list(items)
    a = full.without_hydrogens().with_optimized_cell()
    b = full.with_optimized_cell().without_hydrogens()
    assert set(a.t) == set(b.t)
    for k in a.t:
        x, y = a.t[k].cpu(), b.t[k].cpu()
        assert x.dtype == y.dtype and x.shape == y.shape, k
        if x.dtype.is_floating_point:
            _close(x, y, k)
        else:
            assert torch.equal(x, y), k
    for k in ("atom_ptr", "edge_ptr", "y_ptr"):
        assert np.array_equal(getattr(a, k), getattr(b, k))
    host = [optimize_cell(remove_hydrogens(d)) for d in items]          # the reference's order
    _check_shard(shard.pack([remove_hydrogens(d) for d in items]), a, what="composed")
    _assert_same_batch(a.collate([0, 1, 2, 3, 4, 5]), Batch.from_data_list(host))


def _assert_same_batch(b, ref):
    for k in BATCH_INTS + BATCH_FLOATS:
        if not hasattr(ref, k):
            assert not hasattr(b, k), k
            continue
        got, want = getattr(b, k).cpu(), getattr(ref, k).cpu()
        assert got.dtype == want.dtype and got.shape == want.shape, (k, got.dtype, got.shape, want.dtype, want.shape)
        if k in BATCH_INTS:
            assert torch.equal(got, want), k
        else:
            _close(got, want, k)


def _clear_crystals(first, sizes, redescribe=None):
    items = [make_crystal(first + g, n) for g, n in enumerate(sizes)]
    for d in items:
        if redescribe is not None:                                       # the same lattice in another basis
            d.cell = (torch.tensor(redescribe, dtype=torch.float32) @ d.cell[0]).unsqueeze(0)
        gap, cos = lattice_margins(d.cell[0])
        assert gap >= 1e-4 and cos >= 1e-4                               # host and device pick the same basis
    return items


def test_collate_agrees_with_the_host_transformed_crystals():
    items = _clear_crystals(780, (5, 9, 14, 3, 64, 30, 21))
    out = shard.DeviceShard.from_data_list(items).with_optimized_cell()
    host = [optimize_cell(d) for d in items]
    for sel in ([0, 1, 2, 3, 4, 5, 6], [4], [6, 0, 4, 4, 5], [3, 3]):
        b = out.collate(sel)
        _assert_same_batch(b, Batch.from_data_list([host[i] for i in sel]))
        assert b.num_graphs == len(sel)


def test_icomformer_forward_agrees_on_the_device_and_the_host_transformed_batch():
    from conftest import rel_err
    from cartnet_amd.comformer import iComformer, make_icomformer_state_dict
    items = _clear_crystals(790, (30, 45, 64, 38), redescribe=[[1, 0, 0], [1, 1, 0], [0, 1, 1]])
    out = shard.DeviceShard.from_data_list(items).with_optimized_cell()
    host = [optimize_cell(d) for d in items]
    sel = [2, 0, 3, 1]
    m = iComformer(32)
    m.load_state_dict(make_icomformer_state_dict(32, seed=5))
    m = m.to("cuda:0").eval()
    with torch.no_grad():
        pred_dev, true_dev = m(out.collate(sel))
        pred_host, true_host = m(Batch.from_data_list([host[i] for i in sel]).to("cuda:0"))
        pred_raw, _ = m(Batch.from_data_list([items[i] for i in sel]).to("cuda:0"))
    assert torch.isfinite(pred_dev).all()
    print(f"\niComformer, device vs host transform: rel_err {rel_err(pred_dev, pred_host):.3e}")
    assert rel_err(pred_dev, pred_host) < PRED_TOL and rel_err(true_dev, true_host) < PRED_TOL
    # the model reads the lattice: the cell as it was written gives another prediction than the canonical one
    assert rel_err(pred_raw, pred_host) > 10 * PRED_TOL


def test_degenerate_cell_in_the_shard_raises_value_error():
    items = [make_crystal(800 + g, n) for g, n in enumerate((8, 12, 6, 10))]
    arrays = shard.pack(items)
    arrays["cell"] = arrays["cell"].copy()
    arrays["cell"][2] = np.array([4, 0, 0, 8, 0, 0, 0, 0, 5], dtype=np.float32)          # two collinear vectors
    with pytest.raises(ValueError, match="crystal 2"):
        shard.DeviceShard(arrays).with_optimized_cell()
    arrays["cell"][2] = np.array([4, 0, 0, 0, 5, 0, 4, 5, 0], dtype=np.float32)          # coplanar
    arrays["cell"][3] = arrays["cell"][2]
    with pytest.raises(ValueError, match="crystal 2"):
        shard.DeviceShard(arrays).with_optimized_cell()
    arrays["cell"][2] = arrays["cell"][3] = arrays["cell"][0]
    shard.DeviceShard(arrays).with_optimized_cell()


MAIN_ARGS = ["--synthetic", "20", "--atoms", "14", "24", "--batch", "4", "--max_neighbours", "6"]


def _loaders(extra):
    import main
    args = main.build_parser().parse_args(MAIN_ARGS + extra)
    main.fill_cfg(args)
    return main.create_loaders(args, 0, 1)


def _cap_bounds():
    """first-atom position -> per-atom in-degree bound of the cap rule (dataset/utils.py:240-360 with
    enforce_max_strictly False): a target with more than k edges keeps those within its (k+1)-th smallest squared
    distance + 0.01, so its bound is the number of its edges within that cutoff (1e-4 of slack for rounding); any other
    target keeps what it has."""
    k, out = 6, {}
    for g in range(20):
        d = make_crystal(g, None, 5.0, (14, 24))
        tgt, d2 = d.edge_index[1], d.cart_dist.double() ** 2
        bound = torch.bincount(tgt, minlength=d.x.shape[0])
        for a in torch.nonzero(bound > k).flatten().tolist():
            row = d2[tgt == a]
            bound[a] = int((row <= torch.sort(row).values[k] + 0.01 + 1e-4).sum())
        out[d.pos[0].numpy().tobytes()] = bound
    return out


@pytest.mark.parametrize("resident", [False, True])
def test_icomformer_loaders_hand_out_capped_graphs_in_the_canonical_frame(resident):
    bounds = _cap_bounds()
    seen, edges = 0, 0
    for loader in _loaders(["--model", "icomformer"] + (["--resident_dataset"] if resident else [])):
        for b in loader:
            c = b.cell.cpu()
            assert float(torch.stack((c[:, 0, 1], c[:, 0, 2], c[:, 1, 2])).abs().max()) <= 1e-5 * float(c.abs().max())
            assert bool((torch.diagonal(c, dim1=1, dim2=2) > 0).all())
            deg = torch.bincount(b.edge_index[1].cpu(), minlength=b.x.shape[0])
            ptr, pos = b.ptr.cpu(), b.pos.cpu()
            for g in range(b.num_graphs):
                bound = bounds[pos[ptr[g]].numpy().tobytes()]
                mine = deg[ptr[g]:ptr[g + 1]]
                assert mine.shape == bound.shape and bool((mine <= bound).all())
            seen += b.num_graphs
            edges += int(b.edge_index.shape[1])
    assert seen == 20
    uncapped = sum(int(make_crystal(g, None, 5.0, (14, 24)).edge_index.shape[1]) for g in range(20))
    assert edges < uncapped                                              # the cap bites on these crystals


@pytest.mark.parametrize("resident", [False, True])
def test_cartnet_batches_are_what_they_were(resident):
    """--model CartNet: no cap (main.py:176 sets -1) and no canonical frame -- the batches are byte-identical to those of
    loaders built directly from the uncapped crystals, as create_loaders built them before."""
    import main
    from cartnet_amd.config import cfg
    from cartnet_amd.data import DataLoader
    got = _loaders(["--augment"] + (["--resident_dataset"] if resident else []))
    graphs = [make_crystal(g, None, 5.0, (14, 24)) for g in range(20)]
    perm = torch.randperm(20, generator=torch.Generator().manual_seed(123)).tolist()
    parts = [[graphs[i] for i in perm[:16]], [graphs[i] for i in perm[16:18]], [graphs[i] for i in perm[18:]]]
    if resident:
        shards = [shard.DeviceShard.from_data_list(p, cfg.device) for p in parts]
        want = [shard.ShardLoader(shards[0], 4, shuffle=True, seed=cfg.seed, augment=True),
                shard.ShardLoader(shards[1], 4), shard.ShardLoader(shards[2], 1)]
    else:
        from cartnet_amd.synthetic import augment_data
        gen = torch.Generator().manual_seed(cfg.seed)
        want = [DataLoader(parts[0], 4, shuffle=True, seed=cfg.seed, transform=lambda d: augment_data(d, gen)),
                DataLoader(parts[1], 4), DataLoader(parts[2], 1)]
    n = 0
    for lg, lw in zip(got, want):
        for b, w in zip(list(lg), list(lw)):
            assert set(b.keys()) == set(w.keys())
            for k in BATCH_INTS + BATCH_FLOATS:
                x, y = getattr(b, k).cpu(), getattr(w, k).cpu()
                assert x.dtype == y.dtype and x.numpy().tobytes() == y.numpy().tobytes(), k
            n += b.num_graphs
    assert n == 20


@pytest.mark.parametrize("resident", [False, True])
def test_main_trains_icomformer_on_both_loader_paths(resident, tmp_path, monkeypatch):
    import main as entry
    monkeypatch.chdir(tmp_path)
    res = entry.main(["--synthetic", "12", "--atoms", "10", "20", "--dim_in", "32", "--epochs", "2", "--batch", "3",
                      "--batch_accumulation", "1", "--name", "icf_cell", "--model", "icomformer", "--max_neighbours", "8"]
                     + (["--resident_dataset"] if resident else []))
    assert len(res["history"]) == 2
    assert all(torch.isfinite(torch.tensor(h["train_mae"])) and torch.isfinite(torch.tensor(h["val_mae"]))
               for h in res["history"])
    assert torch.isfinite(torch.tensor(res["test_mae"]))


def test_hip_pass_is_not_slower_than_the_torch_restatement(large):
    """HIP events around ``with_optimized_cell()`` and around the same transform in torch device ops on the same shard,
    taken alternately in this process (A B A B), warm, medians of 9.  The figures are printed; the only condition is that
    the HIP pass is not the slower one."""
    tool, _, full = large
    r = tool.measure(full, rounds=9)
    print("\nwith_optimized_cell:", r)
    assert r["hip_ms_median"] <= r["torch_ms_median"], r
