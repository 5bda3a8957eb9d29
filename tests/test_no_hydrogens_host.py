"""--disable_H on the host: ``cartnet_amd.data.remove_hydrogens`` against the reference's own
``DatasetADP.get(..., hydrogens=False)`` (dataset/datasetADP.py:49-72; fixture tests/golden/no_hydrogens.npz written by
tests/golden/make_golden_no_hydrogens.py), and the cases the reference leaves undefined (no edge survives: its
renumbering builds a malformed tensor there), which this project defines."""
import os

import numpy as np
import pytest
import torch

from cartnet_amd.data import Batch, Data, remove_hydrogens
from cartnet_amd.shard import pack
from cartnet_amd.synthetic import make_crystal

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "no_hydrogens.npz")
KEYS = ("x", "pos", "edge_index", "cart_dist", "cart_dir", "y", "cell", "temperature", "non_H_mask")


def _golden():
    z = np.load(GOLDEN)
    n = int(z["n_crystals"])
    ins = [Data(**{k: torch.from_numpy(z[f"in{i}_{k}"]) for k in KEYS}) for i in range(n)]
    outs = [{k: z[f"out{i}_{k}"] for k in KEYS} for i in range(n)]
    return ins, outs


def test_fixture_covers_what_it_should():
    ins, outs = _golden()
    assert len(ins) >= 4
    assert any(not bool((d.x == 1).any()) for d in ins), "one crystal without any hydrogen"
    assert sum(bool((d.x == 1).any()) for d in ins) >= 3
    for d, o in zip(ins, outs):
        assert o["edge_index"].shape[1] >= 1                     # the reference's renumbering needs a surviving edge
        assert o["x"].shape[0] == int((d.x != 1).sum())


def test_remove_hydrogens_matches_the_reference_bit_for_bit():
    ins, outs = _golden()
    for i, (d, want) in enumerate(zip(ins, outs)):
        before = {k: getattr(d, k).clone() for k in KEYS}
        got = remove_hydrogens(d)
        for k in KEYS:
            g = getattr(got, k).numpy()
            assert g.dtype == want[k].dtype and g.shape == want[k].shape, (i, k, g.dtype, g.shape, want[k].shape)
            assert g.tobytes() == want[k].tobytes(), (i, k)
            assert torch.equal(getattr(d, k), before[k]), f"crystal {i}: input {k} was modified"


def _edge_cases():
    """(all hydrogen, no edges at all, a kept atom that loses every neighbour)."""
    base = make_crystal(310, 9)
    h_only = base.clone()
    h_only.x = torch.ones_like(base.x)
    h_only.non_H_mask = torch.zeros(9, dtype=torch.bool)
    h_only.y = torch.zeros(0, 3, 3)
    no_edges = make_crystal(311, 8)
    no_edges.edge_index = torch.zeros(2, 0, dtype=torch.int64)
    no_edges.cart_dist = torch.zeros(0)
    no_edges.cart_dir = torch.zeros(0, 3)
    # atoms 0..4: carbon 0 is bonded to hydrogens only, carbons 3 and 4 to each other
    lonely = Data(x=torch.tensor([6, 1, 1, 6, 8]), pos=torch.arange(15, dtype=torch.float32).reshape(5, 3),
                  cell=torch.eye(3).unsqueeze(0) * 9.0, natoms=torch.tensor([5]),
                  edge_index=torch.tensor([[1, 2, 0, 0, 4, 1, 3], [0, 0, 1, 2, 3, 3, 4]]),
                  cart_dist=torch.arange(1, 8, dtype=torch.float32),
                  cart_dir=torch.nn.functional.normalize(torch.arange(21, dtype=torch.float32).reshape(7, 3) + 1, dim=1),
                  y=torch.arange(27, dtype=torch.float32).reshape(3, 3, 3), non_H_mask=torch.tensor([1, 0, 0, 1, 1]).bool(),
                  temperature=torch.tensor([0.25]))
    return h_only, no_edges, lonely


def _check_invariants(d, out):
    keep = d.x != 1
    assert torch.equal(out.x, d.x[keep]) and not bool((out.x == 1).any())
    assert torch.equal(out.pos, d.pos[keep])
    assert int(out.natoms) == out.x.shape[0]
    assert out.edge_index.dtype == torch.int64 and out.edge_index.dim() == 2 and out.edge_index.shape[0] == 2
    E = out.edge_index.shape[1]
    assert out.cart_dist.shape == (E,) and out.cart_dir.shape == (E, 3)
    if E:
        assert int(out.edge_index.min()) >= 0 and int(out.edge_index.max()) < out.x.shape[0]
        assert bool((out.edge_index[1][1:] >= out.edge_index[1][:-1]).all())
    assert out.non_H_mask.dtype == torch.bool and out.non_H_mask.shape == out.x.shape and bool(out.non_H_mask.all())
    for k in ("y", "cell", "temperature"):
        assert torch.equal(getattr(out, k), getattr(d, k))


def test_crystal_of_hydrogens_only_becomes_a_crystal_of_zero_atoms():
    h_only, _, _ = _edge_cases()
    out = remove_hydrogens(h_only)
    _check_invariants(h_only, out)
    assert out.x.shape == (0,) and out.pos.shape == (0, 3) and tuple(out.edge_index.shape) == (2, 0)


def test_crystal_without_edges():
    _, no_edges, _ = _edge_cases()
    out = remove_hydrogens(no_edges)
    _check_invariants(no_edges, out)
    assert tuple(out.edge_index.shape) == (2, 0) and out.x.shape[0] == int((no_edges.x != 1).sum()) > 0


def test_kept_atom_that_loses_all_its_neighbours():
    _, _, lonely = _edge_cases()
    out = remove_hydrogens(lonely)
    _check_invariants(lonely, out)
    assert out.x.tolist() == [6, 6, 8]
    assert out.edge_index.tolist() == [[2, 1], [1, 2]]               # old (4 -> 3), (3 -> 4); atom 0 is isolated now
    assert out.cart_dist.tolist() == [5.0, 7.0]
    assert torch.equal(out.cart_dir, lonely.cart_dir[[4, 6]])


def test_filtered_crystals_pack_with_equal_consecutive_offsets_for_the_empty_one():
    h_only, no_edges, lonely = _edge_cases()
    ds = [remove_hydrogens(d) for d in (lonely, h_only, no_edges, make_crystal(312, 11))]
    a = pack(ds)
    assert a["atom_ptr"][1] == a["atom_ptr"][2] and a["edge_ptr"][1] == a["edge_ptr"][2] == a["edge_ptr"][3]
    assert a["non_h_mask"].all() and not (a["z"] == 1).any()
    assert a["y_ptr"][-1] == a["z"].shape[0]                         # one target row per remaining atom
    b = Batch.from_data_list([ds[0], ds[2], ds[3]])                  # the zero-atom crystal stays out of batches
    assert b.y.shape[0] == b.x.shape[0] and bool(b.non_H_mask.all())


def test_mask_that_contradicts_the_atomic_numbers_is_refused():
    d = make_crystal(313, 10)
    d.non_H_mask = ~d.non_H_mask
    with pytest.raises(ValueError):
        remove_hydrogens(d)


def test_disable_h_reaches_the_host_loaders():
    """``--disable_H`` through main.create_loaders without a GPU: no hydrogen is left in any batch of the three loaders,
    and without the flag (or on a non-ADP dataset, as in the reference's loader.py) the crystals are what they were."""
    import main
    base = ["--synthetic", "12", "--atoms", "10", "16", "--batch", "4", "--dataset", "ADP"]

    def batches(extra):
        args = main.build_parser().parse_args(base + extra)
        main.fill_cfg(args)
        return [b for loader in main.create_loaders(args, 0, 1) for b in loader]
    with_h = batches([])
    assert any(bool((b.x == 1).any()) for b in with_h)
    no_h = batches(["--disable_H"])
    assert len(no_h) == len(with_h)
    for b in no_h:
        assert not bool((b.x == 1).any()) and bool(b.non_H_mask.all()) and b.y.shape[0] == b.x.shape[0]
    assert sum(b.y.shape[0] for b in no_h) == sum(b.y.shape[0] for b in with_h)
    other = batches(["--disable_H", "--dataset", "megnet"])
    assert any(bool((b.x == 1).any()) for b in other)
