"""The iComformer dataset recipe on the host: ``cartnet_amd.data.optimize_cell`` / ``optimize_lattice`` against the
reference's own ``DatasetADP.get(..., optimize_cell=True)`` (dataset/datasetADP.py:75-80, dataset/utils.py:366-452; fixture
tests/golden/optimize_cell.npz written by tests/golden/make_golden_optimize_cell.py), and the neighbour cap of
``make_crystal``.

Float budget: 1e-5 * max|reference| per array, the project's fp32 parity budget.  On cells whose candidates tie (group 2
of the fixture) the reference's result depends on its unstable argsort, so what is checked there is that the host rule's
output is a valid canonical description of the same lattice."""
import os

import numpy as np
import pytest
import torch

from cartnet_amd.data import (Data, lattice_basis, lattice_margins, optimize_cell, optimize_lattice,
                              remove_hydrogens)
from cartnet_amd.synthetic import make_crystal, neighbor_cap_mask

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "optimize_cell.npz")
KEYS = ("x", "pos", "edge_index", "cart_dist", "cart_dir", "y", "cell", "temperature", "non_H_mask")
FLOATS = ("cell", "cart_dir", "y")
BUDGET = 1e-5


def golden():
    z = np.load(GOLDEN)
    n = int(z["n_crystals"])
    ins = [Data(**{k: torch.from_numpy(z[f"in{i}_{k}"]) for k in KEYS}) for i in range(n)]
    outs = [{k: z[f"out{i}_{k}"] for k in KEYS + ("cell_og",)} for i in range(n)]
    meta = {k: z[k] for k in ("group", "partner", "unimodular", "hydrogens")}
    return ins, outs, meta


def host_transform(d: Data, hydrogens: bool = True) -> Data:
    return optimize_cell(d if hydrogens else remove_hydrogens(d))


def assert_close(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err, bound = float(np.abs(got - want).max()), BUDGET * float(np.abs(want).max())
    assert err <= bound, f"{what}: max deviation {err:.3e} > {bound:.3e}"


def assert_valid(old_cell, new_cell, R, what):
    """``new_cell`` is a canonical description of the lattice of ``old_cell`` in the frame ``R``."""
    old, new, R = (np.asarray(a, dtype=np.float64).reshape(3, 3) for a in (old_cell, new_cell, R))
    T = (new @ R) @ np.linalg.inv(old)                   # new_cell @ R = T @ old_cell: integer, unimodular
    assert np.abs(T - np.round(T)).max() < 1e-3, (what, T)
    assert abs(abs(np.linalg.det(np.round(T))) - 1.0) < 1e-9, (what, T)
    assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-5 and np.linalg.det(R) > 0, (what, R)
    scale = np.abs(new).max()
    assert max(abs(new[0, 1]), abs(new[0, 2]), abs(new[1, 2])) <= 1e-5 * scale, (what, new)
    assert (np.diag(new) > 0).all(), (what, new)
    norms = np.linalg.norm(new, axis=1)
    assert norms[0] <= norms[1] * (1 + 1e-6) and norms[1] <= norms[2] * (1 + 1e-6), (what, norms)
    for r in (1, 2):
        assert new[0] @ new[r] >= -1e-5 * norms[r] ** 2, (what, r, new)


def test_fixture_covers_what_it_should():
    ins, outs, meta = golden()
    group = meta["group"]
    assert (group == 0).sum() >= 8 and (group == 1).sum() == (group == 0).sum()
    assert (group == 2).sum() == 7 and (group == 3).sum() >= 1
    assert len({tuple(u.reshape(-1)) for u, g in zip(meta["unimodular"], group) if g == 1}) == 5
    for i in np.flatnonzero(group <= 1):
        gap, cos = lattice_margins(ins[i].cell[0])
        assert gap > 1e-3 and cos > 1e-2, (i, gap, cos)
    for i in np.flatnonzero(group == 1):                 # a re-description: the same lattice, the same atoms and edges
        p, u = int(meta["partner"][i]), meta["unimodular"][i]
        assert abs(round(float(np.linalg.det(u)))) == 1
        assert torch.equal(ins[i].edge_index, ins[p].edge_index) and torch.equal(ins[i].pos, ins[p].pos)
        assert not torch.equal(ins[i].cell, ins[p].cell)
    # exactly orthogonal chosen vectors are in the fixture: acos(0) is not above pi / 2 in fp32, the reference keeps them
    assert any(float(lattice_margins(ins[i].cell[0])[1]) == 0.0 for i in np.flatnonzero(group == 2))
    for i in np.flatnonzero(group == 3):
        assert not meta["hydrogens"][i] and outs[i]["x"].shape[0] < ins[i].x.shape[0]
    assert all(7 <= d.x.shape[0] <= 40 for d in ins)


def test_optimize_cell_matches_the_reference_on_generic_cells():
    ins, outs, meta = golden()
    seen = 0
    for i in np.flatnonzero(meta["group"] != 2):
        d, want = ins[i], outs[i]
        before = {k: getattr(d, k).clone() for k in KEYS}
        got = host_transform(d, bool(meta["hydrogens"][i]))
        for k in KEYS:
            g = getattr(got, k).numpy()
            assert g.dtype == want[k].dtype and g.shape == want[k].shape, (i, k, g.dtype, g.shape, want[k].shape)
            if k in FLOATS:
                assert_close(g, want[k], (i, k))
            else:
                assert g.tobytes() == want[k].tobytes(), (i, k)
            assert torch.equal(getattr(d, k), before[k]), f"crystal {i}: input {k} was modified"
        assert got.cell_og.numpy().tobytes() == want["cell_og"].tobytes() == d.cell.numpy().tobytes()
        seen += 1
    assert seen >= 17


def test_redescribed_cells_give_the_same_crystal():
    ins, _, meta = golden()
    for i in np.flatnonzero(meta["group"] == 1):
        a, b = optimize_cell(ins[int(meta["partner"][i])]), optimize_cell(ins[i])
        for k in FLOATS:
            assert_close(getattr(b, k).numpy(), getattr(a, k).numpy(), (i, k))


def test_special_cells_get_a_valid_canonical_lattice():
    ins, _, meta = golden()
    for i in np.flatnonzero(meta["group"] == 2):
        cell = ins[i].cell[0]
        new_cell, R = optimize_lattice(cell)
        assert_valid(cell, new_cell, R, i)
        b = lattice_basis(cell)
        assert abs(round(float(torch.det(b.to(torch.float64))))) == 1
        np.testing.assert_allclose((new_cell @ R).numpy(), (b.to(torch.float32) @ cell).numpy(), atol=1e-5 * float(cell.abs().max()))
        got = optimize_cell(ins[i])
        assert_close(got.cart_dir.numpy(), (ins[i].cart_dir.double() @ R.double()).numpy(), (i, "cart_dir"))
        assert_close(got.y.numpy(), (R.double().T @ ins[i].y.double() @ R.double()).numpy(), (i, "y"))
    # and on every other cell of the fixture
    for i in np.flatnonzero(meta["group"] != 2):
        assert_valid(ins[i].cell[0], *optimize_lattice(ins[i].cell[0]), i)


def test_basis_is_the_selection_behind_optimize_lattice():
    ins, _, _ = golden()
    for i, d in enumerate(ins):
        cell = d.cell[0]
        b = lattice_basis(cell)
        assert b.dtype == torch.int64 and int(b.abs().max()) <= 2
        new_cell, R = optimize_lattice(cell)
        v = b.to(torch.float64) @ cell.to(torch.float64)
        assert float(torch.det(v)) > 0                                  # right-handed
        assert_close((new_cell.double() @ R.double()).numpy(), v.numpy(), i)


def test_scalar_targets_are_left_alone():
    d = make_crystal(620, 9, adp=False)
    out = optimize_cell(d)
    assert torch.equal(out.y, d.y) and not torch.equal(out.cart_dir, d.cart_dir)
    assert tuple(out.cell.shape) == (1, 3, 3) and torch.equal(out.cell_og, d.cell)


def test_degenerate_cell_raises_value_error():
    d = make_crystal(621, 8)
    d.cell = torch.tensor([[[4.0, 0.0, 0.0], [8.0, 0.0, 0.0], [0.0, 0.0, 5.0]]])      # two collinear vectors
    with pytest.raises(ValueError, match="crystal number-621"):
        optimize_cell(d, name="number-621")
    with pytest.raises(ValueError):
        optimize_lattice(d.cell[0])
    with pytest.raises(ValueError):
        optimize_lattice(torch.tensor([[4.0, 0.0, 0.0], [0.0, 5.0, 0.0], [4.0, 5.0, 0.0]]))   # coplanar
    assert lattice_margins(d.cell[0]) == (0.0, 0.0)


@pytest.mark.parametrize("k", [4, 8, 12])
def test_make_crystal_with_a_cap_is_the_cap_mask_on_the_uncapped_crystal(k):
    """The cap keeps, per target with more than k edges, those within the (k+1)-th smallest squared distance + 0.01
    (dataset/utils.py:240-360).  The squared distances are recomputed from ``cart_dist`` here; they differ from the
    builder's own by rounding (1e-7 relative), five orders of magnitude below the tolerance that separates kept from
    dropped edges."""
    n = 20
    full, capped = make_crystal(630, n), make_crystal(630, n, max_neighbors=k)
    tgt = full.edge_index[1]
    assert int(torch.bincount(tgt, minlength=n).max()) > k                # the cap bites
    keep = neighbor_cap_mask(tgt, full.cart_dist ** 2, n, k)
    assert 0 < int(keep.sum()) < keep.shape[0]
    assert torch.equal(capped.edge_index, full.edge_index[:, keep])
    assert torch.equal(capped.cart_dist, full.cart_dist[keep]) and torch.equal(capped.cart_dir, full.cart_dir[keep])
    for key in ("x", "pos", "cell", "y", "non_H_mask", "temperature"):
        assert torch.equal(getattr(capped, key), getattr(full, key)), key
    assert int(torch.bincount(capped.edge_index[1], minlength=n).min()) >= min(k, int(torch.bincount(tgt).min()))
    assert torch.equal(make_crystal(630, n, max_neighbors=None).edge_index, full.edge_index)     # the default: uncapped


def test_icomformer_loaders_get_capped_canonical_crystals_and_cartnet_loaders_do_not_change():
    """main.create_loaders on the host path: --model icomformer builds capped graphs in the canonical frame (the order of
    the reference: cap on the full crystal, hydrogen removal, canonicalisation); --model CartNet is what it was."""
    import main

    def batches(extra):
        args = main.build_parser().parse_args(["--synthetic", "10", "--atoms", "14", "20", "--batch", "5"] + extra)
        main.fill_cfg(args)
        return [b for loader in main.create_loaders(args, 0, 1) for b in loader]
    icf = batches(["--model", "icomformer", "--max_neighbours", "6"])
    cn = batches([])
    assert sum(b.num_graphs for b in icf) == sum(b.num_graphs for b in cn) == 10
    for b in icf:
        c = b.cell
        assert float(torch.stack((c[:, 0, 1], c[:, 0, 2], c[:, 1, 2])).abs().max()) <= 1e-5 * float(c.abs().max())
        assert bool((torch.diagonal(c, dim1=1, dim2=2) > 0).all())
    assert sum(b.edge_index.shape[1] for b in icf) < sum(b.edge_index.shape[1] for b in cn)
    want = [make_crystal(g, None, 5.0, (14, 20)) for g in range(10)]
    perm = torch.randperm(10, generator=torch.Generator().manual_seed(123)).tolist()
    assert torch.equal(cn[-1].cell, want[perm[-1]].cell) and torch.equal(cn[-1].cart_dir, want[perm[-1]].cart_dir)
    # hydrogen removal composes: the capped graph loses edges, then the frame is applied
    noh = batches(["--model", "icomformer", "--max_neighbours", "6", "--disable_H"])
    assert all(not bool((b.x == 1).any()) for b in noh)
    assert sum(b.edge_index.shape[1] for b in noh) < sum(b.edge_index.shape[1] for b in icf)
    # another dataset name: no canonical frame (loader/loader.py:24 is the ADP branch)
    other = batches(["--model", "icomformer", "--dataset", "megnet"])
    assert any(float(b.cell[:, 0, 1].abs().max()) > 1e-3 for b in other)
