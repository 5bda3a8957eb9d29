"""``cartnet_molecules`` (csrc/molecule_ops.hip) against ``bonds.molecules_host`` on graphs from
``graph.radius_graph_pbc``: labels, numbering, sizes, status and the per-crystal counts exactly, the unwrapped positions
within 1e-12 A (the kernel takes the same fp64 additions along the same edges), two runs with equal bytes."""
import numpy as np
import pytest
import torch

import molecule_utils as mu
from test_gpu_bond_test import _make, _random_crystal

pytestmark = pytest.mark.gpu

BIG = mu.cubic(100.0)


def _check(batch, row_ptr, trivial=False, tol=mu.TOL):
    """Runs the kernel, compares everything with the host rule, returns (result, reference)."""
    from cartnet_amd import metrics as gm
    res = gm.molecules(batch, row_ptr, tol, rows=int(row_ptr[-1]))
    ref, margin, gaps = mu.host_molecules(batch, tol)
    # conditions on the inputs: the case must not pass vacuously, and no decision may hang on a rounding
    assert trivial or ref["size"].max() >= 2
    assert margin > 1e-5
    assert ((gaps < 1e-6) | (gaps > 1.0)).all()
    print(f"sweeps per crystal {ref['sweeps'].tolist()}, bond margin {margin:.3e}, closure gaps below 1e-6: "
          f"{int((gaps < 1e-6).sum())}, above 1: {int((gaps > 1.0).sum())}")
    got = {k: getattr(res, k).cpu().numpy() for k in res._fields}
    assert got["label"].dtype == np.int64 and got["x"].dtype == np.float64 and got["crystal_counts"].dtype == np.float64
    assert all(got[k].dtype == np.int32 for k in ("mol", "size", "status"))
    for k in ("label", "mol", "size", "status", "crystal_counts"):
        assert got[k].shape == ref[k].shape and np.array_equal(got[k], ref[k]), k
    err = np.abs(got["x"] - ref["x"]).max() if got["x"].size else 0.0
    print(f"x: max error {err:.3e} A against 1e-12")
    assert got["x"].shape == ref["x"].shape and err <= 1e-12
    again = gm.molecules(batch, row_ptr, tol, rows=int(row_ptr[-1]))
    for a, b in zip(res, again):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()         # two runs, equal bytes
    return res, ref


def test_an_empty_crystal_first_a_single_atom_and_a_ring():
    single = (np.array([[1.0, 2.0, 3.0]]), mu.cubic(12.0), np.array([6]))
    benzene = (mu.ring([7.0, 7.0, 7.0]), mu.cubic(15.0), np.full(6, 6))
    res, ref = _check(*_make([_random_crystal(0, 3, 1), single, benzene], 1)[::2])
    assert ref["label"].tolist() == [-1, -1, -1, 3] + [4] * 6 and ref["size"].tolist() == [1] + [6] * 6
    assert res.crystal_counts.tolist() == [[0.0] * 5, [1.0, 0.0, 0.0, 0.0, 1.0], [1.0, 1.0, 0.0, 0.0, 6.0]]
    assert res.status.tolist() == [0] * 7 and float(res.x[:4].abs().max()) == 0.0
    # a single atom alone: no edge at all
    alone, _ = _check(*_make([single], 2)[::2], trivial=True)
    assert alone.label.tolist() == [0] and alone.mol.tolist() == [0] and alone.size.tolist() == [1]


@pytest.mark.parametrize("reverse", [False, True])
def test_a_chain_of_70_takes_a_sweep_per_atom(reverse):
    """Numbered along the chain the lowest label travels one hop per sweep: 69 sweeps that change something and one that
    does not, the most a molecule of 70 can need.  Numbered from the far end it is the same molecule, rooted at the other
    end."""
    pos, true = mu.chain(70, (5.0, 50.0, 50.0), BIG, drift=(0.0, 0.05), reverse=reverse)
    res, ref = _check(*_make([(pos, BIG, np.full(70, 6))], 3)[::2])
    assert ref["sweeps"].tolist() == [70] and ref["size"].tolist() == [70] * 70 and ref["status"].tolist() == [0] * 70
    assert np.abs(res.x.cpu().numpy() - (true - true[0])).max() < 1e-3       # the geometry itself, at fp32 accuracy
    assert res.crystal_counts.tolist() == [[1.0, 1.0, 0.0, 0.0, 70.0]]


def test_the_chain_across_two_cell_faces_is_not_periodic():
    pos, true = mu.chain(70, (60.0, 98.0, 50.0), BIG, drift=(0.1, 0.0))
    assert (np.abs(pos - true).max(axis=0) > 50).tolist() == [True, True, False]      # wrapped in x and in y
    res, ref = _check(*_make([(pos, BIG, np.full(70, 6))], 4)[::2])
    assert ref["status"].tolist() == [0] * 70 and ref["size"].tolist() == [70] * 70
    assert np.abs(res.x.cpu().numpy() - (true - true[0])).max() < 1e-3       # unwrapped through both faces


def test_a_polymer_through_the_face_is_periodic():
    from cartnet_amd.bonds import MOLECULE_PERIODIC
    res, ref = _check(*_make([mu.polymer(8), (mu.ring([7.0, 7.0, 7.0]), mu.cubic(15.0), np.full(6, 6))], 5)[::2])
    assert ref["status"].tolist() == [MOLECULE_PERIODIC] * 8 + [0] * 6
    assert res.crystal_counts.tolist() == [[1.0, 0.0, 1.0, 0.0, 8.0], [1.0, 1.0, 0.0, 0.0, 6.0]]


def test_more_atoms_than_the_workgroup_has_threads():
    """Fifteen chains of 20 in one cell, their 300 atoms interleaved by a fixed permutation: every thread of the crystal's
    workgroup owns more than one atom (the one size-dependent step of the kernel), and no molecule's atoms are neighbours
    in atom order."""
    cell = mu.cubic(30.0)
    pos = np.concatenate([mu.chain(20, (2.0, 2.0 + 5.5 * a, 3.0 + 9.0 * b), cell)[0] for a in range(5) for b in range(3)])
    perm = np.random.default_rng(9).permutation(300)
    res, ref = _check(*_make([(pos[perm], cell, np.full(300, 6))], 9)[::2])
    assert res.crystal_counts.tolist() == [[15.0, 15.0, 0.0, 0.0, 20.0]] and ref["size"].tolist() == [20] * 300
    chain_of = perm // 20                                                     # the chain of the atom now at each index
    label = res.label.cpu().numpy()
    assert all(len(set(label[chain_of == c])) == 1 for c in range(15)) and len(set(label)) == 15


def test_a_random_crystal_with_interleaved_hydrogens():
    """Uniformly random atoms at ``_random_crystal``'s density: accidental clusters, periodic and plain ones mixed, the
    hydrogens interleaved so that an atom's index is not its row."""
    from cartnet_amd.bonds import MOLECULE_PERIODIC
    batch, _, row_ptr = _make([_random_crystal(60, 20, 23)], 6)
    mask = batch["non_H_mask"].cpu().numpy()
    assert not np.array_equal(np.nonzero(mask)[0], np.arange(mask.sum()))
    res, ref = _check(batch, row_ptr)
    assert (ref["status"] == MOLECULE_PERIODIC).any() and ((ref["status"] == 0) & (ref["size"] >= 2)).any()
    assert (ref["label"][~mask] == -1).all() and len(np.unique(ref["mol"])) == int(ref["crystal_counts"][0, 0]) > 2


def test_a_deleted_direction_opens_both_molecules_and_leaves_the_others():
    from cartnet_amd.bonds import MOLECULE_OPEN
    five, _ = mu.chain(5, (3.0, 3.0, 3.0), mu.cubic(30.0))
    crystal = (np.concatenate([five, mu.ring([15.0, 15.0, 15.0]), mu.chain(3, (3.0, 20.0, 20.0), mu.cubic(30.0))[0]]),
               mu.cubic(30.0), np.full(14, 6))
    batch, _, row_ptr = _make([crystal], 7)
    whole, _ = _check(batch, row_ptr)
    assert whole.size.tolist() == [5] * 5 + [6] * 6 + [3] * 3 and whole.status.tolist() == [0] * 14
    src, tgt = batch["edge_index"]
    keep = ~((src == 1) & (tgt == 2))                                         # atom 2 never hears of atoms 0 and 1
    assert int((~keep).sum()) == 1
    cut = dict(batch, edge_index=batch["edge_index"][:, keep], cart_dist=batch["cart_dist"][keep],
               cart_dir=batch["cart_dir"][keep])
    res, ref = _check(cut, row_ptr)
    assert ref["label"].tolist() == [0, 0, 2, 2, 2] + [5] * 6 + [11] * 3
    assert res.status.tolist() == [MOLECULE_OPEN] * 5 + [0] * 9 and res.mol.tolist() == [0, 0, 1, 1, 1] + [2] * 6 + [3] * 3
    assert res.crystal_counts.tolist() == [[4.0, 2.0, 0.0, 2.0, 6.0]]
    for k in ("x", "size", "status"):                                         # the ring and the short chain: untouched
        assert torch.equal(getattr(res, k)[5:], getattr(whole, k)[5:]), k


def test_hydrogens_z_of_zero_and_z_beyond_the_table():
    """C - C(-H) - Cm... : the hydrogen has no row and no label, Z = 0 and Z = 97 have rows and never bond."""
    c = np.array([10.0, 10.0, 10.0])
    pos = np.stack([c + [0, 0, 1.0], c, c + [1.4, 0, 0], c + [0, 1.4, 0], c + [-1.4, 0, 0], c + [-1.4, 1.4, 0]])
    res, ref = _check(*_make([(pos, mu.cubic(20.0), np.array([1, 6, 0, 97, 6, 6]))], 8)[::2])
    assert ref["label"].tolist() == [-1, 1, 2, 3, 1, 1] and ref["size"].tolist() == [3, 1, 1, 3, 3]
    assert res.mol.tolist() == [0, 1, 2, 0, 0] and res.crystal_counts.tolist() == [[3.0, 1.0, 0.0, 0.0, 3.0]]


def test_a_batch_of_the_loader_and_argument_checks():
    from cartnet_amd import metrics as gm
    from cartnet_amd.synthetic import make_batch
    b = make_batch(3, 24)
    b.to("cuda:0")
    row_ptr = gm.target_row_ptr(b)
    view = {"x": b.x, "edge_index": b.edge_index, "cart_dist": b.cart_dist, "cart_dir": b.cart_dir,
            "non_H_mask": b.non_H_mask, "ptr": b.ptr}
    direct, of_view = gm.molecules(b, row_ptr), gm.molecules(view, row_ptr)
    for p, q in zip(direct, of_view):
        assert p.cpu().numpy().tobytes() == q.cpu().numpy().tobytes()
    assert tuple(direct.mol.shape) == (int(b.y.shape[0]),) and tuple(direct.x.shape) == (int(b.x.shape[0]), 3)
    with pytest.raises(ValueError, match="batch.ptr"):
        gm.molecules({k: v for k, v in view.items() if k != "ptr"}, row_ptr)
    with pytest.raises(ValueError, match="row_ptr"):
        gm.molecules(view, row_ptr.to(torch.int32))
    with pytest.raises(ValueError, match="crystals"):
        gm.molecules(view, row_ptr[:-1])
    with pytest.raises(ValueError, match="cart_dist"):
        gm.molecules(dict(view, cart_dir=b.cart_dir[:1]), row_ptr)
