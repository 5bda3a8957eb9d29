"""``metrics.batch_graph`` on CPU tensors: the two lookups against a numpy restatement, a ``BatchGraph`` handed back in,
the row count it was built for, and the messages of a batch that lacks what an analysis needs."""
import numpy as np
import pytest
import torch

from cartnet_amd import metrics


def _ragged():
    """Three crystals of 4, 0 and 5 atoms; atom 2 (in the middle) and atom 8 (the last) have no edge; hydrogens at 1, 4
    and 7, so an atom's index is not its row.  Edges sorted by target."""
    z = torch.tensor([6, 1, 8, 6, 1, 7, 6, 1, 6])
    tgt = [0, 0, 1, 3, 3, 3, 4, 5, 5, 6, 7, 7]
    src = [1, 3, 0, 0, 1, 1, 5, 4, 6, 5, 6, 5]
    E = len(tgt)
    rng = np.random.default_rng(0)
    return {"x": z, "edge_index": torch.tensor([src, tgt]), "cart_dist": torch.tensor(rng.random(E), dtype=torch.float32),
            "cart_dir": torch.tensor(rng.random((E, 3)), dtype=torch.float32), "non_H_mask": z != 1,
            "ptr": torch.tensor([0, 4, 4, 9])}


def test_the_lookups_equal_their_numpy_restatement():
    batch = _ragged()
    g = metrics.batch_graph(batch, 6)
    assert isinstance(g, metrics.BatchGraph) and (g.N, g.E, g.M, g.B) == (9, 12, 6, 3)
    mask, tgt = batch["non_H_mask"].numpy(), batch["edge_index"][1].numpy()
    assert g.atom_row.dtype == torch.int64 and g.seg_ptr.dtype == torch.int64
    assert np.array_equal(g.atom_row.numpy(), np.where(mask, np.cumsum(mask) - 1, -1))
    assert np.array_equal(g.seg_ptr.numpy(), np.searchsorted(tgt, np.arange(10), side="left"))
    assert g.seg_ptr.tolist() == [0, 2, 3, 3, 6, 7, 9, 10, 12, 12]           # empty segments at atoms 2 and 8
    assert g.atom_ptr.tolist() == [0, 4, 4, 9] and g.atom_ptr.dtype == torch.int64
    assert g.z is batch["x"] and g.mask is batch["non_H_mask"] and g.cart_dir is not None
    from cartnet_amd.bonds import COVALENT_RADII
    assert g.radii.dtype == torch.float32 and g.radii.tolist() == np.asarray(COVALENT_RADII, dtype=np.float32).tolist()
    # without rows given: the mask is counted; without a mask every atom has a row
    assert metrics.batch_graph(batch).M == 6
    bare = metrics.batch_graph({k: v for k, v in batch.items() if k != "non_H_mask"})
    assert bare.M == 9 and bare.mask is None and bare.atom_row.tolist() == list(range(9))


def test_a_batch_graph_comes_back_as_it_is_and_holds_its_row_count():
    g = metrics.batch_graph(_ragged(), 6)
    assert metrics.batch_graph(g) is g and metrics.batch_graph(g, 6, "bond_test", "u") is g
    with pytest.raises(ValueError, match="u holds 5 rows, the batch graph was built for 6"):
        metrics.batch_graph(g, 5, "bond_test", "u")
    no_dir = metrics.batch_graph(_ragged(), 6, need_dir=False)
    assert no_dir.cart_dir is None and metrics.batch_graph(no_dir, need_dir=False) is no_dir
    with pytest.raises(ValueError, match="cart_dir"):
        metrics.batch_graph(no_dir)


def test_the_messages_of_a_batch_that_lacks_something():
    batch = _ragged()
    with pytest.raises(ValueError, match="bond_test needs the atomic numbers in batch.x \\(a forward has overwritten them\\)"):
        metrics.batch_graph({k: v for k, v in batch.items() if k != "x"}, 6, "bond_test", "u")
    with pytest.raises(ValueError, match="riding_h needs the atomic numbers in batch.x"):
        metrics.batch_graph(dict(batch, x=torch.zeros(9, 8)), 6, "riding_h", "u_eq")
    with pytest.raises(ValueError, match="riding_h needs the crystals' atom offsets in batch.ptr"):
        metrics.batch_graph({k: v for k, v in batch.items() if k != "ptr"}, 6, "riding_h", "u_eq")
    assert metrics.batch_graph({k: v for k, v in batch.items() if k != "ptr"}, 6, need_ptr=False).atom_ptr is None
    with pytest.raises(ValueError, match="u holds 6 rows for 9 atoms and the batch has no non_H_mask"):
        metrics.batch_graph({k: v for k, v in batch.items() if k != "non_H_mask"}, 6, "bond_test", "u")
    with pytest.raises(ValueError, match="non_H_mask must be a tensor \\[N\\] on the data's device"):
        metrics.batch_graph(dict(batch, non_H_mask=batch["non_H_mask"][:3]), 6)
    with pytest.raises(ValueError, match="edge_index must be an int64 tensor \\[2,E\\] on the data's device"):
        metrics.batch_graph(dict(batch, edge_index=batch["edge_index"].to(torch.int32)), 6)
    with pytest.raises(ValueError, match="cart_dist \\[E\\] and cart_dir \\[E,3\\] must be fp32 tensors on the data's device"):
        metrics.batch_graph(dict(batch, cart_dir=batch["cart_dir"][:1]), 6)
    with pytest.raises(ValueError, match="cart_dist \\[E\\] must be an fp32 tensor on the data's device"):
        metrics.batch_graph(dict(batch, cart_dist=batch["cart_dist"][:1]), 6, need_dir=False)
