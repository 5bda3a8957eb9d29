"""The two kernels of ``--predict --model icomformer`` and the reduced frame of an unlabeled shard, on the GPU:
``DeviceShard.frame_view`` (``cartnet_collate_frame_view``, csrc/collate.hip) against ``reduced.collate``,
``metrics.stored_frame`` (``cartnet_adp_stored_frame``, csrc/frame_ops.hip) against ``frame_mean`` with K = 1 and against
the host form of tests/model_frame_utils.py, ``with_optimized_cell()`` of an unlabeled shard against the labeled one's, and
both new calls under the poisoned allocator of tests/poison_utils.py.  Everything here is compared bit for bit."""
import numpy as np
import pytest
import torch

import model_frame_utils as mf
import poison_utils as pz

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _bare(d):
    """``d`` without its edges: a crystal the graph gave none."""
    out = d.__class__()
    out.__dict__.update(d.__dict__)
    out.edge_index = torch.zeros(2, 0, dtype=torch.int64)
    out.cart_dist, out.cart_dir = torch.zeros(0), torch.zeros(0, 3)
    return out


@pytest.fixture(scope="module")
def shards():
    """(stored, reduced) of the four crystals plus the second one without edges, labeled and unlabeled."""
    from cartnet_amd.shard import DeviceShard
    out = {}
    for labeled in (True, False):
        items = mf.crystals(labeled)
        stored = DeviceShard.from_data_list(items + [_bare(items[1])], DEV)
        assert stored.labeled == labeled
        out[labeled] = (stored, stored.with_optimized_cell())
    return out


def test_an_unlabeled_shard_gets_the_reduced_frame_of_the_labeled_one(shards):
    (lab, lab_red), (unl, unl_red) = shards[True], shards[False]
    assert not unl_red.labeled and "y" not in unl_red.t and unl_red.per_atom_target
    assert set(unl_red.t) == set(unl.t) | {"rotation", "basis"}
    for k in ("cell", "rotation", "basis", "cart_dir"):
        assert unl_red.t[k].dtype == lab_red.t[k].dtype and mf.bits(unl_red.t[k]) == mf.bits(lab_red.t[k]), k
    for k in unl.t:                                                           # owns what the frame changes, shares the rest
        assert (unl_red.t[k].data_ptr() != unl.t[k].data_ptr()) == (k in ("cell", "cart_dir")), k
    for k in ("atom_ptr", "edge_ptr", "y_ptr"):
        assert np.array_equal(getattr(unl_red, k), getattr(unl, k))
    # what the CPU check of the fixture promises, on the device: the stored-reduced crystal keeps its basis and its frame
    basis, rot = unl_red.t["basis"].cpu().view(-1, 3, 3), unl_red.t["rotation"].cpu().view(-1, 3, 3)
    eye = torch.eye(3)
    assert torch.equal(basis[mf.REDUCED_IN_PLACE], eye.to(torch.int8)) and float((rot[0] - eye).abs().max()) <= 1e-6
    for g in mf.UNREDUCED:
        assert not torch.equal(basis[g].abs(), eye.to(torch.int8)) and float((rot[g] - eye).abs().max()) > 0.1
    from cartnet_amd.data import lattice_basis
    for g, d in enumerate(mf.crystals(False)):
        assert torch.equal(basis[g].to(torch.int64), lattice_basis(d.cell[0])), g
    # two runs, the same bytes; and a batch of the reduced unlabeled shard is the labeled one's but for y
    again = unl.with_optimized_cell()
    for k in ("cell", "rotation", "basis", "cart_dir"):
        assert mf.bits(again.t[k]) == mf.bits(unl_red.t[k]), k
    a, b = unl_red.collate([3, 0, 4, 1], temp_mean=mf.TEMP_MEAN, temp_std=mf.TEMP_STD), \
        lab_red.collate([3, 0, 4, 1], temp_mean=mf.TEMP_MEAN, temp_std=mf.TEMP_STD)
    for k in ("x", "batch", "ptr", "edge_index", "cart_dist", "cart_dir", "cell", "temperature", "pos", "non_H_mask"):
        assert mf.bits(getattr(a, k)) == mf.bits(getattr(b, k)), k
    assert tuple(a.y.shape) == tuple(b.y.shape) and not bool(a.y.any())


SELECTIONS = ([2, 0, 3, 1], [1, 1, 3], [4, 0, 4, 2], [4], [3, 2, 1, 0, 4, 2])       # shuffled, repeated, without edges


@pytest.mark.parametrize("labeled", [True, False])
def test_frame_view_has_the_bits_of_the_reduced_collate(shards, labeled):
    stored, reduced = shards[labeled]
    for sel in SELECTIONS:
        batch = stored.collate(sel, temp_mean=mf.TEMP_MEAN, temp_std=mf.TEMP_STD)
        before = {k: (v.data_ptr(), mf.bits(v)) for k, v in batch.__dict__.items() if torch.is_tensor(v)}
        view = reduced.frame_view(batch)
        want = reduced.collate(sel, temp_mean=mf.TEMP_MEAN, temp_std=mf.TEMP_STD)
        assert view is not batch and type(view) is type(batch) and view.num_graphs == batch.num_graphs == len(sel)
        for k in ("cart_dir", "cell"):
            got = getattr(view, k)
            assert got.dtype == torch.float32 and got.shape == getattr(want, k).shape, (sel, k)
            assert mf.bits(got) == mf.bits(getattr(want, k)), (sel, k)
            assert got.numel() == 0 or got.data_ptr() != getattr(batch, k).data_ptr()
        assert tuple(view.rotation.shape) == (len(sel), 3, 3)
        assert mf.bits(view.rotation) == mf.bits(reduced.t["rotation"][torch.tensor(sel, device=DEV)])
        for k, (ptr, raw) in before.items():                                  # batch is not modified, the rest is shared
            assert getattr(batch, k).data_ptr() == ptr and mf.bits(getattr(batch, k)) == raw, (sel, k)
            if k not in ("cart_dir", "cell"):
                assert getattr(view, k).data_ptr() == ptr, (sel, k)
        assert not hasattr(batch, "rotation")
        # everything else the model reads of the reduced collate is what the stored batch holds already; y, which only
        # sizes the output, stays the stored batch's (a labeled reduced shard holds R^T y R)
        for k in ("x", "batch", "ptr", "edge_index", "cart_dist", "temperature", "pos", "non_H_mask"):
            assert mf.bits(getattr(view, k)) == mf.bits(getattr(want, k)), (sel, k)
        assert view.y.shape == want.y.shape and (mf.bits(view.y) == mf.bits(want.y)) == (not labeled or len(want.y) == 0)
        again = reduced.frame_view(batch)                                     # two runs, the same bytes
        assert mf.bits(again.cart_dir) == mf.bits(view.cart_dir) and mf.bits(again.cell) == mf.bits(view.cell)
    # the frame changes what it should: an unreduced crystal's directions and cell differ from the stored ones
    batch = stored.collate([1])
    view = reduced.frame_view(batch)
    assert not torch.equal(view.cart_dir, batch.cart_dir) and not torch.equal(view.cell, batch.cell)
    assert torch.allclose(view.cart_dir, batch.cart_dir @ view.rotation[0], atol=1e-6)


def test_frame_view_refuses_what_it_cannot_serve(shards):
    from cartnet_amd.data import Batch
    from cartnet_amd.shard import DeviceShard
    stored, reduced = shards[False]
    batch = stored.collate([0, 1])
    with pytest.raises(ValueError, match="carries no rotation"):
        stored.frame_view(batch)
    with pytest.raises(ValueError, match="another atom or edge count"):
        reduced.without_hydrogens().frame_view(batch)                         # another graph of the same crystals
    # the same totals, other crystals: crystal 1 and its copy without edges, swapped
    two = DeviceShard.from_data_list([_bare(mf.crystals(False)[1]), mf.crystals(False)[1]], DEV).with_optimized_cell()
    other = DeviceShard.from_data_list([mf.crystals(False)[1], _bare(mf.crystals(False)[1])], DEV)
    with pytest.raises(ValueError, match="another atom or edge count"):
        two.frame_view(other.collate([0, 1]))
    empty = other.collate([0])
    empty._sel, empty.num_graphs = empty._sel[:0], 0
    with pytest.raises(ValueError, match="holds no crystal"):
        two.frame_view(empty)
    with pytest.raises(ValueError, match="not collated from a resident shard"):
        reduced.frame_view(Batch.from_data_list(mf.crystals(True)[:2]).to(DEV))
    small = DeviceShard.from_data_list(mf.crystals(False)[:2], DEV).with_optimized_cell()
    with pytest.raises(ValueError, match="not crystals of this shard"):
        small.frame_view(stored.collate([3]))


def _case(M_per, T, seed):
    """Random rows for crystals of ``M_per`` rows at T temperatures, with one random rotation per crystal."""
    from cartnet_amd.shard import random_rotations
    g = torch.Generator(device=DEV).manual_seed(seed)
    row_ptr = torch.tensor([0] + list(M_per), dtype=torch.int64).cumsum(0).to(DEV)
    M = int(sum(M_per))
    pred = torch.randn(T * M, 3, 3, generator=g, device=DEV)
    return pred, random_rotations(len(M_per), g, DEV), row_ptr, M


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("rows", [(5, 0, 7), (0, 1, 0, 0), (300, 0, 1024, 1, 731, 0)])     # empty crystals; over one tile
def test_stored_frame_against_frame_mean_and_the_host_form(T, rows):
    from cartnet_amd.metrics import frame_mean, stored_frame
    pred, R, row_ptr, M = _case(rows, T, 50 + T)
    out = stored_frame(pred, R, row_ptr, T)
    assert out.dtype == torch.float32 and tuple(out.shape) == (T * M, 3, 3) and out.data_ptr() != pred.data_ptr()
    for t in range(T):                                                        # per slice: the frame mean of one frame
        fm = frame_mean(pred[t * M:(t + 1) * M], R.view(1, -1, 3, 3), row_ptr, stats=False)
        assert mf.bits(out[t * M:(t + 1) * M]) == mf.bits(fm.mean), t
        assert not bool(fm.spread.any())
    if M <= 64:                                                               # and the host form's bits
        want = mf.stored_frame_host(pred.cpu().numpy(), R.cpu().numpy(), row_ptr.cpu().numpy(), T)
        assert mf.bits(out) == want.tobytes()
    assert mf.bits(stored_frame(pred, R, row_ptr, T)) == mf.bits(out)         # two runs, the same bytes
    # the identity gives pred's bits
    eye = torch.eye(3, device=DEV).repeat(len(rows), 1, 1)
    assert mf.bits(stored_frame(pred, eye, row_ptr, T)) == mf.bits(pred)
    # a NaN row stays NaN and spoils no neighbour
    bad = pred.clone()
    r = (T - 1) * M + M // 2
    bad[r, 1, 2] = float("nan")
    got = stored_frame(bad, R, row_ptr, T)
    assert bool(torch.isnan(got[r]).all())
    keep = torch.arange(T * M, device=DEV) != r
    assert mf.bits(got[keep]) == mf.bits(out[keep])


def test_stored_frame_argument_checks_and_the_empty_case():
    from cartnet_amd.metrics import stored_frame
    pred, R, row_ptr, M = _case((5, 0, 7), 3, 70)
    with pytest.raises(ValueError, match="no multiple of the 2 slices"):
        stored_frame(pred[:35], R, row_ptr, 2)
    with pytest.raises(ValueError, match="rot must be"):
        stored_frame(pred, R[:2], row_ptr, 3)
    with pytest.raises(ValueError, match="pred"):
        stored_frame(pred.double(), R, row_ptr, 3)
    none = stored_frame(pred[:0], R, torch.zeros(4, dtype=torch.int64, device=DEV), 1)
    assert tuple(none.shape) == (0, 3, 3)


def test_both_calls_do_not_depend_on_the_bytes_of_their_fresh_buffers(shards):
    """``frame_view`` and ``stored_frame`` with every ``torch.empty`` of theirs filled with 0x00 and with 0xFF (NaN as a
    float, -1 as an integer): the same bytes come out, so every output cell is written and nothing unwritten is read."""
    from cartnet_amd.metrics import stored_frame
    stored, reduced = shards[False]
    batch = stored.collate([4, 0, 4, 2, 1], temp_mean=mf.TEMP_MEAN, temp_std=mf.TEMP_STD)      # made outside the fills

    def view():
        v = reduced.frame_view(batch)
        return {"cart_dir": v.cart_dir, "cell": v.cell, "rotation": v.rotation}
    (a, ra), (b, rb) = pz.under_both(view)
    for rec in (ra, rb):
        pz.assert_live(rec, [], "frame_view", workspace=False)
        assert rec.count >= 2                                                 # cart_dir and cell
    pz.assert_same_bytes(a, b, "frame_view")
    assert not bool(torch.isnan(b["cart_dir"]).any()) and not bool(torch.isnan(b["cell"]).any())

    pred, R, row_ptr, _ = _case((300, 0, 1024, 1, 731, 0), 3, 90)
    (a, ra), (b, rb) = pz.under_both(lambda: {"out": stored_frame(pred, R, row_ptr, 3)})
    for rec in (ra, rb):
        pz.assert_live(rec, [], "stored_frame", workspace=False)
    pz.assert_same_bytes(a, b, "stored_frame")
    assert not bool(torch.isnan(b["out"]).any())

    (a, ra), (b, rb) = pz.under_both(lambda: {k: v for k, v in stored.with_optimized_cell().t.items()
                                              if k in ("cell", "rotation", "basis", "cart_dir")})
    for rec in (ra, rb):
        pz.assert_live(rec, [], "with_optimized_cell (unlabeled)", workspace=False)
    pz.assert_same_bytes(a, b, "with_optimized_cell (unlabeled)")
