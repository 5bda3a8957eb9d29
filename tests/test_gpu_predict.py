"""``cartnet_amd.predict.predict_adps`` on unlabeled shards: the forward does not read ``y``, so an unlabeled shard gives
the bits of the labeled pass over the same crystals; batch sizes agree within the bound DESIGN.md §2.4 states; --disable_H
keeps one row per non-hydrogen atom."""
import pytest
import torch

import predict_utils as pu
from conftest import rel_err

pytestmark = pytest.mark.gpu

BATCH_TOL = 2 * 1e-5     # a crystal's prediction across batch sizes, norm-wise


@pytest.fixture(scope="module")
def shards():
    """The six crystals as resident geometry-only shards, labeled and not."""
    from cartnet_amd.shard import DeviceShard
    names = [f"c{g}" for g, _, _ in pu.SIX]
    lab = DeviceShard.from_data_list(pu.six_crystals(True))
    unl = DeviceShard.from_data_list(pu.six_crystals(False))
    unl.names = names
    assert lab.labeled and not unl.labeled and not lab.has_graph and not unl.has_graph
    assert "y" not in unl.t and unl.y_ptr.tolist() == lab.y_ptr.tolist() and unl.per_atom_target
    assert torch.equal(unl.t["non_h_mask"], lab.t["non_h_mask"])            # derived from z
    return lab, unl


def _setup(extra):
    """cfg and a fresh tiny model in eval mode, as main.py builds them (the synthetic temperatures are standardised already:
    --no_standarize_temp)."""
    import main as entry
    from cartnet_amd.master import create_model
    entry.fill_cfg(entry.build_parser().parse_args(["--dim_in", "32", "--no_standarize_temp"] + extra))
    torch.manual_seed(0)
    return entry, create_model().eval()


def _loader(entry, shard, n):
    from cartnet_amd.shard import ShardLoader
    (s,), (mean, std) = entry.shard_recipe([shard])
    return ShardLoader(s, n, temp_mean=mean, temp_std=std)


def _labeled_pass(model, loader):
    out = []
    with torch.no_grad():
        for b in loader:
            pred, true = model(b)
            assert true.shape == pred.shape
            out.append(pred.cpu())
    return torch.cat(out)


@pytest.fixture(autouse=True)
def _restore_cfg():
    yield
    from cartnet_amd.config import set_cfg
    set_cfg()


@pytest.mark.parametrize("extra,n", [(["--num_layers", "2"], 4), (["--num_layers", "2"], 1), (["--model", "ecomformer"], 3)])
def test_unlabeled_shard_gives_the_bits_of_the_labeled_pass(shards, extra, n):
    from cartnet_amd.predict import predict_adps
    lab, unl = shards
    entry, model = _setup(extra)
    want = _labeled_pass(model, _loader(entry, lab, n))
    res = predict_adps(model, _loader(entry, unl, n), "cuda:0")
    counts = pu.non_h_counts()
    assert res["name"] == [f"c{g}" for g, _, _ in pu.SIX]
    assert [int(t.shape[0]) for t in res["u_cart"]] == counts == [int(t.shape[0]) for t in res["u_cif"]]
    assert torch.equal(torch.cat(res["u_cart"]), want)
    crystals = pu.six_crystals(False)
    for k, d in enumerate(crystals):
        assert torch.equal(res["z"][k], d.x) and torch.equal(res["atoms"][k], d.x[d.x != 1])
        assert torch.equal(res["cell"][k], d.cell[0])
        # fp32 inverse and two products on positions of up to ~15 A in a cell of condition number < 10: a few 1e-5
        assert torch.allclose(res["frac"][k] @ d.cell[0], d.pos, atol=1e-4)
        assert tuple(res["axes"][k].shape) == (counts[k], 3, 3) and tuple(res["principal"][k].shape) == (counts[k], 3)
        assert res["stats"][k].dtype == torch.float64 and res["stats"][k][0].item() == pytest.approx(
            res["u_eq"][k].double().sum().item(), rel=1e-12)
        # "as stored"
        assert res["temp"][k] == pytest.approx(float(d.temperature), rel=1e-6)
        # u_eq is a third of the Cartesian trace, whatever the cell
        tr = res["u_cart"][k].double().diagonal(dim1=1, dim2=2).sum(1) / 3
        assert torch.allclose(res["u_eq"][k].double(), tr, rtol=2e-7, atol=0)


def test_batch_sizes_agree_within_the_stated_bound(shards):
    from cartnet_amd.predict import predict_adps
    _, unl = shards
    entry, model = _setup(["--num_layers", "2"])
    one = predict_adps(model, _loader(entry, unl, 1), "cuda:0")
    four = predict_adps(model, _loader(entry, unl, 4), "cuda:0")
    for k in range(6):
        err = rel_err(four["u_cart"][k], one["u_cart"][k])
        print(f"crystal {k}: eval_batch 4 against 1: {err:.3e} (bound {BATCH_TOL:.1e})")
        assert err <= BATCH_TOL


def test_disable_h_keeps_one_row_per_non_hydrogen_atom(shards):
    from cartnet_amd.predict import predict_adps
    from cartnet_amd.shard import ShardLoader
    _, unl = shards
    entry, model = _setup(["--num_layers", "2", "--disable_H"])
    loader = _loader(entry, unl, 4)
    counts = pu.non_h_counts()
    assert loader.shard.atom_ptr.tolist() == loader.shard.y_ptr.tolist()      # every hydrogen is gone
    res = predict_adps(model, loader, "cuda:0")
    assert [int(t.shape[0]) for t in res["u_cart"]] == counts == [int(t.shape[0]) for t in res["z"]]
    assert all(bool((z != 1).all()) for z in res["z"]) and all(torch.equal(a, z) for a, z in zip(res["atoms"], res["z"]))
    assert all(bool(torch.isfinite(t).all()) for t in res["u_cif"])
    with pytest.raises(ValueError, match="unlabeled"):
        ShardLoader(loader.shard, 2, augment=True)
