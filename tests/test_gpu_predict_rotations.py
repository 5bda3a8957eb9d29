"""``predict_adps(rotations=K)``: the replica batch against the collation kernel bit for bit, the frame mean against a
manual restatement (one forward per frame, ``R P R^T`` and the mean in fp64 on the host), the export and the site average
on the mean, the seed, and ``rotations=1`` against the pass as it was."""
import numpy as np
import pytest
import torch

import cif_utils as cu
from conftest import rel_err

pytestmark = pytest.mark.gpu

BATCH_TOL = 2 * 1e-5     # tests/test_gpu_predict.py:12: a crystal's prediction across batch compositions, norm-wise
K, EVAL_BATCH, SEED = 3, 2, 11


@pytest.fixture(scope="module")
def setup():
    """cfg, a fresh tiny model in eval mode, six unlabeled synthetic crystals of 10-30 atoms as a resident shard with the
    recipe applied, and the pass under test, run once: (entry, model, shard, (mean, std), result)."""
    import main as entry
    from cartnet_amd.config import set_cfg
    from cartnet_amd.master import create_model
    from cartnet_amd.predict import predict_adps
    from cartnet_amd.shard import DeviceShard
    from cartnet_amd.synthetic import make_geometry
    entry.fill_cfg(entry.build_parser().parse_args(["--dim_in", "32", "--num_layers", "2", "--no_standarize_temp"]))
    torch.manual_seed(0)
    model = create_model().eval()
    crystals = [make_geometry(700 + g, None, (10, 30)) for g in range(6)]
    for d in crystals:
        del d.y
    (shard,), norm = entry.shard_recipe([DeviceShard.from_data_list(crystals)])
    assert not shard.labeled and shard.has_graph
    res = predict_adps(model, _loader(shard, norm), "cuda:0", rotations=K, seed=SEED)
    yield entry, model, shard, norm, res
    set_cfg()


def _loader(shard, norm, n=EVAL_BATCH):
    from cartnet_amd.shard import ShardLoader
    return ShardLoader(shard, n, temp_mean=norm[0], temp_std=norm[1])


def _same(a, b):
    assert list(a) == list(b)
    for k in a:
        assert len(a[k]) == len(b[k]), k
        for x, y in zip(a[k], b[k]):
            if torch.is_tensor(x):
                assert x.dtype == y.dtype and x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), k
            else:
                assert x == y or (x != x and y != y), k


def test_replicate_equals_the_collation_kernel_bit_for_bit(setup):
    from cartnet_amd.predict import frames, replicate
    _, _, shard, norm, _ = setup
    gen = torch.Generator(device="cuda:0").manual_seed(3)
    for sel in ([4, 1], [2], [5, 0, 3]):
        B = len(sel)
        batch = shard.collate(sel, None, *norm)
        before = batch.clone()
        R = frames(B, K, gen, "cuda:0")
        assert torch.equal(R[0], torch.eye(3, device="cuda:0").expand(B, 3, 3)) and tuple(R.shape) == (K, B, 3, 3)
        rep = replicate(batch, K, R)
        col = shard.collate(list(sel) * K, R.view(K * B, 3, 3), *norm)
        assert rep.num_graphs == col.num_graphs == K * B
        for name in ("x", "batch", "ptr", "edge_index", "cart_dist", "cart_dir", "pos", "non_H_mask", "temperature"):
            a, b = getattr(rep, name), getattr(col, name)
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), name
        # the stored cell is repeated (the export works in the stored frame); the collation's augmentation rotates it
        assert rep.y.shape == col.y.shape and torch.equal(rep.cell, batch.cell.repeat(K, 1, 1))
        assert torch.equal(rep.cell[:B], col.cell[:B])
        for name in before.keys():
            v = getattr(before, name)
            if torch.is_tensor(v):
                assert torch.equal(v, getattr(batch, name)), name            # the input batch is as it was
        assert batch.x.dtype == torch.int64


def test_replicate_serves_a_batch_of_the_host_loader():
    from cartnet_amd.data import Batch, DataLoader
    from cartnet_amd.metrics import edge_row_ptr, rotate_rows
    from cartnet_amd.predict import frames, replicate
    from cartnet_amd.synthetic import make_crystal
    items = [make_crystal(800 + g, None, 5.0, (10, 30)) for g in range(3)]
    (batch,) = list(DataLoader(items, 3))
    batch.to("cuda:0")
    R = frames(3, 2, torch.Generator(device="cuda:0").manual_seed(1), "cuda:0")
    rep = replicate(batch, 2, R)
    want = Batch.from_data_list(items * 2).to("cuda:0")
    for name in ("x", "batch", "ptr", "edge_index", "cart_dist", "pos", "non_H_mask", "cell", "temperature", "y"):
        assert torch.equal(getattr(rep, name), getattr(want, name)), name
    assert torch.equal(rep.cart_dir, rotate_rows(want.cart_dir.contiguous(), edge_row_ptr(want), R.view(6, 3, 3)))
    assert torch.equal(rep.cart_dir[:batch.cart_dir.shape[0]], batch.cart_dir)            # frame 0 is the stored one


def test_one_rotation_is_the_pass_as_it_was(setup):
    from cartnet_amd.predict import KEYS, predict_adps
    _, model, shard, norm, _ = setup
    plain = predict_adps(model, _loader(shard, norm), "cuda:0")
    one = predict_adps(model, _loader(shard, norm), "cuda:0", rotations=1, seed=5)
    assert tuple(plain) == KEYS
    _same(plain, one)
    with pytest.raises(ValueError, match="rotations"):
        predict_adps(model, _loader(shard, norm), "cuda:0", rotations=0)


def test_the_mean_against_a_manual_restatement(setup):
    """Per batch of the same eval_batch, without replication: the stored frames, ``rotate_rows``, one forward per frame, then
    ``R P R^T`` and the mean in fp64 on the host."""
    from cartnet_amd.metrics import edge_row_ptr, rotate_rows
    from cartnet_amd.predict import KEYS, ROT_KEYS
    _, model, shard, norm, res = setup
    assert tuple(res) == KEYS + ROT_KEYS and len(res["name"]) == 6
    counts = [int(t.shape[0]) for t in res["u_cart"]]
    for c in range(6):
        assert tuple(res["frames"][c].shape) == (K, 3, 3) and torch.equal(res["frames"][c][0], torch.eye(3))
        assert tuple(res["rot_spread"][c].shape) == (counts[c],) and res["rot_stats"][c].dtype == torch.float64
        s = res["rot_spread"][c].double()
        assert res["rot_stats"][c][0].item() == pytest.approx(s.sum().item(), rel=1e-12)
        assert res["rot_stats"][c][1].item() == s.max().item()
    loader = _loader(shard, norm)
    at = 0
    with torch.no_grad():
        for sel in loader._batches():
            members = []
            for k in range(K):
                b = shard.collate(sel, None, *norm)
                Rk = torch.stack([res["frames"][at + j][k] for j in range(len(sel))]).cuda()
                b.cart_dir = rotate_rows(b.cart_dir, edge_row_ptr(b), Rk)
                members.append(model(b)[0].double().cpu())
            lo = 0
            for j in range(len(sel)):
                c, n = at + j, counts[at + j]
                R = res["frames"][c].double()                                              # [K,3,3]
                U = torch.stack([R[k] @ members[k][lo:lo + n] @ R[k].T for k in range(K)])   # [K,n,3,3]
                mean = U.mean(0)
                spread = (U - mean).abs().amax(dim=(0, 2, 3))
                err = rel_err(res["u_cart"][c], mean)
                scale = float(res["u_cart"][c].abs().max())
                serr = float((res["rot_spread"][c].double() - spread).abs().max())
                print(f"crystal {c}: u_cart against the restatement {err:.3e} (bound {BATCH_TOL:.1e}); rot_spread off by "
                      f"{serr:.3e} (bound {2 * BATCH_TOL * scale:.3e}), rot_spread max {float(spread.max()):.3e}")
                assert err <= BATCH_TOL
                assert serr <= 2 * BATCH_TOL * scale
                lo += n
            at += len(sel)
    assert at == 6


def test_the_export_derives_from_the_mean(setup):
    from cartnet_amd.metrics import adp_export
    _, _, _, _, res = setup
    counts = [int(t.shape[0]) for t in res["u_cart"]]
    row_ptr = torch.tensor([0] + counts, dtype=torch.int64).cumsum(0).cuda()
    ex = adp_export(torch.cat(res["u_cart"]).cuda(), row_ptr, torch.stack(res["cell"]).cuda())
    for name in ("u_cif", "u_eq", "principal", "axes"):
        assert torch.equal(torch.cat(res[name]), getattr(ex, name).cpu()), name


def test_the_seed_decides_the_frames(setup):
    from cartnet_amd.predict import predict_adps
    _, model, shard, norm, res = setup
    again = predict_adps(model, _loader(shard, norm), "cuda:0", rotations=K, seed=SEED)
    _same(res, again)
    other = predict_adps(model, _loader(shard, norm), "cuda:0", rotations=K, seed=SEED + 1)
    for c in range(6):
        assert torch.equal(other["frames"][c][0], torch.eye(3))
        assert not torch.equal(other["frames"][c][1:], res["frames"][c][1:])
    assert not torch.equal(res["frames"][0][1:], res["frames"][1][1:])       # one draw per crystal, not one per batch


def test_the_site_average_derives_from_the_mean(setup, tmp_path):
    from cartnet_amd.cif import load_crystals
    from cartnet_amd.predict import KEYS, ROT_KEYS, SYM_KEYS, predict_adps
    from cartnet_amd.shard import DeviceShard
    from cartnet_amd.symmetry import expand, site_average
    entry, model, _, _, _ = setup
    keys = ("a", "b", "c", "d")
    for k in keys:
        (tmp_path / f"{k}.cif").write_text(cu.cif_text(k, name=f"crystal_{k}", labeled=False))
    crystals, rejected = load_crystals(str(tmp_path), False, None)
    assert len(crystals) == 4 and not rejected
    arrays, sym = expand(crystals, "cuda:0", labeled=False)
    (shard,), norm = entry.shard_recipe([DeviceShard(arrays, "cuda:0", labeled=False, names=sym.names)])
    res = predict_adps(model, _loader(shard, norm), "cuda:0", sym=sym, rotations=K, seed=SEED)
    assert tuple(res) == KEYS + SYM_KEYS + ROT_KEYS
    counts = [int(t.shape[0]) for t in res["u_cart"]]
    assert counts == [cu.ATOMS[k][1] for k in keys]
    row_ptr = torch.tensor([0] + counts, dtype=torch.int64).cumsum(0).cuda()
    u, spread = site_average(torch.cat(res["u_cart"]).cuda(), row_ptr, list(range(4)), sym)
    assert torch.equal(torch.cat(res["u_cif_asym"]), u.cpu()) and torch.equal(torch.cat(res["spread"]), spread.cpu())
    assert all(bool(torch.isfinite(t).all()) for t in res["u_cif_asym"])
    assert all(bool((t >= 0).all()) for t in res["rot_spread"])
